// kernels_nmt.hip -- row and column namespaced-Merkle-tree roots of a
// device-resident EDS, as rsmt2d's erasured NMT wrappers build them
// (nmtwrapper_test.go:94-120; the pooled tree nmtbuffered_tree_test.go:118-152
// pushes identically) over celestiaorg/nmt v0.24.3 (go.mod:7, not vendored;
// published algorithm restated in merkle.cpp and oracle/nmt.py):
//   cell (r, c) is pushed as ns || share, ns = share[:NS] when r < k and c < k
//   (quadrant 0; the same for the cell's row tree and its column tree), else the
//   parity namespace 0xFF..;
//   leaf node  = ns || ns || H(0x00 || ns || share);
//   inner node = l.min || max || H(0x01 || l || r), max = l.max when r.min is the
//                parity namespace (IgnoreMaxNamespace), else r.max;
//   root       = RFC 6962 split: pairing level by level and carrying an unpaired
//                last node up unchanged gives the same tree.
// Push order (namespaces non-decreasing along a vector) and sibling order are
// checked; a failing tree reports status 1 (the reference's Push/Root error,
// which Repair turns into ErrByzantineData, extendeddatacrossword.go:316-320).
//
// Two kernels, as for the DefaultTree (kernels_sha.hip):
//   nmt_leaf_kernel : one thread per cell, streams ns || share through SHA-256;
//                     one leaf record (ns, digest) serves the cell's row and column
//                     (nmt_leaf29_kernel: the same for 29-byte namespaces, 16-byte loads);
//   nmt_tree_kernel : one workgroup per tree, levels ping-pong in LDS; each thread
//                     lays its node message out in its own LDS bytes and hashes it.
// Also nmt_nodes_kernel (every node kept: the proofs' node store) and
// nmt_proof_verify_kernel (one lane per sampled share: leaf, fold of its proof through
// hash_node, compare with the committed root; any width up to 65536),
// nmt_proof_verify_data_root_kernel (the same lane, hashing the fold's node as a leaf of
// the data-root tree and folding on to the square's data root: no root table) and
// nmt_ns_verify_kernel (one wave per namespace proof: the leaves of its range, the fold of
// its range proof in the wave's LDS, the completeness checks; any width up to 1024) and
// nmt_range_verify_kernel (the same wave for a range the caller names, an inclusion claim
// with no completeness checks; also chained to the data root).
// Namespace sizes up to 32 bytes (Celestia: 29), widths up to 1024 (LDS permitting).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <utility>

#include "dataroot_dev.hpp"
#include "nmt_dev.hpp"
#include "rsm_kernels.hpp"
#include "sha256_dev.hpp"

namespace rsm {

namespace {

template <int N, typename F>
__device__ __forceinline__ void sfor_n(F&& f) {
    [&]<int... I>(std::integer_sequence<int, I...>) {
        (f(std::integral_constant<int, I>{}), ...);
    }(std::make_integer_sequence<int, N>{});
}

// (Node, hash_node, the LDS node forms and the leaf node of a share, verify_leaf /
// verify_leaf29: nmt_dev.hpp, shared with the packed-vector trees of kernels_fraud.hip.)
constexpr uint32_t kMaxWidth = 1024;
constexpr size_t kLdsCap = 160 * 1024 - 256;  // per workgroup, less the static words

// Leaf records: leaf[cell][0..7] = namespace (big-endian words, zero padded),
// leaf[cell][8..15] = SHA256(0x00 || ns || share).
// Batched: blockIdx.y is the square (consecutive [W][W][S] buffers, leaf records
// consecutive per square).
__global__ __launch_bounds__(256) void nmt_leaf_kernel(const uint8_t* __restrict__ eds, uint32_t W, uint32_t S,
                                                       uint32_t ns, uint32_t k, uint32_t* __restrict__ leaf) {
    const uint32_t cell = blockIdx.x * 256u + threadIdx.x;
    if (cell >= W * W) return;
    eds += (uint64_t)blockIdx.y * W * W * S;
    leaf += (uint64_t)blockIdx.y * W * W * kLeafWords;
    const uint32_t r = cell / W, c = cell - r * W;
    const bool q0 = r < k && c < k;
    const uint32_t* dw = reinterpret_cast<const uint32_t*>(eds + (uint64_t)cell * S);
    const int nD = (int)(S / 4u);
    const int off = 1 + (int)ns;           // message bytes before the share
    const int L = off + (int)S;            // message length
    const int m0 = off >> 2;               // first word holding share bytes
    const uint32_t sh = 8u * (uint32_t)(off & 3);
    const int nb = (L + 8) / 64 + 1;       // SHA blocks
    // the namespace prefix words (message words 0..8 at most): 0x00 || ns
    uint32_t d0[kNsWords + 1];
#pragma unroll
    for (int i = 0; i <= (int)kNsWords; ++i) d0[i] = be_word(dw, i < nD ? i : 0);
    uint32_t h[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = kH0[i];
    uint32_t prev = 0;
    for (int b = 0; b < nb; ++b) {
        uint32_t w[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int m = 16 * b + i;
            const int p = 4 * m;  // byte position of the word
            uint32_t pre = 0;
            if (m <= (int)kNsWords) {  // only block 0 reaches here (m <= 8)
                const uint32_t lo = d0[i <= (int)kNsWords ? i : 0];
                const uint32_t hi = i >= 1 && i <= (int)kNsWords + 1 ? d0[i >= 1 ? i - 1 : 0] : 0u;
                pre = q0 ? __builtin_amdgcn_alignbit(m == 0 ? 0u : hi, lo, 8) : (m == 0 ? 0x00FFFFFFu : 0xFFFFFFFFu);
            }
            const int j = m - m0;  // share word index of this message word
            const uint32_t cur = be_word(dw, j < 0 ? 0 : (j < nD ? j : nD - 1));
            const uint32_t r2 = __builtin_amdgcn_alignbit(j <= 0 ? 0u : prev, cur, sh);
            prev = cur;
            const uint32_t mpre = head_mask(off - p);
            const uint32_t mr2 = head_mask(L - p) & ~mpre;
            uint32_t x = (pre & mpre) | (r2 & mr2);
            if (p <= L && L < p + 4) x |= 0x80u << (8 * (3 - (L - p)));
            if (b == nb - 1 && i == 15) x = 8u * (uint32_t)L;  // bit length (< 2^32), word 14 stays 0
            w[i] = x;
        }
        sha_block(h, w);
    }
    uint32_t* o = leaf + (uint64_t)cell * kLeafWords;
#pragma unroll
    for (int i = 0; i < (int)kNsWords; ++i) o[i] = (q0 ? d0[i] : 0xFFFFFFFFu) & head_mask((int)ns - 4 * i);
#pragma unroll
    for (int i = 0; i < 8; ++i) o[kNsWords + i] = h[i];
}

// The same leaf records for Celestia's 29-byte namespace and shares a multiple of 64
// bytes, streamed like kernels_sha.hip's leaf_hash_kernel: 16-byte loads of 64-byte
// share chunks, big-endian words.  The message 0x00 || ns || share puts share byte j
// at message byte 30 + j, so message word m >= 8 is the funnel shift of share words
// m - 8 and m - 7 by 16 bits; words 0..7 carry the prefix (for a Q0 cell ns is the
// share's first 29 bytes: share words shifted by 8 bits, as the DefaultTree leaf).
// Block b (of S/64 + 1) takes chunk b - 1's upper half and chunk b's first nine
// words; the last block's share word S/4 is the 0x80 pad (at message byte 30 + S, byte
// 2 of word S/4 + 7), word 15 the bit length.  The generic kernel above reads each
// word with its own 4-byte load and runtime masks.
__global__ __launch_bounds__(256) void nmt_leaf29_kernel(const uint8_t* __restrict__ eds, uint32_t W, uint32_t S,
                                                         uint32_t k, uint32_t* __restrict__ leaf) {
    const uint32_t cell = blockIdx.x * 256u + threadIdx.x;
    if (cell >= W * W) return;
    eds += (uint64_t)blockIdx.y * W * W * S;
    leaf += (uint64_t)blockIdx.y * W * W * kLeafWords;
    const uint32_t r = cell / W, c = cell - r * W;
    const bool q0 = r < k && c < k;
    const nv4u* p = reinterpret_cast<const nv4u*>(eds + (uint64_t)cell * S);
    const uint32_t chunks = S / 64u, L = 30u + S;
    uint32_t h[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = kH0[i];
    uint32_t hi[8];   // words 8..15 of the previous chunk
    uint32_t nsw[8];  // the namespace words (chunk 0's first eight)
    for (uint32_t b = 0; b <= chunks; ++b) {
        uint32_t cw[16];
        if (b < chunks) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const nv4u v = p[b * 4u + q];
                cw[4 * q + 0] = __builtin_bswap32(v.x);
                cw[4 * q + 1] = __builtin_bswap32(v.y);
                cw[4 * q + 2] = __builtin_bswap32(v.z);
                cw[4 * q + 3] = __builtin_bswap32(v.w);
            }
        } else {
            cw[0] = 0x80000000u;  // the pad byte after the share
#pragma unroll
            for (int i = 1; i < 16; ++i) cw[i] = 0u;
        }
        uint32_t w[16];
        if (b == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) nsw[i] = cw[i];
#pragma unroll
            for (int i = 0; i < 7; ++i)
                w[i] = q0 ? __builtin_amdgcn_alignbit(i == 0 ? 0u : cw[i - 1], cw[i], 8)
                          : (i == 0 ? 0x00FFFFFFu : 0xFFFFFFFFu);
            w[7] = (q0 ? (__builtin_amdgcn_alignbit(cw[6], cw[7], 8) & 0xFFFF0000u) : 0xFFFF0000u) | (cw[0] >> 16);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) w[i] = __builtin_amdgcn_alignbit(hi[i], i < 7 ? hi[i + 1] : cw[0], 16);
        }
        if (b < chunks) {
#pragma unroll
            for (int i = 8; i < 16; ++i) w[i] = __builtin_amdgcn_alignbit(cw[i - 8], cw[i - 7], 16);
#pragma unroll
            for (int i = 0; i < 8; ++i) hi[i] = cw[8 + i];
        } else {
#pragma unroll
            for (int i = 8; i < 15; ++i) w[i] = 0u;
            w[15] = 8u * L;
        }
        sha_block(h, w);
    }
    uint32_t* o = leaf + (uint64_t)cell * kLeafWords;
#pragma unroll
    for (int i = 0; i < (int)kNsWords; ++i) o[i] = (q0 ? nsw[i] : 0xFFFFFFFFu) & head_mask(29 - 4 * i);
#pragma unroll
    for (int i = 0; i < 8; ++i) o[kNsWords + i] = h[i];
}

// One workgroup per tree (blockIdx.x < W: row tree, else column tree; blockIdx.y the
// square of a batch).  Dynamic LDS: two levels of W/2 nodes (ping-pong) + 256
// per-thread message buffers (block_tree_levels, nmt_dev.hpp).
// LIST (checked Repair; rsm_kernels.hpp): the tree is entry blockIdx.x of the square's
// lists instead, and its root is not stored but compared with the committed one
// (`committed`: [squares][2][W][2 ns + 32] bytes): the entry's word of `verdict` receives
// kByzTree where the tree fails, else kByzRoot where the roots differ, else 0.
template <bool LIST>
__global__ __launch_bounds__(256) void nmt_tree_kernel(const uint32_t* __restrict__ leaf, uint32_t W, uint32_t ns,
                                                       uint32_t ignore_max, uint8_t* __restrict__ roots,
                                                       uint32_t* __restrict__ status, const uint32_t* __restrict__ list,
                                                       const uint32_t* __restrict__ list_cnt,
                                                       const uint8_t* __restrict__ committed,
                                                       uint32_t* __restrict__ verdict) {
    extern __shared__ uint32_t lds[];
    uint32_t l_axis = 0, l_index = 0;
    uint64_t l_slot = 0;
    if constexpr (LIST) {  // the whole workgroup, before any barrier
        if (!list_entry(list, list_cnt, W, blockIdx.y, blockIdx.x, &l_axis, &l_index, &l_slot)) return;
    }
    leaf += (uint64_t)blockIdx.y * W * W * kLeafWords;
    if constexpr (!LIST) {
        roots += (uint64_t)blockIdx.y * 2 * W * (2 * ns + 32);
        if (status) status += (uint64_t)blockIdx.y * 2 * W;
    }
    const uint32_t tree = LIST ? l_axis * W + l_index : blockIdx.x;
    const uint32_t axis = tree >= W ? 1u : 0u;
    const uint32_t idx = tree - axis * W;
    uint32_t bad;
    const uint32_t* const top = block_tree_levels(
        leaf, [&](uint32_t pos) -> uint64_t { return axis == 0 ? (uint64_t)idx * W + pos : (uint64_t)pos * W + idx; }, W, ns,
        ignore_max != 0, lds, &bad);
    if (LIST) {
        if (threadIdx.x == 0) {
            Node rt;
            lds_node(top, rt);
            const uint8_t* c = committed + ((uint64_t)blockIdx.y * 2 * W + tree) * (2 * ns + 32);
            verdict[l_slot] = bad ? kByzTree : (node_differs(rt, c, ns) ? kByzRoot : 0u);
        }
        return;
    }
    if (threadIdx.x == 0) {
        Node rt;
        lds_node(top, rt);
        uint8_t* o = roots + (uint64_t)tree * (2 * ns + 32);
#pragma unroll
        for (int i = 0; i < (int)kMaxNs; ++i)
            if (i < (int)ns) {
                o[i] = be_byte(rt.mn, i);
                o[ns + i] = be_byte(rt.mx, i);
            }
#pragma unroll
        for (int i = 0; i < 32; ++i) o[2 * ns + i] = be_byte(rt.d, i);
        if (status) status[tree] = bad;
    }
}

// ---------------------------------------------------------------------------
// Wave-per-tree form for a compile-time namespace size (Celestia: 29): TPW trees per
// wave, four waves per workgroup, each tree's levels in place in the wave's own LDS
// (node j of a level reads 2j and 2j + 1 >= j: a level's reads precede its writes),
// no workgroup barrier -- the DefaultTree kernel's structure (kernels_sha.hip), which
// beat the level-by-level workgroup form 3x there.  The node message
// 0x01 || l || r (l, r = min || max || digest) is assembled in registers from
// compile-time byte positions (the backend forms v_perm / v_alignbit from them)
// instead of byte stores to a per-thread LDS buffer.  Same tree, same checks, same
// output as nmt_tree_kernel.
template <int NS>
struct WNode {
    static constexpr int kW = (NS + 3) / 4;
    uint32_t mn[kW], mx[kW], d[8];
};
template <int NS, int B>
__device__ __forceinline__ uint32_t node_byte(const WNode<NS>& n) {  // byte B of min || max || digest
    if constexpr (B < NS) return (n.mn[B >> 2] >> (24 - 8 * (B & 3))) & 0xFFu;
    else if constexpr (B < 2 * NS) return (n.mx[(B - NS) >> 2] >> (24 - 8 * ((B - NS) & 3))) & 0xFFu;
    else return (n.d[(B - 2 * NS) >> 2] >> (24 - 8 * ((B - 2 * NS) & 3))) & 0xFFu;
}
template <int NS, int I>
__device__ __forceinline__ uint32_t msg_byte(const WNode<NS>& l, const WNode<NS>& r) {
    constexpr int NL = 2 * NS + 32, LEN = 1 + 2 * NL, NB = (LEN + 8) / 64 + 1;
    if constexpr (I == 0) return 0x01u;
    else if constexpr (I <= NL) return node_byte<NS, I - 1>(l);
    else if constexpr (I <= 2 * NL) return node_byte<NS, I - 1 - NL>(r);
    else if constexpr (I == LEN) return 0x80u;
    else if constexpr (I == 64 * NB - 2) return ((8u * LEN) >> 8) & 0xFFu;
    else if constexpr (I == 64 * NB - 1) return (8u * LEN) & 0xFFu;
    else return 0u;
}
template <int NS>
__device__ __forceinline__ bool hash_node_w(const WNode<NS>& l, const WNode<NS>& r, bool ignore_max, WNode<NS>& out) {
    constexpr int NL = 2 * NS + 32, LEN = 1 + 2 * NL, NB = (LEN + 8) / 64 + 1;
    uint32_t h[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = kH0[i];
    sfor_n<NB>([&](auto Bc) {
        constexpr int b = decltype(Bc)::value;
        uint32_t w[16];
        sfor_n<16>([&](auto Ic) {
            constexpr int t = 16 * b + decltype(Ic)::value;
            w[decltype(Ic)::value] = (msg_byte<NS, 4 * t>(l, r) << 24) | (msg_byte<NS, 4 * t + 1>(l, r) << 16) |
                                     (msg_byte<NS, 4 * t + 2>(l, r) << 8) | msg_byte<NS, 4 * t + 3>(l, r);
        });
        sha_block(h, w);
    });
    constexpr int kW = WNode<NS>::kW;
    bool rmin_is_max = true;
#pragma unroll
    for (int i = 0; i < kW; ++i) rmin_is_max &= r.mn[i] == head_mask(NS - 4 * i);
    bool less = false, decided = false;  // r.mn < l.mx ?
#pragma unroll
    for (int i = 0; i < kW; ++i)
        if (!decided && r.mn[i] != l.mx[i]) {
            less = r.mn[i] < l.mx[i];
            decided = true;
        }
#pragma unroll
    for (int i = 0; i < kW; ++i) {
        out.mn[i] = l.mn[i];
        out.mx[i] = (ignore_max && rmin_is_max) ? l.mx[i] : r.mx[i];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) out.d[i] = h[i];
    return !less;
}
template <int NS>
__host__ __device__ constexpr uint32_t wnode_words() { return 2 * WNode<NS>::kW + 8; }
template <int NS>
__host__ __device__ constexpr uint32_t wtree_lds_words(uint32_t W, bool f2 = false) {
    return (f2 ? W / 4 : (W + 1) / 2) * wnode_words<NS>();  // f2: levels 1 and 2 in one pass
}
// one wave's LDS: its trees, then a spare node that lanes past a level's last node
// store to (so every lane hashes: see the level loops)
template <int NS>
__host__ __device__ constexpr uint32_t wwave_lds_words(uint32_t W, uint32_t tpw, bool f2 = false) {
    return tpw * wtree_lds_words<NS>(W, f2) + wnode_words<NS>();
}
constexpr uint32_t kNmtTreesPerBlock = 4;  // waves per workgroup of the one-tree-per-wave form

// WPB waves per workgroup, TPW trees per wave.  F2 (W a multiple of 4): the first pass
// hashes leaves 4j .. 4j + 3 into level-1 nodes 2j, 2j + 1 and on into level-2 node j,
// so LDS holds W/4 nodes per tree instead of W/2 (more trees, or more waves, per CU).
// Once a wave's TPW trees have fewer than 64 nodes in a level, the workgroup's WPB TPW
// trees are built together (as kernels_sha.hip's COOP form): node U * next + j of the
// workgroup on lane (U * next + j) mod 64 of wave (U * next + j) / 64, a barrier
// between a level's reads and its in-place writes, waves past the level's last node
// idle.  At W = 256, TPW = 2, WPB = 4: 34 wave-passes of three compressions per
// workgroup of 8 trees instead of 48 (each wave's own top five levels were one pass
// each for 32 .. 2 nodes).
template <int NS, int TPW, int WPB, bool F2>
__global__ __launch_bounds__(64 * WPB) void nmt_tree_wave_kernel(const uint32_t* __restrict__ leaf, uint32_t W,
                                                                 uint32_t ignore_max, uint8_t* __restrict__ roots,
                                                                 uint32_t* __restrict__ status) {
    constexpr int kW = WNode<NS>::kW;
    constexpr uint32_t NW = wnode_words<NS>();
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t tw0 = blockIdx.x * WPB * TPW, count = 2 * W;  // the workgroup's first tree
    const uint32_t t0 = tw0 + wv * TPW;
    // waves without trees stay for the workgroup barriers of the upper levels
    const uint32_t nt = t0 >= count ? 0u : (count - t0 < (uint32_t)TPW ? count - t0 : (uint32_t)TPW);
    const uint32_t ntw = count - tw0 < (uint32_t)(WPB * TPW) ? count - tw0 : (uint32_t)(WPB * TPW);
    __shared__ uint32_t wg_bad;  // bit U: workgroup tree U failed
    if (threadIdx.x == 0) wg_bad = 0;
    __syncthreads();  // before any wave's atomicOr (a W whose levels need no other barrier)
    leaf += (uint64_t)blockIdx.y * W * W * kLeafWords;
    roots += (uint64_t)blockIdx.y * 2 * W * (2 * NS + 32);
    if (status) status += (uint64_t)blockIdx.y * 2 * W;
    extern __shared__ uint32_t lds_raw[];
    // workgroup tree U: wave U / TPW's tree U % TPW
    auto tlvl = [&](uint32_t U) {
        return lds_raw + (size_t)(U / TPW) * wwave_lds_words<NS>(W, TPW, F2) + (size_t)(U % TPW) * wtree_lds_words<NS>(W, F2);
    };
    uint32_t* const base = lds_raw + (size_t)wv * wwave_lds_words<NS>(W, TPW, F2);
    auto lvl = [&](uint32_t u) { return base + (size_t)u * wtree_lds_words<NS>(W, F2); };
    uint32_t* const spare = base + (size_t)TPW * wtree_lds_words<NS>(W, F2);
    const bool ig = ignore_max != 0;
    auto leaf_at = [&](uint32_t tree, uint32_t pos, WNode<NS>& n) {
        const uint32_t axis = tree >= W ? 1u : 0u, idx = tree - axis * W;
        const uint64_t cell = axis == 0 ? (uint64_t)idx * W + pos : (uint64_t)pos * W + idx;
        const uint32_t* sp = leaf + cell * kLeafWords;
#pragma unroll
        for (int i = 0; i < kW; ++i) n.mn[i] = n.mx[i] = sp[i];
#pragma unroll
        for (int i = 0; i < 8; ++i) n.d[i] = sp[kNsWords + i];
    };
    auto ld = [&](const uint32_t* p, WNode<NS>& n) {
#pragma unroll
        for (int i = 0; i < kW; ++i) n.mn[i] = p[i], n.mx[i] = p[kW + i];
#pragma unroll
        for (int i = 0; i < 8; ++i) n.d[i] = p[2 * kW + i];
    };
    auto st = [&](uint32_t* p, const WNode<NS>& n) {
#pragma unroll
        for (int i = 0; i < kW; ++i) p[i] = n.mn[i], p[kW + i] = n.mx[i];
#pragma unroll
        for (int i = 0; i < 8; ++i) p[2 * kW + i] = n.d[i];
    };
    auto ns_lt = [&](const uint32_t* a, const uint32_t* b) {  // a < b
        bool less = false, decided = false;
#pragma unroll
        for (int i = 0; i < kW; ++i)
            if (!decided && a[i] != b[i]) {
                less = a[i] < b[i];
                decided = true;
            }
        return less;
    };
    auto wave_sync = [] {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    uint32_t bad = 0;  // bit U: workgroup tree U failed (push order / sibling order)
    // level 1 from the leaf records (push order checked on every consecutive pair)
    // Every lane hashes in every pass of a level: past the level's last node a lane
    // repeats node v0 + lane % rem and stores it to the wave's spare node (a wave
    // with <= 8 lanes active runs its SHA rounds 2-3.5x slower per compression:
    // kernels_sha.hip; the store keeps the compiler from shrinking the hash to the
    // owning lanes).
    uint32_t cnt = W, next = (W + 1) / 2;
    if constexpr (F2) {
        next = W / 4;
        for (uint32_t v0 = 0; v0 < nt * next; v0 += 64u) {
            const uint32_t rem = nt * next - v0;
            const bool own = lane < rem;
            const uint32_t v = v0 + (own ? lane : lane % rem);
            const uint32_t u = v / next, j = v - u * next;
            WNode<NS> a, b, c, d, l, r, o;
            leaf_at(t0 + u, 4 * j, a);
            leaf_at(t0 + u, 4 * j + 1, b);
            leaf_at(t0 + u, 4 * j + 2, c);
            leaf_at(t0 + u, 4 * j + 3, d);
            bool ok = !ns_lt(b.mn, a.mn) && !ns_lt(c.mn, b.mn) && !ns_lt(d.mn, c.mn);
            if (4 * j + 4 < cnt) {  // push order across the next group's first leaf
                WNode<NS> e;
                leaf_at(t0 + u, 4 * j + 4, e);
                if (ns_lt(e.mn, d.mn)) ok = false;
            }
            if (!hash_node_w<NS>(a, b, ig, l)) ok = false;
            if (!hash_node_w<NS>(c, d, ig, r)) ok = false;
            if (!hash_node_w<NS>(l, r, ig, o)) ok = false;
            st(own ? lvl(u) + (size_t)j * NW : spare, o);
            if (own && !ok) bad |= 1u << (wv * TPW + u);
        }
    } else {
        for (uint32_t v0 = 0; v0 < nt * next; v0 += 64u) {
            const uint32_t rem = nt * next - v0;
            const bool own = lane < rem;
            const uint32_t v = v0 + (own ? lane : lane % rem);
            const uint32_t u = v / next, j = v - u * next;
            WNode<NS> a, b, o;
            leaf_at(t0 + u, 2 * j, a);
            bool ok = true;
            if (2 * j + 1 < cnt) {
                leaf_at(t0 + u, 2 * j + 1, b);
                if (ns_lt(b.mn, a.mn)) ok = false;
                if (2 * j + 2 < cnt) {
                    WNode<NS> c;
                    leaf_at(t0 + u, 2 * j + 2, c);
                    if (ns_lt(c.mn, b.mn)) ok = false;
                }
                if (!hash_node_w<NS>(a, b, ig, o)) ok = false;
            } else {
                o = a;
            }
            st(own ? lvl(u) + (size_t)j * NW : spare, o);
            if (own && !ok) bad |= 1u << (wv * TPW + u);
        }
    }
    wave_sync();
    for (cnt = next; cnt > 1; cnt = next) {
        next = (cnt + 1) / 2;
        if ((uint32_t)TPW * next < 64u) {
            // the workgroup's trees together: at most one pass per wave (WPB TPW next < 64 WPB)
            const uint32_t tot = ntw * next, v0 = wv * 64u;
            __syncthreads();  // the previous level's nodes (any wave's) are written
            uint32_t U = 0, j = 0;
            bool own = false;
            WNode<NS> o;
            if (v0 < tot) {
                const uint32_t rem = tot - v0;  // every lane of a working wave hashes
                own = lane < rem;
                const uint32_t v = v0 + (own ? lane : lane % rem);
                U = v / next;
                j = v - U * next;
                WNode<NS> a, b;
                ld(tlvl(U) + (size_t)(2 * j) * NW, a);
                if (2 * j + 1 < cnt) {
                    ld(tlvl(U) + (size_t)(2 * j + 1) * NW, b);
                    if (!hash_node_w<NS>(a, b, ig, o) && own) bad |= 1u << U;
                } else {
                    o = a;
                }
            }
            __syncthreads();  // every read of this level precedes its in-place writes
            if (v0 < tot) st(own ? tlvl(U) + (size_t)j * NW : spare, o);
            continue;
        }
        for (uint32_t v0 = 0; v0 < nt * next; v0 += 64u) {
            const uint32_t rem = nt * next - v0;
            const bool own = lane < rem;
            const uint32_t v = v0 + (own ? lane : lane % rem);
            const uint32_t u = v / next, j = v - u * next;
            WNode<NS> a, b, o;
            ld(lvl(u) + (size_t)(2 * j) * NW, a);
            if (2 * j + 1 < cnt) {
                ld(lvl(u) + (size_t)(2 * j + 1) * NW, b);
                if (!hash_node_w<NS>(a, b, ig, o) && own) bad |= 1u << (wv * TPW + u);
            } else {
                o = a;
            }
            wave_sync();  // every lane's reads of this level before any write (j < 2j)
            st(own ? lvl(u) + (size_t)j * NW : spare, o);
        }
        wave_sync();
    }
    // OR of every lane's failure bits, per workgroup tree
    uint32_t all = bad;
#pragma unroll
    for (int sft = 1; sft < 64; sft <<= 1) all |= __shfl_xor(all, sft);
    if (lane == 0 && all) atomicOr(&wg_bad, all);
    __syncthreads();  // the roots (written by any wave) and wg_bad
    all = wg_bad >> (wv * TPW);
    if (lane < nt) {
        const uint32_t tree = t0 + lane;
        WNode<NS> rt;
        ld(lvl(lane), rt);
        uint8_t* o = roots + (uint64_t)tree * (2 * NS + 32);
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            o[i] = be_byte(rt.mn, i);
            o[NS + i] = be_byte(rt.mx, i);
        }
#pragma unroll
        for (int i = 0; i < 32; ++i) o[2 * NS + i] = be_byte(rt.d, i);
        if (status) status[tree] = (all >> lane) & 1u;
    }
}

// Trees per wave and waves per workgroup.  A batch packs two trees per wave (the upper
// levels of one tree leave most lanes repeating work, so packing cuts the batch's
// wave-instructions) in four-wave workgroups when their LDS fits a third of the CU,
// else two-wave ones; one square (latency: Repair's checks) takes one tree per wave.
// W = 256, 32 squares (scripts/diag/nmtprobe.hip, profiles/r05aa_nmtprobe.txt): one tree
// per wave 1142 us; two per wave 1012; with levels 1-2 fused (F2) 786 at 2 x 4 or 2 x 2
// waves, 913 at four trees per wave.
template <int NS>
inline void nmt_tree_shape(uint32_t W, bool latency, bool f2, uint32_t* tpw, uint32_t* wpb) {
    *tpw = 1;
    *wpb = kNmtTreesPerBlock;
    if (latency) return;
    for (uint32_t b = 4; b >= 2; b >>= 1)
        if ((size_t)b * wwave_lds_words<NS>(W, 2, f2) * 4u <= 52u * 1024u) {
            *tpw = 2;
            *wpb = b;
            return;
        }
}
template <int NS>
hipError_t launch_nmt_tree_wave(const uint32_t* d_leaf, uint32_t W, uint32_t ignore_max, uint8_t* d_roots,
                                uint32_t* d_status, uint32_t squares, hipStream_t st) {
    const bool f2 = W % 4 == 0;
    uint32_t tpw, wpb;
    nmt_tree_shape<NS>(W, squares == 1, f2, &tpw, &wpb);
    const uint32_t blocks = (2 * W + wpb * tpw - 1) / (wpb * tpw);
    const size_t lds = (size_t)wpb * wwave_lds_words<NS>(W, tpw, f2) * 4u;
    const dim3 grid(blocks, squares);
#define RSM_NMT_WAVE(T, B, F)                                                                                     \
    hipLaunchKernelGGL((nmt_tree_wave_kernel<NS, T, B, F>), grid, dim3(64 * B), lds, st, d_leaf, W, ignore_max,    \
                       d_roots, d_status)
#define RSM_NMT_WAVE_F(T, B)      \
    if (f2) RSM_NMT_WAVE(T, B, true); \
    else RSM_NMT_WAVE(T, B, false)
    if (tpw == 2 && wpb == 4) { RSM_NMT_WAVE_F(2, 4); }
    else if (tpw == 2) { RSM_NMT_WAVE_F(2, 2); }
    else { RSM_NMT_WAVE_F(1, 4); }
#undef RSM_NMT_WAVE_F
#undef RSM_NMT_WAVE
    return hipGetLastError();
}

// Node-store build (share inclusion proofs, rsm_kernels.hpp "proof_*"): the trees above
// by levels, every node of levels 1 .. L written to the store by the lane that hashed
// it (six 16-byte stores: min[8] | max[8] | digest[8] words), an unpaired last node
// carried up as a copy.  One workgroup builds `tpb` <= 32 trees together (first tree
// blockIdx.x * tpb, square blockIdx.y): node j of tree u of a level is slot u * cnt + j,
// the level in place in the tree's LDS (ceil(W / 2) nodes; a barrier between a pass's
// reads and its writes).  NS = 29: the register-assembled node message of the wave
// kernel; NS = 0: any namespace size, the message in the lane's LDS bytes.  Checks,
// roots and statuses as nmt_tree_kernel.
template <int NS>
__global__ __launch_bounds__(256) void nmt_nodes_kernel(uint32_t* __restrict__ store, uint32_t W, uint32_t ns,
                                                        uint32_t ignore_max, uint32_t tpb, uint8_t* __restrict__ roots,
                                                        uint32_t* __restrict__ status) {
    extern __shared__ uint32_t lds[];
    __shared__ uint32_t wg_bad;  // bit u: workgroup tree u failed
    if (threadIdx.x == 0) wg_bad = 0;
    const uint32_t half = (W + 1) / 2, L = proof_levels(W), U = proof_tree_nodes(W);
    const uint32_t tw0 = blockIdx.x * tpb;
    const uint32_t ntw = 2 * W - tw0 < tpb ? 2 * W - tw0 : tpb;
    const uint32_t* leaf = store + (uint64_t)blockIdx.y * W * W * kLeafWords;
    uint32_t* upper = store + (uint64_t)gridDim.y * W * W * kLeafWords +
                      ((uint64_t)blockIdx.y * 2 * W + tw0) * U * kNodeWords;
    uint8_t* mb = reinterpret_cast<uint8_t*>(lds + (size_t)tpb * half * kNodeWords) +
                  (NS == 0 ? threadIdx.x * (64u * node_blocks(ns)) : 0u);
    const bool ig = ignore_max != 0;
    auto cell_of = [&](uint32_t tree, uint32_t pos) -> uint64_t {
        const uint32_t axis = tree >= W ? 1u : 0u, idx = tree - axis * W;
        return axis == 0 ? (uint64_t)idx * W + pos : (uint64_t)pos * W + idx;
    };
    auto hash = [&](const Node& a, const Node& b, Node& o) -> bool {
        if constexpr (NS == 0) {
            return hash_node(a, b, ns, ig, mb, o);
        } else {
            static_assert(WNode<NS>::kW == (int)kNsWords, "a WNode laid out as a Node");
            WNode<NS> x, y, z;
#pragma unroll
            for (int i = 0; i < (int)kNsWords; ++i) x.mn[i] = a.mn[i], x.mx[i] = a.mx[i], y.mn[i] = b.mn[i], y.mx[i] = b.mx[i];
#pragma unroll
            for (int i = 0; i < 8; ++i) x.d[i] = a.d[i], y.d[i] = b.d[i];
            const bool ok = hash_node_w<NS>(x, y, ig, z);
#pragma unroll
            for (int i = 0; i < (int)kNsWords; ++i) o.mn[i] = z.mn[i], o.mx[i] = z.mx[i];
#pragma unroll
            for (int i = 0; i < 8; ++i) o.d[i] = z.d[i];
            return ok;
        }
    };
    __syncthreads();  // wg_bad zeroed before any atomicOr
    uint32_t prev = W, off = 0;  // nodes of level l - 1; level l's first node in a tree's block
    for (uint32_t l = 1; l <= L; ++l) {
        const uint32_t cnt = (prev + 1) / 2, tot = ntw * cnt;
        for (uint32_t v0 = 0; v0 < tot; v0 += 256u) {
            const uint32_t v = v0 + threadIdx.x;
            const bool act = v < tot;
            const uint32_t u = act ? v / cnt : 0u, j = act ? v - u * cnt : 0u;
            Node o;
            if (act) {
                Node a, b;
                bool ok = true;
                const bool pair = 2 * j + 1 < prev;
                if (l == 1) {  // from the leaf records; push order on every consecutive pair
                    leaf_node(leaf, cell_of(tw0 + u, 2 * j), a);
                    if (pair) {
                        leaf_node(leaf, cell_of(tw0 + u, 2 * j + 1), b);
                        if (ns_less(b.mn, a.mn)) ok = false;
                        if (2 * j + 2 < prev) {
                            Node c;
                            leaf_node(leaf, cell_of(tw0 + u, 2 * j + 2), c);
                            if (ns_less(c.mn, b.mn)) ok = false;
                        }
                    }
                } else {
                    const uint32_t* lv = lds + (size_t)u * half * kNodeWords;
                    lds_node(lv + (size_t)(2 * j) * kNodeWords, a);
                    if (pair) lds_node(lv + (size_t)(2 * j + 1) * kNodeWords, b);
                }
                if (pair) {
                    if (!hash(a, b, o)) ok = false;
                } else {
                    o = a;  // carried up unchanged
                }
                if (!ok) atomicOr(&wg_bad, 1u << u);
            }
            __syncthreads();  // every read of this pass precedes its in-place writes
            if (act) {
                lds_store(lds + ((size_t)u * half + j) * kNodeWords, o);
                nv4u* g = reinterpret_cast<nv4u*>(upper + ((uint64_t)u * U + off + j) * kNodeWords);
                g[0] = nv4u{o.mn[0], o.mn[1], o.mn[2], o.mn[3]};
                g[1] = nv4u{o.mn[4], o.mn[5], o.mn[6], o.mn[7]};
                g[2] = nv4u{o.mx[0], o.mx[1], o.mx[2], o.mx[3]};
                g[3] = nv4u{o.mx[4], o.mx[5], o.mx[6], o.mx[7]};
                g[4] = nv4u{o.d[0], o.d[1], o.d[2], o.d[3]};
                g[5] = nv4u{o.d[4], o.d[5], o.d[6], o.d[7]};
                if (l == L && roots) {  // cnt == 1: the root, as nmt_tree_kernel lays it out
                    uint8_t* r = roots + ((uint64_t)blockIdx.y * 2 * W + tw0 + u) * (2 * ns + 32);
#pragma unroll
                    for (int i = 0; i < (int)kMaxNs; ++i)
                        if (i < (int)ns) {
                            r[i] = be_byte(o.mn, i);
                            r[ns + i] = be_byte(o.mx, i);
                        }
#pragma unroll
                    for (int i = 0; i < 32; ++i) r[2 * ns + i] = be_byte(o.d, i);
                }
            }
            __syncthreads();
        }
        off += cnt;
        prev = cnt;
    }
    // (the last pass's barrier orders every atomicOr before this read)
    if (status && threadIdx.x < ntw)
        status[(uint64_t)blockIdx.y * 2 * W + tw0 + threadIdx.x] = (wg_bad >> threadIdx.x) & 1u;
}

// ---------------------------------------------------------------------------
// Proof verification (rsm_kernels.hpp "Proof verification"), NMT: one lane per sample,
// as kernels_sha.hip's proof_verify_kernel.  The lane derives node count and operand
// sides from (W, pos) and compares the record's header with them (kProofMalformed),
// hashes its leaf as the leaf kernels above do (ns = the share's first bytes for a
// quadrant-0 sample, index < k and pos < k, else 0xFF..), folds the derived number of
// siblings through hash_node (kProofOrder where one returns false) and compares
// min || max || digest with its root (kProofRoot).  NS = 29: the streaming leaf of
// nmt_leaf29_kernel and hash_node_w<29>, nodes read as 22 words and a half-word; NS = 0:
// any namespace size, the word-load leaf and hash_node on the lane's LDS message bytes.
// Records and roots sit at any alignment (memcpy loads); nothing past a record's derived
// nodes is read, and no address depends on what a record or a share holds.
template <typename T>
__device__ __forceinline__ T ld_any(const uint8_t* p) {
    T v;
    __builtin_memcpy(&v, p, sizeof(T));
    return v;
}

// the node min || max || digest at p (2 ns + 32 bytes) as zero-padded big-endian words
template <int NS>
__device__ __forceinline__ void node_from_bytes(const uint8_t* p, uint32_t ns, Node& n) {
    if constexpr (NS == 29) {
        uint32_t B[23];  // the 90 bytes as big-endian words; B[22]: bytes 88, 89
#pragma unroll
        for (int i = 0; i < 22; ++i) B[i] = __builtin_bswap32(ld_any<uint32_t>(p + 4 * i));
        B[22] = __builtin_bswap32((uint32_t)ld_any<uint16_t>(p + 88));
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            n.mn[i] = B[i] & head_mask(29 - 4 * i);
            n.mx[i] = __builtin_amdgcn_alignbit(B[7 + i], B[8 + i], 24) & head_mask(29 - 4 * i);  // from byte 29
            n.d[i] = __builtin_amdgcn_alignbit(B[14 + i], B[15 + i], 16);                         // from byte 58
        }
    } else {
#pragma unroll
        for (int i = 0; i < (int)kNsWords; ++i) n.mn[i] = n.mx[i] = n.d[i] = 0u;
#pragma unroll
        for (int i = 0; i < (int)kMaxNs; ++i)
            if (i < (int)ns) {
                n.mn[i >> 2] |= (uint32_t)p[i] << (24 - 8 * (i & 3));
                n.mx[i >> 2] |= (uint32_t)p[ns + i] << (24 - 8 * (i & 3));
            }
#pragma unroll
        for (int i = 0; i < 32; ++i) n.d[i >> 2] |= (uint32_t)p[2 * ns + i] << (24 - 8 * (i & 3));
    }
}

// The share's leaf node folded through the n_nodes derived siblings at `nodes` (NL bytes
// each; bit i of mask: sibling i is the right operand) into acc; false where a fold step
// has unordered siblings.  mb: the lane's LDS message bytes (NS == 0).
template <int NS>
__device__ __forceinline__ bool nmt_share_fold(const uint8_t* share, uint32_t S, const uint8_t* nodes, uint32_t n_nodes,
                                               uint32_t mask, uint32_t ns, bool q0, bool ig, uint8_t* mb, Node& acc) {
    const uint32_t NL = 2u * ns + 32u;
    if constexpr (NS == 29) verify_leaf29(share, S, q0, acc);
    else verify_leaf(share, S, ns, q0, acc);
    bool ordered = true;
    for (uint32_t i = 0; i < n_nodes; ++i) {
        Node nd, l, r, o;
        node_from_bytes<NS>(nodes + i * NL, ns, nd);
        const bool right = (mask >> i) & 1u;  // the sibling is the right operand
#pragma unroll
        for (int q = 0; q < (int)kNsWords; ++q) {
            l.mn[q] = right ? acc.mn[q] : nd.mn[q], r.mn[q] = right ? nd.mn[q] : acc.mn[q];
            l.mx[q] = right ? acc.mx[q] : nd.mx[q], r.mx[q] = right ? nd.mx[q] : acc.mx[q];
            l.d[q] = right ? acc.d[q] : nd.d[q], r.d[q] = right ? nd.d[q] : acc.d[q];
        }
        if constexpr (NS == 0) {
            if (!hash_node(l, r, ns, ig, mb, o)) ordered = false;
        } else {
            static_assert(NS == 0 || WNode<NS>::kW == (int)kNsWords, "a WNode laid out as a Node");
            WNode<NS> x, y, z;
#pragma unroll
            for (int q = 0; q < (int)kNsWords; ++q) x.mn[q] = l.mn[q], x.mx[q] = l.mx[q], y.mn[q] = r.mn[q], y.mx[q] = r.mx[q];
#pragma unroll
            for (int q = 0; q < 8; ++q) x.d[q] = l.d[q], y.d[q] = r.d[q];
            if (!hash_node_w<NS>(x, y, ig, z)) ordered = false;
#pragma unroll
            for (int q = 0; q < (int)kNsWords; ++q) o.mn[q] = z.mn[q], o.mx[q] = z.mx[q];
#pragma unroll
            for (int q = 0; q < 8; ++q) o.d[q] = z.d[q];
        }
        acc = o;
    }
    return ordered;
}

// Leaf records of the listed vectors' cells that have none yet (checked Repair;
// rsm_kernels.hpp): one lane per (entry, position) of square blockIdx.y.  The lane that
// sets the cell's bit in `recorded` computes its record, as nmt_leaf29_kernel (NS = 29)
// or nmt_leaf_kernel would; hashed[s] += the records computed (one add per wave).
template <int NS>
__global__ __launch_bounds__(256) void nmt_list_leaf_kernel(const uint8_t* __restrict__ eds, uint32_t W, uint32_t S,
                                                            uint32_t ns, uint32_t k, const uint32_t* __restrict__ list,
                                                            const uint32_t* __restrict__ cnt, uint32_t* recorded,
                                                            uint32_t* hashed, uint32_t* __restrict__ leaf) {
    const uint32_t s = blockIdx.y, i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t e = i / W, pos = i - e * W;
    uint32_t axis, index;
    uint64_t slot;
    if (!list_entry(list, cnt, W, s, e, &axis, &index, &slot)) return;
    const uint32_t r = axis == 0 ? index : pos, c = axis == 0 ? pos : index;
    const uint32_t cell = r * W + c;
    const uint32_t bit = 1u << (cell & 31u);
    const bool fresh = !(atomicOr(&recorded[(uint64_t)s * ((W * W + 31u) / 32u) + (cell >> 5)], bit) & bit);
    if (fresh) {
        Node n;
        const uint8_t* share = eds + ((uint64_t)s * W * W + cell) * S;
        if constexpr (NS == 29) verify_leaf29(share, S, r < k && c < k, n);
        else verify_leaf(share, S, ns, r < k && c < k, n);
        uint32_t* o = leaf + ((uint64_t)s * W * W + cell) * kLeafWords;
#pragma unroll
        for (int q = 0; q < (int)kNsWords; ++q) o[q] = n.mn[q];
#pragma unroll
        for (int q = 0; q < 8; ++q) o[kNsWords + q] = n.d[q];
    }
    const uint64_t b = __ballot(fresh);
    if (b && (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(b)) atomicAdd(&hashed[s], (uint32_t)__popcll(b));
}

template <int NS>
__global__ __launch_bounds__(256) void nmt_proof_verify_kernel(const uint8_t* __restrict__ shares,
                                                               const uint8_t* __restrict__ records,
                                                               const uint8_t* __restrict__ roots, uint32_t W, uint32_t S,
                                                               uint32_t ns, uint32_t k, uint32_t ignore_max,
                                                               const ProofSample* __restrict__ samples, uint32_t n,
                                                               uint32_t* __restrict__ status) {
    extern __shared__ uint32_t lds[];  // NS == 0: the lanes' node messages
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n) return;
    const ProofSample sm = samples[t];
    const uint32_t L = proof_levels(W), NL = 2u * ns + 32u;
    const uint8_t* rec = records + (uint64_t)t * (8u + L * NL);
    uint32_t mask = 0;
    const uint32_t n_nodes = proof_shape(W, sm.pos, &mask);
    if (ld_any<uint32_t>(rec) != n_nodes || ld_any<uint32_t>(rec + 4) != mask) {
        status[t] = kProofMalformed;
        return;
    }
    const bool q0 = sm.index < k && sm.pos < k, ig = ignore_max != 0;
    uint8_t* mb = reinterpret_cast<uint8_t*>(lds) + (NS == 0 ? threadIdx.x * (64u * node_blocks(ns)) : 0u);
    Node acc;
    const bool ordered = nmt_share_fold<NS>(shares + (uint64_t)t * S, S, rec + 8u, n_nodes, mask, ns, q0, ig, mb, acc);
    Node rt;
    node_from_bytes<NS>(roots + (((uint64_t)sm.square * 2u + sm.axis) * W + sm.index) * NL, ns, rt);
    uint32_t diff = 0;
#pragma unroll
    for (int q = 0; q < (int)kNsWords; ++q) diff |= (acc.mn[q] ^ rt.mn[q]) | (acc.mx[q] ^ rt.mx[q]) | (acc.d[q] ^ rt.d[q]);
    status[t] = !ordered ? kProofOrder : (diff ? kProofRoot : kProofOk);
}

// The node's 2 ns + 32 bytes min || max || digest as zero-padded big-endian words: what the
// data-root tree hashes as a leaf.  NS = 29: from compile-time positions; NS = 0: through
// the lane's LDS message bytes mb (at least 128 for every namespace size), as hash_node
// lays out a node.
template <int NS>
__device__ __forceinline__ void node_root_words(const Node& acc, uint32_t ns, uint8_t* mb, uint32_t (&B)[kRootWords]) {
    if constexpr (NS == 0) {
        uint32_t* mw = reinterpret_cast<uint32_t*>(mb);
#pragma unroll
        for (int i = 0; i < kRootWords; ++i) mw[i] = 0;
#pragma unroll
        for (int i = 0; i < (int)kMaxNs; ++i)
            if (i < (int)ns) {
                mb[i] = be_byte(acc.mn, i);
                mb[(int)ns + i] = be_byte(acc.mx, i);
            }
#pragma unroll
        for (int i = 0; i < 32; ++i) mb[2 * (int)ns + i] = be_byte(acc.d, i);
#pragma unroll
        for (int i = 0; i < kRootWords; ++i) B[i] = __builtin_bswap32(mw[i]);
    } else {
        WNode<NS> x;
#pragma unroll
        for (int q = 0; q < (int)kNsWords; ++q) x.mn[q] = acc.mn[q], x.mx[q] = acc.mx[q];
#pragma unroll
        for (int q = 0; q < 8; ++q) x.d[q] = acc.d[q];
        constexpr int NLc = 2 * NS + 32;
        sfor_n<kRootWords>([&](auto Ic) {
            constexpr int i = decltype(Ic)::value;
            uint32_t v = 0;
            if constexpr (4 * i < NLc) v |= node_byte<NS, 4 * i>(x) << 24;
            if constexpr (4 * i + 1 < NLc) v |= node_byte<NS, 4 * i + 1>(x) << 16;
            if constexpr (4 * i + 2 < NLc) v |= node_byte<NS, 4 * i + 2>(x) << 8;
            if constexpr (4 * i + 3 < NLc) v |= node_byte<NS, 4 * i + 3>(x);
            B[i] = v;
        });
    }
}

// Chained verification (rsm_kernels.hpp "data root"), NMT: the same lane, with no root
// table.  Both headers -- the share record's against (W, pos), the root record's against
// (2W, axis W + index) -- are compared before anything is hashed.  The share fold's node
// min || max || digest is the candidate root: its 2 ns + 32 bytes are hashed as leaf
// axis W + index of the data-root tree (dataroot_dev.hpp), folded through the root
// record's 32-byte digests and compared with the square's data root.  NS = 29: the
// candidate's bytes come from compile-time positions; NS = 0: from the lane's LDS message
// bytes (at least 128 for every namespace size), as hash_node lays out a node.
template <int NS>
__global__ __launch_bounds__(256) void nmt_proof_verify_data_root_kernel(
    const uint8_t* __restrict__ shares, const uint8_t* __restrict__ records, const uint8_t* __restrict__ root_records,
    const uint8_t* __restrict__ data_roots, uint32_t W, uint32_t S, uint32_t ns, uint32_t k, uint32_t ignore_max,
    const ProofSample* __restrict__ samples, uint32_t n, uint32_t* __restrict__ status) {
    extern __shared__ uint32_t lds[];  // NS == 0: the lanes' node messages
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n) return;
    const ProofSample sm = samples[t];
    const uint32_t NL = 2u * ns + 32u;
    const uint8_t* rec = records + (uint64_t)t * (8u + proof_levels(W) * NL);
    const uint8_t* rrec = root_records + (uint64_t)t * (8u + proof_levels(2u * W) * 32u);
    uint32_t mask = 0, mask2 = 0;
    const uint32_t n_nodes = proof_shape(W, sm.pos, &mask);
    const uint32_t n2 = proof_shape(2u * W, sm.axis * W + sm.index, &mask2);
    if (ld_any<uint32_t>(rec) != n_nodes || ld_any<uint32_t>(rec + 4) != mask || ld_any<uint32_t>(rrec) != n2 ||
        ld_any<uint32_t>(rrec + 4) != mask2) {
        status[t] = kProofMalformed;
        return;
    }
    const bool q0 = sm.index < k && sm.pos < k, ig = ignore_max != 0;
    uint8_t* mb = reinterpret_cast<uint8_t*>(lds) + (NS == 0 ? threadIdx.x * (64u * node_blocks(ns)) : 0u);
    Node acc;
    if (!nmt_share_fold<NS>(shares + (uint64_t)t * S, S, rec + 8u, n_nodes, mask, ns, q0, ig, mb, acc)) {
        status[t] = kProofOrder;
        return;
    }
    uint32_t B[kRootWords], g[8];  // the candidate root's bytes as big-endian words
    node_root_words<NS>(acc, ns, mb, B);
    root_leaf_hash(B, NL, g);
    status[t] = data_root_matches(g, rrec, n2, mask2, data_roots + (uint64_t)sm.square * 32u) ? kProofOk : kProofRoot;
}

// ---------------------------------------------------------------------------
// Namespace proof verification (rsm_kernels.hpp "Namespace proof verification"): one WAVE
// per query -- a query hashes end - start leaves and folds a tree over them, so one lane
// per query (as above) would leave a wave waiting for its longest range.  The wave's LDS
// holds one tree level in place, node p of a level at entry p (W entries of kNodeWords
// words and a spare one), then, NS = 0, the 64 lanes' message bytes.  No workgroup barrier
// anywhere: the waves of a workgroup share nothing and finish at different times; a wave
// orders its own LDS traffic as nmt_tree_wave_kernel does (wave_sync between a pass's
// reads and its in-place writes and after every level).
//   header : every lane reads the two offsets, the 16-byte header, the query and the root;
//            wave-uniform exits follow rsm_nmt_namespace_verify's precedence (merkle.cpp)
//   leaves : lane j hashes shares start + j, + 64, .. into entries start + j ..; ABSENCE:
//            entry start is the record's leaf node
//   nodes  : lane i < the derived count checks proof node i against nid (INCOMPLETE)
//   fold   : level l grafts the left proof node at entry a - 1 when a is odd and the
//            right one at last + 1 when last is even and below the level's last node; lane
//            j joins entries a + 2j and a + 2j + 1 into entry a / 2 + j (both reads at or
//            past the write: a level's reads precede its writes), an unpaired last entry is
//            carried up; a >>= 1, last >>= 1.  Left nodes are taken from n_left - 1
//            downward, right ones from n_left upward.
// Counts, sides and every address come from (W, start, end) and the offsets, after the
// header passed the MALFORMED checks; nothing of a record past its derived nodes (and, for
// ABSENCE, the leaf slot) is read.

// The leaves of a range (the namespace and the range verifier): lane j hashes shares j,
// j + 64, .. of the n_shares at share o0 into entries start + j, ..; the leaf's namespace
// is the wrapper's (quadrant 0: the share's own).  Returns whether one of the lane's own
// leaves carries a namespace other than nid (nid == nullptr: nothing is compared).
// Every lane hashes in every pass, here and in the fold: past the pass's last leaf (node)
// a lane repeats leaf i0 + lane % rem and stores it to the spare entry (a wave with few
// lanes active runs its SHA rounds 2-3.5x slower per compression: kernels_sha.hip; the
// store keeps the compiler from shrinking the hash to the owning lanes).
template <int NS>
__device__ __forceinline__ bool range_leaves(const uint8_t* __restrict__ shares, uint32_t o0, uint32_t n_shares, uint32_t S,
                                             uint32_t ns, uint32_t k, uint32_t index, uint32_t start, const uint32_t* nid,
                                             uint32_t lane, uint32_t* __restrict__ row, uint32_t* __restrict__ spare) {
    bool flag = false;
    for (uint32_t i0 = 0; i0 < n_shares; i0 += 64u) {
        const uint32_t rem = n_shares - i0;
        const bool own = lane < rem;
        const uint32_t i = i0 + (own ? lane : lane % rem);
        const uint8_t* sp = shares + ((uint64_t)o0 + i) * S;
        const bool q0 = index < k && start + i < k;
        Node lf;
        if constexpr (NS == 29) verify_leaf29(sp, S, q0, lf);
        else verify_leaf(sp, S, ns, q0, lf);
        if (nid) {
            bool differs = false;
#pragma unroll
            for (int w = 0; w < (int)kNsWords; ++w) differs |= lf.mn[w] != nid[w];
            flag |= own && differs;
        }
        lds_store(own ? row + (size_t)(start + i) * kNodeWords : spare, lf);
    }
    return flag;
}

// The fold of a range whose level-0 entries start .. end - 1 are written (the "fold" step
// above), the proof nodes taken from rec + 16; the root is entry 0 when it returns.
// Returns whether one of the lane's own joins had unordered siblings.
template <int NS>
__device__ __forceinline__ bool range_fold(const uint8_t* __restrict__ rec, uint32_t W, uint32_t start, uint32_t end,
                                           uint32_t n_left, uint32_t ns, bool ig, uint32_t lane, uint32_t* __restrict__ row,
                                           uint8_t* __restrict__ mb) {
    uint32_t* const spare = row + (size_t)W * kNodeWords;
    const uint32_t L = proof_levels(W), NL = 2u * ns + 32u;
    bool flag = false;
    auto wave_sync = [] {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    auto hash = [&](const Node& a, const Node& b, Node& o) -> bool {
        if constexpr (NS == 0) {
            return hash_node(a, b, ns, ig, mb, o);
        } else {
            static_assert(NS == 0 || WNode<NS>::kW == (int)kNsWords, "a WNode laid out as a Node");
            WNode<NS> x, y, z;
#pragma unroll
            for (int i = 0; i < (int)kNsWords; ++i) x.mn[i] = a.mn[i], x.mx[i] = a.mx[i], y.mn[i] = b.mn[i], y.mx[i] = b.mx[i];
#pragma unroll
            for (int i = 0; i < 8; ++i) x.d[i] = a.d[i], y.d[i] = b.d[i];
            const bool ok = hash_node_w<NS>(x, y, ig, z);
#pragma unroll
            for (int i = 0; i < (int)kNsWords; ++i) o.mn[i] = z.mn[i], o.mx[i] = z.mx[i];
#pragma unroll
            for (int i = 0; i < 8; ++i) o.d[i] = z.d[i];
            return ok;
        }
    };
    uint32_t a = start, last = end - 1u, li = n_left, ri = n_left;  // next left node: li - 1; next right: ri
    for (uint32_t l = 0; l < L; ++l) {
        if (a & 1u) {
            --li;
            --a;
            if (lane == 0) {
                Node nd;
                node_from_bytes<NS>(rec + 16u + li * NL, ns, nd);
                lds_store(row + (size_t)a * kNodeWords, nd);
            }
        }
        if (!(last & 1u) && last + 1u < proof_level_count(W, l)) {
            ++last;
            if (lane == 0) {
                Node nd;
                node_from_bytes<NS>(rec + 16u + ri * NL, ns, nd);
                lds_store(row + (size_t)last * kNodeWords, nd);
            }
            ++ri;
        }
        wave_sync();  // the leaves / the level below and the grafts are written
        const uint32_t have = last - a + 1u, np = have / 2u, up = np + (have & 1u);  // a is even
        for (uint32_t v0 = 0; v0 < up; v0 += 64u) {
            const uint32_t rem = up - v0;
            const bool own = lane < rem;
            const uint32_t j = v0 + (own ? lane : lane % rem);
            Node x, o;
            lds_node(row + (size_t)(a + 2u * j) * kNodeWords, x);
            if (j < np) {
                Node y;
                lds_node(row + (size_t)(a + 2u * j + 1u) * kNodeWords, y);
                if (!hash(x, y, o) && own) flag = true;
            } else {
                o = x;  // carried up unchanged
            }
            wave_sync();  // every lane's reads of this pass before any write (a / 2 + j <= a + 2 j)
            lds_store(own ? row + (size_t)(a / 2u + j) * kNodeWords : spare, o);
        }
        a >>= 1;
        last >>= 1;
    }
    wave_sync();
    return flag;
}

template <int NS>
__device__ __forceinline__ uint32_t ns_verify_query(const uint8_t* __restrict__ rec, const uint32_t* __restrict__ offsets,
                                                    const uint8_t* __restrict__ shares, uint64_t shares_total,
                                                    const uint8_t* __restrict__ roots, uint32_t W, uint32_t S, uint32_t ns,
                                                    uint32_t k, bool ig, const NsQuery& qu, uint32_t lane,
                                                    uint32_t* __restrict__ row, uint8_t* __restrict__ mb) {
    uint32_t* const spare = row + (size_t)W * kNodeWords;  // entry W: what lanes past a pass's last node store
    const uint32_t o0 = __builtin_amdgcn_readfirstlane(offsets[0]), o1 = __builtin_amdgcn_readfirstlane(offsets[1]);
    if (o0 > o1 || o1 > shares_total) return kProofMalformed;  // nothing of the record or the shares is read
    const uint32_t n_shares = o1 - o0, L = proof_levels(W), NL = 2u * ns + 32u;
    const uint32_t kind = __builtin_amdgcn_readfirstlane(ld_any<uint32_t>(rec)),
                   start = __builtin_amdgcn_readfirstlane(ld_any<uint32_t>(rec + 4)),
                   end = __builtin_amdgcn_readfirstlane(ld_any<uint32_t>(rec + 8)),
                   n_nodes = __builtin_amdgcn_readfirstlane(ld_any<uint32_t>(rec + 12));
    Node rt;
    node_from_bytes<NS>(roots + (((uint64_t)qu.square * 2u + qu.axis) * W + qu.index) * NL, ns, rt);
    // 1. the header against what (W, start, end) dictates
    if (kind == kNsEmpty) {
        if (start | end | n_nodes | n_shares) return kProofMalformed;
        return !ns_less(qu.nid, rt.mn) && !ns_less(rt.mx, qu.nid) ? kProofIncomplete : kProofOk;
    }
    if (kind == kNsInclusion) {
        if (!(start < end && end <= W) || n_shares != end - start) return kProofMalformed;
    } else if (kind == kNsAbsence) {
        if (start >= W || end != start + 1u || n_shares != 0u) return kProofMalformed;
    } else {
        return kProofMalformed;  // kNsTree among them
    }
    uint32_t n_left = 0;
    const uint32_t nn = ns_range_nodes(W, start, end, &n_left);
    if (n_nodes != nn) return kProofMalformed;
    // 2. the leaves carry nid / the absence leaf is one leaf above nid
    bool flag = false;
    if (kind == kNsInclusion) {
        flag = range_leaves<NS>(shares, o0, n_shares, S, ns, k, qu.index, start, qu.nid, lane, row, spare);
    } else {
        Node lf;
        node_from_bytes<NS>(rec + 16u + 2u * L * NL, ns, lf);
#pragma unroll
        for (int w = 0; w < (int)kNsWords; ++w) flag |= lf.mn[w] != lf.mx[w];
        flag |= !ns_less(qu.nid, lf.mn);
        if (lane == 0) lds_store(row + (size_t)start * kNodeWords, lf);
    }
    if (__ballot(flag)) return kProofNamespace;
    // 3. nothing of nid lies under a proof node (nn <= 2 L < 64)
    if (lane < nn) {
        Node nd;
        node_from_bytes<NS>(rec + 16u + lane * NL, ns, nd);
        flag = lane < n_left ? !ns_less(nd.mx, qu.nid) : !ns_less(qu.nid, nd.mn);
    }
    if (__ballot(flag)) return kProofIncomplete;
    // 4, 5. the fold
    if (__ballot(range_fold<NS>(rec, W, start, end, n_left, ns, ig, lane, row, mb))) return kProofOrder;
    Node acc;
    lds_node(row, acc);
    uint32_t diff = 0;
#pragma unroll
    for (int w = 0; w < (int)kNsWords; ++w) diff |= (acc.mn[w] ^ rt.mn[w]) | (acc.mx[w] ^ rt.mx[w]) | (acc.d[w] ^ rt.d[w]);
    return diff ? kProofRoot : kProofOk;
}

template <int NS>
__global__ __launch_bounds__(256) void nmt_ns_verify_kernel(const uint8_t* __restrict__ records,
                                                            const uint32_t* __restrict__ offsets,
                                                            const uint8_t* __restrict__ shares, uint64_t shares_total,
                                                            const uint8_t* __restrict__ roots, uint32_t W, uint32_t S,
                                                            uint32_t ns, uint32_t k, uint32_t ignore_max,
                                                            const NsQuery* __restrict__ queries, uint32_t n,
                                                            uint32_t record_bytes, uint32_t wave_words,
                                                            uint32_t* __restrict__ status) {
    extern __shared__ uint32_t lds[];  // per wave: W nodes and a spare one, then (NS == 0) the lanes' node messages
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * (blockDim.x >> 6) + wv;
    if (q >= n) return;
    uint32_t* const row = lds + (size_t)wv * wave_words;
    uint8_t* const mb = reinterpret_cast<uint8_t*>(row + (size_t)(W + 1u) * kNodeWords) + (NS == 0 ? lane * (64u * node_blocks(ns)) : 0u);
    const NsQuery qu = queries[q];
    const uint32_t st = ns_verify_query<NS>(records + (uint64_t)q * record_bytes, offsets + q, shares, shares_total, roots, W,
                                            S, ns, k, ignore_max != 0, qu, lane, row, mb);
    if (lane == 0) status[q] = st;
}

// Range proof verification (rsm_kernels.hpp "range proofs"): the namespace verifier's wave
// with the claim bound to the caller's question instead of a namespace.  [start, end) is the
// QUERY's (host-validated: start < end <= W); the record's header is only compared with it
// and with the node count it dictates, so leaves, grafts and joins are addressed from the
// query and the offsets alone.  The leaves take the wrapper's namespace position by
// position (a range may cross square_size and hold several namespaces); there is no
// NAMESPACE or INCOMPLETE step.  CHAINED: no root table -- root record rrec is checked
// against (2W, axis W + index) with the other headers, before anything is hashed; the
// fold's root is then hashed as that leaf of the data-root tree (every lane the same
// work), folded on and compared with the square's data root dr.
template <int NS, bool CHAINED>
__device__ __forceinline__ uint32_t range_verify_query(const uint8_t* __restrict__ rec, const uint32_t* __restrict__ offsets,
                                                       const uint8_t* __restrict__ shares, uint64_t shares_total,
                                                       const uint8_t* __restrict__ root, const uint8_t* __restrict__ rrec,
                                                       const uint8_t* __restrict__ dr, uint32_t W, uint32_t S, uint32_t ns,
                                                       uint32_t k, bool ig, const RangeQuery& qu, uint32_t lane,
                                                       uint32_t* __restrict__ row, uint8_t* __restrict__ mb) {
    uint32_t* const spare = row + (size_t)W * kNodeWords;
    const uint32_t o0 = __builtin_amdgcn_readfirstlane(offsets[0]), o1 = __builtin_amdgcn_readfirstlane(offsets[1]);
    if (o0 > o1 || o1 > shares_total) return kProofMalformed;  // nothing of the record or the shares is read
    const uint32_t start = __builtin_amdgcn_readfirstlane(qu.start), end = __builtin_amdgcn_readfirstlane(qu.end);
    const uint32_t NL = 2u * ns + 32u;
    if (o1 - o0 != end - start || ld_any<uint32_t>(rec) != kNsInclusion || ld_any<uint32_t>(rec + 4) != start ||
        ld_any<uint32_t>(rec + 8) != end)
        return kProofMalformed;
    uint32_t n_left = 0;
    if (ld_any<uint32_t>(rec + 12) != ns_range_nodes(W, start, end, &n_left)) return kProofMalformed;
    uint32_t n2 = 0, mask2 = 0;
    if constexpr (CHAINED) {
        n2 = proof_shape(2u * W, qu.axis * W + qu.index, &mask2);
        if (ld_any<uint32_t>(rrec) != n2 || ld_any<uint32_t>(rrec + 4) != mask2) return kProofMalformed;
    }
    range_leaves<NS>(shares, o0, end - start, S, ns, k, qu.index, start, nullptr, lane, row, spare);
    if (__ballot(range_fold<NS>(rec, W, start, end, n_left, ns, ig, lane, row, mb))) return kProofOrder;
    Node acc;
    lds_node(row, acc);
    if constexpr (CHAINED) {
        uint32_t B[kRootWords], g[8];  // the candidate root's bytes as big-endian words
        node_root_words<NS>(acc, ns, mb, B);
        root_leaf_hash(B, NL, g);
        return data_root_matches(g, rrec, n2, mask2, dr) ? kProofOk : kProofRoot;
    } else {
        Node rt;
        node_from_bytes<NS>(root, ns, rt);
        uint32_t diff = 0;
#pragma unroll
        for (int w = 0; w < (int)kNsWords; ++w) diff |= (acc.mn[w] ^ rt.mn[w]) | (acc.mx[w] ^ rt.mx[w]) | (acc.d[w] ^ rt.d[w]);
        return diff ? kProofRoot : kProofOk;
    }
}

template <int NS, bool CHAINED>
__global__ __launch_bounds__(256) void nmt_range_verify_kernel(
    const uint8_t* __restrict__ records, const uint32_t* __restrict__ offsets, const uint8_t* __restrict__ shares,
    uint64_t shares_total, const uint8_t* __restrict__ roots, const uint8_t* __restrict__ root_records,
    const uint8_t* __restrict__ data_roots, uint32_t W, uint32_t S, uint32_t ns, uint32_t k, uint32_t ignore_max,
    const RangeQuery* __restrict__ queries, uint32_t n, uint32_t record_bytes, uint32_t wave_words,
    uint32_t* __restrict__ status) {
    extern __shared__ uint32_t lds[];  // per wave, as nmt_ns_verify_kernel
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * (blockDim.x >> 6) + wv;
    if (q >= n) return;
    uint32_t* const row = lds + (size_t)wv * wave_words;
    uint8_t* const mb = reinterpret_cast<uint8_t*>(row + (size_t)(W + 1u) * kNodeWords) + (NS == 0 ? lane * (64u * node_blocks(ns)) : 0u);
    const RangeQuery qu = queries[q];
    const uint8_t* root = CHAINED ? nullptr : roots + (((uint64_t)qu.square * 2u + qu.axis) * W + qu.index) * (2u * ns + 32u);
    const uint8_t* rrec = CHAINED ? root_records + (uint64_t)q * (8u + proof_levels(2u * W) * 32u) : nullptr;
    const uint8_t* dr = CHAINED ? data_roots + (uint64_t)qu.square * 32u : nullptr;
    const uint32_t st = range_verify_query<NS, CHAINED>(records + (uint64_t)q * record_bytes, offsets + q, shares, shares_total,
                                                        root, rrec, dr, W, S, ns, k, ignore_max != 0, qu, lane, row, mb);
    if (lane == 0) status[q] = st;
}

}  // namespace

hipError_t launch_nmt_proof_verify(const uint8_t* d_shares, const uint8_t* d_records, const uint8_t* d_roots, uint32_t W,
                                   uint32_t S, uint32_t ns, uint32_t k, uint32_t ignore_max, const ProofSample* d_samples,
                                   uint32_t n, uint32_t* d_status, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const dim3 grid((n + 255) / 256);
    if (ns == 29 && S % 64 == 0 && S >= 64)
        hipLaunchKernelGGL(nmt_proof_verify_kernel<29>, grid, dim3(256), 0, st, d_shares, d_records, d_roots, W, S, ns, k,
                           ignore_max, d_samples, n, d_status);
    else
        hipLaunchKernelGGL(nmt_proof_verify_kernel<0>, grid, dim3(256), (size_t)256 * 64u * node_blocks(ns), st, d_shares,
                           d_records, d_roots, W, S, ns, k, ignore_max, d_samples, n, d_status);
    return hipGetLastError();
}

hipError_t launch_nmt_proof_verify_data_root(const uint8_t* d_shares, const uint8_t* d_records,
                                             const uint8_t* d_root_records, const uint8_t* d_data_roots, uint32_t W,
                                             uint32_t S, uint32_t ns, uint32_t k, uint32_t ignore_max,
                                             const ProofSample* d_samples, uint32_t n, uint32_t* d_status, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const dim3 grid((n + 255) / 256);
    if (ns == 29 && S % 64 == 0 && S >= 64)
        hipLaunchKernelGGL(nmt_proof_verify_data_root_kernel<29>, grid, dim3(256), 0, st, d_shares, d_records,
                           d_root_records, d_data_roots, W, S, ns, k, ignore_max, d_samples, n, d_status);
    else
        hipLaunchKernelGGL(nmt_proof_verify_data_root_kernel<0>, grid, dim3(256), (size_t)256 * 64u * node_blocks(ns), st,
                           d_shares, d_records, d_root_records, d_data_roots, W, S, ns, k, ignore_max, d_samples, n,
                           d_status);
    return hipGetLastError();
}

bool nmt_ns_verify_supported(uint32_t W, uint32_t ns) { return W >= 1 && W <= kMaxWidth && ns >= 1 && ns <= kMaxNs; }

// One wave per query, up to four waves per workgroup: the count that lets most waves share
// a CU's LDS (W = 256: 24 KiB a wave, six waves per CU as two workgroups of three;
// W = 1024, ns = 32: 112 KiB, one wave).  False where not even one wave fits.
static bool ns_verify_shape(uint32_t W, uint32_t S, uint32_t ns, bool* f29, uint32_t* wave_words, uint32_t* wpb) {
    *f29 = ns == 29 && S % 64 == 0 && S >= 64;
    *wave_words = (W + 1u) * kNodeWords + (*f29 ? 0u : 64u * 16u * node_blocks(ns));
    const size_t wave_bytes = (size_t)*wave_words * 4u;
    uint32_t best = 0;
    *wpb = 1;
    for (uint32_t b = 1; b <= 4; ++b) {
        if (b * wave_bytes > kLdsCap) break;
        const uint32_t waves = (uint32_t)(kLdsCap / (b * wave_bytes)) * b;  // per CU
        if (waves >= best) best = waves, *wpb = b;
    }
    return best != 0;
}

hipError_t launch_nmt_ns_verify(const uint8_t* d_records, const uint32_t* d_offsets, const uint8_t* d_shares,
                                uint64_t shares_total, const uint8_t* d_roots, uint32_t W, uint32_t S, uint32_t ns,
                                uint32_t k, uint32_t ignore_max, const NsQuery* d_queries, uint32_t n, uint32_t* d_status,
                                hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (!nmt_ns_verify_supported(W, ns)) return hipErrorInvalidValue;
    bool f29;
    uint32_t wave_words, wpb;
    if (!ns_verify_shape(W, S, ns, &f29, &wave_words, &wpb)) return hipErrorInvalidValue;
    const size_t wave_bytes = (size_t)wave_words * 4u;
    const uint32_t record_bytes = 16u + (2u * proof_levels(W) + 1u) * (2u * ns + 32u);
    const dim3 grid((n + wpb - 1) / wpb);
    if (f29)
        hipLaunchKernelGGL(nmt_ns_verify_kernel<29>, grid, dim3(64 * wpb), wpb * wave_bytes, st, d_records, d_offsets, d_shares,
                           shares_total, d_roots, W, S, ns, k, ignore_max, d_queries, n, record_bytes, wave_words, d_status);
    else
        hipLaunchKernelGGL(nmt_ns_verify_kernel<0>, grid, dim3(64 * wpb), wpb * wave_bytes, st, d_records, d_offsets, d_shares,
                           shares_total, d_roots, W, S, ns, k, ignore_max, d_queries, n, record_bytes, wave_words, d_status);
    return hipGetLastError();
}

hipError_t launch_nmt_range_verify(const uint8_t* d_records, const uint32_t* d_offsets, const uint8_t* d_shares,
                                   uint64_t shares_total, const uint8_t* d_roots, const uint8_t* d_root_records,
                                   const uint8_t* d_data_roots, uint32_t W, uint32_t S, uint32_t ns, uint32_t k,
                                   uint32_t ignore_max, const RangeQuery* d_queries, uint32_t n, uint32_t* d_status,
                                   hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (!nmt_ns_verify_supported(W, ns)) return hipErrorInvalidValue;
    bool f29;
    uint32_t wave_words, wpb;
    if (!ns_verify_shape(W, S, ns, &f29, &wave_words, &wpb)) return hipErrorInvalidValue;
    const size_t lds = (size_t)wpb * wave_words * 4u;
    const uint32_t record_bytes = 16u + (2u * proof_levels(W) + 1u) * (2u * ns + 32u);
    const dim3 grid((n + wpb - 1) / wpb), block(64 * wpb);
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, lds, st, d_records, d_offsets, d_shares, shares_total, d_roots, d_root_records,
                           d_data_roots, W, S, ns, k, ignore_max, d_queries, n, record_bytes, wave_words, d_status);
    };
    if (d_root_records) f29 ? go(nmt_range_verify_kernel<29, true>) : go(nmt_range_verify_kernel<0, true>);
    else f29 ? go(nmt_range_verify_kernel<29, false>) : go(nmt_range_verify_kernel<0, false>);
    return hipGetLastError();
}

hipError_t launch_nmt_nodes(const uint8_t* d_eds, uint32_t W, uint32_t S, uint32_t ns, uint32_t k, uint32_t ignore_max,
                            uint32_t squares, uint32_t* d_store, uint8_t* d_roots, uint32_t* d_status, hipStream_t st) {
    if (squares == 0) return hipSuccess;
    const uint32_t cells = W * W;
    // the leaf records are the store's level 0 (the leaf kernels as launch_nmt_roots picks them)
    if (ns == 29 && S % 64 == 0 && S >= 64 && (reinterpret_cast<uintptr_t>(d_eds) & 15u) == 0)
        hipLaunchKernelGGL(nmt_leaf29_kernel, dim3((cells + 255) / 256, squares), dim3(256), 0, st, d_eds, W, S, k, d_store);
    else
        hipLaunchKernelGGL(nmt_leaf_kernel, dim3((cells + 255) / 256, squares), dim3(256), 0, st, d_eds, W, S, ns, k, d_store);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t tpb = proof_trees_per_block(W);
    const dim3 grid((2 * W + tpb - 1) / tpb, squares);
    const size_t levels = (size_t)tpb * ((W + 1) / 2) * kNodeWords * 4u;
    if (ns == 29)
        hipLaunchKernelGGL(nmt_nodes_kernel<29>, grid, dim3(256), levels, st, d_store, W, ns, ignore_max, tpb, d_roots,
                           d_status);
    else
        hipLaunchKernelGGL(nmt_nodes_kernel<0>, grid, dim3(256), levels + (size_t)256 * 64u * node_blocks(ns), st, d_store,
                           W, ns, ignore_max, tpb, d_roots, d_status);
    return hipGetLastError();
}

bool nmt_dev_supported(uint32_t W, uint32_t ns) {
    return W >= 2 && W <= kMaxWidth && ns >= 1 && ns <= kMaxNs && tree_lds_bytes(W, ns) <= kLdsCap;
}

// d_leaf: squares * W*W*64 bytes of scratch; the squares are consecutive [W][W][S]
// buffers, their 2W roots (and statuses) consecutive per square.
hipError_t launch_nmt_roots(const uint8_t* d_eds, uint32_t W, uint32_t S, uint32_t ns, uint32_t k, uint32_t ignore_max,
                            uint32_t* d_leaf, uint8_t* d_roots, uint32_t* d_status, hipStream_t st, uint32_t squares) {
    if (squares == 0) return hipSuccess;
    const uint32_t cells = W * W;
    // Celestia's namespace: the streaming leaf kernel (16-byte loads at eds + cell*S, so
    // the base must be 16-byte aligned; a caller-supplied unaligned square takes the
    // word-load kernel)
    if (ns == 29 && S % 64 == 0 && S >= 64 && (reinterpret_cast<uintptr_t>(d_eds) & 15u) == 0)
        hipLaunchKernelGGL(nmt_leaf29_kernel, dim3((cells + 255) / 256, squares), dim3(256), 0, st, d_eds, W, S, k, d_leaf);
    else
        hipLaunchKernelGGL(nmt_leaf_kernel, dim3((cells + 255) / 256, squares), dim3(256), 0, st, d_eds, W, S, ns, k, d_leaf);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // Celestia's namespace size: the wave-per-tree kernel (its LDS permitting)
    if (ns == 29 && (size_t)kNmtTreesPerBlock * wwave_lds_words<29>(W, 1, W % 4 == 0) * 4u <= kLdsCap)
        return launch_nmt_tree_wave<29>(d_leaf, W, ignore_max, d_roots, d_status, squares, st);
    const size_t lds = tree_lds_bytes(W, ns);
    hipLaunchKernelGGL(nmt_tree_kernel<false>, dim3(2 * W, squares), dim3(256), lds, st, d_leaf, W, ns, ignore_max, d_roots,
                       d_status, nullptr, nullptr, nullptr, nullptr);
    return hipGetLastError();
}

// ---- list-driven forms (checked Repair; rsm_kernels.hpp) ------------------------------
hipError_t launch_nmt_list_leaves(const uint8_t* d_eds, uint32_t W, uint32_t S, uint32_t ns, uint32_t k, uint32_t count,
                                  uint32_t max_n, const uint32_t* d_list, const uint32_t* d_cnt, uint32_t* d_recorded,
                                  uint32_t* d_hashed, uint32_t* d_leaf, hipStream_t st) {
    if (count == 0 || max_n == 0) return hipSuccess;
    const dim3 grid((max_n * W + 255) / 256, count);
    if (ns == 29 && S % 64 == 0 && S >= 64 && (reinterpret_cast<uintptr_t>(d_eds) & 15u) == 0)
        hipLaunchKernelGGL(nmt_list_leaf_kernel<29>, grid, dim3(256), 0, st, d_eds, W, S, ns, k, d_list, d_cnt, d_recorded,
                           d_hashed, d_leaf);
    else
        hipLaunchKernelGGL(nmt_list_leaf_kernel<0>, grid, dim3(256), 0, st, d_eds, W, S, ns, k, d_list, d_cnt, d_recorded,
                           d_hashed, d_leaf);
    return hipGetLastError();
}

hipError_t launch_nmt_list_tree_check(const uint32_t* d_leaf, uint32_t W, uint32_t ns, uint32_t ignore_max,
                                      uint32_t count, uint32_t max_n, const uint32_t* d_list, const uint32_t* d_cnt,
                                      const uint8_t* d_committed, uint32_t* d_verdict, hipStream_t st) {
    if (count == 0 || max_n == 0) return hipSuccess;
    if (!nmt_dev_supported(W, ns)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nmt_tree_kernel<true>, dim3(max_n, count), dim3(256), tree_lds_bytes(W, ns), st, d_leaf, W, ns,
                       ignore_max, nullptr, nullptr, d_list, d_cnt, d_committed, d_verdict);
    return hipGetLastError();
}

}  // namespace rsm
