// kernels_sha.hip -- row and column Merkle roots of a device-resident EDS.
//
// computeRoots / getRowRoot / getColRoot (datasquare.go:218-327)
// with rsmt2d's DefaultTree (tree.go:32-59): celestiaorg/merkletree over SHA-256,
//   leaf = SHA256(0x00 || share),  node = SHA256(0x01 || left || right),
// and for a leaf count that is not a power of two the NebulousLabs stack order:
// perfect subtrees for the set bits of n (largest first), folded from the right
//   root = node(sub_hi, node(sub_mid, ... sub_lo)).
// Host restatement: merkle.cpp (rsm_default_tree_root); tests compare both with
// Python hashlib.
//
// Two kernels:
//   leaf_hash_kernel : one thread per cell, streams its share through SHA-256
//                      (S/64 + 1 blocks); the digest of a cell serves both its row
//                      tree and its column tree.
//   tree_root_kernel : a few trees per wave (2W trees), levels in place in LDS.
// Also tree_nodes_kernel (every node kept: the proofs' node store),
// proof_verify_kernel (one lane per sampled share: leaf hash, fold of its proof, compare
// with the committed root) and proof_verify_data_root_kernel (the same lane, folding on
// through the root's proof under the square's data root) and range_verify_kernel (one wave
// per range proof: the leaves of the range, the fold in the wave's LDS; any width up to 2048).
#include <hip/hip_runtime.h>
#include <cstdint>

#include "dataroot_dev.hpp"
#include "rsm_kernels.hpp"
#include "sha256_dev.hpp"

namespace rsm {

namespace {

// leaf[cell][8] = SHA256(0x00 || share(cell)), cell = row * W + col.
__global__ __launch_bounds__(256) void leaf_hash_kernel(const uint8_t* __restrict__ eds, uint32_t cells,
                                                        uint32_t S, uint32_t* __restrict__ leaf) {
    const uint32_t cell = blockIdx.x * 256u + threadIdx.x;
    if (cell >= cells) return;
    const v4u* p = reinterpret_cast<const v4u*>(eds + (uint64_t)cell * S);
    uint32_t h[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = kH0[i];
    uint32_t prev = 0;  // the 0x00 leaf prefix
    for (uint32_t blk = 0; blk < S / 64u; ++blk) {
        uint32_t w[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const v4u v = p[blk * 4u + q];  // plain load: the other half of the 128-B line is the next block
            const uint32_t b0 = __builtin_bswap32(v.x), b1 = __builtin_bswap32(v.y);
            const uint32_t b2 = __builtin_bswap32(v.z), b3 = __builtin_bswap32(v.w);
            w[4 * q + 0] = shift8(prev, b0);
            w[4 * q + 1] = shift8(b0, b1);
            w[4 * q + 2] = shift8(b1, b2);
            w[4 * q + 3] = shift8(b2, b3);
            prev = b3;
        }
        sha_block(h, w);
    }
    uint32_t w[16];
    w[0] = (prev << 24) | 0x00800000u;  // last share byte, then the 0x80 pad byte
#pragma unroll
    for (int i = 1; i < 15; ++i) w[i] = 0;
    w[15] = (S + 1u) * 8u;
    sha_block(h, w);
    v4u* o = reinterpret_cast<v4u*>(leaf + (uint64_t)cell * 8u);
    o[0] = v4u{h[0], h[1], h[2], h[3]};
    o[1] = v4u{h[4], h[5], h[6], h[7]};
}

constexpr uint32_t kMaxLevel1 = 1024;  // W <= 2048
constexpr uint32_t kTreesPerBlock = 4;  // one wave per tree

// LDS bytes of one tree: level-1 digests (W/2) in place, plus the carried
// subtrees of the odd levels (16 digests)
__host__ __device__ constexpr uint32_t tree_lds_words(uint32_t W) { return (W / 2) * 8u + 16u * 8u; }

// TPW trees per WAVE (four waves per 256-thread workgroup): trees
// (blockIdx.x * 4 + wave) * TPW + u (u < TPW) + first (< W: row tree, else column
// tree) of square blockIdx.y.  A wave's trees are built level by level together
// (node (u, j) of a level is lane-slot u * cnt + j), in place in the wave's own LDS
// (a level's reads all precede its writes: node j reads 2j and 2j + 1 >= j), with
// no workgroup barrier: the many waves of a CU interleave their dependent SHA
// rounds, and packing TPW trees keeps the upper levels' lanes busy (the
// level-by-level workgroup form left most lanes idle behind __syncthreads: 3x
// slower).  roots: [squares][2][W][32] bytes (big-endian digest bytes, as
// Tree.Root() returns them).
// COOP (batches): once a wave's TPW trees have fewer than 64 nodes in a level, the
// workgroup's 4 TPW trees are built together instead -- node U * cnt + j of the
// workgroup (tree U, whose LDS is U tree-slots from the workgroup's first) on lane
// (U * cnt + j) mod 64 of wave (U * cnt + j) / 64, a barrier between a level's reads
// and its writes, waves past the level's last node idle.  At W = 256 and TPW = 2 the
// workgroup then issues 34 wave-passes of two compressions for its 8 trees instead
// of 48 (each wave's own top five levels were one pass each for 32 .. 2 nodes), and
// a SIMD's SHA throughput is its issued wave-passes (kernels_sha.hip above).  The
// launcher uses COOP for every form (one square's depth is the same either way).
template <int TPW, bool COOP>
__global__ __launch_bounds__(256) void tree_root_kernel(const uint32_t* __restrict__ leaf, uint32_t W,
                                                        uint8_t* __restrict__ roots, uint32_t first, uint32_t count) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t tw0 = blockIdx.x * kTreesPerBlock * TPW;  // the workgroup's first tree
    const uint32_t t0 = tw0 + wv * TPW;
    if (!COOP && t0 >= count) return;  // whole wave (no workgroup barrier without COOP)
    const uint32_t nt = t0 >= count ? 0u : (count - t0 < (uint32_t)TPW ? count - t0 : (uint32_t)TPW);
    const uint32_t ntw = count - tw0 < kTreesPerBlock * TPW ? count - tw0 : kTreesPerBlock * TPW;
    leaf += (uint64_t)blockIdx.y * W * W * 8u;
    roots += (uint64_t)blockIdx.y * 2u * W * 32u;
    extern __shared__ uint32_t lds_raw[];
    // tree U of the workgroup (wave U / TPW, its tree U % TPW)
    auto tlvl = [&](uint32_t U) { return lds_raw + (size_t)U * tree_lds_words(W); };
    auto tsub = [&](uint32_t U) { return tlvl(U) + (W / 2) * 8u; };
    auto sub = [&](uint32_t u) { return tsub(wv * TPW + u); };
    const uint32_t n = W;
    auto leaf_at = [&](uint32_t tree, uint32_t pos, uint32_t (&d)[8]) {
        const uint32_t axis = tree >= W ? 1u : 0u, idx = tree - axis * W;
        const uint64_t cell = axis == 0 ? (uint64_t)idx * W + pos : (uint64_t)pos * W + idx;
        const v4u* s = reinterpret_cast<const v4u*>(leaf + cell * 8u);
        const v4u a = s[0], b = s[1];
        d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
    };
    // children 2j, 2j + 1 of node j of workgroup tree U at height hgt
    auto children = [&](uint32_t U, uint32_t j, uint32_t hgt, uint32_t (&L)[8], uint32_t (&R)[8]) {
        if (hgt == 1) {
            leaf_at(tw0 + first + U, 2 * j, L);
            leaf_at(tw0 + first + U, 2 * j + 1, R);
        } else {
            const uint32_t* lv = tlvl(U);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                L[i] = lv[(2 * j) * 8u + i];
                R[i] = lv[(2 * j + 1) * 8u + i];
            }
        }
    };
    // node j of workgroup tree U (own: this lane's node; else a repeat, to the spare
    // slot); the last node of an odd level is also the carried subtree of its height
    auto put = [&](uint32_t U, uint32_t j, uint32_t hgt, uint32_t cnt, bool own, const uint32_t (&o)[8]) {
        uint32_t* dst = own ? tlvl(U) + j * 8u : tsub(U) + 15u * 8u;
#pragma unroll
        for (int i = 0; i < 8; ++i) dst[i] = o[i];
        if (own && (cnt & 1u) && j == cnt - 1) {
#pragma unroll
            for (int i = 0; i < 8; ++i) tsub(U)[hgt * 8u + i] = o[i];
        }
    };
    auto wave_sync = [] {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    if ((n & 1u) && lane < nt) {  // height-0 subtree: the last leaf
        uint32_t d[8];
        leaf_at(t0 + first + lane, n - 1, d);
#pragma unroll
        for (int i = 0; i < 8; ++i) sub(lane)[i] = d[i];
    }
    for (uint32_t hgt = 1; (n >> hgt) > 0; ++hgt) {
        const uint32_t cnt = n >> hgt;
        if (COOP && (uint32_t)TPW * cnt < 64u) {
            // the workgroup's trees together: at most one pass per wave (4 TPW cnt < 256)
            const uint32_t tot = ntw * cnt, v0 = wv * 64u;
            __syncthreads();  // the previous level's nodes (any wave's) are written
            uint32_t U = 0, j = 0, o[8];
            bool own = false;
            if (v0 < tot) {
                const uint32_t rem = tot - v0;  // every lane of a working wave hashes, as below
                own = lane < rem;
                const uint32_t v = v0 + (own ? lane : lane % rem);
                U = v / cnt;
                j = v - U * cnt;
                uint32_t L[8], R[8];
                children(U, j, hgt, L, R);
                node_hash(L, R, o);
            }
            __syncthreads();  // every read of this level precedes its in-place writes
            if (v0 < tot) put(U, j, hgt, cnt, own, o);
            continue;
        }
        const uint32_t tot = nt * cnt;
        for (uint32_t v0 = 0; v0 < tot; v0 += 64u) {
            // Every lane hashes: past the level's last node a lane repeats node
            // v0 + lane % rem and stores it to the tree's spare slot (sub slot 15:
            // heights stay below 12), so the compiler cannot shrink the hash to the
            // owning lanes.  A wave with <= 8 of its lanes active runs its SHA
            // rounds 2-3.5x slower per compression than a full wave
            // (profiles/r05j_sha_lanes.txt), and a tree's upper levels have 1-8
            // nodes.
            const uint32_t rem = tot - v0;
            const bool own = lane < rem;
            const uint32_t v = v0 + (own ? lane : lane % rem);
            const uint32_t u = v / cnt, j = v - u * cnt;
            uint32_t L[8], R[8], o[8];
            children(wv * TPW + u, j, hgt, L, R);
            node_hash(L, R, o);
            put(wv * TPW + u, j, hgt, cnt, own, o);
        }
        wave_sync();
    }
    if constexpr (COOP) {
        __syncthreads();  // the top levels' nodes and carried subtrees, from any wave
        if (nt == 0) return;
    }
    {  // fold the carried subtrees (a W that is not a power of two); all lanes, as above
        const uint32_t ul = lane % nt;
        const uint32_t tree = t0 + first + ul;
        const uint32_t axis = tree >= W ? 1u : 0u, idx = tree - axis * W;
        const uint32_t* sb = sub(ul);
        uint32_t acc[8];
        const int lo = __builtin_ctz(n);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = sb[lo * 8 + i];
        for (int hgt = lo + 1; hgt < 16; ++hgt) {
            if (!((n >> hgt) & 1u)) continue;
            uint32_t L[8], o[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) L[i] = sb[hgt * 8 + i];
            node_hash(L, acc, o);
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = o[i];
        }
        // lane ul + nt i writes word i of its tree's root: one store instruction covers the
        // wave's nt consecutive roots (coalesced -- also when `roots` is host memory, as
        // Repair's checks pass it)
        const uint32_t wi = lane / nt;
        if (wi < 8u) {
            uint32_t x = acc[0];
#pragma unroll
            for (int i = 1; i < 8; ++i) x = wi == (uint32_t)i ? acc[i] : x;
            uint32_t* r = reinterpret_cast<uint32_t*>(roots + ((uint64_t)axis * W + idx) * 32u);
            r[wi] = __builtin_bswap32(x);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) sub(ul)[15u * 8u + i] = acc[i];  // keeps every lane hashing
        }
    }
}

// trees per wave: as many as keep four waves' LDS within a third of the CU (so
// three workgroups share it), at least one.  A latency launch (one square's 2W
// trees, too few waves to fill the chip) takes one tree per wave: a lone wave's
// compressions run back to back, so the launch time is the tree depth in
// compressions per lane -- at W = 256, 18 (two level-1 nodes per lane, then one
// per level) against 24 at two trees per wave.
inline uint32_t trees_per_wave(uint32_t W) {
    for (uint32_t t = 4; t > 1; t >>= 1)
        if ((size_t)kTreesPerBlock * t * tree_lds_words(W) * 4u <= 52u * 1024u) return t;
    return 1;
}
hipError_t launch_tree_kernel(const uint32_t* d_leaf, uint32_t W, uint8_t* d_roots, uint32_t first, uint32_t count,
                              uint32_t squares, bool latency, hipStream_t st) {
    const uint32_t tpw = latency ? 1u : trees_per_wave(W);
    const uint32_t blocks = (count + kTreesPerBlock * tpw - 1) / (kTreesPerBlock * tpw);
    const size_t lds = (size_t)kTreesPerBlock * tpw * tree_lds_words(W) * 4u;
    const dim3 grid(blocks, squares);
    // (the cooperative upper levels in every form: one square's depth is the same either
    // way -- W = 256: 53.6 against 54.6 us -- and a wide square's many trees, W = 1024:
    // 2048 waves on 1024 SIMDs, need fewer wave-passes; profiles/r05av_eds_roots.json)
    if (tpw == 4)
        hipLaunchKernelGGL((tree_root_kernel<4, true>), grid, dim3(256), lds, st, d_leaf, W, d_roots, first, count);
    else if (tpw == 2)
        hipLaunchKernelGGL((tree_root_kernel<2, true>), grid, dim3(256), lds, st, d_leaf, W, d_roots, first, count);
    else
        hipLaunchKernelGGL((tree_root_kernel<1, true>), grid, dim3(256), lds, st, d_leaf, W, d_roots, first, count);
    return hipGetLastError();
}

// Node-store build (share inclusion proofs, rsm_kernels.hpp "proof_*"): the same trees
// by levels -- node (l, j) over leaves [j 2^l, min((j + 1) 2^l, W)), an unpaired last
// node carried up unchanged -- with every node of levels 1 .. L written to the store as
// it is produced (the level picture and the stack of subtrees above give the same
// tree: a carried node is the right-hand subtree waiting for its fold).  One
// workgroup builds `tpb` trees (first tree blockIdx.x * tpb, square blockIdx.y)
// together: node j of tree u of a level is slot u * cnt + j of the workgroup, the
// level in place in the tree's LDS (ceil(W / 2) nodes; node j reads 2j and 2j + 1 >= j,
// a barrier between a pass's reads and its writes), and the lane that hashed a node
// also stores it: two 16-byte stores, consecutive lanes to consecutive nodes.
__global__ __launch_bounds__(256) void tree_nodes_kernel(uint32_t* __restrict__ store, uint32_t W, uint32_t tpb,
                                                         uint8_t* __restrict__ roots) {
    extern __shared__ uint32_t lds_raw[];
    const uint32_t half = (W + 1) / 2, L = proof_levels(W), U = proof_tree_nodes(W);
    const uint32_t tw0 = blockIdx.x * tpb;
    const uint32_t ntw = 2 * W - tw0 < tpb ? 2 * W - tw0 : tpb;
    const uint32_t* leaf = store + (uint64_t)blockIdx.y * W * W * 8u;
    uint32_t* upper = store + (uint64_t)gridDim.y * W * W * 8u + ((uint64_t)blockIdx.y * 2 * W + tw0) * U * 8u;
    auto leaf_at = [&](uint32_t tree, uint32_t pos, uint32_t (&d)[8]) {
        const uint32_t axis = tree >= W ? 1u : 0u, idx = tree - axis * W;
        const uint64_t cell = axis == 0 ? (uint64_t)idx * W + pos : (uint64_t)pos * W + idx;
        const v4u* s = reinterpret_cast<const v4u*>(leaf + cell * 8u);
        const v4u a = s[0], b = s[1];
        d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
    };
    uint32_t prev = W, off = 0;  // nodes of level l - 1; level l's first node in a tree's block
    for (uint32_t l = 1; l <= L; ++l) {
        const uint32_t cnt = (prev + 1) / 2, tot = ntw * cnt;
        for (uint32_t v0 = 0; v0 < tot; v0 += 256u) {
            const uint32_t v = v0 + threadIdx.x;
            const bool act = v < tot;
            const uint32_t u = act ? v / cnt : 0u, j = act ? v - u * cnt : 0u;
            uint32_t o[8];
            if (act) {
                uint32_t a[8], b[8];
                const bool pair = 2 * j + 1 < prev;
                if (l == 1) {
                    leaf_at(tw0 + u, 2 * j, a);
                    if (pair) leaf_at(tw0 + u, 2 * j + 1, b);
                } else {
                    const uint32_t* lv = lds_raw + (size_t)u * half * 8u;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        a[i] = lv[(2 * j) * 8u + i];
                        b[i] = pair ? lv[(2 * j + 1) * 8u + i] : 0u;
                    }
                }
                if (pair) {
                    node_hash(a, b, o);
                } else {  // carried up unchanged
#pragma unroll
                    for (int i = 0; i < 8; ++i) o[i] = a[i];
                }
            }
            __syncthreads();  // every read of this pass precedes its in-place writes
            if (act) {
                uint32_t* lv = lds_raw + ((size_t)u * half + j) * 8u;
#pragma unroll
                for (int i = 0; i < 8; ++i) lv[i] = o[i];
                v4u* g = reinterpret_cast<v4u*>(upper + ((uint64_t)u * U + off + j) * 8u);
                g[0] = v4u{o[0], o[1], o[2], o[3]};
                g[1] = v4u{o[4], o[5], o[6], o[7]};
                if (l == L && roots) {  // cnt == 1: the root, as tree_root_kernel lays it out
                    uint32_t* r = reinterpret_cast<uint32_t*>(roots + ((uint64_t)blockIdx.y * 2 * W + tw0 + u) * 32u);
#pragma unroll
                    for (int i = 0; i < 8; ++i) r[i] = __builtin_bswap32(o[i]);
                }
            }
            __syncthreads();
        }
        off += cnt;
        prev = cnt;
    }
}

// Proof verification (rsm_kernels.hpp "Proof verification"), DefaultTree: one lane per
// sample.  The lane derives its proof's node count and operand sides from (W, pos) --
// level l contributes when ((pos >> l) ^ 1) < ceil(W / 2^l), its sibling is the right
// operand when pos >> l is even, proof_gather_kernel's picture -- and only compares the
// record's header with them (kProofMalformed).  It then streams its share through
// SHA-256 as leaf_hash_kernel does, folds the derived number of siblings in registers
// (two compressions each) and compares with its root: no intermediate buffer.  Records
// sit at any alignment (memcpy loads: gfx950 global loads need none); nothing past the
// derived nodes is read, and no address depends on what a record or a share holds.
// (proof_shape, fold_digests: dataroot_dev.hpp, shared with the chained kernels;
// share_leaf_hash, the leaf digest of a share: sha256_dev.hpp, shared with kernels_fraud.hip.)

__global__ __launch_bounds__(256) void proof_verify_kernel(const uint8_t* __restrict__ shares,
                                                           const uint8_t* __restrict__ records,
                                                           const uint8_t* __restrict__ roots, uint32_t W, uint32_t S,
                                                           const ProofSample* __restrict__ samples, uint32_t n,
                                                           uint32_t* __restrict__ status) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n) return;
    const ProofSample sm = samples[t];
    const uint8_t* rec = records + (uint64_t)t * (8u + proof_levels(W) * 32u);
    uint32_t mask = 0;
    const uint32_t n_nodes = proof_shape(W, sm.pos, &mask);
    if (ld_u32(rec) != n_nodes || ld_u32(rec + 4) != mask) {
        status[t] = kProofMalformed;
        return;
    }
    uint32_t h[8];
    share_leaf_hash(shares + (uint64_t)t * S, S, h);
    fold_digests(h, rec + 8u, n_nodes, mask);
    const uint8_t* rt = roots + (((uint64_t)sm.square * 2u + sm.axis) * W + sm.index) * 32u;
    uint32_t diff = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) diff |= h[q] ^ __builtin_bswap32(ld_u32(rt + 4 * q));
    status[t] = diff ? kProofRoot : kProofOk;
}

// Chained verification (rsm_kernels.hpp "data root"), DefaultTree: the same lane, with no
// root table.  Both headers -- the share record's against (W, pos), the root record's
// against (2W, axis W + index) -- are compared before anything is hashed; the share fold's
// digest is then hashed as leaf axis W + index of the data-root tree, folded through the
// root record and compared with the square's data root.  Both records sit at any
// alignment; nothing past either record's derived nodes is read.
__global__ __launch_bounds__(256) void proof_verify_data_root_kernel(
    const uint8_t* __restrict__ shares, const uint8_t* __restrict__ records, const uint8_t* __restrict__ root_records,
    const uint8_t* __restrict__ data_roots, uint32_t W, uint32_t S, const ProofSample* __restrict__ samples, uint32_t n,
    uint32_t* __restrict__ status) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n) return;
    const ProofSample sm = samples[t];
    const uint8_t* rec = records + (uint64_t)t * (8u + proof_levels(W) * 32u);
    const uint8_t* rrec = root_records + (uint64_t)t * (8u + proof_levels(2u * W) * 32u);
    uint32_t mask = 0, mask2 = 0;
    const uint32_t n_nodes = proof_shape(W, sm.pos, &mask);
    const uint32_t n2 = proof_shape(2u * W, sm.axis * W + sm.index, &mask2);
    if (ld_u32(rec) != n_nodes || ld_u32(rec + 4) != mask || ld_u32(rrec) != n2 || ld_u32(rrec + 4) != mask2) {
        status[t] = kProofMalformed;
        return;
    }
    uint32_t h[8];
    share_leaf_hash(shares + (uint64_t)t * S, S, h);
    fold_digests(h, rec + 8u, n_nodes, mask);
    uint32_t B[kRootWords], g[8];  // the candidate root: the digest itself
#pragma unroll
    for (int i = 0; i < kRootWords; ++i) B[i] = i < 8 ? h[i] : 0u;
    root_leaf_hash(B, 32u, g);
    status[t] = data_root_matches(g, rrec, n2, mask2, data_roots + (uint64_t)sm.square * 32u) ? kProofOk : kProofRoot;
}

// Range proof verification (rsm_kernels.hpp "range proofs"), DefaultTree: one WAVE per
// query, the picture of kernels_nmt.hip's namespace verifier with 8-word digests.  The
// wave's LDS holds one tree level in place, node p of a level at entry p (W entries and a
// spare one); no workgroup barrier: the waves of a workgroup share nothing.
//   header : the two offsets first (kProofMalformed: nothing else of the query is read),
//            then the record's header against the QUERY's [start, end) (host-validated:
//            start < end <= W) and the node count it dictates, then (CHAINED) the root
//            record's against (2W, axis W + index)
//   leaves : lane j hashes shares j, j + 64, .. into entries start + j, ..
//   fold   : level l grafts the left proof node at entry a - 1 when a is odd and the right
//            one at last + 1 when last is even and below the level's last node; lane j joins
//            entries a + 2j, a + 2j + 1 into entry a / 2 + j (both reads at or past the
//            write; a pass's reads precede its writes), an unpaired last entry is carried up
// Every lane hashes in every pass: past a pass's last leaf (node) a lane repeats one of the
// pass and stores it to the spare entry (a wave with few lanes active runs its SHA rounds
// slower per compression, see above).  Every address comes from (W, start, end) and the
// offsets; nothing of a record past its derived nodes is read.
constexpr size_t kRangeLdsCap = 160 * 1024 - 256;  // per workgroup

template <bool CHAINED>
__global__ __launch_bounds__(256) void range_verify_kernel(
    const uint8_t* __restrict__ records, const uint32_t* __restrict__ offsets, const uint8_t* __restrict__ shares,
    uint64_t shares_total, const uint8_t* __restrict__ roots, const uint8_t* __restrict__ root_records,
    const uint8_t* __restrict__ data_roots, uint32_t W, uint32_t S, const RangeQuery* __restrict__ queries, uint32_t n,
    uint32_t* __restrict__ status) {
    extern __shared__ uint32_t lds[];  // per wave: W digests and a spare one
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * (blockDim.x >> 6) + wv;
    if (q >= n) return;
    uint32_t* const row = lds + (size_t)wv * (W + 1u) * 8u;
    uint32_t* const spare = row + (size_t)W * 8u;
    auto done = [&](uint32_t st) {
        if (lane == 0) status[q] = st;
    };
    const uint32_t o0 = __builtin_amdgcn_readfirstlane(offsets[q]), o1 = __builtin_amdgcn_readfirstlane(offsets[q + 1]);
    if (o0 > o1 || o1 > shares_total) return done(kProofMalformed);
    const RangeQuery qu = queries[q];
    const uint32_t start = __builtin_amdgcn_readfirstlane(qu.start), end = __builtin_amdgcn_readfirstlane(qu.end);
    const uint32_t L = proof_levels(W);
    const uint8_t* rec = records + (uint64_t)q * (16u + (2u * L + 1u) * 32u);
    if (o1 - o0 != end - start || ld_u32(rec) != kNsInclusion || ld_u32(rec + 4) != start || ld_u32(rec + 8) != end)
        return done(kProofMalformed);
    uint32_t n_left = 0;
    if (ld_u32(rec + 12) != ns_range_nodes(W, start, end, &n_left)) return done(kProofMalformed);
    const uint8_t* rrec = nullptr;
    uint32_t n2 = 0, mask2 = 0;
    if constexpr (CHAINED) {
        rrec = root_records + (uint64_t)q * (8u + proof_levels(2u * W) * 32u);
        n2 = proof_shape(2u * W, qu.axis * W + qu.index, &mask2);
        if (ld_u32(rrec) != n2 || ld_u32(rrec + 4) != mask2) return done(kProofMalformed);
    }
    auto wave_sync = [] {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    auto put = [](uint32_t* p, const uint32_t (&d)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) p[i] = d[i];
    };
    auto get = [](const uint32_t* p, uint32_t (&d)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = p[i];
    };
    auto graft = [&](uint32_t entry, uint32_t node) {  // proof node `node` of the record into a level's entry
        if (lane == 0) {
            uint32_t d[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) d[i] = __builtin_bswap32(ld_u32(rec + 16u + node * 32u + 4 * i));
            put(row + (size_t)entry * 8u, d);
        }
    };
    for (uint32_t i0 = 0, n_shares = end - start; i0 < n_shares; i0 += 64u) {
        const uint32_t rem = n_shares - i0;
        const bool own = lane < rem;
        const uint32_t i = i0 + (own ? lane : lane % rem);
        uint32_t h[8];
        share_leaf_hash(shares + ((uint64_t)o0 + i) * S, S, h);
        put(own ? row + (size_t)(start + i) * 8u : spare, h);
    }
    uint32_t a = start, last = end - 1u, li = n_left, ri = n_left;  // next left node: li - 1; next right: ri
    for (uint32_t l = 0; l < L; ++l) {
        if (a & 1u) graft(--a, --li);
        if (!(last & 1u) && last + 1u < proof_level_count(W, l)) graft(++last, ri++);
        wave_sync();  // the leaves / the level below and the grafts are written
        const uint32_t have = last - a + 1u, np = have / 2u, up = np + (have & 1u);  // a is even
        for (uint32_t v0 = 0; v0 < up; v0 += 64u) {
            const uint32_t rem = up - v0;
            const bool own = lane < rem;
            const uint32_t j = v0 + (own ? lane : lane % rem);
            uint32_t x[8], o[8];
            get(row + (size_t)(a + 2u * j) * 8u, x);
            if (j < np) {
                uint32_t y[8];
                get(row + (size_t)(a + 2u * j + 1u) * 8u, y);
                node_hash(x, y, o);
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) o[i] = x[i];  // carried up unchanged
            }
            wave_sync();  // every lane's reads of this pass before any write (a / 2 + j <= a + 2 j)
            put(own ? row + (size_t)(a / 2u + j) * 8u : spare, o);
        }
        a >>= 1;
        last >>= 1;
    }
    wave_sync();
    uint32_t h[8];
    get(row, h);
    if constexpr (CHAINED) {
        uint32_t B[kRootWords], g[8];  // the candidate root: the digest itself
#pragma unroll
        for (int i = 0; i < kRootWords; ++i) B[i] = i < 8 ? h[i] : 0u;
        root_leaf_hash(B, 32u, g);
        done(data_root_matches(g, rrec, n2, mask2, data_roots + (uint64_t)qu.square * 32u) ? kProofOk : kProofRoot);
    } else {
        const uint8_t* rt = roots + (((uint64_t)qu.square * 2u + qu.axis) * W + qu.index) * 32u;
        done(digest_differs(h, rt) ? kProofRoot : kProofOk);
    }
}

}  // namespace

bool range_verify_supported(uint32_t W, uint32_t ns) {
    return ns == 0 ? W >= 1 && W <= 2 * kMaxLevel1 : nmt_ns_verify_supported(W, ns);
}

// One wave per query, up to four waves per workgroup: the count that lets most waves share
// a CU's LDS, as launch_nmt_ns_verify (W = 2048: 64 KiB a wave, two per CU).
hipError_t launch_range_verify(const uint8_t* d_records, const uint32_t* d_offsets, const uint8_t* d_shares,
                               uint64_t shares_total, const uint8_t* d_roots, const uint8_t* d_root_records,
                               const uint8_t* d_data_roots, uint32_t W, uint32_t S, const RangeQuery* d_queries, uint32_t n,
                               uint32_t* d_status, hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (!range_verify_supported(W, 0)) return hipErrorInvalidValue;
    const size_t wave_bytes = (size_t)(W + 1u) * 32u;
    uint32_t wpb = 1, best = 0;
    for (uint32_t b = 1; b <= 4; ++b) {
        if (b * wave_bytes > kRangeLdsCap) break;
        const uint32_t waves = (uint32_t)(kRangeLdsCap / (b * wave_bytes)) * b;  // per CU
        if (waves >= best) best = waves, wpb = b;
    }
    const dim3 grid((n + wpb - 1) / wpb), block(64 * wpb);
    if (d_root_records)
        hipLaunchKernelGGL(range_verify_kernel<true>, grid, block, wpb * wave_bytes, st, d_records, d_offsets, d_shares,
                           shares_total, d_roots, d_root_records, d_data_roots, W, S, d_queries, n, d_status);
    else
        hipLaunchKernelGGL(range_verify_kernel<false>, grid, block, wpb * wave_bytes, st, d_records, d_offsets, d_shares,
                           shares_total, d_roots, d_root_records, d_data_roots, W, S, d_queries, n, d_status);
    return hipGetLastError();
}

hipError_t launch_proof_verify(const uint8_t* d_shares, const uint8_t* d_records, const uint8_t* d_roots, uint32_t W,
                               uint32_t S, const ProofSample* d_samples, uint32_t n, uint32_t* d_status, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(proof_verify_kernel, dim3((n + 255) / 256), dim3(256), 0, st, d_shares, d_records, d_roots, W, S,
                       d_samples, n, d_status);
    return hipGetLastError();
}

hipError_t launch_proof_verify_data_root(const uint8_t* d_shares, const uint8_t* d_records, const uint8_t* d_root_records,
                                         const uint8_t* d_data_roots, uint32_t W, uint32_t S,
                                         const ProofSample* d_samples, uint32_t n, uint32_t* d_status, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(proof_verify_data_root_kernel, dim3((n + 255) / 256), dim3(256), 0, st, d_shares, d_records,
                       d_root_records, d_data_roots, W, S, d_samples, n, d_status);
    return hipGetLastError();
}

// Trees a workgroup of the node-store builds takes: as many as fill its 256 lanes at
// level 1 (at most 32: the NMT build keeps one failure bit per tree in a word).
uint32_t proof_trees_per_block(uint32_t W) {
    const uint32_t half = (W + 1) / 2;
    const uint32_t t = 256u / half;
    return t < 1u ? 1u : (t > 32u ? 32u : t);
}

hipError_t launch_tree_nodes(const uint8_t* d_eds, uint32_t W, uint32_t S, uint32_t squares, uint32_t* d_store,
                             uint8_t* d_roots, hipStream_t st) {
    const uint32_t cells = W * W * squares;
    hipLaunchKernelGGL(leaf_hash_kernel, dim3((cells + 255) / 256), dim3(256), 0, st, d_eds, cells, S, d_store);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t tpb = proof_trees_per_block(W);
    const size_t lds = (size_t)tpb * ((W + 1) / 2) * 8u * 4u;
    hipLaunchKernelGGL(tree_nodes_kernel, dim3((2 * W + tpb - 1) / tpb, squares), dim3(256), lds, st, d_store, W, tpb,
                       d_roots);
    return hipGetLastError();
}

bool roots_dev_supported(uint32_t W) { return W >= 2 && W <= 2 * kMaxLevel1 && W < (1u << 16); }

// `squares` consecutive [W][W][S] squares; d_leaf: scratch of squares*W*W*32 bytes.
// The cells of all squares are one leaf launch (a single square is only W*W
// threads: one wave per SIMD on a 256-CU chip, latency-bound SHA rounds).
hipError_t launch_roots(const uint8_t* d_eds, uint32_t W, uint32_t S, uint32_t squares, uint32_t* d_leaf,
                        uint8_t* d_roots, hipStream_t st) {
    const uint32_t cells = W * W * squares;
    hipLaunchKernelGGL(leaf_hash_kernel, dim3((cells + 255) / 256), dim3(256), 0, st, d_eds, cells, S, d_leaf);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_tree_kernel(d_leaf, W, d_roots, 0u, 2 * W, squares, squares == 1, st);
}

// Pieces of launch_roots for one square, so a caller can hash rows as they become
// final: leaf digests of `cells` consecutive cells (d_cells -> d_leaf, both already
// offset to the first cell), and the trees [first, first + count) (row trees 0..W-1,
// column trees W..2W-1) over a complete leaf array.
hipError_t launch_leaf_hashes(const uint8_t* d_cells, uint32_t cells, uint32_t S, uint32_t* d_leaf, hipStream_t st) {
    if (cells == 0) return hipSuccess;
    hipLaunchKernelGGL(leaf_hash_kernel, dim3((cells + 255) / 256), dim3(256), 0, st, d_cells, cells, S, d_leaf);
    return hipGetLastError();
}
hipError_t launch_tree_roots(const uint32_t* d_leaf, uint32_t W, uint32_t first, uint32_t count, uint8_t* d_roots,
                             hipStream_t st) {
    if (count == 0) return hipSuccess;
    return launch_tree_kernel(d_leaf, W, d_roots, first, count, 1, true, st);
}

// ---- list-driven forms (checked Repair; rsm_kernels.hpp) ------------------------------
namespace {

// One lane per (entry, position) of square blockIdx.y.  The lane that sets the cell's bit
// in `recorded` hashes the cell; hashed[s] += the records computed (one add per wave).
__global__ __launch_bounds__(256) void list_leaf_hash_kernel(const uint8_t* __restrict__ eds, uint32_t W, uint32_t S,
                                                             const uint32_t* __restrict__ list,
                                                             const uint32_t* __restrict__ cnt, uint32_t* recorded,
                                                             uint32_t* hashed, uint32_t* __restrict__ leaf) {
    const uint32_t s = blockIdx.y, i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t e = i / W, pos = i - e * W;
    uint32_t axis, index;
    uint64_t slot;
    if (!list_entry(list, cnt, W, s, e, &axis, &index, &slot)) return;
    const uint32_t cell = axis == 0 ? index * W + pos : pos * W + index;
    const uint32_t bit = 1u << (cell & 31u);
    const bool fresh = !(atomicOr(&recorded[(uint64_t)s * ((W * W + 31u) / 32u) + (cell >> 5)], bit) & bit);
    if (fresh) {
        uint32_t h[8];
        share_leaf_hash(eds + ((uint64_t)s * W * W + cell) * S, S, h);
        v4u* o = reinterpret_cast<v4u*>(leaf + ((uint64_t)s * W * W + cell) * 8u);
        o[0] = v4u{h[0], h[1], h[2], h[3]};
        o[1] = v4u{h[4], h[5], h[6], h[7]};
    }
    const uint64_t b = __ballot(fresh);
    if (b && (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(b)) atomicAdd(&hashed[s], (uint32_t)__popcll(b));
}

// One tree per wave (entry blockIdx.x * 4 + wave of square blockIdx.y) in the wave's own
// LDS (wave_tree_levels, sha256_dev.hpp), the leaves along the row or strided down the
// column.  Lane 0 compares the root with the committed one.
__global__ __launch_bounds__(256) void list_tree_check_kernel(const uint32_t* __restrict__ leaf, uint32_t W,
                                                              const uint32_t* __restrict__ list,
                                                              const uint32_t* __restrict__ cnt,
                                                              const uint8_t* __restrict__ committed,
                                                              uint32_t* __restrict__ verdict) {
    extern __shared__ uint32_t lds_raw[];
    const uint32_t s = blockIdx.y, wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t axis, index;
    uint64_t slot;
    if (!list_entry(list, cnt, W, s, blockIdx.x * 4u + wv, &axis, &index, &slot)) return;  // the whole wave
    uint32_t* const lv = lds_raw + (size_t)wv * ((W + 1) / 2) * 8u;
    leaf += (uint64_t)s * W * W * 8u;
    wave_tree_levels(
        [&](uint32_t pos) {
            const uint64_t cell = axis == 0 ? (uint64_t)index * W + pos : (uint64_t)pos * W + index;
            return leaf + cell * 8u;
        },
        W, lv, lane);
    if (lane == 0)
        verdict[slot] = digest_differs(lv, committed + (((uint64_t)s * 2u + axis) * W + index) * 32u) ? kByzRoot : 0u;
}

}  // namespace

hipError_t launch_list_leaf_hashes(const uint8_t* d_eds, uint32_t W, uint32_t S, uint32_t count, uint32_t max_n,
                                   const uint32_t* d_list, const uint32_t* d_cnt, uint32_t* d_recorded,
                                   uint32_t* d_hashed, uint32_t* d_leaf, hipStream_t st) {
    if (count == 0 || max_n == 0) return hipSuccess;
    hipLaunchKernelGGL(list_leaf_hash_kernel, dim3((max_n * W + 255) / 256, count), dim3(256), 0, st, d_eds, W, S, d_list,
                       d_cnt, d_recorded, d_hashed, d_leaf);
    return hipGetLastError();
}

hipError_t launch_list_tree_check(const uint32_t* d_leaf, uint32_t W, uint32_t count, uint32_t max_n,
                                  const uint32_t* d_list, const uint32_t* d_cnt, const uint8_t* d_committed,
                                  uint32_t* d_verdict, hipStream_t st) {
    if (count == 0 || max_n == 0) return hipSuccess;
    if (!roots_dev_supported(W)) return hipErrorInvalidValue;
    const size_t lds = (size_t)4 * ((W + 1) / 2) * 8u * 4u;  // W = 2048: 128 KiB
    hipLaunchKernelGGL(list_tree_check_kernel, dim3((max_n + 3) / 4, count), dim3(256), lds, st, d_leaf, W, d_list, d_cnt,
                       d_committed, d_verdict);
    return hipGetLastError();
}

}  // namespace rsm
