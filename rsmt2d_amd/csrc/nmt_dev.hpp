// nmt_dev.hpp -- device helpers of the namespaced-Merkle-tree kernels (kernels_nmt.hip:
// squares; kernels_fraud.hip: packed vectors): a node as big-endian words, HashNode on a
// lane's LDS message bytes, and the leaf node of a share.  The tree itself is described
// in kernels_nmt.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "sha256_dev.hpp"

namespace rsm {
namespace {

constexpr uint32_t kMaxNs = 32;
constexpr uint32_t kNsWords = kMaxNs / 4;
constexpr uint32_t kNodeWords = 3 * kNsWords;  // min[8] | max[8] | digest[8] (LDS)
constexpr uint32_t kLeafWords = 16;            // ns[8] | digest[8] (global, per cell)

// SHA blocks of a node message 0x01 || l || r (nodes of 2 ns + 32 bytes)
__host__ __device__ constexpr uint32_t node_blocks(uint32_t ns) { return (1 + 2 * (2 * ns + 32) + 8) / 64 + 1; }
inline size_t tree_lds_bytes(uint32_t W, uint32_t ns) {  // two levels, a spare node, 256 message buffers
    return ((size_t)(2 * (W / 2) + 1) * kNodeWords + (size_t)256 * 16 * node_blocks(ns)) * 4;
}

// the first n bytes of a big-endian word (n clamped to 0..4)
__device__ __forceinline__ uint32_t head_mask(int n) {
    return n <= 0 ? 0u : (n >= 4 ? 0xFFFFFFFFu : ~(0xFFFFFFFFu >> (8 * n)));
}
__device__ __forceinline__ uint32_t be_word(const uint32_t* p, int i) { return __builtin_bswap32(p[i]); }

struct Node {
    uint32_t mn[kNsWords], mx[kNsWords], d[8];
};

// a < b over namespaces held as zero-padded big-endian words
__device__ __forceinline__ bool ns_less(const uint32_t (&a)[kNsWords], const uint32_t (&b)[kNsWords]) {
#pragma unroll
    for (int i = 0; i < (int)kNsWords; ++i)
        if (a[i] != b[i]) return a[i] < b[i];
    return false;
}

// byte i of a big-endian word array (i static after unrolling)
__device__ __forceinline__ uint8_t be_byte(const uint32_t* w, int i) { return (uint8_t)(w[i >> 2] >> (24 - 8 * (i & 3))); }

// HashNode(l, r) (nmt hasher): message 0x01 || l || r laid out in this thread's
// LDS bytes `mb`, then hashed as big-endian words.  Returns false on unordered
// siblings (r.min < l.max).
__device__ __forceinline__ bool hash_node(const Node& l, const Node& r, uint32_t ns, bool ignore_max, uint8_t* mb, Node& out) {
    const int NL = 2 * (int)ns + 32;
    const int len = 1 + 2 * NL;
    const int nb = (int)node_blocks(ns);
    uint32_t* mw = reinterpret_cast<uint32_t*>(mb);
    for (int i = 0; i < 16 * nb; ++i) mw[i] = 0;
    mb[0] = 0x01;
    auto put = [&](const Node& n, int at) {
#pragma unroll
        for (int i = 0; i < (int)kMaxNs; ++i)
            if (i < (int)ns) {
                mb[at + i] = be_byte(n.mn, i);
                mb[at + (int)ns + i] = be_byte(n.mx, i);
            }
#pragma unroll
        for (int i = 0; i < 32; ++i) mb[at + 2 * (int)ns + i] = be_byte(n.d, i);
    };
    put(l, 1);
    put(r, 1 + NL);
    mb[len] = 0x80;
    const uint32_t bits = 8u * (uint32_t)len;
    mb[64 * nb - 2] = (uint8_t)(bits >> 8);
    mb[64 * nb - 1] = (uint8_t)bits;
    uint32_t h[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = kH0[i];
    for (int b = 0; b < nb; ++b) {
        uint32_t w[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = __builtin_bswap32(mw[16 * b + i]);
        sha_block(h, w);
    }
    bool rmin_is_max = true;
#pragma unroll
    for (int i = 0; i < (int)kNsWords; ++i) rmin_is_max &= r.mn[i] == head_mask((int)ns - 4 * i);
    const bool ok = !ns_less(r.mn, l.mx);
#pragma unroll
    for (int i = 0; i < (int)kNsWords; ++i) {
        out.mn[i] = l.mn[i];
        out.mx[i] = (ignore_max && rmin_is_max) ? l.mx[i] : r.mx[i];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) out.d[i] = h[i];
    return ok;
}

__device__ __forceinline__ void leaf_node(const uint32_t* __restrict__ leaf, uint64_t cell, Node& n) {
    const uint32_t* s = leaf + cell * kLeafWords;
#pragma unroll
    for (int i = 0; i < (int)kNsWords; ++i) n.mn[i] = n.mx[i] = s[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) n.d[i] = s[kNsWords + i];
}
__device__ __forceinline__ void lds_node(const uint32_t* p, Node& n) {
#pragma unroll
    for (int i = 0; i < (int)kNsWords; ++i) n.mn[i] = p[i], n.mx[i] = p[kNsWords + i];
#pragma unroll
    for (int i = 0; i < 8; ++i) n.d[i] = p[2 * kNsWords + i];
}
__device__ __forceinline__ void lds_store(uint32_t* p, const Node& n) {
#pragma unroll
    for (int i = 0; i < (int)kNsWords; ++i) p[i] = n.mn[i], p[kNsWords + i] = n.mx[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) p[2 * kNsWords + i] = n.d[i];
}

// One tree per workgroup of 256 lanes over W leaf records (leaf + cell_of(pos) * kLeafWords),
// level by level.  lds: tree_lds_bytes(W, ns) -- two levels of W / 2 nodes (ping-pong), a
// spare node, 256 per-thread message buffers.  Push order is checked on every consecutive
// leaf pair and sibling order at every node: *failed is non-zero where either fails.  The
// whole workgroup calls this; the root's LDS words are returned after its last barrier.
template <class CellOf>
__device__ __forceinline__ const uint32_t* block_tree_levels(const uint32_t* __restrict__ leaf, CellOf&& cell_of, uint32_t W,
                                                             uint32_t ns, bool ig, uint32_t* lds, uint32_t* failed) {
    const uint32_t half = W / 2;
    auto lvl = [&](uint32_t which) -> uint32_t* { return lds + (size_t)which * half * kNodeWords; };
    // the spare node: lanes past a level's last node store their repeat there (below)
    uint32_t* const spare = lds + (size_t)2 * half * kNodeWords;
    uint8_t* mb = reinterpret_cast<uint8_t*>(spare + kNodeWords) + threadIdx.x * (64u * node_blocks(ns));
    __shared__ uint32_t bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    uint32_t my_bad = 0;
    // level 1 from the leaf records: pairs (2j, 2j+1); push order checked on
    // every consecutive leaf pair
    // A level's pass runs every lane of the wave that holds its last node: lanes past
    // it repeat node j0 + tid % rem and store to the spare node (a wave with few lanes
    // active hashes 2-3.5x slower per compression: kernels_sha.hip); whole waves past
    // it stay idle.
    auto pass_lane = [&](uint32_t j0, uint32_t n, uint32_t& j, bool& own) -> bool {
        const uint32_t rem = n - j0;
        own = threadIdx.x < rem;
        if (!own && (threadIdx.x >> 6) != ((rem - 1) >> 6)) return false;
        j = j0 + (own ? threadIdx.x : threadIdx.x % rem);
        return true;
    };
    uint32_t cnt = W;
    uint32_t next = (cnt + 1) / 2;
    for (uint32_t j0 = 0; j0 < next; j0 += 256u) {
        uint32_t j;
        bool own;
        if (!pass_lane(j0, next, j, own)) continue;
        Node a, b, o;
        uint32_t bad_here = 0;
        leaf_node(leaf, cell_of(2 * j), a);
        if (2 * j + 1 < cnt) {
            leaf_node(leaf, cell_of(2 * j + 1), b);
            if (ns_less(b.mn, a.mn)) bad_here = 1;
            if (2 * j + 2 < cnt) {
                Node c;
                leaf_node(leaf, cell_of(2 * j + 2), c);
                if (ns_less(c.mn, b.mn)) bad_here = 1;
            }
            if (!hash_node(a, b, ns, ig, mb, o)) bad_here = 1;
        } else {
            o = a;
        }
        if (own) my_bad |= bad_here;
        lds_store(own ? lvl(0) + (size_t)j * kNodeWords : spare, o);
    }
    __syncthreads();
    uint32_t cur = 0;
    for (cnt = next; cnt > 1; cnt = next) {
        next = (cnt + 1) / 2;
        for (uint32_t j0 = 0; j0 < next; j0 += 256u) {
            uint32_t j;
            bool own;
            if (!pass_lane(j0, next, j, own)) continue;
            Node a, b, o;
            lds_node(lvl(cur) + (size_t)(2 * j) * kNodeWords, a);
            if (2 * j + 1 < cnt) {
                lds_node(lvl(cur) + (size_t)(2 * j + 1) * kNodeWords, b);
                if (!hash_node(a, b, ns, ig, mb, o) && own) my_bad = 1;
            } else {
                o = a;
            }
            lds_store(own ? lvl(cur ^ 1u) + (size_t)j * kNodeWords : spare, o);
        }
        __syncthreads();
        cur ^= 1u;
    }
    if (my_bad) atomicOr(&bad, 1u);
    __syncthreads();
    *failed = bad;
    return lvl(cur);
}

// whether node n differs from the min || max || digest bytes at c (2 ns + 32, any alignment)
__device__ __forceinline__ bool node_differs(const Node& n, const uint8_t* c, uint32_t ns) {
    uint32_t diff = 0;
#pragma unroll
    for (int i = 0; i < (int)kMaxNs; ++i)
        if (i < (int)ns) diff |= (uint32_t)(be_byte(n.mn, i) ^ c[i]) | (uint32_t)(be_byte(n.mx, i) ^ c[ns + i]);
#pragma unroll
    for (int i = 0; i < 32; ++i) diff |= (uint32_t)(be_byte(n.d, i) ^ c[2 * ns + i]);
    return diff != 0;
}

typedef uint32_t nv4u __attribute__((ext_vector_type(4)));

// the leaf node of a share (S a multiple of 64; 16-byte aligned), as nmt_leaf29_kernel
__device__ __forceinline__ void verify_leaf29(const uint8_t* share, uint32_t S, bool q0, Node& out) {
    const nv4u* p = reinterpret_cast<const nv4u*>(share);
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
#pragma unroll
    for (int i = 0; i < (int)kNsWords; ++i) out.mn[i] = out.mx[i] = (q0 ? nsw[i] : 0xFFFFFFFFu) & head_mask(29 - 4 * i);
#pragma unroll
    for (int i = 0; i < 8; ++i) out.d[i] = h[i];
}

// the same for any namespace size (S >= ns, a multiple of 4), as nmt_leaf_kernel
__device__ __forceinline__ void verify_leaf(const uint8_t* share, uint32_t S, uint32_t ns, bool q0, Node& out) {
    const uint32_t* dw = reinterpret_cast<const uint32_t*>(share);
    const int nD = (int)(S / 4u);
    const int off = 1 + (int)ns;  // message bytes before the share
    const int L = off + (int)S;   // message length
    const int m0 = off >> 2;      // first word holding share bytes
    const uint32_t sh = 8u * (uint32_t)(off & 3);
    const int nb = (L + 8) / 64 + 1;
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
            if (b == nb - 1 && i == 15) x = 8u * (uint32_t)L;
            w[i] = x;
        }
        sha_block(h, w);
    }
#pragma unroll
    for (int i = 0; i < (int)kNsWords; ++i) out.mn[i] = out.mx[i] = (q0 ? d0[i] : 0xFFFFFFFFu) & head_mask((int)ns - 4 * i);
#pragma unroll
    for (int i = 0; i < 8; ++i) out.d[i] = h[i];
}

}  // namespace
}  // namespace rsm
