// dataroot_dev.hpp -- device helpers of the data-root tree (DESIGN.md §4 "Data root";
// rsm_kernels.hpp "data root"), shared by its build and gather kernels
// (kernels_dataroot.hip) and by the chained verify kernels (kernels_sha.hip,
// kernels_nmt.hip).  The tree is the level picture over N = 2W leaves, leaf t the root
// bytes of tree t (rows, then columns); every node is a 32-byte digest:
//   leaf = SHA256(0x00 || root bytes),  node = SHA256(0x01 || l || r),
// an unpaired last node carried up unchanged (RFC 6962's split).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "rsm_kernels.hpp"
#include "sha256_dev.hpp"

namespace rsm {
namespace {

// Node count of the proof of leaf `pos` among n leaves; *mask: bit i set where node i is
// the right operand of its parent hash (proof_gather_kernel's picture).
__device__ __forceinline__ uint32_t proof_shape(uint32_t n, uint32_t pos, uint32_t* mask) {
    uint32_t n_nodes = 0, m = 0;
    for (uint32_t l = 0, L = proof_levels(n); l < L; ++l) {
        const uint32_t j = pos >> l;
        if ((j ^ 1u) < proof_level_count(n, l)) {
            if (!(j & 1u)) m |= 1u << n_nodes;
            ++n_nodes;
        }
    }
    *mask = m;
    return n_nodes;
}

// Folds n_nodes 32-byte siblings at `nodes` (any alignment) into h, bottom-up; bit i of
// mask: sibling i is the right operand.  Two compressions each; reads nothing past them.
__device__ __forceinline__ void fold_digests(uint32_t (&h)[8], const uint8_t* nodes, uint32_t n_nodes, uint32_t mask) {
    for (uint32_t i = 0; i < n_nodes; ++i) {
        const uint8_t* nd = nodes + i * 32u;
        const bool right = (mask >> i) & 1u;  // the sibling is the right operand
        uint32_t a[8], b[8], o[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const uint32_t x = __builtin_bswap32(ld_u32(nd + 4 * q));
            a[q] = right ? h[q] : x;
            b[q] = right ? x : h[q];
        }
        node_hash(a, b, o);
#pragma unroll
        for (int q = 0; q < 8; ++q) h[q] = o[q];
    }
}

constexpr int kRootWords = 24;  // a root of at most 96 bytes as big-endian words

// the first n bytes of a big-endian word (n clamped to 0..4)
__device__ __forceinline__ uint32_t dr_head_mask(int n) {
    return n <= 0 ? 0u : (n >= 4 ? 0xFFFFFFFFu : ~(0xFFFFFFFFu >> (8 * n)));
}

// h = SHA256(0x00 || the first len bytes of B) for 32 <= len <= 96, B the root bytes as
// big-endian words (what lies past byte len is masked off).  Message word m holds
// message bytes 4m .. 4m + 3: the prefix shifts B by one byte; the 0x80 pad byte sits at
// message byte 1 + len; 1 + len <= 55 is one block, else two (1 + len = 56 .. 64: the
// second holds padding only).
__device__ __forceinline__ void root_leaf_hash(const uint32_t (&B)[kRootWords], uint32_t len, uint32_t (&h)[8]) {
    const int L = 1 + (int)len;  // message length
    const bool two = L > 55;
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = kH0[i];
    uint32_t w[16];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        if (b == 1 && !two) break;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int m = 16 * b + i, p = 4 * m;
            uint32_t x = 0;
            if (m <= kRootWords) x = shift8(m == 0 ? 0u : B[m - 1], m < kRootWords ? B[m] : 0u) & dr_head_mask(L - p);
            if (p <= L && L < p + 4) x |= 0x80u << (8 * (3 - (L - p)));
            w[i] = x;
        }
        if ((b == 1) == two) w[15] = 8u * (uint32_t)L;
        sha_block(h, w);
    }
}

// The root bytes at p (len bytes, any alignment) as big-endian words; nothing past
// p + len is read.
__device__ __forceinline__ void root_words_from_bytes(const uint8_t* p, uint32_t len, uint32_t (&B)[kRootWords]) {
#pragma unroll
    for (int i = 0; i < kRootWords; ++i) {
        uint32_t x = 0;
        if (4u * i + 4u <= len) {
            x = __builtin_bswap32(ld_u32(p + 4 * i));
        } else {
#pragma unroll
            for (int q = 0; q < 3; ++q)
                if (4u * i + q < len) x |= (uint32_t)p[4 * i + q] << (24 - 8 * q);
        }
        B[i] = x;
    }
}

// The second half of a chained verification: h is the leaf digest of the candidate
// root; folds the derived n2 nodes of the root record and compares with the 32-byte
// data root at `dr` (any alignment).
__device__ __forceinline__ bool data_root_matches(uint32_t (&h)[8], const uint8_t* root_rec, uint32_t n2, uint32_t mask2,
                                                  const uint8_t* dr) {
    fold_digests(h, root_rec + 8u, n2, mask2);
    uint32_t diff = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) diff |= h[q] ^ __builtin_bswap32(ld_u32(dr + 4 * q));
    return diff == 0;
}

}  // namespace
}  // namespace rsm
