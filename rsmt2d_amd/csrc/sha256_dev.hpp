// sha256_dev.hpp -- SHA-256 compression for the device hashing kernels
// (kernels_sha.hip: DefaultTree; kernels_nmt.hip: namespaced Merkle tree).
// Messages are handled as big-endian 32-bit words, as the standard defines them.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rsm {
namespace {

__constant__ uint32_t kK[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
    0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
    0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
    0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
    0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

constexpr uint32_t kH0[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a,
                             0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};

__device__ __forceinline__ uint32_t rotr(uint32_t x, int n) { return __builtin_amdgcn_alignbit(x, x, n); }
// Big-endian message word whose first byte is the last byte of `prev` and whose
// other three are the first three bytes of `cur` (both big-endian words): the
// 1-byte domain prefix shifts every share word by one byte.
__device__ __forceinline__ uint32_t shift8(uint32_t prev, uint32_t cur) {
    return __builtin_amdgcn_alignbit(prev, cur, 8);
}

// three-input XOR in one VALU op (gfx950 v_bitop3_b32, truth table 0x96)
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

__device__ __forceinline__ void sha_block(uint32_t (&h)[8], uint32_t (&w)[16]) {
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        if (i >= 16) {
            const uint32_t x = w[(i + 1) & 15], y = w[(i + 14) & 15];
            const uint32_t s0 = xor3(rotr(x, 7), rotr(x, 18), x >> 3);
            const uint32_t s1 = xor3(rotr(y, 17), rotr(y, 19), y >> 10);
            w[i & 15] += s0 + w[(i + 9) & 15] + s1;
        }
        const uint32_t S1 = xor3(rotr(e, 6), rotr(e, 11), rotr(e, 25));
        const uint32_t ch = (e & f) ^ (~e & g);
        const uint32_t t1 = hh + S1 + ch + kK[i] + w[i & 15];
        const uint32_t S0 = xor3(rotr(a, 2), rotr(a, 13), rotr(a, 22));
        const uint32_t mj = (a & b) ^ (a & c) ^ (b & c);
        hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + S0 + mj;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

// SHA256(0x01 || L || R) for digests held as 8 big-endian words each.
__device__ __forceinline__ void node_hash(const uint32_t (&L)[8], const uint32_t (&R)[8], uint32_t (&out)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = kH0[i];
    uint32_t w[16];
    w[0] = shift8(0x01u, L[0]);
#pragma unroll
    for (int i = 1; i < 8; ++i) w[i] = shift8(L[i - 1], L[i]);
    w[8] = shift8(L[7], R[0]);
#pragma unroll
    for (int i = 1; i < 8; ++i) w[8 + i] = shift8(R[i - 1], R[i]);
    sha_block(out, w);
    w[0] = (R[7] << 24) | 0x00800000u;
#pragma unroll
    for (int i = 1; i < 15; ++i) w[i] = 0;
    w[15] = 65u * 8u;
    sha_block(out, w);
}

// a 32-bit load at any alignment (memcpy: gfx950 global loads need none)
__device__ __forceinline__ uint32_t ld_u32(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// the leaf digest of a share (S a multiple of 64, 16-byte aligned), as leaf_hash_kernel
__device__ __forceinline__ void share_leaf_hash(const uint8_t* share, uint32_t S, uint32_t (&h)[8]) {
    const v4u* p = reinterpret_cast<const v4u*>(share);
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = kH0[i];
    uint32_t prev = 0;  // the 0x00 leaf prefix
    for (uint32_t blk = 0; blk < S / 64u; ++blk) {
        uint32_t w[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const v4u v = p[blk * 4u + q];
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
    w[0] = (prev << 24) | 0x00800000u;
#pragma unroll
    for (int i = 1; i < 15; ++i) w[i] = 0;
    w[15] = (S + 1u) * 8u;
    sha_block(h, w);
}

// One DefaultTree per wave, by levels in the wave's own LDS `lv` (ceil(W / 2) digests of 8
// words; W >= 2): node (l, j) over leaves [j 2^l, min((j + 1) 2^l, W)), an unpaired last
// node carried up unchanged -- tree_nodes_kernel's picture, the same tree as
// tree_root_kernel's stack of subtrees.  A level is built in place (node j reads 2j and
// 2j + 1 >= j; a 64-node pass reads before it writes, later passes read beyond what it
// wrote), level 1 from the leaf records: record_at(pos) is leaf pos' 8 words, 16-byte
// aligned.  The root is lv[0 .. 7] when it returns.
template <class RecordAt>
__device__ __forceinline__ void wave_tree_levels(RecordAt&& record_at, uint32_t W, uint32_t* lv, uint32_t lane) {
    auto leaf_at = [&](uint32_t pos, uint32_t (&d)[8]) {
        const v4u* p = reinterpret_cast<const v4u*>(record_at(pos));
        const v4u a = p[0], b = p[1];
        d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
    };
    uint32_t prev = W;
    for (uint32_t l = 1; prev > 1; ++l) {
        const uint32_t n = (prev + 1) / 2;
        for (uint32_t j0 = 0; j0 < n; j0 += 64u) {
            const uint32_t j = j0 + lane;
            uint32_t a[8], b[8], o[8];
            const bool act = j < n, pair = 2 * j + 1 < prev;
            if (act) {
                if (l == 1) {
                    leaf_at(2 * j, a);
                    if (pair) leaf_at(2 * j + 1, b);
                } else {
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        a[q] = lv[(2 * j) * 8u + q];
                        b[q] = pair ? lv[(2 * j + 1) * 8u + q] : 0u;
                    }
                }
                if (pair) {
                    node_hash(a, b, o);
                } else {
#pragma unroll
                    for (int q = 0; q < 8; ++q) o[q] = a[q];
                }
            }
            // every read of this pass precedes its in-place writes
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (act) {
#pragma unroll
                for (int q = 0; q < 8; ++q) lv[j * 8u + q] = o[q];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        prev = n;
    }
}

// whether the digest d (8 big-endian words) differs from the 32 bytes at rt (any alignment)
__device__ __forceinline__ bool digest_differs(const uint32_t* d, const uint8_t* rt) {
    uint32_t diff = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) diff |= d[q] ^ __builtin_bswap32(ld_u32(rt + 4 * q));
    return diff != 0;
}

}  // namespace
}  // namespace rsm
