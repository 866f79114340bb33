// merkle.cpp -- host restatement of rsmt2d's DefaultTree (tree.go:32-59):
// celestiaorg/merkletree over SHA-256 with leaf = H(0x00 || data) and
// node = H(0x01 || left || right); for a non-power-of-two leaf count the
// subtrees are joined right-to-left exactly as the NebulousLabs-style stack
// (push joins equal-height subtrees; Root folds the stack from the newest).
// The Tree plugin is out of the GPU hot path: it stays on
// the host, and callers may pass their own rsm_tree_root_fn instead.
//
// Also the host form of the namespaced Merkle tree (celestiaorg/nmt v0.24.3, a
// go.mod dependency absent from /root/reference) as rsmt2d's NMT wrappers push it
// (nmtwrapper_test.go:94-120, nmtbuffered_tree_test.go:118-152): see
// rsm_nmt_tree_root below; the device form is kernels_nmt.hip.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__x86_64__)
#include <cpuid.h>
#include <immintrin.h>
#endif

#include "../../include/rsmt2d_hip.h"

namespace {

#if defined(__x86_64__)
// SHA-256 compression with the x86 SHA extensions (the GPU box's EPYC and Intel
// hosts since Ice Lake have them): ~5-7x the scalar loop below, which stays as the
// fallback.  The host roots are on the fraud-proof and pre-repair paths.
bool cpu_has_sha_ni() {
    unsigned a = 0, b = 0, c = 0, d = 0;
    if (!__get_cpuid_count(7, 0, &a, &b, &c, &d) || !(b & (1u << 29))) return false;  // SHA
    if (!__get_cpuid(1, &a, &b, &c, &d)) return false;
    return (c & (1u << 19)) && (c & (1u << 9));  // SSE4.1, SSSE3
}

alignas(16) constexpr uint32_t kShaK[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
    0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
    0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
    0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
    0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

__attribute__((target("sha,sse4.1,ssse3"))) void sha256_block_ni(uint32_t h[8], const uint8_t* p) {
    const __m128i bswap = _mm_set_epi64x(0x0c0d0e0f08090a0bLL, 0x0405060700010203LL);
    __m128i t = _mm_shuffle_epi32(_mm_loadu_si128(reinterpret_cast<const __m128i*>(h)), 0xB1);  // CDAB
    __m128i s1 = _mm_shuffle_epi32(_mm_loadu_si128(reinterpret_cast<const __m128i*>(h + 4)), 0x1B);  // EFGH
    __m128i s0 = _mm_alignr_epi8(t, s1, 8);  // ABEF
    s1 = _mm_blend_epi16(s1, t, 0xF0);        // CDGH
    const __m128i abef = s0, cdgh = s1;
    __m128i w[4];
    for (int g = 0; g < 16; ++g) {  // four rounds per group
        __m128i m;
        if (g < 4) {
            m = _mm_shuffle_epi8(_mm_loadu_si128(reinterpret_cast<const __m128i*>(p + 16 * g)), bswap);
        } else {  // W[t..t+3] from the groups g-4, g-3, g-2, g-1
            m = _mm_sha256msg1_epu32(w[g & 3], w[(g + 1) & 3]);
            m = _mm_add_epi32(m, _mm_alignr_epi8(w[(g + 3) & 3], w[(g + 2) & 3], 4));
            m = _mm_sha256msg2_epu32(m, w[(g + 3) & 3]);
        }
        w[g & 3] = m;
        const __m128i wk = _mm_add_epi32(m, _mm_load_si128(reinterpret_cast<const __m128i*>(kShaK + 4 * g)));
        s1 = _mm_sha256rnds2_epu32(s1, s0, wk);
        s0 = _mm_sha256rnds2_epu32(s0, s1, _mm_shuffle_epi32(wk, 0x0E));
    }
    s0 = _mm_add_epi32(s0, abef);
    s1 = _mm_add_epi32(s1, cdgh);
    t = _mm_shuffle_epi32(s0, 0x1B);      // FEBA
    s1 = _mm_shuffle_epi32(s1, 0xB1);     // DCHG
    s0 = _mm_blend_epi16(t, s1, 0xF0);    // DCBA
    s1 = _mm_alignr_epi8(s1, t, 8);       // HGFE
    _mm_storeu_si128(reinterpret_cast<__m128i*>(h), s0);
    _mm_storeu_si128(reinterpret_cast<__m128i*>(h + 4), s1);
}
const bool kShaNi = cpu_has_sha_ni();

// N independent compressions interleaved (multi-buffer SHA-NI): one message's
// sha256rnds2 chain is latency-bound, N independent chains keep the SHA unit busy.
// Same rounds as sha256_block_ni, per state.
template <int N>
__attribute__((target("sha,sse4.1,ssse3"))) void sha256_blocks_ni(uint32_t (*h)[8], const uint8_t* const* p) {
    const __m128i bswap = _mm_set_epi64x(0x0c0d0e0f08090a0bLL, 0x0405060700010203LL);
    __m128i s0[N], s1[N], abef[N], cdgh[N], w[N][4];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const __m128i t = _mm_shuffle_epi32(_mm_loadu_si128(reinterpret_cast<const __m128i*>(h[i])), 0xB1);
        const __m128i u = _mm_shuffle_epi32(_mm_loadu_si128(reinterpret_cast<const __m128i*>(h[i] + 4)), 0x1B);
        s0[i] = _mm_alignr_epi8(t, u, 8);
        s1[i] = _mm_blend_epi16(u, t, 0xF0);
        abef[i] = s0[i];
        cdgh[i] = s1[i];
    }
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        const __m128i kg = _mm_load_si128(reinterpret_cast<const __m128i*>(kShaK + 4 * g));
#pragma unroll
        for (int i = 0; i < N; ++i) {
            __m128i m;
            if (g < 4) {
                m = _mm_shuffle_epi8(_mm_loadu_si128(reinterpret_cast<const __m128i*>(p[i] + 16 * g)), bswap);
            } else {
                m = _mm_sha256msg1_epu32(w[i][g & 3], w[i][(g + 1) & 3]);
                m = _mm_add_epi32(m, _mm_alignr_epi8(w[i][(g + 3) & 3], w[i][(g + 2) & 3], 4));
                m = _mm_sha256msg2_epu32(m, w[i][(g + 3) & 3]);
            }
            w[i][g & 3] = m;
            const __m128i wk = _mm_add_epi32(m, kg);
            s1[i] = _mm_sha256rnds2_epu32(s1[i], s0[i], wk);
            s0[i] = _mm_sha256rnds2_epu32(s0[i], s1[i], _mm_shuffle_epi32(wk, 0x0E));
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const __m128i a = _mm_add_epi32(s0[i], abef[i]);
        const __m128i c = _mm_add_epi32(s1[i], cdgh[i]);
        const __m128i t = _mm_shuffle_epi32(a, 0x1B);  // FEBA
        const __m128i u = _mm_shuffle_epi32(c, 0xB1);  // DCHG
        _mm_storeu_si128(reinterpret_cast<__m128i*>(h[i]), _mm_blend_epi16(t, u, 0xF0));      // DCBA
        _mm_storeu_si128(reinterpret_cast<__m128i*>(h[i] + 4), _mm_alignr_epi8(u, t, 8));     // HGFE
    }
}
#endif

struct Sha256 {
    uint32_t h[8];
    uint8_t buf[64];
    uint64_t len = 0;
    size_t blen = 0;

    static constexpr uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
        0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
        0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
        0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
        0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
        0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
        0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
        0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

    Sha256() {
        static constexpr uint32_t H0[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a,
                                           0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
        memcpy(h, H0, sizeof(h));
    }
    static inline uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
    void block(const uint8_t* p) {
#if defined(__x86_64__)
        if (kShaNi) {
            sha256_block_ni(h, p);
            return;
        }
#endif
        uint32_t w[64];
        for (int i = 0; i < 16; ++i)
            w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
        for (int i = 16; i < 64; ++i) {
            uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
            uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
            w[i] = w[i - 16] + s0 + w[i - 7] + s1;
        }
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
        for (int i = 0; i < 64; ++i) {
            uint32_t S1 = rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25);
            uint32_t ch = (e & f) ^ (~e & g);
            uint32_t t1 = hh + S1 + ch + K[i] + w[i];
            uint32_t S0 = rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22);
            uint32_t mj = (a & b) ^ (a & c) ^ (b & c);
            uint32_t t2 = S0 + mj;
            hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
    }
    void update(const uint8_t* p, size_t n) {
        len += n;
        if (blen) {
            size_t t = 64 - blen < n ? 64 - blen : n;
            memcpy(buf + blen, p, t);
            blen += t; p += t; n -= t;
            if (blen == 64) { block(buf); blen = 0; }
        }
        while (n >= 64) { block(p); p += 64; n -= 64; }
        if (n) { memcpy(buf, p, n); blen = n; }
    }
    void final(uint8_t out[32]) {
        const uint64_t bits = len * 8;
        uint8_t pad[72] = {0x80};  // 0x80, zeros to 56 mod 64, then the bit length
        const size_t zeros = (blen < 56 ? 56 - blen : 120 - blen) - 1;
        for (int i = 0; i < 8; ++i) pad[1 + zeros + i] = (uint8_t)(bits >> (56 - 8 * i));
        update(pad, 1 + zeros + 8);
        for (int i = 0; i < 8; ++i) {
            out[4 * i] = (uint8_t)(h[i] >> 24); out[4 * i + 1] = (uint8_t)(h[i] >> 16);
            out[4 * i + 2] = (uint8_t)(h[i] >> 8); out[4 * i + 3] = (uint8_t)h[i];
        }
    }
};
constexpr uint32_t Sha256::K[64];

struct Digest { uint8_t b[32]; };

Digest node_hash(const Digest& l, const Digest& r) {
    Sha256 s;
    uint8_t pre = 0x01;
    s.update(&pre, 1);
    s.update(l.b, 32);
    s.update(r.b, 32);
    Digest o;
    s.final(o.b);
    return o;
}

// SHA-256 of prefix || msg[i][0, len) for `count` <= kHashBatch messages of one length,
// compressed side by side (sha256_blocks_ni<kHashBatch>; the scalar Sha256 without the
// SHA extensions).  Block b of a message is assembled in a 64-byte buffer: the 1-byte
// prefix shifts the payload off the block grid.  Eight at a time: one DefaultTree root
// of 256 leaves x 512 B on the GPU box's EPYC 9575F takes 55.8 us against 77 at four
// and 121 one message at a time (profiles/r05p_host_tree.txt).
constexpr int kHashBatch = 8;
void hash_prefixed(uint8_t prefix, const uint8_t* const* msg, int count, uint32_t len, Digest* out) {
#if defined(__x86_64__)
    if (kShaNi) {
        const uint64_t total = 1ull + len, bits = total * 8;
        const uint64_t nblk = (total + 8) / 64 + 1;
        uint32_t h[kHashBatch][8];
        static constexpr uint32_t H0[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a,
                                           0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
        for (auto& x : h) memcpy(x, H0, sizeof(H0));
        alignas(16) uint8_t buf[kHashBatch][64];
        const uint8_t* bp[kHashBatch];
        for (int i = 0; i < kHashBatch; ++i) bp[i] = buf[i];
        for (uint64_t b = 0; b < nblk; ++b) {
            const uint64_t t0 = 64 * b;  // message bytes [t0, t0 + 64) of prefix || payload || padding
            for (int i = 0; i < kHashBatch; ++i) {
                const uint8_t* m = msg[i < count ? i : count - 1];
                uint8_t* d = buf[i];
                memset(d, 0, 64);
                // payload byte j sits at message position 1 + j
                const uint64_t lo = t0 > 0 ? t0 - 1 : 0, hi = std::min<uint64_t>(t0 + 63, len);
                if (hi > lo) memcpy(d + (1 + lo - t0), m + lo, hi - lo);
                if (t0 == 0) d[0] = prefix;
                if (total >= t0 && total < t0 + 64) d[total - t0] = 0x80;
                if (b == nblk - 1)
                    for (int q = 0; q < 8; ++q) d[56 + q] = (uint8_t)(bits >> (56 - 8 * q));
            }
            sha256_blocks_ni<kHashBatch>(h, bp);
        }
        for (int i = 0; i < count; ++i)
            for (int q = 0; q < 8; ++q) {
                out[i].b[4 * q] = (uint8_t)(h[i][q] >> 24);
                out[i].b[4 * q + 1] = (uint8_t)(h[i][q] >> 16);
                out[i].b[4 * q + 2] = (uint8_t)(h[i][q] >> 8);
                out[i].b[4 * q + 3] = (uint8_t)h[i][q];
            }
        return;
    }
#endif
    for (int i = 0; i < count; ++i) {
        Sha256 s;
        s.update(&prefix, 1);
        s.update(msg[i], len);
        s.final(out[i].b);
    }
}

// ---- namespaced Merkle tree (celestiaorg/nmt v0.24.3, published algorithm) ----
// A node is minNs || maxNs || digest.  HashLeaf(ndata) = ns || ns || H(0x00 || ndata)
// with ns = ndata[:nsSize]; HashNode(l, r) = l.min || max || H(0x01 || l || r) where
// max = l.max when IgnoreMaxNamespace and r.min is the all-0xFF namespace, else
// r.max; the root over n leaves splits at the largest power of two below n
// (RFC 6962 MTH), i.e. the perfect subtrees of the set bits of n folded from the
// right, as the DefaultTree's stack.  Empty tree: zero namespaces || H("").
// Nodes of a level sit contiguously (2 ns + 32 bytes each), so a pair is already the
// message body 0x01 || l || r; leaves and each level are hashed kHashBatch at a time.
// HashNode's validateSiblingsNamespaceOrder: r.min < l.max is an error.
bool nmt_pair(const uint8_t* l, const uint8_t* r, uint32_t nsz, bool ignore_max, uint8_t* out_ns) {
    const uint8_t *lmin = l, *lmax = l + nsz, *rmin = r, *rmax = r + nsz;
    if (memcmp(lmax, rmin, nsz) > 0) return false;
    bool rmin_is_max = true;
    for (uint32_t i = 0; i < nsz; ++i) rmin_is_max &= rmin[i] == 0xFF;
    memcpy(out_ns, lmin, nsz);
    memcpy(out_ns + nsz, (ignore_max && rmin_is_max) ? lmax : rmax, nsz);
    return true;
}

}  // namespace

extern "C" int rsm_nmt_tree_root(void* user, int /*axis*/, uint32_t index, const uint8_t* const* leaves,
                                 uint32_t n_leaves, uint32_t leaf_size, uint8_t* root_out, uint32_t* root_len) {
    const auto* p = static_cast<const rsm_nmt_params*>(user);
    if (!p || !root_len || !root_out || p->namespace_size == 0 || p->square_size == 0) return RSM_EINVAL;
    const uint32_t nsz = p->namespace_size, k = p->square_size, NB = 2 * nsz + 32;
    const bool ig = p->ignore_max_namespace != 0;
    if (*root_len < NB) return RSM_EINVAL;
    // erasuredNamespacedMerkleTree.Push (nmtwrapper_test.go:94-120)
    if (index + 1 > 2 * k || n_leaves > 2 * k) return RSM_ETREE;  // pushed past predetermined square size
    if (leaf_size < nsz) return RSM_ETREE;                         // data is too short to contain namespace ID
    if (n_leaves == 0) {
        Sha256 s;
        memset(root_out, 0, NB);
        s.final(root_out + 2 * nsz);
        *root_len = NB;
        return RSM_OK;
    }
    std::vector<uint8_t> parity(nsz, 0xFF);
    const size_t ML = (size_t)nsz + leaf_size;  // a leaf's message body: ns || share
    std::vector<uint8_t> msg((size_t)n_leaves * ML), nodes((size_t)n_leaves * NB);
    const uint8_t* prev = nullptr;
    for (uint32_t i = 0; i < n_leaves; ++i) {
        if (!leaves[i]) return RSM_ETREE;
        const uint8_t* ns = (i < k && index < k) ? leaves[i] : parity.data();  // isQuadrantZero
        if (prev && memcmp(ns, prev, nsz) < 0) return RSM_ETREE;           // nmt: ErrInvalidPushOrder
        prev = ns;
        memcpy(&msg[i * ML], ns, nsz);
        memcpy(&msg[i * ML + nsz], leaves[i], leaf_size);
        memcpy(&nodes[(size_t)i * NB], ns, nsz);
        memcpy(&nodes[(size_t)i * NB + nsz], ns, nsz);
    }
    std::vector<Digest> dg(kHashBatch);
    std::vector<uint8_t> nsb((size_t)kHashBatch * 2 * nsz);  // the pairs' new min || max
    for (uint32_t i = 0; i < n_leaves; i += kHashBatch) {
        const int c = (int)std::min<uint32_t>(kHashBatch, n_leaves - i);
        const uint8_t* m[kHashBatch];
        for (int q = 0; q < c; ++q) m[q] = &msg[(size_t)(i + q) * ML];
        hash_prefixed(0x00, m, c, (uint32_t)ML, dg.data());
        for (int q = 0; q < c; ++q) memcpy(&nodes[(size_t)(i + q) * NB + 2 * nsz], dg[q].b, 32);
    }
    std::vector<uint32_t> subs;  // first leaf of each perfect subtree, largest first
    for (uint32_t s0 = 0, bit = 31; s0 < n_leaves; --bit) {
        const uint32_t size = 1u << bit;
        if (!(n_leaves & size)) continue;
        for (uint32_t cnt = size; cnt > 1; cnt /= 2) {  // level by level, in place from node s0
            const uint32_t np = cnt / 2;
            for (uint32_t j = 0; j < np; j += kHashBatch) {
                const int c = (int)std::min<uint32_t>(kHashBatch, np - j);
                const uint8_t* m[kHashBatch];
                for (int q = 0; q < c; ++q) {
                    const uint8_t* l = &nodes[(size_t)(s0 + 2 * (j + q)) * NB];
                    if (!nmt_pair(l, l + NB, nsz, ig, &nsb[(size_t)q * 2 * nsz])) return RSM_ETREE;
                    m[q] = l;
                }
                hash_prefixed(0x01, m, c, 2 * NB, dg.data());  // every pair read before any write
                for (int q = 0; q < c; ++q) {
                    uint8_t* o = &nodes[(size_t)(s0 + j + q) * NB];
                    memcpy(o, &nsb[(size_t)q * 2 * nsz], 2 * nsz);
                    memcpy(o + 2 * nsz, dg[q].b, 32);
                }
            }
        }
        subs.push_back(s0);
        s0 += size;
    }
    std::vector<uint8_t> acc(&nodes[(size_t)subs.back() * NB], &nodes[(size_t)subs.back() * NB] + NB);
    std::vector<uint8_t> pair(2 * NB);
    for (int i = (int)subs.size() - 2; i >= 0; --i) {
        memcpy(pair.data(), &nodes[(size_t)subs[i] * NB], NB);
        memcpy(pair.data() + NB, acc.data(), NB);
        if (!nmt_pair(pair.data(), pair.data() + NB, nsz, ig, acc.data())) return RSM_ETREE;
        const uint8_t* m[1] = {pair.data()};
        hash_prefixed(0x01, m, 1, 2 * NB, dg.data());
        memcpy(acc.data() + 2 * nsz, dg[0].b, 32);
    }
    memcpy(root_out, acc.data(), NB);
    *root_len = NB;
    return RSM_OK;
}

extern "C" int rsm_default_tree_root(void* /*user*/, int /*axis*/, uint32_t /*index*/,
                                     const uint8_t* const* leaves, uint32_t n_leaves, uint32_t leaf_size,
                                     uint8_t* root_out, uint32_t* root_len) {
    if (!root_len || *root_len < 32 || !root_out) return RSM_EINVAL;
    if (n_leaves == 0) {  // merkletree.Root() of an empty tree is nil
        *root_len = 0;
        return RSM_OK;
    }
    for (uint32_t i = 0; i < n_leaves; ++i)
        if (!leaves[i]) return RSM_ETREE;
    // The push/join stack ends as the perfect subtrees of the set bits of n (largest
    // first) folded from the newest: root = node(sub_0, node(sub_1, ... sub_last)).
    // Leaves, then each subtree's levels, are hashed kHashBatch messages at a time.
    std::vector<Digest> d(n_leaves);
    for (uint32_t i = 0; i < n_leaves; i += kHashBatch)
        hash_prefixed(0x00, leaves + i, (int)std::min<uint32_t>(kHashBatch, n_leaves - i), leaf_size, &d[i]);
    std::vector<Digest> subs;
    std::vector<uint8_t> pairs;
    for (uint32_t s0 = 0, bit = 31; s0 < n_leaves; --bit) {
        const uint32_t size = 1u << bit;
        if (!(n_leaves & size)) continue;
        for (uint32_t cnt = size; cnt > 1; cnt /= 2) {  // level by level, in place in d[s0 ..)
            const uint32_t np = cnt / 2;
            pairs.resize((size_t)np * 64);
            for (uint32_t j = 0; j < np; ++j) {
                memcpy(&pairs[(size_t)j * 64], d[s0 + 2 * j].b, 32);
                memcpy(&pairs[(size_t)j * 64 + 32], d[s0 + 2 * j + 1].b, 32);
            }
            for (uint32_t j = 0; j < np; j += kHashBatch) {
                const uint8_t* m[kHashBatch];
                const int c = (int)std::min<uint32_t>(kHashBatch, np - j);
                for (int q = 0; q < c; ++q) m[q] = &pairs[(size_t)(j + q) * 64];
                hash_prefixed(0x01, m, c, 64, &d[s0 + j]);
            }
        }
        subs.push_back(d[s0]);
        s0 += size;
    }
    Digest acc = subs.back();
    for (int i = (int)subs.size() - 2; i >= 0; --i) acc = node_hash(subs[i], acc);
    memcpy(root_out, acc.b, 32);
    *root_len = 32;
    return RSM_OK;
}

// ---- share inclusion proofs (include/rsmt2d_hip.h "share inclusion proofs") ----
// Host restatements of the device node store + gather (kernels_proof.hip): the same
// trees built level by level -- node (l, j) over leaves [j 2^l, min((j+1) 2^l, n)), an
// unpaired last node carried up unchanged, which is the stack of perfect subtrees
// above folded from the right -- keeping, at each level, the sibling of the node above
// leaf `pos` where there is one.
namespace {

uint32_t proof_levels_of(uint32_t n) {  // ceil(log2 n)
    uint32_t l = 0;
    while ((1ull << l) < n) ++l;
    return l;
}

// Walks the levels of a tree whose level-0 nodes are `lvl` (NB bytes each): `join`
// hashes pair j of a level into `out` (false: tree error).  Fills the record; leaves
// the root in lvl[0 .. NB).
template <typename Join>
bool prove_levels(std::vector<uint8_t>& lvl, uint32_t n, uint32_t NB, uint32_t pos, uint8_t* rec, Join&& join) {
    const uint32_t L = proof_levels_of(n);
    memset(rec, 0, 8 + (size_t)L * NB);
    uint32_t n_nodes = 0, mask = 0, cnt = n;
    std::vector<uint8_t> nxt;
    for (uint32_t l = 0; l < L; ++l) {
        const uint32_t j = pos >> l, sib = j ^ 1u;
        if (sib < cnt) {
            memcpy(rec + 8 + (size_t)n_nodes * NB, &lvl[(size_t)sib * NB], NB);
            if (!(j & 1u)) mask |= 1u << n_nodes;  // the sibling is the right operand
            ++n_nodes;
        }
        const uint32_t np = cnt / 2, up = (cnt + 1) / 2;
        nxt.assign((size_t)up * NB, 0);
        if (!join(lvl.data(), np, nxt.data())) return false;
        if (cnt & 1u) memcpy(&nxt[(size_t)np * NB], &lvl[(size_t)(cnt - 1) * NB], NB);
        lvl.swap(nxt);
        cnt = up;
    }
    for (int b = 0; b < 4; ++b) {
        rec[b] = (uint8_t)(n_nodes >> (8 * b));
        rec[4 + b] = (uint8_t)(mask >> (8 * b));
    }
    return true;
}

}  // namespace

extern "C" int rsm_default_tree_prove(const uint8_t* const* leaves, uint32_t n_leaves, uint32_t leaf_size, uint32_t pos,
                                      uint8_t* record_out, uint8_t* root_out) {
    if (!leaves || !record_out || n_leaves == 0 || pos >= n_leaves) return RSM_EINVAL;
    for (uint32_t i = 0; i < n_leaves; ++i)
        if (!leaves[i]) return RSM_ETREE;
    std::vector<uint8_t> lvl((size_t)n_leaves * 32);
    Digest dg[kHashBatch];
    for (uint32_t i = 0; i < n_leaves; i += kHashBatch) {
        const int c = (int)std::min<uint32_t>(kHashBatch, n_leaves - i);
        hash_prefixed(0x00, leaves + i, c, leaf_size, dg);
        for (int q = 0; q < c; ++q) memcpy(&lvl[(size_t)(i + q) * 32], dg[q].b, 32);
    }
    auto join = [&](const uint8_t* cur, uint32_t np, uint8_t* out) {
        for (uint32_t j = 0; j < np; j += kHashBatch) {  // a pair is already the message body l || r
            const int c = (int)std::min<uint32_t>(kHashBatch, np - j);
            const uint8_t* m[kHashBatch];
            for (int q = 0; q < c; ++q) m[q] = cur + (size_t)(j + q) * 64;
            hash_prefixed(0x01, m, c, 64, dg);
            for (int q = 0; q < c; ++q) memcpy(out + (size_t)(j + q) * 32, dg[q].b, 32);
        }
        return true;
    };
    prove_levels(lvl, n_leaves, 32, pos, record_out, join);
    if (root_out) memcpy(root_out, lvl.data(), 32);
    return RSM_OK;
}

namespace {

// Level 0 of the erasured NMT over `leaves` (erasuredNamespacedMerkleTree.Push, as
// rsm_nmt_tree_root): n_leaves nodes ns || ns || H(0x00 || ns || share) in `lvl`.
int nmt_leaf_level(const rsm_nmt_params* p, uint32_t index, const uint8_t* const* leaves, uint32_t n_leaves,
                   uint32_t leaf_size, std::vector<uint8_t>& lvl) {
    const uint32_t nsz = p->namespace_size, k = p->square_size, NB = 2 * nsz + 32;
    if (index + 1 > 2 * k || n_leaves > 2 * k) return RSM_ETREE;
    if (leaf_size < nsz) return RSM_ETREE;
    std::vector<uint8_t> parity(nsz, 0xFF);
    const size_t ML = (size_t)nsz + leaf_size;
    std::vector<uint8_t> msg((size_t)n_leaves * ML);
    lvl.assign((size_t)n_leaves * NB, 0);
    const uint8_t* prev = nullptr;
    for (uint32_t i = 0; i < n_leaves; ++i) {
        if (!leaves[i]) return RSM_ETREE;
        const uint8_t* ns = (i < k && index < k) ? leaves[i] : parity.data();
        if (prev && memcmp(ns, prev, nsz) < 0) return RSM_ETREE;
        prev = ns;
        memcpy(&msg[i * ML], ns, nsz);
        memcpy(&msg[i * ML + nsz], leaves[i], leaf_size);
        memcpy(&lvl[(size_t)i * NB], ns, nsz);
        memcpy(&lvl[(size_t)i * NB + nsz], ns, nsz);
    }
    Digest dg[kHashBatch];
    for (uint32_t i = 0; i < n_leaves; i += kHashBatch) {
        const int c = (int)std::min<uint32_t>(kHashBatch, n_leaves - i);
        const uint8_t* m[kHashBatch];
        for (int q = 0; q < c; ++q) m[q] = &msg[(size_t)(i + q) * ML];
        hash_prefixed(0x00, m, c, (uint32_t)ML, dg);
        for (int q = 0; q < c; ++q) memcpy(&lvl[(size_t)(i + q) * NB + 2 * nsz], dg[q].b, 32);
    }
    return RSM_OK;
}

// HashNode of pairs 0 .. np-1 of the level `cur` into `out`; false: unordered siblings
bool nmt_join_pairs(const uint8_t* cur, uint32_t np, uint8_t* out, uint32_t nsz, bool ig) {
    const uint32_t NB = 2 * nsz + 32;
    Digest dg[kHashBatch];
    for (uint32_t j = 0; j < np; j += kHashBatch) {
        const int c = (int)std::min<uint32_t>(kHashBatch, np - j);
        const uint8_t* m[kHashBatch];
        for (int q = 0; q < c; ++q) {
            const uint8_t* l = cur + (size_t)(2 * (j + q)) * NB;
            if (!nmt_pair(l, l + NB, nsz, ig, out + (size_t)(j + q) * NB)) return false;
            m[q] = l;
        }
        hash_prefixed(0x01, m, c, 2 * NB, dg);
        for (int q = 0; q < c; ++q) memcpy(out + (size_t)(j + q) * NB + 2 * nsz, dg[q].b, 32);
    }
    return true;
}

}  // namespace

extern "C" int rsm_nmt_tree_prove(const rsm_nmt_params* p, uint32_t index, const uint8_t* const* leaves,
                                  uint32_t n_leaves, uint32_t leaf_size, uint32_t pos, uint8_t* record_out,
                                  uint8_t* root_out) {
    if (!p || !leaves || !record_out || p->namespace_size == 0 || p->square_size == 0 || n_leaves == 0 ||
        pos >= n_leaves)
        return RSM_EINVAL;
    const uint32_t nsz = p->namespace_size, NB = 2 * nsz + 32;
    const bool ig = p->ignore_max_namespace != 0;
    std::vector<uint8_t> lvl;
    if (int rc = nmt_leaf_level(p, index, leaves, n_leaves, leaf_size, lvl)) return rc;
    auto join = [&](const uint8_t* cur, uint32_t np, uint8_t* out) { return nmt_join_pairs(cur, np, out, nsz, ig); };
    if (!prove_levels(lvl, n_leaves, NB, pos, record_out, join)) return RSM_ETREE;
    if (root_out) memcpy(root_out, lvl.data(), NB);
    return RSM_OK;
}

// ---- proof verification (include/rsmt2d_hip.h "proof verification") ----
// Host restatements of the device verifiers (kernels_sha.hip proof_verify_kernel,
// kernels_nmt.hip nmt_proof_verify_kernel): node count and operand sides are derived
// from (n_leaves, pos) and only compared with the record's header; the fold then runs
// over the derived count and reads nothing past those nodes.
namespace {

// nodes of the proof of leaf `pos` among n leaves; *mask: bit i set where node i is the
// right operand
uint32_t proof_shape(uint32_t n, uint32_t pos, uint32_t* mask) {
    const uint32_t L = proof_levels_of(n);
    uint32_t n_nodes = 0, m = 0;
    for (uint32_t l = 0; l < L; ++l) {
        const uint64_t j = pos >> l, cnt = ((uint64_t)n + (1ull << l) - 1) >> l;
        if ((j ^ 1u) < cnt) {
            if (!(j & 1u)) m |= 1u << n_nodes;
            ++n_nodes;
        }
    }
    *mask = m;
    return n_nodes;
}

bool header_matches(const uint8_t* rec, uint32_t n_nodes, uint32_t mask) {
    uint32_t a = 0, b = 0;
    for (int i = 0; i < 4; ++i) {
        a |= (uint32_t)rec[i] << (8 * i);
        b |= (uint32_t)rec[4 + i] << (8 * i);
    }
    return a == n_nodes && b == mask;
}

}  // namespace

namespace {

// SHA256(0x00 || msg): a leaf of the DefaultTree and of the data-root tree
Digest leaf_hash(const uint8_t* msg, size_t len) {
    Sha256 s;
    const uint8_t pre = 0x00;
    s.update(&pre, 1);
    s.update(msg, len);
    Digest o;
    s.final(o.b);
    return o;
}

// acc folded through n_nodes 32-byte siblings, bottom-up (bit i of mask: sibling i is the
// right operand)
void fold_digests(Digest& acc, const uint8_t* nodes, uint32_t n_nodes, uint32_t mask) {
    for (uint32_t i = 0; i < n_nodes; ++i) {
        Digest nd;
        memcpy(nd.b, nodes + (size_t)i * 32, 32);
        acc = (mask >> i) & 1u ? node_hash(acc, nd) : node_hash(nd, acc);
    }
}

// The NMT leaf node of `share` (quadrant 0: its own namespace, else 0xFF..) folded through
// n_nodes siblings of 2 ns + 32 bytes into acc; false on unordered siblings.
bool nmt_fold(const rsm_nmt_params* p, bool q0, const uint8_t* share, uint32_t share_size, const uint8_t* nodes,
              uint32_t n_nodes, uint32_t mask, std::vector<uint8_t>& acc) {
    const uint32_t nsz = p->namespace_size, NB = 2 * nsz + 32;
    const bool ig = p->ignore_max_namespace != 0;
    std::vector<uint8_t> pair(2 * (size_t)NB), ns(nsz, 0xFF);
    acc.assign(NB, 0);
    if (q0) memcpy(ns.data(), share, nsz);
    memcpy(acc.data(), ns.data(), nsz);
    memcpy(acc.data() + nsz, ns.data(), nsz);
    {
        Sha256 s;
        const uint8_t pre = 0x00;
        s.update(&pre, 1);
        s.update(ns.data(), nsz);
        s.update(share, share_size);
        s.final(acc.data() + 2 * nsz);
    }
    for (uint32_t i = 0; i < n_nodes; ++i) {
        const uint8_t* nd = nodes + (size_t)i * NB;
        const bool right = (mask >> i) & 1u;
        memcpy(pair.data(), right ? acc.data() : nd, NB);
        memcpy(pair.data() + NB, right ? nd : acc.data(), NB);
        if (!nmt_pair(pair.data(), pair.data() + NB, nsz, ig, acc.data())) return false;
        Sha256 s;
        const uint8_t pre = 0x01;
        s.update(&pre, 1);
        s.update(pair.data(), 2 * (size_t)NB);
        s.final(acc.data() + 2 * nsz);
    }
    return true;
}

}  // namespace

extern "C" int rsm_default_tree_verify(const uint8_t* share, uint32_t share_size, uint32_t n_leaves, uint32_t pos,
                                       const uint8_t* record, const uint8_t* root, uint32_t* status) {
    if ((!share && share_size) || !record || !root || !status || n_leaves == 0 || pos >= n_leaves) return RSM_EINVAL;
    uint32_t mask = 0;
    const uint32_t n_nodes = proof_shape(n_leaves, pos, &mask);
    if (!header_matches(record, n_nodes, mask)) {
        *status = RSM_PROOF_MALFORMED;
        return RSM_OK;
    }
    Digest acc = leaf_hash(share, share_size);
    fold_digests(acc, record + 8, n_nodes, mask);
    *status = memcmp(acc.b, root, 32) == 0 ? RSM_PROOF_OK : RSM_PROOF_ROOT;
    return RSM_OK;
}

extern "C" int rsm_nmt_tree_verify(const rsm_nmt_params* p, uint32_t index, const uint8_t* share, uint32_t share_size,
                                   uint32_t n_leaves, uint32_t pos, const uint8_t* record, const uint8_t* root,
                                   uint32_t* status) {
    if (!p || !share || !record || !root || !status || p->namespace_size == 0 || p->square_size == 0 || n_leaves == 0 ||
        pos >= n_leaves)
        return RSM_EINVAL;
    const uint32_t nsz = p->namespace_size, k = p->square_size, NB = 2 * nsz + 32;
    if (share_size < nsz) return RSM_ETREE;  // data is too short to contain namespace ID
    uint32_t mask = 0;
    const uint32_t n_nodes = proof_shape(n_leaves, pos, &mask);
    if (!header_matches(record, n_nodes, mask)) {
        *status = RSM_PROOF_MALFORMED;
        return RSM_OK;
    }
    std::vector<uint8_t> acc;
    if (!nmt_fold(p, index < k && pos < k, share, share_size, record + 8, n_nodes, mask, acc)) {
        *status = RSM_PROOF_ORDER;
        return RSM_OK;
    }
    *status = memcmp(acc.data(), root, NB) == 0 ? RSM_PROOF_OK : RSM_PROOF_ROOT;
    return RSM_OK;
}

// ---- data root (include/rsmt2d_hip.h "data root") ----
// Host restatements of kernels_dataroot.hip and the chained verify kernels: the level
// picture over the 2 * width roots, 32-byte digests at every level.
namespace {

// level 0 of the data-root tree: the leaf digests of the 2 * width roots
std::vector<uint8_t> data_root_leaves(const uint8_t* roots, uint32_t width, uint32_t root_len) {
    std::vector<uint8_t> lvl((size_t)2 * width * 32);
    for (uint32_t t = 0; t < 2 * width; ++t) {
        const Digest d = leaf_hash(roots + (size_t)t * root_len, root_len);
        memcpy(&lvl[(size_t)t * 32], d.b, 32);
    }
    return lvl;
}

bool digest_join_pairs(const uint8_t* cur, uint32_t np, uint8_t* out) {
    Digest dg[kHashBatch];
    for (uint32_t j = 0; j < np; j += kHashBatch) {  // a pair is already the message body l || r
        const int c = (int)std::min<uint32_t>(kHashBatch, np - j);
        const uint8_t* m[kHashBatch];
        for (int q = 0; q < c; ++q) m[q] = cur + (size_t)(j + q) * 64;
        hash_prefixed(0x01, m, c, 64, dg);
        for (int q = 0; q < c; ++q) memcpy(out + (size_t)(j + q) * 32, dg[q].b, 32);
    }
    return true;
}

bool data_root_args(const uint8_t* roots, uint32_t width, uint32_t root_len) {
    return roots && width >= 1 && width <= (1u << 30) && root_len >= 1 && root_len <= 96;
}

}  // namespace

extern "C" int rsm_data_root_prove(const uint8_t* roots, uint32_t width, uint32_t root_len, uint32_t axis, uint32_t index,
                                   uint8_t* record_out) {
    if (!data_root_args(roots, width, root_len) || !record_out || axis > 1 || index >= width) return RSM_EINVAL;
    std::vector<uint8_t> lvl = data_root_leaves(roots, width, root_len);
    prove_levels(lvl, 2 * width, 32, axis * width + index, record_out, digest_join_pairs);
    return RSM_OK;
}

extern "C" int rsm_data_root(const uint8_t* roots, uint32_t width, uint32_t root_len, uint8_t* out) {
    if (!data_root_args(roots, width, root_len) || !out) return RSM_EINVAL;
    std::vector<uint8_t> lvl = data_root_leaves(roots, width, root_len);
    std::vector<uint8_t> rec(8 + (size_t)proof_levels_of(2 * width) * 32);
    prove_levels(lvl, 2 * width, 32, 0, rec.data(), digest_join_pairs);
    memcpy(out, lvl.data(), 32);
    return RSM_OK;
}

extern "C" int rsm_data_root_verify(const uint8_t* root_bytes, uint32_t root_len, uint32_t width, uint32_t axis,
                                    uint32_t index, const uint8_t* record, const uint8_t* data_root, uint32_t* status) {
    if (!data_root_args(root_bytes, width, root_len) || !record || !data_root || !status || axis > 1 || index >= width)
        return RSM_EINVAL;
    uint32_t mask = 0;
    const uint32_t n_nodes = proof_shape(2 * width, axis * width + index, &mask);
    if (!header_matches(record, n_nodes, mask)) {
        *status = RSM_PROOF_MALFORMED;
        return RSM_OK;
    }
    Digest acc = leaf_hash(root_bytes, root_len);
    fold_digests(acc, record + 8, n_nodes, mask);
    *status = memcmp(acc.b, data_root, 32) == 0 ? RSM_PROOF_OK : RSM_PROOF_ROOT;
    return RSM_OK;
}

extern "C" int rsm_sample_verify_data_root(const rsm_nmt_params* nmt, uint32_t width, const rsm_sample* sm,
                                           const uint8_t* share, uint32_t share_size, const uint8_t* record,
                                           const uint8_t* root_record, const uint8_t* data_root, uint32_t* status) {
    if (!sm || !share || !record || !root_record || !data_root || !status || width == 0 || width > (1u << 30) ||
        sm->axis > 1 || sm->index >= width || sm->pos >= width)
        return RSM_EINVAL;
    if (nmt && (nmt->namespace_size == 0 || nmt->namespace_size > 32 || nmt->square_size == 0)) return RSM_EINVAL;
    if (nmt && share_size < nmt->namespace_size) return RSM_ETREE;  // data is too short to contain namespace ID
    uint32_t mask = 0, mask2 = 0;
    const uint32_t n_nodes = proof_shape(width, sm->pos, &mask);
    const uint32_t n2 = proof_shape(2 * width, sm->axis * width + sm->index, &mask2);
    if (!header_matches(record, n_nodes, mask) || !header_matches(root_record, n2, mask2)) {
        *status = RSM_PROOF_MALFORMED;
        return RSM_OK;
    }
    Digest acc;
    if (nmt) {
        std::vector<uint8_t> cand;
        const uint32_t k = nmt->square_size;
        if (!nmt_fold(nmt, sm->index < k && sm->pos < k, share, share_size, record + 8, n_nodes, mask, cand)) {
            *status = RSM_PROOF_ORDER;
            return RSM_OK;
        }
        acc = leaf_hash(cand.data(), cand.size());
    } else {
        Digest cand = leaf_hash(share, share_size);
        fold_digests(cand, record + 8, n_nodes, mask);
        acc = leaf_hash(cand.b, 32);
    }
    fold_digests(acc, root_record + 8, n2, mask2);
    *status = memcmp(acc.b, data_root, 32) == 0 ? RSM_PROOF_OK : RSM_PROOF_ROOT;
    return RSM_OK;
}

// ---- namespace proofs (include/rsmt2d_hip.h "namespace proofs") ----
// Host restatements of kernels_nsproof.hip: the same range [start, end) and the same
// range-proof nodes, by levels, out of a tree built here instead of a node store; and
// the verifier, which derives counts and operand sides from (n_leaves, start, end).
namespace {

struct RangeNode {
    uint32_t level, j;
};

// The range proof's nodes of [start, end) of n leaves in record order: the left nodes
// from the top level down, then the right nodes from the bottom level up.
std::vector<RangeNode> range_nodes(uint32_t n, uint32_t start, uint32_t end, uint32_t* n_left) {
    std::vector<RangeNode> left, right;
    uint32_t a = start, last = end - 1;
    for (uint32_t l = 0, L = proof_levels_of(n); l < L; ++l) {
        const uint32_t cnt = (uint32_t)(((uint64_t)n + (1ull << l) - 1) >> l);
        if (a & 1u) left.push_back({l, a - 1});
        if (!(last & 1u) && last + 1 < cnt) right.push_back({l, last + 1});
        a >>= 1;
        last >>= 1;
    }
    *n_left = (uint32_t)left.size();
    std::vector<RangeNode> out(left.rbegin(), left.rend());
    out.insert(out.end(), right.begin(), right.end());
    return out;
}

void put_le32(uint8_t* p, uint32_t v) {
    for (int b = 0; b < 4; ++b) p[b] = (uint8_t)(v >> (8 * b));
}
uint32_t get_le32(const uint8_t* p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// Every level of the tree over the n level-0 nodes in lv[0] (NB bytes each) into lv[1 .. L];
// `join` as prove_levels takes it (false: tree error).
template <typename Join>
bool build_levels(std::vector<std::vector<uint8_t>>& lv, uint32_t n, uint32_t NB, Join&& join) {
    for (uint32_t l = 0, cnt = n; l + 1 < lv.size(); ++l) {
        const uint32_t np = cnt / 2, up = (cnt + 1) / 2;
        lv[l + 1].assign((size_t)up * NB, 0);
        if (!join(lv[l].data(), np, lv[l + 1].data())) return false;
        if (cnt & 1u) memcpy(&lv[l + 1][(size_t)np * NB], &lv[l][(size_t)(cnt - 1) * NB], NB);
        cnt = up;
    }
    return true;
}

// Header (kind | start | end | n_nodes) and range-proof nodes of [start, end) out of the
// levels lv of a tree of n leaves; the caller zeroed the record.
void put_range_record(uint8_t* rec, uint32_t kind, const std::vector<std::vector<uint8_t>>& lv, uint32_t n, uint32_t NB,
                      uint32_t start, uint32_t end) {
    uint32_t n_left;
    const std::vector<RangeNode> nodes = range_nodes(n, start, end, &n_left);
    put_le32(rec, kind);
    put_le32(rec + 4, start);
    put_le32(rec + 8, end);
    put_le32(rec + 12, (uint32_t)nodes.size());
    for (size_t i = 0; i < nodes.size(); ++i) memcpy(rec + 16 + i * NB, &lv[nodes[i].level][(size_t)nodes[i].j * NB], NB);
}

// The fold of a range proof, level by level: cur holds the range's nodes a .. last of a
// level (level 0: leaves start .. end - 1), the proof's left node goes in front when a is
// odd, its right node behind when last is even and not the level's last node; an unpaired
// last node is carried up.  join(l, out): the parent of the adjacent nodes l, l + NB
// (false: unordered siblings).  Leaves the root in cur; false on a failed join.
template <typename Join>
bool fold_range(std::vector<uint8_t>& cur, uint32_t n_leaves, uint32_t NB, uint32_t start, uint32_t end, uint32_t n_left,
                const uint8_t* record, Join&& join) {
    uint32_t a = start, last = end - 1, li = n_left, ri = n_left;  // next left node: li - 1; next right: ri
    std::vector<uint8_t> row, nxt;
    for (uint32_t l = 0, L = proof_levels_of(n_leaves); l < L; ++l) {
        const uint32_t cnt = (uint32_t)(((uint64_t)n_leaves + (1ull << l) - 1) >> l);
        row.clear();
        if (a & 1u) {
            const uint8_t* nd = record + 16 + (size_t)(--li) * NB;
            row.insert(row.end(), nd, nd + NB);
            --a;
        }
        row.insert(row.end(), cur.begin(), cur.end());
        if (!(last & 1u) && last + 1 < cnt) {
            const uint8_t* nd = record + 16 + (size_t)(ri++) * NB;
            row.insert(row.end(), nd, nd + NB);
            ++last;
        }
        const uint32_t have = last - a + 1, np = have / 2;  // a is even; an odd count ends in the carried node
        nxt.assign((size_t)(np + (have & 1u)) * NB, 0);
        for (uint32_t j = 0; j < np; ++j)
            if (!join(&row[(size_t)2 * j * NB], &nxt[(size_t)j * NB])) return false;
        if (have & 1u) memcpy(&nxt[(size_t)np * NB], &row[(size_t)(have - 1) * NB], NB);
        cur.swap(nxt);
        a >>= 1;
        last >>= 1;
    }
    return true;
}

// HashNode of the adjacent NMT nodes l, l + NB into out; false: unordered siblings
bool nmt_join(const uint8_t* l, uint8_t* out, uint32_t nsz, bool ig) {
    const uint32_t NB = 2 * nsz + 32;
    if (!nmt_pair(l, l + NB, nsz, ig, out)) return false;
    Sha256 s;
    const uint8_t pre = 0x01;
    s.update(&pre, 1);
    s.update(l, 2 * (size_t)NB);
    s.final(out + 2 * nsz);
    return true;
}

// the wrapper's NMT leaf node of leaf p of vector `index`: ns || ns || H(0x00 || ns || share)
void nmt_leaf_node(const rsm_nmt_params* p, uint32_t index, uint32_t pos, const uint8_t* share, uint32_t share_size,
                   uint8_t* out) {
    const uint32_t nsz = p->namespace_size, k = p->square_size;
    if (index < k && pos < k) memcpy(out, share, nsz);  // quadrant 0
    else memset(out, 0xFF, nsz);
    memcpy(out + nsz, out, nsz);
    Sha256 s;
    const uint8_t pre = 0x00;
    s.update(&pre, 1);
    s.update(out, nsz);
    s.update(share, share_size);
    s.final(out + 2 * nsz);
}

}  // namespace

extern "C" uint32_t rsm_ns_record_bytes(uint32_t width, const rsm_nmt_params* nmt) {
    if (width == 0 || !nmt || nmt->namespace_size == 0) return 0;
    return 16 + (2 * proof_levels_of(width) + 1) * (2 * nmt->namespace_size + 32);
}

extern "C" int rsm_nmt_namespace_prove(const rsm_nmt_params* p, uint32_t index, const uint8_t* const* leaves,
                                       uint32_t n_leaves, uint32_t leaf_size, const uint8_t* nid, uint8_t* record_out,
                                       uint8_t* root_out) {
    if (!p || !leaves || !nid || !record_out || p->namespace_size == 0 || p->square_size == 0 || n_leaves == 0)
        return RSM_EINVAL;
    const uint32_t nsz = p->namespace_size, NB = 2 * nsz + 32, L = proof_levels_of(n_leaves);
    const bool ig = p->ignore_max_namespace != 0;
    std::vector<std::vector<uint8_t>> lv(L + 1);  // every level of the tree
    if (int rc = nmt_leaf_level(p, index, leaves, n_leaves, leaf_size, lv[0])) return rc;
    auto join = [&](const uint8_t* cur, uint32_t np, uint8_t* out) { return nmt_join_pairs(cur, np, out, nsz, ig); };
    if (!build_levels(lv, n_leaves, NB, join)) return RSM_ETREE;
    const uint8_t* root = lv[L].data();
    if (root_out) memcpy(root_out, root, NB);
    memset(record_out, 0, rsm_ns_record_bytes(n_leaves, p));
    if (memcmp(nid, root, nsz) < 0 || memcmp(nid, root + nsz, nsz) > 0) return RSM_OK;  // RSM_NS_EMPTY: all zeros
    uint32_t start = 0, end;
    while (start < n_leaves && memcmp(&lv[0][(size_t)start * NB], nid, nsz) < 0) ++start;
    for (end = start; end < n_leaves && memcmp(&lv[0][(size_t)end * NB], nid, nsz) == 0;) ++end;
    if (start >= n_leaves) return RSM_OK;  // unreachable on a tree that passed: root.max is a leaf's
    const bool absent = start == end;
    if (absent) {
        end = start + 1;
        memcpy(record_out + 16 + (size_t)2 * L * NB, &lv[0][(size_t)start * NB], NB);
    }
    put_range_record(record_out, absent ? RSM_NS_ABSENCE : RSM_NS_INCLUSION, lv, n_leaves, NB, start, end);
    return RSM_OK;
}

extern "C" int rsm_nmt_namespace_verify(const rsm_nmt_params* p, uint32_t index, const uint8_t* nid,
                                        const uint8_t* shares, uint32_t n_shares, uint32_t share_size,
                                        uint32_t n_leaves, const uint8_t* record, const uint8_t* root,
                                        uint32_t* status) {
    if (!p || !nid || !record || !root || !status || (n_shares && !shares) || p->namespace_size == 0 ||
        p->square_size == 0 || n_leaves == 0)
        return RSM_EINVAL;
    const uint32_t nsz = p->namespace_size, NB = 2 * nsz + 32, L = proof_levels_of(n_leaves);
    const bool ig = p->ignore_max_namespace != 0;
    if (n_shares && share_size < nsz) return RSM_ETREE;  // data is too short to contain namespace ID
    const uint32_t kind = get_le32(record), start = get_le32(record + 4), end = get_le32(record + 8),
                   n_nodes = get_le32(record + 12);
    auto done = [&](uint32_t s) {
        *status = s;
        return RSM_OK;
    };
    // 1. the header against what (n_leaves, start, end) dictates
    if (kind == RSM_NS_EMPTY) {
        if (start || end || n_nodes || n_shares) return done(RSM_PROOF_MALFORMED);
        const bool covered = memcmp(root, nid, nsz) <= 0 && memcmp(nid, root + nsz, nsz) <= 0;
        return done(covered ? RSM_PROOF_INCOMPLETE : RSM_PROOF_OK);
    }
    if (kind == RSM_NS_INCLUSION) {
        if (!(start < end && end <= n_leaves) || n_shares != end - start) return done(RSM_PROOF_MALFORMED);
    } else if (kind == RSM_NS_ABSENCE) {
        if (start >= n_leaves || end != start + 1 || n_shares != 0) return done(RSM_PROOF_MALFORMED);
    } else {
        return done(RSM_PROOF_MALFORMED);
    }
    uint32_t n_left;
    const std::vector<RangeNode> shape = range_nodes(n_leaves, start, end, &n_left);
    if (n_nodes != shape.size()) return done(RSM_PROOF_MALFORMED);
    // 2. the leaves carry nid / the absence leaf is one leaf above nid
    std::vector<uint8_t> cur((size_t)(end - start) * NB);
    if (kind == RSM_NS_INCLUSION) {
        for (uint32_t i = 0; i < n_shares; ++i) {
            uint8_t* o = &cur[(size_t)i * NB];
            nmt_leaf_node(p, index, start + i, shares + (size_t)i * share_size, share_size, o);
            if (memcmp(o, nid, nsz) != 0) return done(RSM_PROOF_NAMESPACE);
        }
    } else {
        const uint8_t* leaf = record + 16 + (size_t)2 * L * NB;
        if (memcmp(leaf, leaf + nsz, nsz) != 0 || memcmp(leaf, nid, nsz) <= 0) return done(RSM_PROOF_NAMESPACE);
        memcpy(cur.data(), leaf, NB);
    }
    // 3. nothing of nid lies under a proof node
    for (uint32_t i = 0; i < n_nodes; ++i) {
        const uint8_t* nd = record + 16 + (size_t)i * NB;
        if (i < n_left ? memcmp(nd + nsz, nid, nsz) >= 0 : memcmp(nd, nid, nsz) <= 0) return done(RSM_PROOF_INCOMPLETE);
    }
    // 4, 5. the fold
    if (!fold_range(cur, n_leaves, NB, start, end, n_left, record,
                    [&](const uint8_t* l, uint8_t* o) { return nmt_join(l, o, nsz, ig); }))
        return done(RSM_PROOF_ORDER);
    return done(memcmp(cur.data(), root, NB) == 0 ? RSM_PROOF_OK : RSM_PROOF_ROOT);
}

// ---- range proofs (include/rsmt2d_hip.h "range proofs") ----
// Host restatements of rsm_range_proofs_dev and the range verify kernels: the namespace
// record of kind INCLUSION over the caller's [start, end), of either tree; the verifiers
// bind the record to the caller's start and end and fold as the namespace verifier does.
extern "C" int rsm_default_tree_range_prove(const uint8_t* const* leaves, uint32_t n_leaves, uint32_t leaf_size,
                                            uint32_t start, uint32_t end, uint8_t* record_out, uint8_t* root_out) {
    if (!leaves || !record_out || n_leaves == 0 || !(start < end && end <= n_leaves)) return RSM_EINVAL;
    for (uint32_t i = 0; i < n_leaves; ++i)
        if (!leaves[i]) return RSM_ETREE;
    const uint32_t L = proof_levels_of(n_leaves);
    std::vector<std::vector<uint8_t>> lv(L + 1);
    lv[0].resize((size_t)n_leaves * 32);
    Digest dg[kHashBatch];
    for (uint32_t i = 0; i < n_leaves; i += kHashBatch) {
        const int c = (int)std::min<uint32_t>(kHashBatch, n_leaves - i);
        hash_prefixed(0x00, leaves + i, c, leaf_size, dg);
        for (int q = 0; q < c; ++q) memcpy(&lv[0][(size_t)(i + q) * 32], dg[q].b, 32);
    }
    build_levels(lv, n_leaves, 32, digest_join_pairs);
    if (root_out) memcpy(root_out, lv[L].data(), 32);
    memset(record_out, 0, 16 + (size_t)(2 * L + 1) * 32);
    put_range_record(record_out, RSM_NS_INCLUSION, lv, n_leaves, 32, start, end);
    return RSM_OK;
}

extern "C" int rsm_nmt_tree_range_prove(const rsm_nmt_params* p, uint32_t index, const uint8_t* const* leaves,
                                        uint32_t n_leaves, uint32_t leaf_size, uint32_t start, uint32_t end,
                                        uint8_t* record_out, uint8_t* root_out) {
    if (!p || !leaves || !record_out || p->namespace_size == 0 || p->square_size == 0 || n_leaves == 0 ||
        !(start < end && end <= n_leaves))
        return RSM_EINVAL;
    const uint32_t nsz = p->namespace_size, NB = 2 * nsz + 32, L = proof_levels_of(n_leaves);
    const bool ig = p->ignore_max_namespace != 0;
    std::vector<std::vector<uint8_t>> lv(L + 1);
    if (int rc = nmt_leaf_level(p, index, leaves, n_leaves, leaf_size, lv[0])) return rc;
    auto join = [&](const uint8_t* cur, uint32_t np, uint8_t* out) { return nmt_join_pairs(cur, np, out, nsz, ig); };
    if (!build_levels(lv, n_leaves, NB, join)) return RSM_ETREE;
    if (root_out) memcpy(root_out, lv[L].data(), NB);
    memset(record_out, 0, 16 + (size_t)(2 * L + 1) * NB);
    put_range_record(record_out, RSM_NS_INCLUSION, lv, n_leaves, NB, start, end);
    return RSM_OK;
}

namespace {

// rule 1 of the range verifiers: the record against the caller's question
bool range_header_ok(const uint8_t* record, uint32_t n_leaves, uint32_t start, uint32_t end, uint32_t n_shares,
                     uint32_t* n_left) {
    if (n_shares != end - start || get_le32(record) != RSM_NS_INCLUSION || get_le32(record + 4) != start ||
        get_le32(record + 8) != end)
        return false;
    return get_le32(record + 12) == range_nodes(n_leaves, start, end, n_left).size();
}

}  // namespace

extern "C" int rsm_default_tree_range_verify(uint32_t start, uint32_t end, const uint8_t* shares, uint32_t n_shares,
                                             uint32_t share_size, uint32_t n_leaves, const uint8_t* record,
                                             const uint8_t* root, uint32_t* status) {
    if (!record || !root || !status || (n_shares && share_size && !shares) || n_leaves == 0 || !(start < end && end <= n_leaves))
        return RSM_EINVAL;
    uint32_t n_left = 0;
    if (!range_header_ok(record, n_leaves, start, end, n_shares, &n_left)) {
        *status = RSM_PROOF_MALFORMED;
        return RSM_OK;
    }
    std::vector<uint8_t> cur((size_t)n_shares * 32);
    for (uint32_t i = 0; i < n_shares; ++i) {
        const Digest d = leaf_hash(shares + (size_t)i * share_size, share_size);
        memcpy(&cur[(size_t)i * 32], d.b, 32);
    }
    fold_range(cur, n_leaves, 32, start, end, n_left, record, [](const uint8_t* l, uint8_t* o) {
        Digest a, b;
        memcpy(a.b, l, 32);
        memcpy(b.b, l + 32, 32);
        memcpy(o, node_hash(a, b).b, 32);
        return true;
    });
    *status = memcmp(cur.data(), root, 32) == 0 ? RSM_PROOF_OK : RSM_PROOF_ROOT;
    return RSM_OK;
}

extern "C" int rsm_nmt_tree_range_verify(const rsm_nmt_params* p, uint32_t index, uint32_t start, uint32_t end,
                                         const uint8_t* shares, uint32_t n_shares, uint32_t share_size, uint32_t n_leaves,
                                         const uint8_t* record, const uint8_t* root, uint32_t* status) {
    if (!p || !record || !root || !status || (n_shares && !shares) || p->namespace_size == 0 || p->square_size == 0 ||
        n_leaves == 0 || !(start < end && end <= n_leaves))
        return RSM_EINVAL;
    const uint32_t nsz = p->namespace_size, NB = 2 * nsz + 32;
    const bool ig = p->ignore_max_namespace != 0;
    if (share_size < nsz) return RSM_ETREE;  // data is too short to contain namespace ID
    uint32_t n_left = 0;
    if (!range_header_ok(record, n_leaves, start, end, n_shares, &n_left)) {
        *status = RSM_PROOF_MALFORMED;
        return RSM_OK;
    }
    std::vector<uint8_t> cur((size_t)n_shares * NB);
    for (uint32_t i = 0; i < n_shares; ++i)
        nmt_leaf_node(p, index, start + i, shares + (size_t)i * share_size, share_size, &cur[(size_t)i * NB]);
    if (!fold_range(cur, n_leaves, NB, start, end, n_left, record,
                    [&](const uint8_t* l, uint8_t* o) { return nmt_join(l, o, nsz, ig); })) {
        *status = RSM_PROOF_ORDER;
        return RSM_OK;
    }
    *status = memcmp(cur.data(), root, NB) == 0 ? RSM_PROOF_OK : RSM_PROOF_ROOT;
    return RSM_OK;
}

// ---- share commitments (include/rsmt2d_hip.h "share commitments") ----
// Host restatements of kernels_commit.hip, stated twice: rsm_blob_commitment from the
// blob's own runs (an NMT per run, every leaf under its own namespace), and
// rsm_square_commitment from the levels of the touched rows' trees, read at the
// coordinates the blob's place in the square dictates.  The RFC 6962 root over the
// subtree roots is the DefaultTree over them.
namespace {

uint64_t pow2ceil64(uint64_t x) {
    uint64_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

// The RFC 6962 root over M roots of NB bytes (tendermint's HashFromByteSlices).
int commitment_of(const std::vector<uint8_t>& roots, uint32_t M, uint32_t NB, uint8_t out[32]) {
    std::vector<const uint8_t*> ptrs(M);
    for (uint32_t i = 0; i < M; ++i) ptrs[i] = &roots[(size_t)i * NB];
    uint32_t len = 32;
    return rsm_default_tree_root(nullptr, 0, 0, ptrs.data(), M, NB, out, &len);
}

}  // namespace

extern "C" uint32_t rsm_subtree_width(uint32_t share_count, uint32_t threshold) {
    if (share_count == 0 || threshold == 0) return 0;
    const uint64_t by_threshold = pow2ceil64(((uint64_t)share_count + threshold - 1) / threshold);
    uint64_t s = 1;  // ceil(sqrt(share_count))
    while (s * s < share_count) ++s;
    return (uint32_t)std::min(by_threshold, pow2ceil64(s));
}

extern "C" int rsm_subtree_sizes(uint32_t share_count, uint32_t width, uint32_t* sizes_out, uint32_t cap, uint32_t* n_out) {
    if (!n_out || share_count == 0 || width == 0 || (width & (width - 1))) return RSM_EINVAL;
    uint32_t m = share_count / width;
    for (uint32_t rem = share_count % width; rem; rem &= rem - 1) ++m;
    *n_out = m;
    if (!sizes_out) return RSM_OK;
    if (m > cap) return RSM_EINVAL;
    uint32_t i = 0;
    for (uint32_t n = share_count; n > 0;) {
        uint32_t z = width;
        while (z > n) z >>= 1;  // the largest power of two <= n
        sizes_out[i++] = z;
        n -= z;
    }
    return RSM_OK;
}

extern "C" int rsm_blob_commitment(const rsm_nmt_params* p, const uint8_t* shares, uint32_t n_shares, uint32_t share_size,
                                   uint32_t threshold, uint8_t out[32], uint32_t* status) {
    if (!p || !shares || !out || !status || n_shares == 0 || threshold == 0 || p->namespace_size == 0 ||
        p->namespace_size > 32)
        return RSM_EINVAL;
    const uint32_t nsz = p->namespace_size, NB = 2 * nsz + 32;
    if (share_size < nsz) return RSM_ETREE;  // data is too short to contain namespace ID
    const uint32_t w = rsm_subtree_width(n_shares, threshold);
    std::vector<uint8_t> roots;
    std::vector<const uint8_t*> leaves;
    uint32_t M = 0;
    for (uint32_t at = 0; at < n_shares; ++M) {
        uint32_t z = w;
        while (z > n_shares - at) z >>= 1;
        // the run's own tree: a wrapper over z leaves whose every leaf is in quadrant 0
        rsm_nmt_params run{nsz, p->ignore_max_namespace, z};
        leaves.resize(z);
        for (uint32_t i = 0; i < z; ++i) leaves[i] = shares + (size_t)(at + i) * share_size;
        roots.resize((size_t)(M + 1) * NB);
        uint32_t len = NB;
        const int rc = rsm_nmt_tree_root(&run, 0, 0, leaves.data(), z, share_size, &roots[(size_t)M * NB], &len);
        if (rc == RSM_ETREE) {
            memset(out, 0, 32);
            *status = RSM_COMMIT_ORDER;
            return RSM_OK;
        }
        if (rc) return rc;
        at += z;
    }
    *status = 0;
    return commitment_of(roots, M, NB, out);
}

extern "C" int rsm_square_commitment(const rsm_nmt_params* p, const uint8_t* const* ods, const uint8_t* eds, uint32_t k,
                                     uint32_t share_size, uint32_t start, uint32_t len, uint32_t threshold, uint8_t out[32],
                                     uint8_t* roots_out, uint32_t* status) {
    if (!p || !out || !status || (ods == nullptr) == (eds == nullptr) || k == 0 || (k & (k - 1)) || k > 32768u ||
        threshold == 0 || len == 0 || p->namespace_size == 0 || p->namespace_size > 32)
        return RSM_EINVAL;
    if ((uint64_t)start + len > (uint64_t)k * k) return RSM_EINVAL;
    const uint32_t w = rsm_subtree_width(len, threshold);
    if (start % w) return RSM_EINVAL;
    const uint32_t nsz = p->namespace_size, NB = 2 * nsz + 32;
    const bool ig = p->ignore_max_namespace != 0;
    if (share_size < nsz) return RSM_ETREE;
    const rsm_nmt_params half{nsz, p->ignore_max_namespace, k};  // the row's quadrant-0 half: k leaves of their own
    uint32_t top = 0;                                             // levels 0 .. log2 w are read
    while ((1u << top) < w) ++top;
    std::vector<std::vector<uint8_t>> lv(top + 1);
    std::vector<const uint8_t*> leaves(k);
    std::vector<uint8_t> roots;
    uint32_t M = 0, have_row = ~0u;
    for (uint32_t at = start; at < start + len; ++M) {
        uint32_t z = w;
        while (z > start + len - at) z >>= 1;
        const uint32_t row = at / k, col = at % k;
        if (row != have_row) {
            for (uint32_t c = 0; c < k; ++c) {
                leaves[c] = ods ? ods[(size_t)row * k + c] : eds + ((size_t)row * 2 * k + c) * share_size;
                if (!leaves[c]) return RSM_ETREE;
            }
            if (nmt_leaf_level(&half, 0, leaves.data(), k, share_size, lv[0]) != RSM_OK) {  // namespace order
                memset(out, 0, 32);
                *status = RSM_COMMIT_TREE;
                return RSM_OK;
            }
            for (uint32_t l = 1; l <= top; ++l) {
                lv[l].assign((size_t)(k >> l) * NB, 0);
                if (!nmt_join_pairs(lv[l - 1].data(), k >> l, lv[l].data(), nsz, ig)) {
                    memset(out, 0, 32);
                    *status = RSM_COMMIT_TREE;
                    return RSM_OK;
                }
            }
            have_row = row;
        }
        uint32_t level = 0;
        while ((1u << level) < z) ++level;
        roots.resize((size_t)(M + 1) * NB);
        memcpy(&roots[(size_t)M * NB], &lv[level][(size_t)(col >> level) * NB], NB);
        at += z;
    }
    if (roots_out) memcpy(roots_out, roots.data(), roots.size());
    *status = 0;
    return commitment_of(roots, M, NB, out);
}
