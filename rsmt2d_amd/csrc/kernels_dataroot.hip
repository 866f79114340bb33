// kernels_dataroot.hip -- the data root of a square: the Merkle root over its 2W row and
// column roots (RFC 6962 over rowRoots ++ colRoots, Celestia's
// DataAvailabilityHeader.Hash()), and proofs of a root under it (DESIGN.md §4 "Data
// root"; layout: rsm_kernels.hpp "data root"; hashes: dataroot_dev.hpp).
//
//   data_root_kernel        : one workgroup per square.  Leaf pass: one lane per leaf
//                             hashes 0x00 || root (one or two blocks); a leaf's lane pair
//                             (2j, 2j + 1: neighbours of one wave) joins into level-1 node
//                             j, kept in LDS.  Levels 2 .. L2 in place in LDS as
//                             tree_nodes_kernel runs them; the lane that hashed a node
//                             also stores it when a node store is given.
//   data_root_gather_kernel : one lane per (ref, level) copies that level's sibling (or
//                             zero-fills one unused slot); level 0's lane also writes the
//                             header -- proof_gather_kernel's shape over 32-byte nodes.
// The chained verify kernels sit beside the verifiers they extend (kernels_sha.hip,
// kernels_nmt.hip).  Refs are validated on the host: no kernel sees one out of range.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "dataroot_dev.hpp"
#include "proof_node.hpp"
#include "rsm_kernels.hpp"

namespace rsm {

namespace {

typedef uint32_t dv4u __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void store_digest(uint32_t* g, const uint32_t (&o)[8]) {
    dv4u* v = reinterpret_cast<dv4u*>(g);
    v[0] = dv4u{o[0], o[1], o[2], o[3]};
    v[1] = dv4u{o[4], o[5], o[6], o[7]};
}

// roots: [squares][2W][root_len] bytes at any alignment; data_roots: [squares][32] bytes
// at any alignment; store (nullable, 16-byte aligned): data_root_store_words.  Dynamic
// LDS: W digests (level 1; the upper levels in place).
__global__ __launch_bounds__(256) void data_root_kernel(const uint8_t* __restrict__ roots, uint32_t W, uint32_t root_len,
                                                        uint8_t* __restrict__ data_roots, uint32_t* __restrict__ store) {
    extern __shared__ uint32_t lds_raw[];
    const uint32_t N = 2u * W, L = proof_levels(N);
    const uint8_t* rt = roots + (uint64_t)blockIdx.x * N * root_len;
    uint32_t* st = store ? store + (uint64_t)blockIdx.x * data_root_tree_words(W) : nullptr;
    // leaves and level 1: N is even, so every leaf has its partner, on the next lane
    for (uint32_t v0 = 0; v0 < N; v0 += 256u) {
        const uint32_t v = v0 + threadIdx.x;
        const bool act = v < N;
        uint32_t B[kRootWords], h[8], r[8], o[8];
        root_words_from_bytes(rt + (uint64_t)(act ? v : 0u) * root_len, root_len, B);
        root_leaf_hash(B, root_len, h);
        if (act && st) store_digest(st + (uint64_t)v * 8u, h);
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] = __shfl_down(h[i], 1);
        if (act && !(v & 1u)) {
            node_hash(h, r, o);
            uint32_t* lv = lds_raw + (size_t)(v >> 1) * 8u;
#pragma unroll
            for (int i = 0; i < 8; ++i) lv[i] = o[i];
            if (st) store_digest(st + ((uint64_t)N + (v >> 1)) * 8u, o);
        }
    }
    __syncthreads();
    uint32_t prev = W, off = W;  // nodes of level l - 1; level l's first node among levels 1 .. L
    for (uint32_t l = 2; l <= L; ++l) {
        const uint32_t cnt = (prev + 1) / 2;
        for (uint32_t v0 = 0; v0 < cnt; v0 += 256u) {
            const uint32_t j = v0 + threadIdx.x;
            const bool act = j < cnt;
            uint32_t o[8];
            if (act) {
                uint32_t a[8], b[8];
                const bool pair = 2 * j + 1 < prev;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    a[i] = lds_raw[(size_t)(2 * j) * 8u + i];
                    b[i] = pair ? lds_raw[(size_t)(2 * j + 1) * 8u + i] : 0u;
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
                uint32_t* lv = lds_raw + (size_t)j * 8u;
#pragma unroll
                for (int i = 0; i < 8; ++i) lv[i] = o[i];
                if (st) store_digest(st + ((uint64_t)N + off + j) * 8u, o);
            }
            __syncthreads();
        }
        off += cnt;
        prev = cnt;
    }
    if (threadIdx.x < 8u) {  // the root, big-endian digest bytes
        const uint32_t x = __builtin_bswap32(lds_raw[threadIdx.x]);
        __builtin_memcpy(data_roots + (uint64_t)blockIdx.x * 32u + 4u * threadIdx.x, &x, 4);
    }
}

__global__ __launch_bounds__(256) void data_root_gather_kernel(const uint32_t* __restrict__ store, uint32_t W,
                                                               const RootRef* __restrict__ refs, uint32_t n,
                                                               uint8_t* __restrict__ records) {
    const uint32_t N = 2u * W, L = proof_levels(N);
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n * L) return;
    const uint32_t s = t / L, l = t - s * L;
    const RootRef rf = refs[s];
    const uint32_t pos = rf.axis * W + rf.index;
    uint8_t* rec = records + (uint64_t)s * (8u + L * 32u);
    // slots below this level's, the record's node count and the operand sides
    uint32_t below = 0, n_nodes = 0, mask = 0;
    bool mine = false;
    for (uint32_t i = 0; i < L; ++i) {
        const uint32_t j = pos >> i;
        const bool has = (j ^ 1u) < proof_level_count(N, i);
        if (i == l) mine = has;
        if (has) {
            if (!(j & 1u)) mask |= 1u << n_nodes;  // the sibling j + 1 is the right operand
            if (i < l) ++below;
            ++n_nodes;
        }
    }
    if (l == 0) {
        for (int b = 0; b < 4; ++b) {
            rec[b] = (uint8_t)(n_nodes >> (8 * b));
            rec[4 + b] = (uint8_t)(mask >> (8 * b));
        }
    }
    // a level without a sibling zero-fills one of the unused slots n_nodes .. L - 1
    const uint32_t slot = mine ? below : n_nodes + (l - below);
    uint8_t* out = rec + 8u + slot * 32u;
    if (!mine) {
        for (uint32_t i = 0; i < 32; ++i) out[i] = 0;
        return;
    }
    const uint32_t j = (pos >> l) ^ 1u;
    const uint32_t* dg = store + (uint64_t)rf.square * data_root_tree_words(W) +
                         ((uint64_t)(l == 0 ? 0u : N + proof_level_offset(N, l)) + j) * 8u;
    if ((reinterpret_cast<uintptr_t>(out) & 3u) == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) reinterpret_cast<uint32_t*>(out)[i] = __builtin_bswap32(dg[i]);
    } else {
        for (uint32_t i = 0; i < 32; ++i) out[i] = word_byte(dg, i);
    }
}

}  // namespace

bool data_roots_dev_supported(uint32_t W) { return W >= 1 && W <= kDataRootMaxWidth; }

hipError_t launch_data_roots(const uint8_t* d_roots, uint32_t W, uint32_t root_len, uint32_t squares,
                             uint8_t* d_data_roots, uint32_t* d_store, hipStream_t st) {
    if (squares == 0) return hipSuccess;
    if (!data_roots_dev_supported(W) || root_len < 32u || root_len > 4u * kRootWords) return hipErrorInvalidValue;
    hipLaunchKernelGGL(data_root_kernel, dim3(squares), dim3(256), (size_t)W * 32u, st, d_roots, W, root_len, d_data_roots,
                       d_store);
    return hipGetLastError();
}

hipError_t launch_data_root_gather(const uint32_t* d_store, uint32_t W, const RootRef* d_refs, uint32_t n,
                                   uint8_t* d_records, hipStream_t st) {
    const uint64_t lanes = (uint64_t)n * proof_levels(2u * W);
    if (lanes == 0) return hipSuccess;
    hipLaunchKernelGGL(data_root_gather_kernel, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, st, d_store, W, d_refs,
                       n, d_records);
    return hipGetLastError();
}

}  // namespace rsm
