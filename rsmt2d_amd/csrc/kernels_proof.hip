// kernels_proof.hip -- share inclusion proofs out of a node store (DESIGN.md §4
// "Proofs"; the stores are built by tree_nodes_kernel, kernels_sha.hip, and
// nmt_nodes_kernel, kernels_nmt.hip; layout: rsm_kernels.hpp "proof_*").
//
// A proof of leaf p of a tree of W leaves is, for l = 0 .. L - 1 (L = ceil(log2 W)) and
// j = p >> l, the sibling (l, j ^ 1) where that node exists (j ^ 1 < ceil(W / 2^l));
// where it does not, node (l, j) is carried up and the level adds nothing.  Bottom-up
// that is the order merkletree.Prove() lists after the leaf.
//
// Record (8 + L * node_len bytes): u32 n_nodes | u32 right_mask (bit i: node i is the
// right operand of its parent hash) | n_nodes nodes | zeros.  Node bytes: DefaultTree
// the 32-byte digest; NMT min || max || digest (2 ns + 32 bytes).
//
//   proof_gather_kernel : one lane per (sample, level) copies that level's sibling
//                         (or zero-fills one unused slot); level 0's lane also writes
//                         the header
//   share_gather_kernel : one lane per 16 bytes of a sampled share
// Samples are validated on the host: no kernel sees a coordinate out of range.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "proof_node.hpp"
#include "rsm_kernels.hpp"

namespace rsm {

namespace {

typedef uint32_t pv4u __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void proof_gather_kernel(const uint32_t* __restrict__ store, uint32_t W,
                                                           uint32_t squares, uint32_t ns,
                                                           const ProofSample* __restrict__ samples, uint32_t n,
                                                           uint8_t* __restrict__ records) {
    const uint32_t L = proof_levels(W);
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n * L) return;
    const uint32_t s = t / L, l = t - s * L;
    const ProofSample sm = samples[s];
    const uint32_t node_len = ns ? 2 * ns + 32 : 32;
    uint8_t* rec = records + (uint64_t)s * (8u + L * node_len);
    // slots below this level's, the record's node count and the operand sides
    uint32_t below = 0, n_nodes = 0, mask = 0;
    bool mine = false;
    for (uint32_t i = 0; i < L; ++i) {
        const uint32_t j = sm.pos >> i;
        const bool has = (j ^ 1u) < proof_level_count(W, i);
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
    uint8_t* out = rec + 8u + slot * node_len;
    if (!mine) {
        for (uint32_t i = 0; i < node_len; ++i) out[i] = 0;
        return;
    }
    store_node_bytes(store, W, squares, ns, sm.square, sm.axis, sm.index, l, (sm.pos >> l) ^ 1u, out);
}

__global__ __launch_bounds__(256) void share_gather_kernel(const uint8_t* __restrict__ eds, uint32_t W, uint32_t S,
                                                           const ProofSample* __restrict__ samples, uint32_t n,
                                                           uint8_t* __restrict__ shares) {
    const uint32_t q = S / 16u;  // 16-byte words per share
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (uint64_t)n * q) return;
    const uint32_t s = (uint32_t)(t / q), c = (uint32_t)(t - (uint64_t)s * q);
    const ProofSample sm = samples[s];
    const uint64_t cell = (uint64_t)sm.square * W * W +
                          (sm.axis == 0 ? (uint64_t)sm.index * W + sm.pos : (uint64_t)sm.pos * W + sm.index);
    reinterpret_cast<pv4u*>(shares + (uint64_t)s * S)[c] = reinterpret_cast<const pv4u*>(eds + cell * S)[c];
}

}  // namespace

hipError_t launch_proof_gather(const uint32_t* d_store, uint32_t W, uint32_t squares, uint32_t ns,
                               const ProofSample* d_samples, uint32_t n, uint8_t* d_records, hipStream_t st) {
    const uint64_t lanes = (uint64_t)n * proof_levels(W);
    if (lanes == 0) return hipSuccess;
    hipLaunchKernelGGL(proof_gather_kernel, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, st, d_store, W, squares,
                       ns, d_samples, n, d_records);
    return hipGetLastError();
}

hipError_t launch_share_gather(const uint8_t* d_eds, uint32_t W, uint32_t S, const ProofSample* d_samples, uint32_t n,
                               uint8_t* d_shares, hipStream_t st) {
    const uint64_t lanes = (uint64_t)n * (S / 16u);
    if (lanes == 0) return hipSuccess;
    hipLaunchKernelGGL(share_gather_kernel, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, st, d_eds, W, S,
                       d_samples, n, d_shares);
    return hipGetLastError();
}

}  // namespace rsm
