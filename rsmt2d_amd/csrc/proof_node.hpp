// proof_node.hpp -- device helpers of the gather kernels (kernels_proof.hip,
// kernels_nsproof.hip): a node of the node store (rsm_kernels.hpp "proof_*") written
// out in the byte order of roots and proof records.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "rsm_kernels.hpp"

namespace rsm {

// byte i of a big-endian word array
__device__ __forceinline__ uint8_t word_byte(const uint32_t* w, uint32_t i) {
    return (uint8_t)(w[i >> 2] >> (24u - 8u * (i & 3u)));
}

// Node (l, j) of tree (square, axis, index) of a store of `squares` squares of width W,
// as node_len bytes at `out` (any alignment).  ns = 0: DefaultTree store (the 32-byte
// digest); else min || max || digest, a level-0 node being the leaf record with its
// namespace as both.
__device__ __forceinline__ void store_node_bytes(const uint32_t* __restrict__ store, uint32_t W, uint32_t squares,
                                                 uint32_t ns, uint32_t square, uint32_t axis, uint32_t index,
                                                 uint32_t l, uint32_t j, uint8_t* __restrict__ out) {
    const uint32_t lw = ns ? kProofNmtLeafWords : kProofShaWords, nw = ns ? kProofNmtNodeWords : kProofShaWords;
    const uint32_t *mn, *mx, *dg;  // the node's min / max namespace and digest words
    if (l == 0) {
        const uint64_t cell = axis == 0 ? (uint64_t)index * W + j : (uint64_t)j * W + index;
        const uint32_t* p = store + ((uint64_t)square * W * W + cell) * lw;
        mn = mx = p;  // a leaf's namespace is both
        dg = ns ? p + 8 : p;
    } else {
        const uint64_t tree = (uint64_t)square * 2 * W + (uint64_t)axis * W + index;
        const uint32_t* p =
            store + (uint64_t)squares * W * W * lw + (tree * proof_tree_nodes(W) + proof_level_offset(W, l) + j) * nw;
        mn = p;
        mx = p + 8;
        dg = ns ? p + 16 : p;
    }
    for (uint32_t i = 0; i < ns; ++i) {
        out[i] = word_byte(mn, i);
        out[ns + i] = word_byte(mx, i);
    }
    out += 2 * ns;
    if ((reinterpret_cast<uintptr_t>(out) & 3u) == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) reinterpret_cast<uint32_t*>(out)[i] = __builtin_bswap32(dg[i]);
    } else {
        for (uint32_t i = 0; i < 32; ++i) out[i] = word_byte(dg, i);
    }
}

}  // namespace rsm
