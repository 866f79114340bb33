// kernels_commit.hip -- blob share commitments (celestia-app's inclusion.CreateCommitment
// and GetCommitment; DESIGN.md §4 "Commitments"; layout: rsm_kernels.hpp "share
// commitments").  A commitment is the RFC 6962 root over a blob's subtree roots, the NMT
// roots over the runs of its mountain range.  Three stages:
//
//   commit_leaf_kernel  : shares path.  One lane per packed share: the leaf record
//                         (namespace, digest) of the share under its own namespace
//                         (verify_leaf29 / verify_leaf with q0 = true).
//   subtree pass        : shares path, one launch per subtree size present (the host groups
//                         the tasks by size, so every launch is uniform):
//     commit_copy_kernel  size 1: the root is the leaf node; one lane per task.
//     commit_wave_kernel  sizes 2 .. 128: size / 2 lanes per subtree, 128 / size subtrees
//                         per wave of 64 lanes, levels in place in the wave's LDS.
//     commit_block_kernel sizes 256 .. 1024: one workgroup per subtree
//                         (block_tree_levels, the row trees' reduction).
//                         Each writes the root bytes min || max || digest at the task's
//                         packed slot and the slot's flag word: non-zero where a leaf's
//                         namespace is below its predecessor's (or siblings are unordered).
//   commit_fold_kernel  : both paths.  One workgroup per blob over its M roots: leaf
//                         hashes SHA256(0x00 || root), a lane pair's join into level 1 kept
//                         in LDS, the upper levels in place as data_root_kernel runs them,
//                         an unpaired last node carried up; any 1 <= M <= 4096.  STORE: the
//                         roots are gathered from the node store (store_node_bytes) at the
//                         row-tree coordinates the blob's (start, len, width) dictate, no
//                         share is read; a touched row's non-zero tree status word fails
//                         the blob.
// Counts and coordinates come from the host-validated offsets and blob refs, never from
// what a share holds.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "dataroot_dev.hpp"
#include "nmt_dev.hpp"
#include "proof_node.hpp"
#include "rsm_kernels.hpp"
#include "sha256_dev.hpp"

namespace rsm {

namespace {

constexpr uint32_t kRootStride = 2 * kMaxNs + 32;  // a lane's gather buffer (STORE)

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// min || max || digest of node n at o (2 ns + 32 bytes, any alignment)
__device__ __forceinline__ void put_root(const Node& n, uint32_t ns, uint8_t* __restrict__ o) {
#pragma unroll
    for (int i = 0; i < (int)kMaxNs; ++i)
        if (i < (int)ns) {
            o[i] = be_byte(n.mn, i);
            o[ns + i] = be_byte(n.mx, i);
        }
#pragma unroll
    for (int i = 0; i < 32; ++i) o[2 * ns + i] = be_byte(n.d, i);
}

// leaf: [total][kLeafWords]; shares: [total][S], 16-byte aligned
template <bool NS29>
__global__ __launch_bounds__(256) void commit_leaf_kernel(const uint8_t* __restrict__ shares, uint32_t total, uint32_t S,
                                                          uint32_t ns, uint32_t* __restrict__ leaf) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    Node n;
    if constexpr (NS29) verify_leaf29(shares + (uint64_t)i * S, S, true, n);
    else verify_leaf(shares + (uint64_t)i * S, S, ns, true, n);
    uint32_t* o = leaf + (uint64_t)i * kLeafWords;
#pragma unroll
    for (int q = 0; q < (int)kNsWords; ++q) o[q] = n.mn[q];
#pragma unroll
    for (int q = 0; q < 8; ++q) o[kNsWords + q] = n.d[q];
}

__global__ __launch_bounds__(256) void commit_copy_kernel(const uint32_t* __restrict__ leaf,
                                                          const CommitTask* __restrict__ tasks, uint32_t n_tasks,
                                                          uint32_t ns, uint8_t* __restrict__ roots,
                                                          uint32_t* __restrict__ flags) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_tasks) return;
    const CommitTask tk = tasks[t];
    Node n;
    leaf_node(leaf, tk.first, n);
    put_root(n, ns, roots + (uint64_t)tk.slot * (2u * ns + 32u));
    flags[tk.slot] = 0u;
}

// z = 2 .. 128 leaves per subtree: lane = (subtree g of the wave, pair j of its level 1).
// Dynamic LDS: 64 nodes and 64 message buffers.  Every lane runs to the end: a group past
// the last task works on task 0 and stores nothing.
__global__ __launch_bounds__(64) void commit_wave_kernel(const uint32_t* __restrict__ leaf,
                                                         const CommitTask* __restrict__ tasks, uint32_t n_tasks, uint32_t z,
                                                         uint32_t ns, uint32_t ignore_max, uint8_t* __restrict__ roots,
                                                         uint32_t* __restrict__ flags) {
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x, hz = z / 2u, G = 64u / hz;
    const uint32_t g = lane / hz, j = lane - g * hz;
    const uint32_t t = blockIdx.x * G + g;
    const bool act = t < n_tasks, ig = ignore_max != 0;
    uint32_t* const nodes = lds;
    uint8_t* const mb = reinterpret_cast<uint8_t*>(lds + 64u * kNodeWords) + lane * (64u * node_blocks(ns));
    const CommitTask tk = tasks[act ? t : 0u];
    bool bad = false;
    Node a, b, o;
    leaf_node(leaf, (uint64_t)tk.first + 2u * j, a);
    leaf_node(leaf, (uint64_t)tk.first + 2u * j + 1u, b);
    if (ns_less(b.mn, a.mn)) bad = true;
    if (2u * j + 2u < z) {
        Node c;
        leaf_node(leaf, (uint64_t)tk.first + 2u * j + 2u, c);
        if (ns_less(c.mn, b.mn)) bad = true;
    }
    if (!hash_node(a, b, ns, ig, mb, o)) bad = true;
    lds_store(nodes + (size_t)lane * kNodeWords, o);
    wave_sync();
    for (uint32_t cnt = hz; cnt > 1u; cnt >>= 1) {
        const bool mine = j < cnt / 2u;
        if (mine) {
            lds_node(nodes + (size_t)(g * hz + 2u * j) * kNodeWords, a);
            lds_node(nodes + (size_t)(g * hz + 2u * j + 1u) * kNodeWords, b);
            if (!hash_node(a, b, ns, ig, mb, o)) bad = true;
        }
        wave_sync();  // every read of this level before its in-place writes
        if (mine) lds_store(nodes + (size_t)(g * hz + j) * kNodeWords, o);
        wave_sync();
    }
    const uint64_t failing = __ballot(bad);
    if (act && j == 0u) {
        lds_node(nodes + (size_t)(g * hz) * kNodeWords, o);
        put_root(o, ns, roots + (uint64_t)tk.slot * (2u * ns + 32u));
        const uint64_t mine = (hz == 64u ? ~0ull : ((1ull << hz) - 1ull)) << (g * hz);
        flags[tk.slot] = (failing & mine) ? 1u : 0u;
    }
}

// z = 256 .. 1024: one workgroup per subtree.  Dynamic LDS: tree_lds_bytes(z, ns).
__global__ __launch_bounds__(256) void commit_block_kernel(const uint32_t* __restrict__ leaf,
                                                           const CommitTask* __restrict__ tasks, uint32_t z, uint32_t ns,
                                                           uint32_t ignore_max, uint8_t* __restrict__ roots,
                                                           uint32_t* __restrict__ flags) {
    extern __shared__ uint32_t lds[];
    const CommitTask tk = tasks[blockIdx.x];
    uint32_t bad;
    const uint32_t* const top = block_tree_levels(
        leaf, [&](uint32_t pos) -> uint64_t { return (uint64_t)tk.first + pos; }, z, ns, ignore_max != 0, lds, &bad);
    if (threadIdx.x == 0) {
        Node rt;
        lds_node(top, rt);
        put_root(rt, ns, roots + (uint64_t)tk.slot * (2u * ns + 32u));
        flags[tk.slot] = bad;
    }
}

// The fold of M roots of NB bytes; lane v of a pass reads root_at(v) (v < M).  dg: room
// for ceil(M / 2) digests.  The root is dg[0 .. 7] when it returns (after a barrier).
template <class RootAt>
__device__ __forceinline__ void fold_roots(RootAt&& root_at, uint32_t M, uint32_t NB, uint32_t* __restrict__ dg) {
    // leaves and level 1: a pass starts at a multiple of 256, so leaf 2j's partner is on the next lane
    for (uint32_t v0 = 0; v0 < M; v0 += 256u) {
        const uint32_t v = v0 + threadIdx.x;
        const bool act = v < M;
        uint32_t B[kRootWords], h[8], r[8], o[8];
        root_words_from_bytes(root_at(act ? v : 0u, act), NB, B);
        root_leaf_hash(B, NB, h);
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] = __shfl_down(h[i], 1);
        if (act && !(v & 1u)) {
            if (v + 1u < M) {
                node_hash(h, r, o);
            } else {  // the unpaired last leaf (M = 1: the commitment itself)
#pragma unroll
                for (int i = 0; i < 8; ++i) o[i] = h[i];
            }
            uint32_t* lv = dg + (size_t)(v >> 1) * 8u;
#pragma unroll
            for (int i = 0; i < 8; ++i) lv[i] = o[i];
        }
    }
    __syncthreads();
    for (uint32_t prev = (M + 1u) / 2u; prev > 1u;) {
        const uint32_t cnt = (prev + 1u) / 2u;
        for (uint32_t v0 = 0; v0 < cnt; v0 += 256u) {
            const uint32_t j = v0 + threadIdx.x;
            const bool act = j < cnt;
            uint32_t o[8];
            if (act) {
                uint32_t a[8], b[8];
                const bool pair = 2u * j + 1u < prev;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    a[i] = dg[(size_t)(2u * j) * 8u + i];
                    b[i] = pair ? dg[(size_t)(2u * j + 1u) * 8u + i] : 0u;
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
                uint32_t* lv = dg + (size_t)j * 8u;
#pragma unroll
                for (int i = 0; i < 8; ++i) lv[i] = o[i];
            }
            __syncthreads();
        }
        prev = cnt;
    }
}

// commitments: [n][32] at any alignment (zeros where the blob fails); status: [n] words
__device__ __forceinline__ void put_commitment(const uint32_t* dg, uint32_t failed, uint32_t code,
                                               uint8_t* __restrict__ commitments, uint32_t* __restrict__ status) {
    if (threadIdx.x < 8u) {
        const uint32_t x = failed ? 0u : __builtin_bswap32(dg[threadIdx.x]);
        __builtin_memcpy(commitments + (uint64_t)blockIdx.x * 32u + 4u * threadIdx.x, &x, 4);
    }
    if (threadIdx.x == 0) status[blockIdx.x] = failed ? code : 0u;
}

// Shares path: blob b's roots are slots [root_offs[b], root_offs[b + 1]) of roots / flags.
// Dynamic LDS: ceil(max M / 2) digests.
__global__ __launch_bounds__(256) void commit_fold_kernel(const uint8_t* __restrict__ roots,
                                                          const uint32_t* __restrict__ flags,
                                                          const uint32_t* __restrict__ root_offs, uint32_t ns,
                                                          uint8_t* __restrict__ commitments, uint32_t* __restrict__ status) {
    extern __shared__ uint32_t lds[];
    __shared__ uint32_t first_bad;
    const uint32_t r0 = root_offs[blockIdx.x], M = root_offs[blockIdx.x + 1] - r0, NB = 2u * ns + 32u;
    if (threadIdx.x == 0) first_bad = ~0u;
    __syncthreads();
    // the lowest failing subtree: a minimum over keys, whichever lane finds it
    for (uint32_t v = threadIdx.x; v < M; v += 256u)
        if (flags[r0 + v]) atomicMin(&first_bad, v);
    fold_roots([&](uint32_t v, bool) -> const uint8_t* { return roots + (uint64_t)(r0 + v) * NB; }, M, NB, lds);
    put_commitment(lds, first_bad != ~0u, kCommitOrder, commitments, status);
}

// Store path: blob b is blobs[b]; its root v is node (level, j) of row `row` of its square
// (mountain_node).  Dynamic LDS: ceil(max M / 2) digests, then 256 gather buffers.
__device__ __forceinline__ void mountain_node(const CommitBlob& bl, uint32_t k, uint32_t v, uint32_t* row, uint32_t* level,
                                              uint32_t* j) {
    const uint32_t q = bl.len / bl.w;
    uint32_t off, z = bl.w;
    if (v < q) {
        off = v * bl.w;
    } else {  // the (v - q)-th set bit of the remainder, from the top
        const uint32_t rem = bl.len - q * bl.w;
        uint32_t idx = v - q;
        off = q * bl.w;
        for (uint32_t bit = bl.w >> 1; bit; bit >>= 1)
            if (rem & bit) {
                z = bit;
                if (idx == 0) break;
                off += bit;
                --idx;
            }
    }
    const uint32_t p = bl.start + off;
    *row = p / k;
    *level = (uint32_t)__builtin_ctz(z);
    *j = (p - *row * k) >> *level;
}

__global__ __launch_bounds__(256) void commit_fold_store_kernel(const uint32_t* __restrict__ store,
                                                                const uint32_t* __restrict__ status_trees, uint32_t W,
                                                                uint32_t squares, uint32_t ns,
                                                                const CommitBlob* __restrict__ blobs, uint32_t n,
                                                                uint32_t max_m, uint8_t* __restrict__ roots_out,
                                                                uint32_t* __restrict__ root_offs_out,
                                                                uint8_t* __restrict__ commitments,
                                                                uint32_t* __restrict__ status) {
    extern __shared__ uint32_t lds[];
    __shared__ uint32_t tree_bad;
    const CommitBlob bl = blobs[blockIdx.x];
    const uint32_t k = W / 2u, NB = 2u * ns + 32u;
    uint8_t* const tmp = reinterpret_cast<uint8_t*>(lds + (size_t)((max_m + 1u) / 2u) * 8u) + threadIdx.x * kRootStride;
    if (threadIdx.x == 0) {
        tree_bad = 0u;
        if (root_offs_out) {
            root_offs_out[blockIdx.x] = bl.root_off;
            if (blockIdx.x == n - 1u) root_offs_out[n] = bl.root_off + bl.m;
        }
    }
    __syncthreads();
    const uint32_t row0 = bl.start / k, row1 = (bl.start + bl.len - 1u) / k;
    for (uint32_t r = row0 + threadIdx.x; r <= row1; r += 256u)
        if (status_trees[(uint64_t)bl.square * 2u * W + r]) atomicOr(&tree_bad, 1u);
    fold_roots(
        [&](uint32_t v, bool act) -> const uint8_t* {
            uint32_t row, level, j;
            mountain_node(bl, k, v, &row, &level, &j);
            store_node_bytes(store, W, squares, ns, bl.square, 0u, row, level, j, tmp);
            if (act && roots_out) {
                uint8_t* o = roots_out + ((uint64_t)bl.root_off + v) * NB;
                for (uint32_t i = 0; i < NB; ++i) o[i] = tmp[i];
            }
            return tmp;
        },
        bl.m, NB, lds);
    put_commitment(lds, tree_bad, kCommitTree, commitments, status);
}

}  // namespace

bool commit_subtree_supported(uint32_t z, uint32_t ns) {
    if (z == 0 || (z & (z - 1u)) || ns < 1 || ns > kMaxNs) return false;
    return z <= kCommitWaveMax || nmt_dev_supported(z, ns);
}

hipError_t launch_commit_leaves(const uint8_t* d_shares, uint32_t total, uint32_t S, uint32_t ns, uint32_t* d_leaf,
                                hipStream_t st) {
    if (total == 0) return hipSuccess;
    const dim3 grid((total + 255u) / 256u);
    if (ns == 29 && S % 64 == 0 && S >= 64)
        hipLaunchKernelGGL(commit_leaf_kernel<true>, grid, dim3(256), 0, st, d_shares, total, S, ns, d_leaf);
    else
        hipLaunchKernelGGL(commit_leaf_kernel<false>, grid, dim3(256), 0, st, d_shares, total, S, ns, d_leaf);
    return hipGetLastError();
}

hipError_t launch_commit_subtrees(const uint32_t* d_leaf, const CommitTask* d_tasks, uint32_t n_tasks, uint32_t z,
                                  uint32_t ns, uint32_t ignore_max, uint8_t* d_roots, uint32_t* d_flags, hipStream_t st) {
    if (n_tasks == 0) return hipSuccess;
    if (!commit_subtree_supported(z, ns)) return hipErrorInvalidValue;
    if (z == 1) {
        hipLaunchKernelGGL(commit_copy_kernel, dim3((n_tasks + 255u) / 256u), dim3(256), 0, st, d_leaf, d_tasks, n_tasks, ns,
                           d_roots, d_flags);
    } else if (z <= kCommitWaveMax) {
        const uint32_t per_wave = 128u / z;
        const size_t lds = (size_t)64 * kNodeWords * 4u + (size_t)64 * 64u * node_blocks(ns);
        hipLaunchKernelGGL(commit_wave_kernel, dim3((n_tasks + per_wave - 1u) / per_wave), dim3(64), lds, st, d_leaf, d_tasks,
                           n_tasks, z, ns, ignore_max, d_roots, d_flags);
    } else {
        hipLaunchKernelGGL(commit_block_kernel, dim3(n_tasks), dim3(256), tree_lds_bytes(z, ns), st, d_leaf, d_tasks, z, ns,
                           ignore_max, d_roots, d_flags);
    }
    return hipGetLastError();
}

hipError_t launch_commit_fold(const uint8_t* d_roots, const uint32_t* d_flags, const uint32_t* d_root_offs, uint32_t n,
                              uint32_t max_m, uint32_t ns, uint8_t* d_commitments, uint32_t* d_status, hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (max_m == 0 || max_m > kCommitMaxRoots) return hipErrorInvalidValue;
    hipLaunchKernelGGL(commit_fold_kernel, dim3(n), dim3(256), (size_t)((max_m + 1u) / 2u) * 32u, st, d_roots, d_flags,
                       d_root_offs, ns, d_commitments, d_status);
    return hipGetLastError();
}

hipError_t launch_commit_fold_store(const uint32_t* d_store, const uint32_t* d_status_trees, uint32_t W, uint32_t squares,
                                    uint32_t ns, const CommitBlob* d_blobs, uint32_t n, uint32_t max_m, uint8_t* d_roots_out,
                                    uint32_t* d_root_offs_out, uint8_t* d_commitments, uint32_t* d_status, hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (max_m == 0 || max_m > kCommitMaxRoots) return hipErrorInvalidValue;
    const size_t lds = (size_t)((max_m + 1u) / 2u) * 32u + (size_t)256 * kRootStride;
    hipLaunchKernelGGL(commit_fold_store_kernel, dim3(n), dim3(256), lds, st, d_store, d_status_trees, W, squares, ns, d_blobs,
                       n, max_m, d_roots_out, d_root_offs_out, d_commitments, d_status);
    return hipGetLastError();
}

}  // namespace rsm
