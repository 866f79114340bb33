// kernels_fraud.hip -- validation of bad-encoding fraud proofs (rsm_fraud_proofs_verify_dev;
// rsm_kernels.hpp "fraud proofs", DESIGN.md §5 "Fraud proofs").  Proof i claims that vector
// refs[i] = (square, axis, index) is badly encoded; it comes as a PACKED vector, row i of
// shares [n][W][S] with presence bytes [n][W], as launch_vectors_gather writes them.  The
// kernels here are what the packed layout needs and the square kernels cannot give:
//   fraud_plan_kernel   : one wave per proof -- its presence count and the samples
//                         {square, axis ^ 1, j, index} of its slots for the verify launch;
//   fraud_lists_kernel  : one workgroup per chunk of W proofs -- the proofs to decode
//                         (k <= present < W) and to check (present >= k), ascending, as
//                         chunk-local indices, their counts reported to the host;
//   fraud_leaf_kernel, fraud_nmt_leaf_kernel
//                       : one lane per (proof, pos) -- the leaf record of a packed share,
//                         the NMT namespace chosen from the proof's own (index, pos);
//   fraud_tree_kernel, fraud_nmt_tree_kernel
//                       : one tree per proof over its W records (list_tree_check_kernel's /
//                         nmt_tree_kernel's level picture), compared with the committed
//                         root (square, axis, index) in the kernel;
//   fraud_verdict_kernel: one wave per proof -- the minimum failing present slot with its
//                         status word (a minimum over keys: no lane order shows), the
//                         tree and parity words, reduced into the verdict record.
// Every address comes from (n, W, S) and the refs the host validated, never from what a
// share, a record or a presence byte holds.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "nmt_dev.hpp"
#include "rsm_kernels.hpp"
#include "sha256_dev.hpp"

namespace rsm {

namespace {

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = __shfl_xor(v, m, 64);
        v = o < v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(64) void fraud_plan_kernel(const uint8_t* __restrict__ present, const RootRef* __restrict__ refs,
                                                        uint32_t W, uint32_t* __restrict__ have,
                                                        ProofSample* __restrict__ samples) {
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    const RootRef r = refs[i];
    uint32_t c = 0;
    for (uint32_t j = lane; j < W; j += 64u) {
        c += present[(uint64_t)i * W + j] != 0 ? 1u : 0u;
        samples[(uint64_t)i * W + j] = ProofSample{r.square, r.axis ^ 1u, j, r.index};
    }
    c = wave_sum(c);
    if (lane == 0) have[i] = c;
}

// Chunk blockIdx.x: proofs [chunk W, min((chunk + 1) W, n)).  A 256-proof step's flags are
// compacted in proof order (ballots per wave, the waves' counts through LDS).
__global__ __launch_bounds__(256) void fraud_lists_kernel(const uint32_t* __restrict__ have, uint32_t W, uint32_t n,
                                                          uint32_t* __restrict__ dec_list, uint32_t* __restrict__ chk_list,
                                                          uint32_t* __restrict__ slot, uint32_t* report) {
    __shared__ uint32_t wave_cnt[2][4];
    const uint32_t chunk = blockIdx.x, k = W / 2, wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t n_dec = 0, n_chk = 0;  // uniform over the workgroup
    for (uint32_t t0 = 0; t0 < W; t0 += 256u) {
        const uint32_t t = t0 + threadIdx.x;
        const uint64_t i = (uint64_t)chunk * W + t;
        const bool in = t < W && i < n;
        const uint32_t p = in ? have[i] : 0u;
        const bool chk = in && p >= k, dec = chk && p < W;
        const uint64_t bd = __ballot(dec), bc = __ballot(chk);
        if (lane == 0) {
            wave_cnt[0][wv] = (uint32_t)__popcll(bd);
            wave_cnt[1][wv] = (uint32_t)__popcll(bc);
        }
        __syncthreads();
        uint32_t od = n_dec, oc = n_chk, td = 0, tc = 0;
        for (uint32_t w = 0; w < 4u; ++w) {
            if (w < wv) od += wave_cnt[0][w], oc += wave_cnt[1][w];
            td += wave_cnt[0][w];
            tc += wave_cnt[1][w];
        }
        const uint64_t below = lane ? (~0ull >> (64u - lane)) : 0ull;
        od += (uint32_t)__popcll(bd & below);
        oc += (uint32_t)__popcll(bc & below);
        if (dec) dec_list[(uint64_t)chunk * W + od] = t;
        if (chk) chk_list[(uint64_t)chunk * W + oc] = t;
        if (in) slot[i] = chk ? chunk * W + oc : ~0u;
        n_dec += td;
        n_chk += tc;
        __syncthreads();  // wave_cnt is rewritten by the next step
    }
    if (threadIdx.x == 0) {
        report[2 * chunk] = n_dec;
        report[2 * chunk + 1] = n_chk;
    }
}

// leaf[(i, pos)][8] = SHA256(0x00 || share), as leaf_hash_kernel; proofs below k are skipped
__global__ __launch_bounds__(256) void fraud_leaf_kernel(const uint8_t* __restrict__ shares, const uint32_t* __restrict__ have,
                                                         uint32_t W, uint32_t S, uint32_t cells, uint32_t* __restrict__ leaf) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= cells) return;
    if (have[t / W] < W / 2) return;
    uint32_t h[8];
    share_leaf_hash(shares + (uint64_t)t * S, S, h);
    v4u* o = reinterpret_cast<v4u*>(leaf + (uint64_t)t * 8u);
    o[0] = v4u{h[0], h[1], h[2], h[3]};
    o[1] = v4u{h[4], h[5], h[6], h[7]};
}

// leaf[(i, pos)][16] = ns | SHA256(0x00 || ns || share), as nmt_leaf29_kernel (NS = 29) or
// nmt_leaf_kernel: ns is the share's own namespace when proof i's vector and pos both lie
// below the original square's size (quadrant 0), else the parity namespace
template <int NS>
__global__ __launch_bounds__(256) void fraud_nmt_leaf_kernel(const uint8_t* __restrict__ shares,
                                                             const uint32_t* __restrict__ have,
                                                             const RootRef* __restrict__ refs, uint32_t W, uint32_t S,
                                                             uint32_t ns, uint32_t sq, uint32_t cells,
                                                             uint32_t* __restrict__ leaf) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= cells) return;
    const uint32_t i = t / W, pos = t - i * W;
    if (have[i] < W / 2) return;
    const bool q0 = refs[i].index < sq && pos < sq;
    Node nd;
    const uint8_t* share = shares + (uint64_t)t * S;
    if constexpr (NS == 29) verify_leaf29(share, S, q0, nd);
    else verify_leaf(share, S, ns, q0, nd);
    uint32_t* o = leaf + (uint64_t)t * kLeafWords;
#pragma unroll
    for (int q = 0; q < (int)kNsWords; ++q) o[q] = nd.mn[q];
#pragma unroll
    for (int q = 0; q < 8; ++q) o[kNsWords + q] = nd.d[q];
}

// One tree per wave (proof blockIdx.x * 4 + wave) in the wave's own LDS, as
// list_tree_check_kernel (wave_tree_levels, sha256_dev.hpp), over the proof's W consecutive
// records.  Lane 0 compares the root with the committed one of the proof's vector.
__global__ __launch_bounds__(256) void fraud_tree_kernel(const uint32_t* __restrict__ leaf, const uint32_t* __restrict__ have,
                                                         const RootRef* __restrict__ refs, uint32_t W, uint32_t n,
                                                         const uint8_t* __restrict__ committed, uint32_t* __restrict__ tree) {
    extern __shared__ uint32_t lds_raw[];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * 4u + wv;
    if (i >= n || have[i] < W / 2) return;  // the whole wave
    uint32_t* const lv = lds_raw + (size_t)wv * ((W + 1) / 2) * 8u;
    leaf += (uint64_t)i * W * 8u;
    wave_tree_levels([&](uint32_t pos) { return leaf + (uint64_t)pos * 8u; }, W, lv, lane);
    if (lane == 0) {
        const RootRef r = refs[i];
        tree[i] = digest_differs(lv, committed + (((uint64_t)r.square * 2u + r.axis) * W + r.index) * 32u) ? kByzRoot : 0u;
    }
}

// One workgroup per proof, nmt_tree_kernel's level-by-level form (block_tree_levels,
// nmt_dev.hpp) over the proof's W consecutive leaf records.  tree[i] receives kByzTree where
// the tree fails, else kByzRoot where the root differs from the committed one of the proof's
// vector, else 0.
__global__ __launch_bounds__(256) void fraud_nmt_tree_kernel(const uint32_t* __restrict__ leaf,
                                                             const uint32_t* __restrict__ have,
                                                             const RootRef* __restrict__ refs, uint32_t W, uint32_t ns,
                                                             uint32_t ignore_max, const uint8_t* __restrict__ committed,
                                                             uint32_t* __restrict__ tree) {
    extern __shared__ uint32_t lds[];
    const uint32_t i = blockIdx.x;
    if (have[i] < W / 2) return;  // the whole workgroup, before any barrier
    uint32_t bad;
    const uint32_t* const top = block_tree_levels(
        leaf + (uint64_t)i * W * kLeafWords, [](uint32_t pos) -> uint64_t { return pos; }, W, ns, ignore_max != 0, lds, &bad);
    if (threadIdx.x == 0) {
        Node rt;
        lds_node(top, rt);
        const RootRef r = refs[i];
        const uint8_t* c = committed + (((uint64_t)r.square * 2u + r.axis) * W + r.index) * (2 * ns + 32);
        tree[i] = bad ? kByzTree : (node_differs(rt, c, ns) ? kByzRoot : 0u);
    }
}

// One wave per proof.  The failing slot is the minimum over the present slots of
// pos << 3 | status (the verify kernels' words are below 8), so whichever lane holds it,
// the same one is named.  out: four words per proof (the C ABI's rsm_fraud_verdict).
__global__ __launch_bounds__(64) void fraud_verdict_kernel(const uint8_t* __restrict__ present,
                                                           const uint32_t* __restrict__ have,
                                                           const uint32_t* __restrict__ status,
                                                           const uint32_t* __restrict__ tree,
                                                           const uint32_t* __restrict__ slot,
                                                           const uint32_t* __restrict__ parity, uint32_t W, uint32_t* out) {
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    const uint32_t p = have[i];
    uint32_t key = ~0u;
    if (p >= W / 2)
        for (uint32_t j = lane; j < W; j += 64u) {
            const uint32_t s = status[(uint64_t)i * W + j];
            if (present[(uint64_t)i * W + j] != 0 && s != kProofOk) {
                const uint32_t kj = j << 3 | (s & 7u);
                key = kj < key ? kj : key;
            }
        }
    key = wave_min(key);
    if (lane != 0) return;
    uint32_t verdict, reason = 0, pos = 0;
    if (p < W / 2) {
        verdict = kFraudTooFew;
    } else if (key != ~0u) {
        verdict = kFraudShare;
        reason = key & 7u;
        pos = key >> 3;
    } else {
        const uint32_t tr = tree[i];
        reason = tr ? tr : (parity[slot[i]] ? kByzEncoding : 0u);
        verdict = reason ? kFraudValid : kFraudConsistent;
    }
    *reinterpret_cast<v4u*>(out + (uint64_t)i * 4u) = v4u{verdict, reason, pos, p};
}

}  // namespace

bool fraud_supported(uint32_t W, uint32_t ns) {
    return ns ? nmt_dev_supported(W, ns) : roots_dev_supported(W);
}

hipError_t launch_fraud_plan(const uint8_t* d_present, const RootRef* d_refs, uint32_t W, uint32_t n, uint32_t* d_have,
                             ProofSample* d_samples, uint32_t* d_dec_list, uint32_t* d_chk_list, uint32_t* d_slot,
                             uint32_t* report, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(fraud_plan_kernel, dim3(n), dim3(64), 0, st, d_present, d_refs, W, d_have, d_samples);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fraud_lists_kernel, dim3((n + W - 1) / W), dim3(256), 0, st, d_have, W, n, d_dec_list, d_chk_list,
                       d_slot, report);
    return hipGetLastError();
}

hipError_t launch_fraud_trees(const uint8_t* d_shares, const uint32_t* d_have, const RootRef* d_refs, uint32_t W, uint32_t S,
                              uint32_t n, uint32_t ns, uint32_t sq, uint32_t ignore_max, const uint8_t* d_committed,
                              uint32_t* d_leaf, uint32_t* d_tree, hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (!fraud_supported(W, ns)) return hipErrorInvalidValue;
    const uint32_t cells = n * W;
    const dim3 grid((cells + 255) / 256);
    if (ns == 0) {
        hipLaunchKernelGGL(fraud_leaf_kernel, grid, dim3(256), 0, st, d_shares, d_have, W, S, cells, d_leaf);
    } else if (ns == 29 && S % 64 == 0 && S >= 64) {
        hipLaunchKernelGGL(fraud_nmt_leaf_kernel<29>, grid, dim3(256), 0, st, d_shares, d_have, d_refs, W, S, ns, sq, cells,
                           d_leaf);
    } else {
        hipLaunchKernelGGL(fraud_nmt_leaf_kernel<0>, grid, dim3(256), 0, st, d_shares, d_have, d_refs, W, S, ns, sq, cells,
                           d_leaf);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (ns == 0) {
        const size_t lds = (size_t)4 * ((W + 1) / 2) * 8u * 4u;  // W = 2048: 128 KiB
        hipLaunchKernelGGL(fraud_tree_kernel, dim3((n + 3) / 4), dim3(256), lds, st, d_leaf, d_have, d_refs, W, n,
                           d_committed, d_tree);
    } else {
        hipLaunchKernelGGL(fraud_nmt_tree_kernel, dim3(n), dim3(256), tree_lds_bytes(W, ns), st, d_leaf, d_have, d_refs, W, ns,
                           ignore_max, d_committed, d_tree);
    }
    return hipGetLastError();
}

hipError_t launch_fraud_verdicts(const uint8_t* d_present, const uint32_t* d_have, const uint32_t* d_status,
                                 const uint32_t* d_tree, const uint32_t* d_slot, const uint32_t* d_parity, uint32_t W,
                                 uint32_t n, uint32_t* out, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(fraud_verdict_kernel, dim3(n), dim3(64), 0, st, d_present, d_have, d_status, d_tree, d_slot, d_parity,
                       W, out);
    return hipGetLastError();
}

}  // namespace rsm
