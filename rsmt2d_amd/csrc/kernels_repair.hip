// kernels_repair.hip -- the device half of rsm_repair_squares_dev and
// rsm_samples_scatter_dev (DESIGN.md §5 "Device-resident Repair"): the sweep planner over
// [count][W][W] presence bytes, the batch verification's gather and compare kernels, and
// the decide / apply pair that sets verified samples into device squares.
//
// Every kernel does bounded work: no device-side waits, no flags to spin on, no
// persistent loops.  What comes next is the host loop's decision (rsm_repair_dev.cpp).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "rsm_kernels.hpp"

namespace rsm {

namespace {

constexpr uint32_t kPlanThreads = 256;

__device__ inline uint32_t nonzero_bytes(uint32_t x) {
    return (uint32_t)((x & 0xFFu) != 0) + (uint32_t)((x & 0xFF00u) != 0) + (uint32_t)((x & 0xFF0000u) != 0) +
           (uint32_t)((x & 0xFF000000u) != 0);
}

// One workgroup per square.  In order:
//   mark   every cell of the vectors the previous pass decoded (prev_todo, of the other
//          axis; their count is the square's state word) becomes present;
//   count  have[i] of the W vectors of `axis`.  Rows: the square's bytes as one flat
//          array of 16-byte words (W a multiple of 16: a word never leaves its row) or
//          4-byte words (a word may straddle two rows: per byte then), LDS adds.
//          Columns: a lane owns 4 (or 2) adjacent columns and walks a slice of the rows,
//          so a wave reads consecutive words of one row at a time; LDS adds;
//   list   the indices with k <= have < W, ascending, by a prefix scan over per-lane
//          chunks of consecutive indices;
//   report the todo count and the cells still missing (before this pass's decodes): two
//          words per square in `report` (pinned host memory through its device mapping);
//          the count also in the square's state word, for the next launch's marks.
// first != 0: the state word is not read (first pass of a call).
__global__ __launch_bounds__(kPlanThreads) void repair_plan_kernel(uint8_t* pres, uint32_t W, uint32_t k, uint32_t axis,
                                                                    uint32_t first, const uint32_t* prev_todo,
                                                                    uint32_t* todo, uint32_t* state, uint32_t* report) {
    __shared__ uint32_t have[2048];
    __shared__ uint32_t scan[kPlanThreads];
    __shared__ uint32_t total;
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    uint8_t* const p = pres + (uint64_t)s * W * W;
    const uint32_t prev_cnt = first ? 0u : state[s];
    // ---- mark ----
    if (prev_cnt) {
        const uint32_t* const pt = prev_todo + (uint64_t)s * W;
        for (uint32_t i = t; i < prev_cnt * W; i += kPlanThreads) {
            const uint32_t v = pt[i / W], e = i % W;
            // the previous pass ran on the other axis
            p[axis == 0 ? (uint64_t)e * W + v : (uint64_t)v * W + e] = 1;
        }
    }
    for (uint32_t i = t; i < W; i += kPlanThreads) have[i] = 0;
    if (t == 0) total = 0;
    __syncthreads();  // marks visible to the workgroup, have[] zeroed
    // ---- count ----
    const uint32_t cells = W * W;
    if (axis == 0) {
        if ((W & 15u) == 0 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
            const uint4* const q = reinterpret_cast<const uint4*>(p);
            const uint32_t per_row = W / 16;
            for (uint32_t i = t; i < cells / 16; i += kPlanThreads) {
                const uint4 x = q[i];
                const uint32_t n = nonzero_bytes(x.x) + nonzero_bytes(x.y) + nonzero_bytes(x.z) + nonzero_bytes(x.w);
                if (n) atomicAdd(&have[i / per_row], n);
            }
        } else {  // cells is a multiple of 4 and so is every square's first byte
            const uint32_t* const q = reinterpret_cast<const uint32_t*>(p);
            for (uint32_t i = t; i < cells / 4; i += kPlanThreads) {
                const uint32_t x = q[i];
                const uint32_t r0 = (4 * i) / W, r1 = (4 * i + 3) / W;
                if (r0 == r1) {
                    const uint32_t n = nonzero_bytes(x);
                    if (n) atomicAdd(&have[r0], n);
                } else {
                    for (uint32_t b = 0; b < 4; ++b)
                        if ((x >> (8 * b)) & 0xFFu) atomicAdd(&have[(4 * i + b) / W], 1u);
                }
            }
        }
    } else {
        // a lane owns 4 adjacent columns (W a multiple of 4: every row is 4-byte aligned) or
        // 2 (W is even) and walks a slice of the rows; a wave reads consecutive words of
        // one row at a time.  Narrow squares split the rows over the lanes left over.
        const bool quad = (W & 3u) == 0;
        const uint32_t G = quad ? W / 4 : W / 2;  // column groups
        const uint32_t slices = G < kPlanThreads ? kPlanThreads / G : 1u;
        const uint32_t rows_per = (W + slices - 1) / slices;
        for (uint32_t u = t; u < G * slices; u += kPlanThreads) {
            const uint32_t g = u % G, r0 = (u / G) * rows_per;
            const uint32_t r1 = r0 + rows_per < W ? r0 + rows_per : W;
            uint32_t n0 = 0, n1 = 0, n2 = 0, n3 = 0;
            if (quad) {
                const uint8_t* col = p + 4 * g;
#pragma unroll 8
                for (uint32_t r = r0; r < r1; ++r) {
                    const uint32_t x = *reinterpret_cast<const uint32_t*>(col + (uint64_t)r * W);
                    n0 += (x & 0xFFu) != 0;
                    n1 += (x & 0xFF00u) != 0;
                    n2 += (x & 0xFF0000u) != 0;
                    n3 += (x & 0xFF000000u) != 0;
                }
                if (n0) atomicAdd(&have[4 * g], n0);
                if (n1) atomicAdd(&have[4 * g + 1], n1);
                if (n2) atomicAdd(&have[4 * g + 2], n2);
                if (n3) atomicAdd(&have[4 * g + 3], n3);
            } else {
                const uint8_t* col = p + 2 * g;
#pragma unroll 8
                for (uint32_t r = r0; r < r1; ++r) {
                    const uint32_t x = *reinterpret_cast<const uint16_t*>(col + (uint64_t)r * W);
                    n0 += (x & 0xFFu) != 0;
                    n1 += (x & 0xFF00u) != 0;
                }
                if (n0) atomicAdd(&have[2 * g], n0);
                if (n1) atomicAdd(&have[2 * g + 1], n1);
            }
        }
    }
    __syncthreads();
    // ---- list ----
    const uint32_t per = (W + kPlanThreads - 1) / kPlanThreads;  // <= 8
    const uint32_t i0 = t * per, i1 = i0 + per < W ? i0 + per : W;
    uint32_t mine = 0, sum = 0;
    for (uint32_t i = i0; i < i1; ++i) {
        const uint32_t h = have[i];
        mine += (h >= k && h < W) ? 1u : 0u;
        sum += h;
    }
    if (sum) atomicAdd(&total, sum);
    scan[t] = mine;
    __syncthreads();
    for (uint32_t d = 1; d < kPlanThreads; d <<= 1) {  // inclusive Hillis-Steele scan
        const uint32_t add = t >= d ? scan[t - d] : 0u;
        __syncthreads();
        scan[t] += add;
        __syncthreads();
    }
    uint32_t at = scan[t] - mine;
    uint32_t* const out = todo + (uint64_t)s * W;
    for (uint32_t i = i0; i < i1; ++i) {
        const uint32_t h = have[i];
        if (h >= k && h < W) out[at++] = i;
    }
    // ---- report ----
    if (t == 0) {
        const uint32_t cnt = scan[kPlanThreads - 1];
        state[s] = cnt;
        report[2 * s] = cnt;
        report[2 * s + 1] = cells - total;
    }
}

// Q0 of square map[j] (rows 0 .. k-1, k * S bytes each) into the top-left quadrant of work
// square j; grid (k, n).
__global__ __launch_bounds__(256) void repair_gather_q0_kernel(const uint8_t* eds, uint8_t* work, const uint32_t* map,
                                                               uint32_t k, uint32_t S) {
    const uint64_t row = 2ull * k * S, sq = 2ull * k * row;
    const uint4* const src = reinterpret_cast<const uint4*>(eds + map[blockIdx.y] * sq + blockIdx.x * row);
    uint4* const dst = reinterpret_cast<uint4*>(work + blockIdx.y * sq + blockIdx.x * row);
    const uint64_t n16 = (uint64_t)k * S / 16;
    for (uint64_t i = threadIdx.x; i < n16; i += 256) dst[i] = src[i];
}

// flags[2 * j] = 1 where square map[j] differs from work square j (flags start at 0);
// grid (blocks per square, n).
__global__ __launch_bounds__(256) void repair_compare_squares_kernel(const uint8_t* eds, const uint8_t* work,
                                                                     const uint32_t* map, uint64_t sq_bytes,
                                                                     uint32_t* flags) {
    const uint4* const a = reinterpret_cast<const uint4*>(eds + map[blockIdx.y] * sq_bytes);
    const uint4* const b = reinterpret_cast<const uint4*>(work + blockIdx.y * sq_bytes);
    uint32_t diff = 0;
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < sq_bytes / 16; i += (uint64_t)gridDim.x * 256ull) {
        const uint4 x = a[i], y = b[i];
        diff |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
    }
    if (__any(diff != 0) && (threadIdx.x & 63u) == 0) flags[2 * blockIdx.y] = 1u;
}

// flags[2 * j + 1] = 1 where the roots computed for work square j (got: roots_bytes per
// square, any alignment) differ from the committed roots of square map[j], or one of the
// square's tree status words (status: words per square, nullable) is non-zero; grid
// (blocks per square, n).
__global__ __launch_bounds__(256) void repair_compare_roots_kernel(const uint8_t* got, const uint32_t* status,
                                                                   const uint8_t* committed, const uint32_t* map,
                                                                   uint32_t roots_bytes, uint32_t words,
                                                                   uint32_t* flags) {
    const uint32_t j = blockIdx.y, i0 = blockIdx.x * 256u + threadIdx.x, step = gridDim.x * 256u;
    const uint8_t* const a = got + (uint64_t)j * roots_bytes;
    const uint8_t* const b = committed + (uint64_t)map[j] * roots_bytes;
    uint32_t diff = 0;
    for (uint32_t i = i0; i < roots_bytes; i += step) diff |= (uint32_t)(a[i] ^ b[i]);
    if (status)
        for (uint32_t i = i0; i < words; i += step) diff |= status[(uint64_t)j * words + i];
    if (__any(diff != 0) && (threadIdx.x & 63u) == 0) flags[2 * j + 1] = 1u;
}

__device__ inline uint64_t sample_cell(const ProofSample& s, uint32_t W) {
    const uint32_t r = s.axis == 0 ? s.index : s.pos, c = s.axis == 0 ? s.pos : s.index;
    return ((uint64_t)s.square * W + r) * W + c;
}

// One lane per sample, from the statuses and the presence map as they stand on entry
// (nothing is written to either here): verdict 1 = this sample sets its cell, 2 = it
// becomes OCCUPIED, 0 = it writes nothing.  prev[i]: the next lower sample of the batch
// that addresses the same cell, or ~0 (the host's); a status-0 sample loses to any
// status-0 sample down that chain.
__global__ __launch_bounds__(256) void scatter_decide_kernel(const ProofSample* samples, const uint32_t* prev,
                                                             const uint32_t* status, const uint8_t* pres, uint32_t W,
                                                             uint32_t n, uint32_t* verdict) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t v = 0;
    if (status[i] == kProofOk) {
        v = 1;
        if (pres[sample_cell(samples[i], W)] != 0) {
            v = 2;
        } else {
            for (uint32_t j = prev[i]; j != ~0u; j = prev[j])  // j strictly decreases
                if (status[j] == kProofOk) {
                    v = 2;
                    break;
                }
        }
    }
    verdict[i] = v;
}

// One wave per sample: verdict 1 copies the share into its cell and sets the presence
// byte, verdict 2 stores kProofOccupied into the status word.
constexpr uint32_t kProofOccupied = 4;
__global__ __launch_bounds__(256) void scatter_apply_kernel(const ProofSample* samples, const uint32_t* verdict,
                                                            const uint8_t* shares, uint8_t* eds, uint8_t* pres,
                                                            uint32_t* status, uint32_t W, uint32_t S, uint32_t n) {
    const uint32_t i = blockIdx.x * 4u + threadIdx.x / 64u, lane = threadIdx.x & 63u;
    if (i >= n) return;
    const uint32_t v = verdict[i];
    if (v == 2u) {
        if (lane == 0) status[i] = kProofOccupied;
        return;
    }
    if (v != 1u) return;
    const uint64_t cell = sample_cell(samples[i], W);
    const uint4* const src = reinterpret_cast<const uint4*>(shares + (uint64_t)i * S);
    uint4* const dst = reinterpret_cast<uint4*>(eds + cell * S);
    for (uint32_t w = lane; w < S / 16; w += 64) dst[w] = src[w];
    if (lane == 0) pres[cell] = 1;
}

}  // namespace

bool repair_plan_supported(uint32_t W) { return W >= 2 && W <= 2048; }

hipError_t launch_repair_plan(uint8_t* d_presence, uint32_t W, uint32_t count, uint32_t axis, bool first,
                              const uint32_t* d_prev_todo, uint32_t* d_todo, uint32_t* d_state, uint32_t* report,
                              hipStream_t st) {
    if (count == 0) return hipSuccess;
    if (!repair_plan_supported(W)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(repair_plan_kernel, dim3(count), dim3(kPlanThreads), 0, st, d_presence, W, W / 2, axis,
                       first ? 1u : 0u, d_prev_todo, d_todo, d_state, report);
    return hipGetLastError();
}

hipError_t launch_repair_gather_q0(const uint8_t* d_eds, uint8_t* d_work, const uint32_t* d_map, uint32_t k, uint32_t S,
                                   uint32_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(repair_gather_q0_kernel, dim3(k, n), dim3(256), 0, st, d_eds, d_work, d_map, k, S);
    return hipGetLastError();
}

hipError_t launch_repair_compare_squares(const uint8_t* d_eds, const uint8_t* d_work, const uint32_t* d_map,
                                         uint64_t sq_bytes, uint32_t n, uint32_t* d_flags, hipStream_t st) {
    if (n == 0) return hipSuccess;
    uint64_t blocks = (sq_bytes / 16 + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(repair_compare_squares_kernel, dim3((uint32_t)blocks, n), dim3(256), 0, st, d_eds, d_work, d_map,
                       sq_bytes, d_flags);
    return hipGetLastError();
}

hipError_t launch_repair_compare_roots(const uint8_t* d_got, const uint32_t* d_status, const uint8_t* d_committed,
                                       const uint32_t* d_map, uint32_t roots_bytes, uint32_t words, uint32_t n,
                                       uint32_t* d_flags, hipStream_t st) {
    if (n == 0) return hipSuccess;
    uint32_t blocks = (roots_bytes + 1023) / 1024;  // 4 bytes per lane
    if (blocks > 64) blocks = 64;
    hipLaunchKernelGGL(repair_compare_roots_kernel, dim3(blocks ? blocks : 1, n), dim3(256), 0, st, d_got, d_status, d_committed, d_map,
                       roots_bytes, words, d_flags);
    return hipGetLastError();
}

hipError_t launch_samples_scatter(const ProofSample* d_samples, const uint32_t* d_prev, uint32_t* d_verdict,
                                  const uint8_t* d_shares, uint8_t* d_eds, uint8_t* d_presence, uint32_t* d_status,
                                  uint32_t W, uint32_t S, uint32_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(scatter_decide_kernel, dim3((n + 255) / 256), dim3(256), 0, st, d_samples, d_prev, d_status,
                       d_presence, W, n, d_verdict);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(scatter_apply_kernel, dim3((n + 3) / 4), dim3(256), 0, st, d_samples, d_verdict, d_shares, d_eds,
                       d_presence, d_status, W, S, n);
    return hipGetLastError();
}

}  // namespace rsm
