// kernels_repair.hip -- the device half of rsm_repair_squares_dev and
// rsm_samples_scatter_dev (DESIGN.md §5 "Device-resident Repair"): the sweep planner over
// [count][W][W] presence bytes, the batch verification's gather and compare kernels, and
// the decide / apply pair that sets verified samples into device squares; and of
// rsm_repair_squares_checked_dev / rsm_vectors_gather_dev ("Checked Repair"): the check
// planner, the verdict kernel and the vector gather (the list-driven leaf and tree kernels
// are in kernels_sha.hip and kernels_nmt.hip).
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
// skip (nullable; the checked call's): a square whose word is non-zero has dropped out --
// nothing of it is marked, listed or read, and it reports an empty list.
__global__ __launch_bounds__(kPlanThreads) void repair_plan_kernel(uint8_t* pres, uint32_t W, uint32_t k, uint32_t axis,
                                                                    uint32_t first, const uint32_t* prev_todo,
                                                                    uint32_t* todo, uint32_t* state, uint32_t* report,
                                                                    const uint32_t* skip) {
    __shared__ uint32_t have[2048];
    __shared__ uint32_t scan[kPlanThreads];
    __shared__ uint32_t total;
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    if (skip && skip[s]) {  // the whole workgroup, before any barrier
        if (t == 0) state[s] = report[2 * s] = report[2 * s + 1] = 0u;
        return;
    }
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

// ---- checked Repair (rsm_repair_squares_checked_dev) --------------------------------
// The lists of one check stage, one workgroup per square: list [count][2][W] (rows, then
// columns; ascending), cnt [count][2], checked [count][2][W] bytes (a listed vector's byte
// becomes 1: every vector is listed once per call).  A square whose skip word is set, or
// (modes 1, 2) whose last plan listed nothing, lists nothing.
//   mode 0  every complete vector of either axis, from the presence bytes alone (the
//           entry check); report[3 s + 2] = the cells missing
//   mode 1  the vectors the last plan listed for `axis` (todo; their count is the state
//           word): the ones this pass decoded
//   mode 2  the vectors of the other axis that this pass completed: a cell counts when
//           its presence byte is set or it lies in a vector of todo (the pass's cells
//           are marked by the next plan only), and the vector is not checked yet
// report (pinned host memory through its device mapping): three words per square, the
// two counts and mode 0's missing cells.
__global__ __launch_bounds__(kPlanThreads) void repair_check_plan_kernel(const uint8_t* pres, uint32_t W, uint32_t mode,
                                                                          uint32_t axis, const uint32_t* todo,
                                                                          const uint32_t* state, const uint32_t* skip,
                                                                          uint8_t* checked, uint32_t* list,
                                                                          uint32_t* cnt, uint32_t* report) {
    __shared__ uint32_t have[2048];
    __shared__ uint8_t dec[2048];
    __shared__ uint32_t wave_cnt[kPlanThreads / 64];
    const uint32_t s = blockIdx.x, t = threadIdx.x, wv = t >> 6, lane = t & 63u;
    const uint32_t n_dec = mode == 0 ? 0u : state[s];
    uint8_t* const ck = checked + (uint64_t)s * 2 * W;
    uint32_t* const lst = list + (uint64_t)s * 2 * W;
    if (skip[s] || (mode != 0 && n_dec == 0)) {  // the whole workgroup, before any barrier
        if (t == 0) cnt[2 * s] = cnt[2 * s + 1] = report[3 * s] = report[3 * s + 1] = 0u;
        return;
    }
    const uint32_t* const td = todo + (uint64_t)s * W;
    if (mode == 1) {
        for (uint32_t i = t; i < n_dec; i += kPlanThreads) {
            const uint32_t v = td[i];
            lst[axis * W + i] = v;
            ck[axis * W + v] = 1;
        }
        if (t == 0) {
            cnt[2 * s + axis] = report[3 * s + axis] = n_dec;
            cnt[2 * s + (axis ^ 1u)] = report[3 * s + (axis ^ 1u)] = 0u;
        }
        return;
    }
    const uint8_t* const p = pres + (uint64_t)s * W * W;
    for (uint32_t i = t; i < W; i += kPlanThreads) dec[i] = 0;
    __syncthreads();
    for (uint32_t i = t; i < n_dec; i += kPlanThreads) dec[td[i]] = 1;
    __syncthreads();
    const uint32_t da = mode == 2 ? axis : 2u;  // the axis of the decoded vectors (2: none)
    uint32_t missing = 0;
    for (uint32_t o = (mode == 2 ? axis ^ 1u : 0u); o < (mode == 2 ? (axis ^ 1u) + 1u : 2u); ++o) {
        // ---- count: have[i] of the unchecked vectors of axis o ----
        if (o == 0) {  // a wave per row, its lanes along the row
            for (uint32_t r = wv; r < W; r += kPlanThreads / 64) {
                if (mode == 2 && ck[r]) {  // wave-uniform
                    if (lane == 0) have[r] = 0;
                    continue;
                }
                uint32_t n = 0;
                for (uint32_t c0 = 0; c0 < W; c0 += 64) {
                    const uint32_t c = c0 + lane;
                    const bool on = c < W && (p[(uint64_t)r * W + c] != 0 || (da == 1 && dec[c]));
                    n += (uint32_t)__popcll(__ballot(on));
                }
                if (lane == 0) have[r] = n;
            }
        } else {  // a lane per column: a wave reads consecutive bytes of one row at a time
            for (uint32_t c = t; c < W; c += kPlanThreads) {
                uint32_t n = 0;
                if (!(mode == 2 && ck[W + c]))
                    for (uint32_t r = 0; r < W; ++r) n += (p[(uint64_t)r * W + c] != 0 || (da == 0 && dec[r])) ? 1u : 0u;
                have[c] = n;
            }
        }
        __syncthreads();
        // ---- list: the complete unchecked ones, ascending, 256 indices at a time ----
        uint32_t at = 0;  // the same in every lane
        for (uint32_t i0 = 0; i0 < W; i0 += kPlanThreads) {
            const uint32_t i = i0 + t;
            const bool take = i < W && have[i] == W && ck[o * W + i] == 0;
            const uint64_t b = __ballot(take);
            if (lane == 0) wave_cnt[wv] = (uint32_t)__popcll(b);
            __syncthreads();
            uint32_t before = 0, all = 0;
            for (uint32_t w = 0; w < kPlanThreads / 64; ++w) {
                before += w < wv ? wave_cnt[w] : 0u;
                all += wave_cnt[w];
            }
            if (take) {
                lst[o * W + at + before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = i;
                ck[o * W + i] = 1;
            }
            at += all;
            __syncthreads();
        }
        if (mode == 0 && o == 0)
            for (uint32_t i = t; i < W; i += kPlanThreads) missing += W - have[i];
        if (t == 0) cnt[2 * s + o] = report[3 * s + o] = at;
        __syncthreads();  // have[] is read no more: the next axis may count
    }
    if (t == 0 && mode == 2) cnt[2 * s + axis] = report[3 * s + axis] = 0u;
    if (mode == 0) {  // the cells missing on entry, summed over the rows
        __syncthreads();
        if (t == 0) have[0] = 0;
        __syncthreads();
        if (missing) atomicAdd(&have[0], missing);
        __syncthreads();
        if (t == 0) report[3 * s + 2] = have[0];
    }
}

// The verdict of one check stage, one workgroup per square: over the listed vectors the
// minimum of key = (2 index + axis) << 2 | reason, reason = the tree kernel's verdict word
// (kByzRoot, kByzTree) where non-zero, else kByzEncoding where the parity flag is set; ~0
// when every listed vector passed.  A minimum, so no lane order shows in it; row i comes
// before column i.  report[2 s] = the key; a failing square's skip word becomes 1.
// stage2 != 0 (the lists are the vectors a pass of `axis` completed): a failing square's
// decoded vectors (todo, state, as the pass's plan left them) all passed stage 1, and
// their cells are marked present here, since no later plan will; report[2 s + 1] = the
// cells that were missing among them.
__global__ __launch_bounds__(kPlanThreads) void repair_check_pick_kernel(const uint32_t* list, const uint32_t* cnt,
                                                                          const uint32_t* verdict, const uint32_t* parity,
                                                                          uint32_t W, uint32_t stage2, uint32_t axis,
                                                                          const uint32_t* todo, const uint32_t* state,
                                                                          uint8_t* pres, uint32_t* skip, uint32_t* report) {
    __shared__ uint32_t best, marked;
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    const uint32_t n0 = cnt[2 * s], n1 = cnt[2 * s + 1];
    if (n0 + n1 == 0) {
        if (t == 0) {
            report[2 * s] = ~0u;
            report[2 * s + 1] = 0u;
        }
        return;
    }
    if (t == 0) {
        best = ~0u;
        marked = 0u;
    }
    __syncthreads();
    uint32_t key = ~0u;
    for (uint32_t e = t; e < n0 + n1; e += kPlanThreads) {
        const uint32_t ax = e >= n0 ? 1u : 0u;
        const uint64_t at = (uint64_t)s * 2 * W + ax * W + (e - ax * n0);
        const uint32_t v = verdict[at];
        const uint32_t reason = v ? v : (parity[at] ? kByzEncoding : 0u);
        if (reason) {
            const uint32_t mine = ((2u * list[at] + ax) << 2) | reason;
            key = mine < key ? mine : key;
        }
    }
    if (key != ~0u) atomicMin(&best, key);
    __syncthreads();
    if (best != ~0u && stage2) {
        uint8_t* const p = pres + (uint64_t)s * W * W;
        const uint32_t* const td = todo + (uint64_t)s * W;
        uint32_t fresh = 0;
        for (uint32_t i = t; i < state[s] * W; i += kPlanThreads) {
            const uint32_t v = td[i / W], e = i % W;
            uint8_t* const c = p + (axis == 0 ? (uint64_t)v * W + e : (uint64_t)e * W + v);
            if (*c == 0) {  // a cell lies in one decoded vector only: no other lane writes it
                *c = 1;
                ++fresh;
            }
        }
        if (fresh) atomicAdd(&marked, fresh);
        __syncthreads();
    }
    if (t == 0) {
        report[2 * s] = best;
        report[2 * s + 1] = marked;
        if (best != ~0u) skip[s] = 1u;
    }
}

// Vector refs[i] (square, axis, index) of the squares, packed: shares [n][W][S] (16-byte
// words) and present [n][W], the presence bytes as they stand.  One workgroup per vector.
__global__ __launch_bounds__(256) void vectors_gather_kernel(const uint8_t* eds, const uint8_t* pres, uint32_t W,
                                                             uint32_t S, const RootRef* refs, uint8_t* shares,
                                                             uint8_t* present) {
    const RootRef ref = refs[blockIdx.x];
    const uint64_t sq = (uint64_t)ref.square * W * W;
    const uint32_t per = S / 16;
    for (uint32_t i = threadIdx.x; i < W * per; i += 256) {
        const uint32_t pos = i / per, w = i - pos * per;
        const uint64_t cell = sq + (ref.axis == 0 ? (uint64_t)ref.index * W + pos : (uint64_t)pos * W + ref.index);
        reinterpret_cast<uint4*>(shares + ((uint64_t)blockIdx.x * W + pos) * S)[w] =
            reinterpret_cast<const uint4*>(eds + cell * S)[w];
    }
    for (uint32_t pos = threadIdx.x; pos < W; pos += 256) {
        const uint64_t cell = sq + (ref.axis == 0 ? (uint64_t)ref.index * W + pos : (uint64_t)pos * W + ref.index);
        present[(uint64_t)blockIdx.x * W + pos] = pres[cell];
    }
}

}  // namespace

hipError_t launch_repair_check_plan(const uint8_t* d_presence, uint32_t W, uint32_t count, uint32_t mode, uint32_t axis,
                                    const uint32_t* d_todo, const uint32_t* d_state, const uint32_t* d_skip,
                                    uint8_t* d_checked, uint32_t* d_list, uint32_t* d_cnt, uint32_t* report,
                                    hipStream_t st) {
    if (count == 0) return hipSuccess;
    if (!repair_plan_supported(W) || mode > 2 || axis > 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(repair_check_plan_kernel, dim3(count), dim3(kPlanThreads), 0, st, d_presence, W, mode, axis, d_todo,
                       d_state, d_skip, d_checked, d_list, d_cnt, report);
    return hipGetLastError();
}

hipError_t launch_repair_check_pick(const uint32_t* d_list, const uint32_t* d_cnt, const uint32_t* d_verdict,
                                    const uint32_t* d_parity, uint32_t W, uint32_t count, bool stage2, uint32_t axis,
                                    const uint32_t* d_todo, const uint32_t* d_state, uint8_t* d_presence,
                                    uint32_t* d_skip, uint32_t* report, hipStream_t st) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(repair_check_pick_kernel, dim3(count), dim3(kPlanThreads), 0, st, d_list, d_cnt, d_verdict,
                       d_parity, W, stage2 ? 1u : 0u, axis, d_todo, d_state, d_presence, d_skip, report);
    return hipGetLastError();
}

hipError_t launch_vectors_gather(const uint8_t* d_eds, const uint8_t* d_presence, uint32_t W, uint32_t S,
                                 const RootRef* d_refs, uint32_t n, uint8_t* d_shares, uint8_t* d_present,
                                 hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(vectors_gather_kernel, dim3(n), dim3(256), 0, st, d_eds, d_presence, W, S, d_refs, d_shares,
                       d_present);
    return hipGetLastError();
}

bool repair_plan_supported(uint32_t W) { return W >= 2 && W <= 2048; }

hipError_t launch_repair_plan(uint8_t* d_presence, uint32_t W, uint32_t count, uint32_t axis, bool first,
                              const uint32_t* d_prev_todo, uint32_t* d_todo, uint32_t* d_state, uint32_t* report,
                              hipStream_t st, const uint32_t* d_skip) {
    if (count == 0) return hipSuccess;
    if (!repair_plan_supported(W)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(repair_plan_kernel, dim3(count), dim3(kPlanThreads), 0, st, d_presence, W, W / 2, axis,
                       first ? 1u : 0u, d_prev_todo, d_todo, d_state, report, d_skip);
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
