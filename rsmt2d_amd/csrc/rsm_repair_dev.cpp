// rsm_repair_dev.cpp -- Repair of device-resident squares: rsm_repair_squares_dev (the
// sweep loop of eds.cpp's fast_repair over a batch of squares that stay in device memory,
// planned by kernels_repair.hip, decoded by the existing decoders, verified as a batch)
// and rsm_samples_scatter_dev (the apply step of rsm_eds_import_samples on the device).
// Contract: include/rsmt2d_hip.h; design: DESIGN.md §5 "Device-resident Repair".
#include "eds_internal.hpp"

#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

using namespace rsm;

static_assert(sizeof(rsm_repair_result) == 16, "rsm_repair_result is four words");
static_assert(RSM_PROOF_OCCUPIED == 4, "the scatter kernel's OCCUPIED word is the C ABI's");

namespace {

// Sections of d_work, each a multiple of 256 bytes from its start.
struct WorkLayout {
    uint64_t todo[2];  // [count][W] words each: the lists of this pass and the one before
    uint64_t state;    // [count] words: the planner's
    uint64_t map;      // [count] words: completed square j of the verification -> square
    uint64_t flags;    // [count][2] words: encoding mismatch, root mismatch
    uint64_t roots;    // [count][2W][root_len]
    uint64_t status;   // [count][2W] words
    uint64_t leaf;     // [count][W * W] leaf records (32 bytes; NMT 64)
    uint64_t copies;   // [count][W][W][S]: Q0 copies, re-extended
    uint64_t total;
};

// The device tree and the layout of (k, S, count, nmt); false beyond the limits.
bool repair_shape(uint32_t k, uint32_t S, uint32_t count, const rsm_nmt_params* nmt, DevTree* t, WorkLayout* out) {
    if (k == 0 || k > 1024 || S == 0 || S % 64 != 0) return false;
    const uint64_t W = 2ull * k;
    if (!device_tree_for(nmt ? rsm_nmt_tree_root : nullptr, const_cast<rsm_nmt_params*>(nmt), (uint32_t)W, t) ||
        !repair_plan_supported((uint32_t)W))
        return false;
    if (W * W * count >= (1ull << 32) || count > 65535) return false;  // one launch of the root kernels
    WorkLayout l{};
    uint64_t at = 0;
    auto take = [&](uint64_t bytes) {
        const uint64_t o = at;
        at += (bytes + 255) / 256 * 256;
        return o;
    };
    l.todo[0] = take(count * W * 4);
    l.todo[1] = take(count * W * 4);
    l.state = take((uint64_t)count * 4);
    l.map = take((uint64_t)count * 4);
    l.flags = take((uint64_t)count * 8);
    l.roots = take(count * 2 * W * t->root_len);
    l.status = take(count * 2 * W * 4);
    l.leaf = take(count * W * W * (t->nmt ? 64 : 32));
    l.copies = take(count * W * W * S);
    l.total = at ? at : 256;
    *out = l;
    return true;
}

// An early return must not hand the lane's pinned staging back while the stream still
// reads or writes it.
struct Drain {
    hipStream_t st;
    bool armed = true;
    ~Drain() {
        if (armed) (void)hipStreamSynchronize(st);
    }
};

}  // namespace

extern "C" {

uint64_t rsm_repair_work_bytes(uint32_t k, uint32_t share_size, uint32_t count, const rsm_nmt_params* nmt) {
    DevTree t;
    WorkLayout l;
    return repair_shape(k, share_size, count, nmt, &t, &l) ? l.total : 0;
}

int rsm_repair_squares_dev(rsm_ctx* ctx, void* d_eds, void* d_presence, uint32_t k, uint32_t share_size, uint32_t count,
                           const rsm_nmt_params* nmt, const void* d_roots, void* d_work, rsm_repair_result* results,
                           void* stream) {
    if (!ctx || k == 0) return fail(RSM_EINVAL, "rsm_repair_squares_dev: bad arguments");
    if (int rc = validate_chunk_size(share_size)) return rc;
    if (share_size == 0) return fail(RSM_EINVAL, "rsm_repair_squares_dev: empty shares");
    DevTree t;
    WorkLayout lay;
    if (!repair_shape(k, share_size, count, nmt, &t, &lay))
        return fail(RSM_EUNSUPPORTED, "rsm_repair_squares_dev: %u squares of width %u%s not supported", count, 2 * k,
                    nmt ? " (NMT)" : "");
    if (count == 0) return RSM_OK;
    if (!d_eds || !d_presence || !d_roots || !d_work || !results)
        return fail(RSM_EINVAL, "rsm_repair_squares_dev: bad arguments");
    if ((reinterpret_cast<uintptr_t>(d_eds) | reinterpret_cast<uintptr_t>(d_presence) | reinterpret_cast<uintptr_t>(d_work)) & 15u)
        return fail(RSM_EINVAL, "rsm_repair_squares_dev: d_eds, d_presence and d_work must be 16-byte aligned");
    if (t.nmt && share_size < t.p.namespace_size) return fail(RSM_ETREE, "data is too short to contain namespace ID");
    if (int rc = use_device(ctx)) return rc;
    hipStream_t st = pick(ctx, stream);
    const uint32_t W = 2 * k, S = share_size, RL = t.root_len;
    const uint64_t sq = (uint64_t)W * W * S, cells = (uint64_t)W * W;
    auto* const eds = static_cast<uint8_t*>(d_eds);
    auto* const pres = static_cast<uint8_t*>(d_presence);
    auto* const work = static_cast<uint8_t*>(d_work);
    uint32_t* const todo[2] = {reinterpret_cast<uint32_t*>(work + lay.todo[0]), reinterpret_cast<uint32_t*>(work + lay.todo[1])};
    uint32_t* const state = reinterpret_cast<uint32_t*>(work + lay.state);
    uint32_t* const map = reinterpret_cast<uint32_t*>(work + lay.map);
    uint32_t* const flags = reinterpret_cast<uint32_t*>(work + lay.flags);

    // pinned staging of a lane: the planner's report (written by the kernel through the
    // mapping), then the verification's map (up) and flags (back)
    LaneGuard g(ctx);
    if (!g.lane) return g.rc;
    hipError_t e;
    if ((e = g.lane->host.ensure((size_t)count * 20)) != hipSuccess) return hip_fail(e, "hipHostMalloc (repair staging)");
    uint32_t* const report = static_cast<uint32_t*>(g.lane->host.ptr);
    uint32_t* const h_map = report + 2 * (size_t)count;
    uint32_t* const h_flags = h_map + count;
    void* report_dev = nullptr;
    if ((e = hipHostGetDevicePointer(&report_dev, report, 0)) != hipSuccess || !report_dev)
        return hip_fail(e == hipSuccess ? hipErrorInvalidValue : e, "hipHostGetDevicePointer (repair staging)");
    Drain drain{st};

    for (uint32_t s = 0; s < count; ++s) results[s] = rsm_repair_result{};
    // The schedule of fast_repair's general loop (eds.cpp): a row pass, then a column pass,
    // each decoding every vector with k <= have < 2k at once.  Every vector is decoded at
    // most once, so at most 2W passes decode anything.
    // A square is finished once it misses nothing, or after two empty lists in a row (no
    // pass can change it any more); the loop ends on a pass that found every square so.
    std::vector<uint8_t> idle(count, 0);
    bool finished = false;
    for (uint32_t pass = 0; pass < 2 * W + 4 && !finished; ++pass) {
        const uint32_t axis = pass & 1u;
        if ((e = launch_repair_plan(pres, W, count, axis, pass == 0, todo[axis ^ 1u], todo[axis], state,
                                    static_cast<uint32_t*>(report_dev), st)) != hipSuccess)
            return hip_fail(e, "repair plan kernel launch");
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "repair stream");
        finished = true;
        for (uint32_t s = 0; s < count; ++s) {
            const uint32_t n = report[2 * s];
            if (n == 0) {
                if (idle[s] < 2) ++idle[s];
                if (report[2 * s + 1] != 0 && idle[s] < 2) finished = false;
                continue;
            }
            if (n > W) return fail(RSM_EDEVICE, "rsm_repair_squares_dev: planner reported %u vectors of %u", n, W);
            if (int rc = launch_decode(ctx, decode_vectors(eds + s * sq, k, S, axis, todo[axis] + (size_t)s * W, n,
                                                           pres + s * cells), st))
                return rc;
            results[s].sweeps++;
            results[s].decoded_vectors += n;
            idle[s] = 0;
            finished = false;
        }
    }
    if (!finished) return fail(RSM_EDEVICE, "rsm_repair_squares_dev: the sweeps did not end within %u passes", 2 * W + 4);

    // the last plan listed nothing anywhere: the report's missing counts are final
    uint32_t n_done = 0;
    for (uint32_t s = 0; s < count; ++s) {
        results[s].missing = report[2 * s + 1];
        results[s].status = results[s].missing ? RSM_REPAIR_STUCK : RSM_REPAIR_OK;
        if (!results[s].missing) h_map[n_done++] = s;
    }
    if (n_done == 0) {
        drain.armed = false;  // synchronised above, nothing enqueued since
        return RSM_OK;
    }
    // Completed squares, as one batch: Q0 copied out and re-extended, compared with the
    // square; the roots of the re-extended copies (the square's own wherever the compare
    // passes, and the compare is consulted first) against the committed ones.
    uint8_t* const copies = work + lay.copies;
    uint8_t* const got = work + lay.roots;
    uint32_t* const status = reinterpret_cast<uint32_t*>(work + lay.status);
    uint32_t* const leaf = reinterpret_cast<uint32_t*>(work + lay.leaf);
    if ((e = hipMemcpyAsync(map, h_map, (size_t)n_done * 4, hipMemcpyHostToDevice, st)) != hipSuccess ||
        (e = hipMemsetAsync(flags, 0, (size_t)n_done * 8, st)) != hipSuccess)
        return hip_fail(e, "repair verification (map, flags)");
    if ((e = launch_repair_gather_q0(eds, copies, map, k, S, n_done, st)) != hipSuccess)
        return hip_fail(e, "repair Q0 gather kernel launch");
    if (int rc = extend_squares(ctx, copies, k, S, n_done, st)) return rc;
    if ((e = launch_repair_compare_squares(eds, copies, map, sq, n_done, flags, st)) != hipSuccess)
        return hip_fail(e, "repair encoding compare kernel launch");
    e = t.nmt ? launch_nmt_roots(copies, W, S, t.p.namespace_size, t.p.square_size, t.p.ignore_max_namespace, leaf, got,
                                 status, st, n_done)
              : launch_roots(copies, W, S, n_done, leaf, got, st);
    if (e != hipSuccess) return hip_fail(e, "repair roots kernel launch");
    if ((e = launch_repair_compare_roots(got, t.nmt ? status : nullptr, static_cast<const uint8_t*>(d_roots), map,
                                         2 * W * RL, 2 * W, n_done, flags, st)) != hipSuccess)
        return hip_fail(e, "repair root compare kernel launch");
    if ((e = hipMemcpyAsync(h_flags, flags, (size_t)n_done * 8, hipMemcpyDeviceToHost, st)) != hipSuccess)
        return hip_fail(e, "D2H repair flags");
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "repair stream");
    drain.armed = false;
    if (int rc = check_queue_reports(ctx, st)) return rc;  // a re-extension that timed out is no verdict
    for (uint32_t j = 0; j < n_done; ++j)
        results[h_map[j]].status = h_flags[2 * j] ? RSM_REPAIR_ENCODING : h_flags[2 * j + 1] ? RSM_REPAIR_ROOTS : RSM_REPAIR_OK;
    return RSM_OK;
}

int rsm_samples_scatter_dev(rsm_ctx* ctx, void* d_eds, void* d_presence, uint32_t k, uint32_t share_size, uint32_t count,
                            const rsm_sample* samples, uint32_t n, const void* d_shares, void* d_status, void* stream) {
    if (!ctx || k == 0 || k > 32768u) return fail(RSM_EINVAL, "rsm_samples_scatter_dev: bad arguments");
    if (int rc = validate_chunk_size(share_size)) return rc;
    if (share_size == 0) return fail(RSM_EINVAL, "rsm_samples_scatter_dev: empty shares");
    if (n > (1u << 24)) return fail(RSM_EINVAL, "rsm_samples_scatter_dev: at most %u samples per call", 1u << 24);
    if (n == 0 || count == 0) return RSM_OK;
    if (!d_eds || !d_presence || !samples || !d_shares || !d_status)
        return fail(RSM_EINVAL, "rsm_samples_scatter_dev: bad arguments");
    if ((reinterpret_cast<uintptr_t>(d_eds) | reinterpret_cast<uintptr_t>(d_shares)) & 15u)
        return fail(RSM_EINVAL, "rsm_samples_scatter_dev: d_eds and d_shares must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_status) & 3u)
        return fail(RSM_EINVAL, "rsm_samples_scatter_dev: d_status must be 4-byte aligned");
    const uint32_t W = 2 * k;
    for (uint32_t i = 0; i < n; ++i)
        if (samples[i].square >= count || samples[i].axis > 1 || samples[i].index >= W || samples[i].pos >= W)
            return fail(RSM_EINVAL, "rsm_samples_scatter_dev: sample %u (square %u, axis %u, index %u, pos %u) is out of range",
                        i, samples[i].square, samples[i].axis, samples[i].index, samples[i].pos);
    // prev[i]: the next lower sample of the batch that addresses the same cell (~0: none)
    std::vector<std::pair<uint64_t, uint32_t>> by_cell(n);
    for (uint32_t i = 0; i < n; ++i) {
        const rsm_sample& s = samples[i];
        const uint64_t r = s.axis == RSM_AXIS_ROW ? s.index : s.pos, c = s.axis == RSM_AXIS_ROW ? s.pos : s.index;
        by_cell[i] = {((uint64_t)s.square * W + r) * W + c, i};
    }
    std::sort(by_cell.begin(), by_cell.end());
    // one upload: samples | prev | the decide launch's verdict words
    std::vector<uint32_t> pack((size_t)n * 6, 0u);
    memcpy(pack.data(), samples, (size_t)n * sizeof(rsm_sample));
    uint32_t* const prev = pack.data() + (size_t)n * 4;
    for (uint32_t j = 0; j < n; ++j)
        prev[by_cell[j].second] = j && by_cell[j - 1].first == by_cell[j].first ? by_cell[j - 1].second : ~0u;
    if (int rc = use_device(ctx)) return rc;
    hipStream_t st = pick(ctx, stream);
    StreamScratch& ss = stream_scratch(ctx, st);
    std::lock_guard<std::mutex> lk(ss.mu);
    const void* d = nullptr;
    if (int rc = stage_bytes(st, ss, pack.data(), pack.size() * 4, &d)) return rc;
    auto* const words = static_cast<uint32_t*>(const_cast<void*>(d));
    const hipError_t e = launch_samples_scatter(reinterpret_cast<const ProofSample*>(words), words + (size_t)n * 4,
                                                words + (size_t)n * 5, static_cast<const uint8_t*>(d_shares),
                                                static_cast<uint8_t*>(d_eds), static_cast<uint8_t*>(d_presence),
                                                static_cast<uint32_t*>(d_status), W, share_size, n, st);
    return e == hipSuccess ? RSM_OK : hip_fail(e, "sample scatter kernel launch");
}

}  // extern "C"
