// rsm_repair_dev.cpp -- Repair of device-resident squares: rsm_repair_squares_dev (the
// sweep loop of eds.cpp's fast_repair over a batch of squares that stay in device memory,
// planned by kernels_repair.hip, decoded by the existing decoders, verified as a batch),
// rsm_repair_squares_checked_dev (the same passes with every vector checked against its
// root and encoding when it becomes complete, so a bad one is named) with
// rsm_vectors_gather_dev, and rsm_samples_scatter_dev (the apply step of
// rsm_eds_import_samples on the device).
// Contract: include/rsmt2d_hip.h; design: DESIGN.md §5 "Device-resident Repair", "Checked Repair".
#include "eds_internal.hpp"

#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

using namespace rsm;

static_assert(sizeof(rsm_repair_result) == 16, "rsm_repair_result is four words");
static_assert(sizeof(rsm_repair_check) == 24, "rsm_repair_check is six words");
static_assert(RSM_BYZ_ROOT == kByzRoot && RSM_BYZ_ENCODING == kByzEncoding && RSM_BYZ_TREE == kByzTree,
              "the check kernels' reason words are the C ABI's");
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

// Sections of the checked call's d_work, each a multiple of 256 bytes from its start.
struct CheckedLayout {
    uint64_t todo[2];   // [count][W] words each, as above
    uint64_t state;     // [count] words: the planner's
    uint64_t skip;      // [count] words: non-zero = the square is BYZANTINE and has dropped out
    uint64_t hashed;    // [count] words: leaf records computed
    uint64_t cnt;       // [count][2] words: this stage's list lengths (rows, columns)
    uint64_t checked;   // [count][2][W] bytes: the vector has been listed for its check
    uint64_t recorded;  // [count][ceil(W * W / 32)] words: one bit per cell with a leaf record
    uint64_t zero_end;  // everything from `skip` to here starts a call zeroed
    uint64_t list;      // [count][2][W] words: this stage's vectors
    uint64_t verdict;   // [count][2][W] words: the tree kernel's
    uint64_t parity;    // [count][2][W] words: the parity compare's
    uint64_t leaf;      // [count][W * W] leaf records (32 bytes; NMT 64)
    uint64_t scratch;   // [W][W][S]: re-encoded parity, one square at a time
    uint64_t total;
};

bool checked_shape(uint32_t k, uint32_t S, uint32_t count, const rsm_nmt_params* nmt, DevTree* t, CheckedLayout* out) {
    WorkLayout unchecked;
    if (!repair_shape(k, S, count, nmt, t, &unchecked)) return false;  // the same limits
    const uint64_t W = 2ull * k;
    CheckedLayout l{};
    uint64_t at = 0;
    auto take = [&](uint64_t bytes) {
        const uint64_t o = at;
        at += (bytes + 255) / 256 * 256;
        return o;
    };
    l.todo[0] = take(count * W * 4);
    l.todo[1] = take(count * W * 4);
    l.state = take((uint64_t)count * 4);
    l.skip = take((uint64_t)count * 4);
    l.hashed = take((uint64_t)count * 4);
    l.cnt = take((uint64_t)count * 8);
    l.checked = take(count * 2 * W);
    l.recorded = take(count * ((W * W + 31) / 32) * 4);
    l.zero_end = at;
    l.list = take(count * 2 * W * 4);
    l.verdict = take(count * 2 * W * 4);
    l.parity = take(count * 2 * W * 4);
    l.leaf = take(count * W * W * (t->nmt ? 64 : 32));
    l.scratch = take(W * W * S);
    l.total = at;
    *out = l;
    return true;
}

// The argument checks both repair calls make before any device use; `extra_ok`: the
// call's further host operands are there.
int repair_args(const char* fn, rsm_ctx* ctx, const void* d_eds, const void* d_presence, uint32_t k, uint32_t share_size,
                uint32_t count, const rsm_nmt_params* nmt, const void* d_roots, const void* d_work, const void* results,
                bool extra_ok, bool shape_ok, const DevTree& t, bool* nothing) {
    *nothing = false;
    if (!ctx || k == 0) return fail(RSM_EINVAL, "%s: bad arguments", fn);
    if (int rc = validate_chunk_size(share_size)) return rc;
    if (share_size == 0) return fail(RSM_EINVAL, "%s: empty shares", fn);
    if (!shape_ok)
        return fail(RSM_EUNSUPPORTED, "%s: %u squares of width %u%s not supported", fn, count, 2 * k, nmt ? " (NMT)" : "");
    if (count == 0) {
        *nothing = true;
        return RSM_OK;
    }
    if (!d_eds || !d_presence || !d_roots || !d_work || !results || !extra_ok) return fail(RSM_EINVAL, "%s: bad arguments", fn);
    if ((reinterpret_cast<uintptr_t>(d_eds) | reinterpret_cast<uintptr_t>(d_presence) | reinterpret_cast<uintptr_t>(d_work)) & 15u)
        return fail(RSM_EINVAL, "%s: d_eds, d_presence and d_work must be 16-byte aligned", fn);
    if (t.nmt && share_size < t.p.namespace_size) return fail(RSM_ETREE, "data is too short to contain namespace ID");
    return RSM_OK;
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
    DevTree t;
    WorkLayout lay;
    const bool shape_ok = k != 0 && repair_shape(k, share_size, count, nmt, &t, &lay);
    bool nothing;
    if (int rc = repair_args("rsm_repair_squares_dev", ctx, d_eds, d_presence, k, share_size, count, nmt, d_roots, d_work,
                             results, true, shape_ok, t, &nothing))
        return rc;
    if (nothing) return RSM_OK;
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

uint64_t rsm_repair_checked_work_bytes(uint32_t k, uint32_t share_size, uint32_t count, const rsm_nmt_params* nmt) {
    DevTree t;
    CheckedLayout l;
    return checked_shape(k, share_size, count, nmt, &t, &l) ? l.total : 0;
}

int rsm_repair_squares_checked_dev(rsm_ctx* ctx, void* d_eds, void* d_presence, uint32_t k, uint32_t share_size,
                                   uint32_t count, const rsm_nmt_params* nmt, const void* d_roots, void* d_work,
                                   rsm_repair_result* results, rsm_repair_check* checks, void* stream) {
    static const char* const fn = "rsm_repair_squares_checked_dev";
    DevTree t;
    CheckedLayout lay;
    const bool shape_ok = k != 0 && checked_shape(k, share_size, count, nmt, &t, &lay);
    bool nothing;
    if (int rc = repair_args(fn, ctx, d_eds, d_presence, k, share_size, count, nmt, d_roots, d_work, results,
                             checks != nullptr, shape_ok, t, &nothing))
        return rc;
    if (nothing) return RSM_OK;
    if (int rc = use_device(ctx)) return rc;
    hipStream_t st = pick(ctx, stream);
    const uint32_t W = 2 * k, S = share_size;
    const uint64_t sq = (uint64_t)W * W * S, cells = (uint64_t)W * W;
    auto* const eds = static_cast<uint8_t*>(d_eds);
    auto* const pres = static_cast<uint8_t*>(d_presence);
    auto* const work = static_cast<uint8_t*>(d_work);
    auto words = [&](uint64_t off) { return reinterpret_cast<uint32_t*>(work + off); };
    uint32_t* const todo[2] = {words(lay.todo[0]), words(lay.todo[1])};
    uint32_t *const state = words(lay.state), *const skip = words(lay.skip), *const hashed = words(lay.hashed);
    uint32_t *const cnt = words(lay.cnt), *const recorded = words(lay.recorded), *const list = words(lay.list);
    uint32_t *const verdict = words(lay.verdict), *const parity = words(lay.parity), *const leaf = words(lay.leaf);
    uint8_t *const checked = work + lay.checked, *const scratch = work + lay.scratch;
    const uint8_t* const committed = static_cast<const uint8_t*>(d_roots);

    // pinned staging of a lane, written by the kernels through the mapping: the planner's
    // report [2], a check stage's list lengths and the entry check's missing cells [3], its
    // verdict key and the cells it marked [2]; then the records computed [1] (a copy at the end)
    LaneGuard g(ctx);
    if (!g.lane) return g.rc;
    hipError_t e;
    if ((e = g.lane->host.ensure((size_t)count * 32)) != hipSuccess) return hip_fail(e, "hipHostMalloc (repair staging)");
    uint32_t* const report = static_cast<uint32_t*>(g.lane->host.ptr);
    uint32_t* const lens = report + 2 * (size_t)count;
    uint32_t* const keys = lens + 3 * (size_t)count;
    uint32_t* const h_hashed = keys + 2 * (size_t)count;
    void* mapped = nullptr;
    if ((e = hipHostGetDevicePointer(&mapped, report, 0)) != hipSuccess || !mapped)
        return hip_fail(e == hipSuccess ? hipErrorInvalidValue : e, "hipHostGetDevicePointer (repair staging)");
    uint32_t* const report_dev = static_cast<uint32_t*>(mapped);
    uint32_t* const lens_dev = report_dev + 2 * (size_t)count;
    uint32_t* const keys_dev = lens_dev + 3 * (size_t)count;
    Drain drain{st};

    for (uint32_t s = 0; s < count; ++s) {
        results[s] = rsm_repair_result{};
        checks[s] = rsm_repair_check{};
    }
    if ((e = hipMemsetAsync(work + lay.skip, 0, lay.zero_end - lay.skip, st)) != hipSuccess)
        return hip_fail(e, "repair check state (memset)");

    std::vector<uint8_t> idle(count, 0), dropped(count, 0);
    std::vector<uint32_t> n_list(2 * (size_t)count, 0u), last_missing(count, 0u);
    // One check stage over the vectors the check planner just listed (n_list: their counts
    // per square and axis, as the host knows them): leaf records of the cells that have none,
    // every tree of the batch in one launch with its root compare, per square and axis a
    // re-encode into the scratch square and the parity compare, then the verdict.
    // plan2: the launch of stage 2's check plan follows stage 1's verdict on the stream (the
    // verdict kernel has set the failing squares' skip words by then), so one wait serves both.
    auto run_checks = [&](bool stage2, uint32_t axis, bool plan2) -> int {
        uint32_t max_n = 0;
        for (uint32_t s = 0; s < count; ++s) max_n = std::max(max_n, n_list[2 * s] + n_list[2 * s + 1]);
        if (max_n == 0) return RSM_OK;
        hipError_t r;
        r = t.nmt ? launch_nmt_list_leaves(eds, W, S, t.p.namespace_size, t.p.square_size, count, max_n, list, cnt, recorded,
                                           hashed, leaf, st)
                  : launch_list_leaf_hashes(eds, W, S, count, max_n, list, cnt, recorded, hashed, leaf, st);
        if (r != hipSuccess) return hip_fail(r, "repair check leaf kernel launch");
        r = t.nmt ? launch_nmt_list_tree_check(leaf, W, t.p.namespace_size, t.p.ignore_max_namespace, count, max_n, list, cnt,
                                               committed, verdict, st)
                  : launch_list_tree_check(leaf, W, count, max_n, list, cnt, committed, verdict, st);
        if (r != hipSuccess) return hip_fail(r, "repair check tree kernel launch");
        for (uint32_t s = 0; s < count; ++s)
            for (uint32_t a = 0; a < 2; ++a) {
                const uint32_t n = n_list[2 * s + a];
                if (n == 0) continue;
                if (n > W) return fail(RSM_EDEVICE, "%s: the check planner listed %u vectors of %u", fn, n, W);
                const uint32_t* const idx = list + ((size_t)s * 2 + a) * W;
                if (int rc = launch_encode(ctx, indexed_vectors(eds + s * sq, k, S, a, idx, n, scratch), st)) return rc;
                if ((r = launch_compare_parity(eds + s * sq, scratch, k, S, a, idx, n, parity + ((size_t)s * 2 + a) * W,
                                               st)) != hipSuccess)
                    return hip_fail(r, "repair check parity compare kernel launch");
            }
        if ((r = launch_repair_check_pick(list, cnt, verdict, parity, W, count, stage2, axis, todo[axis], state, pres, skip,
                                          keys_dev, st)) != hipSuccess)
            return hip_fail(r, "repair check verdict kernel launch");
        if (plan2 && (r = launch_repair_check_plan(pres, W, count, 2, axis, todo[axis], state, skip, checked, list, cnt,
                                                   lens_dev, st)) != hipSuccess)
            return hip_fail(r, "repair check plan kernel launch");
        if ((r = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(r, "repair stream");
        for (uint32_t s = 0; s < count; ++s) {
            const uint32_t n = n_list[2 * s] + n_list[2 * s + 1];
            if (n == 0) continue;
            checks[s].checked_vectors += n;
            const uint32_t key = keys[2 * s];
            if (key == ~0u) continue;
            dropped[s] = 1;
            results[s].status = RSM_REPAIR_BYZANTINE;
            results[s].missing = last_missing[s] - keys[2 * s + 1];
            checks[s].reason = key & 3u;
            checks[s].axis = (key >> 2) & 1u;
            checks[s].index = key >> 3;
            checks[s].round = results[s].sweeps;
        }
        return RSM_OK;
    };
    // a check plan whose counts the host does not know yet: run it, wait, read them
    auto plan_checks = [&](uint32_t mode, uint32_t axis) -> int {
        hipError_t r = launch_repair_check_plan(pres, W, count, mode, axis, todo[axis], state, skip, checked, list, cnt,
                                                lens_dev, st);
        if (r != hipSuccess) return hip_fail(r, "repair check plan kernel launch");
        if ((r = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(r, "repair stream");
        for (uint32_t s = 0; s < count; ++s) {
            n_list[2 * s] = dropped[s] ? 0u : lens[3 * s];
            n_list[2 * s + 1] = dropped[s] ? 0u : lens[3 * s + 1];
        }
        return RSM_OK;
    };

    // round 0: the vectors complete on entry
    if (int rc = plan_checks(0, 0)) return rc;
    for (uint32_t s = 0; s < count; ++s) last_missing[s] = lens[3 * s + 2];
    if (int rc = run_checks(false, 0, false)) return rc;

    // The passes of rsm_repair_squares_dev (above), each followed by its two check stages.
    bool finished = false;
    std::vector<uint32_t> n_pass(count, 0u);
    for (uint32_t pass = 0; pass < 2 * W + 4 && !finished; ++pass) {
        const uint32_t axis = pass & 1u;
        if ((e = launch_repair_plan(pres, W, count, axis, pass == 0, todo[axis ^ 1u], todo[axis], state, report_dev, st,
                                    skip)) != hipSuccess)
            return hip_fail(e, "repair plan kernel launch");
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "repair stream");
        finished = true;
        bool decoded = false;
        for (uint32_t s = 0; s < count; ++s) {
            n_pass[s] = 0;
            if (dropped[s]) continue;
            const uint32_t n = report[2 * s];
            last_missing[s] = report[2 * s + 1];
            if (n == 0) {
                if (idle[s] < 2) ++idle[s];
                if (report[2 * s + 1] != 0 && idle[s] < 2) finished = false;
                continue;
            }
            if (n > W) return fail(RSM_EDEVICE, "%s: planner reported %u vectors of %u", fn, n, W);
            if (int rc = launch_decode(ctx, decode_vectors(eds + s * sq, k, S, axis, todo[axis] + (size_t)s * W, n,
                                                           pres + s * cells), st))
                return rc;
            results[s].sweeps++;
            results[s].decoded_vectors += n;
            idle[s] = 0;
            n_pass[s] = n;
            finished = false;
            decoded = true;
        }
        if (!decoded) continue;
        // stage 1: the decoded vectors (their counts are the plan's)
        if ((e = launch_repair_check_plan(pres, W, count, 1, axis, todo[axis], state, skip, checked, list, cnt, lens_dev,
                                          st)) != hipSuccess)
            return hip_fail(e, "repair check plan kernel launch");
        for (uint32_t s = 0; s < count; ++s) {
            n_list[2 * s + axis] = n_pass[s];
            n_list[2 * s + (axis ^ 1u)] = 0;
        }
        if (int rc = run_checks(false, axis, true)) return rc;
        // stage 2: the vectors of the other axis that this pass completed, in the squares
        // whose stage 1 was clean (the others' skip words are set, and they listed nothing)
        for (uint32_t s = 0; s < count; ++s) {
            n_list[2 * s] = dropped[s] ? 0u : lens[3 * s];
            n_list[2 * s + 1] = dropped[s] ? 0u : lens[3 * s + 1];
        }
        if (int rc = run_checks(true, axis, false)) return rc;
    }
    if (!finished) return fail(RSM_EDEVICE, "%s: the sweeps did not end within %u passes", fn, 2 * W + 4);

    if ((e = hipMemcpyAsync(h_hashed, hashed, (size_t)count * 4, hipMemcpyDeviceToHost, st)) != hipSuccess)
        return hip_fail(e, "D2H repair check counters");
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "repair stream");
    drain.armed = false;
    for (uint32_t s = 0; s < count; ++s) {
        checks[s].hashed_cells = h_hashed[s];
        if (dropped[s]) continue;
        // the last plan listed nothing anywhere: the report's missing counts are final
        results[s].missing = report[2 * s + 1];
        results[s].status = results[s].missing ? RSM_REPAIR_STUCK : RSM_REPAIR_OK;
    }
    return RSM_OK;
}

int rsm_vectors_gather_dev(rsm_ctx* ctx, const void* d_eds, const void* d_presence, uint32_t k, uint32_t share_size,
                           uint32_t count, const rsm_root_ref* refs, uint32_t n, void* d_shares, void* d_present,
                           void* stream) {
    if (!ctx || k == 0 || k > 32768u) return fail(RSM_EINVAL, "rsm_vectors_gather_dev: bad arguments");
    if (int rc = validate_chunk_size(share_size)) return rc;
    if (share_size == 0) return fail(RSM_EINVAL, "rsm_vectors_gather_dev: empty shares");
    if (n > (1u << 24)) return fail(RSM_EINVAL, "rsm_vectors_gather_dev: at most %u refs per call", 1u << 24);
    if (n == 0 || count == 0) return RSM_OK;
    if (!d_eds || !d_presence || !refs || !d_shares || !d_present)
        return fail(RSM_EINVAL, "rsm_vectors_gather_dev: bad arguments");
    if ((reinterpret_cast<uintptr_t>(d_eds) | reinterpret_cast<uintptr_t>(d_shares)) & 15u)
        return fail(RSM_EINVAL, "rsm_vectors_gather_dev: d_eds and d_shares must be 16-byte aligned");
    const uint32_t W = 2 * k;
    for (uint32_t i = 0; i < n; ++i)
        if (refs[i].square >= count || refs[i].axis > 1 || refs[i].index >= W)
            return fail(RSM_EINVAL, "rsm_vectors_gather_dev: ref %u (square %u, axis %u, index %u) is out of range", i,
                        refs[i].square, refs[i].axis, refs[i].index);
    if (int rc = use_device(ctx)) return rc;
    hipStream_t st = pick(ctx, stream);
    StreamScratch& ss = stream_scratch(ctx, st);
    std::lock_guard<std::mutex> lk(ss.mu);
    const void* d = nullptr;
    if (int rc = stage_bytes(st, ss, refs, (size_t)n * sizeof(rsm_root_ref), &d)) return rc;
    const hipError_t e = launch_vectors_gather(static_cast<const uint8_t*>(d_eds), static_cast<const uint8_t*>(d_presence), W,
                                               share_size, static_cast<const RootRef*>(d), n,
                                               static_cast<uint8_t*>(d_shares), static_cast<uint8_t*>(d_present), st);
    return e == hipSuccess ? RSM_OK : hip_fail(e, "vector gather kernel launch");
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
