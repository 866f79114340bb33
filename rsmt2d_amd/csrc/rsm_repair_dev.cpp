// rsm_repair_dev.cpp -- Repair of device-resident squares: rsm_repair_squares_dev (the
// sweep loop of eds.cpp's fast_repair over a batch of squares that stay in device memory,
// planned by kernels_repair.hip, decoded by the existing decoders, verified as a batch) and
// rsm_repair_squares_checked_dev (every vector checked against its root and encoding when
// it becomes complete, so a bad one is named).  Both are a Session, a decode_pass per pass
// and close_squares, with their own stages around them.  With them rsm_vectors_gather_dev,
// and rsm_samples_scatter_dev (the apply step of rsm_eds_import_samples on the device).
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

// Sections of d_work.
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
    Carver c;
    l.todo[0] = c.take(count * W * 4);
    l.todo[1] = c.take(count * W * 4);
    l.state = c.take((uint64_t)count * 4);
    l.map = c.take((uint64_t)count * 4);
    l.flags = c.take((uint64_t)count * 8);
    l.roots = c.take(count * 2 * W * t->root_len);
    l.status = c.take(count * 2 * W * 4);
    l.leaf = c.take(count * W * W * (t->nmt ? 64 : 32));
    l.copies = c.take(count * W * W * S);
    l.total = c.at ? c.at : 256;
    *out = l;
    return true;
}

// Sections of the checked call's d_work.
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
    Carver c;
    l.todo[0] = c.take(count * W * 4);
    l.todo[1] = c.take(count * W * 4);
    l.state = c.take((uint64_t)count * 4);
    l.skip = c.take((uint64_t)count * 4);
    l.hashed = c.take((uint64_t)count * 4);
    l.cnt = c.take((uint64_t)count * 8);
    l.checked = c.take(count * 2 * W);
    l.recorded = c.take(count * ((W * W + 31) / 32) * 4);
    l.zero_end = c.at;
    l.list = c.take(count * 2 * W * 4);
    l.verdict = c.take(count * 2 * W * 4);
    l.parity = c.take(count * 2 * W * 4);
    l.leaf = c.take(count * W * W * (t->nmt ? 64 : 32));
    l.scratch = c.take(W * W * S);
    l.total = c.at;
    *out = l;
    return true;
}

// The argument checks both repair calls make before any device use; `extra_ok`: the
// call's further host operands are there.  RSM_OK at once for no square: the caller returns.
int repair_args(const char* fn, rsm_ctx* ctx, const void* d_eds, const void* d_presence, uint32_t k, uint32_t share_size,
                uint32_t count, const rsm_nmt_params* nmt, const void* d_roots, const void* d_work, const void* results,
                bool extra_ok, bool shape_ok, const DevTree& t) {
    if (!ctx || k == 0) return fail(RSM_EINVAL, "%s: bad arguments", fn);
    if (int rc = validate_chunk_size(share_size)) return rc;
    if (share_size == 0) return fail(RSM_EINVAL, "%s: empty shares", fn);
    if (!shape_ok)
        return fail(RSM_EUNSUPPORTED, "%s: %u squares of width %u%s not supported", fn, count, 2 * k, nmt ? " (NMT)" : "");
    if (count == 0) return RSM_OK;
    if (!d_eds || !d_presence || !d_roots || !d_work || !results || !extra_ok) return fail(RSM_EINVAL, "%s: bad arguments", fn);
    if ((reinterpret_cast<uintptr_t>(d_eds) | reinterpret_cast<uintptr_t>(d_presence) | reinterpret_cast<uintptr_t>(d_work)) & 15u)
        return fail(RSM_EINVAL, "%s: d_eds, d_presence and d_work must be 16-byte aligned", fn);
    if (t.nmt && share_size < t.p.namespace_size) return fail(RSM_ETREE, "data is too short to contain namespace ID");
    return RSM_OK;
}

// What a Repair call holds from its argument checks to its return (the device selected).
struct Session {
    rsm_ctx* const ctx;
    const hipStream_t st;
    const uint32_t k, W, S, count;
    const uint64_t sq, cells;  // bytes and cells of a square
    uint8_t *const eds, *const pres, *const work;
    uint32_t *const todo[2], *const state;  // the planner's sections of `work`
    // Members are destroyed last to first, so `drain` goes before `lane`: on an early
    // return the stream is drained before the lane, with its staging, goes back.
    LaneGuard lane;
    uint32_t* host = nullptr;    // the lane's pinned staging; the planner's report comes first
    uint32_t* mapped = nullptr;  // its device address
    Drain drain;

    Session(rsm_ctx* c, void* stream, void* d_eds, void* d_presence, void* d_work, uint32_t k_, uint32_t S_, uint32_t n,
            const uint64_t (&todo_at)[2], uint64_t state_at)
        : ctx(c), st(pick(c, stream)), k(k_), W(2 * k_), S(S_), count(n), sq((uint64_t)W * W * S), cells((uint64_t)W * W),
          eds(static_cast<uint8_t*>(d_eds)), pres(static_cast<uint8_t*>(d_presence)), work(static_cast<uint8_t*>(d_work)),
          todo{words(todo_at[0]), words(todo_at[1])}, state(words(state_at)), lane(c), drain{st, false} {}
    uint32_t* words(uint64_t at) const { return reinterpret_cast<uint32_t*>(work + at); }
    // Sizes and maps the staging, `per_square` words a square, and arms the drain.
    int open(uint32_t per_square) {
        if (!lane.lane) return lane.rc;
        hipError_t e;
        if ((e = lane.lane->host.ensure((size_t)count * per_square * 4)) != hipSuccess)
            return hip_fail(e, "hipHostMalloc (repair staging)");
        host = static_cast<uint32_t*>(lane.lane->host.ptr);
        void* dev = nullptr;
        if ((e = hipHostGetDevicePointer(&dev, host, 0)) != hipSuccess || !dev)
            return hip_fail(e == hipSuccess ? hipErrorInvalidValue : e, "hipHostGetDevicePointer (repair staging)");
        mapped = static_cast<uint32_t*>(dev);
        drain.armed = true;
        return RSM_OK;
    }
};

// One pass of the schedule of fast_repair's general loop (eds.cpp): row passes and column
// passes in turn, each decoding every vector with k <= have < 2k at once.  Every vector is
// decoded at most once, so at most 2W passes decode anything: pass 2W + 4 is an error.
// A square is finished once it misses nothing, or after two empty lists in a row (no pass
// can change it any more); *finished: this pass found every square so.  idle: a byte per
// square, zero before pass 0.  The checked call's, null otherwise: `skip` (device) and
// `dropped`: squares that take no further part; `last_missing`, `n_pass`: per square the
// plan's missing cells and the vectors decoded; `decoded`: something was.
int decode_pass(const char* fn, Session& s, uint32_t pass, uint8_t* idle, rsm_repair_result* results, bool* finished,
                const uint32_t* skip = nullptr, const uint8_t* dropped = nullptr, uint32_t* last_missing = nullptr,
                uint32_t* n_pass = nullptr, bool* decoded = nullptr) {
    const uint32_t axis = pass & 1u, W = s.W;
    if (pass == 2 * W + 4) return fail(RSM_EDEVICE, "%s: the sweeps did not end within %u passes", fn, 2 * W + 4);
    hipError_t e;
    if ((e = launch_repair_plan(s.pres, W, s.count, axis, pass == 0, s.todo[axis ^ 1u], s.todo[axis], s.state, s.mapped, s.st,
                                skip)) != hipSuccess)
        return hip_fail(e, "repair plan kernel launch");
    if ((e = hipStreamSynchronize(s.st)) != hipSuccess) return hip_fail(e, "repair stream");
    const uint32_t* const report = s.host;
    *finished = true;
    if (decoded) *decoded = false;
    for (uint32_t q = 0; q < s.count; ++q) {
        if (n_pass) n_pass[q] = 0;
        if (dropped && dropped[q]) continue;
        const uint32_t n = report[2 * q];
        if (last_missing) last_missing[q] = report[2 * q + 1];
        if (n == 0) {
            if (idle[q] < 2) ++idle[q];
            if (report[2 * q + 1] != 0 && idle[q] < 2) *finished = false;
            continue;
        }
        if (n > W) return fail(RSM_EDEVICE, "%s: planner reported %u vectors of %u", fn, n, W);
        if (int rc = launch_decode(s.ctx, decode_vectors(s.eds + q * s.sq, s.k, s.S, axis, s.todo[axis] + (size_t)q * W, n,
                                                         s.pres + q * s.cells), s.st))
            return rc;
        results[q].sweeps++;
        results[q].decoded_vectors += n;
        idle[q] = 0;
        if (n_pass) n_pass[q] = n;
        *finished = false;
        if (decoded) *decoded = true;
    }
    return RSM_OK;
}

// After the pass that found every square finished: the report's missing counts are final.
void close_squares(const Session& s, rsm_repair_result* results, const uint8_t* dropped = nullptr) {
    for (uint32_t q = 0; q < s.count; ++q) {
        if (dropped && dropped[q]) continue;
        results[q].missing = s.host[2 * q + 1];
        results[q].status = results[q].missing ? RSM_REPAIR_STUCK : RSM_REPAIR_OK;
    }
}

// What rsm_vectors_gather_dev and rsm_samples_scatter_dev check first, down to the
// alignment of d_eds and d_shares; `noun`: what the n items are; `operands`: the call's
// pointers are all there.  RSM_OK at once for no item or no square: the caller returns.
int cell_call_args(const char* fn, const char* noun, rsm_ctx* ctx, uint32_t k, uint32_t share_size, uint32_t count, uint32_t n,
                   const void* d_eds, const void* d_shares, bool operands) {
    if (!ctx || k == 0 || k > 32768u) return fail(RSM_EINVAL, "%s: bad arguments", fn);
    if (int rc = validate_chunk_size(share_size)) return rc;
    if (share_size == 0) return fail(RSM_EINVAL, "%s: empty shares", fn);
    if (n > (1u << 24)) return fail(RSM_EINVAL, "%s: at most %u %s per call", fn, 1u << 24, noun);
    if (n == 0 || count == 0) return RSM_OK;
    if (!operands) return fail(RSM_EINVAL, "%s: bad arguments", fn);
    if ((reinterpret_cast<uintptr_t>(d_eds) | reinterpret_cast<uintptr_t>(d_shares)) & 15u)
        return fail(RSM_EINVAL, "%s: d_eds and d_shares must be 16-byte aligned", fn);
    return RSM_OK;
}

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
    static const char* const fn = "rsm_repair_squares_dev";
    DevTree t;
    WorkLayout lay;
    const bool shape_ok = k != 0 && repair_shape(k, share_size, count, nmt, &t, &lay);
    if (int rc = repair_args(fn, ctx, d_eds, d_presence, k, share_size, count, nmt, d_roots, d_work, results, true, shape_ok, t))
        return rc;
    if (count == 0) return RSM_OK;
    if (int rc = use_device(ctx)) return rc;
    Session s(ctx, stream, d_eds, d_presence, d_work, k, share_size, count, lay.todo, lay.state);
    // staging: the planner's report [2] (written by the kernel through the mapping), then
    // the verification's map [1] (up) and flags [2] (back)
    if (int rc = s.open(5)) return rc;
    hipStream_t st = s.st;
    const uint32_t W = s.W, S = s.S, RL = t.root_len;
    uint8_t *const eds = s.eds, *const work = s.work;
    uint32_t *const map = s.words(lay.map), *const flags = s.words(lay.flags);
    uint32_t* const h_map = s.host + 2 * (size_t)count;
    uint32_t* const h_flags = h_map + count;

    for (uint32_t q = 0; q < count; ++q) results[q] = rsm_repair_result{};
    std::vector<uint8_t> idle(count, 0);
    bool finished = false;
    for (uint32_t pass = 0; !finished; ++pass)
        if (int rc = decode_pass(fn, s, pass, idle.data(), results, &finished)) return rc;
    close_squares(s, results);
    uint32_t n_done = 0;
    for (uint32_t q = 0; q < count; ++q)
        if (!results[q].missing) h_map[n_done++] = q;
    if (n_done == 0) {
        s.drain.armed = false;  // synchronised by the last pass, nothing enqueued since
        return RSM_OK;
    }
    // Completed squares, as one batch: Q0 copied out and re-extended, compared with the
    // square; the roots of the re-extended copies (the square's own wherever the compare
    // passes, and the compare is consulted first) against the committed ones.
    uint8_t* const copies = work + lay.copies;
    uint8_t* const got = work + lay.roots;
    uint32_t *const status = s.words(lay.status), *const leaf = s.words(lay.leaf);
    hipError_t e;
    if ((e = hipMemcpyAsync(map, h_map, (size_t)n_done * 4, hipMemcpyHostToDevice, st)) != hipSuccess ||
        (e = hipMemsetAsync(flags, 0, (size_t)n_done * 8, st)) != hipSuccess)
        return hip_fail(e, "repair verification (map, flags)");
    if ((e = launch_repair_gather_q0(eds, copies, map, k, S, n_done, st)) != hipSuccess)
        return hip_fail(e, "repair Q0 gather kernel launch");
    if (int rc = extend_squares(ctx, copies, k, S, n_done, st)) return rc;
    if ((e = launch_repair_compare_squares(eds, copies, map, s.sq, n_done, flags, st)) != hipSuccess)
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
    s.drain.armed = false;
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
    if (int rc = repair_args(fn, ctx, d_eds, d_presence, k, share_size, count, nmt, d_roots, d_work, results,
                             checks != nullptr, shape_ok, t))
        return rc;
    if (count == 0) return RSM_OK;
    if (int rc = use_device(ctx)) return rc;
    Session s(ctx, stream, d_eds, d_presence, d_work, k, share_size, count, lay.todo, lay.state);
    // staging, written by the kernels through the mapping: the planner's report [2], a check
    // stage's list lengths and the entry check's missing cells [3], its verdict key and the
    // cells it marked [2]; then the records computed [1] (a copy at the end)
    if (int rc = s.open(8)) return rc;
    hipStream_t st = s.st;
    const uint32_t W = s.W, S = s.S;
    uint8_t *const eds = s.eds, *const pres = s.pres;
    uint32_t *const skip = s.words(lay.skip), *const hashed = s.words(lay.hashed), *const cnt = s.words(lay.cnt);
    uint32_t *const recorded = s.words(lay.recorded), *const list = s.words(lay.list), *const verdict = s.words(lay.verdict);
    uint32_t *const parity = s.words(lay.parity), *const leaf = s.words(lay.leaf);
    uint8_t *const checked = s.work + lay.checked, *const scratch = s.work + lay.scratch;
    const uint8_t* const committed = static_cast<const uint8_t*>(d_roots);
    const uint32_t* const lens = s.host + 2 * (size_t)count;
    const uint32_t* const keys = lens + 3 * (size_t)count;
    uint32_t* const h_hashed = s.host + 7 * (size_t)count;
    uint32_t* const lens_dev = s.mapped + 2 * (size_t)count;
    uint32_t* const keys_dev = lens_dev + 3 * (size_t)count;

    for (uint32_t q = 0; q < count; ++q) {
        results[q] = rsm_repair_result{};
        checks[q] = rsm_repair_check{};
    }
    hipError_t e;
    if ((e = hipMemsetAsync(s.work + lay.skip, 0, lay.zero_end - lay.skip, st)) != hipSuccess)
        return hip_fail(e, "repair check state (memset)");

    std::vector<uint8_t> idle(count, 0), dropped(count, 0);
    std::vector<uint32_t> n_list(2 * (size_t)count, 0u), last_missing(count, 0u);
    // the check planner: lists this stage's vectors and reports their counts into `lens`
    auto check_plan = [&](uint32_t mode, uint32_t axis) -> int {
        const hipError_t r = launch_repair_check_plan(pres, W, count, mode, axis, s.todo[axis], s.state, skip, checked, list,
                                                      cnt, lens_dev, st);
        return r == hipSuccess ? RSM_OK : hip_fail(r, "repair check plan kernel launch");
    };
    // its counts, once the stream has been waited for, as the stage's (none in a square that dropped out)
    auto read_lens = [&] {
        for (uint32_t q = 0; q < count; ++q) {
            n_list[2 * q] = dropped[q] ? 0u : lens[3 * q];
            n_list[2 * q + 1] = dropped[q] ? 0u : lens[3 * q + 1];
        }
    };
    // One check stage over the vectors the check planner just listed (n_list: their counts
    // per square and axis, as the host knows them): leaf records of the cells that have none,
    // every tree of the batch in one launch with its root compare, per square and axis a
    // re-encode into the scratch square and the parity compare, then the verdict.
    // plan2: the launch of stage 2's check plan follows stage 1's verdict on the stream (the
    // verdict kernel has set the failing squares' skip words by then), so one wait serves both.
    auto run_checks = [&](bool stage2, uint32_t axis, bool plan2) -> int {
        uint32_t max_n = 0;
        for (uint32_t q = 0; q < count; ++q) max_n = std::max(max_n, n_list[2 * q] + n_list[2 * q + 1]);
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
        for (uint32_t q = 0; q < count; ++q)
            for (uint32_t a = 0; a < 2; ++a) {
                const uint32_t n = n_list[2 * q + a];
                if (n == 0) continue;
                if (n > W) return fail(RSM_EDEVICE, "%s: the check planner listed %u vectors of %u", fn, n, W);
                const uint32_t* const idx = list + ((size_t)q * 2 + a) * W;
                if (int rc = launch_encode(ctx, indexed_vectors(eds + q * s.sq, k, S, a, idx, n, scratch), st)) return rc;
                if ((r = launch_compare_parity(eds + q * s.sq, scratch, k, S, a, idx, n, parity + ((size_t)q * 2 + a) * W,
                                               st)) != hipSuccess)
                    return hip_fail(r, "repair check parity compare kernel launch");
            }
        if ((r = launch_repair_check_pick(list, cnt, verdict, parity, W, count, stage2, axis, s.todo[axis], s.state, pres, skip,
                                          keys_dev, st)) != hipSuccess)
            return hip_fail(r, "repair check verdict kernel launch");
        if (plan2)
            if (int rc = check_plan(2, axis)) return rc;
        if ((r = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(r, "repair stream");
        for (uint32_t q = 0; q < count; ++q) {
            const uint32_t n = n_list[2 * q] + n_list[2 * q + 1];
            if (n == 0) continue;
            checks[q].checked_vectors += n;
            const uint32_t key = keys[2 * q];
            if (key == ~0u) continue;
            dropped[q] = 1;
            results[q].status = RSM_REPAIR_BYZANTINE;
            results[q].missing = last_missing[q] - keys[2 * q + 1];
            checks[q].reason = key & 3u;
            checks[q].axis = (key >> 2) & 1u;
            checks[q].index = key >> 3;
            checks[q].round = results[q].sweeps;
        }
        return RSM_OK;
    };

    // round 0: the vectors complete on entry -- a check plan whose counts the host does not
    // know yet: run it, wait, read them
    if (int rc = check_plan(0, 0)) return rc;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "repair stream");
    read_lens();
    for (uint32_t q = 0; q < count; ++q) last_missing[q] = lens[3 * q + 2];
    if (int rc = run_checks(false, 0, false)) return rc;

    // The passes of the unchecked call (decode_pass), each followed by its two check stages.
    bool finished = false, decoded = false;
    std::vector<uint32_t> n_pass(count, 0u);
    for (uint32_t pass = 0; !finished; ++pass) {
        const uint32_t axis = pass & 1u;
        if (int rc = decode_pass(fn, s, pass, idle.data(), results, &finished, skip, dropped.data(), last_missing.data(),
                                 n_pass.data(), &decoded))
            return rc;
        if (!decoded) continue;
        // stage 1: the decoded vectors (their counts are the plan's)
        if (int rc = check_plan(1, axis)) return rc;
        for (uint32_t q = 0; q < count; ++q) {
            n_list[2 * q + axis] = n_pass[q];
            n_list[2 * q + (axis ^ 1u)] = 0;
        }
        if (int rc = run_checks(false, axis, true)) return rc;
        // stage 2: the vectors of the other axis that this pass completed, in the squares
        // whose stage 1 was clean (the others' skip words are set, and they listed nothing)
        read_lens();
        if (int rc = run_checks(true, axis, false)) return rc;
    }

    if ((e = hipMemcpyAsync(h_hashed, hashed, (size_t)count * 4, hipMemcpyDeviceToHost, st)) != hipSuccess)
        return hip_fail(e, "D2H repair check counters");
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "repair stream");
    s.drain.armed = false;
    for (uint32_t q = 0; q < count; ++q) checks[q].hashed_cells = h_hashed[q];
    close_squares(s, results, dropped.data());
    return RSM_OK;
}

int rsm_vectors_gather_dev(rsm_ctx* ctx, const void* d_eds, const void* d_presence, uint32_t k, uint32_t share_size,
                           uint32_t count, const rsm_root_ref* refs, uint32_t n, void* d_shares, void* d_present,
                           void* stream) {
    static const char* const fn = "rsm_vectors_gather_dev";
    if (int rc = cell_call_args(fn, "refs", ctx, k, share_size, count, n, d_eds, d_shares,
                                d_eds && d_presence && refs && d_shares && d_present))
        return rc;
    if (n == 0 || count == 0) return RSM_OK;
    const uint32_t W = 2 * k;
    if (int rc = check_refs(fn, "ref", refs, n, count, W)) return rc;
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
    static const char* const fn = "rsm_samples_scatter_dev";
    if (int rc = cell_call_args(fn, "samples", ctx, k, share_size, count, n, d_eds, d_shares,
                                d_eds && d_presence && samples && d_shares && d_status))
        return rc;
    if (n == 0 || count == 0) return RSM_OK;
    if (reinterpret_cast<uintptr_t>(d_status) & 3u) return fail(RSM_EINVAL, "%s: d_status must be 4-byte aligned", fn);
    const uint32_t W = 2 * k;
    if (int rc = check_samples(fn, samples, n, count, W)) return rc;
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
