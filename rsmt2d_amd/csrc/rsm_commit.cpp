// rsm_commit.cpp -- blob share commitments: the C ABI over kernels_commit.hip.
// rsm_blob_commitments_dev (shares path: leaf records, one subtree launch per size
// present, the fold), rsm_commitments_dev (store path: the fold over nodes gathered from
// an NMT node store) and rsm_eds_commitments / rsm_eds_subtree_roots of the
// ExtendedDataSquare object (the cached node store of rsm_eds_proofs, or the host
// restatement rsm_square_commitment of merkle.cpp).  Formats: include/rsmt2d_hip.h
// "share commitments".
#include "eds_internal.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace rsm;

static_assert(kCommitOrder == RSM_COMMIT_ORDER && kCommitTree == RSM_COMMIT_TREE, "the kernels' status words are the C ABI's");

namespace {

constexpr uint32_t kMaxBlobs = 1u << 20, kMaxShares = 1u << 24, kMaxSubtree = 1024;
constexpr uint32_t kSizeClasses = 11;  // subtree sizes 1 .. 1024

bool ns_ok(const rsm_nmt_params* nmt) { return nmt->namespace_size >= 1 && nmt->namespace_size <= 32; }

// M of a blob of `len` shares at subtree width w
uint32_t mountain_count(uint32_t len, uint32_t w) {
    uint32_t m = 0;
    (void)rsm_subtree_sizes(len, w, nullptr, 0, &m);
    return m;
}

// The sections of d_work: leaf records, packed roots, flag words.
struct WorkPlan {
    uint64_t leaf, roots, flags, total;
};
WorkPlan work_plan(uint64_t shares, uint64_t roots, uint32_t ns) {
    Carver c;
    WorkPlan w{};
    w.leaf = c.take(shares * kProofNmtLeafWords * 4);
    w.roots = c.take(roots * (2ull * ns + 32));
    w.flags = c.take(roots * 4);
    w.total = c.at;
    return w;
}

// RSM_EINVAL naming the first blob the store path refuses; RSM_EUNSUPPORTED for one of more
// than kCommitMaxRoots roots.  plan[i]: the staged blob.
int plan_blobs(const char* fn, const rsm_blob_ref* blobs, uint32_t n, uint32_t count, uint32_t k, uint32_t threshold,
               std::vector<CommitBlob>* plan, uint32_t* max_m, uint64_t* total_roots) {
    plan->resize(n);
    uint64_t off = 0;
    uint32_t mm = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const rsm_blob_ref& b = blobs[i];
        const uint32_t w = b.len ? rsm_subtree_width(b.len, threshold) : 1;
        if (b.square >= count || b.len == 0 || (uint64_t)b.start + b.len > (uint64_t)k * k || b.start % w)
            return fail(RSM_EINVAL, "%s: blob %u (square %u, shares [%u, %u + %u)) is out of range or not aligned to its subtree width %u",
                        fn, i, b.square, b.start, b.start, b.len, w);
        const uint32_t m = mountain_count(b.len, w);
        if (m > kCommitMaxRoots)
            return fail(RSM_EUNSUPPORTED, "%s: blob %u has %u subtree roots (at most %u)", fn, i, m, kCommitMaxRoots);
        if (off + m > 0xFFFFFFFFull) return fail(RSM_EUNSUPPORTED, "%s: more than 2^32 - 1 subtree roots", fn);
        (*plan)[i] = CommitBlob{b.square, b.start, b.len, w, (uint32_t)off, m};
        off += m;
        mm = std::max(mm, m);
    }
    *max_m = mm;
    *total_roots = off;
    return RSM_OK;
}

int eds_commit(const char* fn, rsm_eds* e, rsm_tree_root_fn tree_fn, void* user, const rsm_blob_ref* blobs, uint32_t n,
               uint32_t threshold, uint8_t* out, uint32_t* status_out, uint8_t* roots_out, uint32_t* root_offsets_out) {
    if (!e || threshold == 0 || (n && (!blobs || !out || !status_out))) return fail(RSM_EINVAL, "%s: bad arguments", fn);
    const rsm_nmt_params* nmt = eds_nmt_of(tree_fn, user);
    if (!nmt) return fail(RSM_EUNSUPPORTED, "%s: share commitments are built for the NMT only", fn);
    const uint32_t W = e->width, k = e->odw, S = e->S;
    if (!ns_ok(nmt) || nmt->square_size != k || k == 0)
        return fail(RSM_EINVAL, "%s: namespace size %u (1..32) or square size %u (the ODS width %u)", fn, nmt->namespace_size,
                    nmt->square_size, k);
    if (k & (k - 1)) return fail(RSM_EUNSUPPORTED, "%s: ODS width %u is not a power of two", fn, k);
    if (n > kMaxBlobs) return fail(RSM_EUNSUPPORTED, "%s: at most %u blobs per call", fn, kMaxBlobs);
    if (S < nmt->namespace_size) return fail(RSM_ETREE, "data is too short to contain namespace ID");
    std::vector<CommitBlob> plan;
    uint32_t max_m = 0;
    uint64_t total_roots = 0;
    if (int rc = plan_blobs(fn, blobs, n, 1, k, threshold, &plan, &max_m, &total_roots)) return rc;
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t row = blobs[i].start / k; row <= (blobs[i].start + blobs[i].len - 1) / k; ++row)
            for (uint32_t c = 0; c < k; ++c)
                if (!e->has(row, c)) return fail(RSM_ETREE, "can not commit to a blob in incomplete row %u", row);
    if (root_offsets_out) {
        for (uint32_t i = 0; i < n; ++i) root_offsets_out[i] = plan[i].root_off;
        root_offsets_out[n] = (uint32_t)total_roots;
    }
    if (n == 0) return RSM_OK;
    const uint32_t NB = 2 * nmt->namespace_size + 32;
    DevTree dt;
    if (eds_store_path(e, nmt, &dt)) {
        rsm_ctx* ctx = e->ctx;
        std::lock_guard<std::mutex> lk(ctx->eds_mu);
        if (int rc = use_device(ctx)) return rc;
        hipStream_t st = ctx->stream;
        hipError_t r;
        if (int rc = eds_ensure_store(e, nmt, dt)) return rc;
        ProofStore& ps = e->proofs;
        // commitments | status words | roots in one scratch buffer
        Carver c;
        const uint64_t o_com = c.take((uint64_t)n * 32), o_st = c.take((uint64_t)n * 4),
                       o_roots = c.take(roots_out ? total_roots * NB : 0);
        DevBuf& rb = ctx->eds.scratch;
        DevBuf& sb = ctx->eds.status;
        if ((r = rb.ensure(c.at)) != hipSuccess || (r = sb.ensure((size_t)2 * W * 4)) != hipSuccess)
            return hip_fail(r, "hipMalloc (commitments)");
        if ((r = hipMemcpyAsync(sb.ptr, ps.status.data(), (size_t)2 * W * 4, hipMemcpyHostToDevice, st)) != hipSuccess)
            return hip_fail(r, "H2D tree status");
        auto* d = static_cast<uint8_t*>(rb.ptr);
        if (int rc = rsm_commitments_dev(ctx, ps.d_nodes, sb.ptr, W, 1, nmt, threshold, blobs, n, roots_out ? d + o_roots : nullptr,
                                         nullptr, d + o_com, d + o_st, st))
            return rc;
        if ((r = hipMemcpyAsync(out, d + o_com, (size_t)n * 32, hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (r = hipMemcpyAsync(status_out, d + o_st, (size_t)n * 4, hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (roots_out &&
             (r = hipMemcpyAsync(roots_out, d + o_roots, total_roots * NB, hipMemcpyDeviceToHost, st)) != hipSuccess))
            return hip_fail(r, "D2H commitments");
        if ((r = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(r, "proof stream");
    } else {
        for (uint32_t i = 0; i < n; ++i) {
            const int rc = rsm_square_commitment(nmt, nullptr, e->data.data(), k, S, blobs[i].start, blobs[i].len, threshold,
                                                 out + (size_t)i * 32, roots_out ? roots_out + (size_t)plan[i].root_off * NB : nullptr,
                                                 &status_out[i]);
            if (rc) return fail(rc, "%s: blob %u: bad tree parameters", fn, i);
        }
    }
    // a failing blob has no subtree roots to hand out, on either path
    if (roots_out)
        for (uint32_t i = 0; i < n; ++i)
            if (status_out[i]) memset(roots_out + (size_t)plan[i].root_off * NB, 0, (size_t)plan[i].m * NB);
    return RSM_OK;
}

}  // namespace

extern "C" {

uint64_t rsm_commit_work_bytes(uint64_t total_shares, uint64_t total_subtree_roots, const rsm_nmt_params* nmt) {
    if (!nmt || !ns_ok(nmt) || total_shares > kMaxShares || total_subtree_roots > total_shares) return 0;
    return work_plan(total_shares, total_subtree_roots, nmt->namespace_size).total;
}

int rsm_blob_commitments_dev(rsm_ctx* ctx, const void* d_shares, uint32_t share_size, const rsm_nmt_params* nmt,
                             uint32_t threshold, const uint32_t* offsets, uint32_t n, void* d_work, void* d_commitments,
                             void* d_status, void* stream) {
    const char* fn = "rsm_blob_commitments_dev";
    if (!ctx || threshold == 0 || (n && (!offsets || !d_shares || !d_work || !d_commitments || !d_status)))
        return fail(RSM_EINVAL, "%s: bad arguments", fn);
    if (!nmt) return fail(RSM_EUNSUPPORTED, "%s: share commitments are built for the NMT only", fn);
    if (!ns_ok(nmt)) return fail(RSM_EINVAL, "%s: namespace size %u (1..32)", fn, nmt->namespace_size);
    if ((reinterpret_cast<uintptr_t>(d_shares) & 15u) || (reinterpret_cast<uintptr_t>(d_work) & 15u))
        return fail(RSM_EINVAL, "%s: d_shares and d_work must be 16-byte aligned", fn);
    if (reinterpret_cast<uintptr_t>(d_status) & 3u) return fail(RSM_EINVAL, "%s: d_status must be 4-byte aligned", fn);
    if (int rc = validate_chunk_size(share_size)) return rc;
    const uint32_t ns = nmt->namespace_size;
    if (share_size < ns) return fail(RSM_ETREE, "data is too short to contain namespace ID");
    if (n > kMaxBlobs) return fail(RSM_EUNSUPPORTED, "%s: at most %u blobs per call", fn, kMaxBlobs);
    if (n == 0) return RSM_OK;
    for (uint32_t i = 0; i < n; ++i)
        if (offsets[i + 1] <= offsets[i])
            return fail(RSM_EINVAL, "%s: blob %u (shares [%u, %u)) is empty or its offsets decrease", fn, i, offsets[i],
                        offsets[i + 1]);
    const uint32_t base = offsets[0], total = offsets[n] - base;
    if (total > kMaxShares) return fail(RSM_EUNSUPPORTED, "%s: %u shares (at most %u per call)", fn, total, kMaxShares);
    // the plan: root offsets, then the tasks grouped by subtree size
    std::vector<uint32_t> head((size_t)n + 2, 0);  // n + 1 root offsets, padded to 8 bytes
    std::vector<CommitTask> tasks[kSizeClasses];
    uint32_t max_m = 0, slot = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t len = offsets[i + 1] - offsets[i], w = rsm_subtree_width(len, threshold);
        if (w > kMaxSubtree || !commit_subtree_supported(w, ns))
            return fail(RSM_EUNSUPPORTED, "%s: blob %u has subtree width %u (at most %u, LDS permitting)", fn, i, w, kMaxSubtree);
        const uint32_t m = mountain_count(len, w);
        if (m > kCommitMaxRoots)
            return fail(RSM_EUNSUPPORTED, "%s: blob %u has %u subtree roots (at most %u)", fn, i, m, kCommitMaxRoots);
        head[i] = slot;
        for (uint32_t at = 0; at < len;) {
            uint32_t z = w;
            while (z > len - at) z >>= 1;
            tasks[__builtin_ctz(z)].push_back(CommitTask{offsets[i] - base + at, slot++});
            at += z;
        }
        max_m = std::max(max_m, m);
    }
    head[n] = slot;
    const uint32_t head_words = (n + 2) & ~1u;
    std::vector<uint8_t> staged((size_t)head_words * 4 + (size_t)slot * sizeof(CommitTask));
    memcpy(staged.data(), head.data(), (size_t)head_words * 4);
    size_t task_at[kSizeClasses], at = (size_t)head_words * 4;
    for (uint32_t c = 0; c < kSizeClasses; ++c) {
        task_at[c] = at;
        if (!tasks[c].empty()) memcpy(&staged[at], tasks[c].data(), tasks[c].size() * sizeof(CommitTask));
        at += tasks[c].size() * sizeof(CommitTask);
    }
    if (int rc = use_device(ctx)) return rc;
    hipStream_t st = pick(ctx, stream);
    StreamScratch& ss = stream_scratch(ctx, st);
    std::lock_guard<std::mutex> lk(ss.mu);
    const void* dp = nullptr;
    if (int rc = stage_bytes(st, ss, staged.data(), staged.size(), &dp)) return rc;
    const auto* plan = static_cast<const uint8_t*>(dp);
    const WorkPlan wp = work_plan(total, slot, ns);
    auto* work = static_cast<uint8_t*>(d_work);
    auto* leaf = reinterpret_cast<uint32_t*>(work + wp.leaf);
    uint8_t* roots = work + wp.roots;
    auto* flags = reinterpret_cast<uint32_t*>(work + wp.flags);
    hipError_t e = launch_commit_leaves(static_cast<const uint8_t*>(d_shares) + (uint64_t)base * share_size, total, share_size,
                                        ns, leaf, st);
    if (e != hipSuccess) return hip_fail(e, "commitment leaf kernel launch");
    for (uint32_t c = 0; c < kSizeClasses; ++c) {
        if (tasks[c].empty()) continue;
        e = launch_commit_subtrees(leaf, reinterpret_cast<const CommitTask*>(plan + task_at[c]), (uint32_t)tasks[c].size(),
                                   1u << c, ns, nmt->ignore_max_namespace, roots, flags, st);
        if (e != hipSuccess) return hip_fail(e, "commitment subtree kernel launch");
    }
    e = launch_commit_fold(roots, flags, reinterpret_cast<const uint32_t*>(plan), n, max_m, ns,
                           static_cast<uint8_t*>(d_commitments), static_cast<uint32_t*>(d_status), st);
    return e == hipSuccess ? RSM_OK : hip_fail(e, "commitment fold kernel launch");
}

int rsm_commitments_dev(rsm_ctx* ctx, const void* d_nodes, const void* d_status_trees, uint32_t width, uint32_t count,
                        const rsm_nmt_params* nmt, uint32_t threshold, const rsm_blob_ref* blobs, uint32_t n,
                        void* d_roots_out, void* d_root_offsets, void* d_commitments, void* d_status, void* stream) {
    const char* fn = "rsm_commitments_dev";
    if (!ctx || width == 0 || threshold == 0 ||
        (n && count && (!d_nodes || !d_status_trees || !blobs || !d_commitments || !d_status)))
        return fail(RSM_EINVAL, "%s: bad arguments", fn);
    if (!nmt) return fail(RSM_EUNSUPPORTED, "%s: share commitments are built for the NMT only", fn);
    if (!ns_ok(nmt) || nmt->square_size == 0)
        return fail(RSM_EINVAL, "%s: namespace size %u (1..32) or square size 0", fn, nmt->namespace_size);
    if ((reinterpret_cast<uintptr_t>(d_nodes) & 15u) || (reinterpret_cast<uintptr_t>(d_status_trees) & 3u) ||
        (reinterpret_cast<uintptr_t>(d_status) & 3u) || (reinterpret_cast<uintptr_t>(d_root_offsets) & 3u))
        return fail(RSM_EINVAL, "%s: d_nodes must be 16-byte, d_status_trees, d_status and d_root_offsets 4-byte aligned", fn);
    const uint32_t k = width / 2;
    if ((width & 1u) || (k & (k - 1)) || rsm_proof_nodes_bytes(width, nmt, count ? count : 1) == 0)
        return fail(RSM_EUNSUPPORTED, "%s: %u squares of width %u (NMT, ODS width a power of two) not supported", fn, count, width);
    if (n > kMaxBlobs) return fail(RSM_EUNSUPPORTED, "%s: at most %u blobs per call", fn, kMaxBlobs);
    if (n == 0 || count == 0) return RSM_OK;
    std::vector<CommitBlob> plan;
    uint32_t max_m = 0;
    uint64_t total_roots = 0;
    if (int rc = plan_blobs(fn, blobs, n, count, k, threshold, &plan, &max_m, &total_roots)) return rc;
    if (int rc = use_device(ctx)) return rc;
    hipStream_t st = pick(ctx, stream);
    StreamScratch& ss = stream_scratch(ctx, st);
    std::lock_guard<std::mutex> lk(ss.mu);
    const void* dp = nullptr;
    if (int rc = stage_bytes(st, ss, plan.data(), (size_t)n * sizeof(CommitBlob), &dp)) return rc;
    const hipError_t e = launch_commit_fold_store(
        static_cast<const uint32_t*>(d_nodes), static_cast<const uint32_t*>(d_status_trees), width, count, nmt->namespace_size,
        static_cast<const CommitBlob*>(dp), n, max_m, static_cast<uint8_t*>(d_roots_out), static_cast<uint32_t*>(d_root_offsets),
        static_cast<uint8_t*>(d_commitments), static_cast<uint32_t*>(d_status), st);
    return e == hipSuccess ? RSM_OK : hip_fail(e, "commitment fold kernel launch");
}

int rsm_eds_commitments(rsm_eds* eds, rsm_tree_root_fn tree_fn, void* user, const rsm_blob_ref* blobs, uint32_t n,
                        uint32_t threshold, uint8_t* out, uint32_t* status_out) {
    return eds_commit("rsm_eds_commitments", eds, tree_fn, user, blobs, n, threshold, out, status_out, nullptr, nullptr);
}

int rsm_eds_subtree_roots(rsm_eds* eds, rsm_tree_root_fn tree_fn, void* user, const rsm_blob_ref* blobs, uint32_t n,
                          uint32_t threshold, uint8_t* out, uint32_t* status_out, uint8_t* roots_out,
                          uint32_t* root_offsets_out) {
    if (!roots_out || !root_offsets_out) return fail(RSM_EINVAL, "rsm_eds_subtree_roots: bad arguments");
    return eds_commit("rsm_eds_subtree_roots", eds, tree_fn, user, blobs, n, threshold, out, status_out, roots_out,
                      root_offsets_out);
}

}  // extern "C"
