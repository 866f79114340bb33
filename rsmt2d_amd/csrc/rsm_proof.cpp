// rsm_proof.cpp -- share inclusion proofs: the C ABI over the node-store builds
// (kernels_sha.hip, kernels_nmt.hip) and the gather kernels (kernels_proof.hip), and
// rsm_eds_proofs of the ExtendedDataSquare object (device path with a cached node
// store; host restatements of merkle.cpp otherwise); the receiving side:
// rsm_proofs_verify_dev over the verify kernels (kernels_sha.hip, kernels_nmt.hip) and
// rsm_eds_import_samples (verify, then SetCell); namespace proofs: rsm_ns_proofs_dev over
// kernels_nsproof.hip, rsm_eds_namespace_proofs, and their receiving side
// rsm_ns_proofs_verify_dev over nmt_ns_verify_kernel (kernels_nmt.hip); the data root:
// rsm_data_roots_dev and rsm_root_proofs_dev over kernels_dataroot.hip, and
// rsm_proofs_verify_data_root_dev over the chained verify kernels, and rsm_eds_data_root
// (the roots on the device as rsm_eds_roots computes them, then the data root there); range
// proofs: rsm_range_proofs_dev over kernels_nsproof.hip, rsm_range_proofs_verify_dev and its
// chained form over the range verify kernels, rsm_eds_range_proofs, rsm_share_range_queries.
// Formats: include/rsmt2d_hip.h.
#include "eds_internal.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace rsm;

static_assert(sizeof(rsm_sample) == sizeof(ProofSample) && sizeof(rsm_sample) == 16, "rsm_sample is the kernels' sample");

static_assert(sizeof(rsm_root_ref) == sizeof(RootRef) && sizeof(rsm_root_ref) == 12, "rsm_root_ref is the kernels' ref");

static_assert(sizeof(NsQuery) == 44&& kNsEmpty == RSM_NS_EMPTY && kNsInclusion == RSM_NS_INCLUSION &&
                  kNsAbsence == RSM_NS_ABSENCE && kNsTree == RSM_NS_TREE,
              "the kernels' namespace proof kinds are the C ABI's");

static_assert(sizeof(rsm_range_query) == sizeof(RangeQuery) && sizeof(rsm_range_query) == 20,
              "rsm_range_query is the kernels' range query");

static_assert(kProofOk == RSM_PROOF_OK && kProofMalformed == RSM_PROOF_MALFORMED && kProofOrder == RSM_PROOF_ORDER &&
                  kProofRoot == RSM_PROOF_ROOT && kProofNamespace == RSM_PROOF_NAMESPACE &&
                  kProofIncomplete == RSM_PROOF_INCOMPLETE,
              "the kernels' status words are the C ABI's");

namespace rsm {

// Uploads `bytes` of a call's host arguments through the stream's staging buffers
// (ss.mu held): *dev is the device copy, valid for kernels enqueued on `st` before the
// next call on it.
int stage_bytes(hipStream_t st, StreamScratch& ss, const void* src, size_t bytes, const void** dev) {
    hipError_t e;
    // the staging buffer is free once the previous call's upload has left it; the
    // device copy is read by that call's kernels, ordered before this upload on `st`
    if (ss.samp_ev && (e = hipEventSynchronize(ss.samp_ev)) != hipSuccess) return hip_fail(e, "hipEventSynchronize");
    if (!ss.samp_ev && (e = hipEventCreateWithFlags(&ss.samp_ev, hipEventDisableTiming)) != hipSuccess) {
        ss.samp_ev = nullptr;
        return hip_fail(e, "hipEventCreate");
    }
    if (bytes > ss.samp_dev.cap) {
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
        if ((e = ss.samp_dev.ensure(bytes)) != hipSuccess) return hip_fail(e, "hipMalloc (samples)");
    }
    if ((e = ss.samp_host.ensure(bytes)) != hipSuccess) return hip_fail(e, "hipHostMalloc (samples)");
    memcpy(ss.samp_host.ptr, src, bytes);
    if ((e = hipMemcpyAsync(ss.samp_dev.ptr, ss.samp_host.ptr, bytes, hipMemcpyHostToDevice, st)) != hipSuccess)
        return hip_fail(e, "H2D samples");
    if ((e = hipEventRecord(ss.samp_ev, st)) != hipSuccess) return hip_fail(e, "hipEventRecord");
    *dev = ss.samp_dev.ptr;
    return RSM_OK;
}

int check_samples(const char* fn, const rsm_sample* s, uint32_t n, uint32_t count, uint32_t width) {
    for (uint32_t i = 0; i < n; ++i)
        if (s[i].square >= count || s[i].axis > 1 || s[i].index >= width || s[i].pos >= width)
            return fail(RSM_EINVAL, "%s: sample %u (square %u, axis %u, index %u, pos %u) is out of range", fn, i, s[i].square,
                        s[i].axis, s[i].index, s[i].pos);
    return RSM_OK;
}

}  // namespace rsm

namespace {

// The device tree of (width, nmt), or false beyond the root kernels' limits.
bool proof_tree_for(uint32_t width, const rsm_nmt_params* nmt, DevTree* t) {
    return device_tree_for(nmt ? rsm_nmt_tree_root : nullptr, const_cast<rsm_nmt_params*>(nmt), width, t);
}

uint64_t store_bytes(const DevTree& t, uint32_t W, uint32_t count) {
    return 4 * (t.nmt ? proof_store_words(W, count, kProofNmtLeafWords, kProofNmtNodeWords)
                      : proof_store_words(W, count, kProofShaWords, kProofShaWords));
}

// The staged queries of the two namespace calls: the range check, then each namespace as
// big-endian words, zero padded, as the leaf records hold them.
int pack_ns_queries(const char* fn, const rsm_ns_query* queries, const uint8_t* nids, uint32_t n, uint32_t ns, uint32_t count,
                    uint32_t width, std::vector<NsQuery>* out) {
    if (int rc = check_refs(fn, "query", queries, n, count, width)) return rc;
    out->assign(n, NsQuery{});
    for (uint32_t i = 0; i < n; ++i) {
        NsQuery& q = (*out)[i] = NsQuery{queries[i].square, queries[i].axis, queries[i].index, {}};
        for (uint32_t b = 0; b < ns; ++b) q.nid[b >> 2] |= (uint32_t)nids[(size_t)i * ns + b] << (24u - 8u * (b & 3u));
    }
    return RSM_OK;
}

int check_range_queries(const char* fn, const rsm_range_query* q, uint32_t n, uint32_t count, uint32_t width) {
    for (uint32_t i = 0; i < n; ++i)
        if (q[i].square >= count || q[i].axis > 1 || q[i].index >= width || !(q[i].start < q[i].end && q[i].end <= width))
            return fail(RSM_EINVAL, "%s: query %u (square %u, axis %u, index %u, leaves [%u, %u)) is out of range", fn, i,
                        q[i].square, q[i].axis, q[i].index, q[i].start, q[i].end);
    return RSM_OK;
}

// The two range verification calls: their checks before any device use, in
// rsm_ns_proofs_verify_dev's order (`operands`: the call's pointers are all there), then
// the queries staged and the launch; d_roots or (chained) d_root_records / d_data_roots.
int range_verify_call(const char* fn, rsm_ctx* ctx, bool operands, const void* d_records, const void* d_offsets,
                      const void* d_shares, uint64_t shares_total, const void* d_roots, const void* d_root_records,
                      const void* d_data_roots, uint32_t width, uint32_t share_size, uint32_t count,
                      const rsm_nmt_params* nmt, const rsm_range_query* queries, uint32_t n, void* d_status, void* stream) {
    if (!ctx || width == 0 || (n && count && (!operands || (shares_total && !d_shares))))
        return fail(RSM_EINVAL, "%s: bad arguments", fn);
    if (nmt && (nmt->namespace_size == 0 || nmt->namespace_size > 32 || nmt->square_size == 0))
        return fail(RSM_EINVAL, "%s: namespace size %u (1..32) or square size 0", fn, nmt->namespace_size);
    if (reinterpret_cast<uintptr_t>(d_shares) & 15u) return fail(RSM_EINVAL, "%s: d_shares must be 16-byte aligned", fn);
    if ((reinterpret_cast<uintptr_t>(d_offsets) & 3u) || (reinterpret_cast<uintptr_t>(d_status) & 3u))
        return fail(RSM_EINVAL, "%s: d_offsets and d_status must be 4-byte aligned", fn);
    if (int rc = validate_chunk_size(share_size)) return rc;
    if (!range_verify_supported(width, nmt ? nmt->namespace_size : 0u))
        return fail(RSM_EUNSUPPORTED, "%s: width %u not supported (at most %u)", fn, width, nmt ? 1024u : 2048u);
    if (nmt && share_size < nmt->namespace_size) return fail(RSM_ETREE, "data is too short to contain namespace ID");
    if (n > (1u << 20)) return fail(RSM_EINVAL, "%s: at most %u queries per call", fn, 1u << 20);
    if (n == 0 || count == 0) return RSM_OK;
    if (int rc = check_range_queries(fn, queries, n, count, width)) return rc;
    if (int rc = use_device(ctx)) return rc;
    hipStream_t st = pick(ctx, stream);
    StreamScratch& ss = stream_scratch(ctx, st);
    std::lock_guard<std::mutex> lk(ss.mu);
    const void* dq = nullptr;
    if (int rc = stage_bytes(st, ss, queries, (size_t)n * sizeof(rsm_range_query), &dq)) return rc;
    const auto* rec = static_cast<const uint8_t*>(d_records);
    const auto* offs = static_cast<const uint32_t*>(d_offsets);
    const auto* sh = static_cast<const uint8_t*>(d_shares);
    const auto* roots = static_cast<const uint8_t*>(d_roots);
    const auto* rrec = static_cast<const uint8_t*>(d_root_records);
    const auto* dr = static_cast<const uint8_t*>(d_data_roots);
    const auto* q = static_cast<const RangeQuery*>(dq);
    const hipError_t e =
        nmt ? launch_nmt_range_verify(rec, offs, sh, shares_total, roots, rrec, dr, width, share_size, nmt->namespace_size,
                                      nmt->square_size, nmt->ignore_max_namespace, q, n, static_cast<uint32_t*>(d_status), st)
            : launch_range_verify(rec, offs, sh, shares_total, roots, rrec, dr, width, share_size, q, n,
                                  static_cast<uint32_t*>(d_status), st);
    return e == hipSuccess ? RSM_OK : hip_fail(e, "range proof verify kernel launch");
}

int stage_samples(hipStream_t st, StreamScratch& ss, const rsm_sample* samples, uint32_t n, const ProofSample** ds) {
    const void* d = nullptr;
    if (int rc = stage_bytes(st, ss, samples, (size_t)n * sizeof(rsm_sample), &d)) return rc;
    *ds = static_cast<const ProofSample*>(d);
    return RSM_OK;
}

// The two sample-verification calls: their checks before any device use, in their order
// (`operands`: the call's pointers are all there), then the samples staged and
// launch(staged samples, status words, stream); `what` names that launch in an error.
template <class Launch>
int verify_call(const char* fn, rsm_ctx* ctx, bool operands, const void* d_shares, void* d_status, uint32_t width,
                uint32_t share_size, uint32_t count, const rsm_nmt_params* nmt, const rsm_sample* samples, uint32_t n,
                void* stream, const char* what, Launch launch) {
    if (!ctx || width == 0 || width > 65536u || (n && count && !operands)) return fail(RSM_EINVAL, "%s: bad arguments", fn);
    if (nmt && (nmt->namespace_size == 0 || nmt->namespace_size > 32 || nmt->square_size == 0))
        return fail(RSM_EINVAL, "%s: namespace size %u (1..32) or square size 0", fn, nmt->namespace_size);
    if (reinterpret_cast<uintptr_t>(d_shares) & 15u) return fail(RSM_EINVAL, "%s: d_shares must be 16-byte aligned", fn);
    if (reinterpret_cast<uintptr_t>(d_status) & 3u) return fail(RSM_EINVAL, "%s: d_status must be 4-byte aligned", fn);
    if (int rc = validate_chunk_size(share_size)) return rc;
    if (nmt && share_size < nmt->namespace_size) return fail(RSM_ETREE, "data is too short to contain namespace ID");
    if (n > (1u << 24)) return fail(RSM_EINVAL, "%s: at most %u samples per call", fn, 1u << 24);
    if (n == 0 || count == 0) return RSM_OK;
    if (int rc = check_samples(fn, samples, n, count, width)) return rc;
    if (int rc = use_device(ctx)) return rc;
    hipStream_t st = pick(ctx, stream);
    StreamScratch& ss = stream_scratch(ctx, st);
    std::lock_guard<std::mutex> lk(ss.mu);
    const ProofSample* ds = nullptr;
    if (int rc = stage_samples(st, ss, samples, n, &ds)) return rc;
    const hipError_t e = launch(ds, static_cast<uint32_t*>(d_status), st);
    return e == hipSuccess ? RSM_OK : hip_fail(e, what);
}

uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// The NMT params of (tree_fn, user), or nullptr.
const rsm_nmt_params* nmt_of(rsm_tree_root_fn tree_fn, void* user) {
    return tree_fn == rsm_nmt_tree_root && user ? static_cast<const rsm_nmt_params*>(user) : nullptr;
}

// Whether a complete square with a context takes the device path for tree `nmt`.
bool store_path(rsm_eds* e, const rsm_nmt_params* nmt, DevTree* dt) {
    const bool complete = memchr(e->present.data(), 0, e->present.size()) == nullptr;
    return e->ctx && complete && proof_tree_for(e->width, nmt, dt) && rsm_proof_nodes_bytes(e->width, nmt, 1) != 0 &&
           (!dt->nmt || e->S >= dt->p.namespace_size);
}

// The square's cached node store for tree `dt`, built once (ctx->eds_mu held, device
// selected); later calls only gather.
int ensure_store(rsm_eds* e, const rsm_nmt_params* nmt, const DevTree& dt) {
    rsm_ctx* ctx = e->ctx;
    hipStream_t st = ctx->stream;
    const uint32_t W = e->width, S = e->S;
    hipError_t r;
    ProofStore& ps = e->proofs;
    const bool same =
        ps.d_nodes && ps.ctx == ctx && ps.nmt == dt.nmt && (!dt.nmt || memcmp(&ps.p, &dt.p, sizeof(dt.p)) == 0);
    if (same) return RSM_OK;
    ps.drop();
    DevBuf& sq = ctx->eds.eds;
    DevBuf& sb = ctx->eds.status;
    if ((r = sq.ensure(e->data.size())) != hipSuccess || (r = sb.ensure((size_t)2 * W * 4)) != hipSuccess)
        return hip_fail(r, "hipMalloc (proof square)");
    if ((r = hipMalloc(&ps.d_nodes, store_bytes(dt, W, 1))) != hipSuccess) {
        ps.d_nodes = nullptr;
        return hip_fail(r, "hipMalloc (node store)");
    }
    ps.ctx = ctx;
    ps.nmt = dt.nmt;
    ps.p = dt.p;
    ps.status.assign((size_t)2 * W, 0);
    int rc = RSM_OK;
    if ((r = hipMemcpyAsync(sq.ptr, e->data.data(), e->data.size(), hipMemcpyHostToDevice, st)) != hipSuccess)
        rc = hip_fail(r, "H2D square");
    if (!rc) rc = rsm_proof_nodes_dev(ctx, sq.ptr, W, S, 1, nmt, ps.d_nodes, nullptr, sb.ptr, st);
    if (!rc && (r = hipMemcpyAsync(ps.status.data(), sb.ptr, (size_t)2 * W * 4, hipMemcpyDeviceToHost, st)) != hipSuccess)
        rc = hip_fail(r, "D2H tree status");
    if (!rc && (r = hipStreamSynchronize(st)) != hipSuccess) rc = hip_fail(r, "proof stream");
    if (rc) ps.drop();
    return rc;
}

}  // namespace

namespace rsm {
const rsm_nmt_params* eds_nmt_of(rsm_tree_root_fn tree_fn, void* user) { return nmt_of(tree_fn, user); }
bool eds_store_path(rsm_eds* e, const rsm_nmt_params* nmt, DevTree* dt) { return store_path(e, nmt, dt); }
int eds_ensure_store(rsm_eds* e, const rsm_nmt_params* nmt, const DevTree& dt) { return ensure_store(e, nmt, dt); }
}  // namespace rsm

extern "C" {

uint64_t rsm_proof_nodes_bytes(uint32_t width, const rsm_nmt_params* nmt, uint32_t count) {
    DevTree t;
    if (!proof_tree_for(width, nmt, &t)) return 0;
    if ((uint64_t)width * width * count >= (1ull << 32) || count > 65535) return 0;  // one launch
    return store_bytes(t, width, count);
}

uint32_t rsm_proof_record_bytes(uint32_t width, const rsm_nmt_params* nmt) {
    if (width == 0 || (nmt && nmt->namespace_size == 0)) return 0;
    return 8 + proof_levels(width) * (nmt ? 2 * nmt->namespace_size + 32 : 32);
}

int rsm_proof_nodes_dev(rsm_ctx* ctx, const void* d_eds, uint32_t width, uint32_t share_size, uint32_t count,
                        const rsm_nmt_params* nmt, void* d_nodes, void* d_roots, void* d_status, void* stream) {
    if (!ctx || !d_eds || !d_nodes || width == 0) return fail(RSM_EINVAL, "rsm_proof_nodes_dev: bad arguments");
    if ((reinterpret_cast<uintptr_t>(d_nodes) & 15u) || (reinterpret_cast<uintptr_t>(d_eds) & 15u))
        return fail(RSM_EINVAL, "rsm_proof_nodes_dev: d_eds and d_nodes must be 16-byte aligned");
    if (int rc = validate_chunk_size(share_size)) return rc;
    if (share_size == 0) return fail(RSM_EINVAL, "rsm_proof_nodes_dev: empty shares");
    DevTree t;
    if (!proof_tree_for(width, nmt, &t) || (count && rsm_proof_nodes_bytes(width, nmt, count) == 0))
        return fail(RSM_EUNSUPPORTED, "rsm_proof_nodes_dev: %u squares of width %u%s not supported", count, width,
                    nmt ? " (NMT)" : "");
    if (count == 0) return RSM_OK;
    if (t.nmt && share_size < t.p.namespace_size) return fail(RSM_ETREE, "data is too short to contain namespace ID");
    if (int rc = use_device(ctx)) return rc;
    hipStream_t st = pick(ctx, stream);
    hipError_t e;
    if (t.nmt) {
        e = launch_nmt_nodes(static_cast<const uint8_t*>(d_eds), width, share_size, t.p.namespace_size, t.p.square_size,
                             t.p.ignore_max_namespace, count, static_cast<uint32_t*>(d_nodes),
                             static_cast<uint8_t*>(d_roots), static_cast<uint32_t*>(d_status), st);
    } else {
        if (d_status && (e = hipMemsetAsync(d_status, 0, (size_t)count * 2 * width * 4, st)) != hipSuccess)
            return hip_fail(e, "hipMemsetAsync (status)");
        e = launch_tree_nodes(static_cast<const uint8_t*>(d_eds), width, share_size, count,
                              static_cast<uint32_t*>(d_nodes), static_cast<uint8_t*>(d_roots), st);
    }
    return e == hipSuccess ? RSM_OK : hip_fail(e, "node store kernel launch");
}

int rsm_proofs_dev(rsm_ctx* ctx, const void* d_nodes, const void* d_eds, uint32_t width, uint32_t share_size,
                   uint32_t count, const rsm_nmt_params* nmt, const rsm_sample* samples, uint32_t n, void* d_records,
                   void* d_shares, void* stream) {
    if (!ctx || !d_nodes || width == 0 || (n && (!samples || !d_records)))
        return fail(RSM_EINVAL, "rsm_proofs_dev: bad arguments");
    if (d_shares && !d_eds) return fail(RSM_EINVAL, "rsm_proofs_dev: d_shares needs d_eds");
    if (d_shares && ((reinterpret_cast<uintptr_t>(d_shares) & 15u) || (reinterpret_cast<uintptr_t>(d_eds) & 15u)))
        return fail(RSM_EINVAL, "rsm_proofs_dev: d_eds and d_shares must be 16-byte aligned");
    if (int rc = validate_chunk_size(share_size)) return rc;
    DevTree t;
    if (!proof_tree_for(width, nmt, &t) || rsm_proof_nodes_bytes(width, nmt, count ? count : 1) == 0)
        return fail(RSM_EUNSUPPORTED, "rsm_proofs_dev: %u squares of width %u%s not supported", count, width,
                    nmt ? " (NMT)" : "");
    if (n > (1u << 24)) return fail(RSM_EINVAL, "rsm_proofs_dev: at most %u samples per call", 1u << 24);
    if (int rc = check_samples("rsm_proofs_dev", samples, n, count, width)) return rc;
    if (n == 0) return RSM_OK;
    if (int rc = use_device(ctx)) return rc;
    hipStream_t st = pick(ctx, stream);
    StreamScratch& ss = stream_scratch(ctx, st);
    std::lock_guard<std::mutex> lk(ss.mu);
    hipError_t e;
    const ProofSample* ds = nullptr;
    if (int rc = stage_samples(st, ss, samples, n, &ds)) return rc;
    if ((e = launch_proof_gather(static_cast<const uint32_t*>(d_nodes), width, count, t.nmt ? t.p.namespace_size : 0u,
                                 ds, n, static_cast<uint8_t*>(d_records), st)) != hipSuccess)
        return hip_fail(e, "proof gather kernel launch");
    if (d_shares && (e = launch_share_gather(static_cast<const uint8_t*>(d_eds), width, share_size, ds, n,
                                             static_cast<uint8_t*>(d_shares), st)) != hipSuccess)
        return hip_fail(e, "share gather kernel launch");
    return RSM_OK;
}

int rsm_proofs_verify_dev(rsm_ctx* ctx, const void* d_shares, const void* d_records, const void* d_roots,
                          uint32_t width, uint32_t share_size, uint32_t count, const rsm_nmt_params* nmt,
                          const rsm_sample* samples, uint32_t n, void* d_status, void* stream) {
    const auto* sh = static_cast<const uint8_t*>(d_shares);
    const auto* rec = static_cast<const uint8_t*>(d_records);
    const auto* roots = static_cast<const uint8_t*>(d_roots);
    return verify_call("rsm_proofs_verify_dev", ctx, samples && d_shares && d_records && d_roots && d_status, d_shares,
                       d_status, width, share_size, count, nmt, samples, n, stream, "proof verify kernel launch",
                       [&](const ProofSample* ds, uint32_t* status, hipStream_t st) {
                           return nmt ? launch_nmt_proof_verify(sh, rec, roots, width, share_size, nmt->namespace_size,
                                                                nmt->square_size, nmt->ignore_max_namespace, ds, n, status, st)
                                      : launch_proof_verify(sh, rec, roots, width, share_size, ds, n, status, st);
                       });
}

uint32_t rsm_data_root_record_bytes(uint32_t width) { return width == 0 ? 0 : 8 + proof_levels(2 * width) * 32; }

uint64_t rsm_data_root_nodes_bytes(uint32_t width, uint32_t count) {
    if (!data_roots_dev_supported(width)) return 0;
    return (uint64_t)count * data_root_tree_words(width) * 4;
}

int rsm_data_roots_dev(rsm_ctx* ctx, const void* d_roots, uint32_t width, uint32_t root_len, uint32_t count,
                       void* d_data_roots, void* d_nodes, void* stream) {
    if (!ctx || width == 0 || (count && (!d_roots || !d_data_roots)))
        return fail(RSM_EINVAL, "rsm_data_roots_dev: bad arguments");
    if (root_len < 32 || root_len > 96) return fail(RSM_EINVAL, "rsm_data_roots_dev: roots of %u bytes (32..96)", root_len);
    if (reinterpret_cast<uintptr_t>(d_nodes) & 15u)
        return fail(RSM_EINVAL, "rsm_data_roots_dev: d_nodes must be 16-byte aligned");
    if (!data_roots_dev_supported(width))
        return fail(RSM_EUNSUPPORTED, "rsm_data_roots_dev: width %u not supported (at most %u)", width, kDataRootMaxWidth);
    if (count == 0) return RSM_OK;
    if (int rc = use_device(ctx)) return rc;
    const hipError_t e = launch_data_roots(static_cast<const uint8_t*>(d_roots), width, root_len, count,
                                           static_cast<uint8_t*>(d_data_roots), static_cast<uint32_t*>(d_nodes),
                                           pick(ctx, stream));
    return e == hipSuccess ? RSM_OK : hip_fail(e, "data root kernel launch");
}

int rsm_root_proofs_dev(rsm_ctx* ctx, const void* d_nodes, uint32_t width, uint32_t count, const rsm_root_ref* refs,
                        uint32_t n, void* d_records, void* stream) {
    if (!ctx || !d_nodes || width == 0 || (n && (!refs || !d_records)))
        return fail(RSM_EINVAL, "rsm_root_proofs_dev: bad arguments");
    if (reinterpret_cast<uintptr_t>(d_nodes) & 15u)
        return fail(RSM_EINVAL, "rsm_root_proofs_dev: d_nodes must be 16-byte aligned");
    if (!data_roots_dev_supported(width))
        return fail(RSM_EUNSUPPORTED, "rsm_root_proofs_dev: width %u not supported (at most %u)", width, kDataRootMaxWidth);
    if (n > (1u << 24)) return fail(RSM_EINVAL, "rsm_root_proofs_dev: at most %u refs per call", 1u << 24);
    if (int rc = check_refs("rsm_root_proofs_dev", "ref", refs, n, count, width)) return rc;
    if (n == 0) return RSM_OK;
    if (int rc = use_device(ctx)) return rc;
    hipStream_t st = pick(ctx, stream);
    StreamScratch& ss = stream_scratch(ctx, st);
    std::lock_guard<std::mutex> lk(ss.mu);
    const void* dr = nullptr;
    if (int rc = stage_bytes(st, ss, refs, (size_t)n * sizeof(rsm_root_ref), &dr)) return rc;
    const hipError_t e = launch_data_root_gather(static_cast<const uint32_t*>(d_nodes), width,
                                                 static_cast<const RootRef*>(dr), n, static_cast<uint8_t*>(d_records), st);
    return e == hipSuccess ? RSM_OK : hip_fail(e, "root proof gather kernel launch");
}

int rsm_proofs_verify_data_root_dev(rsm_ctx* ctx, const void* d_shares, const void* d_records, const void* d_root_records,
                                    const void* d_data_roots, uint32_t width, uint32_t share_size, uint32_t count,
                                    const rsm_nmt_params* nmt, const rsm_sample* samples, uint32_t n, void* d_status,
                                    void* stream) {
    const auto* sh = static_cast<const uint8_t*>(d_shares);
    const auto* rec = static_cast<const uint8_t*>(d_records);
    const auto* rrec = static_cast<const uint8_t*>(d_root_records);
    const auto* dr = static_cast<const uint8_t*>(d_data_roots);
    return verify_call(
        "rsm_proofs_verify_data_root_dev", ctx, samples && d_shares && d_records && d_root_records && d_data_roots && d_status,
        d_shares, d_status, width, share_size, count, nmt, samples, n, stream, "chained proof verify kernel launch",
        [&](const ProofSample* ds, uint32_t* status, hipStream_t st) {
            return nmt ? launch_nmt_proof_verify_data_root(sh, rec, rrec, dr, width, share_size, nmt->namespace_size,
                                                           nmt->square_size, nmt->ignore_max_namespace, ds, n, status, st)
                       : launch_proof_verify_data_root(sh, rec, rrec, dr, width, share_size, ds, n, status, st);
        });
}

int rsm_eds_data_root(rsm_eds* e, rsm_tree_root_fn tree_fn, void* user, uint8_t* out) {
    if (!e || !out) return fail(RSM_EINVAL, "rsm_eds_data_root: bad arguments");
    const uint32_t W = e->width, S = e->S;
    if (W == 0) return fail(RSM_EINVAL, "rsm_eds_data_root: empty square");
    DevTree dt;
    const bool complete = memchr(e->present.data(), 0, e->present.size()) == nullptr;
    // the condition under which rsm_eds_roots takes the device, and a width the build takes
    if (e->ctx && complete && device_tree_for(tree_fn, user, W, &dt) && rsm_data_root_nodes_bytes(W, 1) != 0) {
        rsm_ctx* ctx = e->ctx;
        std::lock_guard<std::mutex> lk(ctx->eds_mu);
        if (int rc = use_device(ctx)) return rc;
        hipStream_t st = ctx->stream;
        hipError_t r;
        DevBuf& sq = ctx->eds.eds;
        DevBuf& rb = ctx->eds.roots;
        DevBuf& sb = ctx->eds.status;
        // roots | the data root, in one buffer
        const size_t o_dr = ((size_t)2 * W * dt.root_len + 15u) & ~(size_t)15u;
        if ((r = sq.ensure(e->data.size())) != hipSuccess || (r = rb.ensure(o_dr + 32)) != hipSuccess ||
            (r = sb.ensure((size_t)2 * W * 4)) != hipSuccess)
            return hip_fail(r, "hipMalloc (data root)");
        if ((r = hipMemcpyAsync(sq.ptr, e->data.data(), e->data.size(), hipMemcpyHostToDevice, st)) != hipSuccess)
            return hip_fail(r, "H2D square");
        auto* d_roots = static_cast<uint8_t*>(rb.ptr);
        if (int rc = device_tree_roots(ctx, dt, static_cast<const uint8_t*>(sq.ptr), W, S, d_roots,
                                       static_cast<uint32_t*>(sb.ptr), st))
            return rc;
        if (int rc = rsm_data_roots_dev(ctx, d_roots, W, dt.root_len, 1, d_roots + o_dr, nullptr, st)) return rc;
        std::vector<uint32_t> status((size_t)2 * W);
        uint8_t got[32];
        if ((r = hipMemcpyAsync(got, d_roots + o_dr, 32, hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (r = hipMemcpyAsync(status.data(), sb.ptr, status.size() * 4, hipMemcpyDeviceToHost, st)) != hipSuccess)
            return hip_fail(r, "D2H data root");
        if ((r = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(r, "data root stream");
        for (uint32_t i = 0; i < 2 * W; ++i)
            if (status[i]) return fail(RSM_ETREE, "tree error computing root %u (namespace push order)", i % W);
        memcpy(out, got, 32);
        return RSM_OK;
    }
    constexpr uint32_t kCap = 96;  // the longest root a data-root leaf takes
    std::vector<uint8_t> wide((size_t)2 * W * kCap);
    uint32_t len[2] = {0, 0};
    for (int axis = 0; axis < 2; ++axis)
        if (int rc = rsm_eds_roots(e, axis, tree_fn, user, wide.data() + (size_t)axis * W * kCap, kCap, &len[axis])) return rc;
    if (len[0] != len[1] || len[0] == 0)
        return fail(RSM_ETREE, "rsm_eds_data_root: row roots of %u bytes, column roots of %u", len[0], len[1]);
    std::vector<uint8_t> roots((size_t)2 * W * len[0]);
    for (uint32_t t = 0; t < 2 * W; ++t) memcpy(&roots[(size_t)t * len[0]], &wide[(size_t)t * kCap], len[0]);
    if (int rc = rsm_data_root(roots.data(), W, len[0], out)) return fail(rc, "rsm_eds_data_root: bad roots");
    return RSM_OK;
}

int rsm_eds_import_samples(rsm_eds* e, const uint8_t* row_roots, const uint8_t* col_roots, uint32_t root_len,
                           rsm_tree_root_fn tree_fn, void* user, const rsm_sample* samples, uint32_t n,
                           const uint8_t* shares, const uint8_t* records, uint32_t* status_out, uint32_t* accepted) {
    if (!e || !row_roots || !col_roots || (n && (!samples || !shares || !records)))
        return fail(RSM_EINVAL, "rsm_eds_import_samples: bad arguments");
    const rsm_nmt_params* nmt = nullptr;
    if (tree_fn == rsm_nmt_tree_root && user) nmt = static_cast<const rsm_nmt_params*>(user);
    else if (tree_fn != nullptr && tree_fn != rsm_default_tree_root)
        return fail(RSM_EUNSUPPORTED, "rsm_eds_import_samples: samples are verified for the DefaultTree and the NMT only");
    const uint32_t W = e->width, S = e->S;
    if (nmt && (nmt->namespace_size == 0 || nmt->square_size == 0))
        return fail(RSM_EINVAL, "rsm_eds_import_samples: namespace size or square size 0");
    const uint32_t NL = nmt ? 2 * nmt->namespace_size + 32 : 32, RB = 8 + proof_levels(W) * NL;
    if (root_len != NL) return fail(RSM_EINVAL, "rsm_eds_import_samples: roots of %u bytes, the tree's have %u", root_len, NL);
    if (nmt && S < nmt->namespace_size) return fail(RSM_ETREE, "data is too short to contain namespace ID");
    if (int rc = check_samples("rsm_eds_import_samples", samples, n, 1, W)) return rc;
    if (accepted) *accepted = 0;
    if (n == 0) return RSM_OK;
    std::vector<uint32_t> status(n);
    if (e->ctx && W <= 65536u && n <= (1u << 24) && (!nmt || nmt->namespace_size <= 32)) {
        rsm_ctx* ctx = e->ctx;
        std::lock_guard<std::mutex> lk(ctx->eds_mu);
        if (int rc = use_device(ctx)) return rc;
        hipStream_t st = ctx->stream;
        hipError_t r;
        // one upload: shares | row roots | column roots | records
        const size_t o_roots = (size_t)n * S, o_rec = o_roots + (size_t)2 * W * NL, total = o_rec + (size_t)n * RB;
        std::vector<uint8_t> pack(total);
        memcpy(pack.data(), shares, (size_t)n * S);
        memcpy(pack.data() + o_roots, row_roots, (size_t)W * NL);
        memcpy(pack.data() + o_roots + (size_t)W * NL, col_roots, (size_t)W * NL);
        memcpy(pack.data() + o_rec, records, (size_t)n * RB);
        DevBuf& in = ctx->eds.scratch;
        DevBuf& sb = ctx->eds.status;
        if ((r = in.ensure(total)) != hipSuccess || (r = sb.ensure((size_t)n * 4)) != hipSuccess)
            return hip_fail(r, "hipMalloc (samples to verify)");
        auto* d = static_cast<uint8_t*>(in.ptr);
        if ((r = hipMemcpyAsync(d, pack.data(), total, hipMemcpyHostToDevice, st)) != hipSuccess)
            return hip_fail(r, "H2D samples to verify");
        if (int rc = rsm_proofs_verify_dev(ctx, d, d + o_rec, d + o_roots, W, S, 1, nmt, samples, n, sb.ptr, st)) return rc;
        if ((r = hipMemcpyAsync(status.data(), sb.ptr, (size_t)n * 4, hipMemcpyDeviceToHost, st)) != hipSuccess)
            return hip_fail(r, "D2H sample statuses");
        if ((r = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(r, "verify stream");
    } else {
        for (uint32_t i = 0; i < n; ++i) {
            const rsm_sample& s = samples[i];
            const uint8_t* root = (s.axis == RSM_AXIS_ROW ? row_roots : col_roots) + (size_t)s.index * NL;
            const uint8_t* sh = shares + (size_t)i * S;
            const uint8_t* rec = records + (size_t)i * RB;
            const int rc = nmt ? rsm_nmt_tree_verify(nmt, s.index, sh, S, W, s.pos, rec, root, &status[i])
                               : rsm_default_tree_verify(sh, S, W, s.pos, rec, root, &status[i]);
            if (rc) return fail(rc, "rsm_eds_import_samples: bad tree parameters");
        }
    }
    uint32_t set = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const rsm_sample& s = samples[i];
        const uint32_t r = e->rr((int)s.axis, s.index, s.pos), c = e->cc((int)s.axis, s.index, s.pos);
        if (status[i] == RSM_PROOF_OK) {
            if (e->has(r, c)) {
                status[i] = RSM_PROOF_OCCUPIED;
            } else {
                e->proofs.drop();  // as SetCell: the cached tree nodes no longer match
                memcpy(e->cell(r, c), shares + (size_t)i * S, S);
                e->present[(size_t)r * W + c] = 1;
                ++set;
            }
        }
        if (status_out) status_out[i] = status[i];
    }
    if (accepted) *accepted = set;
    return RSM_OK;
}

int rsm_eds_proofs(rsm_eds* e, rsm_tree_root_fn tree_fn, void* user, const rsm_sample* samples, uint32_t n,
                   uint8_t* records_out, uint8_t* shares_out) {
    if (!e || (n && (!samples || !records_out))) return fail(RSM_EINVAL, "rsm_eds_proofs: bad arguments");
    const rsm_nmt_params* nmt = nmt_of(tree_fn, user);
    if (!nmt && tree_fn != nullptr && tree_fn != rsm_default_tree_root)
        return fail(RSM_EUNSUPPORTED, "rsm_eds_proofs: proofs are built for the DefaultTree and the NMT only");
    const uint32_t W = e->width, S = e->S;
    if (int rc = check_samples("rsm_eds_proofs", samples, n, 1, W)) return rc;
    const uint32_t RB = rsm_proof_record_bytes(W, nmt);
    if (n && RB == 0) return fail(RSM_EINVAL, "rsm_eds_proofs: namespace size 0");
    auto cell_of = [&](const rsm_sample& s) { return e->cell(e->rr((int)s.axis, s.index, s.pos), e->cc((int)s.axis, s.index, s.pos)); };
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t p = 0; p < W; ++p)
            if (!e->has(e->rr((int)samples[i].axis, samples[i].index, p), e->cc((int)samples[i].axis, samples[i].index, p)))
                return fail(RSM_ETREE, "can not prove a share of incomplete %s %u", samples[i].axis == 0 ? "row" : "column",
                            samples[i].index);
    if (n == 0) return RSM_OK;
    DevTree dt;
    if (store_path(e, nmt, &dt)) {
        rsm_ctx* ctx = e->ctx;
        std::lock_guard<std::mutex> lk(ctx->eds_mu);
        if (int rc = use_device(ctx)) return rc;
        hipStream_t st = ctx->stream;
        hipError_t r;
        if (int rc = ensure_store(e, nmt, dt)) return rc;
        ProofStore& ps = e->proofs;
        for (uint32_t i = 0; i < n; ++i)
            if (ps.status[(size_t)samples[i].axis * W + samples[i].index])
                return fail(RSM_ETREE, "tree error proving a share of %s %u (namespace order)",
                            samples[i].axis == 0 ? "row" : "column", samples[i].index);
        DevBuf& rb = ctx->eds.scratch;
        if ((r = rb.ensure((size_t)n * RB)) != hipSuccess) return hip_fail(r, "hipMalloc (proof records)");
        if (int rc = rsm_proofs_dev(ctx, ps.d_nodes, nullptr, W, S, 1, nmt, samples, n, rb.ptr, nullptr, st)) return rc;
        if ((r = hipMemcpyAsync(records_out, rb.ptr, (size_t)n * RB, hipMemcpyDeviceToHost, st)) != hipSuccess)
            return hip_fail(r, "D2H proof records");
        if ((r = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(r, "proof stream");
    } else {
        std::vector<const uint8_t*> leaves(W);
        for (uint32_t i = 0; i < n; ++i) {
            const rsm_sample& s = samples[i];
            for (uint32_t p = 0; p < W; ++p) leaves[p] = e->cell(e->rr((int)s.axis, s.index, p), e->cc((int)s.axis, s.index, p));
            uint8_t* rec = records_out + (size_t)i * RB;
            const int rc = nmt ? rsm_nmt_tree_prove(nmt, s.index, leaves.data(), W, S, s.pos, rec, nullptr)
                               : rsm_default_tree_prove(leaves.data(), W, S, s.pos, rec, nullptr);
            if (rc == RSM_ETREE)
                return fail(RSM_ETREE, "tree error proving a share of %s %u", s.axis == 0 ? "row" : "column", s.index);
            if (rc) return fail(rc, "rsm_eds_proofs: bad tree parameters");
        }
    }
    if (shares_out)
        for (uint32_t i = 0; i < n; ++i) memcpy(shares_out + (size_t)i * S, cell_of(samples[i]), S);
    return RSM_OK;
}

int rsm_ns_proofs_dev(rsm_ctx* ctx, const void* d_nodes, const void* d_status, const void* d_eds, uint32_t width,
                      uint32_t share_size, uint32_t count, const rsm_nmt_params* nmt, const rsm_ns_query* queries,
                      const uint8_t* nids, uint32_t n, void* d_records, void* d_offsets, void* d_shares,
                      uint64_t shares_cap, void* stream) {
    if (!ctx || !d_nodes || !d_status || width == 0 || (n && (!queries || !nids || !d_records || !d_offsets)))
        return fail(RSM_EINVAL, "rsm_ns_proofs_dev: bad arguments");
    if (!nmt) return fail(RSM_EUNSUPPORTED, "rsm_ns_proofs_dev: the DefaultTree has no namespaces");
    if (d_shares && !d_eds) return fail(RSM_EINVAL, "rsm_ns_proofs_dev: d_shares needs d_eds");
    if (d_shares && ((reinterpret_cast<uintptr_t>(d_shares) & 15u) || (reinterpret_cast<uintptr_t>(d_eds) & 15u)))
        return fail(RSM_EINVAL, "rsm_ns_proofs_dev: d_eds and d_shares must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(d_nodes) & 15u) || (reinterpret_cast<uintptr_t>(d_offsets) & 3u) ||
        (reinterpret_cast<uintptr_t>(d_status) & 3u))
        return fail(RSM_EINVAL, "rsm_ns_proofs_dev: d_nodes must be 16-byte, d_status and d_offsets 4-byte aligned");
    if (int rc = validate_chunk_size(share_size)) return rc;
    DevTree t;
    if (!proof_tree_for(width, nmt, &t) || !t.nmt || rsm_proof_nodes_bytes(width, nmt, count ? count : 1) == 0)
        return fail(RSM_EUNSUPPORTED, "rsm_ns_proofs_dev: %u squares of width %u (NMT) not supported", count, width);
    if (n > (1u << 20)) return fail(RSM_EINVAL, "rsm_ns_proofs_dev: at most %u queries per call", 1u << 20);
    if (n == 0 || count == 0) return RSM_OK;
    const uint32_t ns = t.p.namespace_size;
    std::vector<NsQuery> q;
    if (int rc = pack_ns_queries("rsm_ns_proofs_dev", queries, nids, n, ns, count, width, &q)) return rc;
    if (int rc = use_device(ctx)) return rc;
    hipStream_t st = pick(ctx, stream);
    StreamScratch& ss = stream_scratch(ctx, st);
    std::lock_guard<std::mutex> lk(ss.mu);
    const void* dq = nullptr;
    if (int rc = stage_bytes(st, ss, q.data(), (size_t)n * sizeof(NsQuery), &dq)) return rc;
    const hipError_t e = launch_ns_proofs(static_cast<const uint32_t*>(d_nodes), static_cast<const uint32_t*>(d_status),
                                          static_cast<const uint8_t*>(d_eds), width, share_size, count, ns,
                                          static_cast<const NsQuery*>(dq), n, static_cast<uint8_t*>(d_records),
                                          static_cast<uint32_t*>(d_offsets), static_cast<uint8_t*>(d_shares), shares_cap,
                                          st);
    return e == hipSuccess ? RSM_OK : hip_fail(e, "namespace proof kernel launch");
}

int rsm_ns_proofs_verify_dev(rsm_ctx* ctx, const void* d_records, const void* d_offsets, const void* d_shares,
                             uint64_t shares_total, const void* d_roots, uint32_t width, uint32_t share_size,
                             uint32_t count, const rsm_nmt_params* nmt, const rsm_ns_query* queries,
                             const uint8_t* nids, uint32_t n, void* d_status, void* stream) {
    if (!ctx || width == 0 ||
        (n && count && (!queries || !nids || !d_records || !d_offsets || !d_roots || !d_status || (shares_total && !d_shares))))
        return fail(RSM_EINVAL, "rsm_ns_proofs_verify_dev: bad arguments");
    if (!nmt) return fail(RSM_EUNSUPPORTED, "rsm_ns_proofs_verify_dev: the DefaultTree has no namespaces");
    if (nmt->namespace_size == 0 || nmt->namespace_size > 32 || nmt->square_size == 0)
        return fail(RSM_EINVAL, "rsm_ns_proofs_verify_dev: namespace size %u (1..32) or square size 0", nmt->namespace_size);
    if (reinterpret_cast<uintptr_t>(d_shares) & 15u)
        return fail(RSM_EINVAL, "rsm_ns_proofs_verify_dev: d_shares must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(d_offsets) & 3u) || (reinterpret_cast<uintptr_t>(d_status) & 3u))
        return fail(RSM_EINVAL, "rsm_ns_proofs_verify_dev: d_offsets and d_status must be 4-byte aligned");
    if (int rc = validate_chunk_size(share_size)) return rc;
    if (!nmt_ns_verify_supported(width, nmt->namespace_size))
        return fail(RSM_EUNSUPPORTED, "rsm_ns_proofs_verify_dev: width %u not supported (at most 1024)", width);
    if (share_size < nmt->namespace_size) return fail(RSM_ETREE, "data is too short to contain namespace ID");
    if (n > (1u << 20)) return fail(RSM_EINVAL, "rsm_ns_proofs_verify_dev: at most %u queries per call", 1u << 20);
    if (n == 0 || count == 0) return RSM_OK;
    const uint32_t ns = nmt->namespace_size;
    std::vector<NsQuery> q;
    if (int rc = pack_ns_queries("rsm_ns_proofs_verify_dev", queries, nids, n, ns, count, width, &q)) return rc;
    if (int rc = use_device(ctx)) return rc;
    hipStream_t st = pick(ctx, stream);
    StreamScratch& ss = stream_scratch(ctx, st);
    std::lock_guard<std::mutex> lk(ss.mu);
    const void* dq = nullptr;
    if (int rc = stage_bytes(st, ss, q.data(), (size_t)n * sizeof(NsQuery), &dq)) return rc;
    const hipError_t e = launch_nmt_ns_verify(
        static_cast<const uint8_t*>(d_records), static_cast<const uint32_t*>(d_offsets), static_cast<const uint8_t*>(d_shares),
        shares_total, static_cast<const uint8_t*>(d_roots), width, share_size, ns, nmt->square_size,
        nmt->ignore_max_namespace, static_cast<const NsQuery*>(dq), n, static_cast<uint32_t*>(d_status), st);
    return e == hipSuccess ? RSM_OK : hip_fail(e, "namespace proof verify kernel launch");
}

int rsm_eds_namespace_proofs(rsm_eds* e, rsm_tree_root_fn tree_fn, void* user, int axis, const uint32_t* indices,
                             uint32_t n, const uint8_t* nid, uint8_t* records_out, uint32_t* offsets_out,
                             uint8_t* shares_out, uint64_t shares_cap) {
    if (!e || !nid || !offsets_out || (axis != RSM_AXIS_ROW && axis != RSM_AXIS_COL) || (n && (!indices || !records_out)))
        return fail(RSM_EINVAL, "rsm_eds_namespace_proofs: bad arguments");
    const rsm_nmt_params* nmt = nmt_of(tree_fn, user);
    if (!nmt) return fail(RSM_EUNSUPPORTED, "rsm_eds_namespace_proofs: namespace proofs are built for the NMT only");
    const uint32_t W = e->width, S = e->S;
    const uint32_t RB = rsm_ns_record_bytes(W, nmt);
    if (RB == 0 || nmt->square_size == 0) return fail(RSM_EINVAL, "rsm_eds_namespace_proofs: namespace size or square size 0");
    for (uint32_t i = 0; i < n; ++i) {
        if (indices[i] >= W)
            return fail(RSM_EINVAL, "rsm_eds_namespace_proofs: %s %u is out of range", axis == 0 ? "row" : "column", indices[i]);
        for (uint32_t p = 0; p < W; ++p)
            if (!e->has(e->rr(axis, indices[i], p), e->cc(axis, indices[i], p)))
                return fail(RSM_ETREE, "can not prove a namespace of incomplete %s %u", axis == 0 ? "row" : "column", indices[i]);
    }
    offsets_out[0] = 0;
    if (n == 0) return RSM_OK;
    DevTree dt;
    if (n <= (1u << 20) && store_path(e, nmt, &dt)) {
        rsm_ctx* ctx = e->ctx;
        std::lock_guard<std::mutex> lk(ctx->eds_mu);
        if (int rc = use_device(ctx)) return rc;
        hipStream_t st = ctx->stream;
        hipError_t r;
        if (int rc = ensure_store(e, nmt, dt)) return rc;
        ProofStore& ps = e->proofs;
        for (uint32_t i = 0; i < n; ++i)
            if (ps.status[(size_t)axis * W + indices[i]])
                return fail(RSM_ETREE, "tree error proving a namespace of %s %u (namespace order)", axis == 0 ? "row" : "column",
                            indices[i]);
        // offsets | records in one scratch buffer; the shares are this square's host bytes
        const size_t o_rec = (size_t)(n + 1) * 4, total = o_rec + (size_t)n * RB;
        DevBuf& rb = ctx->eds.scratch;
        DevBuf& sb = ctx->eds.status;
        if ((r = rb.ensure(total)) != hipSuccess || (r = sb.ensure((size_t)2 * W * 4)) != hipSuccess)
            return hip_fail(r, "hipMalloc (namespace proof records)");
        if ((r = hipMemcpyAsync(sb.ptr, ps.status.data(), (size_t)2 * W * 4, hipMemcpyHostToDevice, st)) != hipSuccess)
            return hip_fail(r, "H2D tree status");
        std::vector<rsm_ns_query> q(n);
        std::vector<uint8_t> nids((size_t)n * nmt->namespace_size);
        for (uint32_t i = 0; i < n; ++i) {
            q[i] = rsm_ns_query{0, (uint32_t)axis, indices[i]};
            memcpy(&nids[(size_t)i * nmt->namespace_size], nid, nmt->namespace_size);
        }
        auto* d = static_cast<uint8_t*>(rb.ptr);
        if (int rc = rsm_ns_proofs_dev(ctx, ps.d_nodes, sb.ptr, nullptr, W, S, 1, nmt, q.data(), nids.data(), n, d + o_rec, d,
                                       nullptr, 0, st))
            return rc;
        if ((r = hipMemcpyAsync(offsets_out, d, o_rec, hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (r = hipMemcpyAsync(records_out, d + o_rec, (size_t)n * RB, hipMemcpyDeviceToHost, st)) != hipSuccess)
            return hip_fail(r, "D2H namespace proof records");
        if ((r = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(r, "proof stream");
    } else {
        std::vector<const uint8_t*> leaves(W);
        for (uint32_t i = 0; i < n; ++i) {
            for (uint32_t p = 0; p < W; ++p) leaves[p] = e->cell(e->rr(axis, indices[i], p), e->cc(axis, indices[i], p));
            uint8_t* rec = records_out + (size_t)i * RB;
            const int rc = rsm_nmt_namespace_prove(nmt, indices[i], leaves.data(), W, S, nid, rec, nullptr);
            if (rc == RSM_ETREE)
                return fail(RSM_ETREE, "tree error proving a namespace of %s %u", axis == 0 ? "row" : "column", indices[i]);
            if (rc) return fail(rc, "rsm_eds_namespace_proofs: bad tree parameters");
            offsets_out[i + 1] = offsets_out[i] + (le32(rec) == RSM_NS_INCLUSION ? le32(rec + 8) - le32(rec + 4) : 0u);
        }
    }
    if (shares_out)
        for (uint32_t i = 0; i < n; ++i) {
            if (offsets_out[i + 1] == offsets_out[i] || offsets_out[i + 1] > shares_cap) continue;
            const uint32_t start = le32(records_out + (size_t)i * RB + 4);
            for (uint32_t p = 0; p < offsets_out[i + 1] - offsets_out[i]; ++p)
                memcpy(shares_out + (size_t)(offsets_out[i] + p) * S, e->cell(e->rr(axis, indices[i], start + p), e->cc(axis, indices[i], start + p)), S);
        }
    return RSM_OK;
}

uint32_t rsm_range_record_bytes(uint32_t width, const rsm_nmt_params* nmt) {
    if (width == 0 || (nmt && nmt->namespace_size == 0)) return 0;
    return 16 + (2 * proof_levels(width) + 1) * (nmt ? 2 * nmt->namespace_size + 32 : 32);
}

int rsm_range_proofs_dev(rsm_ctx* ctx, const void* d_nodes, const void* d_eds, uint32_t width, uint32_t share_size,
                         uint32_t count, const rsm_nmt_params* nmt, const rsm_range_query* queries, uint32_t n,
                         void* d_records, void* d_offsets, void* d_shares, uint64_t shares_cap, void* stream) {
    if (!ctx || !d_nodes || width == 0 || (n && (!queries || !d_records || !d_offsets)))
        return fail(RSM_EINVAL, "rsm_range_proofs_dev: bad arguments");
    if (d_shares && !d_eds) return fail(RSM_EINVAL, "rsm_range_proofs_dev: d_shares needs d_eds");
    if (d_shares && ((reinterpret_cast<uintptr_t>(d_shares) & 15u) || (reinterpret_cast<uintptr_t>(d_eds) & 15u)))
        return fail(RSM_EINVAL, "rsm_range_proofs_dev: d_eds and d_shares must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(d_nodes) & 15u) || (reinterpret_cast<uintptr_t>(d_offsets) & 3u))
        return fail(RSM_EINVAL, "rsm_range_proofs_dev: d_nodes must be 16-byte, d_offsets 4-byte aligned");
    if (int rc = validate_chunk_size(share_size)) return rc;
    DevTree t;
    if (!proof_tree_for(width, nmt, &t) || rsm_proof_nodes_bytes(width, nmt, count ? count : 1) == 0)
        return fail(RSM_EUNSUPPORTED, "rsm_range_proofs_dev: %u squares of width %u%s not supported", count, width,
                    nmt ? " (NMT)" : "");
    if (n > (1u << 20)) return fail(RSM_EINVAL, "rsm_range_proofs_dev: at most %u queries per call", 1u << 20);
    if (n == 0 || count == 0) return RSM_OK;
    if (int rc = check_range_queries("rsm_range_proofs_dev", queries, n, count, width)) return rc;
    if (int rc = use_device(ctx)) return rc;
    hipStream_t st = pick(ctx, stream);
    StreamScratch& ss = stream_scratch(ctx, st);
    std::lock_guard<std::mutex> lk(ss.mu);
    const void* dq = nullptr;
    if (int rc = stage_bytes(st, ss, queries, (size_t)n * sizeof(rsm_range_query), &dq)) return rc;
    const hipError_t e = launch_range_proofs(static_cast<const uint32_t*>(d_nodes), static_cast<const uint8_t*>(d_eds), width,
                                             share_size, count, t.nmt ? t.p.namespace_size : 0u,
                                             static_cast<const RangeQuery*>(dq), n, static_cast<uint8_t*>(d_records),
                                             static_cast<uint32_t*>(d_offsets), static_cast<uint8_t*>(d_shares), shares_cap, st);
    return e == hipSuccess ? RSM_OK : hip_fail(e, "range proof kernel launch");
}

int rsm_range_proofs_verify_dev(rsm_ctx* ctx, const void* d_records, const void* d_offsets, const void* d_shares,
                                uint64_t shares_total, const void* d_roots, uint32_t width, uint32_t share_size,
                                uint32_t count, const rsm_nmt_params* nmt, const rsm_range_query* queries, uint32_t n,
                                void* d_status, void* stream) {
    return range_verify_call("rsm_range_proofs_verify_dev", ctx, queries && d_records && d_offsets && d_roots && d_status,
                             d_records, d_offsets, d_shares, shares_total, d_roots, nullptr, nullptr, width, share_size, count,
                             nmt, queries, n, d_status, stream);
}

int rsm_range_proofs_verify_data_root_dev(rsm_ctx* ctx, const void* d_records, const void* d_offsets, const void* d_shares,
                                          uint64_t shares_total, const void* d_root_records, const void* d_data_roots,
                                          uint32_t width, uint32_t share_size, uint32_t count, const rsm_nmt_params* nmt,
                                          const rsm_range_query* queries, uint32_t n, void* d_status, void* stream) {
    return range_verify_call("rsm_range_proofs_verify_data_root_dev", ctx,
                             queries && d_records && d_offsets && d_root_records && d_data_roots && d_status, d_records,
                             d_offsets, d_shares, shares_total, nullptr, d_root_records, d_data_roots, width, share_size, count,
                             nmt, queries, n, d_status, stream);
}

int rsm_share_range_queries(uint32_t k, uint32_t square, uint32_t start, uint32_t end, rsm_range_query* queries_out,
                            uint32_t* n_out) {
    if (!queries_out || !n_out || k == 0 || k > 32768u || !(start < end && end <= k * k))
        return fail(RSM_EINVAL, "rsm_share_range_queries: bad arguments (1 <= k <= 32768, start < end <= k * k)");
    uint32_t n = 0;
    for (uint32_t row = start / k; row * k < end; ++row) {  // k * k <= 2^30
        const uint32_t lo = std::max(start, row * k), hi = std::min(end, (row + 1) * k);
        queries_out[n++] = rsm_range_query{square, RSM_AXIS_ROW, row, lo - row * k, hi - row * k};
    }
    *n_out = n;
    return RSM_OK;
}

int rsm_eds_range_proofs(rsm_eds* e, rsm_tree_root_fn tree_fn, void* user, const rsm_range_query* queries, uint32_t n,
                         uint8_t* records_out, uint32_t* offsets_out, uint8_t* shares_out, uint64_t shares_cap) {
    if (!e || !offsets_out || (n && (!queries || !records_out))) return fail(RSM_EINVAL, "rsm_eds_range_proofs: bad arguments");
    const rsm_nmt_params* nmt = nmt_of(tree_fn, user);
    if (!nmt && tree_fn != nullptr && tree_fn != rsm_default_tree_root)
        return fail(RSM_EUNSUPPORTED, "rsm_eds_range_proofs: range proofs are built for the DefaultTree and the NMT only");
    const uint32_t W = e->width, S = e->S;
    const uint32_t RB = rsm_range_record_bytes(W, nmt);
    if (RB == 0 || (nmt && nmt->square_size == 0))
        return fail(RSM_EINVAL, "rsm_eds_range_proofs: empty square, namespace size or square size 0");
    if (int rc = check_range_queries("rsm_eds_range_proofs", queries, n, 1, W)) return rc;
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t p = 0; p < W; ++p)
            if (!e->has(e->rr((int)queries[i].axis, queries[i].index, p), e->cc((int)queries[i].axis, queries[i].index, p)))
                return fail(RSM_ETREE, "can not prove a range of incomplete %s %u", queries[i].axis == 0 ? "row" : "column",
                            queries[i].index);
    offsets_out[0] = 0;
    for (uint32_t i = 0; i < n; ++i) offsets_out[i + 1] = offsets_out[i] + (queries[i].end - queries[i].start);
    if (n == 0) return RSM_OK;
    DevTree dt;
    if (n <= (1u << 20) && store_path(e, nmt, &dt)) {
        rsm_ctx* ctx = e->ctx;
        std::lock_guard<std::mutex> lk(ctx->eds_mu);
        if (int rc = use_device(ctx)) return rc;
        hipStream_t st = ctx->stream;
        hipError_t r;
        if (int rc = ensure_store(e, nmt, dt)) return rc;
        ProofStore& ps = e->proofs;
        for (uint32_t i = 0; i < n; ++i)
            if (ps.status[(size_t)queries[i].axis * W + queries[i].index])
                return fail(RSM_ETREE, "tree error proving a range of %s %u (namespace order)",
                            queries[i].axis == 0 ? "row" : "column", queries[i].index);
        // offsets | records in one scratch buffer; the shares are this square's host bytes
        const size_t o_rec = (size_t)(n + 1) * 4, total = o_rec + (size_t)n * RB;
        DevBuf& rb = ctx->eds.scratch;
        if ((r = rb.ensure(total)) != hipSuccess) return hip_fail(r, "hipMalloc (range proof records)");
        auto* d = static_cast<uint8_t*>(rb.ptr);
        if (int rc = rsm_range_proofs_dev(ctx, ps.d_nodes, nullptr, W, S, 1, nmt, queries, n, d + o_rec, d, nullptr, 0, st))
            return rc;
        if ((r = hipMemcpyAsync(records_out, d + o_rec, (size_t)n * RB, hipMemcpyDeviceToHost, st)) != hipSuccess)
            return hip_fail(r, "D2H range proof records");
        if ((r = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(r, "proof stream");
    } else {
        std::vector<const uint8_t*> leaves(W);
        for (uint32_t i = 0; i < n; ++i) {
            const rsm_range_query& q = queries[i];
            for (uint32_t p = 0; p < W; ++p) leaves[p] = e->cell(e->rr((int)q.axis, q.index, p), e->cc((int)q.axis, q.index, p));
            uint8_t* rec = records_out + (size_t)i * RB;
            const int rc = nmt ? rsm_nmt_tree_range_prove(nmt, q.index, leaves.data(), W, S, q.start, q.end, rec, nullptr)
                               : rsm_default_tree_range_prove(leaves.data(), W, S, q.start, q.end, rec, nullptr);
            if (rc == RSM_ETREE)
                return fail(RSM_ETREE, "tree error proving a range of %s %u", q.axis == 0 ? "row" : "column", q.index);
            if (rc) return fail(rc, "rsm_eds_range_proofs: bad tree parameters");
        }
    }
    if (shares_out)
        for (uint32_t i = 0; i < n; ++i) {
            if (offsets_out[i + 1] > shares_cap) continue;
            const rsm_range_query& q = queries[i];
            for (uint32_t p = q.start; p < q.end; ++p)
                memcpy(shares_out + (size_t)(offsets_out[i] + p - q.start) * S,
                       e->cell(e->rr((int)q.axis, q.index, p), e->cc((int)q.axis, q.index, p)), S);
        }
    return RSM_OK;
}

}  // extern "C"
