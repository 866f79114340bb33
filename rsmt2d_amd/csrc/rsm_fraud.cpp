// rsm_fraud.cpp -- rsm_fraud_proofs_verify_dev: n bad-encoding fraud proofs, each a packed
// vector with the proofs of its shares in the orthogonal trees, validated as a batch on the
// device.  The share proofs go through the verify kernels, the missing slots through the
// existing decoders, the rebuilt vectors through the packed-vector trees of
// kernels_fraud.hip, the existing encoders and the parity compare; one kernel reduces all
// of it to the verdict records.
// Contract: include/rsmt2d_hip.h; design: DESIGN.md §5 "Fraud proofs".
#include "eds_internal.hpp"

#include <algorithm>
#include <cstring>

using namespace rsm;

static_assert(sizeof(rsm_fraud_verdict) == 16, "rsm_fraud_verdict is four words");
static_assert(RSM_FRAUD_VALID == kFraudValid && RSM_FRAUD_TOOFEW == kFraudTooFew && RSM_FRAUD_SHARE == kFraudShare &&
                  RSM_FRAUD_CONSISTENT == kFraudConsistent,
              "the verdict kernel's words are the C ABI's");
static_assert(RSM_PROOF_ROOT < 8, "the verdict kernel keeps a status word in three bits of its key");
static_assert(sizeof(rsm_root_ref) == sizeof(RootRef) && sizeof(rsm_sample) == sizeof(ProofSample),
              "the kernels' records are the C ABI's");

namespace {

// Sections of d_work.  The proofs are taken in chunks of W: a chunk is what the decoders and
// encoders address as the rows of one [W][W][S] square, whatever n is.
struct FraudLayout {
    uint64_t refs;     // [n] RootRef
    uint64_t have;     // [n] words: presence counts
    uint64_t slot;     // [n] words: a checked proof's word of chk / parity
    uint64_t tree;     // [n] words: the tree kernel's
    uint64_t dec;      // [chunks][W] words: chunk-local rows to decode
    uint64_t chk;      // [chunks][W] words: chunk-local rows to check
    uint64_t parity;   // [chunks][W] words: the parity compare's, laid out as chk
    uint64_t samples;  // [n][W] ProofSample
    uint64_t status;   // [n][W] words: the verify kernel's
    uint64_t leaf;     // [n][W] leaf records (32 bytes; NMT 64)
    uint64_t scratch;  // [min(n, W)][W][S]: re-encoded parity, one chunk at a time
    uint64_t total;
    uint32_t chunks;
};

// The device tree and the layout of (k, S, n, nmt); false beyond the limits.
bool fraud_shape(uint32_t k, uint32_t S, uint32_t n, const rsm_nmt_params* nmt, DevTree* t, FraudLayout* out) {
    if (k == 0 || k > 1024 || S == 0 || S % 64 != 0) return false;
    const uint64_t W = 2ull * k;
    if (!device_tree_for(nmt ? rsm_nmt_tree_root : nullptr, const_cast<rsm_nmt_params*>(nmt), (uint32_t)W, t) ||
        !fraud_supported((uint32_t)W, t->nmt ? t->p.namespace_size : 0u))
        return false;
    if (n > 65535 || n * W > (1ull << 24)) return false;
    FraudLayout l{};
    l.chunks = (uint32_t)((n + W - 1) / W);
    Carver c;
    l.refs = c.take((uint64_t)n * sizeof(RootRef));
    l.have = c.take((uint64_t)n * 4);
    l.slot = c.take((uint64_t)n * 4);
    l.tree = c.take((uint64_t)n * 4);
    l.dec = c.take(l.chunks * W * 4);
    l.chk = c.take(l.chunks * W * 4);
    l.parity = c.take(l.chunks * W * 4);
    l.samples = c.take(n * W * sizeof(ProofSample));
    l.status = c.take(n * W * 4);
    l.leaf = c.take(n * W * (t->nmt ? 64 : 32));
    l.scratch = c.take(std::min<uint64_t>(n, W) * W * S);
    l.total = c.at ? c.at : 256;
    *out = l;
    return true;
}

}  // namespace

extern "C" {

uint64_t rsm_fraud_work_bytes(uint32_t k, uint32_t share_size, uint32_t n, const rsm_nmt_params* nmt) {
    DevTree t;
    FraudLayout l;
    return fraud_shape(k, share_size, n, nmt, &t, &l) ? l.total : 0;
}

int rsm_fraud_proof_samples(const rsm_root_ref* ref, uint32_t k, rsm_sample* samples_out) {
    static const char* const fn = "rsm_fraud_proof_samples";
    if (!ref || !samples_out || k == 0 || k > 32768u) return fail(RSM_EINVAL, "%s: bad arguments", fn);
    if (ref->axis > 1 || ref->index >= 2 * k)
        return fail(RSM_EINVAL, "%s: ref (square %u, axis %u, index %u) is out of range", fn, ref->square, ref->axis, ref->index);
    for (uint32_t j = 0; j < 2 * k; ++j) samples_out[j] = rsm_sample{ref->square, ref->axis ^ 1u, j, ref->index};
    return RSM_OK;
}

int rsm_fraud_proofs_verify_dev(rsm_ctx* ctx, void* d_shares, const void* d_present, const void* d_records,
                                const void* d_roots, uint32_t k, uint32_t share_size, uint32_t count,
                                const rsm_nmt_params* nmt, const rsm_root_ref* refs, uint32_t n, void* d_work,
                                rsm_fraud_verdict* verdicts, void* stream) {
    static const char* const fn = "rsm_fraud_proofs_verify_dev";
    if (!ctx || k == 0) return fail(RSM_EINVAL, "%s: bad arguments", fn);
    if (int rc = validate_chunk_size(share_size)) return rc;
    if (share_size == 0) return fail(RSM_EINVAL, "%s: empty shares", fn);
    DevTree t;
    FraudLayout lay;
    if (!fraud_shape(k, share_size, n, nmt, &t, &lay))
        return fail(RSM_EUNSUPPORTED, "%s: %u proofs of width %u%s not supported", fn, n, 2 * k, nmt ? " (NMT)" : "");
    if (n == 0 || count == 0) return RSM_OK;
    if (!d_shares || !d_present || !d_records || !d_roots || !refs || !d_work || !verdicts)
        return fail(RSM_EINVAL, "%s: bad arguments", fn);
    if ((reinterpret_cast<uintptr_t>(d_shares) | reinterpret_cast<uintptr_t>(d_work)) & 15u)
        return fail(RSM_EINVAL, "%s: d_shares and d_work must be 16-byte aligned", fn);
    if (t.nmt && share_size < t.p.namespace_size) return fail(RSM_ETREE, "data is too short to contain namespace ID");
    const uint32_t W = 2 * k, S = share_size, chunks = lay.chunks;
    if (int rc = check_refs(fn, "ref", refs, n, count, W)) return rc;
    if (int rc = use_device(ctx)) return rc;

    hipStream_t st = pick(ctx, stream);
    // Destroyed last to first: the stream is drained before the lane, with its staging, goes back.
    LaneGuard lane(ctx);
    if (!lane.lane) return lane.rc;
    Drain drain{st, false};
    // staging: the verdict records [n][4] and the list lengths [chunks][2], both written by
    // the kernels through the mapping; then the refs on their way up
    hipError_t e;
    const size_t stage_words = (size_t)n * 4 + (size_t)chunks * 2 + (size_t)n * 3;
    if ((e = lane.lane->host.ensure(stage_words * 4)) != hipSuccess) return hip_fail(e, "hipHostMalloc (fraud proof staging)");
    uint32_t* const host = static_cast<uint32_t*>(lane.lane->host.ptr);
    void* dev = nullptr;
    if ((e = hipHostGetDevicePointer(&dev, host, 0)) != hipSuccess || !dev)
        return hip_fail(e == hipSuccess ? hipErrorInvalidValue : e, "hipHostGetDevicePointer (fraud proof staging)");
    uint32_t* const mapped = static_cast<uint32_t*>(dev);
    const uint32_t* const h_lens = host + (size_t)n * 4;
    uint32_t* const h_refs = host + (size_t)n * 4 + (size_t)chunks * 2;
    drain.armed = true;

    uint8_t* const shares = static_cast<uint8_t*>(d_shares);
    const uint8_t* const present = static_cast<const uint8_t*>(d_present);
    const uint8_t* const committed = static_cast<const uint8_t*>(d_roots);
    uint8_t* const work = static_cast<uint8_t*>(d_work);
    auto words = [&](uint64_t at) { return reinterpret_cast<uint32_t*>(work + at); };
    RootRef* const d_refs = reinterpret_cast<RootRef*>(work + lay.refs);
    ProofSample* const samples = reinterpret_cast<ProofSample*>(work + lay.samples);
    uint32_t *const have = words(lay.have), *const slot = words(lay.slot), *const tree = words(lay.tree);
    uint32_t *const dec = words(lay.dec), *const chk = words(lay.chk), *const parity = words(lay.parity);
    uint32_t *const status = words(lay.status), *const leaf = words(lay.leaf);
    uint8_t* const scratch = work + lay.scratch;

    // the plan and the share proofs of every slot (an absent slot's word is never consulted)
    memcpy(h_refs, refs, (size_t)n * sizeof(rsm_root_ref));
    if ((e = hipMemcpyAsync(d_refs, h_refs, (size_t)n * sizeof(RootRef), hipMemcpyHostToDevice, st)) != hipSuccess)
        return hip_fail(e, "H2D fraud proof refs");
    if ((e = launch_fraud_plan(present, d_refs, W, n, have, samples, dec, chk, slot, mapped + (size_t)n * 4, st)) != hipSuccess)
        return hip_fail(e, "fraud proof plan kernel launch");
    e = t.nmt ? launch_nmt_proof_verify(shares, static_cast<const uint8_t*>(d_records), committed, W, S, t.p.namespace_size,
                                        t.p.square_size, t.p.ignore_max_namespace, samples, n * W, status, st)
              : launch_proof_verify(shares, static_cast<const uint8_t*>(d_records), committed, W, S, samples, n * W, status,
                                    st);
    if (e != hipSuccess) return hip_fail(e, "fraud proof share verification kernel launch");
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "fraud proof stream");
    for (uint32_t c = 0; c < chunks; ++c)
        if (h_lens[2 * c] > W || h_lens[2 * c + 1] > W || h_lens[2 * c] > h_lens[2 * c + 1])
            return fail(RSM_EDEVICE, "%s: the planner listed %u and %u vectors of %u", fn, h_lens[2 * c], h_lens[2 * c + 1], W);

    // the missing slots of the vectors with k <= present < 2k, a chunk per launch
    const uint64_t chunk_bytes = (uint64_t)W * W * S;
    for (uint32_t c = 0; c < chunks; ++c)
        if (const uint32_t nd = h_lens[2 * c])
            if (int rc = launch_decode(ctx, decode_vectors(shares + c * chunk_bytes, k, S, 0, dec + (size_t)c * W, nd,
                                                           present + (size_t)c * W * W), st))
                return rc;
    // every vector with present >= k: tree and root, then the parity of a re-encode
    if ((e = launch_fraud_trees(shares, have, d_refs, W, S, n, t.nmt ? t.p.namespace_size : 0u, t.p.square_size,
                                t.p.ignore_max_namespace, committed, leaf, tree, st)) != hipSuccess)
        return hip_fail(e, "fraud proof tree kernel launch");
    for (uint32_t c = 0; c < chunks; ++c)
        if (const uint32_t nc = h_lens[2 * c + 1]) {
            uint8_t* const base = shares + c * chunk_bytes;
            const uint32_t* const idx = chk + (size_t)c * W;
            if (int rc = launch_encode(ctx, indexed_vectors(base, k, S, 0, idx, nc, scratch), st)) return rc;
            if ((e = launch_compare_parity(base, scratch, k, S, 0, idx, nc, parity + (size_t)c * W, st)) != hipSuccess)
                return hip_fail(e, "fraud proof parity compare kernel launch");
        }
    if ((e = launch_fraud_verdicts(present, have, status, tree, slot, parity, W, n, mapped, st)) != hipSuccess)
        return hip_fail(e, "fraud proof verdict kernel launch");
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "fraud proof stream");
    drain.armed = false;
    memcpy(verdicts, host, (size_t)n * sizeof(rsm_fraud_verdict));
    return RSM_OK;
}

}  // extern "C"
