// abi_check.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_abi_cpu.py): every single-GPU
// entry point of the C ABI that builds a CodewordSet or a DecodeSet, on the CPU.  The
// product's host code (rsm_runtime.cpp, eds.cpp) runs against the stubbed HIP runtime
// whose launches compute with the C oracle (hip_stub.cpp built with RSM_STUB_ORACLE),
// so a descriptor that names the wrong bytes gives the wrong bytes: every result is
// compared with the oracle's own extension, encode and decode
// (oracle/leopard_oracle.c).  The stub declines the bit-sliced, queue and fused
// launches, so the paths here are the latency form's two launches and the two
// passes; the test also runs this program under AddressSanitizer and UBSan.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "../../include/rsmt2d_hip.h"

extern "C" int leo_extend_square(unsigned k, size_t S, const uint8_t* ods, uint8_t* eds, int nthreads);
extern "C" int leo_encode(unsigned k, size_t S, const uint8_t* const* data, uint8_t* const* parity);
extern "C" int leo_decode(unsigned k, size_t S, uint8_t* const* shards, const uint8_t* present);

namespace {
int g_fail = 0;
#define CHECK(c, ...)                                            \
    do {                                                         \
        if (!(c)) {                                              \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                        \
            fprintf(stderr, " [%s]\n", rsm_last_error());        \
            ++g_fail;                                            \
        }                                                        \
    } while (0)

using Bytes = std::vector<uint8_t>;
constexpr uint32_t S = 64;
constexpr uint8_t kJunk = 0xA5;

Bytes random_bytes(size_t n, uint64_t seed) {
    Bytes v(n);
    for (auto& b : v) {
        seed += 0x9E3779B97F4A7C15ull;
        uint64_t z = seed;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        b = (uint8_t)(z ^ (z >> 31));
    }
    return v;
}

Bytes oracle_eds(uint32_t k, const uint8_t* ods) {
    Bytes eds((size_t)4 * k * k * S);
    CHECK(leo_extend_square(k, S, ods, eds.data(), 1) == 0, "oracle k=%u", k);
    return eds;
}

// `count` squares of junk whose Q0 quadrants hold the ODSs
Bytes seeded(uint32_t k, uint32_t count, const Bytes& ods) {
    const size_t W = 2ull * k, row = W * S, half = (size_t)k * S;
    Bytes e(count * W * row, kJunk);
    for (size_t r = 0; r < (size_t)count * k; ++r) memcpy(&e[(r / k) * W * row + (r % k) * row], &ods[r * half], half);
    return e;
}

// a device buffer holding `init`; back() downloads it
struct Dev {
    rsm_ctx* ctx;
    void* p = nullptr;
    size_t n;
    Dev(rsm_ctx* c, const Bytes& init) : ctx(c), n(init.size()) {
        CHECK(rsm_dev_alloc(ctx, n, &p) == RSM_OK && p, "rsm_dev_alloc");
        CHECK(rsm_memcpy(ctx, p, init.data(), n, 0) == RSM_OK, "upload");
    }
    ~Dev() { CHECK(rsm_dev_free(ctx, p) == RSM_OK, "rsm_dev_free"); }
    Bytes back() const {
        Bytes v(n);
        CHECK(rsm_sync(ctx) == RSM_OK, "rsm_sync");
        CHECK(rsm_memcpy(ctx, v.data(), p, n, 1) == RSM_OK, "download");
        return v;
    }
};

// `run` extends `count` device squares in place: all of them equal the oracle's
void check_extend(rsm_ctx* ctx, const char* what, uint32_t k, uint32_t count, const std::function<int(void*)>& run) {
    const size_t ods_b = (size_t)k * k * S;
    const Bytes ods = random_bytes(count * ods_b, 1000 + k * 7 + count);
    Bytes want;
    for (uint32_t i = 0; i < count; ++i) {
        const Bytes e = oracle_eds(k, &ods[i * ods_b]);
        want.insert(want.end(), e.begin(), e.end());
    }
    Dev d(ctx, seeded(k, count, ods));
    const int rc = run(d.p);
    CHECK(rc == RSM_OK, "%s: rc=%d", what, rc);
    CHECK(d.back() == want, "%s: k=%u, %u squares differ from the oracle", what, k, count);
}

void check_extensions(rsm_ctx* ctx) {
    auto whole = [&](uint32_t k, uint32_t count) {
        return [=](void* d) { return rsm_extend_squares_dev(ctx, d, k, S, count, nullptr); };
    };
    check_extend(ctx, "two passes (queue plan declined)", 4, 3, whole(4, 3));
    check_extend(ctx, "latency form, batch", 16, 2, whole(16, 2));
    check_extend(ctx, "latency form, one k = 128 square", 128, 1, whole(128, 1));
    int prev = -1;
    CHECK(rsm_ctx_set_split_max(ctx, 0, &prev) == RSM_OK, "rsm_ctx_set_split_max");
    check_extend(ctx, "k = 128 without the latency form", 128, 1, whole(128, 1));
    CHECK(rsm_ctx_set_split_max(ctx, prev, nullptr) == RSM_OK, "rsm_ctx_set_split_max (restore)");
    check_extend(ctx, "GF(2^16) single pass", 130, 1, whole(130, 1));
    // rows span 5 * 64 + 64 bytes, columns more: both passes over the limit
    CHECK(rsm_ctx_set_limits(ctx, 256, 0) == RSM_OK, "rsm_ctx_set_limits");
    check_extend(ctx, "wide forms", 4, 3, whole(4, 3));
    CHECK(rsm_ctx_set_limits(ctx, 0, 0) == RSM_OK, "rsm_ctx_set_limits (restore)");
    check_extend(ctx, "phase 1 then phase 2", 8, 2, [&](void* d) {
        if (int rc = rsm_extend_squares_phase_dev(ctx, d, 8, S, 2, 1, nullptr)) return rc;
        return rsm_extend_squares_phase_dev(ctx, d, 8, S, 2, 2, nullptr);
    });
    check_extend(ctx, "phase 3", 8, 2, [&](void* d) { return rsm_extend_squares_phase_dev(ctx, d, 8, S, 2, 3, nullptr); });
    check_extend(ctx, "row and column ranges", 8, 1, [&](void* d) {
        if (int rc = rsm_extend_rows_dev(ctx, d, 8, S, 3, 5, nullptr)) return rc;
        if (int rc = rsm_extend_rows_dev(ctx, d, 8, S, 0, 3, nullptr)) return rc;
        if (int rc = rsm_extend_cols_dev(ctx, d, 8, S, 5, 11, nullptr)) return rc;
        return rsm_extend_cols_dev(ctx, d, 8, S, 0, 5, nullptr);
    });
    // host memory in and out
    for (uint32_t count : {1u, 2u}) {
        const uint32_t k = 8;
        const size_t ods_b = (size_t)k * k * S, eds_b = 4 * ods_b;
        const Bytes ods = random_bytes(count * ods_b, 31 + count);
        Bytes got(count * eds_b, kJunk), want;
        for (uint32_t i = 0; i < count; ++i) {
            const Bytes e = oracle_eds(k, &ods[i * ods_b]);
            want.insert(want.end(), e.begin(), e.end());
        }
        const int rc = count == 1 ? rsm_extend_square(ctx, ods.data(), k, S, got.data())
                                  : rsm_extend_squares_host(ctx, ods.data(), k, S, count, got.data());
        CHECK(rc == RSM_OK && got == want, "host extension of %u squares: rc=%d", count, rc);
    }
}

// Rows [row0, row0 + nrows) of one square extended with their cells also packed into
// nblocks column blocks: block h holds the rows' columns [h cb, (h + 1) cb), row pitch cb S.
void check_rows_blocks(rsm_ctx* ctx, uint32_t k, uint32_t row0, uint32_t nrows, uint32_t nblocks) {
    const size_t W = 2ull * k, row = W * S, half = (size_t)k * S, cb = W / nblocks;
    const Bytes ods = random_bytes((size_t)k * k * S, 500 + k);
    Bytes want = seeded(k, 1, ods);
    std::vector<const uint8_t*> dp(k);
    std::vector<uint8_t*> pp(k);
    for (uint32_t r = row0; r < row0 + nrows; ++r) {
        for (uint32_t e = 0; e < k; ++e) dp[e] = &want[r * row + e * S], pp[e] = &want[r * row + half + e * S];
        CHECK(leo_encode(k, S, dp.data(), pp.data()) == 0, "oracle encode");
    }
    Bytes want_blocks(nrows * row);
    for (size_t h = 0; h < nblocks; ++h)
        for (size_t q = 0; q < nrows; ++q)
            memcpy(&want_blocks[(h * nrows + q) * cb * S], &want[(row0 + q) * row + h * cb * S], cb * S);
    Dev d(ctx, seeded(k, 1, ods)), blocks(ctx, Bytes(nrows * row, kJunk));
    const int rc = rsm_extend_rows_blocks_dev(ctx, d.p, k, S, row0, nrows, blocks.p, nblocks, nullptr);
    CHECK(rc == RSM_OK, "rsm_extend_rows_blocks_dev k=%u: rc=%d", k, rc);
    CHECK(d.back() == want, "rsm_extend_rows_blocks_dev k=%u: rows differ", k);
    CHECK(blocks.back() == want_blocks, "rsm_extend_rows_blocks_dev k=%u: blocks differ", k);
}

// the C ABI's generic batch: strides larger than the packed ones, parity to its own buffer
void check_encode_batch(rsm_ctx* ctx) {
    const uint32_t k = 6, count = 5;
    const size_t es = 2 * S, cws = k * es + 192;
    const Bytes in = random_bytes(count * cws, 77);
    Bytes want(count * cws, kJunk);
    std::vector<const uint8_t*> dp(k);
    std::vector<uint8_t*> pp(k);
    for (uint32_t q = 0; q < count; ++q) {
        for (uint32_t e = 0; e < k; ++e) dp[e] = &in[q * cws + e * es], pp[e] = &want[q * cws + e * es];
        CHECK(leo_encode(k, S, dp.data(), pp.data()) == 0, "oracle encode");
    }
    Dev din(ctx, in), dout(ctx, Bytes(count * cws, kJunk));
    const int rc = rsm_encode_batch_dev(ctx, din.p, dout.p, k, S, count, cws, es, nullptr);
    CHECK(rc == RSM_OK, "rsm_encode_batch_dev: rc=%d", rc);
    CHECK(dout.back() == want, "rsm_encode_batch_dev: parity (or the bytes between it) differs");
    CHECK(din.back() == in, "rsm_encode_batch_dev: input changed");
}

void check_codec(rsm_ctx* ctx, uint32_t k) {
    const Bytes data = random_bytes((size_t)k * S, 900 + k);
    Bytes cw(2ull * k * S), got((size_t)k * S, kJunk);
    memcpy(cw.data(), data.data(), data.size());
    std::vector<const uint8_t*> dp(k);
    std::vector<uint8_t*> pp(k), gp(k), sh(2 * k);
    for (uint32_t i = 0; i < k; ++i) dp[i] = &data[i * S], pp[i] = &cw[(k + i) * S], gp[i] = &got[i * S];
    CHECK(leo_encode(k, S, dp.data(), pp.data()) == 0, "oracle encode");
    int rc = rsm_encode(ctx, dp.data(), k, S, gp.data());
    CHECK(rc == RSM_OK && memcmp(got.data(), &cw[(size_t)k * S], got.size()) == 0, "rsm_encode k=%u: rc=%d", k, rc);
    // every second data share absent
    Bytes holed = cw, oracle = cw;
    std::vector<uint8_t> pres(2 * k, 1);
    for (uint32_t i = 0; i < k; i += 2) {
        pres[i] = 0;
        memset(&holed[i * S], 0xEE, S);
        memset(&oracle[i * S], 0xEE, S);
    }
    for (uint32_t i = 0; i < 2 * k; ++i) sh[i] = &oracle[i * S];
    CHECK(leo_decode(k, S, sh.data(), pres.data()) == 0 && oracle == cw, "oracle decode k=%u", k);
    for (uint32_t i = 0; i < 2 * k; ++i) sh[i] = &holed[i * S];
    rc = rsm_decode(ctx, sh.data(), pres.data(), 2 * k, S);
    CHECK(rc == RSM_OK && holed == cw, "rsm_decode k=%u: rc=%d", k, rc);
}

// rsm_decode_vectors_dev: three vectors of an axis, each with k cells erased
void check_decode_vectors(rsm_ctx* ctx, int axis) {
    const uint32_t k = 8, W = 2 * k;
    const Bytes ods = random_bytes((size_t)k * k * S, 60 + axis);
    const Bytes want = oracle_eds(k, ods.data());
    Bytes holed = want, pres((size_t)W * W, 1);
    const uint32_t vecs[3] = {1, 9, 14};
    for (uint32_t v : vecs)
        for (uint32_t j = 0; j < k; ++j) {
            const uint32_t p = (2 * j + v) % W;  // k positions of the 2k, across both halves
            const size_t cell = axis == RSM_AXIS_ROW ? (size_t)v * W + p : (size_t)p * W + v;
            pres[cell] = 0;
            memset(&holed[cell * S], 0xEE, S);
        }
    Bytes idx(sizeof(vecs));
    memcpy(idx.data(), vecs, sizeof(vecs));
    Dev d(ctx, holed), dp(ctx, pres), di(ctx, idx);
    const int rc = rsm_decode_vectors_dev(ctx, d.p, static_cast<const uint8_t*>(dp.p), k, S, axis,
                                          static_cast<const uint32_t*>(di.p), 3, nullptr);
    CHECK(rc == RSM_OK, "rsm_decode_vectors_dev axis %d: rc=%d", axis, rc);
    CHECK(d.back() == want, "rsm_decode_vectors_dev axis %d: square differs", axis);
}

// the DefaultTree behind another address: not a tree the device computes, so the host trees run
int wrapped_default_tree(void* user, int axis, uint32_t index, const uint8_t* const* leaves, uint32_t n_leaves,
                         uint32_t leaf_size, uint8_t* root_out, uint32_t* root_len) {
    return rsm_default_tree_root(user, axis, index, leaves, n_leaves, leaf_size, root_out, root_len);
}

// Import a k = 4 square without the cells `nil` names and Repair it against the roots
// of the complete square: the original square comes back.  With `bad`: that cell of the
// complete square is corrupted before the roots are taken, so the roots agree with it
// and only the re-encoding of its complete vector (verifyEncoding) can tell: Repair must
// name that vector, (bad_axis, bad_index), as byzantine.
struct Cell {
    uint32_t r, c;
};
void check_repair(rsm_ctx* ctx, const char* what, rsm_tree_root_fn tree, const std::function<bool(uint32_t, uint32_t)>& nil,
                  const Cell* bad = nullptr, int bad_axis = -1, uint32_t bad_index = 0) {
    const uint32_t k = 4, W = 2 * k;
    const Bytes ods = random_bytes((size_t)k * k * S, 4040);
    std::vector<const uint8_t*> ptr(k * k), cells(W * W);
    std::vector<uint32_t> len(W * W, S);
    for (uint32_t i = 0; i < k * k; ++i) ptr[i] = &ods[i * S];
    rsm_eds* full = nullptr;
    CHECK(rsm_eds_compute(ctx, ptr.data(), len.data(), k * k, &full) == RSM_OK && full, "%s: rsm_eds_compute", what);
    if (!full) return;
    Bytes flat((size_t)W * W * S), rr(W * 32), cr(W * 32);
    CHECK(rsm_eds_flattened(full, flat.data(), nullptr) == RSM_OK, "%s: flattened", what);
    CHECK(flat == oracle_eds(k, ods.data()), "%s: rsm_eds_compute differs from the oracle", what);
    rsm_eds_free(full);
    if (bad) flat[((size_t)bad->r * W + bad->c) * S + 7] ^= 0x40;
    // the roots of the (possibly corrupted) complete square, by the host trees
    for (uint32_t i = 0; i < W * W; ++i) cells[i] = &flat[(size_t)i * S];
    rsm_eds* whole = nullptr;
    uint32_t rl = 0;
    CHECK(rsm_eds_import(ctx, cells.data(), len.data(), W * W, &whole) == RSM_OK && whole, "%s: rsm_eds_import (whole)", what);
    if (!whole) return;
    CHECK(rsm_eds_roots(whole, RSM_AXIS_ROW, wrapped_default_tree, nullptr, rr.data(), 32, &rl) == RSM_OK && rl == 32 &&
              rsm_eds_roots(whole, RSM_AXIS_COL, wrapped_default_tree, nullptr, cr.data(), 32, &rl) == RSM_OK && rl == 32,
          "%s: rsm_eds_roots", what);
    rsm_eds_free(whole);
    uint32_t nils = 0;
    for (uint32_t i = 0; i < W * W; ++i)
        if (nil(i / W, i % W)) cells[i] = nullptr, ++nils;
    rsm_eds* e = nullptr;
    CHECK(rsm_eds_import(ctx, cells.data(), len.data(), W * W, &e) == RSM_OK && e, "%s: rsm_eds_import", what);
    if (!e) return;
    rsm_byzantine byz;
    const int rc = rsm_eds_repair(e, rr.data(), cr.data(), 32, tree, nullptr, &byz);
    if (bad) {
        CHECK(rc == RSM_EBYZANTINE && byz.axis == bad_axis && byz.index == bad_index,
              "%s: rc=%d, byzantine axis %d index %u, expected axis %d index %u", what, rc, byz.axis, byz.index, bad_axis,
              bad_index);
        rsm_eds_free(e);
        return;
    }
    CHECK(rc == RSM_OK, "%s: rsm_eds_repair of %u nil cells: rc=%d", what, nils, rc);
    Bytes got((size_t)W * W * S), pres(W * W);
    CHECK(rsm_eds_flattened(e, got.data(), pres.data()) == RSM_OK, "%s: flattened", what);
    CHECK(got == flat && pres == Bytes(W * W, 1), "%s: the repaired square differs", what);
    rsm_repair_stats st{};
    CHECK(rsm_eds_repair_stats(e, &st) == RSM_OK && st.sweeps >= 1 && st.decoded_vectors >= 1, "%s: no device sweep", what);
    // the device decode and verification accepted the square (no exact sequential solver)
    CHECK(st.fast_path == 1, "%s: fast_path %d, fallback reason %u", what, st.fast_path, st.fallback_reason);
    rsm_eds_free(e);
}

// Repair through eds.cpp's decode() and verify_encoding().  No nil pattern is symmetric
// in (row, column): the vectors one axis can decode have too few cells on the other
// axis, and the complete rows and complete columns are different index lists, so a
// descriptor built for the wrong axis fails the decode launch or flags a good vector.
void check_repairs(rsm_ctx* ctx) {
    // a third of the cells nil (21 of 64): columns 0-2 of rows 1-7.  The sanity check
    // re-encodes row 0 and columns 3-7, one ROW sweep decodes rows 1-7 (columns 0-2 hold
    // one cell each).  A caller's tree: host roots.
    auto left = [](uint32_t r, uint32_t c) { return r > 0 && c < 3; };
    check_repair(ctx, "Repair by rows, caller's tree", wrapped_default_tree, left);
    // the transpose: rows 0-2 of columns 1-7 nil, one COLUMN sweep; rows 3-7 and column 0 re-encoded
    auto top = [](uint32_t r, uint32_t c) { return c > 0 && r < 3; };
    check_repair(ctx, "Repair by columns, caller's tree", wrapped_default_tree, top);
    // half of each row nil (columns 0-3), the DefaultTree: one row sweep, roots on the "device"
    check_repair(ctx, "Repair, DefaultTree", nullptr, [](uint32_t, uint32_t c) { return c < 4; });
    // a parity cell of the one complete row / column corrupted under matching roots
    const Cell in_row0{0, 5}, in_col0{5, 0};
    check_repair(ctx, "Repair, byzantine row", wrapped_default_tree, left, &in_row0, RSM_AXIS_ROW, 0);
    check_repair(ctx, "Repair, byzantine column", nullptr, top, &in_col0, RSM_AXIS_COL, 0);
}
}  // namespace

int main() {
    rsm_ctx* ctx = nullptr;
    CHECK(rsm_ctx_create(0, &ctx) == RSM_OK && ctx, "rsm_ctx_create");
    if (!ctx) return 1;
    check_extensions(ctx);
    check_rows_blocks(ctx, 8, 2, 6, 2);       // GF(2^8): the row pass, then block copies
    check_rows_blocks(ctx, 256, 64, 64, 8);   // GF(2^16), 64-column blocks: the encoder's side output
    check_encode_batch(ctx);
    // the copy branch; the zero-copy branch of GF(2^8) (Encode calls the latency form's
    // launcher itself) and of GF(2^16)
    for (uint32_t k : {4u, 100u, 200u}) check_codec(ctx, k);
    for (int axis : {RSM_AXIS_ROW, RSM_AXIS_COL}) check_decode_vectors(ctx, axis);
    check_repairs(ctx);
    rsm_ctx_destroy(ctx);
    if (g_fail) {
        fprintf(stderr, "abi_check: %d failures\n", g_fail);
        return 1;
    }
    printf("abi_check: ok\n");
    return 0;
}
