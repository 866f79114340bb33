// ns_proof_host.cpp -- stand-alone driver of merkle.cpp's namespace proofs
// (rsm_nmt_namespace_prove / rsm_nmt_namespace_verify) for a sanitizer build
// (tests/test_ns_proofs_san_cpu.py).  Every buffer is a heap allocation of exactly the
// documented size, so a read or write past a record, a root or the presented shares is
// an AddressSanitizer report.  Honest proofs must verify; headers altered to every
// boundary value must give a status word and touch nothing else; an inclusion record
// cut off right after its derived nodes must still verify (the verifier reads nothing
// past them).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/rsmt2d_hip.h"

namespace {

int failures = 0;
#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);    \
            ++failures;                                                \
        }                                                              \
    } while (0)

uint32_t rd(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
void wr(uint8_t* p, uint32_t v) {
    for (int b = 0; b < 4; ++b) p[b] = (uint8_t)(v >> (8 * b));
}

std::unique_ptr<uint8_t[]> heap(const uint8_t* src, size_t n) {  // exactly n bytes (n == 0: one, never read)
    std::unique_ptr<uint8_t[]> p(new uint8_t[n ? n : 1]);
    if (n) memcpy(p.get(), src, n);
    return p;
}

void run(uint32_t n, uint32_t nsz, bool ig) {
    const uint32_t S = 64, k = (n + 1) / 2, NB = 2 * nsz + 32;
    const rsm_nmt_params p{nsz, ig ? 1u : 0u, k};
    const uint32_t RB = rsm_ns_record_bytes(n, &p);
    uint32_t L = 0;
    while ((1u << L) < n) ++L;
    CHECK(RB == 16 + (2 * L + 1) * NB);
    // quadrant-0 leaves with namespaces 00..02, 00..02, 00..04, 00..04, ..: sorted, in runs of two
    std::vector<std::vector<uint8_t>> store(n, std::vector<uint8_t>(S));
    std::vector<const uint8_t*> leaves(n);
    for (uint32_t i = 0; i < n; ++i) {
        for (uint32_t b = 0; b < S; ++b) store[i][b] = (uint8_t)(31 * i + 7 * b + 1);
        memset(store[i].data(), 0, nsz);
        store[i][nsz - 1] = (uint8_t)(2 + 2 * (i / 2));
        leaves[i] = store[i].data();
    }
    for (uint32_t v = 0; v <= 2 * (n / 2) + 5; ++v) {
        std::vector<uint8_t> nid(nsz, 0);
        nid[nsz - 1] = (uint8_t)v;
        if (v == 2 * (n / 2) + 5) memset(nid.data(), 0xFF, nsz);
        auto rec = std::make_unique<uint8_t[]>(RB);
        auto root = std::make_unique<uint8_t[]>(NB);
        CHECK(rsm_nmt_namespace_prove(&p, 0, leaves.data(), n, S, nid.data(), rec.get(), root.get()) == RSM_OK);
        const uint32_t kind = rd(rec.get()), start = rd(rec.get() + 4), end = rd(rec.get() + 8), nn = rd(rec.get() + 12);
        CHECK(kind <= RSM_NS_ABSENCE && nn <= 2 * L);
        const uint32_t cnt = kind == RSM_NS_INCLUSION ? end - start : 0;
        std::vector<uint8_t> packed((size_t)cnt * S);
        for (uint32_t i = 0; i < cnt; ++i) memcpy(&packed[(size_t)i * S], leaves[start + i], S);
        auto shares = heap(packed.data(), packed.size());
        uint32_t st = 99;
        CHECK(rsm_nmt_namespace_verify(&p, 0, nid.data(), shares.get(), cnt, S, n, rec.get(), root.get(), &st) == RSM_OK);
        CHECK(st == RSM_PROOF_OK);
        if (kind == RSM_NS_INCLUSION) {  // nothing past the derived nodes is read
            auto cut = heap(rec.get(), 16 + (size_t)nn * NB);
            st = 99;
            CHECK(rsm_nmt_namespace_verify(&p, 0, nid.data(), shares.get(), cnt, S, n, cut.get(), root.get(), &st) == RSM_OK);
            CHECK(st == RSM_PROOF_OK);
        }
        // every header field at its boundary values, with as many shares as were presented
        const uint32_t kinds[] = {0, 1, 2, 3, 4, 0xFFFFFFFFu};
        const uint32_t pos[] = {0, 1, start, start + 1, end, end - 1, n - 1, n, n + 1, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
        const uint32_t cnts[] = {0, nn, nn + 1, 2 * L, 2 * L + 1, 0xFFFFFFFFu};
        for (uint32_t kd : kinds)
            for (uint32_t s2 : pos)
                for (uint32_t e2 : pos)
                    for (uint32_t c2 : cnts) {
                        auto r2 = heap(rec.get(), RB);
                        wr(r2.get(), kd), wr(r2.get() + 4, s2), wr(r2.get() + 8, e2), wr(r2.get() + 12, c2);
                        st = 99;
                        CHECK(rsm_nmt_namespace_verify(&p, 0, nid.data(), shares.get(), cnt, S, n, r2.get(), root.get(),
                                                       &st) == RSM_OK);
                        CHECK(st <= RSM_PROOF_INCOMPLETE && st != RSM_PROOF_OCCUPIED);
                        if (kd == kind && s2 == start && e2 == end && c2 == nn) CHECK(st == RSM_PROOF_OK);
                        if (kd > RSM_NS_ABSENCE) CHECK(st == RSM_PROOF_MALFORMED);
                    }
    }
}

}  // namespace

int main() {
    for (uint32_t n : {1u, 2u, 3u, 5u, 6u, 7u, 12u, 16u, 33u})
        for (uint32_t nsz : {1u, 8u, 29u})
            for (bool ig : {false, true}) run(n, nsz, ig);
    if (failures) return 1;
    puts("ns_proof_host: ok");
    return 0;
}
