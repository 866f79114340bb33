// kernels_nsproof.hip -- namespace proofs out of an NMT node store (DESIGN.md §4
// "Namespace proofs"; the store is built by nmt_nodes_kernel, kernels_nmt.hip; layout
// and record: rsm_kernels.hpp "namespace proofs").
//
// "Every share of namespace nid in this row, with proof that these are all of them" is
// nmt's ProveNamespace: the leaves of a tree whose status word is 0 are sorted by
// namespace, so the answer is the range [start, end) of two binary searches and its
// range proof, whose nodes all sit in the store.  Nothing is hashed.
//
//   ns_locate_kernel : one lane per query: status word, top node, the two searches
//                      (each bounded by L + 1 probes whatever the leaf records hold);
//                      writes the record header and the share count
//   ns_scan_kernel   : one workgroup turns the n counts into offsets[n + 1]
//   ns_gather_kernel : one lane per (query, slot) of the 2L + 1 node slots
//   ns_shares_kernel : one wave per query copies its shares, 16 bytes per lane
// Range proofs (rsm_kernels.hpp "range proofs": the caller names [start, end) itself, of
// either tree's store) put range_header_kernel in ns_locate_kernel's place and share the
// other three: scan, gather and shares take a query as `qwords` words whose first three
// are square, axis, index (NsQuery: 11, RangeQuery: 5).
// Queries are validated on the host: no kernel sees a coordinate out of range.  start
// and end are at most W by construction, so every node and share address is in range
// whatever the store's namespaces are.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "proof_node.hpp"
#include "rsm_kernels.hpp"

namespace rsm {

namespace {

typedef uint32_t nq4u __attribute__((ext_vector_type(4)));

constexpr uint32_t kHeader = 16;

// a (eight words in the store, 16-byte aligned) < b, as big-endian byte strings
__device__ __forceinline__ int ns_cmp(const uint32_t* a, const uint32_t (&b)[8]) {
    const nq4u lo = reinterpret_cast<const nq4u*>(a)[0], hi = reinterpret_cast<const nq4u*>(a)[1];
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    int c = 0;
#pragma unroll
    for (int i = 7; i >= 0; --i) c = w[i] < b[i] ? -1 : (w[i] > b[i] ? 1 : c);
    return c;
}

__device__ __forceinline__ void put_u32(uint8_t* p, uint32_t v) {
    for (int b = 0; b < 4; ++b) p[b] = (uint8_t)(v >> (8 * b));
}
__device__ __forceinline__ uint32_t get_u32(const uint8_t* p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

__host__ __device__ constexpr uint32_t record_bytes(uint32_t W, uint32_t ns) {
    return kHeader + (2 * proof_levels(W) + 1) * (2 * ns + 32);
}

__global__ __launch_bounds__(256) void ns_locate_kernel(const uint32_t* __restrict__ store,
                                                        const uint32_t* __restrict__ status, uint32_t W,
                                                        uint32_t squares, uint32_t ns,
                                                        const NsQuery* __restrict__ queries, uint32_t n,
                                                        uint8_t* __restrict__ records, uint32_t* __restrict__ counts) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= n) return;
    const uint32_t L = proof_levels(W);
    const NsQuery qu = queries[q];
    const uint64_t tree = (uint64_t)qu.square * 2 * W + (uint64_t)qu.axis * W + qu.index;
    // leaf p of the vector: record leaf0 + p * stride
    const uint32_t* leaf0 = store + ((uint64_t)qu.square * W * W + (qu.axis == 0 ? (uint64_t)qu.index * W : qu.index)) *
                                        kProofNmtLeafWords;
    const uint64_t stride = (uint64_t)(qu.axis == 0 ? 1u : W) * kProofNmtLeafWords;
    uint32_t kind, start = 0, end = 0, n_nodes = 0, cnt = 0;
    if (status[tree] != 0) {
        kind = kNsTree;  // push order: the vector is not sorted, nothing is searched
    } else {
        // the stored top node (ignore_max already applied); a one-leaf tree's is its leaf
        const uint32_t* top = store + (uint64_t)squares * W * W * kProofNmtLeafWords +
                              (tree * proof_tree_nodes(W) + proof_level_offset(W, L)) * kProofNmtNodeWords;
        const uint32_t* rmin = L ? top : leaf0;
        const uint32_t* rmax = L ? top + 8 : leaf0;
        if (ns_cmp(rmin, qu.nid) > 0 || ns_cmp(rmax, qu.nid) < 0) {
            kind = kNsEmpty;
        } else {
            uint32_t lo = 0, hi = W;  // first leaf >= nid
            for (uint32_t i = 0; i <= L && lo < hi; ++i) {
                const uint32_t mid = (lo + hi) >> 1;
                if (ns_cmp(leaf0 + mid * stride, qu.nid) < 0) lo = mid + 1;
                else hi = mid;
            }
            start = lo;
            hi = W;  // first leaf > nid
            for (uint32_t i = 0; i <= L && lo < hi; ++i) {
                const uint32_t mid = (lo + hi) >> 1;
                if (ns_cmp(leaf0 + mid * stride, qu.nid) <= 0) lo = mid + 1;
                else hi = mid;
            }
            end = lo;
            if (start >= W) {  // not on a sorted vector (the root's range covers nid)
                kind = kNsEmpty;
                start = end = 0;
            } else {
                if (start < end) {
                    kind = kNsInclusion;
                    cnt = end - start;
                } else {
                    kind = kNsAbsence;  // the first leaf above nid
                    end = start + 1;
                }
                uint32_t nl;
                n_nodes = ns_range_nodes(W, start, end, &nl);
            }
        }
    }
    uint8_t* rec = records + (uint64_t)q * record_bytes(W, ns);
    put_u32(rec, kind);
    put_u32(rec + 4, start);
    put_u32(rec + 8, end);
    put_u32(rec + 12, n_nodes);
    counts[q] = cnt;
}

// A range query's header, kind kNsInclusion over the caller's [start, end) (validated on
// the host: start < end <= W), and its share count; nothing of the store is read.
__global__ __launch_bounds__(256) void range_header_kernel(uint32_t W, uint32_t ns, const RangeQuery* __restrict__ queries,
                                                           uint32_t n, uint8_t* __restrict__ records,
                                                           uint32_t* __restrict__ counts) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= n) return;
    const RangeQuery qu = queries[q];
    uint32_t nl;
    uint8_t* rec = records + (uint64_t)q * record_bytes(W, ns);
    put_u32(rec, kNsInclusion);
    put_u32(rec + 4, qu.start);
    put_u32(rec + 8, qu.end);
    put_u32(rec + 12, ns_range_nodes(W, qu.start, qu.end, &nl));
    counts[q] = qu.end - qu.start;
}

// offs[0 .. n) hold counts; on return offs[i] = the sum of the counts before i, offs[n]
// the total (below 2^32: n <= 2^20 queries of at most W <= 2048 shares).
__global__ __launch_bounds__(1024) void ns_scan_kernel(uint32_t* __restrict__ offs, uint32_t n) {
    __shared__ uint32_t wsum[16];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n; base += 1024u) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < n ? offs[i] : 0u;
        uint32_t x = v;  // inclusive scan of the wave
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        if (lane == 63u) wsum[wave] = x;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < 16u; ++w) {
            const uint32_t s = wsum[w];
            if (w < wave) before += s;
            total += s;
        }
        if (i < n) offs[i] = carry + before + x - v;
        carry += total;
        __syncthreads();  // wsum is rewritten by the next chunk
    }
    if (threadIdx.x == 0) offs[n] = carry;
}

__global__ __launch_bounds__(256) void ns_gather_kernel(const uint32_t* __restrict__ store, uint32_t W,
                                                        uint32_t squares, uint32_t ns,
                                                        const uint32_t* __restrict__ queries, uint32_t qwords,
                                                        uint32_t n, uint8_t* records) {
    const uint32_t L = proof_levels(W), slots = 2 * L + 1;
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (uint64_t)n * slots) return;
    const uint32_t q = (uint32_t)(t / slots), s = (uint32_t)(t - (uint64_t)q * slots);
    const uint32_t node_len = 2 * ns + 32;
    uint8_t* rec = records + (uint64_t)q * record_bytes(W, ns);
    const uint32_t kind = get_u32(rec), start = get_u32(rec + 4), end = get_u32(rec + 8);
    uint8_t* out = rec + kHeader + s * node_len;
    // which node this slot holds: the left nodes from the top level down, then the right
    // nodes from the bottom level up; slot 2L the leaf of an absence proof
    bool mine = false;
    uint32_t lvl = 0, j = 0;
    if (kind == kNsInclusion || kind == kNsAbsence) {
        uint32_t nl;
        const uint32_t nn = ns_range_nodes(W, start, end, &nl);
        if (s < nn) {
            uint32_t a = start, last = end - 1, li = 0, ri = 0;
            for (uint32_t l = 0; l < L; ++l) {
                if (a & 1u) {
                    if (s < nl && nl - 1 - li == s) mine = true, lvl = l, j = a - 1;
                    ++li;
                }
                if (!(last & 1u) && last + 1 < proof_level_count(W, l)) {
                    if (s >= nl && s - nl == ri) mine = true, lvl = l, j = last + 1;
                    ++ri;
                }
                a >>= 1;
                last >>= 1;
            }
        } else if (s == 2 * L && kind == kNsAbsence) {
            mine = true, lvl = 0, j = start;
        }
    }
    if (!mine) {
        for (uint32_t i = 0; i < node_len; ++i) out[i] = 0;
        return;
    }
    const uint32_t* qu = queries + (uint64_t)q * qwords;  // square, axis, index
    store_node_bytes(store, W, squares, ns, qu[0], qu[1], qu[2], lvl, j, out);
}

__global__ __launch_bounds__(256) void ns_shares_kernel(const uint8_t* __restrict__ eds, uint32_t W, uint32_t S,
                                                        uint32_t ns, const uint32_t* __restrict__ queries,
                                                        uint32_t qwords, uint32_t n,
                                                        const uint8_t* __restrict__ records,
                                                        const uint32_t* __restrict__ offs, uint8_t* __restrict__ shares,
                                                        uint64_t shares_cap) {
    const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (q >= n) return;
    const uint32_t o0 = offs[q], o1 = offs[q + 1];
    if (o1 == o0 || (uint64_t)o1 > shares_cap) return;  // nothing to copy, or it does not fit
    const uint32_t start = get_u32(records + (uint64_t)q * record_bytes(W, ns) + 4);
    const uint32_t qw = S / 16u, words = (o1 - o0) * qw;  // 16-byte words per share, of the query
    const uint32_t* qu = queries + (uint64_t)q * qwords;
    const uint32_t square = qu[0], axis = qu[1], index = qu[2];
    const uint8_t* sq = eds + (uint64_t)square * W * W * S;
    nq4u* dst = reinterpret_cast<nq4u*>(shares + (uint64_t)o0 * S);
    for (uint32_t w = lane; w < words; w += 64u) {
        const uint32_t p = start + w / qw, c = w % qw;
        const uint64_t cell = axis == 0 ? (uint64_t)index * W + p : (uint64_t)p * W + index;
        dst[w] = reinterpret_cast<const nq4u*>(sq + cell * S)[c];
    }
}

}  // namespace

// scan, gather and shares behind either header kernel
static hipError_t launch_scan_gather(const uint32_t* d_store, const uint8_t* d_eds, uint32_t W, uint32_t S, uint32_t squares,
                                     uint32_t ns, const uint32_t* d_queries, uint32_t qwords, uint32_t n, uint8_t* d_records,
                                     uint32_t* d_offsets, uint8_t* d_shares, uint64_t shares_cap, hipStream_t st) {
    hipLaunchKernelGGL(ns_scan_kernel, dim3(1), dim3(1024), 0, st, d_offsets, n);
    const uint64_t lanes = (uint64_t)n * (2 * proof_levels(W) + 1);
    hipLaunchKernelGGL(ns_gather_kernel, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, st, d_store, W, squares,
                       ns, d_queries, qwords, n, d_records);
    if (d_shares)
        hipLaunchKernelGGL(ns_shares_kernel, dim3((n + 3) / 4), dim3(256), 0, st, d_eds, W, S, ns, d_queries, qwords, n,
                           d_records, d_offsets, d_shares, shares_cap);
    return hipGetLastError();
}

hipError_t launch_ns_proofs(const uint32_t* d_store, const uint32_t* d_status, const uint8_t* d_eds, uint32_t W,
                            uint32_t S, uint32_t squares, uint32_t ns, const NsQuery* d_queries, uint32_t n,
                            uint8_t* d_records, uint32_t* d_offsets, uint8_t* d_shares, uint64_t shares_cap,
                            hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(ns_locate_kernel, dim3((n + 255) / 256), dim3(256), 0, st, d_store, d_status, W, squares, ns,
                       d_queries, n, d_records, d_offsets);
    return launch_scan_gather(d_store, d_eds, W, S, squares, ns, reinterpret_cast<const uint32_t*>(d_queries),
                              sizeof(NsQuery) / 4, n, d_records, d_offsets, d_shares, shares_cap, st);
}

hipError_t launch_range_proofs(const uint32_t* d_store, const uint8_t* d_eds, uint32_t W, uint32_t S, uint32_t squares,
                               uint32_t ns, const RangeQuery* d_queries, uint32_t n, uint8_t* d_records,
                               uint32_t* d_offsets, uint8_t* d_shares, uint64_t shares_cap, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(range_header_kernel, dim3((n + 255) / 256), dim3(256), 0, st, W, ns, d_queries, n, d_records,
                       d_offsets);
    return launch_scan_gather(d_store, d_eds, W, S, squares, ns, reinterpret_cast<const uint32_t*>(d_queries),
                              sizeof(RangeQuery) / 4, n, d_records, d_offsets, d_shares, shares_cap, st);
}

}  // namespace rsm
