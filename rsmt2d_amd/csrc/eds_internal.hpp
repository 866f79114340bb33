// eds_internal.hpp -- the ExtendedDataSquare object, shared by eds.cpp and rsm_proof.cpp, and
// the staging, range checks and scratch carving the device entry points share (rsm_proof.cpp,
// rsm_repair_dev.cpp, rsm_fraud.cpp).
#pragma once
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "rsm_internal.hpp"

namespace rsm {
// Uploads `bytes` of a call's host arguments through the staging buffers of stream `st`
// (rsm_proof.cpp; ss.mu held): *dev is the device copy, valid for kernels enqueued on
// `st` before the next call on it.
int stage_bytes(hipStream_t st, StreamScratch& ss, const void* src, size_t bytes, const void** dev);
// RSM_EINVAL, naming the first one, unless every sample addresses a cell of `count` squares
// of `width` (rsm_proof.cpp).
int check_samples(const char* fn, const rsm_sample* s, uint32_t n, uint32_t count, uint32_t width);
// The same for the (square, axis, index) that rsm_root_ref and rsm_ns_query begin with;
// `noun`: "ref" or "query".
template <class Ref>
int check_refs(const char* fn, const char* noun, const Ref* r, uint32_t n, uint32_t count, uint32_t width) {
    for (uint32_t i = 0; i < n; ++i)
        if (r[i].square >= count || r[i].axis > 1 || r[i].index >= width)
            return fail(RSM_EINVAL, "%s: %s %u (square %u, axis %u, index %u) is out of range", fn, noun, i, r[i].square,
                        r[i].axis, r[i].index);
    return RSM_OK;
}

// Hands out the sections of a d_work: each a multiple of 256 bytes from its start.
struct Carver {
    uint64_t at = 0;
    uint64_t take(uint64_t bytes) {
        const uint64_t o = at;
        at += (bytes + 255) / 256 * 256;
        return o;
    }
};

// An early return must not hand the lane's pinned staging back while the stream still
// reads or writes it.
struct Drain {
    hipStream_t st;
    bool armed;
    ~Drain() {
        if (armed) (void)hipStreamSynchronize(st);
    }
};
}  // namespace rsm

// Host bytes of a square: pinned (hipHostMalloc) whenever a HIP runtime is
// usable, so Repair's square upload and download are direct DMA; plain memory on
// a host without a GPU (Import/New are host-only operations).
struct HostSquare {
    uint8_t* p = nullptr;
    size_t n = 0;
    bool pinned = false;
    HostSquare() = default;
    HostSquare(const HostSquare&) = delete;
    HostSquare& operator=(const HostSquare&) = delete;
    ~HostSquare() { release(); }
    void release() {
        if (p) {
            if (pinned) (void)hipHostFree(p);
            else free(p);
        }
        p = nullptr;
        n = 0;
    }
    bool assign(size_t bytes) {  // zero-filled
        release();
        if (bytes == 0) return true;
        void* q = nullptr;
        if (hipHostMalloc(&q, bytes, hipHostMallocDefault) == hipSuccess) {
            pinned = true;
        } else {
            (void)hipGetLastError();
            q = malloc(bytes);
            pinned = false;
            if (!q) return false;
        }
        p = static_cast<uint8_t*>(q);
        n = bytes;
        memset(p, 0, n);
        return true;
    }
    uint8_t* data() { return p; }
    const uint8_t* data() const { return p; }
    size_t size() const { return n; }
    void swap(HostSquare& o) {
        std::swap(p, o.p);
        std::swap(n, o.n);
        std::swap(pinned, o.pinned);
    }
};

// The node store of a complete square (rsm_eds_proofs' device path): built once for one
// tree, kept until a cell, the context or the tree changes (the reference's resetRoots
// on SetCell is the pattern).  Its own device allocation, on the context it was built on.
struct ProofStore {
    void* d_nodes = nullptr;
    rsm_ctx* ctx = nullptr;
    bool nmt = false;
    rsm_nmt_params p{};
    std::vector<uint32_t> status;  // 2 * width words: non-zero where a tree fails
    ProofStore() = default;
    ProofStore(const ProofStore&) = delete;
    ProofStore& operator=(const ProofStore&) = delete;
    ~ProofStore() { drop(); }
    void drop() {
        if (d_nodes) {
            if (ctx) (void)hipSetDevice(ctx->device);
            (void)hipFree(d_nodes);
        }
        d_nodes = nullptr;
        ctx = nullptr;
        status.clear();
    }
};

namespace rsm {
// The cached node store of a square, for the entry points outside rsm_proof.cpp
// (rsm_commit.cpp): the NMT params of (tree_fn, user) or nullptr; whether a complete square
// with a context takes the device path for tree `nmt`; the store itself, built once
// (ctx->eds_mu held, device selected).
const rsm_nmt_params* eds_nmt_of(rsm_tree_root_fn tree_fn, void* user);
bool eds_store_path(rsm_eds* e, const rsm_nmt_params* nmt, DevTree* dt);
int eds_ensure_store(rsm_eds* e, const rsm_nmt_params* nmt, const DevTree& dt);
}  // namespace rsm

struct rsm_eds {
    rsm_ctx* ctx = nullptr;
    uint32_t width = 0;
    uint32_t odw = 0;  // originalDataWidth
    uint32_t S = 0;    // shareSize
    HostSquare data;               // width*width*S, row-major
    std::vector<uint8_t> present;  // width*width
    std::vector<uint8_t> byz_data;
    std::vector<uint8_t> byz_present;
    rsm_repair_stats stats{};
    ProofStore proofs;

    uint8_t* cell(uint32_t r, uint32_t c) { return data.data() + ((size_t)r * width + c) * S; }
    const uint8_t* cell(uint32_t r, uint32_t c) const { return data.data() + ((size_t)r * width + c) * S; }
    bool has(uint32_t r, uint32_t c) const { return present[(size_t)r * width + c] != 0; }
    // (axis, index, position) -> cell coordinates
    uint32_t rr(int axis, uint32_t idx, uint32_t pos) const { return axis == RSM_AXIS_ROW ? idx : pos; }
    uint32_t cc(int axis, uint32_t idx, uint32_t pos) const { return axis == RSM_AXIS_ROW ? pos : idx; }
};
