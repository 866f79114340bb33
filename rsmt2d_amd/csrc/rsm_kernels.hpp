// rsm_kernels.hpp -- descriptors shared by the HIP kernels and the host runtime.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rsm {

__host__ __device__ constexpr uint32_t ceil_pow2(uint32_t x) {
    uint32_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

// A batch of codewords laid out affinely in device memory.  Codeword q lives in
// square q / per_square at offset (q % per_square) * cw_stride; its input
// symbol e (e < k) is the share at + e * elem_stride, its parity symbol e at
// + out_offset + e * elem_stride.  Rows of a [W][W][S] square:
//   cw_stride = W*S, elem_stride = S,   out_offset = k*S
// Columns:
//   cw_stride = S,   elem_stride = W*S, out_offset = k*W*S
struct CodewordSet {
    uint8_t* base;
    uint8_t* out_base;          // parity written at the same relative offsets from here
    const uint32_t* indices;    // optional: codeword q is vector indices[q] of square 0
    uint64_t square_stride;
    uint64_t cw_stride;
    uint64_t elem_stride;
    uint64_t out_offset;
    uint32_t per_square;
    uint32_t count;   // total codewords
    uint32_t k;
    uint32_t S;       // share size in bytes (multiple of 64)
    uint32_t chunks;  // ceil(S / bytes-per-wave)
    uint32_t pass;    // 0 = row pass of a square, 1 = column pass / anything else (launch shape)
    uint32_t grid;    // persistent-grid size (workgroups) of the bit-sliced launch: the
                      // context's CU count or its per-pass cap (rsm_ctx_set_pass_grid)
    uint32_t wide;    // non-zero: symbols addressed with 64-bit per-symbol bases (the
                      // wide forms; the host sets it when narrow_fits() fails)
    // Multi-GPU all-to-all (rsm_multi.cpp, round 6): honoured only by the single-pass
    // GF(2^16) encoders (shard_fused_ok(); the host never sets them otherwise).
    //   side (row pass): every cell c of codeword q -- data c = e, parity c = k + e --
    //     whose column block c / side_cols is not side_self is ALSO stored at
    //     side + (c / side_cols) * side_blk + q * side_cols * S + (c % side_cols) * S:
    //     the per-peer send blocks, packed by the encoder instead of a copy pass;
    //   blk (column pass): data symbol e of codeword (column) q whose row block
    //     h = e / blk_rows is not blk_self is read from
    //     blk + h * blk_size + (e % blk_rows) * blk_pitch + q * S -- the received blocks
    //     in place, instead of an unpack pass.
    uint8_t* side;
    uint64_t side_blk;
    uint32_t side_cols, side_self;
    const uint8_t* blk;
    uint64_t blk_size;
    uint32_t blk_rows, blk_self, blk_pitch;
};

// The single-pass kernels address a codeword's symbols with 32-bit buffer offsets
// from one 64-bit base per codeword half (encoders: the data symbols from the
// codeword's first cell, the parity from out_base + out_offset; decoders: each half
// of the 2k cells from its own first cell).  A half of k symbols e * es + byte must
// stay below kOffsetLimit -- the buffer resources' num_records, also the kernels'
// out-of-range marker -- so a half may span up to 2 GiB and a square up to 4 GiB;
// beyond that the wide forms (64-bit per-symbol bases) run instead.
constexpr uint64_t kOffsetLimit = 1ull << 31;
__host__ __device__ constexpr bool narrow_fits(uint64_t k, uint64_t es, uint64_t S, uint64_t limit = kOffsetLimit) {
    return (k + 1) * es + S <= limit;
}

// Parity addressed from its own base: out_base + out_offset with out_offset = 0
// (same bytes; the symbol offsets then span one half instead of out_offset + k es).
__host__ __device__ inline CodewordSet rebased(CodewordSet cs) {
    if (cs.out_base == nullptr) cs.out_base = cs.base;
    cs.out_base += cs.out_offset;
    cs.out_offset = 0;
    return cs;
}

// A list of row (axis 0) or column (axis 1) vectors of ONE [W][W][S] square to
// reconstruct in place; presence is one byte per cell (non-zero = present).
struct DecodeSet {
    uint8_t* base;
    const uint8_t* presence;
    const uint32_t* indices;
    uint32_t count;
    uint32_t axis;
    uint32_t k;
    uint32_t S;
    uint32_t chunks;
    // Zero-copy forms (the M = 128 split decoder and the GF(2^16) single-pass decoders;
    // both nullable): `in_base` (a host-mapped copy of the square): read the present
    // cells from there instead of `base` and store them into `base` as well; `mirror`:
    // write every rebuilt cell there too.
    const uint8_t* in_base;
    uint8_t* mirror;
    // Workgroups of the M = 128 split decoder (0: one per task).  A smaller grid
    // loops over the tasks, so the zero-copy form streams: a workgroup's stores
    // drain over PCIe while its next loads arrive, instead of every workgroup
    // loading, then computing, then storing in lockstep.
    uint32_t grid;
    // diagnostic builds only: per-workgroup phase stamps of the M = 128 split decoder
    // (kDecTraceWords s_memrealtime values per workgroup; nullptr = off)
    uint32_t* trace;
    // diagnostic builds only: the upper half of the split decoder's grid issues its
    // point loads `delay` s_memrealtime ticks (100 MHz) after it starts (0 = off)
    uint32_t delay;
    // wide forms only (64-bit per-cell bases; the host sets `wide` when narrow_fits()
    // fails): bytes between consecutive cells, 0 = S.  The host runs a share wider
    // than one launch handles as byte slabs: base advanced by the slab's first byte,
    // S = the slab's width, pitch = the share size.
    uint32_t wide;
    uint64_t pitch;
};
constexpr int kDecTraceWords = 8;
// DecodeSet::delay value of the diagnostic setup-free floor (rsm_diag_set_dec8_mode(2))
constexpr uint32_t kDecFloor = 0xFFFFFFFFu;
void set_dec_diag_trace(uint32_t* d);
uint32_t* dec_diag_trace_ptr();  // (diagnostic builds; the GF(2^16) single-pass decoders stamp kDec16TraceWords)
constexpr int kDec16TraceWords = 16;
void set_dec_diag_delay(uint32_t ticks);
void set_dec8_diag_mode(uint32_t mode);  // diagnostic builds only: 1 = the other split-decoder locator form
void set_codec_spin_diag(uint32_t us);  // diagnostic builds only (rsm_runtime.cpp)
void set_repair_diag_mode(uint32_t m);  // diagnostic builds only (eds.cpp)

hipError_t launch_encode_gf8(const CodewordSet& cs, hipStream_t st);
// wide forms of the byte-table GF(2^8) kernels (any k <= 128): 64-bit per-symbol
// bases, a capped grid looping over the (codeword, 256-byte chunk) tasks
hipError_t launch_encode_gf8_wide(const CodewordSet& cs, hipStream_t st);
hipError_t launch_decode_gf8_wide(const DecodeSet& ds, hipStream_t st);
// bit-sliced M = 128 encode (kernels_gf8_bs.hip); launch_encode_gf8 picks it when applicable
bool bs128_applicable(const CodewordSet& cs);
hipError_t launch_encode_gf8_bs128(const CodewordSet& cs, hipStream_t st);
hipError_t launch_decode_gf8(const DecodeSet& ds, hipStream_t st);
// Latency form of the M = 128 encode (65 <= k <= 128) for one or a few squares
// (kernels_gf8.hip encode_gf8_split_kernel): NW waves per (codeword, 256-B chunk) on
// byte tables, every CU busy.  Launches the codewords of `a` and, if b != nullptr,
// those of `b` in the same grid.
// nw: waves per (codeword, 256-byte chunk), 8 or 16 (kSplitWavesOne)
hipError_t launch_encode_gf8_split(const CodewordSet& a, const CodewordSet* b, hipStream_t st, int nw);
constexpr int kSplitWavesOne = 16;  // one square / one codeword: the 16-wave latency form
constexpr uint32_t kSplitSmallBatch = 64;  // 9 <= k <= 64: squares per call for the split form (split_max > 0)
void set_split_diag_waves(int first, int second);  // diagnostic builds only
void set_split_diag_fused(bool on);                  // diagnostic builds only
void set_dec16_diag_mode(uint32_t mode);            // diagnostic builds only: dec16h_kernel A/B bits
bool bs128_diag_xcd_queues();                        // diagnostic builds only: XCD-affine queue mode set
bool split_fused_enabled();                          // product: always
// One square in ONE launch of the split encoder (rows -> Q1, Q0 columns -> Q2, then
// Q1 columns -> Q3 behind a device-side wait on the row tasks); ctr: >= 33 zeroed
// words it leaves zeroed, err: pinned host word set by a stuck wait.  Every workgroup
// must be able to be resident at once (the caller checks the grid).
hipError_t launch_extend_gf8_split_fused(const CodewordSet& rows, const CodewordSet& c0, const CodewordSet& c1,
                                         uint32_t* ctr, uint32_t* err, hipStream_t st);
struct Gf16Dev;
hipError_t launch_encode_gf16(const CodewordSet& cs, const Gf16Dev& g, hipStream_t st);
hipError_t launch_decode_gf16(const DecodeSet& ds, const Gf16Dev& g, hipStream_t st);
// Merkle roots (kernels_sha.hip): d_leaf scratch of squares*W*W*32 bytes
bool roots_dev_supported(uint32_t W);
// Namespaced Merkle tree roots (kernels_nmt.hip): d_leaf W*W*64 bytes of scratch,
// d_roots 2W roots of 2*ns+32 bytes, d_status (nullable) 2W words.
bool nmt_dev_supported(uint32_t W, uint32_t ns);
hipError_t launch_nmt_roots(const uint8_t* d_eds, uint32_t W, uint32_t S, uint32_t ns, uint32_t k, uint32_t ignore_max,
                            uint32_t* d_leaf, uint8_t* d_roots, uint32_t* d_status, hipStream_t st, uint32_t squares = 1);
hipError_t launch_roots(const uint8_t* d_eds, uint32_t W, uint32_t S, uint32_t squares, uint32_t* d_leaf,
                        uint8_t* d_roots, hipStream_t st);
hipError_t launch_leaf_hashes(const uint8_t* d_cells, uint32_t cells, uint32_t S, uint32_t* d_leaf, hipStream_t st);
hipError_t launch_tree_roots(const uint32_t* d_leaf, uint32_t W, uint32_t first, uint32_t count, uint8_t* d_roots,
                             hipStream_t st);
// ---- share inclusion proofs (DESIGN.md §4 "Proofs") -----------------------------
// The node store keeps every node of the 2W trees of `squares` squares, by levels: node
// (l, j) of a tree covers leaves [j 2^l, min((j + 1) 2^l, W)); level l has
// ceil(W / 2^l) nodes and an unpaired last node is carried up unchanged (a copy).
// Words of the store:
//   [squares][W * W][leaf_words]   level 0: the leaf records, one per cell (a cell's
//                                  record serves its row tree and its column tree)
//   [squares][2W][U][node_words]   levels 1 .. L of each tree (rows, then columns),
//                                  level after level; U = proof_tree_nodes(W)
// DefaultTree: leaf_words = node_words = 8 (the digest as big-endian words).  NMT:
// leaf_words = 16 (namespace[8] | digest[8]), node_words = 24 (min[8] | max[8] | digest[8]).
__host__ __device__ constexpr uint32_t proof_levels(uint32_t W) {  // ceil(log2 W)
    uint32_t l = 0;
    while ((1u << l) < W) ++l;
    return l;
}
__host__ __device__ constexpr uint32_t proof_level_count(uint32_t W, uint32_t l) { return (W + (1u << l) - 1) >> l; }
// index of node (l, 0) among a tree's nodes of levels 1 .. L (l >= 1)
__host__ __device__ constexpr uint32_t proof_level_offset(uint32_t W, uint32_t l) {
    uint32_t o = 0;
    for (uint32_t i = 1; i < l; ++i) o += proof_level_count(W, i);
    return o;
}
__host__ __device__ constexpr uint32_t proof_tree_nodes(uint32_t W) { return proof_level_offset(W, proof_levels(W) + 1); }
constexpr uint32_t kProofShaWords = 8, kProofNmtLeafWords = 16, kProofNmtNodeWords = 24;
__host__ __device__ constexpr uint64_t proof_store_words(uint32_t W, uint32_t squares, uint32_t leaf_words,
                                                         uint32_t node_words) {
    return (uint64_t)squares * ((uint64_t)W * W * leaf_words + (uint64_t)2 * W * proof_tree_nodes(W) * node_words);
}
// Node-store builds (kernels_sha.hip, kernels_nmt.hip): leaf records, then every tree
// level written to the store as it is produced.  d_store 16-byte aligned; d_roots /
// d_status nullable, laid out as launch_roots / launch_nmt_roots write them.
uint32_t proof_trees_per_block(uint32_t W);  // trees a workgroup of either build takes (kernels_sha.hip)
hipError_t launch_tree_nodes(const uint8_t* d_eds, uint32_t W, uint32_t S, uint32_t squares, uint32_t* d_store,
                             uint8_t* d_roots, hipStream_t st);
hipError_t launch_nmt_nodes(const uint8_t* d_eds, uint32_t W, uint32_t S, uint32_t ns, uint32_t k, uint32_t ignore_max,
                            uint32_t squares, uint32_t* d_store, uint8_t* d_roots, uint32_t* d_status, hipStream_t st);
// A sample: leaf `pos` of row (axis 0) or column (axis 1) `index` of square `square`
// (the C ABI's rsm_sample).
struct ProofSample {
    uint32_t square, axis, index, pos;
};
// Gather kernels (kernels_proof.hip).  ns = 0: DefaultTree store, else an NMT store
// with ns-byte namespaces.  d_records: n records of 8 + L * node_len bytes.  d_shares
// (16-byte aligned, like d_eds): n shares of S bytes.  Every sample must be in range:
// the host validates them.
hipError_t launch_proof_gather(const uint32_t* d_store, uint32_t W, uint32_t squares, uint32_t ns,
                               const ProofSample* d_samples, uint32_t n, uint8_t* d_records, hipStream_t st);
hipError_t launch_share_gather(const uint8_t* d_eds, uint32_t W, uint32_t S, const ProofSample* d_samples, uint32_t n,
                               uint8_t* d_shares, hipStream_t st);
// ---- namespace proofs (DESIGN.md §4 "Namespace proofs"; kernels_nsproof.hip) --------
// A query: every share of namespace `nid` (8 big-endian words, zero padded, as the
// store's leaf records hold a namespace) in row / column `index` of square `square`.
struct NsQuery {
    uint32_t square, axis, index;
    uint32_t nid[8];
};
constexpr uint32_t kNsEmpty = 0, kNsInclusion = 1, kNsAbsence = 2, kNsTree = 3;
// The range proof of leaves [start, end) of a tree of W leaves, by levels: with a = start
// and last = end - 1, level l gives the left node (l, a - 1) when a is odd and the right
// node (l, last + 1) when last is even and below the level's last node; then both halve.
// Returns the node count; *n_left: how many of them are left nodes.
__host__ __device__ constexpr uint32_t ns_range_nodes(uint32_t W, uint32_t start, uint32_t end, uint32_t* n_left) {
    uint32_t a = start, last = end - 1, nl = 0, nr = 0;
    for (uint32_t l = 0, L = proof_levels(W); l < L; ++l) {
        if (a & 1u) ++nl;
        if (!(last & 1u) && last + 1 < proof_level_count(W, l)) ++nr;
        a >>= 1;
        last >>= 1;
    }
    *n_left = nl;
    return nl + nr;
}
// Records of 16 + (2L + 1) * (2 ns + 32) bytes (any alignment): u32 kind | start | end |
// n_nodes, the nodes (left ones top-down, then right ones bottom-up), zeros up to slot
// 2L, slot 2L the leaf node of an absence proof.  Three steps, all on `st`:
//   locate : one lane per query -- the tree's status word, its top node, two binary
//            searches (at most L + 1 probes each) over the vector's level-0 namespaces;
//            writes the record header and the query's share count into d_offsets[i]
//   scan   : d_offsets[0 .. n] becomes the exclusive prefix sum of the counts
//            (d_offsets[n]: the total), one workgroup
//   gather : one lane per (query, slot) copies or zero-fills its node; one wave per
//            query copies its shares (16-byte words) to d_shares + d_offsets[i] * S when
//            d_offsets[i + 1] <= shares_cap (d_shares nullable: no shares)
// d_status: 2W words per square as launch_nmt_nodes wrote them.  Queries are validated
// on the host.
hipError_t launch_ns_proofs(const uint32_t* d_store, const uint32_t* d_status, const uint8_t* d_eds, uint32_t W,
                            uint32_t S, uint32_t squares, uint32_t ns, const NsQuery* d_queries, uint32_t n,
                            uint8_t* d_records, uint32_t* d_offsets, uint8_t* d_shares, uint64_t shares_cap,
                            hipStream_t st);
// Proof verification (DESIGN.md §4 "Verification"; the DefaultTree kernel in
// kernels_sha.hip, the NMT kernels in kernels_nmt.hip): one lane per sample hashes its
// share (d_shares: [n][S], 16-byte aligned), folds the siblings of its record
// (d_records: [n][8 + L * node_len], any alignment) and compares with its root
// (d_roots: [squares][2][W][node_len]); d_status[n] receives a kProof* word.  The node
// count and operand sides come from (W, pos) alone: the record's header is only
// compared with them, and no address depends on record or share contents.  Any
// 1 <= W <= 65536; every sample must be in range (the host validates them).
constexpr uint32_t kProofOk = 0, kProofMalformed = 1, kProofOrder = 2, kProofRoot = 3;
hipError_t launch_proof_verify(const uint8_t* d_shares, const uint8_t* d_records, const uint8_t* d_roots, uint32_t W,
                               uint32_t S, const ProofSample* d_samples, uint32_t n, uint32_t* d_status, hipStream_t st);
hipError_t launch_nmt_proof_verify(const uint8_t* d_shares, const uint8_t* d_records, const uint8_t* d_roots, uint32_t W,
                                   uint32_t S, uint32_t ns, uint32_t k, uint32_t ignore_max, const ProofSample* d_samples,
                                   uint32_t n, uint32_t* d_status, hipStream_t st);
// Namespace proof verification (DESIGN.md §4 "Namespace proofs"; kernels_nmt.hip): one
// wave per query.  Query i: is record i (d_records: [n][16 + (2L + 1) * node_len], any
// alignment) with shares [d_offsets[i], d_offsets[i + 1]) of d_shares (16-byte aligned,
// shares_total shares) a complete answer for d_queries[i].nid in vector (square, axis,
// index), under root (square, axis, index) of d_roots?  d_status[n] receives a kProof*
// word with rsm_nmt_namespace_verify's precedence; offsets that decrease or pass
// shares_total give kProofMalformed before anything else of the query is read.  Counts,
// operand sides and every address come from (W, start, end) and the offsets, never from
// what a record or a share holds.  1 <= W <= 1024 (a wave's LDS holds W nodes); every
// query must be in range (the host validates them).
constexpr uint32_t kProofNamespace = 5, kProofIncomplete = 6;
bool nmt_ns_verify_supported(uint32_t W, uint32_t ns);
hipError_t launch_nmt_ns_verify(const uint8_t* d_records, const uint32_t* d_offsets, const uint8_t* d_shares,
                                uint64_t shares_total, const uint8_t* d_roots, uint32_t W, uint32_t S, uint32_t ns,
                                uint32_t k, uint32_t ignore_max, const NsQuery* d_queries, uint32_t n, uint32_t* d_status,
                                hipStream_t st);
// ---- range proofs (DESIGN.md §4 "Range proofs") ---------------------------------------
// A query: leaves [start, end) of row / column `index` of square `square` (the C ABI's
// rsm_range_query).  Its record is the namespace record of kind kNsInclusion over the
// caller's range, out of either tree's store (ns = 0: DefaultTree, 32-byte nodes).
struct RangeQuery {
    uint32_t square, axis, index, start, end;
};
// launch_ns_proofs with a header kernel in locate's place (kernels_nsproof.hip): one lane
// per query writes kind | start | end | n_nodes and the share count end - start; scan,
// gather and shares are the namespace proofs' kernels.  Queries are validated on the host
// (start < end <= W).
hipError_t launch_range_proofs(const uint32_t* d_store, const uint8_t* d_eds, uint32_t W, uint32_t S, uint32_t squares,
                               uint32_t ns, const RangeQuery* d_queries, uint32_t n, uint8_t* d_records,
                               uint32_t* d_offsets, uint8_t* d_shares, uint64_t shares_cap, hipStream_t st);
// Range proof verification (NMT: kernels_nmt.hip, DefaultTree: kernels_sha.hip): one wave
// per query, as launch_nmt_ns_verify.  Query i: are shares [d_offsets[i], d_offsets[i + 1])
// of d_shares leaves [start, end) of vector (square, axis, index), by record i, under root
// (square, axis, index) of d_roots?  kProofMalformed (the offsets, then the record's header
// against the QUERY's start and end and the node count they dictate), kProofOrder (NMT),
// kProofRoot, kProofOk.  d_root_records non-null: the chained form -- d_roots is not read;
// root record i ([n][8 + L2 * 32]) is checked against (2W, axis W + index) with the other
// headers, the fold's root is hashed as that leaf of the data-root tree, folded on and
// compared with d_data_roots[square].  ns = 0 is not taken by the NMT launch; W <= 1024
// (NMT), 2048 (DefaultTree): a wave's LDS holds W nodes.
bool range_verify_supported(uint32_t W, uint32_t ns);  // ns = 0: DefaultTree
hipError_t launch_nmt_range_verify(const uint8_t* d_records, const uint32_t* d_offsets, const uint8_t* d_shares,
                                   uint64_t shares_total, const uint8_t* d_roots, const uint8_t* d_root_records,
                                   const uint8_t* d_data_roots, uint32_t W, uint32_t S, uint32_t ns, uint32_t k,
                                   uint32_t ignore_max, const RangeQuery* d_queries, uint32_t n, uint32_t* d_status,
                                   hipStream_t st);
hipError_t launch_range_verify(const uint8_t* d_records, const uint32_t* d_offsets, const uint8_t* d_shares,
                               uint64_t shares_total, const uint8_t* d_roots, const uint8_t* d_root_records,
                               const uint8_t* d_data_roots, uint32_t W, uint32_t S, const RangeQuery* d_queries, uint32_t n,
                               uint32_t* d_status, hipStream_t st);
// ---- data root (DESIGN.md §4 "Data root"; kernels_dataroot.hip) ----------------------
// The tree over the N = 2W roots of a square (leaf t: the root bytes of tree t, rows then
// columns, root_len = 32 .. 96 bytes each), in the level picture above with 32-byte
// digests at every level: leaf SHA256(0x00 || root), node SHA256(0x01 || l || r), an
// unpaired last node carried up.  Words of its node store, per square:
//   [N][8]                     level 0: the leaf digests (big-endian words)
//   [proof_tree_nodes(N)][8]   levels 1 .. L2 = proof_levels(N), level after level
constexpr uint32_t kDataRootMaxWidth = 2048;  // every width for which device roots exist
__host__ __device__ constexpr uint64_t data_root_tree_words(uint32_t W) {
    return ((uint64_t)2 * W + proof_tree_nodes(2 * W)) * 8u;
}
// A root to prove: tree (axis, index) of square `square` (the C ABI's rsm_root_ref).
struct RootRef {
    uint32_t square, axis, index;
};
bool data_roots_dev_supported(uint32_t W);
// One workgroup per square: d_roots [squares][2][W][root_len] (any alignment) ->
// d_data_roots [squares][32] (any alignment); d_store (nullable, 16-byte aligned):
// squares * data_root_tree_words(W) words.  LDS: W * 32 bytes.
hipError_t launch_data_roots(const uint8_t* d_roots, uint32_t W, uint32_t root_len, uint32_t squares,
                             uint8_t* d_data_roots, uint32_t* d_store, hipStream_t st);
// n records of 8 + L2 * 32 bytes (any alignment) out of a store; refs validated on the host.
hipError_t launch_data_root_gather(const uint32_t* d_store, uint32_t W, const RootRef* d_refs, uint32_t n,
                                   uint8_t* d_records, hipStream_t st);
// Chained verification (kernels_sha.hip, kernels_nmt.hip): launch_proof_verify /
// launch_nmt_proof_verify with no root table.  Sample i also takes root record i
// (d_root_records: [n][8 + L2 * 32], any alignment) and is compared with
// d_data_roots[square] (32 bytes): the share fold's result is hashed as leaf
// axis * W + index of the data-root tree and folded on.  Both headers are compared with
// what (W, pos) and (2W, axis * W + index) dictate before anything is hashed
// (kProofMalformed); then kProofOrder (NMT), kProofRoot, kProofOk.  Any 1 <= W <= 65536.
hipError_t launch_proof_verify_data_root(const uint8_t* d_shares, const uint8_t* d_records, const uint8_t* d_root_records,
                                         const uint8_t* d_data_roots, uint32_t W, uint32_t S,
                                         const ProofSample* d_samples, uint32_t n, uint32_t* d_status, hipStream_t st);
hipError_t launch_nmt_proof_verify_data_root(const uint8_t* d_shares, const uint8_t* d_records,
                                             const uint8_t* d_root_records, const uint8_t* d_data_roots, uint32_t W,
                                             uint32_t S, uint32_t ns, uint32_t k, uint32_t ignore_max,
                                             const ProofSample* d_samples, uint32_t n, uint32_t* d_status, hipStream_t st);
// ---- device-resident Repair (DESIGN.md §5 "Device-resident Repair"; kernels_repair.hip) ----
// The sweep planner, one workgroup per square of d_presence ([count][W][W] bytes, 4-byte
// aligned, non-zero = present; 2 <= W <= 2048, even).  A launch first marks present every
// cell of the vectors its predecessor listed (d_prev_todo, of the other axis), then lists
// in d_todo ([count][W]) the vectors of `axis` with k <= have < W, ascending.  d_state:
// one word per square that belongs to the planner (its last todo count); first: it is
// not read.  report (pinned host memory through its device mapping, or device memory):
// per square the todo count and the cells missing before this pass's decodes.  d_skip
// (nullable): one word per square, non-zero = the square has dropped out of a checked
// call; its presence bytes are left alone and it reports an empty list.
bool repair_plan_supported(uint32_t W);
hipError_t launch_repair_plan(uint8_t* d_presence, uint32_t W, uint32_t count, uint32_t axis, bool first,
                              const uint32_t* d_prev_todo, uint32_t* d_todo, uint32_t* d_state, uint32_t* report,
                              hipStream_t st, const uint32_t* d_skip = nullptr);
// Batch verification of n completed squares, square d_map[j] of d_eds against work square
// j (both [2k][2k][S], 16-byte aligned): the Q0 copy, then after the work squares are
// re-extended d_flags[2j] = 1 where the squares differ, and d_flags[2j + 1] = 1 where the
// roots computed for work square j (d_got: roots_bytes per square, any alignment) differ
// from the committed ones of square d_map[j] or a tree status word (d_status: `words` per
// square, nullable) is non-zero.  The flags start at 0.
hipError_t launch_repair_gather_q0(const uint8_t* d_eds, uint8_t* d_work, const uint32_t* d_map, uint32_t k, uint32_t S,
                                   uint32_t n, hipStream_t st);
hipError_t launch_repair_compare_squares(const uint8_t* d_eds, const uint8_t* d_work, const uint32_t* d_map,
                                         uint64_t sq_bytes, uint32_t n, uint32_t* d_flags, hipStream_t st);
hipError_t launch_repair_compare_roots(const uint8_t* d_got, const uint32_t* d_status, const uint8_t* d_committed,
                                       const uint32_t* d_map, uint32_t roots_bytes, uint32_t words, uint32_t n,
                                       uint32_t* d_flags, hipStream_t st);
// ---- checked Repair (rsm_repair_squares_checked_dev): every vector is checked against its
// committed root and its own encoding in the stage in which it first has all W cells ----
// A stage's lists (kernels_repair.hip): d_list [count][2][W] words (rows, then columns,
// ascending), d_cnt [count][2], d_checked [count][2][W] bytes (zeroed by the caller once;
// a listed vector's byte becomes 1).  mode 0: every complete vector, from d_presence
// alone; 1: the vectors d_todo lists for `axis` (d_state: their count, as
// launch_repair_plan left both); 2: the unchecked vectors of the other axis that are
// complete once the cells of d_todo's vectors count as present.  A square with a non-zero
// d_skip word lists nothing.  report (pinned, mapped): three words per square -- the two
// counts and (mode 0) the cells missing.
hipError_t launch_repair_check_plan(const uint8_t* d_presence, uint32_t W, uint32_t count, uint32_t mode, uint32_t axis,
                                    const uint32_t* d_todo, const uint32_t* d_state, const uint32_t* d_skip,
                                    uint8_t* d_checked, uint32_t* d_list, uint32_t* d_cnt, uint32_t* report,
                                    hipStream_t st);
// Leaf records of the listed vectors' cells that have none yet (kernels_sha.hip: 8 words
// per cell; kernels_nmt.hip: 16, the node store's level 0), one lane per (list entry,
// position) of grid (ceil(max_n W / 256), count); max_n: the largest cnt[s][0] + cnt[s][1].
// d_recorded: one bit per cell, [count][ceil(W W / 32)] words, zeroed by the caller once
// -- the lane that sets a cell's bit hashes it, so a cell is hashed once per call whichever
// lane that is; d_hashed [count]: records computed so far (sums: no order shows in them).
hipError_t launch_list_leaf_hashes(const uint8_t* d_eds, uint32_t W, uint32_t S, uint32_t count, uint32_t max_n,
                                   const uint32_t* d_list, const uint32_t* d_cnt, uint32_t* d_recorded,
                                   uint32_t* d_hashed, uint32_t* d_leaf, hipStream_t st);
hipError_t launch_nmt_list_leaves(const uint8_t* d_eds, uint32_t W, uint32_t S, uint32_t ns, uint32_t k, uint32_t count,
                                  uint32_t max_n, const uint32_t* d_list, const uint32_t* d_cnt, uint32_t* d_recorded,
                                  uint32_t* d_hashed, uint32_t* d_leaf, hipStream_t st);
// One tree per list entry over the records (leaves along the row, or strided down the
// column), compared in the kernel with its committed root (d_committed: [count][2][W]
// [root_len], any alignment): d_verdict, laid out as d_list, receives 0, kByzRoot or
// (NMT, consulted first) kByzTree.  One launch for every square of the batch.
constexpr uint32_t kByzRoot = 1, kByzEncoding = 2, kByzTree = 3;
// Entry e of square s's lists: the rows first (cnt[s][0] of them), then the columns;
// *slot: its word in d_list, d_verdict and the parity flags.  False past the last entry.
__host__ __device__ inline bool list_entry(const uint32_t* list, const uint32_t* cnt, uint32_t W, uint32_t s, uint32_t e,
                                           uint32_t* axis, uint32_t* index, uint64_t* slot) {
    const uint32_t n0 = cnt[2 * s], n1 = cnt[2 * s + 1];
    if (e >= n0 + n1) return false;
    *axis = e >= n0 ? 1u : 0u;
    *slot = (uint64_t)s * 2 * W + *axis * W + (e - *axis * n0);
    *index = list[*slot];
    return true;
}
hipError_t launch_list_tree_check(const uint32_t* d_leaf, uint32_t W, uint32_t count, uint32_t max_n,
                                  const uint32_t* d_list, const uint32_t* d_cnt, const uint8_t* d_committed,
                                  uint32_t* d_verdict, hipStream_t st);
hipError_t launch_nmt_list_tree_check(const uint32_t* d_leaf, uint32_t W, uint32_t ns, uint32_t ignore_max,
                                      uint32_t count, uint32_t max_n, const uint32_t* d_list, const uint32_t* d_cnt,
                                      const uint8_t* d_committed, uint32_t* d_verdict, hipStream_t st);
// A stage's verdict per square: the minimum over its failing list entries of
// (2 index + axis) << 2 | reason (d_verdict's word, else kByzEncoding where d_parity's
// word -- laid out as d_list -- is set), ~0 when none fails, into report[2 s] (pinned,
// mapped); a failing square's d_skip word becomes 1.  stage2 (the lists are what a pass
// of `axis` completed; d_todo, d_state as its plan left them): a failing square's decoded
// vectors, which all passed stage 1, are marked present in d_presence -- no later plan
// will -- and report[2 s + 1] counts the cells that were missing among them.
hipError_t launch_repair_check_pick(const uint32_t* d_list, const uint32_t* d_cnt, const uint32_t* d_verdict,
                                    const uint32_t* d_parity, uint32_t W, uint32_t count, bool stage2, uint32_t axis,
                                    const uint32_t* d_todo, const uint32_t* d_state, uint8_t* d_presence,
                                    uint32_t* d_skip, uint32_t* report, hipStream_t st);
// d_shares [n][W][S] (16-byte aligned) and d_present [n][W]: vector d_refs[i] of the squares
// and its presence bytes; refs validated on the host.
hipError_t launch_vectors_gather(const uint8_t* d_eds, const uint8_t* d_presence, uint32_t W, uint32_t S,
                                 const RootRef* d_refs, uint32_t n, uint8_t* d_shares, uint8_t* d_present,
                                 hipStream_t st);
// Verified samples into device squares, two launches: decide (one lane per sample, from
// the statuses and the presence bytes as they stand; d_prev[i]: the next lower sample of
// the same cell or ~0; d_verdict: n words of scratch), then apply (one wave per sample:
// the winners' shares and presence bytes, kProofOccupied into the losers' status words).
hipError_t launch_samples_scatter(const ProofSample* d_samples, const uint32_t* d_prev, uint32_t* d_verdict,
                                  const uint8_t* d_shares, uint8_t* d_eds, uint8_t* d_presence, uint32_t* d_status,
                                  uint32_t W, uint32_t S, uint32_t n, hipStream_t st);
// ---- fraud proofs (rsm_fraud_proofs_verify_dev; DESIGN.md §5 "Fraud proofs"; kernels_fraud.hip) ----
// n proofs as packed vectors: d_shares [n][W][S] (16-byte aligned), d_present [n][W], as
// launch_vectors_gather writes them; d_refs[i]: the vector proof i accuses (validated on the
// host).  The proofs are taken in chunks of W: chunk c is rows [c W, min((c + 1) W, n)) of
// d_shares, which the decoders and encoders address as rows of one square.
constexpr uint32_t kFraudValid = 0, kFraudTooFew = 1, kFraudShare = 2, kFraudConsistent = 3;
bool fraud_supported(uint32_t W, uint32_t ns);  // ns = 0: DefaultTree
// Two launches.  d_have [n]: non-zero presence bytes of each proof; d_samples [n][W]: slot j
// of proof i as {square, axis ^ 1, j, index}, the sample its record proves; d_dec_list,
// d_chk_list [chunks][W]: per chunk the chunk-local rows with k <= have < W and with
// have >= k, ascending; d_slot [n]: a checked proof's word of d_chk_list (and of the parity
// flags), ~0 otherwise; report (pinned, mapped): two words per chunk, the lists' lengths.
hipError_t launch_fraud_plan(const uint8_t* d_present, const RootRef* d_refs, uint32_t W, uint32_t n, uint32_t* d_have,
                             ProofSample* d_samples, uint32_t* d_dec_list, uint32_t* d_chk_list, uint32_t* d_slot,
                             uint32_t* report, hipStream_t st);
// Leaf records of every proof with have >= k (d_leaf: [n][W] records of 8 words, NMT 16; the
// NMT namespace of (i, pos) is the share's own when d_refs[i].index < sq and pos < sq),
// then one tree per such proof, compared with committed root (square, axis, index) of
// d_committed ([squares][2][W][root_len], any alignment): d_tree[i] receives 0, kByzRoot or
// (NMT, consulted first) kByzTree.
hipError_t launch_fraud_trees(const uint8_t* d_shares, const uint32_t* d_have, const RootRef* d_refs, uint32_t W, uint32_t S,
                              uint32_t n, uint32_t ns, uint32_t sq, uint32_t ignore_max, const uint8_t* d_committed,
                              uint32_t* d_leaf, uint32_t* d_tree, hipStream_t st);
// The verdict records, four words per proof (rsm_fraud_verdict) into `out` (16-byte aligned;
// pinned and mapped, or device memory): kFraudTooFew below k; else kFraudShare with the
// lowest present slot whose word of d_status ([n][W], the verify kernels') is non-zero; else
// kFraudValid with d_tree's word or kByzEncoding where the proof's parity flag
// (d_parity[d_slot[i]], launch_compare_parity's) is set; else kFraudConsistent.
hipError_t launch_fraud_verdicts(const uint8_t* d_present, const uint32_t* d_have, const uint32_t* d_status,
                                 const uint32_t* d_tree, const uint32_t* d_slot, const uint32_t* d_parity, uint32_t W,
                                 uint32_t n, uint32_t* out, hipStream_t st);
// ---- share commitments (DESIGN.md §4 "Commitments"; kernels_commit.hip) ----------------
// A blob's commitment: the RFC 6962 root (leaf SHA256(0x00 || root), node
// SHA256(0x01 || l || r)) over its subtree roots, the NMT roots (min || max || digest,
// 2 ns + 32 bytes, every leaf under its own namespace) over the runs of its mountain range.
constexpr uint32_t kCommitOrder = 1, kCommitTree = 2;  // status words (the C ABI's RSM_COMMIT_*)
constexpr uint32_t kCommitMaxRoots = 4096;             // subtree roots of one blob: the fold's LDS
constexpr uint32_t kCommitWaveMax = 128;               // subtrees up to this size take the wave form
// A subtree of the shares path: its first leaf record and its slot among the packed roots.
struct CommitTask {
    uint32_t first, slot;
};
// A blob of the store path: ODS shares [start, start + len) of `square`, subtree width w,
// m subtree roots whose packed slots begin at root_off.
struct CommitBlob {
    uint32_t square, start, len, w, root_off, m;
};
// Whether the subtree pass takes subtrees of z leaves (a power of two; above
// kCommitWaveMax the workgroup tree's limits, nmt_dev_supported).
bool commit_subtree_supported(uint32_t z, uint32_t ns);
// d_leaf [total][16] words: the leaf record of each of `total` packed shares (16-byte
// aligned, S a multiple of 64 and >= ns) under the share's own namespace.
hipError_t launch_commit_leaves(const uint8_t* d_shares, uint32_t total, uint32_t S, uint32_t ns, uint32_t* d_leaf,
                                hipStream_t st);
// n_tasks subtrees of z leaves each: root bytes at d_roots + slot * (2 ns + 32), the
// slot's word of d_flags non-zero where the subtree's namespaces are out of order.
hipError_t launch_commit_subtrees(const uint32_t* d_leaf, const CommitTask* d_tasks, uint32_t n_tasks, uint32_t z,
                                  uint32_t ns, uint32_t ignore_max, uint8_t* d_roots, uint32_t* d_flags, hipStream_t st);
// One workgroup per blob: blob b's roots are slots [d_root_offs[b], d_root_offs[b + 1]),
// at most max_m <= kCommitMaxRoots of them.  d_commitments [n][32] (any alignment; zeros
// with status kCommitOrder where a flag of the blob is set), d_status [n].
hipError_t launch_commit_fold(const uint8_t* d_roots, const uint32_t* d_flags, const uint32_t* d_root_offs, uint32_t n,
                              uint32_t max_m, uint32_t ns, uint8_t* d_commitments, uint32_t* d_status, hipStream_t st);
// The same over roots gathered from an NMT node store of `squares` squares of width W
// (d_status_trees: 2W words per square; a touched row's non-zero word gives kCommitTree and
// zeros).  Blobs validated on the host.  d_roots_out (nullable, any alignment) receives the
// roots at their packed slots, d_root_offs_out (nullable) the n + 1 slot offsets.
hipError_t launch_commit_fold_store(const uint32_t* d_store, const uint32_t* d_status_trees, uint32_t W, uint32_t squares,
                                    uint32_t ns, const CommitBlob* d_blobs, uint32_t n, uint32_t max_m, uint8_t* d_roots_out,
                                    uint32_t* d_root_offs_out, uint8_t* d_commitments, uint32_t* d_status, hipStream_t st);
hipError_t launch_fill_random(void* p, uint64_t bytes, uint64_t seed, hipStream_t st);
hipError_t launch_compare(const uint8_t* a, const uint8_t* b, uint64_t n, uint32_t* mismatch, hipStream_t st);
// dst = src for ceil(bytes / 16) 16-byte words (src: e.g. a pinned buffer's device mapping)
hipError_t launch_stage_copy(void* dst, const void* src, uint64_t bytes, hipStream_t st);
hipError_t launch_compare_parity(const uint8_t* a, const uint8_t* b, uint32_t k, uint32_t S, uint32_t axis,
                                 const uint32_t* indices, uint32_t count, uint32_t* flags, hipStream_t st);

// One launch that runs both passes of the 2D extension over `count` k = 128
// squares (kernels_gf8_bs.hip, extend_gf8_bs128q_kernel): row sets and Q0-column
// sets from one queue head, Q1-column sets from a ready list that the last row set
// of each square appends to, so the column sets re-read Q0 and Q1 while they are
// still in the Infinity Cache.  ctr: 224 + 2 * count zeroed words (the kernel
// leaves them zeroed again); a bounded wait that times out (never, by the
// deadlock-freedom argument in the kernel, short of a hardware fault) sets *err,
// a device-visible pinned host word the host checks after the stream completes.
struct QueuePlan {
    CodewordSet rows, cols;
    uint32_t* ctr;
    uint32_t* err;   // pinned host word (device-visible)
    uint32_t count;  // squares
    uint32_t rn, cn; // sets per square: row pass (= Q0-column sets = Q1-column sets), column pass
    uint32_t delay;  // row sets handed out before the first Q0-column set (<= count * rn)
    uint32_t nmain;  // 2 * count * rn: row sets + Q0-column sets
    uint32_t nq1;    // count * rn: Q1-column sets
    uint32_t margin; // a Q1-column set is claimed while more than this many ready ones are unclaimed
    uint32_t* trace; // diagnostic build only (phase timeline), else nullptr
};
constexpr uint32_t kQueueFixedWords = 224;
bool bs128_queue_applicable(const CodewordSet& rows, const CodewordSet& cols);
hipError_t launch_extend_gf8_bs128_queue(const QueuePlan& p, hipStream_t st);


#ifdef RSM_DIAG
// ---------------------------------------------------------------------------
// Diagnostic / A-B kernels: compiled only into librsmt2d_hip_diag.so (make diag),
// never into the product library.
// ---------------------------------------------------------------------------
// Two independent codeword batches in one persistent launch (kernels_gf8_bs.hip,
// encode_gf8_bs128p_kernel): the row pass of one batch of squares and the column
// pass of another, sets interleaved 1 : 2 when nb == 2 * na so that every CU mixes
// the compute-heavier row sets with the memory-heavier column sets.
struct DualPlan {
    CodewordSet a, b;
    uint32_t na, nb;  // sets of a, of b
};

hipError_t launch_encode_gf8_bs128_dual(const DualPlan& p, hipStream_t st);
// A-B kernel variant of the bit-sliced encode: 40 production, 0/8/24/56 A-B
// variants, 2 = no arithmetic, 4 = no global memory (wrong output by design)
void set_bs128_diag_mode(int mode, int rev_col, int xcd);
// per-set phase timeline of the half-split queue kernel (device buffer of
// grid * kTraceSets * kTraceWords words; nullptr: off)
constexpr uint32_t kTraceSets = 256, kTraceWords = 14;
void set_bs128_diag_trace(uint32_t* d);
void set_bs128_diag_row_mode(int mode);
#endif

}  // namespace rsm
