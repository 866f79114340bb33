/*
 * rsmt2d_hip.h -- C ABI of the MI355X-native 2D Reed-Solomon EDS engine.
 *
 * Drop-in boundary for celestiaorg/rsmt2d's hot path: the Codec plugin
 * (codecs.go:14-30, implemented by LeoRSCodec in leopard.go:16-103) and the
 * two-dimensional schedule / crossword solver built on it
 * (extendeddatasquare.go:50-243, extendeddatacrossword.go:74-502).
 * Everything is plain pointers and sizes so a cgo shim can bind
 * it directly; no call ever aborts or throws across the ABI.
 *
 * Return codes: 0 on success, a negative RSM_E* code on failure;
 * rsm_last_error() gives a thread-local human-readable message.
 */
#ifndef RSMT2D_HIP_H
#define RSMT2D_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSM_OK 0
#define RSM_EINVAL (-1)        /* bad argument */
#define RSM_ESHARESIZE (-2)    /* share size not a multiple of 64 (leopard.go:92-99) */
#define RSM_ETOOFEW (-3)       /* Decode: fewer than k of 2k shares present */
#define RSM_ESHAPE (-4)        /* non-square count, uneven shares, odd EDS width, > MaxChunks */
#define RSM_EDEVICE (-5)       /* HIP runtime failure / no GPU: never a silent CPU fallback */
#define RSM_ENOMEM (-6)
#define RSM_EUNSUPPORTED (-7)  /* configuration this build does not implement (2k > 65536,
                                   as klauspost rejects it; device roots beyond their widths) */
#define RSM_EUNREPAIRABLE (-8) /* ErrUnrepairableDataSquare (extendeddatacrossword.go:37) */
#define RSM_EBYZANTINE (-9)    /* ErrByzantineData (extendeddatacrossword.go:42-58) */
#define RSM_ECELL (-10)        /* SetCell on a non-nil cell or wrong size (datasquare.go:341-353) */
#define RSM_ETREE (-11)        /* tree callback error / root of an incomplete vector */

#define RSM_AXIS_ROW 0 /* rsmt2d.Row (extendeddatacrossword.go:15-18) */
#define RSM_AXIS_COL 1 /* rsmt2d.Col */

typedef struct rsm_ctx rsm_ctx;
typedef struct rsm_eds rsm_eds;

/* ---- context --------------------------------------------------------------- */
/* One context per GPU (device ordinal).  Thread-safe: rsmt2d calls the Codec from
 * up to 2k goroutines at once (extendeddatasquare.go:186-224); each Codec /
 * host-memory call takes its own stream and staging buffers from the context's
 * pool (up to 32 in flight, further callers wait), device scratch belongs to the
 * stream it is used on, and every call selects the context's device on the
 * calling thread (cgo moves goroutines between OS threads). */
int rsm_ctx_create(int device, rsm_ctx** out);
void rsm_ctx_destroy(rsm_ctx* ctx);
int rsm_ctx_device(const rsm_ctx* ctx);
/* Throughput tuning for several extensions in flight on different streams: cap the
 * persistent grid (CUs) of this context's GF(2^8) M = 128 row pass (pass 0) or
 * column pass (pass 1); the single-launch queue extension (both passes) takes the
 * pass-0 cap; 0 = all CUs (default).  *previous (may be NULL) receives the old cap.
 * Results never depend on it. */
int rsm_ctx_set_pass_grid(rsm_ctx* ctx, int pass, int cus, int* previous);
/* Latency tuning: GF(2^8) extensions of up to `squares` squares per call with
 * 65 <= k <= 128 run in the latency form (two launches of the split byte-table
 * encoder over every CU) instead of the single queue-driven launch; 0 = always the
 * queue launch.  Default 12.  With 9 <= k <= 64 the latency form takes up to
 * max(squares, 64) squares per call (0: never) instead of the one-wave-per-codeword
 * byte-table passes.  *previous (may be NULL) receives the old value.  Results
 * never depend on it. */
int rsm_ctx_set_split_max(rsm_ctx* ctx, int squares, int* previous);
/* Test hook: the single-pass kernels address each half of a codeword with 32-bit
 * offsets, so codewords whose halves span more than offset_limit bytes (default 2^31:
 * columns of squares over 4 GiB) run on the wide forms (64-bit per-symbol bases), and
 * GF(2^16) work arrays get at most work_budget bytes per stream (default 1 GiB; wider
 * shares run as byte slabs).  Lowering them sends small shapes down those paths so
 * their parity can be tested without 4 GiB squares; 0 restores a default.  Results
 * never depend on them. */
int rsm_ctx_set_limits(rsm_ctx* ctx, uint64_t offset_limit, uint64_t work_budget);
const char* rsm_last_error(void);
const char* rsm_version(void);
int rsm_device_count(void);

/* ---- Codec (codecs.go:14-30; LeoRSCodec leopard.go:16-103) ------------------- */
/* Name() -- "Leopard" (codecs.go:11): EDS.Equals and JSON compare codec names. */
const char* rsm_codec_name(void);
/* MaxChunks() -- 32768 * 32768 (leopard.go:76-84). */
int64_t rsm_codec_max_chunks(void);
/* ValidateChunkSize(shareSize) -- RSM_ESHARESIZE unless a multiple of 64. */
int rsm_codec_validate_chunk_size(int64_t share_size);
/* 8 when 2k <= 256 (GF(2^8)), else 16 (GF(2^16)) -- codecs.go:6-10. */
int rsm_codec_field_bits(uint32_t k);
/* Encode(data) (leopard.go:28-45): k complete shares of share_size bytes in host
 * memory -> k parity shares written to parity[0..k). */
int rsm_encode(rsm_ctx* ctx, const uint8_t* const* data, uint32_t k, uint32_t share_size,
               uint8_t* const* parity);
/* Decode(data) (leopard.go:51-59, klauspost Reconstruct): n = 2k slots; slot i is
 * present iff present[i] != 0; every missing slot's buffer shares[i] (caller
 * allocated, share_size bytes) is filled.  RSM_ETOOFEW if fewer than k present;
 * all present is a no-op. */
int rsm_decode(rsm_ctx* ctx, uint8_t* const* shares, const uint8_t* present, uint32_t n,
               uint32_t share_size);

/* ---- batched 2D extension (erasureExtendSquare, extendeddatasquare.go:154-227) -- */
/* Host memory: ods = k*k shares row-major, eds = (2k)^2 shares row-major.  Only
 * Q1, Q2, Q3 cross PCIe back; Q0 of eds is filled from ods on the host. */
int rsm_extend_square(rsm_ctx* ctx, const uint8_t* ods, uint32_t k, uint32_t share_size,
                      uint8_t* eds);
/* Host memory, in place: the top-left quadrant of eds already holds the ODS (the
 * cgo shim gathers the [][]byte shares straight into a pinned EDS arena from
 * rsm_host_alloc); Q1..Q3 are written around it. */
int rsm_extend_square_inplace_host(rsm_ctx* ctx, uint8_t* eds, uint32_t k, uint32_t share_size);
/* Host memory, `count` consecutive squares (ods: [count][k][k][S], eds:
 * [count][2k][2k][S]): H2D, extension and D2H of different squares overlap on
 * three streams.  Pinned buffers (rsm_host_alloc) make every copy an async DMA. */
int rsm_extend_squares_host(rsm_ctx* ctx, const uint8_t* ods, uint32_t k, uint32_t share_size, uint32_t count,
                            uint8_t* eds);
/* Pinned (page-locked) host memory for the arenas above. */
int rsm_host_alloc(rsm_ctx* ctx, uint64_t bytes, void** out);
int rsm_host_free(rsm_ctx* ctx, void* p);
/* Device-resident, in place: d_eds holds `count` consecutive [2k][2k][S] squares
 * whose top-left quadrant already holds the ODS (the EDS aliases the ODS, as in
 * ComputeExtendedDataSquare).  Enqueued on `stream` (a hipStream_t of this
 * library's HIP runtime; NULL = the context stream); asynchronous.  With
 * 65 <= k <= 128, batches of more than rsm_ctx_set_split_max squares run both passes
 * as ONE queue-driven launch, smaller batches (a single square included) as two
 * latency-form launches over every CU.  The queue launch's bounded waits cannot time
 * out short of a hardware fault, and if one did, the stream's next rsm_stream_check
 * (rsm_sync for the context stream), its rsm_stream_destroy or the next extension on
 * that stream returns RSM_EDEVICE. */
int rsm_extend_squares_dev(rsm_ctx* ctx, void* d_eds, uint32_t k, uint32_t share_size, uint32_t count,
                           void* stream);
/* One phase of the above: phase 1 = row pass (Q0 -> Q1), phase 2 = column pass
 * ([Q0|Q1] -> [Q2|Q3]), 3 = both; for per-kernel timing/profiling.  Asynchronous. */
int rsm_extend_squares_phase_dev(rsm_ctx* ctx, void* d_eds, uint32_t k, uint32_t share_size,
                                 uint32_t count, int phase, void* stream);
/* Rows [row0, row0+nrows) / columns [col0, col0+ncols) of one in-place
 * [2k][2k][S] square: the per-GPU units of the row-sharded multi-GPU schedule
 * (rows of the top half on each GPU, an all-gather of [Q0|Q1], then each GPU's
 * column slice).  Asynchronous on `stream` (NULL = context stream). */
int rsm_extend_rows_dev(rsm_ctx* ctx, void* d_eds, uint32_t k, uint32_t share_size, uint32_t row0,
                        uint32_t nrows, void* stream);
int rsm_extend_cols_dev(rsm_ctx* ctx, void* d_eds, uint32_t k, uint32_t share_size, uint32_t col0,
                        uint32_t ncols, void* stream);
/* The row pass of rows [row0, row0+nrows) (as rsm_extend_rows_dev) that also leaves the
 * extended rows split into `nblocks` column blocks of 2k/nblocks columns each: block h
 * at d_blocks + h*nrows*(2k/nblocks)*S, row pitch (2k/nblocks)*S -- the send buffer of
 * the all-to-all multi-GPU schedule (rank h receives block h), with no copy pass where the
 * encoder stores the blocks itself (GF(2^16), k <= 512, k and the block width multiples
 * of 32; other shapes: the row pass, then strided device copies).  Asynchronous. */
int rsm_extend_rows_blocks_dev(rsm_ctx* ctx, void* d_eds, uint32_t k, uint32_t share_size, uint32_t row0,
                               uint32_t nrows, void* d_blocks, uint32_t nblocks, void* stream);
/* Generic device batch of `count` codewords (k data shares -> k parity shares each,
 * the Encode of leopard.go:28-45 for every codeword): data share e of codeword q is
 * at d_in + q*cw_stride + e*share_stride, its parity share e is written at
 * d_out + q*cw_stride + e*share_stride (byte strides).  Used for the compact
 * column slices of the all-to-all multi-GPU schedule.  Asynchronous. */
int rsm_encode_batch_dev(rsm_ctx* ctx, const void* d_in, void* d_out, uint32_t k, uint32_t share_size,
                         uint32_t count, uint64_t cw_stride, uint64_t share_stride, void* stream);
/* RowRoots()/ColRoots() with DefaultTree (datasquare.go:218-327, tree.go:32-59) of a
 * complete device-resident [width][width][share_size] square, on the GPU:
 * d_roots (device) receives 2*width*32 bytes, the row roots then the column roots.
 * width <= 2048.  Asynchronous on `stream`. */
int rsm_roots_dev(rsm_ctx* ctx, const void* d_eds, uint32_t width, uint32_t share_size, void* d_roots,
                  void* stream);
/* rsm_roots_dev over `count` consecutive squares ([count][width][width][share_size],
 * as rsm_extend_squares_dev lays them out): d_roots receives [count][2][width][32]
 * bytes.  One launch pair for the batch (BenchmarkExtensionWithRoots,
 * extendeddatasquare_test.go:309-334, over many squares). */
int rsm_roots_squares_dev(rsm_ctx* ctx, const void* d_eds, uint32_t width, uint32_t share_size, uint32_t count,
                          void* d_roots, void* stream);
/* Device-resident batched reconstruct of whole rows (axis 0) or columns (axis 1)
 * of one [2k][2k][S] square: d_presence is one byte per cell, d_indices the
 * vectors to rebuild (each must have >= k cells present).  Asynchronous. */
int rsm_decode_vectors_dev(rsm_ctx* ctx, void* d_eds, const uint8_t* d_presence, uint32_t k,
                           uint32_t share_size, int axis, const uint32_t* d_indices, uint32_t count,
                           void* stream);

/* ---- one square over several GPUs of a node (config 5) --------------------------- */
/* One process drives G GPUs: a context per device plus an RCCL clique
 * (ncclCommInitAll).  GPU g owns Q0 rows [g k/G, (g+1) k/G): it row-encodes them,
 * the top half is exchanged over xGMI, and GPU g column-encodes its 2k/G columns
 * (SURVEY.md section 8(e)).  Kernels and collectives of a GPU are ordered on that
 * GPU's context stream -- no host synchronisation between the steps. */
typedef struct rsm_multi rsm_multi;
#define RSM_SCHED_ALLGATHER 0 /* north_star: all-gather of the row-encoded top half */
#define RSM_SCHED_ALLTOALL 1  /* grouped send/recv: each GPU receives only its column slice */
int rsm_multi_create(const int* devices, int n, rsm_multi** out);
void rsm_multi_destroy(rsm_multi* m);
int rsm_multi_size(const rsm_multi* m);
/* The per-GPU context (device memory, streams) of GPU i of the clique. */
rsm_ctx* rsm_multi_context(rsm_multi* m, int i);
/* ComputeExtendedDataSquare (extendeddatasquare.go:50-77) of ONE k x k square from
 * host memory (ods k*k*S row-major -> eds (2k)^2*S row-major) over the clique;
 * k must be a multiple of G.  Synchronous. */
int rsm_multi_extend_square(rsm_multi* m, const uint8_t* ods, uint32_t k, uint32_t share_size, uint8_t* eds,
                            int schedule);
/* Pinned host memory for the multi-GPU host path (hipHostMalloc, portable: every GPU
 * of the clique DMAs it directly). */
int rsm_multi_host_alloc(rsm_multi* m, uint64_t bytes, void** p);
int rsm_multi_host_free(rsm_multi* m, void* p);
/* In-place host form (what the cgo ComputeExtendedDataSquare fast path calls on a
 * pinned arena): eds is (2k)^2*S row-major whose top-left k x k quadrant already
 * holds the ODS (Go's EDS aliases its input); only Q1, Q2, Q3 are written.  From
 * rsm_multi_host_alloc memory every copy is one DMA per GPU (Q0 rows up, Q1 rows and
 * the bottom-half column slice down; the Q1 download overlaps the exchange and the
 * column pass); pageable memory also works (staged by HIP).  Synchronous. */
int rsm_multi_extend_square_inplace(rsm_multi* m, uint8_t* eds, uint32_t k, uint32_t share_size, int schedule);
/* Device-resident form: d_eds[g] is a full [2k][2k][S] buffer on GPU g holding Q0
 * rows of shard g; afterwards it holds shard g's rows of the top half and the bottom
 * half [Q2|Q3] of its column slice [g 2k/G, (g+1) 2k/G) (all-gather: the whole top half
 * as well; all-to-all over the copy passes -- GF(2^8), k > 512 or blocks under 32 rows or
 * columns -- also the other shards' rows of its column slice; the copy-free all-to-all
 * leaves those in the clique's receive staging, where its column pass read them).
 * Asynchronous on the context streams; rsm_multi_sync waits. */
int rsm_multi_extend_dev(rsm_multi* m, void* const* d_eds, uint32_t k, uint32_t share_size, int schedule);
int rsm_multi_sync(rsm_multi* m);

/* ---- device memory / timing on the context's HIP runtime ---------------------- */
/* The context's stream (hipStream_t); the *_dev calls above use it when their
 * stream argument is NULL. */
void* rsm_ctx_stream(rsm_ctx* ctx);
int rsm_dev_alloc(rsm_ctx* ctx, uint64_t bytes, void** out);
int rsm_dev_free(rsm_ctx* ctx, void* p);
/* kind: 0 host->device, 1 device->host, 2 device->device; synchronous. */
int rsm_memcpy(rsm_ctx* ctx, void* dst, const void* src, uint64_t bytes, int kind);
/* SplitMix64 byte stream (seeded synthetic shares), asynchronous on the ctx stream. */
int rsm_dev_fill_random(rsm_ctx* ctx, void* d, uint64_t bytes, uint64_t seed);
int rsm_sync(rsm_ctx* ctx);
/* *equal = 1 iff the device buffers a and b (bytes a multiple of 16, both pointers
 * 16-byte aligned: the kernel reads them as uint4; RSM_EINVAL otherwise) are equal,
 * compared on the device (a kernel on `stream`, NULL = context stream); synchronous. */
int rsm_dev_equal(rsm_ctx* ctx, const void* a, const void* b, uint64_t bytes, void* stream, int* equal);
/* Extra HIP streams on the context's device, for callers that pipeline independent
 * batches (e.g. step n's column pass beside step n+1's row pass on another
 * stream).  Each stream owns its device scratch (GF(2^16) work arrays, leaf
 * digests), released by rsm_stream_destroy. */
int rsm_stream_create(rsm_ctx* ctx, void** out);
int rsm_stream_destroy(rsm_ctx* ctx, void* stream);
int rsm_stream_sync(void* stream);
/* Waits for `stream` (NULL = context stream) and returns RSM_EDEVICE (clearing it)
 * if a queue-driven extension on it reported a stuck wait; rsm_sync does the same
 * for the context stream only. */
int rsm_stream_check(rsm_ctx* ctx, void* stream);
/* HIP events on the context's device, for timing launches inside a caller's loop
 * (NULL stream = context stream).  rsm_event_elapsed_ms waits for `end`. */
int rsm_event_create(rsm_ctx* ctx, void** out);
int rsm_event_destroy(void* ev);
int rsm_event_record(rsm_ctx* ctx, void* ev, void* stream);
int rsm_event_elapsed_ms(void* start, void* end, float* ms);
/* Event-timed extension of `count` in-place squares on the ctx stream, averaged
 * over `reps`: row pass and column pass (the two launches of one extension) and
 * `step` = their sum, in milliseconds. */
int rsm_time_extend(rsm_ctx* ctx, void* d_eds, uint32_t k, uint32_t share_size, uint32_t count,
                    uint32_t reps, float* row_ms, float* col_ms, float* step_ms);

/* ---- Tree plugin (tree.go:11-28) ------------------------------------------------ */
/* Computes the root of one row/column: Push(leaves[0..n)) then Root().  Writes
 * the root to root_out (capacity *root_len on entry), sets *root_len, returns 0;
 * non-zero = tree error (treated as byzantine by Repair, as in the reference). */
typedef int (*rsm_tree_root_fn)(void* user, int axis, uint32_t index, const uint8_t* const* leaves,
                                uint32_t n_leaves, uint32_t leaf_size, uint8_t* root_out,
                                uint32_t* root_len);
/* NewDefaultTree restatement: celestiaorg/merkletree over SHA-256 (leaf
 * H(0x00||d), node H(0x01||l||r)).  Passed as NULL tree_fn below. */
int rsm_default_tree_root(void* user, int axis, uint32_t index, const uint8_t* const* leaves,
                          uint32_t n_leaves, uint32_t leaf_size, uint8_t* root_out,
                          uint32_t* root_len);

/* Namespaced Merkle tree (celestiaorg/nmt v0.24.3) as rsmt2d's erasured-NMT
 * wrappers push it (nmtwrapper_test.go:94-120; the buffered pool tree
 * nmtbuffered_tree_test.go:118-152 pushes identically): leaf i of row/column
 * `index` is pushed as ns || share with ns = share[:namespace_size] when
 * i < square_size and index < square_size (quadrant 0), else the parity namespace
 * 0xFF..; root = minNs || maxNs || SHA-256 digest (2*namespace_size + 32 bytes).
 * Tree errors (push order, too short, past the square) return RSM_ETREE. */
typedef struct {
    uint32_t namespace_size;       /* nmt.NamespaceIDSize (Celestia: 29) */
    uint32_t ignore_max_namespace; /* nmt.IgnoreMaxNamespace (the wrappers force 1) */
    uint32_t square_size;          /* ODS width k the wrapper was built for */
} rsm_nmt_params;
/* Tree plugin form: pass rsm_nmt_tree_root with user = (rsm_nmt_params*) as the
 * tree_fn of rsm_eds_roots / rsm_eds_repair: complete squares then take the
 * device path (kernels_nmt.hip), anything else the host restatement. */
int rsm_nmt_tree_root(void* user, int axis, uint32_t index, const uint8_t* const* leaves, uint32_t n_leaves,
                      uint32_t leaf_size, uint8_t* root_out, uint32_t* root_len);
/* Device NMT roots of a complete device-resident [width][width][share_size]
 * square: d_roots receives 2*width roots of 2*namespace_size + 32 bytes (rows,
 * then columns); d_status (device, may be NULL) 2*width uint32, non-zero where
 * that tree fails (push order).  namespace_size <= 32, width <= 1024.
 * Asynchronous on `stream`. */
int rsm_nmt_roots_dev(rsm_ctx* ctx, const void* d_eds, uint32_t width, uint32_t share_size,
                      const rsm_nmt_params* params, void* d_roots, void* d_status, void* stream);
/* The same for `count` consecutive device squares in one launch pair (a block's
 * worth of squares: the trees of one square alone leave most CUs idle); d_roots and
 * d_status hold 2*width entries per square, square after square. */
int rsm_nmt_roots_squares_dev(rsm_ctx* ctx, const void* d_eds, uint32_t width, uint32_t share_size, uint32_t count,
                              const rsm_nmt_params* params, void* d_roots, void* d_status, void* stream);

/* ---- share inclusion proofs ------------------------------------------------------ */
/* A share with its Merkle proof against the row or column root: what a node serving
 * data-availability samples hands out, and the "Merkle proof for each share" a fraud
 * proof carries (extendeddatacrossword_test.go:19-21).  The tree is selected as in
 * rsm_eds_roots: nmt == NULL is the DefaultTree, else the erasured NMT.
 *
 * The tree over the W leaves of a vector, by levels: node (l, j) covers leaves
 * [j 2^l, min((j+1) 2^l, W)); level l has ceil(W / 2^l) nodes and an unpaired last
 * node is carried up unchanged (the RFC 6962 split, the merkletree stack).  The proof
 * of leaf p lists, for l = 0 .. L-1 (L = ceil(log2 W), 0 for W = 1) and j = p >> l,
 * node (l, j ^ 1) where j ^ 1 is below the level's node count -- bottom-up, the order
 * merkletree.Prove() returns after the leaf (datasquare_test.go:514-537).
 * Node bytes: DefaultTree the 32-byte digest; NMT min || max || digest
 * (2 * namespace_size + 32), as roots.
 * Proof record, fixed stride rsm_proof_record_bytes = 8 + L * node_len:
 *   uint32 n_nodes | uint32 right_mask (bit i: node i is the RIGHT operand of its
 *   parent hash) | n_nodes nodes, bottom-up | zeros                                  */
typedef struct {
    uint32_t square; /* square of a batch */
    uint32_t axis;   /* RSM_AXIS_ROW / RSM_AXIS_COL */
    uint32_t index;  /* row or column */
    uint32_t pos;    /* leaf of that vector */
} rsm_sample;
/* Bytes of the node store of `count` squares (opaque to callers); 0 for shapes the
 * device trees do not take (the limits of rsm_roots_dev / rsm_nmt_roots_dev). */
uint64_t rsm_proof_nodes_bytes(uint32_t width, const rsm_nmt_params* nmt, uint32_t count);
/* Bytes of one proof record (any width >= 1; 0 for width 0 or a namespace size 0). */
uint32_t rsm_proof_record_bytes(uint32_t width, const rsm_nmt_params* nmt);
/* Builds the node store of `count` consecutive complete device squares: every node of
 * their 2 * width trees, into d_nodes (device, rsm_proof_nodes_bytes, 16-byte aligned;
 * no other scratch).  d_roots / d_status (device, nullable) receive what
 * rsm_roots_squares_dev / rsm_nmt_roots_squares_dev write (DefaultTree statuses: 0).
 * RSM_EUNSUPPORTED beyond those calls' limits.  Asynchronous on `stream`. */
int rsm_proof_nodes_dev(rsm_ctx* ctx, const void* d_eds, uint32_t width, uint32_t share_size, uint32_t count,
                        const rsm_nmt_params* nmt, void* d_nodes, void* d_roots, void* d_status, void* stream);
/* n proof records out of a node store: d_records (device) receives n records;
 * d_shares (device, nullable, 16-byte aligned; needs d_eds, the squares the store was
 * built from) the n sampled shares, [n][share_size].  `samples` is HOST memory,
 * validated before anything is enqueued (RSM_EINVAL names the first sample with
 * square >= count, axis > 1, index >= width or pos >= width) and copied before the call
 * returns.  The records are written asynchronously on `stream`. */
int rsm_proofs_dev(rsm_ctx* ctx, const void* d_nodes, const void* d_eds, uint32_t width, uint32_t share_size,
                   uint32_t count, const rsm_nmt_params* nmt, const rsm_sample* samples, uint32_t n, void* d_records,
                   void* d_shares, void* stream);
/* Host restatements (merkle.cpp), any n_leaves >= 1: the proof record of leaf `pos`
 * into record_out (rsm_proof_record_bytes(n_leaves, ..)) and the root into root_out
 * (nullable; 32 / 2 * namespace_size + 32 bytes).  The NMT form applies the wrapper's
 * rules as rsm_nmt_tree_root does (`index` decides quadrant 0; RSM_ETREE on push
 * order, sibling order, a vector past the square, data shorter than a namespace). */
int rsm_default_tree_prove(const uint8_t* const* leaves, uint32_t n_leaves, uint32_t leaf_size, uint32_t pos,
                           uint8_t* record_out, uint8_t* root_out);
int rsm_nmt_tree_prove(const rsm_nmt_params* params, uint32_t index, const uint8_t* const* leaves, uint32_t n_leaves,
                       uint32_t leaf_size, uint32_t pos, uint8_t* record_out, uint8_t* root_out);

/* ---- proof verification ------------------------------------------------------------ */
/* The receiving side: does this share, at this position, belong under this committed
 * row or column root?  One status word per sample; the first condition that applies
 * wins. */
#define RSM_PROOF_OK 0        /* the fold equals the committed root */
#define RSM_PROOF_MALFORMED 1 /* n_nodes or right_mask differs from what (width, pos) dictates */
#define RSM_PROOF_ORDER 2     /* NMT only: a fold step has right.min < left.max (HashNode's error) */
#define RSM_PROOF_ROOT 3      /* the fold completed but differs from the root (NMT: all of
                                 min || max || digest is compared) */
#define RSM_PROOF_OCCUPIED 4  /* rsm_eds_import_samples only: verified, but the cell is not nil */
/* Two rules are part of the contract.  The position is bound: the verifier derives the
 * node count and every operand side from (width, pos) -- level l contributes when
 * ((pos >> l) ^ 1) < ceil(width / 2^l), its sibling is the right operand when pos >> l
 * is even -- and only compares the record's header with them, so a valid proof of leaf p
 * presented as leaf p' does not verify.  No address depends on record or share contents:
 * the fold runs over the derived count (<= L), whatever the header says, and record
 * bytes past the derived nodes are never read.
 * The leaf is built as the trees build it: DefaultTree H(0x00 || share); NMT
 * ns || ns || H(0x00 || ns || share) with ns = share[:namespace_size] when
 * index < square_size and pos < square_size, else 0xFF..; ignore_max_namespace is
 * honoured in the fold as in HashNode.
 *
 * Device form: n samples in one launch.  d_shares [n][share_size] (16-byte aligned) and
 * d_records [n][rsm_proof_record_bytes] (any alignment) as rsm_proofs_dev writes them,
 * d_roots [count][2][width][32 or 2 * namespace_size + 32] as rsm_roots_squares_dev /
 * rsm_nmt_roots_squares_dev write them, d_status [n] uint32.  Sample i is checked
 * against root (square, axis, index) of d_roots.  `samples` is HOST memory, validated
 * and copied as in rsm_proofs_dev (n <= 2^24).  No tree is built, so the limits are not
 * the root kernels': 1 <= width <= 65536, namespace_size 1..32, share_size a multiple of
 * 64 (NMT: >= namespace_size, else RSM_ETREE).  n == 0 or count == 0 launches nothing.
 * Asynchronous on `stream`. */
int rsm_proofs_verify_dev(rsm_ctx* ctx, const void* d_shares, const void* d_records, const void* d_roots,
                          uint32_t width, uint32_t share_size, uint32_t count, const rsm_nmt_params* nmt,
                          const rsm_sample* samples, uint32_t n, void* d_status, void* stream);
/* Host restatements (merkle.cpp), any n_leaves >= 1, the same semantics and status
 * words.  The return value is an argument error only (RSM_EINVAL; RSM_ETREE for a share
 * shorter than the namespace); a proof that fails returns RSM_OK with *status != 0. */
int rsm_default_tree_verify(const uint8_t* share, uint32_t share_size, uint32_t n_leaves, uint32_t pos,
                            const uint8_t* record, const uint8_t* root, uint32_t* status);
int rsm_nmt_tree_verify(const rsm_nmt_params* params, uint32_t index, const uint8_t* share, uint32_t share_size,
                        uint32_t n_leaves, uint32_t pos, const uint8_t* record, const uint8_t* root, uint32_t* status);

/* ---- data root --------------------------------------------------------------------- */
/* What commits the roots: the one 32-byte hash a block header carries.  It is the
 * RFC 6962 Merkle root over rowRoots ++ colRoots (tendermint HashFromByteSlices,
 * Celestia's DataAvailabilityHeader.Hash(); the roots nmtwrapper_test.go:79 speaks of).
 *
 * The tree is the level picture of "share inclusion proofs" above over N = 2 * width
 * leaves: leaf t is the root bytes of tree t as the roots calls lay them out (rows
 * 0 .. W-1, then columns W .. 2W-1), root_len = 32 (DefaultTree) or
 * 2 * namespace_size + 32 (NMT) bytes each.
 *   leaf hash  SHA-256(0x00 || root bytes)
 *   inner node SHA-256(0x01 || l || r)
 *   an unpaired last node is carried up unchanged
 * which equals RFC 6962's recursive split at the largest power of two below n.  Every
 * node is a 32-byte digest at every level, over NMT roots too.  The proof record of a
 * root keeps the share proofs' format with node_len = 32 and L2 = ceil(log2(2 * width))
 * levels: uint32 n_nodes | uint32 right_mask | nodes bottom-up | zeros, fixed stride
 * rsm_data_root_record_bytes = 8 + L2 * 32. */
typedef struct {
    uint32_t square; /* square of a batch */
    uint32_t axis;   /* RSM_AXIS_ROW / RSM_AXIS_COL */
    uint32_t index;  /* row or column: leaf axis * width + index of the data-root tree */
} rsm_root_ref;
/* Bytes of one root proof record (any width >= 1; 0 for width 0). */
uint32_t rsm_data_root_record_bytes(uint32_t width);
/* Bytes of the node store of `count` data-root trees (opaque to callers: the leaf digests
 * and every upper node); 0 beyond the build's width limit (1 <= width <= 2048). */
uint64_t rsm_data_root_nodes_bytes(uint32_t width, uint32_t count);
/* The data roots of `count` squares: d_roots (device, any alignment) is
 * [count][2][width][root_len], exactly as rsm_roots_squares_dev /
 * rsm_nmt_roots_squares_dev / rsm_proof_nodes_dev write it; d_data_roots (device, any
 * alignment) receives [count][32]; d_nodes (device, nullable, 16-byte aligned,
 * rsm_data_root_nodes_bytes) the node store.  root_len is any value 32 .. 96
 * (RSM_EINVAL otherwise): the leaf is the raw bytes, so the call does not need to know
 * which tree made them.  1 <= width <= 2048, every width for which device roots exist;
 * beyond that RSM_EUNSUPPORTED.  count == 0 launches nothing.  No scratch beyond d_nodes.
 * Asynchronous on `stream`. */
int rsm_data_roots_dev(rsm_ctx* ctx, const void* d_roots, uint32_t width, uint32_t root_len, uint32_t count,
                       void* d_data_roots, void* d_nodes, void* stream);
/* n root proof records out of a node store: record i (d_records: device, any alignment,
 * stride rsm_data_root_record_bytes) is the proof of leaf axis * width + index of square
 * `square`.  `refs` is HOST memory, validated before anything is enqueued (RSM_EINVAL
 * names the first ref with square >= count, axis > 1 or index >= width) and copied before
 * the call returns (n <= 2^24).  The records are written asynchronously on `stream`. */
int rsm_root_proofs_dev(rsm_ctx* ctx, const void* d_nodes, uint32_t width, uint32_t count, const rsm_root_ref* refs,
                        uint32_t n, void* d_records, void* stream);
/* The chained verifier: share -> row/column root -> data root, with no root table.
 * Sample i takes share i and record i as in rsm_proofs_verify_dev, and root record i
 * (d_root_records: stride rsm_data_root_record_bytes(width), any alignment); it is
 * checked against d_data_roots[square] (32 bytes each, any alignment).  The lane folds
 * the share proof to a candidate root (DefaultTree: the digest; NMT: min || max ||
 * digest), hashes that candidate as a leaf of the data-root tree, folds the root record
 * and compares with the data root.  Status words, the first that applies:
 *   RSM_PROOF_MALFORMED  the share record's header differs from what (width, pos) dictates
 *   RSM_PROOF_MALFORMED  the root record's header differs from what
 *                        (2 * width, axis * width + index) dictates
 *   RSM_PROOF_ORDER      NMT share fold, as in rsm_proofs_verify_dev
 *   RSM_PROOF_ROOT       the final digest differs from the data root
 *   RSM_PROOF_OK
 * Both header checks come before any hashing.  The contract of rsm_proofs_verify_dev
 * holds for both records: positions are bound, counts and operand sides are derived and
 * never read, bytes past the derived nodes are never read, no address depends on record
 * or share contents, and exactly one status word is written per sample.  Limits and
 * argument errors are those of rsm_proofs_verify_dev (no tree is built): 1 <= width <=
 * 65536, namespace_size 1..32, share_size a multiple of 64 (NMT: >= namespace_size, else
 * RSM_ETREE), n <= 2^24; n == 0 or count == 0 launches nothing.  Asynchronous on
 * `stream`. */
int rsm_proofs_verify_data_root_dev(rsm_ctx* ctx, const void* d_shares, const void* d_records, const void* d_root_records,
                                    const void* d_data_roots, uint32_t width, uint32_t share_size, uint32_t count,
                                    const rsm_nmt_params* nmt, const rsm_sample* samples, uint32_t n, void* d_status,
                                    void* stream);
/* Host restatements (merkle.cpp), any width >= 1.  roots: [2][width][root_len], root_len
 * 1 .. 96 here (the host hashes any length).  rsm_data_root: the data root.
 * rsm_data_root_prove: the record of leaf axis * width + index into record_out
 * (rsm_data_root_record_bytes(width)).  rsm_data_root_verify: root_bytes (root_len bytes)
 * as that leaf under data_root; *status MALFORMED / ROOT / OK.
 * rsm_sample_verify_data_root: the chained verifier for one sample (its `square` is not
 * used), nmt == NULL the DefaultTree; the same semantics and status words as the device
 * form.  The return value is an argument error only (RSM_EINVAL; RSM_ETREE for a share
 * shorter than the namespace). */
int rsm_data_root(const uint8_t* roots, uint32_t width, uint32_t root_len, uint8_t* out);
int rsm_data_root_prove(const uint8_t* roots, uint32_t width, uint32_t root_len, uint32_t axis, uint32_t index,
                        uint8_t* record_out);
int rsm_data_root_verify(const uint8_t* root_bytes, uint32_t root_len, uint32_t width, uint32_t axis, uint32_t index,
                         const uint8_t* record, const uint8_t* data_root, uint32_t* status);
int rsm_sample_verify_data_root(const rsm_nmt_params* nmt, uint32_t width, const rsm_sample* sample, const uint8_t* share,
                                uint32_t share_size, const uint8_t* record, const uint8_t* root_record,
                                const uint8_t* data_root, uint32_t* status);

/* ---- namespace proofs -------------------------------------------------------------- */
/* "Every share of namespace nid in this row (or column), with proof that these are all
 * of them": nmt's ProveNamespace / VerifyNamespace (celestia-node's GetSharesByNamespace
 * asks it of every row), restated in the level picture above.  NMT only.
 *
 * Vector: row (axis 0) or column (axis 1) `index` of a [W][W][S] square, W = 2 *
 * square_size.  Leaf p carries the namespace the wrapper pushes: share[:namespace_size]
 * when p < square_size and index < square_size, else 0xFF..; namespaces compare as
 * big-endian byte strings.  Kind of the answer, the first rule that applies: */
#define RSM_NS_EMPTY 0     /* nid < root.min or nid > root.max (the root as stored, so
                              ignore_max_namespace is applied: 0xFF.. is EMPTY in a quadrant-0
                              row).  start = end = 0, no nodes, no shares */
#define RSM_NS_INCLUSION 1 /* start = first leaf >= nid, end = first leaf > nid, start < end:
                              the range proof of [start, end); shares = leaves start .. end-1 */
#define RSM_NS_ABSENCE 2   /* no such leaf though nid lies in the root's range: the range
                              proof of [start, start + 1), the first leaf above nid, whose node
                              ns || ns || digest the record carries; end = start + 1, no shares */
#define RSM_NS_TREE 3      /* device only, checked first: the tree's status word is non-zero
                              (push order), nothing is searched.  start = end = 0, no nodes */
/* Range proof of [start, end), from (W, start, end) alone: with a = start, last = end - 1,
 * level l = 0 .. L-1 gives the left node (l, a - 1) when a is odd and the right node
 * (l, last + 1) when last is even and last + 1 < ceil(W / 2^l); then a >>= 1, last >>= 1.
 * Record order: the left nodes from the top level down, then the right nodes from the
 * bottom level up (nmt's Proof.Nodes: an in-order walk of the RFC 6962 split).
 * Record, little-endian, fixed stride rsm_ns_record_bytes = 16 + (2L + 1) * node_len,
 * node_len = 2 * namespace_size + 32:
 *   uint32 kind | uint32 start | uint32 end | uint32 n_nodes | n_nodes nodes | zeros up to
 *   slot 2L | slot 2L: the leaf node (ABSENCE only, else zeros)
 * Node bytes min || max || digest as in roots; a level-0 node has the leaf's namespace as
 * both. */
typedef struct {
    uint32_t square; /* square of a batch */
    uint32_t axis;   /* RSM_AXIS_ROW / RSM_AXIS_COL */
    uint32_t index;  /* row or column */
} rsm_ns_query;
/* Bytes of one namespace proof record (0 for width 0, no params or a namespace size 0). */
uint32_t rsm_ns_record_bytes(uint32_t width, const rsm_nmt_params* nmt);
/* n namespace proofs out of an NMT node store.  d_nodes / d_status: what
 * rsm_proof_nodes_dev wrote for these `count` squares (both required); d_eds: the squares
 * (needed with d_shares).  `queries` and `nids` ([n][namespace_size]) are HOST memory,
 * validated before anything is enqueued (RSM_EINVAL names the first query with
 * square >= count, axis > 1 or index >= width) and copied before the call returns;
 * n <= 2^20.  d_records (device, any alignment) receives n records; d_offsets (device,
 * 4-byte aligned, n + 1 uint32) the exclusive prefix sum of the queries' share counts,
 * d_offsets[n] the total; d_shares (device, nullable, 16-byte aligned like d_eds) the
 * shares packed query after query, query i at share d_offsets[i] -- written only where
 * d_offsets[i + 1] <= shares_cap (shares), so a caller compares d_offsets[n] with its
 * capacity and calls again with a larger buffer.  Nothing is stored past shares_cap
 * shares, n records or n + 1 offsets.  nmt == NULL (the DefaultTree has no namespaces)
 * and shapes beyond the NMT node store's limits: RSM_EUNSUPPORTED.  n == 0 or count == 0
 * launches nothing.  Asynchronous on `stream`. */
int rsm_ns_proofs_dev(rsm_ctx* ctx, const void* d_nodes, const void* d_status, const void* d_eds, uint32_t width,
                      uint32_t share_size, uint32_t count, const rsm_nmt_params* nmt, const rsm_ns_query* queries,
                      const uint8_t* nids, uint32_t n, void* d_records, void* d_offsets, void* d_shares,
                      uint64_t shares_cap, void* stream);
/* Host restatement (merkle.cpp), any n_leaves >= 1: the record of namespace `nid`
 * (namespace_size bytes) in the vector `leaves` into record_out
 * (rsm_ns_record_bytes(n_leaves, ..)), the root into root_out (nullable); the shares of
 * an inclusion proof are leaves[start .. end).  RSM_ETREE where the tree fails, as
 * rsm_nmt_tree_prove (so kind 3 never leaves this function). */
int rsm_nmt_namespace_prove(const rsm_nmt_params* params, uint32_t index, const uint8_t* const* leaves,
                            uint32_t n_leaves, uint32_t leaf_size, const uint8_t* nid, uint8_t* record_out,
                            uint8_t* root_out);
/* Verification of a namespace proof (host form; the device form follows): `shares`
 * [n_shares][share_size] are the shares presented with `record` for namespace `nid` of
 * vector `index`, `root` the committed root of the tree of n_leaves leaves.  *status, the
 * first that applies: */
#define RSM_PROOF_NAMESPACE 5  /* INCLUSION: a leaf's wrapper namespace differs from nid;
                                  ABSENCE: the leaf node has min != max or min <= nid */
#define RSM_PROOF_INCOMPLETE 6 /* a left node with max >= nid or a right node with min <= nid
                                  (shares were left out); EMPTY though root.min <= nid <= root.max */
/* 1 RSM_PROOF_MALFORMED: kind not 0..2; EMPTY with a non-zero start, end, n_nodes or with
 *   shares; INCLUSION unless start < end <= n_leaves and n_shares == end - start; ABSENCE
 *   unless end == start + 1 <= n_leaves and n_shares == 0; n_nodes differs from the count
 *   (n_leaves, start, end) dictates.
 * 5 RSM_PROOF_NAMESPACE, 6 RSM_PROOF_INCOMPLETE as above.
 * 2 RSM_PROOF_ORDER: a fold step has right.min < left.max.
 * 3 RSM_PROOF_ROOT: the fold differs from the root (all of min || max || digest).
 * Positions are bound as for single shares: counts and operand sides come from
 * (n_leaves, start, end) once the header passed the MALFORMED check, the fold runs over
 * the derived count, record bytes past the derived nodes (and, for ABSENCE, the leaf
 * slot) are never read, and no address depends on record or share contents.  The return
 * value is an argument error only (RSM_EINVAL; RSM_ETREE for shares shorter than the
 * namespace). */
int rsm_nmt_namespace_verify(const rsm_nmt_params* params, uint32_t index, const uint8_t* nid, const uint8_t* shares,
                             uint32_t n_shares, uint32_t share_size, uint32_t n_leaves, const uint8_t* record,
                             const uint8_t* root, uint32_t* status);
/* Device form: n namespace proofs in one launch, one wave per query, on exactly what the
 * producing calls write, so prove -> verify composes on the device with no repacking.
 * d_records [n][rsm_ns_record_bytes(width, nmt)] (any alignment), d_offsets n + 1 uint32
 * (4-byte aligned) and d_shares (16-byte aligned, shares_total shares of share_size
 * bytes; NULL only with shares_total == 0) as rsm_ns_proofs_dev writes them; d_roots
 * [count][2][width][2 * namespace_size + 32] as rsm_nmt_roots_squares_dev lays them out;
 * d_status [n] uint32 (4-byte aligned).  `queries` and `nids` ([n][namespace_size]) are
 * HOST memory, validated before anything is enqueued (RSM_EINVAL names the first query
 * with square >= count, axis > 1 or index >= width) and copied before the call returns;
 * n <= 2^20.
 * Query i asks: is record i, with shares [d_offsets[i], d_offsets[i + 1]), a complete
 * answer for nids[i] in vector (square, axis, index), under root (square, axis, index) of
 * d_roots?  d_status[i] receives the word rsm_nmt_namespace_verify gives, with the same
 * precedence (1 MALFORMED, 5 NAMESPACE, 6 INCOMPLETE, 2 ORDER, 3 ROOT, 0 OK), n_shares
 * being d_offsets[i + 1] - d_offsets[i].  One device-only rule comes first: if
 * d_offsets[i] > d_offsets[i + 1] or d_offsets[i + 1] > shares_total the status is
 * MALFORMED and nothing of that query's shares or record is read.  A record of kind 3
 * (RSM_NS_TREE) is MALFORMED, as on the host.
 * The contract, as for single shares:
 *   Positions are bound.  Node count, left and right counts and operand sides come from
 *   (width, start, end), and only after the header has passed the MALFORMED checks
 *   (start < end <= width, n_shares == end - start, ..); the record's n_nodes is only
 *   compared with the derived count.
 *   No address depends on record or share contents.  Share addresses come from d_offsets,
 *   bounded by shares_total; node addresses are 16 + i * node_len for i below the derived
 *   count (<= 2L); the leaf slot is at its fixed place and is read for ABSENCE only;
 *   record bytes past the derived nodes are never read.
 *   Writes.  Exactly one status word is written per query, and nothing else.
 * No tree is built and no node store is needed: any 1 <= width <= 1024 is accepted, odd
 * widths included (beyond: RSM_EUNSUPPORTED, a wave's LDS holds `width` nodes), and the
 * quadrant rule uses square_size only.  namespace_size 1..32 (else RSM_EINVAL); nmt ==
 * NULL: RSM_EUNSUPPORTED; share_size a multiple of 64 (else RSM_ESHARESIZE) and >=
 * namespace_size (else RSM_ETREE).  RSM_EINVAL also for NULL or misaligned operands and
 * n > 2^20.  n == 0 or count == 0 launches nothing.  Asynchronous on `stream`. */
int rsm_ns_proofs_verify_dev(rsm_ctx* ctx, const void* d_records, const void* d_offsets, const void* d_shares,
                             uint64_t shares_total, const void* d_roots, uint32_t width, uint32_t share_size,
                             uint32_t count, const rsm_nmt_params* nmt, const rsm_ns_query* queries,
                             const uint8_t* nids, uint32_t n, void* d_status, void* stream);

/* ---- range proofs ------------------------------------------------------------------ */
/* "These shares are leaves [start, end) of this row (or column), under this root": nmt's
 * ProveRange / VerifyInclusion, and per touched row the share half of Celestia's
 * ShareProof (the other half, the row roots under the data root, is "data root" above).
 * An inclusion claim, not a completeness claim: the caller names the range, for either
 * tree.  Vector and leaf namespaces as in "namespace proofs".
 * Record, fixed stride rsm_range_record_bytes = 16 + (2L + 1) * node_len: the namespace
 * record of kind RSM_NS_INCLUSION over [start, end) --
 *   uint32 kind = 1 | uint32 start | uint32 end | uint32 n_nodes | n_nodes nodes | zeros up
 *   to slot 2L | slot 2L zeros
 * with the nodes and their order as "namespace proofs" derives them from (W, start, end)
 * (never more than 2L); node_len = 32 with nmt == NULL (DefaultTree), else
 * 2 * namespace_size + 32.  For an NMT range that is exactly a namespace's range the
 * record is byte-identical to the one rsm_ns_proofs_dev writes. */
typedef struct {
    uint32_t square; /* square of a batch */
    uint32_t axis;   /* RSM_AXIS_ROW / RSM_AXIS_COL */
    uint32_t index;  /* row or column */
    uint32_t start;  /* leaves [start, end) of it */
    uint32_t end;
} rsm_range_query;
/* Bytes of one range proof record (0 for width 0 or a namespace size 0). */
uint32_t rsm_range_record_bytes(uint32_t width, const rsm_nmt_params* nmt);
/* n range proofs out of a node store.  Operands, alignment, the shares_cap rule, limits
 * and asynchrony as rsm_ns_proofs_dev, except: there is no d_status and there are no
 * nids; nmt == NULL is accepted and means a DefaultTree store (every width that store
 * takes); `queries` (HOST memory, copied before the call returns, n <= 2^20) is validated
 * before anything is enqueued, RSM_EINVAL naming the first query with square >= count,
 * axis > 1, index >= width or not start < end <= width.  The call proves ranges of
 * whatever the store holds: a tree whose status word (rsm_proof_nodes_dev) is non-zero
 * still has every node, and its proofs fold to the root stored for it. */
int rsm_range_proofs_dev(rsm_ctx* ctx, const void* d_nodes, const void* d_eds, uint32_t width, uint32_t share_size,
                         uint32_t count, const rsm_nmt_params* nmt, const rsm_range_query* queries, uint32_t n,
                         void* d_records, void* d_offsets, void* d_shares, uint64_t shares_cap, void* stream);
/* Host restatements (merkle.cpp), any n_leaves >= 1: the record of leaves [start, end) of
 * the vector `leaves` into record_out (rsm_range_record_bytes(n_leaves, ..)), the root
 * into root_out (nullable).  RSM_EINVAL unless start < end <= n_leaves; RSM_ETREE where
 * the tree fails, as rsm_nmt_tree_prove. */
int rsm_default_tree_range_prove(const uint8_t* const* leaves, uint32_t n_leaves, uint32_t leaf_size, uint32_t start,
                                 uint32_t end, uint8_t* record_out, uint8_t* root_out);
int rsm_nmt_tree_range_prove(const rsm_nmt_params* params, uint32_t index, const uint8_t* const* leaves,
                             uint32_t n_leaves, uint32_t leaf_size, uint32_t start, uint32_t end, uint8_t* record_out,
                             uint8_t* root_out);
/* Verification (host forms; the device forms follow): are `shares` [n_shares][share_size]
 * leaves [start, end) of the tree of n_leaves leaves with root `root`, by `record`?  start
 * and end are the CALLER's question.  *status, the first that applies:
 * 1 RSM_PROOF_MALFORMED: n_shares != end - start; record kind != 1; the record's start or
 *   end differ from the caller's; n_nodes differs from the count (n_leaves, start, end)
 *   dictates.
 * 2 RSM_PROOF_ORDER (NMT): a join has right.min < left.max.
 * 3 RSM_PROOF_ROOT: the fold differs from the root (NMT: all of min || max || digest).
 * 0 RSM_PROOF_OK.  There is no NAMESPACE or INCOMPLETE status.
 * NMT leaf p takes the wrapper's namespace, so a range may cross square_size and hold
 * several namespaces; ignore_max_namespace is honoured in every join.  The return value
 * is an argument error only (RSM_EINVAL, also unless start < end <= n_leaves; RSM_ETREE
 * for shares shorter than the namespace). */
int rsm_default_tree_range_verify(uint32_t start, uint32_t end, const uint8_t* shares, uint32_t n_shares,
                                  uint32_t share_size, uint32_t n_leaves, const uint8_t* record, const uint8_t* root,
                                  uint32_t* status);
int rsm_nmt_tree_range_verify(const rsm_nmt_params* params, uint32_t index, uint32_t start, uint32_t end,
                              const uint8_t* shares, uint32_t n_shares, uint32_t share_size, uint32_t n_leaves,
                              const uint8_t* record, const uint8_t* root, uint32_t* status);
/* Device form: n range proofs in one launch, one wave per query, on exactly what
 * rsm_range_proofs_dev writes.  d_records [n][rsm_range_record_bytes(width, nmt)] (any
 * alignment), d_offsets n + 1 uint32 (4-byte aligned), d_shares (16-byte aligned,
 * shares_total shares; NULL only with shares_total == 0), d_roots [count][2][width]
 * [node_len] as the roots calls lay them out, d_status [n] uint32 (4-byte aligned).
 * `queries` are HOST memory, validated as in rsm_range_proofs_dev before anything is
 * enqueued and copied before the call returns; n <= 2^20.  d_status[i] receives the word
 * the host form gives for query i's start and end with n_shares = d_offsets[i + 1] -
 * d_offsets[i], after one device-only rule: if d_offsets[i] > d_offsets[i + 1] or
 * d_offsets[i + 1] > shares_total the status is MALFORMED and nothing of that query's
 * record or shares is read.
 * The contract, as for the other verifiers:
 *   Positions are bound.  start and end come from the query, host memory of the verifier;
 *   the record's are only compared with them.  A valid proof of [a, b) presented for
 *   [a + 1, b + 1), or for the same range of another vector, does not verify.
 *   Counts, operand sides and every address come from (width, start, end) and the
 *   offsets, never from what a record or a share holds.  Record bytes past the derived
 *   nodes are never read, slot 2L included.
 *   Writes.  Exactly one status word is written per query, and nothing else.
 * No tree is built and no node store is needed.  NMT: 1 <= width <= 1024, namespace_size
 * 1..32 (else RSM_EINVAL); DefaultTree (nmt == NULL): 1 <= width <= 2048 (64 KiB of LDS
 * per wave at 2048); odd widths included; beyond: RSM_EUNSUPPORTED.  share_size a
 * multiple of 64 (else RSM_ESHARESIZE) and, NMT, >= namespace_size (else RSM_ETREE).
 * RSM_EINVAL also for NULL or misaligned operands and n > 2^20.  Checks in the order of
 * rsm_ns_proofs_verify_dev.  n == 0 or count == 0 launches nothing.  Asynchronous on
 * `stream`. */
int rsm_range_proofs_verify_dev(rsm_ctx* ctx, const void* d_records, const void* d_offsets, const void* d_shares,
                                uint64_t shares_total, const void* d_roots, uint32_t width, uint32_t share_size,
                                uint32_t count, const rsm_nmt_params* nmt, const rsm_range_query* queries, uint32_t n,
                                void* d_status, void* stream);
/* Chained form, with no root table: query i also takes root record i of d_root_records
 * (stride rsm_data_root_record_bytes(width), as rsm_root_proofs_dev writes it for
 * (square, axis, index)) and is compared with d_data_roots[square] (32 bytes).  Straight
 * after rule 1 and before anything is hashed, a root record whose header differs from
 * what (2 * width, axis * width + index) dictates is MALFORMED.  The range's folded root
 * (NMT: min || max || digest) is then hashed as that leaf of the data-root tree and folded
 * through the root record: RSM_PROOF_ORDER (NMT, the range fold), RSM_PROOF_ROOT or
 * RSM_PROOF_OK.  Everything else as rsm_range_proofs_verify_dev. */
int rsm_range_proofs_verify_data_root_dev(rsm_ctx* ctx, const void* d_records, const void* d_offsets,
                                          const void* d_shares, uint64_t shares_total, const void* d_root_records,
                                          const void* d_data_roots, uint32_t width, uint32_t share_size, uint32_t count,
                                          const rsm_nmt_params* nmt, const rsm_range_query* queries, uint32_t n,
                                          void* d_status, void* stream);
/* Host only: ODS shares [start, end) in row-major order of the k x k original square of
 * `square` as one row query per touched row (share i: row i / k, column i % k, all below
 * k) into queries_out[0 .. *n_out), at most k of them -- the row ranges of a ShareProof.
 * RSM_EINVAL unless start < end <= k * k, 1 <= k <= 32768 and the operands are non-NULL. */
int rsm_share_range_queries(uint32_t k, uint32_t square, uint32_t start, uint32_t end,
                            rsm_range_query* queries_out /* [k] */, uint32_t* n_out);

/* ---- share commitments -------------------------------------------------------------- */
/* The 32-byte hash a MsgPayForBlobs carries for a blob: celestia-app's
 * inclusion.CreateCommitment (from the blob's shares) and inclusion.GetCommitment (from a
 * square's cached subtree roots).  With n >= 1 the blob's share count and t >= 1 the
 * subtree root threshold (Celestia: 64), pow2ceil(x) the least power of two >= x:
 *   subtree width  w(n, t) = min(pow2ceil(ceil(n / t)), pow2ceil(ceil(sqrt(n))));
 *   mountain range sizes(n, w): while n > 0 emit w if n >= w, else the largest power of
 *     two <= n, and subtract it -- M sizes, never increasing, each dividing the one before;
 *   subtree root r_i: the NMT root (min || max || digest, 2 * namespace_size + 32 bytes)
 *     over the i-th run of shares, every leaf under its own namespace share[:namespace_size]
 *     (a run of one: the leaf node).  Within a run a namespace below its predecessor's is a
 *     push-order error; across a run boundary it is not;
 *   commitment: the RFC 6962 root over r_0 .. r_{M-1} (leaf SHA-256(0x00 || r_i), node
 *     SHA-256(0x01 || l || r), split at the largest power of two below the count; M = 1
 *     gives the leaf hash) -- tendermint's HashFromByteSlices.
 * In a square of ODS width k (a power of two) a blob at ODS shares [start, start + len),
 * row-major, with start a multiple of w(len, t) (the non-interactive default rules,
 * ADR-013) has w <= k, no subtree crosses a row, and the subtree of size z at position p is
 * node (log2 z, (p mod k) >> log2 z) of row p / k's tree in the level picture of "share
 * inclusion proofs": the node store of rsm_proof_nodes_dev already holds it.
 * square_size of the params is not used by the shares forms.  Only the NMT has
 * commitments: nmt == NULL is RSM_EUNSUPPORTED. */
#define RSM_COMMIT_ORDER 1 /* a push-order error inside a subtree; the commitment is 32 zeros */
#define RSM_COMMIT_TREE 2  /* store forms: a touched row's tree status word is non-zero
                              (its quadrant-0 namespaces are out of order); 32 zeros */
/* Host helpers.  rsm_subtree_width: w(share_count, threshold), 0 for a zero argument.
 * rsm_subtree_sizes: the M sizes into sizes_out[0 .. M) and M into *n_out; sizes_out NULL
 * only counts.  RSM_EINVAL for share_count 0, a width that is no power of two, n_out NULL,
 * or M > cap (then *n_out is still set and nothing is written). */
uint32_t rsm_subtree_width(uint32_t share_count, uint32_t threshold);
int rsm_subtree_sizes(uint32_t share_count, uint32_t width, uint32_t* sizes_out, uint32_t cap, uint32_t* n_out);
/* Host restatements (merkle.cpp).  rsm_blob_commitment: shares [n_shares][share_size],
 * any count, from the blob's own runs.  *status 0 with the commitment in out, or
 * RSM_COMMIT_ORDER with zeros.  RSM_EINVAL for NULL operands, n_shares, threshold or
 * namespace_size 0, namespace_size > 32; RSM_ETREE for shares shorter than a namespace. */
int rsm_blob_commitment(const rsm_nmt_params* params, const uint8_t* shares, uint32_t n_shares, uint32_t share_size,
                        uint32_t threshold, uint8_t out[32], uint32_t* status);
/* rsm_square_commitment: the same value through the row-tree coordinates above, an
 * independent statement.  The square is either ods (k * k share pointers, row-major) or
 * eds ([2k][2k][share_size] bytes), exactly one non-NULL.  The levels of each touched
 * row's quadrant-0 half are built and the blob's nodes read off; roots_out (nullable)
 * receives the M subtree roots, packed.  *status 0, or RSM_COMMIT_TREE with zeros where a
 * touched row's namespaces are out of order.  RSM_EINVAL also unless k is a power of two,
 * len >= 1, start + len <= k * k and start is a multiple of w(len, threshold). */
int rsm_square_commitment(const rsm_nmt_params* params, const uint8_t* const* ods, const uint8_t* eds, uint32_t k,
                          uint32_t share_size, uint32_t start, uint32_t len, uint32_t threshold, uint8_t out[32],
                          uint8_t* roots_out, uint32_t* status);
/* Shares path, device: the commitments of n blobs in one call.  Blob i is shares
 * [offsets[i], offsets[i + 1]) of the packed d_shares (device, 16-byte aligned).  `offsets`
 * (n + 1 share offsets) is HOST memory, validated before anything is enqueued (RSM_EINVAL
 * names the first blob that is empty or whose offsets decrease) and used before the call
 * returns.  d_commitments [n][32] (any alignment) and d_status [n] uint32 (4-byte aligned)
 * receive, per blob, the commitment and 0, or 32 zeros and RSM_COMMIT_ORDER; which
 * subtree failed first is decided as a minimum over subtree indices, so no lane order
 * shows.  d_work (16-byte aligned): rsm_commit_work_bytes(total shares, total subtree
 * roots, nmt) bytes -- the leaf records, the packed subtree roots and their flags.
 * Three stages: one lane per share (leaf records); one launch per subtree size present
 * (size 1 a copy, 2 .. 128 packed into waves, 256 .. 1024 a workgroup each); one workgroup
 * per blob for the fold.  Limits, RSM_EUNSUPPORTED beyond them: n <= 2^20, total shares
 * <= 2^24, subtree width <= 1024 (the device NMT's width and LDS: 512 at namespace_size
 * 32), at most 4096 subtree roots per blob.  rsm_commit_work_bytes is 0 for nmt == NULL, a
 * namespace size outside 1 .. 32, more than 2^24 shares or more roots than shares.
 * Share size rules and argument errors as rsm_range_proofs_verify_dev (a multiple of 64,
 * else RSM_ESHARESIZE; >= namespace_size, else RSM_ETREE; RSM_EINVAL for NULL or
 * misaligned operands, threshold 0, namespace_size outside 1 .. 32).  No address depends
 * on what a share holds.  n == 0 launches nothing.  Asynchronous on `stream`. */
uint64_t rsm_commit_work_bytes(uint64_t total_shares, uint64_t total_subtree_roots, const rsm_nmt_params* nmt);
int rsm_blob_commitments_dev(rsm_ctx* ctx, const void* d_shares, uint32_t share_size, const rsm_nmt_params* nmt,
                             uint32_t threshold, const uint32_t* offsets, uint32_t n, void* d_work, void* d_commitments,
                             void* d_status, void* stream);
/* Store path, device: the commitments of n blobs that sit in `count` squares whose NMT
 * node store (d_nodes) and tree status words (d_status_trees, 2 * width per square) are
 * what rsm_proof_nodes_dev wrote.  No share is read and no leaf is hashed: the call
 * gathers each blob's M nodes and folds them; it takes no scratch. */
typedef struct {
    uint32_t square; /* square of the batch */
    uint32_t start;  /* ODS shares [start, start + len), row-major in the k x k original square */
    uint32_t len;
} rsm_blob_ref;
/* `blobs` is HOST memory, validated before anything is enqueued and copied before the call
 * returns: RSM_EINVAL names the first blob with square >= count, len == 0, start + len >
 * k * k or start not a multiple of w(len, threshold).  RSM_EUNSUPPORTED unless k =
 * width / 2 is a power of two and the store's own limits hold (rsm_proof_nodes_bytes != 0),
 * for n > 2^20 and for a blob of more than 4096 subtree roots.  d_status [n]: 0, or
 * RSM_COMMIT_TREE (a touched row's status word is non-zero) with 32 zeros in
 * d_commitments [n][32] (any alignment).  d_roots_out (nullable, any alignment) receives
 * the subtree roots of all blobs, packed, 2 * namespace_size + 32 bytes each -- the
 * SubtreeRoots of a commitment proof -- and d_root_offsets (nullable, 4-byte aligned) the
 * n + 1 root offsets.  Exactly n commitments and n status words are written, plus the
 * optional outputs.  n == 0 or count == 0 launches nothing.  Asynchronous on `stream`. */
int rsm_commitments_dev(rsm_ctx* ctx, const void* d_nodes, const void* d_status_trees, uint32_t width, uint32_t count,
                        const rsm_nmt_params* nmt, uint32_t threshold, const rsm_blob_ref* blobs, uint32_t n,
                        void* d_roots_out, void* d_root_offsets, void* d_commitments, void* d_status, void* stream);

/* ---- ExtendedDataSquare (extendeddatasquare.go, datasquare.go) ------------------ */
/* ComputeExtendedDataSquare(data, codec, tree) (:50-77): n shares (lens[i] bytes). */
int rsm_eds_compute(rsm_ctx* ctx, const uint8_t* const* data, const uint32_t* lens, uint64_t n,
                    rsm_eds** out);
/* ImportExtendedDataSquare (:95-124): data[i] == NULL marks a missing share.
 * Import/New are host-only and accept ctx == NULL (a context is then needed,
 * via rsm_eds_set_context, before Repair). */
int rsm_eds_import(rsm_ctx* ctx, const uint8_t* const* data, const uint32_t* lens, uint64_t n,
                   rsm_eds** out);
/* NewExtendedDataSquare(codec, tree, edsWidth, shareSize) (:129-152). */
int rsm_eds_new(rsm_ctx* ctx, uint32_t eds_width, uint32_t share_size, rsm_eds** out);
void rsm_eds_free(rsm_eds* eds);
int rsm_eds_set_context(rsm_eds* eds, rsm_ctx* ctx);
uint32_t rsm_eds_width(const rsm_eds* eds);
uint32_t rsm_eds_original_width(const rsm_eds* eds);
uint32_t rsm_eds_share_size(const rsm_eds* eds);
/* GetCell: copies the share to out and returns 1, or returns 0 for nil. */
int rsm_eds_get_cell(const rsm_eds* eds, uint32_t row, uint32_t col, uint8_t* out);
/* SetCell: RSM_ECELL if the cell is non-nil or len != share size. */
int rsm_eds_set_cell(rsm_eds* eds, uint32_t row, uint32_t col, const uint8_t* share, uint32_t len);
/* Test hook mirroring the reference's unexported setCell (datasquare_test.go:735-739):
 * overwrites a cell without the nil check; share == NULL makes it nil. */
int rsm_eds_overwrite_cell(rsm_eds* eds, uint32_t row, uint32_t col, const uint8_t* share, uint32_t len);
/* Flattened(): width^2 * share_size bytes row-major + width^2 presence bytes. */
int rsm_eds_flattened(const rsm_eds* eds, uint8_t* out, uint8_t* present);
/* RowRoots()/ColRoots() (:258-280): width roots of root_cap bytes each. */
int rsm_eds_roots(rsm_eds* eds, int axis, rsm_tree_root_fn tree_fn, void* user, uint8_t* roots_out,
                  uint32_t root_cap, uint32_t* root_len);

/* The square's data root ("data root" above) into out[32]: the row and column roots by
 * the path rsm_eds_roots takes, then the root over rowRoots ++ colRoots.  With a context
 * and a complete square of a supported width the roots stay on the device and
 * rsm_data_roots_dev hashes them there; otherwise the host restatement runs.  root_len
 * is whatever the tree returns, at most 96 bytes.  Errors as rsm_eds_roots.  Results
 * never depend on the path. */
int rsm_eds_data_root(rsm_eds* eds, rsm_tree_root_fn tree_fn, void* user, uint8_t* out);

/* Proofs of n samples (square = 0) of this square: n records of
 * rsm_proof_record_bytes(width, nmt) into records_out, the n shares into shares_out
 * (nullable).  tree_fn / user as rsm_eds_roots (NULL or rsm_default_tree_root: the
 * DefaultTree; rsm_nmt_tree_root with its params: the NMT); any other plugin
 * RSM_EUNSUPPORTED.  RSM_EINVAL for a sample out of range; RSM_ETREE for a sample in
 * an incomplete vector or in a tree that fails.  With a context and a complete square
 * of a width the device trees take, the node store is built once on the GPU and kept
 * with the square (dropped by SetCell, Repair and rsm_eds_set_context); later calls
 * only gather.  Otherwise the host restatement runs per sample.  Results never depend
 * on the path. */
int rsm_eds_proofs(rsm_eds* eds, rsm_tree_root_fn tree_fn, void* user, const rsm_sample* samples, uint32_t n,
                   uint8_t* records_out, uint8_t* shares_out);

/* Namespace proofs of `nid` (namespace_size bytes) in rows (axis 0) or columns (axis 1)
 * indices[0 .. n) of this square: n records of rsm_ns_record_bytes(width, nmt) into
 * records_out, offsets_out[n + 1] and the packed shares into shares_out (nullable,
 * room for shares_cap shares) as rsm_ns_proofs_dev writes them -- vector i's shares only
 * where offsets_out[i + 1] <= shares_cap.  tree_fn / user must be rsm_nmt_tree_root with
 * its params (anything else RSM_EUNSUPPORTED).  RSM_EINVAL for an index out of range,
 * RSM_ETREE for a vector that is incomplete or whose tree fails.  With a context and a
 * complete square of a supported width the cached node store of rsm_eds_proofs is reused
 * or built and one rsm_ns_proofs_dev call answers; otherwise the host restatement runs
 * per vector.  Results never depend on the path. */
int rsm_eds_namespace_proofs(rsm_eds* eds, rsm_tree_root_fn tree_fn, void* user, int axis, const uint32_t* indices,
                             uint32_t n, const uint8_t* nid, uint8_t* records_out, uint32_t* offsets_out,
                             uint8_t* shares_out, uint64_t shares_cap);

/* Range proofs ("range proofs" above) of n queries (square = 0) of this square: n records
 * of rsm_range_record_bytes(width, nmt) into records_out, offsets_out[n + 1] and the
 * packed shares into shares_out (nullable, room for shares_cap shares) as
 * rsm_range_proofs_dev writes them -- query i's shares only where offsets_out[i + 1] <=
 * shares_cap.  tree_fn / user as rsm_eds_proofs (the DefaultTree and the NMT; any other
 * plugin RSM_EUNSUPPORTED).  RSM_EINVAL for a query out of range, RSM_ETREE for a vector
 * that is incomplete or whose tree fails.  With a context and a complete square of a
 * width the device trees take, the cached node store of rsm_eds_proofs is reused or built
 * and one rsm_range_proofs_dev call answers; otherwise the host restatement runs per
 * query.  Results never depend on the path. */
int rsm_eds_range_proofs(rsm_eds* eds, rsm_tree_root_fn tree_fn, void* user, const rsm_range_query* queries, uint32_t n,
                         uint8_t* records_out, uint32_t* offsets_out, uint8_t* shares_out, uint64_t shares_cap);

/* Share commitments ("share commitments" above) of n blobs (square = 0) of this square:
 * out [n][32], status_out [n] (0 or RSM_COMMIT_TREE with zeros).  tree_fn / user must be
 * rsm_nmt_tree_root with its params, square_size the square's ODS width (any other plugin
 * RSM_EUNSUPPORTED).  RSM_EINVAL names the first blob that rsm_commitments_dev would
 * refuse; RSM_ETREE for a blob that touches a nil quadrant-0 cell.  With a context, a
 * complete square and a supported width the cached node store of rsm_eds_proofs is reused
 * or built and one rsm_commitments_dev call answers; otherwise rsm_square_commitment runs
 * per blob.  Results never depend on the path.  rsm_eds_subtree_roots: the same call that
 * also hands out the blobs' subtree roots, packed (roots_out, room for the sum of their
 * counts -- rsm_subtree_sizes), and the n + 1 root offsets (root_offsets_out). */
int rsm_eds_commitments(rsm_eds* eds, rsm_tree_root_fn tree_fn, void* user, const rsm_blob_ref* blobs, uint32_t n,
                        uint32_t threshold, uint8_t* out, uint32_t* status_out);
int rsm_eds_subtree_roots(rsm_eds* eds, rsm_tree_root_fn tree_fn, void* user, const rsm_blob_ref* blobs, uint32_t n,
                          uint32_t threshold, uint8_t* out, uint32_t* status_out, uint8_t* roots_out,
                          uint32_t* root_offsets_out);

/* Rebuilding a square from sampled shares: verifies n samples (square = 0; shares
 * [n][share size], records [n][rsm_proof_record_bytes(width, nmt)]) against the
 * committed roots (row_roots / col_roots / root_len as rsm_eds_repair takes them) and
 * sets the cells of those that verify.  tree_fn / user as rsm_eds_proofs.  A sample
 * addresses cell (index, pos) for a row and (pos, index) for a column and is verified
 * against row_roots[index] / col_roots[index].  The samples are then applied in order:
 * status 0 on a nil cell sets it (SetCell; the cached node store is dropped); status 0
 * on a non-nil cell -- an earlier sample of the same batch included -- becomes
 * RSM_PROOF_OCCUPIED and the cell is left as it is; any other status writes nothing.
 * Returns RSM_OK however many samples were rejected; status_out (n words, nullable)
 * and *accepted (nullable: the number of cells set) report them.  With a context the
 * verification is one upload and one rsm_proofs_verify_dev; without, the host
 * restatement per sample.  Results never depend on the path. */
int rsm_eds_import_samples(rsm_eds* eds, const uint8_t* row_roots, const uint8_t* col_roots, uint32_t root_len,
                           rsm_tree_root_fn tree_fn, void* user, const rsm_sample* samples, uint32_t n,
                           const uint8_t* shares, const uint8_t* records, uint32_t* status_out, uint32_t* accepted);

typedef struct {
    int32_t axis;   /* RSM_AXIS_ROW / RSM_AXIS_COL */
    uint32_t index; /* row or column index */
} rsm_byzantine;

/* Repair(rowRoots, colRoots) (extendeddatacrossword.go:74-84): roots are
 * width * root_len bytes each.  Returns 0, RSM_EUNREPAIRABLE, or RSM_EBYZANTINE
 * (then *byz names the axis/index; rsm_eds_byzantine_shares() returns the
 * vector's shares as they were before repair, missing shares absent). */
int rsm_eds_repair(rsm_eds* eds, const uint8_t* row_roots, const uint8_t* col_roots, uint32_t root_len,
                   rsm_tree_root_fn tree_fn, void* user, rsm_byzantine* byz);
int rsm_eds_byzantine_shares(const rsm_eds* eds, uint8_t* out, uint8_t* present);

/* Diagnostics: counters of the last Repair on this square (reset by every rsm_eds_repair).
 *   fast_path        1 when the device fast path repaired the square and its device
 *                    verification accepted it; 0 otherwise (the pre-repair check
 *                    failed, the square was already complete, or the exact sequential
 *                    solver produced the result).
 *   sweeps           batched device decode sweeps launched by the fast path (one per
 *                    axis pass); 0 when the pre-repair check already failed.
 *   decoded_vectors  rows and columns decoded by those sweeps.
 *   fallback_reason  why the fast path handed over to the exact solver:
 *                      0  it did not (fast path accepted, or never ran)
 *                      1  stuck: the sweeps stopped with cells still missing
 *                      2  encoding: the rebuilt square is not a valid 2D codeword
 *                      3  roots: a row or column root (or an NMT tree status) differs
 *                         from the committed one
 *                    The encoding compare is consulted first, so 3 means the encoding
 *                    was fine. */
typedef struct {
    int32_t fast_path;
    uint32_t sweeps;
    uint32_t decoded_vectors;
    uint32_t fallback_reason;
} rsm_repair_stats;
int rsm_eds_repair_stats(const rsm_eds* eds, rsm_repair_stats* out);

/* ---- Repair of device-resident squares ---------------------------------------------- */
/* The last step of the sampling flow without the host square: samples verified by
 * rsm_proofs_verify_dev are set into device squares (rsm_samples_scatter_dev), and the
 * squares are repaired and checked where they lie, a batch per call
 * (rsm_repair_squares_dev).  No share crosses the bus; between sweeps a few words per
 * square do.  Status of a square: */
#define RSM_REPAIR_OK 0        /* complete, a valid 2D codeword, every root the committed one */
#define RSM_REPAIR_STUCK 1     /* the sweeps stopped with cells missing; nothing was verified */
#define RSM_REPAIR_ENCODING 2  /* complete, but not the extension of its own Q0 */
#define RSM_REPAIR_ROOTS 3     /* a valid codeword, but a root (or an NMT tree status) differs */
typedef struct {
    uint32_t status;          /* RSM_REPAIR_* */
    uint32_t sweeps;          /* passes that decoded something in this square */
    uint32_t decoded_vectors; /* rows and columns decoded by them */
    uint32_t missing;         /* cells still missing (0 unless STUCK) */
} rsm_repair_result;
/* Bytes of the caller's scratch for one call (re-extension copies, leaf digests, roots,
 * tree statuses, todo lists, flags: about count * (4 k^2 share_size + 4 k^2 * 32, NMT 64));
 * 0 for shapes the call does not take. */
uint64_t rsm_repair_work_bytes(uint32_t k, uint32_t share_size, uint32_t count, const rsm_nmt_params* nmt);
/* Repairs `count` squares in place.  d_eds (device, 16-byte aligned) is
 * [count][2k][2k][share_size] as in rsm_extend_squares_dev; d_presence (device, 16-byte
 * aligned, in/out) [count][2k][2k] bytes, non-zero = the cell is given; d_roots (device,
 * any alignment) the committed roots [count][2][2k][root_len] exactly as
 * rsm_roots_squares_dev / rsm_nmt_roots_squares_dev write them (nmt == NULL: the
 * DefaultTree, root_len 32; else 2 * namespace_size + 32); d_work (device, 16-byte
 * aligned) rsm_repair_work_bytes of scratch; results (HOST) count records.  No other
 * device memory is allocated per call (the codec's own grow-only per-stream scratch of
 * the GF(2^16) decoders aside).
 *
 * Schedule: that of rsm_eds_repair's device fast path.  A row pass, then a column pass,
 * and so on; a pass decodes every vector of its axis with k <= cells < 2k at once, in
 * every square that has one, and counts as one sweep for such a square.  The lists come
 * from a planner kernel over the presence bytes (ascending indices, so the result does
 * not depend on scheduling); the host reads one count per square from pinned memory
 * after each pass and launches the decoders.  A square drops out once it misses nothing
 * or two passes in a row found nothing in it (it is stuck), while the others go on; the
 * loop ends when every square has, after at most 4k decoding passes.
 * Completed squares are then verified as one batch on the device: Q0 is copied to d_work
 * and re-extended, and the square must equal the result (else RSM_REPAIR_ENCODING; this
 * compare is consulted first, as in rsm_repair_stats); all 4k roots of every such square
 * are computed and must equal d_roots, with every NMT tree status zero (else
 * RSM_REPAIR_ROOTS).  Two flags per square return to the host.
 *
 * Contract.  A cell whose presence byte is non-zero on entry is never written.  On return
 * d_presence holds the peeling closure: non-zero in every cell of a square that completed
 * (given cells keep their byte unless a decoded vector crosses them, which sets 1), and in
 * a STUCK square exactly in the given cells and the cells of decoded vectors.  In squares
 * that are not OK the cells missing on entry hold unspecified bytes.  The call returns
 * after everything it enqueued on `stream` (NULL: the context's) has completed.
 * This call has no pre-repair check of the given vectors and no attribution: RSM_REPAIR_OK
 * means what acceptance by rsm_eds_repair's fast path means, and anything else names no
 * vector.  A caller who needs ErrByzantineData{Axis, Index, Shares} calls
 * rsm_repair_squares_checked_dev (below) instead, which names the vector on the device.
 * Limits: those of the device trees -- 2k <= 2048 for the DefaultTree, 2k <= 1024 with
 * namespace_size 1..32 and 2k <= 2 * square_size for the NMT -- and count * 4 k^2 < 2^32,
 * count <= 65535; beyond them RSM_EUNSUPPORTED (and rsm_repair_work_bytes is 0).
 * RSM_ESHARESIZE for a share size that is no multiple of 64, RSM_EINVAL for k == 0, empty
 * shares, NULL or misaligned operands, RSM_ETREE for shares shorter than the namespace.
 * count == 0 launches nothing. */
int rsm_repair_squares_dev(rsm_ctx* ctx, void* d_eds, void* d_presence, uint32_t k, uint32_t share_size,
                           uint32_t count, const rsm_nmt_params* nmt, const void* d_roots, void* d_work,
                           rsm_repair_result* results, void* stream);
/* ---- Repair of device-resident squares with attribution ------------------------------- */
/* rsm_repair_squares_dev with rsmt2d's ErrByzantineData: the same decoding passes, and
 * around them every row and column is checked -- once, in the round in which it first has
 * all 2k cells -- against its committed root and its own encoding.  A vector is therefore
 * only ever built from cells that were given or that lie in vectors which passed. */
#define RSM_REPAIR_BYZANTINE 4 /* a complete vector failed its check: see rsm_repair_check */
#define RSM_BYZ_ROOT 1         /* its root differs from the committed one */
#define RSM_BYZ_ENCODING 2     /* root equal, but parity != encode(first half) */
#define RSM_BYZ_TREE 3         /* NMT only: the tree's status word is non-zero (consulted first) */
typedef struct {
    uint32_t axis, index;     /* valid when status == RSM_REPAIR_BYZANTINE */
    uint32_t round;           /* 0 = entry check, p = after the square's p-th decoding pass (its p-th sweep) */
    uint32_t reason;          /* RSM_BYZ_* ; 0 otherwise */
    uint32_t checked_vectors; /* vectors whose root and encoding were evaluated */
    uint32_t hashed_cells;    /* leaf records computed */
} rsm_repair_check;
/* Bytes of the checked call's scratch (one leaf record per cell, 32 bytes, NMT 64; one
 * square for re-encoded parity; lists, verdict words, a bit and two bytes of bookkeeping
 * per cell and vector); 0 exactly where rsm_repair_work_bytes is. */
uint64_t rsm_repair_checked_work_bytes(uint32_t k, uint32_t share_size, uint32_t count, const rsm_nmt_params* nmt);
/* Operands, alignment, limits and argument errors are those of rsm_repair_squares_dev
 * (d_work: rsm_repair_checked_work_bytes); `checks` (HOST) receives count records and must
 * not be NULL.
 *
 * Schedule.  The decoding passes are exactly those of rsm_repair_squares_dev (results[]:
 * the same sweeps, decoded_vectors and missing for a square no check fails in).  Round 0
 * checks the vectors complete on entry and names, among failures, the lowest (index, axis),
 * row i before column i -- rsm_eds_repair's pre-repair order.  After a square's p-th
 * decoding pass, of axis a, round p has two stages: stage 1 checks the vectors the pass
 * decoded and names the lowest failing index; only if it is clean, stage 2 checks the
 * vectors of the other axis that the pass completed and names the lowest failing index
 * (after a stage-1 failure those hold cells of the failed vector, so naming one would be
 * unsound).  A check evaluates, in this order, the NMT tree's status (RSM_BYZ_TREE), the
 * root against d_roots (RSM_BYZ_ROOT) and the parity against a re-encode of the first
 * half (RSM_BYZ_ENCODING).  The named vector is a minimum over keys computed on the
 * device: no result depends on the order lanes run in.  A cell's leaf record is computed
 * once per call (hashed_cells), every tree of a stage in one launch for the whole batch.
 *
 * A square with a failing vector is RSM_REPAIR_BYZANTINE and drops out at once, while
 * the others go on.  After a failure in round 0 or in a stage 1 its d_presence stays as
 * the failing pass's plan found it: that pass's decoded vectors are not marked.  After a
 * failure in a stage 2 the pass's decoded vectors, which all passed stage 1, are marked,
 * so the named vector is complete.  Either way every non-zero presence byte is a cell that
 * was given or lies in a vector that passed its check, the named vector has at least k
 * such cells, and decoding them gives a vector that fails the check: rsm_vectors_gather_dev
 * of it yields ErrByzantineData.Shares, missing as nil, enough for a fraud proof.  (The
 * reference's sequential solver returns an orthogonal vector without the rebuilt share,
 * which can leave fewer than k.)  missing
 * counts the zero presence bytes.  RSM_REPAIR_OK: nothing is missing and no check failed;
 * every row and column was checked (checked_vectors == 4k, hashed_cells == 4k^2), so
 * there is no whole-square verification afterwards.  RSM_REPAIR_STUCK as in
 * rsm_repair_squares_dev, with no complete vector having failed.  RSM_REPAIR_ENCODING and
 * RSM_REPAIR_ROOTS do not occur.  When several vectors are bad the one named may differ
 * from rsm_eds_repair's sequential solver's; it always fails the check stated above on
 * the shares rsm_vectors_gather_dev returns. */
int rsm_repair_squares_checked_dev(rsm_ctx* ctx, void* d_eds, void* d_presence, uint32_t k, uint32_t share_size,
                                   uint32_t count, const rsm_nmt_params* nmt, const void* d_roots, void* d_work,
                                   rsm_repair_result* results, rsm_repair_check* checks, void* stream);
/* Packs n vectors of device squares: refs (HOST; square < count, axis, index < 2k, else
 * RSM_EINVAL; n <= 2^24) name them, d_shares (device, 16-byte aligned) receives
 * [n][2k][share_size] and d_present (device) [n][2k] bytes copied from d_presence: the
 * shares of ErrByzantineData, nil where the byte is 0 (those cells' bytes are whatever
 * the square holds).  d_eds 16-byte aligned; any 1 <= k <= 32768; RSM_ESHARESIZE,
 * RSM_EINVAL as in rsm_samples_scatter_dev; n == 0 or count == 0 launches nothing.
 * Asynchronous on `stream`. */
int rsm_vectors_gather_dev(rsm_ctx* ctx, const void* d_eds, const void* d_presence, uint32_t k, uint32_t share_size,
                           uint32_t count, const rsm_root_ref* refs, uint32_t n, void* d_shares, void* d_present,
                           void* stream);
/* The apply step of rsm_eds_import_samples on device squares: d_eds / d_presence as above
 * (d_presence any alignment here), `samples` HOST memory, validated and copied as in
 * rsm_proofs_verify_dev (against `count` squares of width 2k; n <= 2^24), d_shares
 * [n][share_size] (16-byte aligned) and d_status [n] uint32 as the verifier wrote them.
 * A sample addresses cell (index, pos) for a row and (pos, index) for a column of its
 * square.  With the statuses and presence bytes as they stand on entry: a status-0 sample
 * on a nil cell, with no lower-indexed status-0 sample of the batch on the same cell, has
 * its share copied in and the presence byte set to 1; every other status-0 sample (cell
 * present on entry, or won by a lower index) gets RSM_PROOF_OCCUPIED in d_status and
 * writes nothing else; any other status writes nothing.  These are the results of
 * applying the samples in order, and they do not depend on the order lanes run in: a
 * launch decides from the entry state, a second one applies.  Takes no caller scratch.
 * Argument errors as rsm_repair_squares_dev (any 1 <= k <= 32768: no tree is built).
 * n == 0 or count == 0 launches nothing.  Asynchronous on `stream`. */
int rsm_samples_scatter_dev(rsm_ctx* ctx, void* d_eds, void* d_presence, uint32_t k, uint32_t share_size,
                            uint32_t count, const rsm_sample* samples, uint32_t n, const void* d_shares,
                            void* d_status, void* stream);

/* ---- bad-encoding fraud proofs --------------------------------------------------------
 * The last step of the sampling flow: a node that receives the shares of a vector named by
 * rsm_repair_squares_checked_dev (ErrByzantineData.Shares, as rsm_vectors_gather_dev packs
 * them), each with its Merkle proof in the ORTHOGONAL tree, decides whether the vector is
 * badly encoded -- the reference's PseudoFraudProof (extendeddatacrossword_test.go:19-21,
 * 143-162) with the per-share proofs its TODO asks for.  n proofs are validated per call.
 *
 * Proof i claims that vector refs[i] = (square, axis, index) of a batch of `count` squares
 * of width 2k is badly encoded.  d_shares [n][2k][share_size] (16-byte aligned) and
 * d_present [n][2k] bytes are what rsm_vectors_gather_dev writes.  d_records
 * [n][2k][rsm_proof_record_bytes(2k, nmt)] (any alignment): record (i, j) proves leaf
 * pos = index of tree (axis ^ 1, j) -- what rsm_proofs_dev writes for the samples
 * rsm_fraud_proof_samples lists, so prove -> gather -> validate needs no repacking.
 * d_roots: the committed table [count][2][2k][root_len] of the repair calls.  refs and
 * verdicts are HOST memory (n each).  The first rule that applies gives the verdict:
 *   1. fewer than k presence bytes are non-zero: RSM_FRAUD_TOOFEW;
 *   2. a present slot j whose share does not verify against root (square, axis ^ 1, j) at
 *      position index, by rsm_proofs_verify_dev's contract: RSM_FRAUD_SHARE, pos = the lowest
 *      such j, reason = its RSM_PROOF_* word (a minimum over keys: no lane order shows);
 *   3. the missing slots are decoded from the present ones (a vector with all 2k present is
 *      taken as it is) and the rebuilt vector gets rsm_repair_squares_checked_dev's check in
 *      its order -- the NMT tree's status (quadrant rule index < square_size && pos <
 *      square_size), the root against committed root (square, axis, index), the parity
 *      against a re-encode of the first half: RSM_FRAUD_VALID with that RSM_BYZ_* reason;
 *   4. otherwise RSM_FRAUD_CONSISTENT.
 * A slot whose presence byte is non-zero is never written; d_present, d_records and d_roots
 * are never written; nothing is stored outside the missing slots of d_shares and d_work
 * (rsm_fraud_work_bytes bytes, 16-byte aligned).  For VALID and CONSISTENT the missing slots
 * hold the decoded shares on return, for TOOFEW and SHARE unspecified bytes.  No output
 * depends on the share or record bytes of an absent slot.  The call returns after everything
 * it enqueued on `stream` has completed.
 * Limits: those of the device trees (2k <= 2048; NMT: 2k <= 1024, namespace size 1..32,
 * 2k <= 2 * square_size), n <= 65535 and n * 2k <= 2^24: RSM_EUNSUPPORTED beyond them, and
 * rsm_fraud_work_bytes is 0 exactly there.  Argument errors as rsm_repair_squares_dev and
 * rsm_vectors_gather_dev; n == 0 or count == 0 launches nothing. */
#define RSM_FRAUD_VALID 0       /* the proof holds: the vector is bad; reason = RSM_BYZ_TREE / _ROOT / _ENCODING */
#define RSM_FRAUD_TOOFEW 1      /* fewer than k slots present; nothing else was evaluated */
#define RSM_FRAUD_SHARE 2       /* a present share does not verify under its orthogonal committed root:
                                   pos = the lowest such slot, reason = its RSM_PROOF_* status word */
#define RSM_FRAUD_CONSISTENT 3  /* every share verifies and the rebuilt vector passes all three checks: no fraud */
typedef struct {
    uint32_t verdict, reason, pos, present; /* present: non-zero presence bytes */
} rsm_fraud_verdict;
uint64_t rsm_fraud_work_bytes(uint32_t k, uint32_t share_size, uint32_t n, const rsm_nmt_params* nmt);
/* Host only: samples_out[j] = {ref->square, ref->axis ^ 1, j, ref->index} for j < 2k, the
 * samples whose rsm_proofs_dev records are proof `ref`'s row of d_records.  RSM_EINVAL for a
 * null operand, k == 0 or k > 32768, an axis above 1 or index >= 2k. */
int rsm_fraud_proof_samples(const rsm_root_ref* ref, uint32_t k, rsm_sample* samples_out /* [2k] */);
int rsm_fraud_proofs_verify_dev(rsm_ctx* ctx, void* d_shares, const void* d_present, const void* d_records,
                                const void* d_roots, uint32_t k, uint32_t share_size, uint32_t count,
                                const rsm_nmt_params* nmt, const rsm_root_ref* refs, uint32_t n, void* d_work,
                                rsm_fraud_verdict* verdicts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RSMT2D_HIP_H */
