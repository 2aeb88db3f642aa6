/*
 * bbq.h - C ABI of libbbq: the MI355X-native (gfx950 HIP) implementation of the
 * asymmetric binary-quantized scoring + top-k search path of
 * leolee9086/Better-Binary-Quantization.
 *
 * The reference has no FFI seam on this path (it is pure TypeScript); the boundary is the
 * internal call searchNearestNeighbors -> computeBatchQuantizedScores -> MinHeap.  Each entry
 * point below names the reference interface it replaces (paths relative to the reference
 * checkout).  The N-API addon (better-binary-quantization_amd/napi/bbq_napi.c) and the
 * ctypes binding (better-binary-quantization_amd/python/bbq_amd/capi.py) bind exactly these
 * symbols; INTEGRATION.md shows the reference-side patch.
 *
 * Conventions: plain pointers and sizes, no framework types.  All input arrays are borrowed for
 * the duration of the call and never retained or written.  Every function returns BBQ_OK (0) or
 * a BBQ_ERR_* code; bbq_last_error() returns a thread-local, human-readable message for the last
 * failure on the calling thread.  There is NO CPU fallback: without a usable HIP device every
 * device entry point fails with BBQ_ERR_NO_DEVICE.
 *
 * Corrections layout (src/types.ts:18-27), 4 doubles per vector:
 *   {lowerInterval, upperInterval, additionalCorrection, quantizedComponentSum}.
 * Packed 1-bit rows (src/optimizedScalarQuantizer.ts:420-446): dim d -> byte d>>3, bit 7-(d&7),
 *   ceil(dim/8) bytes per row.
 */
#ifndef BBQ_H
#define BBQ_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BBQ_ABI_VERSION 3  /* 2: multi-bit and multi-device indexes, bbq_stats.host_replays
                              3: creation options (corrections layout), asynchronous shard scans with shard-local answers,
                                 bbq_merge_answers, persistence of shards and multi-device indexes
                              (still 3: filtered search - bbq_filter_*, bbq_search_filtered_batch - only adds symbols, as do the appends
                              and the compaction - bbq_index_compact, bbq_index_remove_rows, bbq_vectors_compact, bbq_filter_kept_rows - and the
                              in-place updates - bbq_index_update_rows, bbq_index_update, bbq_vectors_update, bbq_update_winners - and the scoring of chosen rows -
                              bbq_score_ords, bbq_score_ords_batch, bbq_search_ords_batch - and the range search - bbq_range_key,
                              bbq_count_range_batch, bbq_search_range_batch - and the span search - bbq_search_spans_batch,
                              bbq_search_spans_filtered_batch - and the grouped search - bbq_groups_create, bbq_groups_destroy,
                              bbq_groups_count, bbq_groups_live, bbq_groups_plan, bbq_search_grouped_batch - and the MaxSim search -
                              bbq_search_maxsim_batch, bbq_maxsim_reduce, bbq_maxsim_token_block - and MaxSim over chosen groups -
                              bbq_score_maxsim_groups_batch, bbq_search_maxsim_groups_batch - and the exact MaxSim rerank -
                              bbq_maxsim_reduce_true, bbq_rerank_maxsim_groups_batch, bbq_search_maxsim_rerank_batch - and the exact search -
                              bbq_true_topk, bbq_vectors_search_batch, bbq_vectors_set_option) */

/* status codes */
enum {
  BBQ_OK = 0,
  BBQ_ERR_INVALID_ARG = 1,   /* null pointer, bad size, bits out of 1..8, ... */
  BBQ_ERR_NO_DEVICE = 2,     /* no HIP device / runtime unusable: the product path refuses to run */
  BBQ_ERR_HIP = 3,           /* a HIP call failed; message carries hipGetErrorString */
  BBQ_ERR_OOM = 4,
  BBQ_ERR_UNSUPPORTED = 5,   /* e.g. more than 2^32 rows, k out of the sharded range, a file of another format version */
  BBQ_ERR_DIM_MISMATCH = 6,  /* src/binaryQuantizationFormat.ts:327-329 */
  BBQ_ERR_NEGATIVE_K = 7,    /* src/binaryQuantizationFormat.ts:324-326 */
  BBQ_ERR_NAN_INPUT = 8,     /* src/binaryQuantizationFormat.ts:202-204 */
  BBQ_ERR_INF_INPUT = 9,     /* src/binaryQuantizationFormat.ts:205-207 */
  BBQ_ERR_EMPTY = 10         /* src/binaryQuantizationFormat.ts:169-171 */
};

/* src/types.ts:9-13 VectorSimilarityFunction (string enum in the reference) */
enum { BBQ_EUCLIDEAN = 0, BBQ_COSINE = 1, BBQ_MAXIMUM_INNER_PRODUCT = 2 };

typedef struct bbq_index bbq_index; /* opaque: a device-resident index shard */

/* one top-k candidate as the device emits it: (global row << 32) | IEEE-754 bits of the f32 score */
typedef uint64_t bbq_cand;

const char *bbq_last_error(void);
int bbq_abi_version(void);
/* number of usable HIP devices (0 if none); never fails */
int bbq_device_count(void);

/* ------------------------------------------------------------------------------------------
 * Index: replaces BinarizedByteVectorValuesImpl (src/binaryQuantizationFormat.ts:24-126) as the
 * scorer sees it, and createDirectPackedBuffer (src/batchDotProduct.ts:420-436): the packed rows
 * are staged ONCE, re-tiled into the device layout (DESIGN.md "HBM layout"), instead of being
 * gathered into a contiguous buffer for every batch of 1000.
 *
 *   codes        index_bits == 1: [n_rows * ceil(dim/8)] packed 1-bit rows
 *                index_bits  > 1: [n_rows * dim] one byte per dimension, values < 2^index_bits - the shape quantizeVectors
 *                gives such rows (src/binaryQuantizationFormat.ts:241-245).  Stored as 2-bit (index_bits 2), 4-bit (3-4) or
 *                8-bit (5-8) fields and scanned with the packed-nibble / packed-byte dot instructions.  Scores follow what
 *                the reference RETURNS for such an index: its batch scorer throws on unpacked rows and the per-row scorer
 *                answers (src/binaryQuantizedScorer.ts:403-419, :69-301): bitDotProduct = computeQuantizedDotProduct
 *                (src/bitwiseDotProduct.ts:14-30), centroidDP = 0 unless query_bits == 1 (:290), MAXIMUM_INNER_PRODUCT without the
 *                FOUR_BIT_SCALE division (:207-209).  The reference's per-row scorer only knows query_bits 1 and 4 and throws
 *                for the rest (:95-97); this library scores every query_bits 2..8 with the 4-bit form ("parity unpinned"
 *                beyond the integer dot product, which the reference defines for any widths) - the JS host throws like the
 *                reference does.
 *   corr         [n_rows * 4]            corrections as doubles
 *   centroid_dp  getCentroidDP(undefined) = centroid . centroid  (src/binaryQuantizationFormat.ts:113-121)
 *   device       HIP device ordinal
 */
int bbq_index_create(const uint8_t *codes, const double *corr, int64_t n_rows, int32_t dim,
                     int32_t index_bits, double centroid_dp, int32_t device, bbq_index **out);

/* Creation options (ABI 3): every creator has an _opts twin that takes them; NULL = the defaults, which is what the plain
 * creators pass.  The struct may grow: set `size` to sizeof(bbq_index_options).
 *   corrections   how a row's corrections travel with its codes in HBM (DESIGN.md "HBM layout"):
 *                 BBQ_CORRECTIONS_COMPACT  4 B per row streamed (bf16 lower | bf16 upper) + the exact f64 values in a side array that is
 *                                          read only for rows whose proven score bound beats the threshold (100 B/row at 768-d);
 *                                          falls back to inline when quantizedComponentSum is not the row's popcount / code sum
 *                 BBQ_CORRECTIONS_INLINE   the exact f64 corrections inside the tile record (120 / 128 B/row at 768-d)
 *                 BBQ_CORRECTIONS_DEFAULT  compact, unless the environment variable BBQ_COMPACT_CORRECTIONS=0 overrides it
 *                                          (kept for A/B runs of unchanged callers; an explicit value here always wins)
 * Results never depend on the layout (every fixture runs in both). */
enum { BBQ_CORRECTIONS_DEFAULT = -1, BBQ_CORRECTIONS_INLINE = 0, BBQ_CORRECTIONS_COMPACT = 1 };
typedef struct {
  int32_t size;         /* sizeof(bbq_index_options) */
  int32_t corrections;  /* BBQ_CORRECTIONS_* */
} bbq_index_options;

/* quantizeVectors ON THE DEVICE and the index built in place: BinaryQuantizationFormat.quantizeVectors
 * (src/binaryQuantizationFormat.ts:165-263: normalizeVector for COSINE, NaN/Infinity validation, computeCentroid,
 * scalarQuantize, packAsBinary) for indexBits == 1 (bbq_index_build_bits: any indexBits), bit-exact with the TypeScript path,
 * followed by what bbq_index_create does.  vectors [n*dim] row-major host floats.
 *   centroid [dim]            (host, required)  the f32 centroid; centroid_dp is derived from it
 *   codes [n*ceil(dim/8)], corr [n*4]  (host, each may be NULL) what quantizeVectors returns, for hosts that keep
 *                             the BinarizedByteVectorValues accessors (vectorValue / getCorrectiveTerms)
 * Errors as bbq_quantize_vectors. */
int bbq_index_build(const float *vectors, int64_t n, int32_t dim, int32_t sim, double lambda, int32_t iters,
                    int32_t device, bbq_index **out, float *centroid, uint8_t *codes, double *corr,
                    int64_t *bad_row, int32_t *bad_col);

/* The same for any indexBits (1..8): codes [n*ceil(dim/8)] for index_bits == 1, [n*dim] (one byte per dimension,
 * src/binaryQuantizationFormat.ts:241-245) otherwise. */
int bbq_index_build_bits(const float *vectors, int64_t n, int32_t dim, int32_t sim, int32_t index_bits, double lambda, int32_t iters,
                         int32_t device, bbq_index **out, float *centroid, uint8_t *codes, double *corr,
                         int64_t *bad_row, int32_t *bad_col);
int bbq_index_build_opts(const float *vectors, int64_t n, int32_t dim, int32_t sim, int32_t index_bits, double lambda, int32_t iters,
                         int32_t device, const bbq_index_options *opts, bbq_index **out, float *centroid, uint8_t *codes, double *corr,
                         int64_t *bad_row, int32_t *bad_col);

/* Row-sharded variant for one-process-per-GPU deployments (new; the reference has no distribution).
 *   row_base     global row id of this shard's row 0 (shards are contiguous, ascending)
 *   pilot_codes / pilot_corr / n_pilot
 *                optional replica of n_pilot DISTINCT global rows that all precede this shard (global id <
 *                row_base; n_pilot a multiple of 1024, or all row_base of them): lets every shard derive valid
 *                top-k thresholds without waiting for the shards before it.  The prefix [0, n_pilot) works; an
 *                evenly strided sample of [0, row_base) gives tighter thresholds when rows are stored cluster by
 *                cluster.  Only thresholds are taken from these rows (their ids never appear in a result).
 *                Pass NULL/0 on the shard that owns row 0 (row_base == 0).
 */
int bbq_index_create_shard(const uint8_t *codes, const double *corr, int64_t n_rows, int32_t dim,
                           int32_t index_bits, double centroid_dp, int64_t row_base,
                           const uint8_t *pilot_codes, const double *pilot_corr, int64_t n_pilot,
                           int32_t device, bbq_index **out);
int bbq_index_create_shard_opts(const uint8_t *codes, const double *corr, int64_t n_rows, int32_t dim,
                                int32_t index_bits, double centroid_dp, int64_t row_base,
                                const uint8_t *pilot_codes, const double *pilot_corr, int64_t n_pilot,
                                int32_t device, const bbq_index_options *opts, bbq_index **out);
/* ONE index row-sharded over several GPUs of this process, behind the same handle (new; SURVEY 8b/8e: the reference has no
 * distribution).  Every entry point that takes a bbq_index - bbq_search, bbq_search_batch, bbq_score_rows, bbq_index_export,
 * bbq_search_rerank_batch, bbq_set_option, bbq_get_stats - works on it and returns exactly what the single-device index
 * returns: shards are contiguous row blocks (whole 512-row chunks) in ascending order, each later shard carries a pilot
 * replica of the first pilot_rows global rows (0: none, thresholds start inside the shard), one host thread per shard
 * sweeps it and lands its packed candidate list in pinned host memory over that device's own PCIe link, the calling thread
 * replays the reference heap over the lists in shard order (bbq_replay_batch) while the next round of queries is swept.
 *   n_shards     1..64
 *   devices      [n_shards] HIP device ordinal of every shard (NULL: shard s on device s); a device may appear more than once
 *                (several shards on one GPU: how a single-GPU box tests the path)
 * bbq_shard_scan refuses such a handle.  Extra option: round_queries 1..65536 (512), queries per round. */
int bbq_index_create_multi(const uint8_t *codes, const double *corr, int64_t n_rows, int32_t dim, int32_t index_bits,
                           double centroid_dp, int32_t n_shards, const int32_t *devices, int64_t pilot_rows, bbq_index **out);
int bbq_index_create_multi_opts(const uint8_t *codes, const double *corr, int64_t n_rows, int32_t dim, int32_t index_bits,
                                double centroid_dp, int32_t n_shards, const int32_t *devices, int64_t pilot_rows,
                                const bbq_index_options *opts, bbq_index **out);
/* ------------------------------------------------------------------------------------------
 * Appending rows (new; the reference's index is immutable): the index grows in place.  Rows are independent once the centroid is
 * fixed - quantizeVectors computes the centroid and then calls scalarQuantize row by row (src/binaryQuantizationFormat.ts:214-249) -
 * so "the new rows quantized against the centroid the index was built with" is fully defined by the reference.  After an append the
 * index is indistinguishable from one created whole over the old rows followed by the new ones (same centroid_dp, index_bits,
 * options): size, every search entry point (indices, f32 score bits, order, ties), bbq_index_export and the bytes bbq_index_save
 * writes.  New rows get the next ords, bbq_index_size() ..., in the order given.
 * Strong guarantee: an append that fails - bad argument, NaN / Infinity, a row the layout cannot hold, out of memory - leaves the
 * index exactly as it was.  n == 0: BBQ_OK, nothing changes.  More than 2^32 rows in total: BBQ_ERR_UNSUPPORTED.
 * Out of scope (BBQ_ERR_UNSUPPORTED), as for filters: a multi-device handle, a non-root shard, an index with a pilot replica.
 * The call takes the device context's lock like every entry point and first retires what the index has in flight: a search on
 * another thread sees the index before or after the append, never in between; a bbq_shard_scan_begin batch of this index that has
 * not been waited for: BBQ_ERR_INVALID_ARG.
 * A bbq_filter made BEFORE an append no longer fits the index's size: bbq_search_filtered_batch refuses it (BBQ_ERR_INVALID_ARG);
 * make a new filter over the grown index.
 * Capacity: the allocations hold bbq_index_capacity() rows (whole 64-row tiles).  An append that fits writes in place; one that
 * does not moves the index into allocations of max(tiles needed, 1.5 x tiles held) tiles - a device-to-device copy, the old
 * buffers released after it - so a run of appends costs amortised O(rows appended).  bbq_index_reserve makes room for exactly
 * `rows` rows in total (never shrinks). */
/* rows already quantized, in the shape bbq_index_create takes them (codes [n*ceil(dim/8)] or [n*dim], corr [n*4]).  An index without
 * explicit component sums (compact corrections, or inline with the implicit sum) refuses a row whose quantizedComponentSum is not its
 * popcount / code sum with BBQ_ERR_UNSUPPORTED - holding it would mean re-tiling the whole index; an index that carries explicit sums
 * takes any row.  A multi-bit code >= 2^indexBits: BBQ_ERR_INVALID_ARG, as at creation. */
int bbq_index_append_rows(bbq_index *idx, const uint8_t *codes, const double *corr, int64_t n);
/* raw fp32 rows [n*dim], quantized ON THE DEVICE against `centroid` [dim] (the one the index was built with; the library does not
 * keep it): normalizeVector for COSINE, NaN / Infinity validation, scalarQuantize(indexBits of the index), packAsBinary - what
 * bbq_index_build does after its centroid step; 1-bit rows are quantized straight into their lanes of the tile records.
 * codes_out / corr_out (host, may be NULL): the new rows in the reference's shape.  *bad_row / *bad_col: position inside THIS call's
 * block; messages and codes as bbq_index_build. */
int bbq_index_append(bbq_index *idx, const float *vectors, int64_t n, const float *centroid, int32_t sim, double lambda, int32_t iters,
                     uint8_t *codes_out, double *corr_out, int64_t *bad_row, int32_t *bad_col);
int bbq_index_reserve(bbq_index *idx, int64_t rows);      /* room for `rows` rows in total without another reallocation */
int64_t bbq_index_capacity(const bbq_index *idx);         /* rows the current allocations hold (>= size) */

int32_t bbq_index_shards(const bbq_index *idx);    /* 1 for a single-device index */
void bbq_index_destroy(bbq_index *idx);
int64_t bbq_index_size(const bbq_index *idx);      /* BinarizedByteVectorValues.size()      src/types.ts:46 */
int32_t bbq_index_dimension(const bbq_index *idx); /* BinarizedByteVectorValues.dimension() src/types.ts:34 */
int32_t bbq_index_bits(const bbq_index *idx);      /* indexBits the index was created with (1..8) */
/* bytes of HBM one query sweep reads per row: the figure bench.py prices the roofline with */
int32_t bbq_index_bytes_per_row(const bbq_index *idx);

/* ------------------------------------------------------------------------------------------
 * Search: replaces steps 2-4 of BinaryQuantizationFormat.searchNearestNeighbors
 * (src/binaryQuantizationFormat.ts:349-411): score every row
 * (BinaryQuantizedScorer.computeBatchQuantizedScores, src/binaryQuantizedScorer.ts:315-420;
 * computeBatchFourBitDotProductDirectPacked / computeBatchDotProductDirectPacked;
 * computeBatch{FourBit,OneBit}SimilarityScores src/batchDotProduct.ts:478-617), round to f32,
 * MinHeap top-k (src/minHeap.ts), descending output.  Bit-exact incl. the order among equal scores.
 *
 *   qquant   [dim]   quantized query, one value per dimension (Uint8Array from quantizeQueryVector)
 *   qcorr    [4]     query corrections
 *   query_bits       1 selects the 1-bit formulas, anything else the "4-bit" formulas
 *   out_idx/out_score [k]  (only min(k, size) entries are written); *out_n = number written
 * k == 0 -> *out_n = 0.  k < 0 -> BBQ_ERR_NEGATIVE_K.  k > 4096 is answered by the dense path (every f32 score to the
 * host; 16 ms per 10 M-row query instead of 0.15-4 ms).
 * Multi-bit index (index_bits > 1) with query_bits other than 1 and 4: the reference throws (src/binaryQuantizedScorer.ts:95-97); this
 * entry point scores it with the per-row 4-bit form - integer dot product pinned by fixtures, float score PARITY UNPINNED (the JS and
 * Python hosts throw like the reference).
 */
int bbq_search(bbq_index *idx, const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim,
               int64_t k, int32_t *out_idx, float *out_score, int64_t *out_n);

/* The same for n_queries independent queries (each does its own sweep of the index; the calls are
 * pipelined on the device).  qquant [n_queries*dim], qcorr [n_queries*4], out_idx/out_score
 * [n_queries*k] (row q at offset q*k), out_n [n_queries]. */
int bbq_search_batch(bbq_index *idx, int32_t n_queries, const uint8_t *qquant, const double *qcorr,
                     int32_t query_bits, int32_t sim, int64_t k, int32_t *out_idx, float *out_score,
                     int64_t *out_n);

/* searchNearestNeighbors from the RAW query (src/binaryQuantizationFormat.ts:337-411) for n_queries queries: normalisation (COSINE) +
 * quantizeQueryVector exactly as bbq_quantize_query does them, then bbq_search_batch - but pipelined: the queries are quantized on
 * n_threads host threads (0: half the cores, at most 16) chunk by chunk while the sub-batches in front are already on the device, so
 * the quantizer (~15 us per 768-d query and core) only stands in front of the first sweep.  Results are bit-identical to
 * bbq_quantize_queries followed by bbq_search_batch.
 *   queries [n_queries*dim] raw fp32, centroid [dim] (getCentroid()), lambda / iters: the quantizer's (0.1 / 5 by default in the reference)
 *   qquant_out [n_queries*dim], qcorr_out [n_queries*4]: optional, the quantized queries (what quantizeQueryVector returns)
 *   *bad_query (may be NULL): the first query the quantizer refused (NaN / Infinity input, ...), with its error as the return value */
int bbq_search_raw_batch(bbq_index *idx, int32_t n_queries, const float *queries, const float *centroid, int32_t sim,
                         int32_t query_bits, double lambda, int32_t iters, int32_t n_threads, int64_t k, int32_t *out_idx,
                         float *out_score, int64_t *out_n, uint8_t *qquant_out, double *qcorr_out, int32_t *bad_query);

/* ------------------------------------------------------------------------------------------
 * Filtered search (new; the reference has no filter): exact top-k over a subset A of the rows - rows deleted since the build, one
 * tenant's rows, the rows a metadata predicate accepts.  The result is what the reference's searchNearestNeighbors loop
 * (src/binaryQuantizationFormat.ts:349-411) returns when it visits only the ords in A, ascending, each pushed with its original ord
 * and its f32 score, with a heap of min(k, |A|): indices, score bits and order match bit for bit, ties included
 * (DESIGN.md "Filtered search").  |A| == 0 or k == 0 -> *out_n = 0; k < 0 -> BBQ_ERR_NEGATIVE_K; k > |A| -> |A| results.
 * A filter belongs to ONE single-device index (its size, its device), owns its device memory, is read-only after creation and may
 * be shared by any number of calls and threads.  Using it with an index of another size or device: BBQ_ERR_INVALID_ARG.
 * Out of scope: a multi-device handle (bbq_index_create_multi), a non-root shard and an index with a pilot replica return
 * BBQ_ERR_UNSUPPORTED.  A filtered call takes the pipelined per-query sweep, or with sweep_share 32 the matrix-core shared sweep
 * behind the first k accepted rows (sweep_share 4 / 8 and the latency_* options do not change its path); k > 4096 and force_dense
 * take the dense path over the accepted rows. */
typedef struct bbq_filter bbq_filter;   /* opaque: an accept set of one index, resident on that index's device */
/* accept_bits [ceil(n_rows/64)] little-endian words: row r is accepted iff (accept_bits[r >> 6] >> (r & 63)) & 1; bits at and beyond
 * n_rows are ignored.  n_words must be ceil(bbq_index_size(idx)/64). */
int bbq_filter_create(bbq_index *idx, const uint64_t *accept_bits, int64_t n_words, bbq_filter **out);
/* the same from a list of global row ids (any order, duplicates allowed; a row outside the index: BBQ_ERR_INVALID_ARG) */
int bbq_filter_create_rows(bbq_index *idx, const int32_t *rows, int64_t n, bbq_filter **out);
void bbq_filter_destroy(bbq_filter *f);
int64_t bbq_filter_count(const bbq_filter *f);      /* |A| */
/* Host-only introspection (no device needed): the segments a filtered call sweeps for an index of n_rows rows and this accept set
 * (accept_bits as bbq_filter_create takes them), with rank k_dev (min(k, |A|), + 1 when the device selects the answer) and the options
 * first_segment_rows / segment_growth (bbq_set_option).  segments [max_segments][3] = {first chunk, chunks, candidate slots per chunk}
 * (512-row chunks); *out_n = their number (0: nothing accepted).  What tests/test_filtered_cpu.py holds its numpy restatement to. */
int bbq_filter_plan(const uint64_t *accept_bits, int64_t n_rows, int64_t k_dev, int64_t first_segment_rows, int32_t growth,
                    int32_t max_segments, int64_t *segments, int32_t *out_n);
/* bbq_search_batch restricted to f (arguments and outputs as bbq_search_batch); one filter serves all queries of the call */
int bbq_search_filtered_batch(bbq_index *idx, const bbq_filter *f, int32_t n_queries, const uint8_t *qquant, const double *qcorr,
                              int32_t query_bits, int32_t sim, int64_t k, int32_t *out_idx, float *out_score, int64_t *out_n);

/* ------------------------------------------------------------------------------------------
 * Removing rows (new; the reference's index is immutable): a compaction makes the index the index over the rows a filter accepts,
 * in order, without the rows leaving the device.  New ord of old row r = the number of accepted rows below r.  After
 * bbq_index_compact(idx, f) the index is indistinguishable from one created whole (bbq_index_create_opts) over the kept rows with
 * the same centroid_dp, index_bits and options: bbq_index_size == bbq_filter_count(f), bbq_index_capacity is whole tiles of exactly
 * that many rows, every search entry point (indices, f32 score bits, order, ties), bbq_score_rows, rerank, bbq_shard_scan* on a root
 * index, filtered search with a filter made afterwards, bbq_index_export, the bytes bbq_index_save writes (padding lanes of the last
 * tile and every tile's add range included), and a later append.
 * The record format is never re-decided by a compaction.  An index without explicit component sums - every built index and the
 * normal created one - has its files equal the twin's unconditionally.  An index that stores explicit sums keeps storing them: its
 * files equal the twin's exactly when the twin's own creation decides to store them, that is when a kept row still needs it; its
 * answers and its export always match.
 * Every row kept (|A| == size): BBQ_OK and nothing changes, capacity included.  |A| == 0: the index of zero rows.
 * Strong guarantee: a call that fails - a filter of another size or device (BBQ_ERR_INVALID_ARG), out of memory (BBQ_ERR_OOM), a
 * bbq_shard_scan_begin batch of this index that has not been waited for (BBQ_ERR_INVALID_ARG) - leaves the index exactly as it was.
 * The rows are gathered OUT OF PLACE into new allocations and the old ones are released behind the gather: the peak is old + new,
 * and afterwards the memory of the removed rows is free.
 * Out of scope (BBQ_ERR_UNSUPPORTED), as for filters and appends: a multi-device handle, a non-root shard, an index with a pilot
 * replica.  Re-centring is not offered (giving an ord new contents: "Replacing rows" below).  The call takes the device context's lock and first retires what
 * the index has in flight, as an append does.
 * The filter used, and any filter made earlier, no longer fits the new size: bbq_search_filtered_batch refuses it
 * (BBQ_ERR_INVALID_ARG); make a new filter over the compacted index. */
/* keep the rows f accepts, ascending; new ord of old row r = number of accepted rows below r */
int bbq_index_compact(bbq_index *idx, const bbq_filter *f);
/* convenience: drop these ords (any order, duplicates allowed; a row outside the index: BBQ_ERR_INVALID_ARG) */
int bbq_index_remove_rows(bbq_index *idx, const int32_t *rows, int64_t n);
/* host-only, no device: the accepted ords ascending = the old ord of every new row.  accept_bits as bbq_filter_create takes them
 * (bits at and beyond n_rows are ignored), out_rows [cap]; *out_n = |A| even when cap is too small (then BBQ_ERR_INVALID_ARG and
 * nothing is written) */
int bbq_filter_kept_rows(const uint64_t *accept_bits, int64_t n_rows, int32_t *out_rows, int64_t cap, int64_t *out_n);

/* ------------------------------------------------------------------------------------------
 * Replacing rows (new; the reference's index is immutable): an existing ord gets new contents, in place.  The ord is the id every
 * caller holds; "row r replaced by v quantized against the centroid the index was built with" is defined by the reference exactly
 * as an appended row is.  After an update the index is indistinguishable from one created whole (bbq_index_create_opts) over the
 * same rows with the rows at ords[i] replaced, with the same centroid_dp, index_bits and options: bbq_index_size and
 * bbq_index_capacity (both unchanged), every search entry point (indices, f32 score bits, order, ties), bbq_score_rows, rerank
 * (together with bbq_vectors_update), bbq_shard_scan* on a root index, bbq_index_export, the bytes bbq_index_save writes (the
 * untouched lanes, the padding lanes of the last tile and every touched tile's add range included), and a later append or
 * compaction.
 * Filters: the size does not change, so a bbq_filter made BEFORE an update still fits and still means the same ords;
 * bbq_search_filtered_batch with it answers over the updated rows.
 * Duplicates: among equal ords in one call the last one wins, as applying the block in order would; every row of the block is
 * still validated, losers included.  n == 0: BBQ_OK, nothing changes.  An ord equal to the size is not an append: out of range.
 * Strong guarantee: a call that fails - an ord outside [0, size) (BBQ_ERR_INVALID_ARG), NaN / Infinity (codes, messages and
 * *bad_row / *bad_col as bbq_index_append, positions inside this call's block), a multi-bit code >= 2^indexBits
 * (BBQ_ERR_INVALID_ARG), a row the record format cannot hold (BBQ_ERR_UNSUPPORTED), out of memory for the scratch (BBQ_ERR_OOM),
 * a bbq_shard_scan_begin batch of this index that has not been waited for (BBQ_ERR_INVALID_ARG) - has not written a byte the index
 * can see, not even in a padding lane: the block is staged, quantized and checked in scratch memory first, and the writes that
 * follow go into allocations that already exist.
 * The record format is never re-decided, as in a compaction.  An index without explicit component sums refuses a row whose
 * quantizedComponentSum is not its popcount / code sum (BBQ_ERR_UNSUPPORTED, as an append does).  An index that stores explicit
 * sums takes any row and keeps storing them: its files equal the twin's exactly when the twin's own creation decides to store
 * them; its answers and its export always match.
 * Out of scope (BBQ_ERR_UNSUPPORTED), as for appends: a multi-device handle, a non-root shard, an index with a pilot replica.
 * Re-centring is not offered.  The call takes the device context's lock and first retires what the index has in flight, as an
 * append does. */
/* rows already quantized, shapes as bbq_index_append_rows; ords [n] */
int bbq_index_update_rows(bbq_index *idx, const int32_t *ords, const uint8_t *codes, const double *corr, int64_t n);
/* raw fp32 rows [n*dim] quantized ON THE DEVICE against `centroid`, arguments as bbq_index_append; codes_out / corr_out (host, may be
 * NULL) get all n rows of the block, duplicate losers included.  (bbq_vectors_update, below, is the fp32 side of the rerank recipe.) */
int bbq_index_update(bbq_index *idx, const int32_t *ords, const float *vectors, int64_t n, const float *centroid, int32_t sim,
                     double lambda, int32_t iters, uint8_t *codes_out, double *corr_out, int64_t *bad_row, int32_t *bad_col);
/* host only, no device: which entries of an update block take effect.  out_pos [cap] = positions i into the block, ascending by
 * ords[i], one per distinct ord - the LAST occurrence; *out_n = their number even when cap is too small (then BBQ_ERR_INVALID_ARG,
 * nothing written).  An ord outside [0, n_rows): BBQ_ERR_INVALID_ARG. */
int bbq_update_winners(const int32_t *ords, int64_t n, int64_t n_rows, int64_t *out_pos, int64_t cap, int64_t *out_n);

/* Per-row results of computeBatchQuantizedScores (src/binaryQuantizedScorer.ts:389-400) for the
 * contiguous ords [row_begin, row_begin+row_count): bitDotProduct (integer qcDist), the f64 score and
 * its f32 rounding (src/binaryQuantizationFormat.ts:353,378).  Any output pointer may be NULL. */
int bbq_score_rows(bbq_index *idx, const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim,
                   int64_t row_begin, int64_t row_count, int32_t *out_qcdist, double *out_score64,
                   float *out_score32);

/* ------------------------------------------------------------------------------------------
 * Scoring chosen rows (DESIGN.md "Scoring chosen rows"): computeBatchQuantizedScores(query, corrections, targetVectors, targetOrds,
 * queryBits) (src/binaryQuantizedScorer.ts:315-420) for an ARBITRARY list of ords per query - a graph or IVF layer's neighbours, a
 * metadata pre-filter's short candidate list, a tenant list that differs from query to query, another system's candidates.  The
 * device gathers exactly the rows named: two ords at opposite ends of the index cost two rows, not the range between them.
 * For every list position i of query q, out_*[i] is bit for bit what bbq_score_rows returns for row ords[i] with that query (integer
 * qcDist, f64 score, its f32 rounding; a NaN score is delivered as NaN).  Any order of ords, duplicates allowed: each occurrence is
 * scored.  offsets [n_queries + 1] ascending from 0, as bbq_rerank_scores takes them.  query_bits, sim and the multi-bit corners as
 * bbq_score_rows.
 * Nothing is written and nothing is launched when an argument is bad, when n_queries == 0 or when offsets[n_queries] == 0 (the last
 * two: BBQ_OK).  An ord outside [0, bbq_index_size): BBQ_ERR_INVALID_ARG, "向量索引 <ord> 不存在" naming the first offending entry in
 * list order (what the reference's loop throws on); every list is checked on the host before the first launch.
 * Accepted handles: a single-device index - also a non-root shard or one with a pilot replica; ords are positions among the handle's
 * own rows, as row_begin of bbq_score_rows is - and a multi-device handle (the lists are split by shard on the host).  The call takes
 * the device context's lock and runs on the auxiliary stream, as bbq_score_rows does: it sees an append, a compaction or an update
 * whole or not at all.  A long call is worked through in launches of at most 2^20 entries and 1024 queries: the device scratch stays
 * below 21 MiB whatever the call's size. */
/* n_queries queries at once: query q is scored against ords[offsets[q] .. offsets[q+1]).  Outputs are indexed like ords; any output
 * pointer may be NULL. */
int bbq_score_ords_batch(bbq_index *idx, int32_t n_queries, const uint8_t *qquant, const double *qcorr,
                         int32_t query_bits, int32_t sim, const int64_t *offsets, const int32_t *ords,
                         int32_t *out_qcdist, double *out_score64, float *out_score32);
/* one query, one list of n ords */
int bbq_score_ords(bbq_index *idx, const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim,
                   const int32_t *ords, int64_t n, int32_t *out_qcdist, double *out_score64, float *out_score32);
/* exact top-k over each query's own list: what the reference loop (src/binaryQuantizationFormat.ts:349-411) returns when it visits
 * ords[offsets[q] .. offsets[q+1]) IN THE ORDER GIVEN, pushing (ord, f32 score) into a heap of min(k, list length) - indices, score
 * bits and order, ties included, whatever the list's order; a duplicate is visited once per occurrence.  out_idx / out_score
 * [n_queries*k] (query q at offset q*k), out_n [n_queries].  k < 0: BBQ_ERR_NEGATIVE_K; k == 0 or an empty list: out_n[q] = 0 (out_n is
 * written whenever the arguments are good, also when every list is empty); no upper limit on k.  The device delivers the f32 scores,
 * the host runs the literal heap over them on replay_threads threads. */
int bbq_search_ords_batch(bbq_index *idx, int32_t n_queries, const uint8_t *qquant, const double *qcorr,
                          int32_t query_bits, int32_t sim, int64_t k, const int64_t *offsets, const int32_t *ords,
                          int32_t *out_idx, float *out_score, int64_t *out_n);

/* ------------------------------------------------------------------------------------------
 * Range search (DESIGN.md "Range search"): every row whose score reaches a threshold - the query whose k the caller does not know.
 * For query q with threshold t_q (an f32) the answer is every row r of the index that the filter, if one is given, accepts and whose
 * f32 score - what bbq_score_rows delivers as out_score32 - satisfies score >= t_q as IEEE floats compare, delivered in ascending ord,
 * each with that score: what the reference's loop (src/binaryQuantizationFormat.ts:349-411) would collect if it kept every visited ord
 * whose stored f32 score is >= t and skipped the heap.  A row whose score is NaN is in no answer, whatever the threshold; t = -inf
 * returns every accepted row with a non-NaN score, t = +inf the rows whose score is +inf, t = +0.0 and t = -0.0 the same answer.  A NaN
 * threshold is BBQ_ERR_INVALID_ARG, checked for all queries before the first launch.  query_bits, sim and the multi-bit corners as
 * bbq_score_rows.
 * n_queries == 0, an index of zero rows and an empty filter: BBQ_OK with zeros, nothing is launched.  Accepted handles are those the
 * filtered search accepts - a single-device root index without a pilot replica; a multi-device handle, a non-root shard and an index
 * with a pilot replica: BBQ_ERR_UNSUPPORTED, with or without a filter.  The call takes the device context's lock and runs on the
 * auxiliary stream, as bbq_score_rows and bbq_score_ords do: it sees an append, an update or a compaction whole or not at all.  It
 * writes no bbq_stats field.  The sweep is count-then-fill and deterministic; a long call is worked through in sub-batches of at most
 * 1024 queries and 64 MiB of per-chunk scratch and in fill launches of at most 2^20 entries (always at least one query): the device
 * scratch stays below 64 MiB + max(8 MiB, 8 B x rows) + the staged queries.  A failed allocation: BBQ_ERR_OOM, nothing written. */
/* host only: *out_key = K with  bbq_key_of_score(s) > K  <=>  s >= threshold  for every non-NaN s
 * (bbq_key_of_score(t) - 1 with t = +-0 taken as -0.0f).  NaN: BBQ_ERR_INVALID_ARG. */
int bbq_range_key(float threshold, uint32_t *out_key);
/* f: NULL = all rows; otherwise a filter of this index (size / device as bbq_search_filtered_batch checks them).
 * thresholds [n_queries].  out_counts [n_queries] = number of rows in each answer. */
int bbq_count_range_batch(bbq_index *idx, const bbq_filter *f, int32_t n_queries, const uint8_t *qquant, const double *qcorr,
                          int32_t query_bits, int32_t sim, const float *thresholds, int64_t *out_counts);
/* out_offsets [n_queries + 1] ascending from 0: query q's answer is out_idx / out_score [out_offsets[q], out_offsets[q+1]),
 * ascending by ord.  cap = entries out_idx / out_score hold.  out_offsets is written whenever the arguments are good; when
 * out_offsets[n_queries] > cap: BBQ_ERR_INVALID_ARG and nothing is written to out_idx / out_score (the precedent is
 * bbq_filter_kept_rows) - the caller allocates and calls again.  out_idx / out_score may be NULL iff cap == 0. */
int bbq_search_range_batch(bbq_index *idx, const bbq_filter *f, int32_t n_queries, const uint8_t *qquant, const double *qcorr,
                           int32_t query_bits, int32_t sim, const float *thresholds, int64_t cap,
                           int64_t *out_offsets, int32_t *out_idx, float *out_score);

/* ------------------------------------------------------------------------------------------
 * Span search (DESIGN.md "Span search"): exact top-k over a few contiguous runs of rows that differ from query to query - a coarse
 * quantizer's probed clusters in a store that keeps its rows cluster by cluster, one tenant's block per query, a time window.
 * Query q's spans are spans[2 j], spans[2 j + 1] = begin, end (exclusive) for j in [span_offsets[q], span_offsets[q + 1]); its answer
 * is what the reference loop (src/binaryQuantizationFormat.ts:349-411) returns when it visits exactly the rows of those spans,
 * ascending, pushing (ord, f32 score) into a heap of min(k, L_q), L_q = the total length of q's spans - indices, score bits and order,
 * ties and NaN scores included: the answer of bbq_search_ords_batch over the expanded list and of bbq_search_filtered_batch with a
 * filter of the span union.  The scores are bit for bit those of bbq_score_rows; query_bits, sim and the multi-bit corners as there.
 * Spans: 0 <= begin <= end <= bbq_index_size, ascending and disjoint within a query (end_j <= begin_{j+1}); empty spans and empty
 * lists are allowed.  A violation is BBQ_ERR_INVALID_ARG and the message names the first offending (query, span) in call order; every
 * list is checked on the host before the first launch: nothing is launched and nothing is written.
 * out_idx / out_score [n_queries*k] (query q at offset q*k), out_n [n_queries], as bbq_search_batch.  k < 0: BBQ_ERR_NEGATIVE_K;
 * k == 0 or L_q == 0: out_n[q] = 0 (out_n is written whenever the arguments are good); no upper limit on k; n_queries == 0: BBQ_OK,
 * nothing is launched.
 * out_status [n_queries] (may be NULL): 0 - the device selected the answer, 1 - the host ran the literal heap over the device's scores
 * of all of q's span rows.  It is 0 EXACTLY when L_q > k, 1 <= k <= 4096, no visited row's score is NaN and no two of the k + 1 largest
 * visited scores compare equal as floats (+0.0 == -0.0): the condition under which the heap provably returns the k best in descending
 * order.  0 as well for a query with k == 0 or L_q == 0.
 * Accepted handles as for filters and the range search: a single-device root index without a pilot replica; anything else is
 * BBQ_ERR_UNSUPPORTED.  The call takes the device context's lock and runs on the auxiliary stream: it sees an append, an update or a
 * compaction whole or not at all.  It writes no bbq_stats field.  A long call is worked through in sub-batches of at most 1024 queries
 * and 64 MiB of scores (always at least one query).  A failed allocation: BBQ_ERR_OOM, nothing written.  A filter combined with
 * spans: bbq_search_spans_filtered_batch below.  Out of scope: spans in any other order. */
int bbq_search_spans_batch(bbq_index *idx, int32_t n_queries, const uint8_t *qquant, const double *qcorr,
                           int32_t query_bits, int32_t sim, int64_t k,
                           const int64_t *span_offsets, const int64_t *spans,
                           int32_t *out_idx, float *out_score, int64_t *out_n, uint8_t *out_status);
/* Filtered span search (DESIGN.md "Filtered span search"): the span search over the rows a filter accepts - deletions, one tenant's
 * rows or a metadata predicate in a store that keeps its rows cluster by cluster.  Query q's answer is what the reference loop returns
 * when it visits exactly the rows of q's spans that f accepts, ascending, pushing (original ord, f32 score) into a heap of
 * min(k, A_q), A_q = the number of accepted rows in q's spans - indices, score bits and order, ties and NaN scores included: the answer
 * of bbq_search_filtered_batch with a filter of (f AND the span union) and of bbq_search_ords_batch over the accepted ords of the spans;
 * the scores are those of bbq_score_rows.
 * f: a filter of this index, checked as bbq_search_filtered_batch checks it (another size - a filter made before an append, a removal
 * or a compaction - or another device: BBQ_ERR_INVALID_ARG); NULL = all rows: the call is bbq_search_spans_batch, same answers and same
 * statuses.  Spans, offsets, k, n_queries == 0 and null arguments are checked as there, the messages carry this function's name and
 * name the first offending (query, span).  Every check runs under the context's lock before the first launch: nothing is launched and
 * nothing is written.  k == 0 or A_q == 0: out_n[q] = 0, status 0.
 * out_status follows the span search's rule with the accepted rows in place of the visited rows: 0 EXACTLY when A_q > k,
 * 1 <= k <= 4096, no accepted visited row's score is NaN and no two of the k + 1 largest accepted scores compare equal as floats.  A
 * NaN score on a rejected row changes nothing.
 * Handles, lock, stream and bbq_stats as for the span search.  Sub-batches hold at most 1024 queries and 64 MiB of scratch, 8 bytes per
 * accepted row (its score and its ord), always at least one query; a work item without an accepted row is never launched.  A failed
 * allocation: BBQ_ERR_OOM, nothing written.  Out of scope: a filter per query, spans in any other order. */
int bbq_search_spans_filtered_batch(bbq_index *idx, const bbq_filter *f, int32_t n_queries, const uint8_t *qquant, const double *qcorr,
                                    int32_t query_bits, int32_t sim, int64_t k,
                                    const int64_t *span_offsets, const int64_t *spans,
                                    int32_t *out_idx, float *out_score, int64_t *out_n, uint8_t *out_status);

/* ------------------------------------------------------------------------------------------
 * Grouped search (DESIGN.md "Grouped search"): the k best GROUPS of rows, each through its best row - the k best documents of a store
 * that holds a document as a run of chunk rows (Lucene's diversifying-children kNN query) - exact, in one call, on the device.
 * A group set belongs to ONE single-device root index, as a filter does.  group_offsets [n_groups + 1]: group g is the rows
 * [group_offsets[g], group_offsets[g + 1]); group_offsets[0] == 0, ascending (equal neighbours: an empty group), and
 * group_offsets[n_groups] == bbq_index_size(idx).  Anything else is BBQ_ERR_INVALID_ARG.  f (may be NULL: every row): a filter of this
 * index, checked as bbq_search_filtered_batch checks it; rows it rejects are never visited.  The group set copies the filter's words:
 * the filter may be destroyed before the group set.  A group is LIVE if it has at least one accepted row; L = bbq_groups_live is the
 * same for every query.  The device tables - a 64-bit word of group starts and a group number per tile, a slot per non-empty group,
 * about 0.2 bytes per row - are built here, once.  At most 2^31 - 1 rows and groups.
 * A query's REPRESENTATIVE of a live group is its accepted row with the greatest f32 score (bbq_score_rows' score), where a NaN score
 * ranks below every number, numbers rank in the order of bbq_key_of_score (-0.0 below +0.0) and among rows of equal rank the lowest
 * ord wins; a group whose accepted rows all score NaN is represented by the lowest of them, with a NaN score.
 * bbq_search_grouped_batch: query q's answer is what the reference loop (src/binaryQuantizationFormat.ts:349-411) returns when it visits
 * exactly the L representatives, ascending by ord, pushing (original ord, f32 score) into a heap of min(k, L) - the answer of
 * bbq_search_ords_batch over the representatives: indices, score bits and order, ties and NaN included.
 * out_idx / out_score [n_queries*k] (query q at offset q*k), out_n [n_queries], as bbq_search_batch; out_group [n_queries*k] (may be
 * NULL): the group of each answer row.  k < 0: BBQ_ERR_NEGATIVE_K; k == 0 or L == 0: out_n[q] = 0; k > L: L results; no upper limit on k.
 * out_status [n_queries] (may be NULL) follows the span search's rule over the representatives' scores: 0 - the device selected the
 * answer - EXACTLY when L > k, 1 <= k <= 4096, no representative is NaN and no two of the k + 1 largest compare equal as floats;
 * otherwise 1 - the host ran the literal heap over the device's representatives.  0 as well for k == 0 or L == 0.
 * A group set made for another size or device (used after an append, a removal or a compaction): BBQ_ERR_INVALID_ARG, nothing launched,
 * nothing written; after an in-place update it still serves.  A multi-device handle, a non-root shard or an index with a pilot
 * replica: BBQ_ERR_UNSUPPORTED.  The call takes the device context's lock, runs on the auxiliary stream and writes no bbq_stats field.
 * Every query streams the whole index - nothing is pruned.  A long call is worked through in sub-batches of at most 1024 queries and
 * group_scratch_mb (bbq_set_option) of representatives, always at least one query.  A failed allocation: BBQ_ERR_OOM, nothing written.
 * Results are byte-identical from run to run.  Out of scope: persisted group sets, a group set per query, groups that are not
 * contiguous runs of rows, a sweep pruned by a bound on the k-th best group. */
typedef struct bbq_groups bbq_groups;   /* opaque: the groups of one index, resident on that index's device */
int bbq_groups_create(bbq_index *idx, const int64_t *group_offsets, int64_t n_groups, const bbq_filter *f, bbq_groups **out);
void bbq_groups_destroy(bbq_groups *g);
int64_t bbq_groups_count(const bbq_groups *g);   /* n_groups */
int64_t bbq_groups_live(const bbq_groups *g);    /* L */
/* Host only, no device: validates the offsets as bbq_groups_create does against n_rows rows; out_slot [n_groups]: the rank of group g
 * among the live groups, or -1; *out_live = L.  accept_bits as bbq_filter_create takes them, or NULL: every row. */
int bbq_groups_plan(const int64_t *group_offsets, int64_t n_groups, int64_t n_rows, const uint64_t *accept_bits,
                    int32_t *out_slot, int64_t *out_live);
int bbq_search_grouped_batch(bbq_index *idx, const bbq_groups *g, int32_t n_queries, const uint8_t *qquant, const double *qcorr,
                             int32_t query_bits, int32_t sim, int64_t k,
                             int32_t *out_idx, int32_t *out_group, float *out_score, int64_t *out_n, uint8_t *out_status);

/* ------------------------------------------------------------------------------------------
 * MaxSim search (DESIGN.md "MaxSim search"): the k best GROUPS of a group set for queries that are bags of token vectors - the
 * late-interaction score of ColBERT / ColPali, Lucene's late-interaction field, Elasticsearch's rank_vectors over bit-quantized
 * vectors - exact, in one call, summed on the device.  Query q owns the token vectors [vec_offsets[q], vec_offsets[q + 1]) of the
 * n_vectors = vec_offsets[n_queries] vectors in qquant / qcorr, which are laid out as bbq_search_batch lays out n_vectors queries.
 * vec_offsets [n_queries + 1]: vec_offsets[0] == 0, ascending, and every query has at least one vector; anything else is
 * BBQ_ERR_INVALID_ARG naming the first offending query, with nothing launched and nothing written.
 * For a live group and token t, m_t is the f32 score of that token vector's REPRESENTATIVE of the group, exactly as the grouped
 * search defines it (a NaN score if all accepted rows of the group score NaN).  The group's score is
 *   S = (float)((double)m_0 + (double)m_1 + ...)
 * - the f64 adds strictly in ascending t, starting from m_0 and not from 0.0 (a single -0.0 stays -0.0), one rounding to f32 at the
 * end, no contraction, no reassociation; a NaN m_t makes S NaN.  bbq_maxsim_reduce (host only, no device) is this sum in plain C over
 * rep_scores[t * n_groups + slot] -> out [n_groups], n_vectors >= 1: the normative statement.
 * bbq_search_maxsim_batch: query q's answer is what the reference loop (src/binaryQuantizationFormat.ts:349-411) returns when it visits
 * exactly the L live groups in ascending group number, pushing (group number, S) into a heap of min(k, L): group numbers, score bits
 * and order, ties and NaN included.  out_group / out_score [n_queries*k] (query q at offset q*k), out_n [n_queries].  k < 0:
 * BBQ_ERR_NEGATIVE_K; k == 0 or L == 0: out_n[q] = 0; k > L: L results; n_queries == 0: BBQ_OK, nothing launched.
 * out_status [n_queries] (may be NULL) is the span search's rule over the S values: 0 - the device selected the answer - EXACTLY when
 * L > k, 1 <= k <= 4096, no S is NaN and no two of the k + 1 largest compare equal as floats; otherwise 1 - the host ran the literal
 * heap over the device's S in slot order.  0 as well for k == 0 or L == 0.
 * With one vector per query the groups, score bits, order and statuses are those of bbq_search_grouped_batch.
 * Handles, lock and stream as bbq_search_grouped_batch: a group set made for another size or device is BBQ_ERR_INVALID_ARG, nothing
 * launched, nothing written; a multi-device handle, a non-root shard or an index with a pilot replica is BBQ_ERR_UNSUPPORTED; the call
 * takes the device context's lock, runs on the auxiliary stream and writes no bbq_stats field.  Every token vector scores the whole
 * index - nothing is pruned.  A query's tokens are worked through in blocks of at most bbq_maxsim_token_block() tokens, whose keys cost
 * 8 bytes per token of the block and live group - not per token of the query; a long call in sub-batches of at most 1024 queries and
 * group_scratch_mb (bbq_set_option) of scratch, always at least one query and one token block.  A failed allocation: BBQ_ERR_OOM,
 * nothing written.  Results are byte-identical from run to run and under either value of maxsim_fused (bbq_set_option).
 * Out of scope: returning each answer's per-token best rows, a group set per query, per-token weights, any pruning. */
int bbq_search_maxsim_batch(bbq_index *idx, const bbq_groups *g, int32_t n_queries, const int64_t *vec_offsets,
                            const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim, int64_t k,
                            int32_t *out_group, float *out_score, int64_t *out_n, uint8_t *out_status);
int bbq_maxsim_reduce(const float *rep_scores, int64_t n_vectors, int64_t n_groups, float *out);   /* host only */
int32_t bbq_maxsim_token_block(void);   /* tokens of a block, the same for every index */

/* ------------------------------------------------------------------------------------------
 * MaxSim over chosen groups (DESIGN.md "MaxSim over chosen groups"): the second stage of late interaction.  A first stage - one of
 * this library's searches per token, a grouped or a span search, another system - nominates candidate groups per query; these two
 * calls score and rank exactly those.  Queries, vec_offsets, qquant / qcorr, query_bits, sim and the multi-bit corners are exactly as
 * bbq_search_maxsim_batch takes them, with the same checks and wording under this function's name.
 * cand_offsets [n_queries + 1]: cand_offsets[0] == 0, ascending, equal neighbours = an empty list; query q's candidates are the group
 * numbers cand_groups[cand_offsets[q] .. cand_offsets[q + 1]) of the group set g, in any order; a duplicate is scored and visited once
 * per occurrence.  A group number outside [0, bbq_groups_count(g)) or a group that is not live - it is empty, or g's filter rejects
 * every one of its rows - is BBQ_ERR_INVALID_ARG naming the first offending (query, position, group) in call order: every list is
 * checked on the host, under the context's lock, before the first launch, with nothing launched and nothing written.
 * bbq_score_maxsim_groups_batch: out_score[i] (indexed like cand_groups) is, bit for bit, the S bbq_search_maxsim_batch defines for
 * group cand_groups[i] and that query - per token the representative's f32 score by the grouped search's rule over the group's
 * accepted rows, the f64 adds strictly in ascending token from m_0, one rounding at the end, a NaN m_t makes S NaN; bbq_maxsim_reduce
 * stays the normative statement of the sum.
 * bbq_search_maxsim_groups_batch: query q's answer is what the reference loop (src/binaryQuantizationFormat.ts:349-411) returns when
 * it visits q's candidates IN THE ORDER GIVEN, pushing (group number, S) into a heap of min(k, list length): group numbers, score bits
 * and order, ties and NaN included, whatever the list's order.  out_group / out_score [n_queries*k] (query q at offset q*k), out_n
 * [n_queries].  k < 0: BBQ_ERR_NEGATIVE_K; k == 0 or an empty list: out_n[q] = 0; no upper limit on k.  The device delivers the S
 * values and the host runs the literal heap on replay_threads threads (bbq_set_option), as bbq_search_ords_batch does: there is no
 * out_status.  n_queries == 0 or cand_offsets[n_queries] == 0: BBQ_OK, nothing launched (the search call still writes out_n).
 * Handles, lock, stream, bbq_stats and stale group sets as bbq_search_maxsim_batch: a group set made for another size or device is
 * BBQ_ERR_INVALID_ARG; a multi-device handle, a non-root shard or an index with a pilot replica is BBQ_ERR_UNSUPPORTED; after an
 * in-place update the set still serves.  What travels to the device is one 8-byte record per candidate, never a row list, and what
 * comes back is one f32 per candidate.  The rows of one query's candidates, duplicates counted, may number at most 2^31 - 1
 * (BBQ_ERR_INVALID_ARG).  A long call is worked through in sub-batches of at most 1024 queries and group_scratch_mb (bbq_set_option) of
 * scratch - 8 bytes per token of a block and 12 per query, per entry of the call's longest list - always at least one query and one
 * token block; the scratch does not grow with the call.  A failed allocation: BBQ_ERR_OOM, nothing written.  Results are
 * byte-identical from run to run.
 * Out of scope: a device-side select over the candidates, returning the per-token best rows, per-token weights, candidates given as
 * row spans or ord lists instead of groups of a group set, multi-device handles and shards, any pruning. */
int bbq_score_maxsim_groups_batch(bbq_index *idx, const bbq_groups *g, int32_t n_queries, const int64_t *vec_offsets,
                                  const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim,
                                  const int64_t *cand_offsets, const int32_t *cand_groups, float *out_score);
int bbq_search_maxsim_groups_batch(bbq_index *idx, const bbq_groups *g, int32_t n_queries, const int64_t *vec_offsets,
                                   const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim, int64_t k,
                                   const int64_t *cand_offsets, const int32_t *cand_groups,
                                   int32_t *out_group, float *out_score, int64_t *out_n);

/* ------------------------------------------------------------------------------------------
 * Sharded search (one process per GPU).  bbq_shard_scan sweeps THIS shard for n_queries queries and
 * leaves the shard's candidates - per query a superset of the rows that ever enter the reference's heap,
 * ascending by global row - PACKED in caller-provided DEVICE memory, so the host framework can move them
 * over RCCL; bbq_replay_batch then replays the reference heap
 * (src/binaryQuantizationFormat.ts:383-411) over all shards' lists in shard order.
 *
 *   dev_packed   device pointer, [packed_cap] bbq_cand; query q's entries at [offsets[q], offsets[q+1])
 *   dev_offsets  device pointer, [n_queries + 1] int64
 *   dev_flags    device pointer, [n_queries] int32; non-zero: this shard could not bound the query
 *                (NaN score / more candidates than every buffer holds) - it carries no entries and the query must be
 *                scored densely
 *   *out_total   (host) number of entries written = offsets[n_queries]
 *   k            1..4096
 * The call returns after the device work has completed (buffers are ready for a collective).
 * A query may leave more than bbq_shard_list_cap entries (a flood: rows stored cluster by cluster); as long as the sum over
 * the batch fits packed_cap nothing is dropped, otherwise the flooded queries are flagged.  BBQ_ERR_OOM only if packed_cap is
 * smaller than n_queries x bbq_shard_list_cap and the entries still do not fit.
 */
int bbq_shard_scan(bbq_index *idx, int32_t n_queries, const uint8_t *qquant, const double *qcorr,
                   int32_t query_bits, int32_t sim, int64_t k, void *dev_packed, int64_t packed_cap,
                   void *dev_offsets, void *dev_flags, int64_t *out_total);
/* The same, asynchronous, with SHARD-LOCAL ANSWERS (ABI 3).  bbq_shard_scan_begin enqueues the whole sweep of the batch - and, behind
 * it on the device, the packing - and returns without waiting; the queries are copied before it returns.  A second begin may follow
 * before the first has been waited for (two batches in flight per index: the device never drains between batches); waits are taken in
 * begin order.  bbq_shard_scan_wait blocks until everything the batch wrote is ready and reports the packed total.
 * bbq_shard_scan == begin + wait without answers.
 *
 *   dev_answers     device pointer (NULL: lists only; must be NULL for k > 1024), [n_queries][answers_stride] uint64, answers_stride >= k + 3.
 *                   Per query:
 *       [0]  entries in the packed list | flags << 32
 *       [1]  m = number of answer entries | unproven << 32   (unproven != 0: flags, or more keys than the launch can select among - take the packed list)
 *       [2]  cut: a monotone key (bbq_key_of_score), at most that of the (k+1)-th largest f32 score among ALL rows this shard has seen -
 *            its own and its pilot replica's - and equal to it unless an earlier segment overflowed the key buffer (a flood: the
 *            running top keys are then those of the entries that fitted, a subset of the rows seen; more than k own rows can lie above
 *            such a cut, and the block is then left unproven); 0 when the shard has seen at most k rows
 *       [3 .. 3+m)  the shard's OWN rows whose score key is above the cut, (row << 32 | f32 bits), descending by score (m <= k)
 *   The cut never exceeds the key of the global (k+1)-th largest score (it is an order statistic of a subset of the rows) and a proven
 *   block holds every own row above its cut, so the union of all shards' answer entries contains every row above max(cut):
 *   bbq_merge_answers selects the global answer from them and proves it (DESIGN.md "Exact top-k": when no two of the k+1 largest
 *   scores compare equal the reference heap returns exactly the k best rows in descending order, whatever its history); only for a
 *   query it cannot prove are the packed lists needed (heap replay).
 *   What travels per shard and query is (k + 3) x 8 bytes instead of the ~1.1 K-entry list.
 */
int bbq_shard_scan_begin(bbq_index *idx, int32_t n_queries, const uint8_t *qquant, const double *qcorr,
                         int32_t query_bits, int32_t sim, int64_t k, void *dev_packed, int64_t packed_cap,
                         void *dev_offsets, void *dev_flags, void *dev_answers, int64_t answers_stride);
int bbq_shard_scan_wait(bbq_index *idx, int64_t *out_total);
/* Host-only: the global answers from the shards' answer blocks.  answers[s] = source s's block ([n_queries][strides[s]] uint64 as above,
 * in HOST memory), sources in any order.  n_total = global number of rows; out_idx / out_score [n_queries * k]; out_n [n_queries].
 * status[q]: 0 = answered (bit-identical to the reference's heap), 1 = not provable from the answers (equal scores in or at the edge of
 * the answer, an unproven source): replay the heap over the packed lists (bbq_replay_batch), 2 = a source flagged the query: it needs
 * the dense path.  out_* of queries with status != 0 are left untouched. */
int bbq_merge_answers(int32_t n_sources, const uint64_t *const *answers, const int64_t *strides, int32_t n_queries, int64_t n_total,
                      int64_t k, int32_t n_threads, int32_t *out_idx, float *out_score, int64_t *out_n, uint8_t *status);
/* the monotone key of an f32 score: larger score <=> larger key (NaN excluded); what cuts and thresholds are expressed in */
uint32_t bbq_key_of_score(float score);
/* planned entries ONE query leaves on this shard, with a 4x margin (use n_queries x this for packed_cap) */
int64_t bbq_shard_list_cap(const bbq_index *idx, int64_t k);

/* Host-only (no device needed): exact replay of the reference heap over candidate lists.
 *   lists[i] / counts[i]  i = 0..n_lists-1, in ascending shard order; entries ascending by row
 *   n_total               global number of rows (k2 = min(k, n_total))
 */
int bbq_replay(int32_t n_lists, const bbq_cand *const *lists, const int64_t *counts, int64_t n_total, int64_t k,
               int32_t *out_idx, float *out_score, int64_t *out_n);
/* The same for n_queries queries at once, n_threads host threads: source s (shard s, ascending shard order)
 * contributes packed[s][offsets[s][q] .. offsets[s][q+1]) to query q.  out_idx/out_score [n_queries*k]. */
int bbq_replay_batch(int32_t n_sources, const bbq_cand *const *packed, const int64_t *const *offsets,
                     int32_t n_queries, int64_t n_total, int64_t k, int32_t n_threads, int32_t *out_idx,
                     float *out_score, int64_t *out_n);

/* ------------------------------------------------------------------------------------------
 * On-disk format.  The reference declares a vector-data file ("veb") and a metadata file ("vemb",
 * src/constants.ts:52-57) with the fields of VectorDataFormat / MetadataFormat (src/types.ts:78-113) but only ever
 * builds them in memory (serializeVectorData, src/binaryQuantizationFormat.ts:483-530).  Here they are real files whose
 * payload IS the device layout, so loading is a straight file -> HBM copy with no re-tiling:
 *   <prefix>.vemb  "BVEC", version, MetadataFormat {fieldNumber, vectorEncodingOrdinal, vectorSimilarityOrdinal,
 *                  dimensions, vectorDataOffset, vectorDataLength, vectorCount, centroidSquareMagnitude}, the tile
 *                  geometry, centroid f32[dimensions], checksums            (DESIGN.md "On-disk format")
 *   <prefix>.veb   the 64-row tile records (packed 1-bit codes + corrections per row = VectorDataFormat's
 *                  binaryValues, lowerInterval, upperInterval, additionalCorrection, quantizedComponentSum),
 *                  then the exact-corrections side array of the compact layout
 * Little-endian.  A row shard is saved WITH its pilot replica (format version 3: three more header words, the replica's tile records
 * behind the shard's own), so a one-process-per-GPU service restarts from files without the host rows.  A multi-device index is saved
 * as one ordinary pair per shard, <prefix>.s000, <prefix>.s001, ..., plus the manifest <prefix>.vemb ("BVEM": shard count, the shards'
 * row ranges, totals, centroid, checksum); bbq_index_load_multi puts it back over several devices, bbq_index_load over one.
 */
int bbq_index_save(bbq_index *idx, const char *path_prefix, const float *centroid, int32_t similarity_ordinal);
/* header of <prefix>.vemb; any output pointer may be NULL */
int bbq_index_file_info(const char *path_prefix, int64_t *n_rows, int32_t *dim, int32_t *similarity_ordinal,
                        double *centroid_dp, int64_t *row_base);
/* centroid_out [dim] (may be NULL).  Fails with BBQ_ERR_INVALID_ARG on a malformed, truncated or corrupted file.  A manifest of a
 * multi-device index loads as a multi-device handle with every shard on `device`. */
int bbq_index_load(const char *path_prefix, int32_t device, bbq_index **out, float *centroid_out);
/* a saved multi-device index over several devices: shard s on devices[s % n_devices] (n_devices 0 / devices NULL: shard s on device
 * s modulo the visible devices).  The shards, their row ranges and pilot replicas are the ones that were saved. */
int bbq_index_load_multi(const char *path_prefix, int32_t n_devices, const int32_t *devices, bbq_index **out, float *centroid_out);
/* shards of a saved index: 1 for an ordinary pair, the manifest's count for a multi-device index, 0 if unreadable */
int32_t bbq_index_file_shards(const char *path_prefix);
/* the rows back in the reference's shape: codes [n*ceil(dim/8)] (multi-bit index: [n*dim]), corr [n*4] (either may be NULL) - what
 * vectorValue(ord) / getCorrectiveTerms(ord) return (src/binaryQuantizationFormat.ts:52-76) */
int bbq_index_export(bbq_index *idx, uint8_t *codes, double *corr);

/* ------------------------------------------------------------------------------------------
 * Oversample + exact rerank (the reference's recall recipe: src/topKSelector.ts:29-115,
 * tests/recall-common.ts:188-213).  The ORIGINAL fp32 vectors stay resident in HBM next to the 1-bit
 * index; true scores are computeSimilarity (src/vectorSimilarity.ts:14-126): f64, accumulated in index
 * order, bit-identical to the reference.
 */
typedef struct bbq_vectors bbq_vectors;
/* vectors [n*dim] row-major (the Float32Array[] the reference's selectors take as `vectors`), copied to the device */
int bbq_vectors_create(const float *vectors, int64_t n, int32_t dim, int32_t device, bbq_vectors **out);
/* the fp32 side of the rerank recipe grows with the index (bbq_index_append*): the rows get the next ords; storage grows by half as
 * much again when it runs out.  On failure nothing has changed. */
int bbq_vectors_append(bbq_vectors *v, const float *vectors, int64_t n);
/* the fp32 side of the rerank recipe follows a compaction of the index (bbq_index_compact): f->n_rows must equal bbq_vectors_size(v),
 * same device; the rows f accepts are kept, in order, gathered out of place on the device - storage afterwards is exactly |A| rows */
int bbq_vectors_compact(bbq_vectors *v, const bbq_filter *f);
/* the fp32 side of the rerank recipe follows an update of the index (bbq_index_update*): vectors [n*dim] become the rows ords [n],
 * the last of equal ords wins; an ord outside [0, bbq_vectors_size(v)): BBQ_ERR_INVALID_ARG.  On failure nothing has changed. */
int bbq_vectors_update(bbq_vectors *v, const int32_t *ords, const float *vectors, int64_t n);
void bbq_vectors_destroy(bbq_vectors *v);
int64_t bbq_vectors_size(const bbq_vectors *v);
int32_t bbq_vectors_dimension(const bbq_vectors *v);
/* computeSimilarity(queries[q], vectors[rows[j]], true_sim) for j in [offsets[q], offsets[q+1]), q < n_queries.
 * queries [n_queries*dim] raw fp32 (NOT normalised, exactly what the caller would hand computeCosineSimilarity);
 * offsets [n_queries+1] ascending from 0; out_true [offsets[n_queries]].  A row outside [0, n) fails with
 * BBQ_ERR_INVALID_ARG (the reference skips / throws on a missing vector, src/topKSelector.ts:44-45). */
int bbq_rerank_scores(bbq_vectors *v, int32_t n_queries, const float *queries, const int64_t *offsets,
                      const int32_t *rows, int32_t true_sim, double *out_true);
/* The whole recipe for n_queries queries: searchNearestNeighbors with k*factor on idx (arguments as
 * bbq_search_batch), true scores of those candidates on v, then the reference's selection:
 *   selector 0  getOversampledTopKWithHeap (src/topKSelector.ts:29-79): MinHeap of k on trueScore, drained, sorted
 *   selector 1  getOversampledTopKWithSort (:92-115): stable sort by trueScore descending, first k
 * true_sim is the similarity of the rerank (the reference's selectors always use COSINE = 1).
 * out_idx / out_quantized / out_true [n_queries*k] (query q at offset q*k), out_n [n_queries].
 * NaN true scores (non-finite inputs) make the reference's final Array.sort order engine-defined; here they sort as
 * "equal to everything", which is what the comparator returns. */
int bbq_search_rerank_batch(bbq_index *idx, bbq_vectors *v, int32_t n_queries, const float *queries,
                            const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim, int64_t k,
                            int32_t factor, int32_t selector, int32_t true_sim, int32_t *out_idx,
                            float *out_quantized, double *out_true, int64_t *out_n);

/* ------------------------------------------------------------------------------------------
 * Exact MaxSim rerank (DESIGN.md "Exact MaxSim rerank"): the third stage of late interaction - the candidate groups a MaxSim call
 * nominated, rescored against the fp32 rows of a bbq_vectors.  A query is a run of RAW fp32 token vectors: vec_offsets as
 * bbq_search_maxsim_batch takes and checks it, queries [vec_offsets[n_queries] * dim], not normalised, exactly as bbq_rerank_scores
 * takes a query.
 * Definitions.  For a token vector q_t and a row r, c(t, r) is the f64 bbq_rerank_scores returns for that pair under true_sim:
 * computeSimilarity, accumulated in index order, bit for bit.  For a live group G of a group set, M_t(G) is the greatest c(t, r) over
 * the rows of G that the set's filter accepts: a NaN ranks below every number, numbers rank by value with -0.0 below +0.0, and if every
 * accepted row gives NaN, M_t is NaN.  The group's true score is
 *   T = M_0 + M_1 + ...
 * - the adds f64, strictly in ascending token, starting from M_0 and not from 0.0, no contraction, no reassociation; a NaN result,
 * from a NaN M_t or from +Inf + -Inf, is written as the quiet NaN 0x7ff8000000000000, so host and device agree byte for byte.
 * bbq_maxsim_reduce_true (host only, no device) is this sum in plain C over rep_true[t * n_groups + g] -> out [n_groups],
 * n_vectors >= 1: the normative statement, as bbq_maxsim_reduce is for the f32 sums.
 * bbq_rerank_maxsim_groups_batch: out_true[i] (indexed like cand_groups) is T for group cand_groups[i] of g and that query.
 * cand_offsets / cand_groups as bbq_score_maxsim_groups_batch takes and checks them, with the same wording under this function's name:
 * range, liveness, the first offending (query, position, group) named, any order, a duplicate scored per occurrence, at most 2^31 - 1
 * expanded rows a query - on the host, under the context's lock, before the first launch; on refusal nothing is launched and nothing
 * written.  true_sim outside 0 .. 2 is refused with bbq_rerank_scores' message.  bbq_vectors_size(v) must equal the row count the group
 * set was made for and v must live on its device, otherwise BBQ_ERR_INVALID_ARG: a set made stale by an append or a compaction is
 * refused; after bbq_vectors_update the set still serves.  Non-finite inputs are not refused: they propagate by IEEE arithmetic, as in
 * bbq_rerank_scores.  n_queries == 0 or an empty total list: BBQ_OK, nothing launched.  One 8-byte record per candidate travels to the
 * device and one f64 per candidate comes back; no row list is staged, and a candidate's fp32 row is read once per token block, not
 * once per token.  A long call is worked through in sub-batches of at most 1024 queries and 256 MiB of scratch (the recipe call:
 * group_scratch_mb of its index) - per query 8 bytes per token of a block and 8 more, per entry of the call's longest list, and the
 * f64 image of a token block - in token blocks of bbq_maxsim_token_block() tokens; the scratch does not grow with the call.  A failed
 * allocation: BBQ_ERR_OOM, nothing written.  Results are byte-identical from run to run.
 * bbq_search_maxsim_rerank_batch is the whole recipe, defined by composition: (1) bbq_search_maxsim_batch with k * factor; (2) the
 * call above over each query's returned groups, in returned order; (3) bbq_search_rerank_batch's two selectors over the true scores -
 * selector 0 the heap of k, drained and stably sorted, selector 1 the stable descending sort, first k; NaN as there.  out_group /
 * out_quantized (the MaxSim search's f32 sums) / out_true [n_queries*k] (query q at offset q*k), out_n [n_queries].  Argument checks,
 * k == 0, factor < 1 and a k * factor that overflows as bbq_search_rerank_batch; handle restrictions as bbq_search_maxsim_batch.
 * Out of scope: a device-side select over the true scores, per-token best rows, multi-device handles and shards. */
int bbq_maxsim_reduce_true(const double *rep_true, int64_t n_vectors, int64_t n_groups, double *out);   /* host only */
int bbq_rerank_maxsim_groups_batch(bbq_vectors *v, const bbq_groups *g, int32_t n_queries, const int64_t *vec_offsets,
                                   const float *queries, int32_t true_sim, const int64_t *cand_offsets,
                                   const int32_t *cand_groups, double *out_true);
int bbq_search_maxsim_rerank_batch(bbq_index *idx, bbq_vectors *v, const bbq_groups *g, int32_t n_queries,
                                   const int64_t *vec_offsets, const float *queries, const uint8_t *qquant, const double *qcorr,
                                   int32_t query_bits, int32_t sim, int64_t k, int32_t factor, int32_t selector, int32_t true_sim,
                                   int32_t *out_group, float *out_quantized, double *out_true, int64_t *out_n);

/* ------------------------------------------------------------------------------------------
 * Exact search (DESIGN.md "Exact search"): the true top-k of raw fp32 queries over the rows a bbq_vectors keeps on the device - the
 * reference's getTrueTopK (tests/recall-common.ts:143-149: computeCosineSimilarity against every row, a stable sort by descending
 * score, the first k), the ground truth of every recall figure it publishes; for true_sim 0 and 2 the same sort over computeSimilarity
 * (src/vectorSimilarity.ts:14-126).
 * Definitions.  c(q, r) is the f64 bbq_rerank_scores returns for raw query q and row r under true_sim: computeSimilarity, accumulated
 * in index order, bit for bit.  A is the set of rows f accepts; f == NULL: every row.  The rows of A are ranked by the 64-bit key of
 * c's bits, descending - key = 1 for a NaN, ~bits for a negative number, bits | 2^63 otherwise (true_key, bbq_device.h) - and rows of
 * equal key by ascending row: numbers by value, a NaN below every number, NaNs among themselves by row.  (-0.0 would rank below +0.0,
 * but cannot arise: every chain starts from +0.0 and the Euclidean score is 1 / (1 + sqrt(.)).)  The answer of query q is the first
 * min(k, |A|) rows of that ranking: out_idx / out_true [n_queries*k] (query q at offset q*k), out_n [n_queries] the number written; a
 * NaN is written as 0x7ff8000000000000.  On finite inputs that is getTrueTopK: a stable descending sort leaves equal scores in row order.
 * bbq_true_topk (host only, no device) is that ranking in plain C over one row of scores [n] - accept_bits NULL or [ceil(n / 64)] words,
 * bit l of word t = row 64 t + l - into out_idx / out_true [min(k, |A|)] and *out_n: the normative statement.
 * bbq_vectors_search_batch computes it on the device: queries [n_queries*dim] raw fp32, NOT normalised, exactly as bbq_rerank_scores
 * takes them.  f->n_rows must equal bbq_vectors_size(v) on the same device, as bbq_vectors_compact demands, otherwise
 * BBQ_ERR_INVALID_ARG; true_sim outside 0 .. 2 is refused with bbq_rerank_scores' message; k < 0: BBQ_ERR_NEGATIVE_K; k == 0,
 * n_queries == 0 or |A| == 0: BBQ_OK, out_n = 0, nothing launched; min(k, |A|) > 4096: BBQ_ERR_UNSUPPORTED (bbq_rerank_scores over the
 * accepted rows and a sort on the host serve there).  Non-finite inputs are not refused: they propagate by IEEE arithmetic.  The checks
 * run under the context's lock before the first launch; after bbq_vectors_append, _update or _compact the call answers over the rows as
 * they now are.  A row is read once per block of 32 queries; a call is worked through in sub-batches of at most 1024 queries and slabs
 * of rows whose keys, 8 bytes per (query, row), stay under 256 MiB of scratch inside the handle; k x (row, score) per query is the only
 * copy back.  A failed allocation: BBQ_ERR_OOM, no answer written.  Results are byte-identical from run to run.
 * bbq_vectors_set_option: "exact_slab_rows", the rows scored between two select passes - 0 (automatic: what the scratch allows) or a
 * multiple of 256 in 256 .. 2^24.  A speed and scratch choice: it never changes an answer.  An unknown name or a value out of range:
 * BBQ_ERR_INVALID_ARG.
 * Out of scope: multi-device handles and shards, spans or row lists (bbq_rerank_scores takes lists), k beyond 4096. */
int bbq_true_topk(const double *scores, int64_t n, const uint64_t *accept_bits, int64_t k, int32_t *out_idx, double *out_true,
                  int64_t *out_n);                                                                      /* host only */
int bbq_vectors_search_batch(bbq_vectors *v, const bbq_filter *f, int32_t n_queries, const float *queries, int32_t true_sim,
                             int64_t k, int32_t *out_idx, double *out_true, int64_t *out_n);
int bbq_vectors_set_option(bbq_vectors *v, const char *name, int64_t value);

/* ------------------------------------------------------------------------------------------
 * Host-side quantizer (multithreaded C++): what the JS host calls for quantizeVectors /
 * quantizeQueryVector so that the drop-in API needs no TypeScript arithmetic.
 */
/* BinaryQuantizationFormat.quantizeVectors, src/binaryQuantizationFormat.ts:165-263 (+ normalizeVector,
 * computeCentroid, OptimizedScalarQuantizer.scalarQuantize :108-227, packAsBinary :420-446).
 * vectors [n*dim] row-major.  index_bits == 1: codes [n*ceil(dim/8)] packed; otherwise codes [n*dim] unpacked.
 * Fails with BBQ_ERR_EMPTY / BBQ_ERR_NAN_INPUT / BBQ_ERR_INF_INPUT like the reference throws; for the
 * NaN/Inf cases *bad_row / *bad_col (may be NULL) receive the offending position. */
int bbq_quantize_vectors(const float *vectors, int64_t n, int32_t dim, int32_t sim, int32_t index_bits,
                         double lambda, int32_t iters, int32_t n_threads, uint8_t *codes, double *corr,
                         float *centroid, int64_t *bad_row, int32_t *bad_col);
/* Host only, no device: quantizeVectors' per-row part with a GIVEN centroid - normalizeVector (COSINE), NaN / Infinity validation,
 * scalarQuantize(index_bits, centroid), packAsBinary - which is what bbq_index_append computes on the device.  With the centroid
 * bbq_quantize_vectors returned it reproduces that call's rows bit for bit.  Shapes, threads and errors as bbq_quantize_vectors;
 * n == 0: BBQ_OK. */
int bbq_quantize_rows(const float *vectors, int64_t n, int32_t dim, const float *centroid, int32_t sim, int32_t index_bits,
                      double lambda, int32_t iters, int32_t n_threads, uint8_t *codes, double *corr, int64_t *bad_row, int32_t *bad_col);
/* searchNearestNeighbors' query preparation, src/binaryQuantizationFormat.ts:337-347 + :271-299
 * (COSINE: the query is normalised twice) */
int bbq_quantize_query(const float *query, int32_t dim, const float *centroid, int32_t sim, int32_t query_bits,
                       double lambda, int32_t iters, uint8_t *qquant, double *qcorr);
/* bbq_quantize_query for n queries at once on n_threads host threads (0 = all cores): queries [n*dim], qquant [n*dim],
 * qcorr [n*4].  On failure *bad_query (may be NULL) is the first offending query and the error is the one
 * bbq_quantize_query reports for it.  A 768-d query takes ~50 us on one core; batches feed the device at its own rate. */
int bbq_quantize_queries(const float *queries, int32_t n, int32_t dim, const float *centroid, int32_t sim,
                         int32_t query_bits, double lambda, int32_t iters, int32_t n_threads, uint8_t *qquant,
                         double *qcorr, int32_t *bad_query);
/* quantizeQueryVector alone, src/binaryQuantizationFormat.ts:271-299 (normalises once for COSINE) */
int bbq_quantize_query_vector(const float *query, int32_t dim, const float *centroid, int32_t sim,
                              int32_t query_bits, double lambda, int32_t iters, uint8_t *qquant, double *qcorr);
/* computeDotProduct(centroid, centroid), src/vectorOperations.ts:171-185 */
double bbq_centroid_dp(const float *centroid, int32_t dim);

/* ------------------------------------------------------------------------------------------
 * Introspection for bench.py / profiling (not part of the drop-in surface)
 */
typedef struct {
  double last_scan_ms;        /* hipEvent time of the dominant (largest) scan launch of the last batch call */
  int64_t last_scan_rows;     /* rows x queries that launch covered */
  int64_t last_scan_bytes;    /* algorithmic HBM bytes of that launch */
  int64_t candidates;         /* candidates replayed on the host in the last call (all queries) */
  int64_t dense_fallbacks;    /* queries of the last call that took the dense path */
  double total_scan_ms;       /* sum of hipEvent times of every dominant-scan launch since the last reset */
  int64_t total_scan_bytes;   /* and their algorithmic bytes */
  int64_t total_scan_launches;
  int64_t host_replays;       /* queries of the last call whose heap was replayed on the host (equal scores in or at the edge of the
                                 answer, k > 1024, device_select 0); the others were selected and sorted by the last finalize launch */
  int64_t resident_bytes;     /* bytes of ONE query's sweep of the index (all launches of its sub-batch; pilot replica included) that are
                                 loaded with the default cache policy, so that they stay in the device's 256 MiB Infinity Cache from one
                                 query's sweep to the next (option resident_mb, per launch); the rest is streamed with non-temporal loads.
                                 Their re-reads do not reach HBM */
} bbq_stats;
int bbq_get_stats(bbq_index *idx, bbq_stats *out);
int bbq_reset_stats(bbq_index *idx);
/* tuning knobs; returns BBQ_ERR_INVALID_ARG for unknown names or values out of range (DESIGN.md "Knobs"):
 *   batch_queries 0..1024 (0 = by index size: 32 from 6 M rows, 64 from 2.5 M, 128 below; at least 64 with sweep_share 32)   pipeline_slots 1..4 (3)   segment_growth 2..1024 (8)   first_segment_rows 1024..8192 (4096)
 *   resident_mb -1..2^20 (MiB of its row range a sweep launch keeps cache-resident; -1: this index's share of 224 MiB, by size among the
 *     indexes active on its device; 0: stream everything - the "no reuse across queries" mode: with it the automatic l2_share is 1 as
 *     well, so that every byte of every query's sweep comes from HBM)   resident_interleave 0|1 (1: the resident chunks are spread over the range)
 *   l2_share -1|1|2|4|8|16|32 (-1): queries per chunk whose workgroups a per-query sweep launch dispatches back to back onto one XCD, so
 *     that only the first of them reads the chunk beyond that XCD's L2 (every query still runs its own workgroups, loads and popcounts;
 *     a launch order, never a different answer).  1: off, the plain order.  -1: the library's choice, 1 with resident_mb 0.  An explicit
 *     value holds whatever resident_mb says; a launch co-schedules no more queries than it has, and fewer per chunk when it sweeps more
 *     than 134 M rows (the grid's x extent is a 32-bit count of work-items)
 *   row_sums -1|0|1 (-1): compact corrections: 1 lets the per-query sweep read a row's component sum (its popcount / code sum) from a
 *     derived side array of 2 B/row instead of counting it for every query again; 0: always count.  -1: the library's choice - read,
 *     except with resident_mb 0, whose launches stay what they were.  An explicit value holds whatever resident_mb says.  The array
 *     exists where dim * (2^store bits - 1) <= 65535 (elsewhere 1 is accepted and the sweep counts), and a few row widths keep counting
 *     whatever the option says, because the reading kernel would run with fewer waves there: 1-bit rows of 1409..1536 dimensions at
 *     queryBits 1 (filtered searches: also at queryBits 8), 4-bit rows of 353..384 and of 481..512 dimensions at queryBits 8
 *     (filtered: also at 4).  No statistic tells which kernel ran.  The array is kept beside the rows through
 *     every append, update and compaction, and is in no file: a load derives it again.  The same value either way: never a different answer
 *   digit_planes -1|0|1 (-1): 1-bit index, compact corrections, queryBits 3..4 (query values that need four bit-planes): 1 and -1 let the
 *     per-query sweep score a query in three planes of ternary digits (q - 4 = t0 + 3 t1 + 9 t2) and the row's component sum instead of
 *     four bit-planes, wherever that sweep reads the sum (row_sums) - so never with resident_mb 0 and an automatic row_sums - and the
 *     row is 6, 8 or 12 16-byte chunks wide (641..768, 897..1024, 1409..1536 dimensions; a filtered search: 641..768 only) - where it
 *     was measured faster; 0: always bit-planes.  The digit masks are staged with the query in addition to its bit-planes (5 x 16 bytes per 128 dimensions).  The dot
 *     product is the same exact integer either way: never a different answer
 *   tiles_per_wave -1|1|2|4|8 (-1): tiles (64 rows) a wave of the per-query sweep takes one after the other where digit_planes applies to
 *     an unfiltered search (6, 8 or 12 chunks): the workgroup has 8 / tiles_per_wave waves, and what belongs to the workgroup or the wave -
 *     addresses, the query's uniforms, staging, the end of the chunk - is executed once for that many tiles.  -1: the library's choice per row
 *     width - 8 at 641..768 dimensions, 4 at 897..1024, 1 elsewhere; an explicit value holds wherever the kernel exists and means 1 elsewhere (filtered
 *     searches, other widths and query widths, resident_mb 0 with an automatic row_sums).  Never a different answer
 *   group_scratch_mb 1..8192 (256): MiB of device scratch a sub-batch of bbq_search_grouped_batch may take for its representatives, 16
 *     bytes per live group and query: a score launch takes as many queries as fit (at most 1024, at least one).  Never a different answer
 *     The same budget bounds a sub-batch of bbq_search_maxsim_batch: 8 bytes per token of a block and 16 per query, per live group
 *   maxsim_fused -1|0|1 (-1): the score pass of bbq_search_maxsim_batch.  0: the grouped search's score kernel, every token vector of a
 *     block as one of its queries; 1: wherever it exists - 4 query bit-planes against 1-bit rows of 6, 8 or 12 16-byte chunks - the fused
 *     kernel, which loads a tile once for all tokens of a query's block; -1: the fused kernel, which was measured faster at 1 M rows of each
 *     of its three widths (profiles/maxsim_search*.json).  Never a different answer
 *   fast_bound 0|1 (1): compact corrections: 1 tests the score bound of a row in f32 against the threshold's image in the linear space of
 *     the score formula, for every query whose corrections have f32 images (others keep the f64 bound); 0: always the f64 bound through
 *     the similarity transform.  A pre-filter in front of the exact score either way: never a different answer
 *   replay_threads 1..256 (half the host cores, at most 16)   flood_rows 0..2^24 (262144)   force_dense 0|1 (0)
 *   sweep_share 1|4|8|32 (1: every query sweeps the index itself; 32: shared sweep on the matrix cores, groups of 32 queries, two groups per load of the rows;
 *     32 also serves bbq_search_filtered_batch - tiles without an accepted row are not loaded; 4 and 8 do not: a filtered call sweeps per query under them)
 *   device_select 0|1 (1: for k <= 1024 the device selects and sorts the answer itself whenever no two scores in or at the edge of it
 *   compare equal - then the reference heap provably returns that order - and the host replays the heap only for the rest)
 *   latency_queries 0..1024 (4), latency_growth 2..4096 (64): calls with at most latency_queries queries walk the index in
 *   segments that grow by latency_growth instead of segment_growth (fewer dependent launches, more candidates per query) and their
 *   sweeps append the candidates to the query's list themselves (one atomic per workgroup; append_last 0|1 (1): also the last segment)
 *   latency_fused 0|1 (1): a call with ONE query runs without a copy at either end (query in the kernel arguments of every sweep, answer
 *   polled from mapped host memory); latency_presample 0|1 (1): and, from 262144 rows, with its threshold from per-wave top keys of a
 *   prefix - four launches in all (DESIGN.md "The single-query call") */
int bbq_set_option(bbq_index *idx, const char *name, int64_t value);

#ifdef __cplusplus
}
#endif
#endif
