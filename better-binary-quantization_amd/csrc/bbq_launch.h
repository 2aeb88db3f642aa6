// bbq_launch.h - host-callable launch wrappers of every kernel file: the sweeps, finalize and pack (bbq_kernels.hip, bbq_filter_kernels.hip,
// bbq_mfma_kernels.hip, bbq_latency_kernels.hip), the index build (bbq_build_kernels.hip), the rerank (bbq_rerank_kernels.hip), the scoring of chosen rows (bbq_gather_kernels.hip)
// the range search (bbq_range_kernels.hip), the span search (bbq_span_kernels.hip), the grouped search (bbq_group_kernels.hip), the MaxSim
// search (bbq_maxsim_kernels.hip), MaxSim over chosen groups (bbq_maxsim_cand_kernels.hip), the exact MaxSim rerank (bbq_maxsim_rerank_kernels.hip) and the
// exact search (bbq_exact_kernels.hip)
#pragma once
#include <hip/hip_runtime.h>
#include "bbq_device.h"

namespace bbq {

// planes: number of query bit-planes (1, 2, 4 or 8); multi-bit index: 4 (query values <= 15) or 8
// tiles_per_wave (1, 2, 4 or 8): tiles a wave of the sparse sweep takes one after the other where the launch has such a twin (tiles_twin,
// bbq_scan_body.h); 1 - and everywhere else - one tile per wave.  A speed choice only
hipError_t launch_scan(const ScanArgs &a, int planes, bool dense, int n_queries, int n_chunks, hipStream_t s, int tiles_per_wave = 1);
// the sparse sweep of a filtered search: accept[tile] = the tile's accept word (bit l = row l of the tile), one word per tile of a.idx
hipError_t launch_scan_filtered(const ScanArgs &a, const uint64_t *accept, int planes, int n_queries, int n_chunks, hipStream_t s);
// shared sweep: `share` (4 or 8) queries per workgroup reuse every loaded row (sparse segments, fixed-width dims only)
bool shared_sweep_supported(const ScanArgs &a, int share);
hipError_t launch_scan_shared(const ScanArgs &a, int planes, int share, int n_queries, int n_chunks, hipStream_t s);
// shared sweep on the matrix cores: 32 queries per workgroup (bbq_mfma_kernels.hip); query values must be <= 127 (fp_scale > 0: <= 15,
// staged as FP6 times fp_scale against the bit weights for v_mfma_f32_32x32x64_f8f6f4; 0: int8 for v_mfma_i32_32x32x32_i8), every
// query's interval width positive and finite
bool mfma_sweep_supported(const ScanArgs &a);
int64_t mfma_query_bytes_per_group(int w16, bool fp);  // staged operand bytes of 32 queries
int mfma_queries_per_tile_load(const ScanArgs &a, int n_queries, bool fp);  // 32, or 64 where a workgroup serves two groups per tile
hipError_t launch_scan_mfma(const ScanArgs &a, const uint8_t *qbytes, const float *qmax, float fp_scale, int n_queries, int n_chunks, hipStream_t s);
// ... of a filtered search: accept as launch_scan_filtered takes it.  Tiles without an accepted row are not loaded, a rejected row is
// never a candidate; same shapes, same queries per tile load (mfma_sweep_supported, mfma_queries_per_tile_load).  Every query needs a
// threshold already (the kernel flags one without as overflowed): the caller sweeps here only behind k accepted rows
hipError_t launch_scan_mfma_filtered(const ScanArgs &a, const uint64_t *accept, const uint8_t *qbytes, const float *qmax, float fp_scale, int n_queries,
                                     int n_chunks, hipStream_t s);
hipError_t launch_finalize(const FinalizeArgs &a, int n_queries, hipStream_t s);
// lists are [nq][list_stride]; a query may hold more than advertised_cap entries (a flood): such queries are only dropped
// (flagged) when the packed buffer cannot take the sum
hipError_t launch_pack(const int32_t *counts, const uint64_t *lists, int64_t list_stride, int64_t advertised_cap, int32_t nq, int64_t *offsets,
                       int32_t *flags_out, int64_t *total_out, uint64_t *packed, int64_t packed_cap, hipStream_t s);
// latency path (bbq_latency_kernels.hip): false when this index shape has no instantiation (the caller takes the general path)
bool latency_path_supported(const IndexView &v, int planes);
hipError_t launch_lat_scan(const LatScanArgs &a, int planes, hipStream_t s);
// pre-sampled threshold: per-wave top keys of the first rows, then theta := the rank-th largest of them (0 when there are fewer)
hipError_t launch_lat_pre(const LatPreArgs &a, int planes, hipStream_t s);
hipError_t launch_lat_select(const uint32_t *pre_keys, int n_keys, int rank, Threshold *theta, const QueryParams &p, hipStream_t s);

// index build on the device (bbq_build_kernels.hip).  Every wrapper that writes or reads tile records takes them as a TileDest
// (records, side rows, geometry: bbq_device.h) and rows in the caller's shape as StagedRows.  Those that take row0 (tile0) work at a
// row offset: the rows handed over are the rows [row0, n_rows) of the storage, the first of them lands in lane row0 % 64 of tile
// row0 / 64 and nothing below row0 is touched (0: a creation).
// vT4 is the [ceil(dim/4)][npad] float4 transposed copy of the fp32 rows
hipError_t launch_build_transpose(const float *in, int64_t n, int32_t dim, int64_t npad, float *vT4, hipStream_t s);
hipError_t launch_build_normalize(float *vT4, int64_t n, int32_t dim, int64_t npad, hipStream_t s);
hipError_t launch_build_validate(const float *vT4, int64_t n, int32_t dim, int64_t npad, unsigned long long *first_bad, hipStream_t s);
hipError_t launch_build_centroid(const float *vT4, int64_t n, int32_t dim, int64_t npad, float *centroid, hipStream_t s);
// 1-bit: the n vectors become the rows [row0, row0 + n) of `out`, quantized straight into their lanes (corr_rm, optional, stays indexed
// by the vector).  A freshly quantized row's component sum is its popcount: `out` is a geometry with has_x1 = 0
hipError_t launch_build_quantize1(const float *vT4, int64_t n, int64_t npad, const float *centroid, int32_t sim, double lambda, int32_t iters,
                                  const TileDest &out, double *corr_rm, hipStream_t s, int64_t row0);
// indexBits > 1: unpacked codes [n][dim] (one byte per dimension) + row-major corrections [n][4], both in device memory
hipError_t launch_build_quantize_bits(const float *vT4, int64_t n, int32_t dim, int64_t npad, const float *centroid, int32_t sim,
                                      double lambda, int32_t iters, int32_t bits, uint8_t *codes_rm, double *corr_rm, hipStream_t s);
// the n rows of `src` from row0 on -> codes_rm [n][pb] (1-bit rows)
hipError_t launch_build_untile(const TileDest &src, int64_t n, uint8_t *codes_rm, hipStream_t s, int64_t row0);
// rows in the caller's shape -> tile records.  Multi-bit rows: *bad is raised by a code that is not below 2^index_bits (1-bit: unused)
hipError_t launch_retile(const TileDest &out, const StagedRows &in, int64_t n_rows, int64_t row0, int32_t index_bits, uint32_t *bad, hipStream_t s);
// *mismatch is raised by a row whose quantizedComponentSum is not its popcount (1-bit) / the sum of its codes (multi-bit)
hipError_t launch_check_x1(const StagedRows &in, int64_t n_rows, const TileGeom &g, uint32_t *mismatch, hipStream_t s);
// multi-bit rows [count bytes]: *bad is raised by a code that is not below 2^index_bits (nothing is written)
hipError_t launch_check_code_range(const uint8_t *codes, int64_t count, int32_t index_bits, uint32_t *bad, hipStream_t s);
// compact layout: each tile's {min, max} of additionalCorrection (read from exact[]) -> add_range[tile][2]
hipError_t launch_tile_add_range(const double *exact, int64_t n_rows, float *add_range, hipStream_t s, int64_t tile0);
// the same for the n_listed tiles named (each below ceil(n_rows / 64)): an update's touched tiles
hipError_t launch_tile_add_range_list(const double *exact, int64_t n_rows, float *add_range, const int64_t *tiles, int64_t n_listed, hipStream_t s);
// compact layout with a row_sums side array (row_sums_fit): each row's popcount / code sum, computed from the codes the tiles of `src`
// hold -> row_sums[tile * 64 + lane], the lanes at and beyond n_rows 0.  Tiles [tile0, ceil(n_rows / 64)), or the n_listed tiles named:
// launched wherever add_range is written, over the same tiles
hipError_t launch_tile_row_sums(const TileDest &src, int64_t n_rows, uint16_t *row_sums, hipStream_t s, int64_t tile0);
hipError_t launch_tile_row_sums_list(const TileDest &src, int64_t n_rows, uint16_t *row_sums, const int64_t *tiles, int64_t n_listed, hipStream_t s);
// rows in the caller's shape -> the lanes of the rows they replace: staged row pos[i] becomes row ords[pos[i]] for the n_winners
// entries of pos, which name distinct ords in ascending order (bbq_update_winners); nothing else is written.  ords are rows of `out`;
// multi-bit codes have been range-checked (launch_check_code_range): *bad is the shared packer's and stays clear
hipError_t launch_scatter_rows(const TileDest &out, const StagedRows &in, const int32_t *ords, const int64_t *pos, int64_t n_winners,
                               int32_t index_bits, uint32_t *bad, hipStream_t s);
// the rows of `src` that map.accept keeps -> the rows [0, map.kept) of `out`, in order, padding lanes of the last tile included.  `out`
// holds ceil(map.kept / 64) tiles of src's geometry and is not src (the gather runs out of place)
hipError_t launch_compact_tiles(const TileDest &out, const TileDest &src, const CompactMap &map, hipStream_t s);

// exact rerank (bbq_rerank_kernels.hip): one wave per 64 candidates of a query; max_count = longest candidate list
hipError_t launch_rerank(const RerankArgs &a, int n_queries, int64_t max_count, hipStream_t s);
// scoring chosen rows (bbq_gather_kernels.hip): one workgroup per kGatherThreads entries of a query's list; max_count = longest list,
// n_queries <= 65535; planes as launch_scan takes them
hipError_t launch_score_ords(const GatherArgs &a, int planes, int n_queries, int64_t max_count, hipStream_t s);
// range search (bbq_range_kernels.hip), in the order a sub-batch launches them.  theta[q] = {keys[q], its z image for query q}
hipError_t launch_range_theta(Threshold *theta, const uint32_t *keys, const QueryParams *qparams, int n_queries, hipStream_t s);
// counts[q][chunk] = rows of the chunk that a.accept takes and whose score key beats theta[q], for the n_queries queries from a.q_first on
// (n_queries <= 65535); planes as launch_scan takes them
hipError_t launch_range_count(const RangeArgs &a, int planes, int n_queries, hipStream_t s);
// per query: counts -> their exclusive prefix IN PLACE, totals[q] = their sum, nonempty[q][0 .. n_nonempty[q]) = the chunks with a count, ascending
hipError_t launch_range_offsets(uint32_t *counts, uint32_t *nonempty, uint32_t *totals, uint32_t *n_nonempty, int n_chunks, int n_queries, hipStream_t s);
// the passing rows of the n_queries queries from a.q_first on, as entries at a.out[a.base[q] + ...], ascending by row; max_nonempty = the
// longest non-empty-chunk list among them
hipError_t launch_range_fill(const RangeArgs &a, int planes, int n_queries, int64_t max_nonempty, hipStream_t s);
// span search (bbq_span_kernels.hip).  The f32 scores of the rows of n_items work items (a.items[0 .. n_items), at most
// kGridWorkItemsMax / kChunkRows of them) -> a.scores; planes as launch_scan takes them.  With a.accept (a filter's words) only the
// accepted rows, compacted, and each one's ord -> a.ords beside its score
hipError_t launch_span_score(const SpanScoreArgs &a, int planes, int64_t n_items, hipStream_t s);
// per selected query (a.sel[0 .. n_selected)): the exact (a.k + 1)-th largest of its scores, the number of rows above it and, when that
// is a.k and no score is NaN, those rows as entries in any order -> the query's block of a.out.  With a.ords a row's ord is read from
// there (the compacted scores of a filtered call), from a.runs otherwise
hipError_t launch_span_select(const SpanSelectArgs &a, int n_selected, hipStream_t s);
// grouped search (bbq_group_kernels.hip).  Every chunk of a.idx for each of a.n_queries queries (<= 65535): the packed key of every live
// group's best accepted row -> a.rep[q][slot], which the caller has cleared; planes as launch_scan takes them.  At most two global
// atomics per workgroup - a max, so the result does not depend on their order
hipError_t launch_group_score(const GroupScoreArgs &a, int planes, hipStream_t s);
// rep[i] -> scores[i] (key 0: a quiet NaN), ords[i] for the n packed keys of a sub-batch
hipError_t launch_group_unpack(const unsigned long long *rep, float *scores, uint32_t *ords, int64_t n, hipStream_t s);
// MaxSim search (bbq_maxsim_kernels.hip).  The accumulate pass of one token block for the n_queries (<= 65535) entries of a.queries
hipError_t launch_maxsim_accumulate(const MaxSimAccArgs &a, int n_queries, hipStream_t s);
// is there a fused score kernel for this index and plane count?  (4 planes against 1-bit rows of 6, 8 or 12 chunks)
bool maxsim_fused_exists(const TileGeom &geom, int planes);
// the fused score pass of one token block: every chunk of a.g.idx for each of a.g.n_queries entries of a.queries -> a.g.rep, which the
// caller has cleared.  hipErrorInvalidValue where maxsim_fused_exists says no: the caller asks first
hipError_t launch_maxsim_score(const MaxSimScoreArgs &a, int planes, hipStream_t s);
// MaxSim over chosen groups (bbq_maxsim_cand_kernels.hip).  The score pass of one token block: for each of the n_queries (<= 65535)
// entries of a.queries the expanded rows of its candidate list, `longest` (<= kMaxSimCandMaxRows) the most of any of them -> a.rep, which
// the caller has cleared; planes as launch_scan takes them.  The launch sets a.tok_pass.  launch_maxsim_accumulate follows it
hipError_t launch_maxsim_cand_score(const MaxSimCandArgs &a, int planes, int n_queries, int64_t longest, hipStream_t s);
// exact MaxSim rerank (bbq_maxsim_rerank_kernels.hip).  The score pass of one token block: for each of the n_queries (<= 65535) entries
// of a.queries the expanded rows of its candidate list, `longest` (<= kMaxSimCandMaxRows) the most of any of them, against the block's
// tokens -> a.rep, which the caller has cleared
hipError_t launch_maxsim_rerank_score(const MaxSimRerankArgs &a, int n_queries, int64_t longest, hipStream_t s);
// its accumulate pass for the same entries of a.queries
hipError_t launch_maxsim_true_accumulate(const MaxSimTrueAccArgs &a, int n_queries, hipStream_t s);
// exact search (bbq_exact_kernels.hip).  The score pass of one slab: the rows [a.row0, a.row0 + rows) against every query block of the
// sub-batch -> a.keys; rows a multiple of 64 unless the slab is the last
hipError_t launch_exact_score(const ExactScoreArgs &a, int64_t rows, hipStream_t s);
// its select pass: the slab folded into the running list of each of the n_queries queries
hipError_t launch_exact_select(const ExactSelectArgs &a, int n_queries, hipStream_t s);
// the fp32 rows [n][dim] of `src` that map.accept keeps (word t = rows 64 t .. 64 t + 63) -> the rows [0, map.kept) of `out`, out of place
hipError_t launch_compact_vectors(float *out, const float *src, int32_t dim, const CompactMap &map, hipStream_t s);
// staged fp32 row pos[i] -> row ords[pos[i]] of `out` [rows][dim], for the n_winners entries of pos (distinct ords), in place
hipError_t launch_scatter_vectors(float *out, const float *staged, int32_t dim, const int32_t *ords, const int64_t *pos, int64_t n_winners, hipStream_t s);

}  // namespace bbq
