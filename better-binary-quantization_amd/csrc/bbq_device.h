// bbq_device.h - structs shared by the HIP kernels and the host orchestration (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "bbq_entry.h"

namespace bbq {

constexpr int kTileRows = 64;        // one wavefront = one tile: lane r owns row r of the tile
#ifndef BBQ_CHUNK_ROWS
#define BBQ_CHUNK_ROWS 512
#endif
constexpr int kChunkRows = BBQ_CHUNK_ROWS;  // rows per workgroup (one 64-row tile per wave); candidate slots are per chunk
constexpr int kTilesPerChunk = kChunkRows / kTileRows;
constexpr uint32_t kCountRedirect = 0x80000000u;  // chunk count: the entries live in the overflow area
constexpr uint32_t kFlagOverflow = 1u;   // a candidate slot / list / key buffer overflowed
constexpr uint32_t kFlagNaN = 2u;        // a NaN score was produced: order statistics are meaningless
// Append counters (ScanArgs::append_counts, FinalizeArgs::append_counts): one per query, each in a 128-byte line of its own.  The
// memory side retires returning atomics on ONE line one after the other (scripts/ubench/atomic_lines.hip: 5.8 ns each on 32 adjacent
// words, 0.4 ns on 32 words in separate lines): with the counters of a sub-batch side by side the atomics of a sweep's workgroups
// took longer than the sweep.
constexpr int kAppendStride = 32;        // uint32 words between two queries' counters

// Device layout of one index storage (DESIGN.md "HBM layout").  A tile record holds 64 rows:
//   [w16][64] uint4    16-byte code chunk j of row r at (j*64 + r)*16      -> 1 KiB coalesced per wave load
// followed by the corrections, in one of two layouts:
//  kLayoutInline (exact corrections streamed with the codes, 24 or 32 B/row)
//   [64] double2       {lowerInterval, upperInterval}                      -> 1 KiB
//   [64] double        additionalCorrection                                -> 512 B
//   [64] double        quantizedComponentSum (only if has_x1)              -> 512 B
//  kLayoutCompact (4 B/row streamed; exact corrections in a side array, gathered only for rows whose score BOUND passes
//  the threshold)
//   [64] uint32        bf16(lower) | bf16(upper) << 16 (f32 bits truncated)       -> tiles stay multiples of 128 B
//   side array exact[row] = {lower, upper, additional, 0} as 4 doubles (32 B/row), followed by
//   side array add_range[tile] = {min, max} of the tile's additionalCorrection as f32 (8 B per 64 rows, one broadcast load
//   per wave): the bound takes whichever end makes the score larger; the additive term varies far less inside a tile than
//   scores vary between rows, followed (where a row's sum fits 16 bits, row_sums_fit) by
//   side array row_sums[row] = the row's popcount / code sum as uint16 (128 B per tile, lanes beyond the last row 0): derived from the
//   stored codes wherever add_range is written, never stored in a file; the per-query sparse sweep reads it instead of counting
constexpr int kLayoutInline = 0;
constexpr int kLayoutCompact = 1;
// Multi-bit indexes (indexBits > 1; the reference keeps such rows as one byte per dimension,
// src/binaryQuantizationFormat.ts:241-245): a row is stored as `store_bits`-wide fields, field f of row dword w = dimension
// w * (32 / store_bits) + f at bits [f * store_bits, (f + 1) * store_bits); rows are zero-padded to 16-byte chunks and laid out
// in the same [w16][64] uint4 tile records, followed by the same corrections blocks.
__host__ __device__ inline int store_bits_of(int index_bits) { return index_bits <= 1 ? 1 : index_bits <= 2 ? 2 : index_bits <= 4 ? 4 : 8; }
__host__ __device__ inline int row_bytes_of(int dim, int store_bits) { return (dim * store_bits + 7) / 8; }
// 16-byte units of staged query data per 16-byte chunk of a row.  1-bit rows: one bit-plane per query bit (QB = 1, 2, 4, 8).
// Multi-bit rows: per row dword, the query's low nibbles (and, for query values above 15: QB = 8, its high nibbles) in the order
// the kernel unfolds the fields: store_bits 2 -> {even fields, odd fields}, 4 -> the 8 nibbles, 8 -> the 4 bytes.
__host__ __device__ constexpr int query_units_per_chunk(int qb, int store_bits) {
  return store_bits == 1 ? qb : store_bits == 2 ? (qb > 4 ? 4 : 2) : store_bits == 4 ? (qb > 4 ? 2 : 1) : 1;
}
// ---- a 4-plane query against 1-bit rows as three planes of ternary digits (the digit form of the per-query sparse sweep, tile_digit_dot).
// q - 4 = t0 + 3 t1 + 9 t2 with t0, t1 in {-1, 0, 1} and t2 in {0, 1}: balanced ternary of [-4, 11].  A digit plane is a pair of disjoint
// masks - P where the digit is +1, N where it is -1 - and costs what a bit-plane costs, one bit operation and one popcount per row dword:
//   pop(x & P) - pop(x & N) = pop((x & P) | (~x & N)) - pop(N),
// a bit-field insert with the row word as the selector; pop(N) does not depend on the row.  The top digit is never negative: a plain AND.
//   qcDist = sum_d q[d] x[d] = 4 ones + a0 + 3 a1 + 9 a2 - K,   a_i = sum over the row's dwords of pop(bfi(x, P_i, N_i)),   K = pop(N_0) + 3 pop(N_1)
// with ones = the row's popcount (the row_sums side array): three planes instead of four, an exact integer below 2^32.
// The staged form is kDigitMasks 16-byte masks per 16-byte chunk of a row, [j][5] = {P0, N0, P1, N1, P2}, packed like the rows; a padding
// position is staged as the value 0 (bits in N0 and N1), so that a row bit there weighs 4 - 1 - 3 = 0 (fill_query_digits).  K travels in
// QueryParams::digit_k.
constexpr int kDigitOffset = 4;
constexpr int kDigitMasks = 5;
struct DigitTriple { int8_t t0, t1, t2; };
constexpr DigitTriple kDigitTable[16] = {{-1, -1, 0}, {0, -1, 0}, {1, -1, 0}, {-1, 0, 0}, {0, 0, 0}, {1, 0, 0}, {-1, 1, 0}, {0, 1, 0},
                                         {1, 1, 0},   {-1, -1, 1}, {0, -1, 1}, {1, -1, 1}, {-1, 0, 1}, {0, 0, 1}, {1, 0, 1}, {-1, 1, 1}};
constexpr bool digit_table_is_exact() {
  for (int q = 0; q < 16; ++q) {
    const DigitTriple t = kDigitTable[q];
    if (t.t0 < -1 || t.t0 > 1 || t.t1 < -1 || t.t1 > 1 || t.t2 < 0 || t.t2 > 1) return false;
    if (q != kDigitOffset + t.t0 + 3 * t.t1 + 9 * t.t2) return false;
  }
  return true;
}
static_assert(digit_table_is_exact(), "q == 4 + t0 + 3 t1 + 9 t2 for every 4-bit value, and the top digit is never negative");
// the masks a value sets, bit m = mask m of {P0, N0, P1, N1, P2}
constexpr uint32_t digit_mask_bits(int q) {
  const DigitTriple t = kDigitTable[q];
  return (t.t0 > 0 ? 1u : 0u) | (t.t0 < 0 ? 2u : 0u) | (t.t1 > 0 ? 4u : 0u) | (t.t1 < 0 ? 8u : 0u) | (t.t2 > 0 ? 16u : 0u);
}

// ---- the tile record: the ONE definition of its bytes.  Every kernel that reads or writes a record, bbq_index_export on the host and
// the file (<prefix>.veb holds the records as they are) take their offsets from here.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));  // one 16-byte code chunk
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef double f64x2 __attribute__((ext_vector_type(2)));    // {lowerInterval, upperInterval}
typedef float f32x4 __attribute__((ext_vector_type(4)));
struct TileGeom {
  int32_t w16;          // 16-byte chunks per row = ceil(stored row bytes / 16)
  int32_t tile_stride;  // bytes per tile record (tile_stride_of)
  int32_t has_x1;       // 0: quantizedComponentSum == popcount / code sum of the row, recomputed on the fly
  int32_t dim;
  int32_t layout;
  int32_t store_bits;   // 1: packed 1-bit rows; 2 / 4 / 8: multi-bit fields (indexBits 2 / 3-4 / 5-8)
};
// ---- the per-query sweep's workgroup -> (chunk, query) map (bbq_scan_kernel and its launch, bbq_scan_body.h).  P = 2^s queries are
// co-scheduled per chunk (option l2_share): grid.x = 8 P ceil(n_chunks / 8), grid.y = ceil(n_queries / P).  The device deals the
// workgroups of a row round-robin over its 8 XCDs, so L & 7 labels the workgroups that share an XCD - and its L2 - and the P
// workgroups that sweep one chunk for P different queries are consecutive among the workgroups of one label: they are dispatched
// back to back onto one XCD, the first of them brings the chunk's lines into that L2 and the others find them there (or in flight).
// A speed choice only: the answer does not depend on where or when a workgroup runs.  s = 0 is the plain map, chunks fastest,
// grid = (n_chunks, n_queries) without padding.  A workgroup whose chunk_local >= n_chunks or whose query >= n_queries has no work.
struct SweepCoord {
  int32_t chunk_local;  // chunk inside the launch: + ScanArgs::chunk_begin = the chunk of the index
  int32_t query;
};
__host__ __device__ constexpr SweepCoord sweep_coord(uint32_t bx, uint32_t by, int s) {
  return SweepCoord{(int32_t)(((bx >> (3 + s)) << 3) | (bx & 7u)), (int32_t)((by << s) + ((bx >> 3) & ((1u << s) - 1u)))};
}
__host__ __device__ constexpr uint32_t sweep_grid_x(int n_chunks, int s) { return s == 0 ? (uint32_t)n_chunks : ((uint32_t)(n_chunks + 7) / 8u * 8u) << s; }
__host__ __device__ constexpr uint32_t sweep_grid_y(int n_queries, int s) { return ((uint32_t)n_queries + (1u << s) - 1u) >> s; }
// The limit of the reordered grid: a launch's x extent in WORK-ITEMS, grid.x * kChunkRows, is a 32-bit count (the dispatch packet's
// grid_size_x; the runtime refuses more with hipErrorInvalidConfiguration).  The plain grid has n_chunks * kChunkRows = the launch's rows
// there, which fits for every index the library accepts (at most 2^32 - 1 rows); the reordered one has P times as many, so P = 32
// fits up to 262 136 chunks (134 M rows) per launch, and a longer launch co-schedules fewer queries per chunk.
// (The extent is grid.x times the BLOCK size: a launch with several tiles per wave - kChunkRows / TPW threads, bbq_scan_body.h - has a TPW-th
// of the work-items on the same grid, so the limit of the one-tile kernel, which is the one tested here, holds for every TPW.)
constexpr uint64_t kGridWorkItemsMax = 0xFFFFFFFFull;
__host__ __device__ constexpr bool sweep_grid_fits(int n_chunks, int s) { return (uint64_t)sweep_grid_x(n_chunks, s) * (uint64_t)kChunkRows <= kGridWorkItemsMax; }
// the largest s <= want with 2^s <= n_queries - a launch co-schedules no more queries than it has - whose grid the device takes
__host__ __device__ constexpr int sweep_shift_for(int want, int n_queries, int n_chunks) {
  int s = want < 0 ? 0 : want;
  while (s > 0 && ((1 << s) > n_queries || !sweep_grid_fits(n_chunks, s))) --s;
  return s;
}
// the map hits every (chunk, query) pair of a launch exactly once: a pair covered twice would pass every parity test and only cost time
constexpr bool sweep_map_is_exact(int n_chunks, int n_queries, int s) {
  uint64_t hits[32] = {};  // one bit per pair (n_chunks * n_queries <= 2048)
  const uint32_t gx = sweep_grid_x(n_chunks, s), gy = sweep_grid_y(n_queries, s);
  int64_t covered = 0;
  for (uint32_t y = 0; y < gy; ++y)
    for (uint32_t x = 0; x < gx; ++x) {
      const SweepCoord c = sweep_coord(x, y, s);
      if (c.chunk_local < 0 || c.query < 0) return false;
      if (c.chunk_local >= n_chunks || c.query >= n_queries) continue;
      const int pair = c.query * n_chunks + c.chunk_local;
      if (hits[pair >> 6] >> (pair & 63) & 1u) return false;
      hits[pair >> 6] |= 1ull << (pair & 63);
      ++covered;
    }
  return covered == (int64_t)n_chunks * n_queries;
}
static_assert(sweep_grid_x(38, 0) == 38 && sweep_grid_y(37, 0) == 37 && sweep_coord(21, 5, 0).chunk_local == 21 && sweep_coord(21, 5, 0).query == 5,
              "s = 0 is the plain grid: (n_chunks, n_queries), blockIdx.x the chunk, blockIdx.y the query");
static_assert(sweep_map_is_exact(38, 37, 0) && sweep_map_is_exact(38, 37, 5) && sweep_map_is_exact(38, 37, 3) && sweep_map_is_exact(38, 5, 2),
              "n_chunks not a multiple of 8, n_queries not a multiple of P");
static_assert(sweep_map_is_exact(2, 32, 5) && sweep_map_is_exact(7, 9, 1) && sweep_map_is_exact(1, 1, 0) && sweep_map_is_exact(8, 32, 4), "n_chunks < 8, = 8");
static_assert(sweep_map_is_exact(19, 3, 5) && sweep_map_is_exact(16, 1, 3) && sweep_map_is_exact(40, 3, sweep_shift_for(5, 3, 40)), "n_queries < P");
static_assert(sweep_shift_for(5, 3, 40) == 1 && sweep_shift_for(3, 32, 40) == 3 && sweep_shift_for(5, 1, 40) == 0 && sweep_shift_for(0, 7, 40) == 0, "the cap by the query count");
// the cap by the grid's extent: 2^18 chunks x 32 queries would be 2^32 work-items in x
static_assert(sweep_grid_fits(262136, 5) && !sweep_grid_fits(262137, 5) && !sweep_grid_fits(1 << 18, 5) && sweep_grid_fits(1 << 18, 4), "grid.x * kChunkRows <= 2^32 - 1");
static_assert(sweep_shift_for(5, 32, 262136) == 5 && sweep_shift_for(5, 32, 1 << 18) == 4 && sweep_shift_for(5, 32, 1 << 19) == 3 && sweep_shift_for(5, 32, 1 << 20) == 2 &&
              sweep_shift_for(5, 32, 4000000) == 1 && sweep_shift_for(5, 32, 8388607) == 0 && sweep_grid_fits(8388607, 0), "a long launch co-schedules fewer queries");

constexpr int kChunkBytes = 16;
// code chunk j of row r inside a record: its index among the record's chunks, and its byte offset
__host__ __device__ constexpr int tile_chunk_index(int j, int r) { return j * kTileRows + r; }
__host__ __device__ constexpr size_t tile_chunk_offset(int j, int r) { return (size_t)tile_chunk_index(j, r) * kChunkBytes; }
// ... and of the corrections block, behind the w16 chunk blocks
__host__ __device__ constexpr size_t tile_corr_offset(int w16) { return (size_t)w16 * (kTileRows * kChunkBytes); }
// inline corrections block: [64] {lower, upper} at 0, [64] additionalCorrection, [64] quantizedComponentSum (has_x1 only)
constexpr int kCorrAddOffset = kTileRows * 16;
constexpr int kCorrSumOffset = kCorrAddOffset + kTileRows * 8;
constexpr int kCorrSumBytes = kTileRows * 8;
// compact corrections block: [64] compact words
constexpr int kCorrCompactBytes = kTileRows * 4;
// the compact word: the upper 16 bits (bf16 by truncation) of f32(lower) in its low half, of f32(upper) in its high half
__host__ __device__ inline uint32_t bf16_trunc_bits(double v) { return __builtin_bit_cast(uint32_t, (float)v) >> 16; }
__host__ __device__ inline uint32_t compact_word(double lower, double upper) { return bf16_trunc_bits(lower) | (bf16_trunc_bits(upper) << 16); }
__host__ __device__ inline float compact_lower(uint32_t cw) { return __builtin_bit_cast(float, cw << 16); }
__host__ __device__ inline float compact_upper(uint32_t cw) { return __builtin_bit_cast(float, cw & 0xffff0000u); }
// bytes of one tile record
__host__ __device__ inline int tile_stride_of(int w16, int layout, int has_x1) {
  return (int)tile_corr_offset(w16) + (layout == kLayoutCompact ? kCorrCompactBytes : kCorrSumOffset + (has_x1 ? kCorrSumBytes : 0));
}
__host__ __device__ inline int pb_of(const TileGeom &g) { return row_bytes_of(g.dim, g.store_bits); }  // stored bytes per row, before the padding
__host__ __device__ inline int bytes_per_row_of(const TileGeom &g) { return g.tile_stride / kTileRows; }
// the compact layout's row_sums side array exists iff the largest possible component sum of a row fits its 16 bits
__host__ __device__ inline bool row_sums_fit(const TileGeom &g) {
  return g.layout == kLayoutCompact && (int64_t)g.dim * ((1 << g.store_bits) - 1) <= 65535;
}
// where the build kernels write: the records of a storage (or a scratch tile set), the compact layout's side rows, and their geometry
struct TileDest {
  uint8_t *tiles;
  double *exact;  // kLayoutCompact: [rows padded to 64][4]; null otherwise
  TileGeom geom;
};
// rows staged in device memory in the caller's shape: codes [n][pb] packed bits (store_bits 1) or [n][dim] one byte per dimension,
// corr [n][4] {lower, upper, additionalCorrection, quantizedComponentSum}
struct StagedRows {
  const uint8_t *codes;
  const double *corr;
};

// A compaction (DESIGN.md "Removing rows"): which old row becomes new row R.  accept[t] is the accept word of source tile t (bit l =
// lane l, clear beyond the last row: a bbq_filter's d_bits), rank[t] the accepted rows in front of tile t, rank[src_tiles] = kept.
struct CompactMap {
  const uint64_t *accept;  // [src_tiles]
  const uint32_t *rank;    // [src_tiles + 1] exclusive prefix of the words' popcounts
  int64_t src_tiles;
  int64_t kept;            // |A| = rows afterwards
};
// the source tile of new row R < kept: the t in [lo, hi] with rank[t] <= R < rank[t + 1] (the caller knows it lies in that range)
__device__ __forceinline__ int64_t compact_source_tile(const CompactMap &m, int64_t R, int64_t lo, int64_t hi) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)m.rank[mid + 1] <= R) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// position of the k-th (from 0) set bit of w; w has more than k bits set
__device__ __forceinline__ int select_bit64(uint64_t w, int k) {
  int pos = 0;
  uint32_t x = (uint32_t)w;
  int c = __popc(x);
  if (k >= c) { k -= c; pos = 32; x = (uint32_t)(w >> 32); }
#pragma unroll
  for (int width = 16; width >= 1; width >>= 1) {
    c = __popc(x & ((1u << width) - 1u));
    if (k >= c) { k -= c; pos += width; x >>= width; }
  }
  return pos;
}
// the old row behind new row R < kept, for the lanes of one wave that own 64 consecutive new rows [R0, R0 + 64): the wave's first and
// last row bound every lane's search, and both are uniform
__device__ __forceinline__ int64_t compact_source_row(const CompactMap &m, int64_t R0, int64_t R) {
  const int64_t last = (R0 + kTileRows <= m.kept ? R0 + kTileRows : m.kept) - 1;
  const int64_t t_lo = compact_source_tile(m, R0, 0, m.src_tiles - 1);
  const int64_t t_hi = compact_source_tile(m, last, t_lo, m.src_tiles - 1);
  const int64_t t = compact_source_tile(m, R, t_lo, t_hi);
  return t * kTileRows + select_bit64(m.accept[t], (int)(R - (int64_t)m.rank[t]));
}

struct IndexView {
  const uint8_t *tiles;
  const double *exact;  // kLayoutCompact: [n_rows padded to 64][4]
  const float *add_range;  // kLayoutCompact: [tiles][2] {min, max} of additionalCorrection inside the tile
  int64_t n_rows;       // valid rows in this storage
  TileGeom geom;
  // cache residency of a launch (launch_view(), bbq_core.cpp): the chunks read with the default cache policy - they stay in the 256 MiB
  // Infinity Cache from one query's sweep to the next - the others are streamed with non-temporal loads
  int64_t resident_tiles;  // resident_share < 0: chunks whose first tile is below this
  int64_t resident_share;  // >= 0: chunk c is resident iff (c & 63) < resident_share (the resident chunks spread over the whole sweep)
  int64_t nt_delta;        // always 0.  The streamed loads add it to their address so that the compiler sees two different addresses
                           // in the two branches: it merges loads that differ only in the cache policy into ONE plain load
  const uint16_t *row_sums;  // kLayoutCompact: [tiles][64] each row's popcount / code sum, or null.  A storage's view holds the array where
                             // it exists (row_sums_fit); a LAUNCH's view carries it only where the per-query sparse sweep is to read the
                             // sum instead of counting it (option row_sums, row_sums_for_launch) - every other kernel ignores it
};
// the kernels' argument loads depend on these offsets
static_assert(offsetof(IndexView, geom) == 32 && sizeof(TileGeom) == 24 && offsetof(IndexView, resident_tiles) == 56 &&
                  offsetof(IndexView, row_sums) == 80 && sizeof(IndexView) == 88,
              "IndexView layout");

// Per-query uniforms of the score formula (src/batchDotProduct.ts:478-617)
struct QueryParams {
  double ay;     // query lowerInterval
  double ly;     // (upper-lower) [* FOUR_BIT_SCALE for every queryBits != 1]
  double y1;     // query quantizedComponentSum
  double qadd;   // query additionalCorrection
  double cdp;    // centroid . centroid
  double dimd;   // dimension as a double
  int32_t sim;   // BBQ_EUCLIDEAN / BBQ_COSINE / BBQ_MAXIMUM_INNER_PRODUCT
  int32_t one_bit;
  int32_t mip_plain;  // 1: MAXIMUM_INNER_PRODUCT is scaleMaxInnerProductScore(t) without the division by FOUR_BIT_SCALE: the
                      // per-row scorer's form (src/binaryQuantizedScorer.ts:207-209), which answers for multi-bit indexes
  int32_t fast_bound; // 1: the f32 images below are usable and the compact layout's score bound is tested in f32 against the threshold's
                      // z image (compact_bound_passes); 0: the f64 bound.  Decided by fill_query (fast_bound_images)
  // f32 images for the f32 bound, each computed in f64 and rounded once (k2mf and tinyf rounded up)
  float ayf, lyf;     // ay, ly
  float c1f;          // ay * dim + ly * y1
  float k2mf;         // 2^-20 * M, M >= |c1| + 2 (|ay| * x1max + |ly| * qcmax): the rounding allowance per unit of |al| + |au|
  float tinyf;        // the absolute allowance (denormal corrections, underflow)
  float csf, caf;     // z = cs * s + ca * add: (2, -1) EUCLIDEAN, (1, 1) otherwise
  uint32_t digit_k;   // K = pop(N_0) + 3 pop(N_1) of the query's digit masks (fill_query_digits); 0 where none are staged
};
static_assert(sizeof(QueryParams) == 96 && sizeof(QueryParams) % 16 == 0, "QueryParams: staged in arrays behind 16-byte query data, and part of kernel arguments");

// A query's threshold: the monotone key rows are tested against (a row is a candidate iff key(score) > key), and the same threshold
// in the linear space of the score formula, z = cs * s + ca * add (z_threshold, bbq_kernel_common.h): score > threshold => z > z image.
// The two live in ONE 8-byte word and are only ever written together (store_threshold): a key whose image is stale would reject rows
// that belong to the answer.  The image is stored XOR the bits of -inf, so that all-zero bytes - what the host resets the control words
// to - are {key 0, -inf}: everything is a candidate.
struct Threshold {
  uint32_t key;
  uint32_t zenc;
};
static_assert(sizeof(Threshold) == 8, "one 8-byte word per query");
constexpr uint32_t kZthXor = 0xff800000u;  // bits of -inf
__host__ __device__ inline float threshold_z(const Threshold &t) { return __builtin_bit_cast(float, t.zenc ^ kZthXor); }
__host__ __device__ inline Threshold make_threshold(uint32_t key, float z) { return Threshold{key, __builtin_bit_cast(uint32_t, z) ^ kZthXor}; }

struct ScanArgs {
  IndexView idx;
  const uint4 *qplanes;        // [Q][w16][QB] bit-planes of the quantized query, packed like the rows (multi-bit index: [Q][w16*4][QN]
                               // dwords, the query's nibbles / bytes in the field order of the row dwords, see tile_dot_multibit)
  const QueryParams *qparams;  // [Q]
  int64_t chunk_begin;         // first chunk of this launch inside idx
  int64_t row_id_base;         // global row id of idx row 0
  // sparse output (candidates above the per-query threshold)
  const Threshold *theta;      // [Q] monotone keys (and their z images); a row is a candidate iff key(score) > theta.key
  uint32_t *counts;            // [Q][n_chunks]
  uint64_t *entries;           // [Q][n_chunks][cap], ascending by row inside a chunk
  uint32_t *flags;             // [Q]
  int32_t cap;
  int32_t n_chunks;            // chunks in this launch (the slot and count arrays' stride; the grid's x extent follows from it, sweep_grid_x)
  // flood tier (may be null): a chunk with more than `cap` candidates parks ALL of them, row-ordered, in a block of the
  // query's overflow area and leaves counts = kCountRedirect | n, entries[0] = block offset (bbq_scan_kernel only)
  uint64_t *ovf;               // [Q][ovf_cap]
  uint32_t *ovf_counts;        // [Q] entries handed out so far
  int32_t ovf_cap;
  // the digit form of a 4-plane query against 1-bit rows (kDigitMasks above): [Q][w16][kDigitMasks] masks staged IN ADDITION to the
  // bit-planes and in the same buffer, qdigits_at 16-byte units behind qplanes; 0 - the caller staged none, and the launch runs the plane
  // form.  Read by the sparse sweep of bbq_scan_kernel's DG twin alone
  int32_t qdigits_at;
  // append mode (calls with few queries; null: chunk slots as above): a workgroup reserves room for its candidates right in the
  // query's list with ONE atomic and writes them there, unordered inside the segment - the finalize launch then has nothing to
  // compact (walking 19 K chunk counters cost it 20-30 us of a 250 us call).  The answer is selected on the device and does not
  // care about the order; the rare host replay (equal scores) sorts the list by row first.
  uint64_t *append_lists;      // [Q][append_cap]
  const int32_t *append_base;  // [Q][2]: entries the list holds from the earlier segments (list_counts)
  uint32_t *append_counts;     // [Q][kAppendStride] entries this launch has reserved so far (word 0 of each query's line)
  int64_t append_cap;
  // dense output (every row), indexed by row - chunk_begin*1024
  float *dense_score32;        // [Q][dense_stride] or null
  int32_t *dense_qcdist;       // or null
  double *dense_score64;       // or null
  int64_t dense_stride;
  // the workgroup -> (chunk, query) map of bbq_scan_kernel (sweep_coord): l2_shift = s, 2^s queries co-scheduled per chunk.  The caller
  // sets what it asks for (0: the plain grid); the launch caps it by its query count and by the grid's extent (sweep_shift_for) and fills in n_queries
  int32_t l2_shift;
  int32_t n_queries;
};
// (qdigits_at fills what was padding: eight more bytes of kernel arguments moved the register allocation of three existing instantiations)
static_assert(sizeof(ScanArgs) == 256 && offsetof(ScanArgs, qdigits_at) == 180 && offsetof(ScanArgs, append_lists) == 184, "ScanArgs layout");

struct FinalizeArgs {
  // input: either slots of one sparse launch, or the dense f32 scores of the first segment
  const uint32_t *counts;      // [Q][n_chunks]
  const uint64_t *entries;     // [Q][n_chunks][cap]
  const float *dense_score32;  // [Q][dense_stride]  (dense_rows > 0 selects this input)
  int64_t dense_stride;
  int32_t dense_rows;
  int64_t dense_row_id_base;
  int32_t n_chunks;
  int32_t cap;
  const uint64_t *ovf;         // flood tier of the scan launch (null: none)
  int32_t ovf_cap;
  uint32_t *append_counts;     // [Q][kAppendStride] non-null: the scan launch appended its candidates to the list itself (ScanArgs::append_lists);
                               // counts / entries are unused, the launch only takes the keys from list[base, base + count) and resets the counter
  // candidate list being built, ascending by global row
  uint64_t *lists;             // [Q][list_cap]
  int32_t *list_counts;        // [Q][2] {count, flags}
  int64_t list_cap;
  int32_t emit;                // 0: thresholds only (pilot replica on a shard that does not own those rows)
  // running top-k keys and the threshold for the next segment
  uint32_t *topk_keys;         // [Q][k]
  int32_t *topk_counts;        // [Q]
  Threshold *theta;            // [Q] written through store_threshold alone
  const QueryParams *qparams;  // [Q] the queries of the launch: a threshold's z image depends on its query.  Null: one query, `qp1`
  QueryParams qp1;             // the single-query chain's query (it lives in kernel arguments, not in device memory)
  uint32_t *flags;             // [Q]
  int32_t k;
  int32_t need_theta;          // 0 on the last segment
  // final selection (last segment only; null: none).  The caller runs the whole query with k = k2 + 1, so the running top keys
  // hold the (k2 + 1) largest keys seen: the launch then knows the (k2 + 1)-th largest f32 score of the whole index exactly,
  // gathers the k2 rows above it from the list, sorts them by score and checks that no two of them - and not the boundary -
  // compare equal.  In that case the reference's heap (src/binaryQuantizationFormat.ts:383-411) ends up holding exactly those rows
  // whatever its history was and pops them in ascending score order, so the answer is the descending sort (header slot 1 = {k2, 0}).
  // Any tie, NaN flag, list overflow, a flood beyond the key buffer or k2 > kFinalSelectMax leaves {0, 1} there: the host
  // replays the heap over the list as before.
  // final_out [Q][final_stride]: slot 0 = {list count, flags} (a copy of list_counts), slot 1 = {entries that follow, 1 = replay
  // the list on the host}, then the answer (global row << 32 | f32 score bits) descending by score: ONE device-to-host copy
  // brings everything the host needs
  uint64_t *final_out;
  int32_t final_stride;        // >= final_k + 2 (+ 3 in shard mode)
  int32_t final_k;             // k2 = min(k, rows of the index)
  // latency path: final_out is MAPPED HOST memory; after the answer the launch stores `seq` into *done_flag (system scope) - the host
  // polls it instead of waiting for a copy and an event - and leaves the query's control words clean for the next call (the chain has
  // no host-to-device copy that would reset them)
  uint64_t *done_flag;
  uint64_t seq;
  // Shard mode (bbq_shard_scan_begin's dev_answers, include/bbq.h): this storage is one row shard of a larger index and the running top
  // keys may include rows of a pilot replica, so the launch cannot prove an answer by itself.  It leaves what the merge needs instead:
  // slot 1 = {m, unproven}, slot 2 = the cut: at most the (k2 + 1)-th largest key of the rows this shard has seen, equal to it unless an
  // earlier segment overflowed the key buffer (m_use < m_new: the running top keys are a subset's); 0: it has seen at most k2.  Then the
  // m <= k2 listed rows above the cut, descending by score.  No tie check here: the merge checks the global answer.
  int32_t final_shard;
};
constexpr int kFinalSelectMax = 1024;  // largest k2 the finalize kernel selects and sorts itself

// Latency path (bbq_latency_kernels.hip + the finalize kernel): ONE query per call - the reference's own call shape - with no copy at
// either end: every sweep takes the query from its KERNEL ARGUMENTS, the last finalize launch writes the answer into mapped host
// memory and raises a sequence word the host is polling.
constexpr int kLatPlaneMax = 96;     // 16-byte blocks of staged query data that fit the kernel arguments (768-d / 1536-d x 4 planes: 24 / 48)
struct LatScanArgs {
  IndexView idx;
  int64_t row_id_base;
  int64_t chunk_begin;
  int32_t n_chunks;
  int32_t first;                     // 1: the dense prefix - threshold 0 (every row is listed), nothing listed before it
  const Threshold *theta;            // the query's control words (device memory), as ScanArgs has them per query
  uint32_t *flags;
  const int32_t *list_counts;        // {count, flags}: entries the list holds from the earlier segments
  uint32_t *append_count;
  uint64_t *list;
  int64_t list_cap;
  // the query itself, in the arguments of every launch of the chain
  QueryParams p;
  uint4 planes[kLatPlaneMax];
};

// Pre-sampled threshold (the first step of the single-query call on large indexes): the first `rows` rows are scored exactly, every
// wave leaves the `per_wave` largest keys of its 64 rows, and one small launch selects the rank-th largest of all of them - the
// k-th largest of a SUBSET of the rows is a valid lower bound of the k-th largest of the index, and with per_wave = 4 it is the
// prefix's true order statistic unless one wave holds five of its best rows.  ONE sweep over all rows with that threshold then lists
// every row above it (a few thousand) and the final selection works on that list alone.
constexpr int kLatPreKeys = 12288;  // keys the selection launch takes (48 KB of LDS; = kFinalizeKeyCap, what the final selection holds)
struct LatPreArgs {
  IndexView idx;
  int32_t rows;                      // rows [0, rows) are sampled (a multiple of kChunkRows, <= idx.n_rows)
  int32_t per_wave;                  // 1..4 keys per wave
  uint32_t *pre_keys;                // [rows / 64 * per_wave]
  uint32_t *flags;                   // NaN scores raise kFlagNaN
  QueryParams p;
  uint4 planes[kLatPlaneMax];
};

// exact rerank (bbq_rerank_kernels.hip): candidates of query q are rows[offsets[q] .. offsets[q+1])
struct RerankArgs {
  const float *vecs;       // [n][dim] original fp32 rows, row-major
  int64_t n;
  int32_t dim;
  int32_t sim;             // 0 EUCLIDEAN, 1 COSINE, 2 MAXIMUM_INNER_PRODUCT
  const float *queries;    // [Q][dim] raw fp32 queries
  const int64_t *offsets;  // [Q+1]
  const int32_t *rows;     // [offsets[Q]] row numbers, all in [0, n)
  double *out;             // [offsets[Q]] computeSimilarity(query, row)
};

// scoring chosen rows (bbq_gather_kernels.hip): query q is scored against the rows ords[offsets[q] .. offsets[q+1]), one lane per entry
constexpr int kGatherThreads = 256;  // entries per workgroup (four waves share the staged query)
struct GatherArgs {
  IndexView idx;
  const uint4 *qplanes;        // [Q][w16][QU] staged query data, as ScanArgs::qplanes
  const QueryParams *qparams;  // [Q]
  const int64_t *offsets;      // [Q+1] ascending from 0
  const int32_t *ords;         // [offsets[Q]] rows of idx, all in [0, idx.n_rows): the host has checked every one
  // outputs, indexed like ords; each may be null
  int32_t *out_qcdist;
  double *out_score64;
  float *out_score32;
};

// range search (bbq_range_kernels.hip): every row of the index whose f32 score key beats the caller's threshold, count-then-fill.  The
// count pass leaves counts[q][chunk]; bbq_range_offsets_kernel turns them IN PLACE into each chunk's offset inside its query's answer
// and lists the chunks that hold a row; the fill pass sweeps those chunks once more and writes every passing row at
// base[q] + chunk_off[q][chunk] + its rank inside the chunk: the answer comes out ascending by row without an atomic.
constexpr int kRangeOffsetsThreads = 1024;
struct RangeArgs {
  IndexView idx;
  const uint4 *qplanes;        // [Q][w16][QU] staged query data, as ScanArgs::qplanes
  const QueryParams *qparams;  // [Q]
  const Threshold *theta;      // [Q] written by bbq_range_theta_kernel from the host's keys (bbq_range_key)
  const uint64_t *accept;      // [tiles of idx] the accept words of a filter, or null: every row
  int32_t n_chunks;            // chunks of idx: the stride of the three per-chunk arrays
  int32_t q_first;             // the launch's first query (blockIdx.y counts from it)
  uint32_t *counts;            // count pass: [Q][n_chunks] passing rows of each chunk
  // fill pass
  const uint32_t *chunk_off;   // [Q][n_chunks] passing rows of the query in front of each chunk (the counts, scanned in place)
  const uint32_t *nonempty;    // [Q][n_chunks] the chunks with a passing row, ascending; n_nonempty[q] of them
  const uint32_t *n_nonempty;  // [Q]
  const int64_t *base;         // [Q] where the query's answer starts inside `out`
  uint64_t *out;               // entries (row << 32 | f32 score bits) of the launch's queries, back to back
};

// span search (bbq_span_kernels.hip): the k best rows among each query's own contiguous spans of rows.  The score pass leaves the f32
// score of every visited row of query q at scores[q's base + the row's position in q's visiting order]; the select pass finds each
// selected query's (k + 1)-th largest score key and writes the rows above it.  With a row filter (bbq_search_spans_filtered_batch) only
// the accepted rows of the spans are visited: the positions are those of the COMPACTED visiting order, and the score pass leaves each
// accepted row's ord beside its score, in a parallel array the select pass reads only for its k winners.
constexpr int kSpanSelectMax = 4096;  // largest k the select pass takes
// one workgroup of the score pass: the rows [row_lo, row_hi) of one span, cut by the host at tile-aligned kChunkRows-row steps, so
// row_lo >> 6 == first_tile and row_hi <= (first_tile + kTilesPerChunk) * 64
struct SpanItem {
  uint32_t query;       // of the sub-batch
  uint32_t first_tile;  // wave w takes tile first_tile + w
  uint32_t row_lo, row_hi;
  int64_t out;          // scores[out + (r - row_lo)] takes row r; filtered: out = the position of the item's first accepted row
};
static_assert(sizeof(SpanItem) == 24, "SpanItem: staged in an array behind 8-byte data");
struct SpanScoreArgs {
  IndexView idx;
  const uint4 *qplanes;        // [Q][w16][QU] staged query data, as ScanArgs::qplanes
  const QueryParams *qparams;  // [Q]
  const SpanItem *items;       // [grid.x] the launch's first item
  float *scores;               // the sub-batch's scores, query by query
  const uint64_t *accept;      // filtered: the filter's words (word t = tile t, bit l = lane l); null otherwise
  uint32_t *ords;              // filtered: ords[i] = the row whose score is scores[i]
};
// a non-empty span of a query in its visiting order: position `pos` of the query's scores is row `begin`
struct SpanRun { int64_t pos, begin; };
// a query of the select pass
struct SpanQuery {
  int64_t score_off;  // its scores start at scores[score_off] ...
  int64_t len;        // ... and there are len > k of them
  int64_t run_first;  // its runs: runs[run_first .. run_first + n_runs); a filtered query has none
  int32_t n_runs;
  int32_t pad;
};
struct SpanSelectArgs {
  const float *scores;
  const SpanQuery *sel;   // [grid.x]
  const SpanRun *runs;
  const uint32_t *ords;   // filtered: the row of every score (SpanScoreArgs::ords), runs is unused; null otherwise
  uint64_t *out;          // [grid.x][out_stride]: {rows above the cut | flags << 32}, the cut's f32 bits, then k entries if there are exactly k
  int32_t k;              // 1 .. kSpanSelectMax
  int32_t out_stride;     // >= k + 2
};

// grouped search (bbq_group_kernels.hip): the k best GROUPS of rows - contiguous runs, a document's chunks - each through its best
// accepted row, its representative.  The score pass sweeps every chunk for every query of a sub-batch and leaves each live group's
// representative as a packed key in rep[q][slot]; the unpack pass turns the keys into the parallel scores / ords arrays the span
// search's select pass takes.  The tables are those of one group set (bbq_groups, bbq_group.cpp), built once at its creation:
//   starts[t]       bit l = row 64 t + l is the first row of a non-empty group (an empty group has no row and no bit); the row behind
//                   the last one counts as a start too, and so does row 0 of the tile behind the last one (starts[tiles] = 1): every
//                   group ends in front of a set bit
//   first_group[t]  the group row 64 t lies in, counted over the non-empty groups
//   slot[g]         of non-empty group g: its rank among the live groups - those with an accepted row - or -1
struct GroupScoreArgs {
  IndexView idx;
  const uint4 *qplanes;         // [Q][w16][QU] staged query data, as ScanArgs::qplanes
  const QueryParams *qparams;   // [Q]
  const uint64_t *accept;       // the accept words of the group set's filter (word t = tile t, bit l = lane l); null: every row
  const uint64_t *starts;       // [tiles + 1]
  const uint32_t *first_group;  // [tiles + 1]
  const int32_t *slot;          // [non-empty groups + 1]
  unsigned long long *rep;      // [Q][live] cleared to 0 before the launch: only ever raised (group_key)
  int64_t live;
  int32_t n_chunks;             // chunks of idx: the grid's x extent follows from it (sweep_grid_x)
  int32_t n_queries;
  int32_t l2_shift;             // the workgroup -> (chunk, query) map, as ScanArgs::l2_shift: the launch caps it (sweep_shift_for)
  int32_t pad;
};
// a row's packed key: larger = the better representative.  A NaN score ranks below every number, numbers in the order of their score
// keys, and among equals the lowest ord wins.  Never 0 for a row of an index of at most kGroupMaxRows rows: 0 = nothing seen
constexpr int64_t kGroupMaxRows = 0x7fffffff;
__host__ __device__ inline unsigned long long group_key(uint32_t score_bits, bool is_nan, uint32_t ord) {
  return ((unsigned long long)(is_nan ? 0u : key_of_bits(score_bits)) << 32) | (0x7fffffffu - ord);
}
constexpr uint32_t kGroupNaNBits = 0x7fc00000u;  // the score a representative with key 0 is unpacked to: a quiet NaN
__host__ __device__ inline uint32_t group_key_score_bits(unsigned long long k) { return (uint32_t)(k >> 32) ? bits_of_key((uint32_t)(k >> 32)) : kGroupNaNBits; }
__host__ __device__ inline uint32_t group_key_ord(unsigned long long k) { return 0x7fffffffu - (uint32_t)k; }

// MaxSim search (bbq_maxsim_kernels.hip): a query is a run of token vectors and a live group scores the sum, in ascending token, of its
// representatives' f32 scores for them.  A query's tokens are worked through in blocks of at most kMaxSimTokenBlock: a block's score
// pass leaves the packed key of every (token, live group) in rep[token of the block][slot] - the grouped search's pass with the block's
// token vectors as its queries, or the fused pass that loads a tile once for all of a query's tokens of the block - and the accumulate
// pass adds them into acc[query][slot], an f64 that lives across the blocks; behind a query's last block it leaves scores[query][slot]
// and ords[query][slot] = the slot's group number, which the span search's select pass takes as they are.
// kMaxSimTokenBlock: the fused pass keeps a block's planes (64 W bytes a token, W <= 12), uniforms (96) and edge slots (128) in LDS -
// 31 KB at the widest row, under the 40 KB at which four workgroups of eight waves, all a CU holds, still fit its 160 KB.
constexpr int kMaxSimTokenBlock = 32;
constexpr int kMaxSimFirst = 1, kMaxSimLast = 2;  // MaxSimQuery::flags
struct MaxSimQuery {
  int32_t vec_first;  // its first token vector of this block among the block's staged vectors; the rest follow it
  int32_t n_tok;      // 1 .. kMaxSimTokenBlock
  int32_t query;      // of the sub-batch: its row of acc, scores and ords
  int32_t flags;      // kMaxSimFirst: the block holds its token 0 - acc is initialised, not read; kMaxSimLast: its last token - scores and ords are written
};
struct MaxSimAccArgs {
  const unsigned long long *rep;  // [the block's vectors][live]
  const MaxSimQuery *queries;     // [grid.y]
  double *acc;                    // [sub-batch's queries][live]
  float *scores;                  // the same shape
  uint32_t *ords;                 // the same shape
  const int32_t *live_group;      // [live] the group number of every slot; null (MaxSim over chosen groups): ords is not written
  int64_t live;
};
struct MaxSimScoreArgs {
  GroupScoreArgs g;            // qplanes / qparams / rep: per staged VECTOR of the block; n_queries: the length of `queries`
  const MaxSimQuery *queries;  // a workgroup is one chunk for one of them
};

// MaxSim over chosen groups (bbq_maxsim_cand_kernels.hip): a query scores its own candidate list, groups of a group set in the caller's
// order, duplicates included.  The rows of a query's candidates, back to back in list order, are its EXPANDED rows; a lane of the score
// pass is one of them.  The host stages one record per candidate - never a row list - and per query one more behind them, {0, total}.
// Entry e of a query is its e-th candidate: token t's key goes to rep[vec_first + t][e], the rows of the three keyed arrays `stride`
// entries long (the longest list of the sub-batch); MaxSimAccArgs::live is that stride and live_group is null.
constexpr int kMaxSimCandThreads = 256;  // expanded rows per workgroup (four waves share the staged token block)
constexpr int64_t kMaxSimCandMaxRows = 0x7fffffff;  // of one query's expanded rows
struct MaxSimCand {
  uint32_t first_row;  // the candidate group's first row
  uint32_t pos;        // its first row's position among the query's expanded rows: the prefix sum of the group lengths in front of it
};
struct MaxSimCandQuery {
  int64_t rec_first;  // its records: recs[rec_first .. rec_first + n_cand], the last one the terminator
  int32_t n_cand;     // >= 1 for a query that is launched
  int32_t total;      // its expanded rows = recs[rec_first + n_cand].pos
};
static_assert(sizeof(MaxSimCand) == 8 && sizeof(MaxSimCandQuery) == 16, "staged in arrays behind 8-byte data");
struct MaxSimCandArgs {
  IndexView idx;
  const uint4 *qplanes;           // [the block's vectors][w16][QU] staged query data, as ScanArgs::qplanes
  const QueryParams *qparams;     // [the block's vectors]
  const uint64_t *accept;         // the accept words of the group set's filter; null: every row
  const MaxSimQuery *queries;     // [grid.y] the token block of each query that has one; .query indexes cq
  const MaxSimCandQuery *cq;      // [sub-batch's queries]
  const MaxSimCand *recs;
  unsigned long long *rep;        // [the block's vectors][stride] cleared to 0 before the launch: only ever raised (group_key)
  int64_t stride;
  int32_t tok_pass;               // tokens a workgroup stages in LDS at a time: kMaxSimTokenBlock unless the row is too wide for that
  int32_t pad;
};

// Exact MaxSim rerank (bbq_maxsim_rerank_kernels.hip): the candidate lists and records of MaxSim over chosen groups, scored against the
// fp32 rows of a bbq_vectors with computeSimilarity's f64 chain.  A workgroup is one wave: 64 expanded rows of one query, each row loaded
// once per token block and run against every token of the block.  A query's block takes tp = its token count rounded up to
// kMaxSimRerankTokenGroup vector SLOTS: MaxSimQuery::vec_first counts slots (a multiple of the group), its token t of the block at column
// j is tokens[vec_first * dim + j * tp + t] - the host widens the raw f32 to f64, which is exact, lays a column's tokens side by side, so
// that the tokens of a run of columns are one contiguous, 64-byte aligned piece for the kernel to stage, and pads with 0.0 - and
// na[vec_first + t] is the token's squared norm, the reference's na chain, which depends on the token alone.  Token t's key goes to
// rep[vec_first + t][e]; a slot that pads is never written or read.
constexpr int kMaxSimRerankThreads = 64;    // expanded rows per workgroup
constexpr int kMaxSimRerankTokenGroup = 8;  // tokens a chain step takes together: a query pays for whole groups
struct MaxSimRerankArgs {
  const float *vecs;              // [n_rows][dim] the fp32 rows, row-major
  const double *tokens;           // the block's token vectors, as above; 16-byte aligned
  const double *na;               // [the block's slots]; read for COSINE only
  const uint64_t *accept;         // the accept words of the group set's filter; null: every row
  const MaxSimQuery *queries;     // [grid.y] the token block of each query that has one; .query indexes cq
  const MaxSimCandQuery *cq;      // [sub-batch's queries]
  const MaxSimCand *recs;
  unsigned long long *rep;        // [the block's slots][stride] cleared to 0 before the launch: only ever raised (true_key)
  int64_t stride;
  int32_t dim;
  int32_t sim;                    // 0 EUCLIDEAN, 1 COSINE, 2 MAXIMUM_INNER_PRODUCT
};
// an f64 score's key: larger = the greater score, -0.0 below +0.0; a NaN's is 1, below every number's (-Inf: 0x000fffffffffffff);
// 0 = nothing seen
constexpr unsigned long long kTrueNaNBits = 0x7ff8000000000000ull;  // the one NaN the exact MaxSim calls write
__host__ __device__ inline unsigned long long true_key(unsigned long long bits, bool is_nan) {
  return is_nan ? 1ull : (bits >> 63) ? ~bits : bits | 0x8000000000000000ull;
}
__host__ __device__ inline unsigned long long true_key_bits(unsigned long long k) {
  return k <= 1ull ? kTrueNaNBits : (k >> 63) ? k ^ 0x8000000000000000ull : ~k;
}
// the accumulate pass behind it: acc[query][entry] takes the block's decoded keys in ascending token, from the first token's and not
// from 0.0; behind a query's last block a NaN sum is replaced by kTrueNaNBits
struct MaxSimTrueAccArgs {
  const unsigned long long *rep;  // [the block's slots][stride]
  const MaxSimQuery *queries;     // [grid.y]
  double *acc;                    // [sub-batch's queries][stride]: lives across the blocks, the true scores behind the last
  int64_t stride;
};

// Exact search (bbq_exact_kernels.hip): the true top-k of a block of independent raw queries over the CONTIGUOUS fp32 rows of a
// bbq_vectors, a slab of rows at a time.  The score pass is the exact MaxSim rerank's chain with the row known from the lane: a wave is
// the 64 rows of one accept word, a workgroup runs them against one block of up to kExactQueryBlock queries and leaves
// keys[query][row - row0] = true_key of c(query, row), 0 for a row the filter rejects; a wave without an accepted row loads and writes
// nothing.  The queries are staged as MaxSimRerankArgs::tokens are: block b's slots start at b * kExactQueryBlock, its tp = its query
// count rounded up to kMaxSimRerankTokenGroup, query t of the block at column j is queries[b * kExactQueryBlock * dim + j * tp + t],
// na[b * kExactQueryBlock + t] its squared norm.  The select pass keeps per query the best kk (key, row) pairs seen so far, sorted by
// key descending and row ascending - a strict order, so the list is the answer - and folds a slab into it: a key is looked at only if
// it beats the list's last key (every row of a later slab is behind every listed row, so an equal key loses), what passes is merged in
// by sorting list and candidates together.  It reads the accept word itself and never a key the score pass did not write.
constexpr int kExactQueryBlock = 32;
constexpr int kExactSelectThreads = 1024;
constexpr int kExactSelectMax = 4096;                     // largest kk the select pass takes
constexpr int kExactSelectSlots = 2 * kExactSelectMax;    // (key, row) pairs it sorts at a time: the list and a tile of candidates
constexpr int kExactSelectTile = 4 * kExactSelectThreads; // rows it tests between two barriers: four consecutive keys a thread
constexpr int kExactSelectLdsBytes = kExactSelectSlots * 12;
struct ExactScoreArgs {
  const float *vecs;              // [n][dim] the fp32 rows, row-major
  const double *queries;          // the sub-batch's queries, as above; 16-byte aligned
  const double *na;               // [slots]; read for COSINE only
  const uint64_t *accept;         // the accept words of a filter (word t = rows 64 t .. 64 t + 63); null: every row
  unsigned long long *keys;       // [sub-batch's queries][stride]
  int64_t n;                      // rows in use
  int64_t row0;                   // the slab's first row, a multiple of 64
  int64_t stride;                 // slab rows the key rows are long
  int32_t n_queries;              // of the sub-batch
  int32_t dim;
  int32_t sim;                    // 0 EUCLIDEAN, 1 COSINE, 2 MAXIMUM_INNER_PRODUCT
  int32_t pad;
};
struct ExactSelectArgs {
  const unsigned long long *keys; // [grid.x][stride]
  const uint64_t *accept;         // as ExactScoreArgs::accept
  unsigned long long *list_keys;  // [grid.x][kk] the running lists, best first
  int32_t *list_rows;             // [grid.x][kk]
  int32_t *list_count;            // [grid.x] cleared before the first slab
  int64_t n, row0, stride;        // as ExactScoreArgs'
  int32_t rows;                   // rows of this slab: [row0, row0 + rows), rows <= stride, row0 + rows <= n rounded up to 64
  int32_t kk;                     // 1 .. kExactSelectMax
};
// the accept word of the 64 rows from row w * 64 on: the filter's, or every row below n
__host__ __device__ inline unsigned long long exact_accept_word(const uint64_t *accept, int64_t n, int64_t w) {
  if (accept) return accept[w];
  const int64_t left = n - w * 64;
  return left >= 64 ? ~0ull : left <= 0 ? 0ull : (1ull << left) - 1ull;
}

constexpr int kFinalizeThreads = 1024;
constexpr int kFinalizeJobs = 4096;     // non-empty chunks one finalize launch copies entry-parallel (more: thread by thread)
constexpr int kFinalizeKeyCap = 12288;   // LDS key buffer of the finalize kernel (new keys + running top-k)
constexpr int kFinalizeCountCap = 24576; // chunk counters one launch stages in LDS, 16 bits each (12.6 M rows per segment; longer segments read them from memory)
constexpr int kFinalizeLdsBytes = (kFinalizeKeyCap + 3 * kFinalizeJobs + 512 + 16 + 16) * 4 + kFinalizeCountCap * 2;  // 146 KB of the CU's 160 KB
// a finalize launch behind an appending or a dense sweep: keys, histogram, scratch and the 8 KB of the job table the final selection sorts in
constexpr int kFinalizeLdsBytesSmall = (kFinalizeKeyCap + 512 + 16 + 16) * 4 + kFinalSelectMax * 8;

}  // namespace bbq
