// bbq_scan_body.h - the per-query sweep (bbq_scan_kernel), unfiltered and filtered from one template, and the dispatch over its
// instantiations.  Included by bbq_kernels.hip (FILT = false) and bbq_filter_kernels.hip (FILT = true): each
// translation unit instantiates its own kernels only.
#pragma once
#include <hip/hip_runtime.h>
#include "bbq_device.h"
#include "bbq_kernel_common.h"

#pragma clang fp contract(off)

namespace bbq {

// Multi-bit index rows (indexBits > 1): qcDist = sum_d q[d] * x[d] (computeQuantizedDotProduct, src/bitwiseDotProduct.ts:14-30)
// over SB-bit fields with the packed-nibble / packed-byte dot instructions - 8 (v_dot8_u32_u4) or 4 (v_dot4_u32_u8) exact
// integer products per lane and instruction.  2-bit fields are unfolded in registers into two dwords of nibbles (even / odd
// fields: one AND, one shift + AND); query values above 15 (QB == 8) are split into low and high nibbles,
// q = lo + 16 hi, so the dot is dot(x, lo) + 16 dot(x, hi).  s_q holds, per row dword, the matching query dwords
// (query_units_per_chunk; written by the host in exactly this order).  `sum` = the row's component sum (= quantizedComponentSum
// of a freshly quantized row, src/optimizedScalarQuantizer.ts:204-209) - left alone with SUM false: the caller has it from the row_sums
// side array.
template <int QB, int SB, bool SUM = true>
__device__ __forceinline__ void dot_chunk_multibit(const u32x4 c, const uint32_t *__restrict__ sq, uint32_t &lo, uint32_t &hi, uint32_t &sum) {
  const uint32_t x[4] = {c.x, c.y, c.z, c.w};
  constexpr int QN = query_units_per_chunk(QB, SB);  // query dwords per row dword
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const uint32_t *__restrict__ qw = sq + t * QN;
    if constexpr (SB == 2) {
      const uint32_t e = x[t] & 0x33333333u, o = (x[t] >> 2) & 0x33333333u;
      lo = __builtin_amdgcn_udot8(e, qw[0], lo, false);
      lo = __builtin_amdgcn_udot8(o, qw[1], lo, false);
      if constexpr (QB > 4) {
        hi = __builtin_amdgcn_udot8(e, qw[2], hi, false);
        hi = __builtin_amdgcn_udot8(o, qw[3], hi, false);
      }
      if constexpr (SUM) sum = __builtin_amdgcn_udot8(e + o, 0x11111111u, sum, false);  // nibbles of e + o are at most 6
    } else if constexpr (SB == 4) {
      lo = __builtin_amdgcn_udot8(x[t], qw[0], lo, false);
      if constexpr (QB > 4) hi = __builtin_amdgcn_udot8(x[t], qw[1], hi, false);
      if constexpr (SUM) sum = __builtin_amdgcn_udot8(x[t], 0x11111111u, sum, false);
    } else {
      lo = __builtin_amdgcn_udot4(x[t], qw[0], lo, false);
      if constexpr (SUM) sum = __builtin_amdgcn_udot4(x[t], 0x01010101u, sum, false);
    }
  }
}

template <int QB, int W, int SB, bool SUM = true>
__device__ __forceinline__ void tile_dot_multibit(const u32x4 (&c)[W], const u32x4 *__restrict__ s_planes, uint32_t &qc, uint32_t &sum) {
  const uint32_t *__restrict__ sq = reinterpret_cast<const uint32_t *>(s_planes);
  constexpr int QN = query_units_per_chunk(QB, SB);
  uint32_t lo = 0, hi = 0;
  if constexpr (SUM) sum = 0;
#pragma unroll
  for (int j = 0; j < W; ++j) dot_chunk_multibit<QB, SB, SUM>(c[j], sq + j * 4 * QN, lo, hi, sum);
  qc = lo + (hi << 4);
}
template <int QB, int SB, bool SUM = true>
__device__ __forceinline__ void tile_dot_multibit_any(const uint8_t *__restrict__ tp, int lane, int w16, const u32x4 *__restrict__ s_planes,
                                                      uint32_t &qc, uint32_t &sum) {
  const u32x4 *__restrict__ cp = reinterpret_cast<const u32x4 *>(tp) + lane;
  const uint32_t *__restrict__ sq = reinterpret_cast<const uint32_t *>(s_planes);
  constexpr int QN = query_units_per_chunk(QB, SB);
  uint32_t lo = 0, hi = 0;
  if constexpr (SUM) sum = 0;
  for (int j = 0; j < w16; ++j) {
    const u32x4 c = BBQ_STREAM_LOAD(cp + j * kTileRows);
    dot_chunk_multibit<QB, SB, SUM>(c, sq + j * 4 * QN, lo, hi, sum);
  }
  qc = lo + (hi << 4);
}

// The instantiations whose waves issue their tile's loads in front of the query staging and the first barrier (EARLY in the kernel): the sparse
// sweeps of a compile-time width.  The run-time width streams its row chunk by chunk behind the staging and dense launches are bound by their
// writes: both keep their order.  An instantiation that the early order would cost a wave of occupancy is excluded here (docs/dropped.md,
// "early loads").  To check again: build both kernel files with -Rpass-analysis=kernel-resource-usage with and without the exclusion and
// compare VGPRs / Occupancy / ScratchSize of every bbq_scan_kernel instantiation (scripts/scan_resources.py).
template <bool FILT, int QB, int W, int MODE, int SB, bool RS, bool DG>
constexpr bool early_loads() {
  if (W == 0 || (MODE & 1)) return false;
  // The filtered family keeps its order: there the masks' load stands behind the branch on the tile's accept word, a memory round trip of
  // its own, and where most tiles of a filter are empty most staging waves paid the two in series: measured at 10 M x 768-d, +3.4 % under
  // dense filters, -9 % with 0.1 % of the rows accepted and -16 % with 1000 rows (Measurement; docs/dropped.md).
  if (FILT) return false;
  // the nine that came out of this build's compiler (ROCm 7.2) with a wave of occupancy less in the early order: five unfiltered sweeps of the
  // inline layout at 12 chunks (72 -> 74 vector registers, 7 -> 6 waves) and one filtered sweep of the compact layout (72 -> 118, 7 -> 4)
  if (MODE == 0 && W == 12 && !FILT && ((SB == 1 && QB <= 2) || (SB == 2 && QB == 4) || SB == 4)) return false;
  if (MODE == 2 && W == 12 && SB == 1 && QB == 8 && !RS && FILT) return false;
  // ... and three compact sweeps of 4-bit rows at 16 chunks that count the sum themselves (80 -> 82, 6 -> 5 waves)
  if (MODE == 2 && W == 16 && SB == 4 && !RS && (QB == 8 || FILT)) return false;
  return true;
}

// ---- several tiles per wave (TPW in the kernel; option tiles_per_wave).  A workgroup of the TPW form has kTilesPerChunk / TPW waves and wave w
// sweeps the TPW consecutive tiles wave_first_tile(TPW, w) ... + TPW - 1 of its chunk one after the other: what belongs to the workgroup or is
// wave-uniform - the map, the query's uniforms, the staging and its barrier, the residency test, the tile's addresses, the end of the chunk -
// is executed once for TPW tiles instead of once per tile.
__host__ __device__ constexpr int wave_first_tile(int tpw, int wave) { return wave * tpw; }
// the map covers the tiles of a chunk exactly once: a tile swept twice would list its rows twice, one left out would only lose rows
constexpr bool wave_tiles_are_exact(int tpw) {
  if (tpw < 1 || kTilesPerChunk % tpw != 0) return false;
  int hits[kTilesPerChunk] = {};
  for (int w = 0; w < kTilesPerChunk / tpw; ++w)
    for (int t = 0; t < tpw; ++t) {
      const int tile = wave_first_tile(tpw, w) + t;
      if (tile < 0 || tile >= kTilesPerChunk) return false;
      ++hits[tile];
    }
  for (int i = 0; i < kTilesPerChunk; ++i)
    if (hits[i] != 1) return false;
  return true;
}
static_assert(wave_tiles_are_exact(1) && wave_tiles_are_exact(2) && wave_tiles_are_exact(4) && wave_tiles_are_exact(8), "1, 2, 4 and 8 tiles per wave");
static_assert(!wave_tiles_are_exact(0) && !wave_tiles_are_exact(3) && !wave_tiles_are_exact(16), "no other count divides a chunk's tiles");

// The end of a chunk for a workgroup of NT threads, as bbq_scan_kernel's body has it (sparse modes): the second barrier, then the append
// path, or the chunk's slot - the flood tier where the slot does not hold the candidates - and the count word.  Used by the kernels with
// several tiles per wave alone; the one-tile kernels keep theirs inline.
template <int NT>
__device__ __forceinline__ void sweep_chunk_end(const ScanArgs &a, const SweepCoord wg, const int q, uint64_t *s_ent, uint32_t *s_cnt) {
  const int tid = threadIdx.x;
  __syncthreads();
  if (a.append_lists) {  // workgroup-uniform
    const uint32_t cnt = *s_cnt;
    if (cnt == 0) return;
    __syncthreads();  // everyone has read *s_cnt: it takes the reserved offset
    append_to_list<NT>(s_ent, cnt, a.append_counts + (size_t)q * kAppendStride, a.append_base[2 * q], a.append_lists + (size_t)q * a.append_cap,
                       a.append_cap, a.flags + q, s_cnt);
    return;
  }
  uint32_t cnt = *s_cnt;
  uint64_t *__restrict__ slot0 = a.entries + ((size_t)q * a.n_chunks + wg.chunk_local) * (size_t)a.cap;
  uint64_t *__restrict__ out = slot0;
  uint32_t count_word = cnt;
  if (cnt > (uint32_t)a.cap) {  // workgroup-uniform
    bool parked = false;
    if (a.ovf) {
      // flood (e.g. rows stored cluster by cluster and this is the query's cluster): one block of the query's overflow
      // area takes the whole chunk, so the list stays row-ordered and the query stays on the sparse path
      __syncthreads();  // everyone has read *s_cnt
      if (tid == 0) *s_cnt = atomicAdd(a.ovf_counts + q, cnt);
      __syncthreads();
      const uint32_t off = *s_cnt;
      if ((uint64_t)off + cnt <= (uint64_t)a.ovf_cap) {
        out = a.ovf + (size_t)q * a.ovf_cap + off;
        count_word = kCountRedirect | cnt;
        if (tid == 0) slot0[0] = off;
        parked = true;
      }
    }
    if (!parked) {
      if (tid == 0) atomicOr(a.flags + q, kFlagOverflow);
      cnt = min(cnt, (uint32_t)a.cap);
      count_word = cnt;
    }
  }
  write_ranked(s_ent, cnt, out, tid, NT);
  if (tid == 0) a.counts[(size_t)q * a.n_chunks + wg.chunk_local] = count_word;
}

// The sweep of a wave's TPW > 1 tiles: the digit form of the unfiltered compact sweep (MODE 2, RS, DG) in the early order, nothing else.
// Tile 0 is loaded in front of the staging and the barrier exactly as the TPW = 1 kernel loads its one tile (the same two arms of the scalar
// branch, the masks the oldest load in flight); tile t + 1's nine loads are issued behind tile t's bound - the code registers and the three
// small words' registers are all dead there, so nothing is copied and no two tiles' codes are held at once - and its popcounts count the
// chunks down as they arrive.  The loop over the wave's tiles is unrolled: as a loop, the next tile's words came back in registers of their
// own and the copies at the back edge waited for every load of the tile.  The loads go through a buffer descriptor per tile, rebased with
// scalar arithmetic (tile_buffer, above); a lane's offsets are computed once per wave.  A wave whose next tile lies beyond the index leaves:
// the tiles are consecutive.  The rows beyond the index - in its last tile alone - are taken out of the bound's ballot by a scalar mask.
// Per row it computes what the kernel computes: the same integer and the same f32 bound.  What only the rows that pass the bound need - the
// f64 bound of a query without f32 images, the exact corrections, the f64 score, the key test, the candidate - is NOT in the tile loop
// (99.9 % of the rows never get there, and unrolled TPW times it held the f64 half of the query, the side array's base and the f64 temporaries
// live across every tile: 103 scalar registers and a wave less at 4 and 8 tiles): a passing row leaves one deferred entry in LDS
// (deferred_entry) and sweep_deferred_exact, behind the loop, takes the entries one per lane.  The loop reads the f32 half of QueryParams alone.
// n_def: the wave's deferred entries (wave-uniform).  false: an idle workgroup, which leaves.

// A deferred entry: the row's place in its chunk and its qcDist, which is all the exact path needs - the sum, the correction word and the
// tile's additive bound are read again there.
constexpr int kDeferredRowShift = 16;
template <int W> constexpr bool deferred_entry_fits() {
  // qcDist of a 1-bit row against a 4-plane query is at most 15 per set bit, 128 bits per 16-byte chunk; a chunk has kChunkRows rows
  return 15 * 128 * W < (1 << kDeferredRowShift) && kChunkRows <= (1 << (32 - kDeferredRowShift));
}
__device__ __forceinline__ uint32_t deferred_entry(uint32_t row_in_chunk, uint32_t qc) { return (row_in_chunk << kDeferredRowShift) | qc; }
// Entry i of wave `wave` of NW: batch-major - the waves' i-th batches of 64 lie side by side - so that the entries of batch b of ALL waves lie
// below those of batch b + 1 (the in-place layout of sweep_deferred_exact depends on it).  One wave: i.
// Where the list lies (deferred_list_bytes is the launch's side of it): in the upper half of s_ent where s_ent holds a whole chunk's candidates -
// the flood tier, the append mode - and behind the count words everywhere else.
__host__ __device__ constexpr size_t deferred_list_bytes(bool stages_whole_chunk) { return stages_whole_chunk ? 0 : (size_t)kChunkRows * 4; }
__device__ __forceinline__ uint32_t *deferred_list(uint64_t *s_ent, uint32_t *s_cnt, uint32_t stage_cap) {
  return stage_cap == (uint32_t)kChunkRows ? reinterpret_cast<uint32_t *>(s_ent) + kChunkRows : s_cnt + 4;
}
template <int NW> __device__ __forceinline__ uint32_t deferred_pos(uint32_t i, int wave) {
  return (i >> 6) * (uint32_t)(NW * 64) + (uint32_t)wave * 64u + (i & 63u);
}
// the f32 half of QueryParams: what the tile loop reads of the query
struct FastBoundParams {
  float ayf, lyf, c1f, k2mf, tinyf, csf, caf;
};

// ---- the tile loop's loads: buffer loads through descriptors built on the scalar unit.  With 64-bit vector addresses every tile paid five or
// six vector instructions for the next tile's addresses (the lane's 64-bit pointer rebuilt, its carry beyond the 4 KB of the instruction's
// offset, the correction word's and the row sums' offsets) and held three address pairs in vector registers across the loop.  Here a lane's
// part of an address is one 32-bit offset computed once per wave (16 and 4 bytes per lane for codes and correction word, 4 per pair of lanes for the row sums), a tile's base is the
// descriptor's - rebased per tile with scalar arithmetic, so that no offset grows with the index - the chunk's offset is the instruction's
// 12 bits and, beyond them, a multiple of 4 KB in a scalar register.  The descriptor's size is the tile's (the wave's tiles' add_range); every access
// is in range by construction, as the 64-bit form's were - the size is no second line of defence for the part in the scalar offset.  STREAM: the streamed arm's cache policy (`nt`, what
// __builtin_nontemporal_load gives the 64-bit form).  The compiler counts these loads in vmcnt like any other.
constexpr int kBufferWord3 = 0x00020000;  // a raw buffer of dwords
constexpr int kBufferImmBits = 12;        // the instruction's own offset
template <class T> __device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_buffer(const T *base, int bytes) {  // both wave-uniform
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(base), 0, bytes, kBufferWord3);
}
template <bool STREAM> __device__ __forceinline__ u32x4 buffer_load16(__amdgpu_buffer_rsrc_t r, uint32_t lane_off, int off, int soff = 0) {
  constexpr int imm = (1 << kBufferImmBits) - 1;
  return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)(lane_off + (uint32_t)(off & imm)), (off & ~imm) + soff, STREAM ? 2 : 0));
}
template <bool STREAM> __device__ __forceinline__ uint32_t buffer_load4(__amdgpu_buffer_rsrc_t r, uint32_t lane_off, int off, int soff = 0) {
  constexpr int imm = (1 << kBufferImmBits) - 1;
  return __builtin_amdgcn_raw_buffer_load_b32(r, (int)(lane_off + (uint32_t)(off & imm)), (off & ~imm) + soff, STREAM ? 2 : 0);
}
// a lane's offsets into its tile, computed once per wave
struct LaneOffsets {
  uint32_t code;  // its 16 bytes of a chunk
  uint32_t word;  // its correction word
  uint32_t sum;   // the aligned pair of row sums its own lies in
};
// the wave's TPW tiles' entries of the two side arrays.  The row sums: a scalar base, which a load takes with the lane's 32-bit offset and a
// constant (two scalar registers where a descriptor takes four).  The additive bounds: a descriptor, read without any vector offset - as a
// scalar base the compiler kept it in a pair of vector registers and read it back into scalar ones, two instructions, for every tile.
struct WaveSides {
  const char *sums;             // row_sums of the wave's first tile
  __amdgpu_buffer_rsrc_t adds;  // add_range of the wave's tiles
  int add_at;                   // tile_add_bound's choice, in bytes
};
template <int W, bool STREAM>
__device__ __forceinline__ void buffer_load_codes(__amdgpu_buffer_rsrc_t tile, const LaneOffsets &lo, u32x4 (&c)[W]) {
#pragma unroll
  for (int j = 0; j < W; ++j) c[j] = buffer_load16<STREAM>(tile, lo.code, j * (kTileRows * kChunkBytes));
}
// Called once per tile in front of its loads: the lane's offsets pass through an empty asm, in place.  Seen as ONE value across the unrolled
// tiles, offset + 1024, + 2048 and + 3072 were formed once in front of the loop and held in three more vector registers, in another block than
// the loads, where they no longer fold into the instruction's offset.
// (An empty asm on a value, as bbq_mfma_kernels.hip has them: no instruction, but it pins what THIS build's compiler does with the value - to
// check again, scripts/scan_resources.py: the twins' registers, and its count of v_pk_* in them.)
__device__ __forceinline__ void per_tile(LaneOffsets &lo) { asm("" : "+v"(lo.code), "+v"(lo.word), "+v"(lo.sum)); }
// tile t's three small words: the correction word, the row's sum, the additive bound (default policy in both arms, as it always was).
// The sum as the aligned PAIR of 16-bit entries the lane's own lies in, a 32-bit load, its half picked behind the popcounts (load_tile's
// rule, bbq_kernel_common.h): loaded as 16 bits, the compiler widened the value at the head of the next block - an instruction in front of
// the tile's first popcount that waited for all of the tile's loads but the last.
template <int W, bool STREAM, bool ADD = true>
__device__ __forceinline__ void buffer_load_words(__amdgpu_buffer_rsrc_t tile, const WaveSides &ws, const LaneOffsets &lo, int t,
                                                  uint32_t &cw, uint32_t &ones, float &aadd) {
  cw = buffer_load4<STREAM>(tile, lo.word, (int)tile_corr_offset(W));
  // (without stream_ptr's other address: the arm's fences alone keep the two arms' loads apart - both forms are in the machine code - and
  // a second base was two more scalar registers, which the loop does not have)
  const uint32_t *__restrict__ rs = reinterpret_cast<const uint32_t *>(ws.sums + lo.sum + t * (kTileRows * 2));
  if constexpr (STREAM) ones = BBQ_STREAM_LOAD(rs);
  else ones = *rs;
  // (the folded bound has the additive bounds of all the wave's tiles from one load in front of the loop)
  if constexpr (ADD) aadd = __builtin_bit_cast(float, buffer_load4<false>(ws.adds, 0u, t * 8, ws.add_at));
}

// tile_digit_dot for the tile loop: the same three chains, the same integer.  The first chain starts at -k (u32 arithmetic: the same sum
// modulo 2^32, and qcDist is below 2^32) instead of 0, so that digit_dot's subtraction is the accumulator's initial move; the row's sum is
// added by the caller.  12 chunks: tile_digit_dot's compiler barrier behind each chunk does not order the chunks' arithmetic, and the
// scheduler, given the codes of a whole tile at once, formed the selections of two and three chunks ahead of their popcounts - 92 vector
// registers in the 2-tile kernel; a scheduling barrier keeps each chunk's work together (this build's scheduler: scripts/scan_resources.py).
template <int W>
__device__ __forceinline__ uint32_t tile_digit_sums(const u32x4 (&c)[W], const u32x4 *__restrict__ s_digits, uint32_t k) {
  uint32_t a0 = 0u - k, a1 = 0, a2 = 0;
#pragma unroll
  for (int j = 0; j < W; ++j) {
    const u32x4 *__restrict__ m = s_digits + j * kDigitMasks;
    a0 = popc4_acc(digit_select(c[j], m[0], m[1]), a0);
    a1 = popc4_acc(digit_select(c[j], m[2], m[3]), a1);
    a2 = popc4_acc(c[j] & m[4], a2);
    if constexpr (W >= 12) {
      BBQ_BRANCH_FENCE();
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  return a0 + 3u * a1 + 9u * a2;
}

// fast_bound_passes for the tile loop: the same operations in the same order on the same values - the same verdict for every row - but
// (1) against a threshold image that is NaN for a query without f32 images, so that such a query passes every row without a branch around
// the bound, (2) without the validity, which the loop applies to the ballot on the scalar unit, and (3) with two values passed through an
// empty asm: left alone, the compiler packs the bound's pairs of like operations into v_pk_*_f32 - half rate on this device - and pays four
// moves per row to line their operands up.  (Which pairs it packs is this build's choice: scripts/scan_resources.py counts the v_pk_* left in
// the twins, 0 with these two.)
__device__ __forceinline__ float keep_unpacked(float x) {
  asm("" : "+v"(x));
  return x;
}
__device__ __forceinline__ bool tile_bound_passes(uint32_t qc, uint32_t cw, float aadd, uint32_t ones, const FastBoundParams &p, float tinyf, float thz) {
  const float al = compact_lower(cw), au = compact_upper(cw);
  const float g = fmaf(p.lyf, (float)qc, p.ayf * (float)ones);
  const float A = p.c1f - g;
  const float pa = keep_unpacked(al * A), pb = au * g;
  const float s = pa + pb;
  const float e = fabsf(pa) + fabsf(pb);
  const float w = fabsf(al) + fabsf(au);
  const float slack = fmaf(kFastK1, e, fmaf(w, p.k2mf, tinyf));
  const float zc = keep_unpacked(fmaf(p.csf, s, p.caf * aadd));
  const float zs = fmaf(p.csf, slack, kFastAddRel * fabsf(aadd));
  const float z0 = zc + zs;
  const float zup = fmaf(kFastAddRel, fabsf(z0), z0);
  return !(zup <= thz);  // NaN anywhere passes -> exact path
}

// ---- the bound, folded (kFoldedBound; the tile loop's other form, tile_bound_passes, stays for the comparison of the two).
// The same inequality as fast_bound_passes, split into a per-row side and a per-tile threshold:
//     row side   r = s + K1 e + k2m w            s = al (c1 - g) + au g,  e = |al (c1 - g)| + |au g|,  w = |al| + |au|
//     tile side  T = ((zth - ca aadd) - pad) / cs,   pad = 2^-21 |aadd| + 2^-21 |zth - ca aadd| + cs tiny
// and the row passes unless r <= T.  g comes from the three digit counts and the row's sum without forming qcDist:
//     g = ly D + b sum,   D = a0 + 3 a1 + 9 a2 - K (an integer, exact in f32: |D| < 2^24),   b = 4 ly + ay,
// which is ay sum + ly qc because qc = D + 4 sum (digit_dot).  qcDist itself is formed inside the rare passing branch, for the deferred entry.
// T is computed ONCE per wave for all its tiles, lane t for tile t (the wave's add_range entries are one load), and read per tile with
// v_readlane into a scalar register: the row's compare reads it from there.  Per row the fold takes out the two products with aadd, two FMAs,
// the z-space sum, the final inflation and one integer addition.
// Error budget, on top of the one above fast_bound_passes (u = 2^-24; M, W, E as there; the twins sweep 1-bit rows with a 4-plane query,
// so qcmax = 15 x1max):
//  * g.  |ly D| <= |ly| (qcmax + 4 x1max) = 1.27 |ly| qcmax and |b sum| <= (4 |ly| + |ay|) x1max.  lyf is within u of ly, the computed
//    b = fl(4 lyf + ayf) within 2 u (4 |ly| + |ay|) of b, D and sum are exact as floats, the product b sum and the FMA round once each
//    (u |b sum|, u |g| <= u M / 2): with x = 2 |ly| qcmax, y = 2 |ay| x1max, x + y <= M, the computed g is within
//    u (1.04 x + 1.5 y + 0.5 M) <= 2.0 u M of g - inside the 2.1 u M the budget above gives g, so |s_f32 - s| <= 9.1 u W M stands.
//  * the row side.  K1 e + k2m w is computed with the same two roundings as before (a product and an FMA where there were two FMAs: the
//    2^-18 in K1 pays them); r = fl(s + slack) adds one rounding, u |r| <= u (1.01 W M + slack): 1.02 u W M of the 6.8 u W M that
//    2^-20 = 16 u leaves above the 9.2 u needed, and u slack of the 2^-18.
//  * the tile side.  ca aadd is exact (ca = +-1), the division by cs exact (cs = 1 or 2); num = fl(zth - ca aadd), pad and fl(num - pad)
//    round five times, each by at most u of a magnitude <= |num| (1 + 2^-20) + pad: 2^-21 |num| = 8 u |num| pays them, 2^-21 |aadd| pays the
//    2^-23 |aadd| that add_range's rounding to nearest needs, cs tiny the absolute parts (tiny is scaled by cs on the row side of
//    fast_bound_passes as well) and what leaves the normal range here (at most 2^-126 per operation, tiny >= 2^-100).
//  * zth is already the conservative image (z_threshold_f32 rounds down), so T <= the true (zth - ca aadd - 2^-23 |aadd| - cs tiny) / cs
//    and  r <= T  implies  cs (s + allowance) + ca aadd + ... <= zth: the row's exact score cannot beat the threshold.
//  * NaN and overflow pass.  s = +-inf needs an infinite product or sum, then e = +inf (e >= |s| before rounding), slack = +inf and r is
//    +inf or NaN: never -inf, so r <= T is false.  zth = -inf gives num = -inf, pad = +inf, T = -inf: every row passes.  A NaN zth (a query
//    without f32 images) or an infinite or NaN aadd gives T = -inf or NaN: every row passes.
//  tests/test_bound_folded_cpu.py restates both sides in numpy f32, fused and unfused, and checks dominance over the exact score.
constexpr bool kFoldedBound = true;
struct FoldedBoundParams {
  float lyf, bf, c1f, k2mf;  // b = 4 ly + ay from the images
};
__device__ __forceinline__ float tile_threshold(float aadd, const FastBoundParams &p, float thz) {
  const float num = thz - p.caf * aadd;
  const float pad = fmaf(kFastAddRel, fabsf(aadd), fmaf(kFastAddRel, fabsf(num), p.csf * p.tinyf));
  return (num - pad) * (p.csf == 2.0f ? 0.5f : 1.0f);  // 1 / cs, exact: cs is 1 or 2 (QueryParams::csf)
}
__device__ __forceinline__ bool folded_bound_passes(uint32_t d, uint32_t cw, uint32_t sum, const FoldedBoundParams &p, float tile_th) {
  const float al = compact_lower(cw), au = compact_upper(cw);
  const float g = fmaf(p.lyf, (float)(int32_t)d, p.bf * (float)sum);
  const float A = p.c1f - g;
  const float pa = keep_unpacked(al * A), pb = au * g;
  const float s = pa + pb;
  const float e = fabsf(pa) + fabsf(pb);
  const float w = fabsf(al) + fabsf(au);
  const float slack = fmaf(kFastK1, e, w * p.k2mf);
  const float r = s + slack;
  return !(r <= tile_th);  // NaN anywhere passes -> exact path
}

template <int W, int TPW, int NT>
__device__ __forceinline__ bool sweep_wave_tiles(const ScanArgs &a, const SweepCoord wg, const bool idle, const int q, u32x4 *s_planes, uint32_t *s_def,
                                                 uint32_t *s_cnt, uint32_t &n_def) {
  constexpr int QU = kDigitMasks;
  constexpr int NW = NT / 64;
  static_assert(W * QU <= NT, "one staging pass: every unit of the query has a thread");
  static_assert(deferred_entry_fits<W>(), "a deferred entry holds the row in its chunk and qcDist in 32 bits");
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const u32x4 *__restrict__ gp = reinterpret_cast<const u32x4 *>(a.qplanes) + (size_t)a.qdigits_at + (size_t)q * W * QU;
  const QueryParams *__restrict__ qp = a.qparams + q;
  const FastBoundParams p = {qp->ayf, qp->lyf, qp->c1f, qp->k2mf, qp->tinyf, qp->csf, qp->caf};
  const int32_t sim = qp->sim, fast_bound = qp->fast_bound;
  const uint32_t digit_k = qp->digit_k;
  const Threshold th = a.theta[q];
  // a query without f32 images defers every valid row - its f64 bound stands in front of the exact path, behind the loop: no row fails a NaN
  const float thz = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, fast_bound ? threshold_z(th) : __builtin_nanf(""))));
  // (tinyf is the addend of an FMA whose other factor is a scalar as well, and an instruction reads one scalar register: kept in a vector
  // register for the wave, or every tile pays the move.  Through a vector load of its own - a lane offset the compiler cannot see through:
  // copied out of the scalar load that brings the images, it took all eight of them into vector registers.  This build's compiler again:
  // scripts/scan_resources.py shows it as +8 registers in every twin)
  float tinyv = 0.0f;
  if constexpr (!kFoldedBound) {
    uint32_t lane_zero = 0;
    asm("" : "+v"(lane_zero));
    tinyv = *reinterpret_cast<const float *>(reinterpret_cast<const char *>(&qp->tinyf) + lane_zero);
  }
  // the folded bound's per-row constants (b = 4 ly + ay: uniform, kept in a scalar register)
  const FoldedBoundParams pf = {p.lyf, __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, fmaf(4.0f, p.lyf, p.ayf)))), p.c1f, p.k2mf};
  n_def = 0;
  const int64_t chunk = a.chunk_begin + wg.chunk_local;
  const int64_t n_tiles = (a.idx.n_rows + kTileRows - 1) / kTileRows;
  const int64_t tile0 = chunk * kTilesPerChunk + wave_first_tile(TPW, wave);
  const bool has_tile = !idle && tile0 < n_tiles;  // wave-uniform, decided on the scalar unit
  const bool resident = chunk_is_resident(chunk, a.idx);
  const int tile_stride = a.idx.geom.tile_stride;
  // what the wave has of the index: its tiles and its rows (both wave-uniform, 0 without a tile)
  const int64_t tiles_left = n_tiles - tile0, rows_left = a.idx.n_rows - tile0 * kTileRows;
  const int my_tiles = !has_tile ? 0 : tiles_left < TPW ? (int)tiles_left : TPW;
  const int my_rows = !has_tile ? 0 : rows_left < TPW * kTileRows ? (int)rows_left : TPW * kTileRows;
  // the wave's first tile, and the TPW tiles' entries of the two side arrays
  const uint8_t *__restrict__ tp = a.idx.tiles + tile0 * tile_stride;
  const WaveSides ws = {reinterpret_cast<const char *>(a.idx.row_sums + tile0 * kTileRows), tile_buffer(a.idx.add_range + tile0 * 2, my_tiles * 8), sim == 0 ? 0 : 4};
  LaneOffsets lo = {(uint32_t)lane << 4, (uint32_t)lane << 2, (uint32_t)(lane >> 1) << 2};
  u32x4 c[W];
  uint32_t cw, ones;
  float aadd;
  if (has_tile) {
    u32x4 staged;
    // (load_tile's shape: both arms of one scalar branch, the masks the oldest load in flight of whichever is taken, the streamed one fenced)
    const __amdgpu_buffer_rsrc_t tb = tile_buffer(tp, tile_stride);
    if (resident) {
      if (tid < W * QU) staged = gp[tid];
      buffer_load_codes<W, false>(tb, lo, c);
      buffer_load_words<W, false, !kFoldedBound>(tb, ws, lo, 0, cw, ones, aadd);
    } else {
      BBQ_BRANCH_FENCE();
      if (tid < W * QU) staged = gp[tid];
      buffer_load_codes<W, true>(tb, lo, c);
      buffer_load_words<W, true, !kFoldedBound>(tb, ws, lo, 0, cw, ones, aadd);
      BBQ_BRANCH_FENCE();
    }
    // the folded bound: lane t takes tile t's additive bound (the wave's last tile's in the lanes beyond: in range, never used), the
    // youngest load of tile 0 - the popcounts' countdown does not wait for it
    if constexpr (kFoldedBound) {
      const int t_lane = lane < my_tiles ? lane : my_tiles - 1;
      aadd = __builtin_bit_cast(float, buffer_load4<false>(ws.adds, (uint32_t)t_lane * 8u, 0, ws.add_at));
    }
    if (tid < W * QU) s_planes[tid] = staged;
    asm volatile("; staged with the first tile's loads in flight" ::: "memory");
  } else {
    u32x4 staged;
    if (tid < W * QU) staged = gp[tid];
    if (tid < W * QU) s_planes[tid] = staged;
    asm volatile("; staged without a tile" ::: "memory");
  }
  if (tid == 0) {
    s_cnt[0] = 0;
    if constexpr (NW > 1) s_cnt[1] = 0;  // the longest deferred list of the workgroup's waves (sweep_deferred_exact)
  }
  if (idle) return false;
  __syncthreads();  // LDS only: a wave that staged nothing passes it with its tile's loads in flight
  if (!has_tile) return true;

  const uint32_t pick_at = (uint32_t)(lane & 1) << 4;  // the lane's half of its pair of row sums
  const uint32_t row_in_chunk0 = (uint32_t)(wave_first_tile(TPW, wave) * kTileRows);  // (scalar: the lane is added where a row is deferred)
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    uint32_t qc = tile_digit_sums<W>(c, s_planes, digit_k);
    __builtin_amdgcn_sched_barrier(0);  // (the bound and the loads below stay behind the popcounts, as the pick of the sum does in the TPW = 1 kernel)
    // The bound's verdicts as a mask in a scalar pair, straight from its compare; the rows beyond the index - in the index's last tile alone -
    // are taken out of it there.  (1 <= rows_here: the tile exists.)
    auto verdicts = [&]() {
      const uint32_t sum = __builtin_amdgcn_ubfe(ones, pick_at, 16u);  // the lane's half of the pair
      bool pass;
      if constexpr (kFoldedBound) {
        // (the wave's thresholds once, behind the first tile's popcounts: lane t has tile t's; aadd becomes the thresholds' register)
        if (t == 0) aadd = tile_threshold(aadd, p, thz);
        const float tile_th = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, aadd), t));
        pass = folded_bound_passes(qc, cw, sum, pf, tile_th);
      }
      if constexpr (!kFoldedBound) {
        qc += sum << 2;  // digit_dot's 4 * ones: u32 arithmetic, the same integer in either order
        pass = tile_bound_passes(qc, cw, aadd, sum, p, tinyv, thz);
      }
      unsigned long long passing = __builtin_amdgcn_ballot_w64(pass);
      const int rows_here = my_rows - t * kTileRows;
      if (rows_here < kTileRows) passing &= (1ull << rows_here) - 1ull;
      return passing;
    };
    // The entry's place: the wave's running count plus the passing lanes below this one.  No atomic, and where nobody passes - nearly every
    // tile - a scalar branch over all of it.
    auto defer = [&](const unsigned long long passing) {
      if (passing) {
        // (the folded bound never formed qcDist: a deferred row's, here, from this tile's pair of row sums)
        if constexpr (kFoldedBound) qc += __builtin_amdgcn_ubfe(ones, pick_at, 16u) << 2;
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(passing >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)passing, 0u));
        if (__builtin_amdgcn_inverse_ballot_w64(passing)) s_def[deferred_pos<NW>(n_def + below, wave)] = deferred_entry(row_in_chunk0 + (uint32_t)(t * kTileRows) + __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)), qc);
        n_def += (uint32_t)__popcll(passing);
      }
    };
    const unsigned long long passing = verdicts();
    if constexpr (kFoldedBound) defer(passing);  // in front of the next tile's loads: it reads this tile's row sums once more
    // The next tile's loads BEHIND the bound, which was this tile's last use of the registers the three small words land in - issued in front
    // of it, with the codes behind the popcounts, they came back in registers of their own, and the copies stood behind a wait for the whole
    // tile in front of the next one's loads.  All nine under ONE scalar branch on the cache policy, as load_tile has them: with the words
    // under a branch of their own, the compiler's count where the arms join made the popcounts wait for the words behind the codes.
    if (t + 1 < TPW && t + 1 < my_tiles) {
      per_tile(lo);
      const __amdgpu_buffer_rsrc_t tb = tile_buffer(tp + (int64_t)(t + 1) * tile_stride, tile_stride);
      if (resident) {
        buffer_load_codes<W, false>(tb, lo, c);
        buffer_load_words<W, false, !kFoldedBound>(tb, ws, lo, t + 1, cw, ones, aadd);
      } else {
        BBQ_BRANCH_FENCE();
        buffer_load_codes<W, true>(tb, lo, c);
        buffer_load_words<W, true, !kFoldedBound>(tb, ws, lo, t + 1, cw, ones, aadd);
        BBQ_BRANCH_FENCE();
      }
      if constexpr (!kFoldedBound) defer(passing);
    } else {  // (the wave's last tile: an arm of its own - as the negation of the condition above, a condition that lives across blocks, the
      if constexpr (!kFoldedBound) defer(passing);  // way out went through a v_cndmask / v_cmp pair per tile)
      break;
    }
  }
  return true;
}

// The exact path of a chunk's deferred rows, once per chunk behind the tile loop: a rolled loop over batches of 64 entries, one entry per lane.
// A row of a query without f32 images passes its f64 bound first (the row's correction word and its tile's additive bound are read again);
// then the exact corrections, the f64 score, the NaN vote, the key test and the candidate, as the one-tile kernel has them.  The f64 half of
// QueryParams is loaded HERE, behind the tile loop's last barrier-free stretch, so that it is live in no tile.
// In place (the flood tier and the append mode, where s_ent holds kChunkRows candidates and LDS must not grow: 32 workgroups of one wave share
// a CU's 160 KB): the deferred list is the upper half of s_ent, 4-byte entries, and the candidates grow from the bottom as entries are
// consumed.  Every batch, ALL waves read their entries, THEN a barrier, then candidates are written: after the batches 0 .. b, m <= 64 NW (b + 1)
// entries are consumed and at most m candidates lie in [0, 8 m) bytes, while the unread batches start at 4 kChunkRows + 4 * 64 NW (b + 1) -
// never below 8 m for 64 NW (b + 1) <= kChunkRows - and a wave that is already writing batch b + 1 has passed that batch's barrier, so all of
// batch b + 1 is read.  Elsewhere (s_ent holds `cap` candidates) the list has 4 kChunkRows bytes of its own behind the count words.
template <int W, int TPW, int NT>
__device__ __forceinline__ void sweep_deferred_exact(const ScanArgs &a, const SweepCoord wg, const int q, const uint32_t *s_def, uint64_t *s_ent,
                                                     uint32_t *s_cnt, const uint32_t stage_cap, const uint32_t n_def, bool &nan_seen) {
  constexpr int NW = NT / 64;
  static_assert(NW * TPW * 64 == kChunkRows, "the workgroup's waves cover the chunk: at most kChunkRows deferred entries, batch b of all waves below batch b + 1");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t n_max = n_def;  // workgroup-uniform: the batches every wave takes part in
  if constexpr (NW > 1) {
    if (lane == 0 && n_def != 0) atomicMax(s_cnt + 1, n_def);
    __syncthreads();
    n_max = __builtin_amdgcn_readfirstlane(s_cnt[1]);
  }
  if (n_max == 0) return;
  const QueryParams p = a.qparams[q];
  const uint32_t theta = a.theta[q].key;
  const int64_t chunk_row0 = (a.chunk_begin + wg.chunk_local) * (int64_t)kChunkRows;
  for (uint32_t base = 0; base < n_max; base += 64) {
    const uint32_t i = base + lane;
    const bool have = i < n_def;
    uint32_t e = 0;
    if (have) e = s_def[deferred_pos<NW>(i, wave)];
    __syncthreads();  // every lane of the workgroup has read its entry of this batch: candidates may take their place
    if (have) {
      const uint32_t qc = e & ((1u << kDeferredRowShift) - 1u);
      const int64_t row = chunk_row0 + (e >> kDeferredRowShift);
      const uint32_t sum = a.idx.row_sums[row];
      bool need_exact = true;
      if (!p.fast_bound) {
        const int64_t tile = row / kTileRows;
        const uint32_t cw = *(reinterpret_cast<const uint32_t *>(a.idx.tiles + tile * (int64_t)a.idx.geom.tile_stride + tile_corr_offset(W)) + (row & (kTileRows - 1)));
        need_exact = f64_bound_passes(true, qc, cw, tile_add_bound(a.idx, tile, p.sim), (double)sum, p, theta);
      }
      if (need_exact) {
        f64x2 lu;
        double xadd;
        exact_corrections(a.idx.exact, row, lu, xadd);
        const double s64 = score_f64((double)qc, lu.x, lu.y, xadd, (double)sum, p);
        const float s32 = (float)s64;
        if (s32 != s32) nan_seen = true;
        if ((s32 == s32) && key_of_bits(__float_as_uint(s32)) > theta) {
          const uint32_t slot = atomicAdd(s_cnt, 1u);
          if (slot < stage_cap) s_ent[slot] = candidate_entry(a.row_id_base + row, s32);
        }
      }
    }
  }
}

// MODE: 0 sparse / inline corrections, 1 dense / inline, 2 sparse / compact corrections + exact gather, 3 dense / compact
// grid = (chunks of kChunkRows rows, queries), or with ScanArgs::l2_shift = s > 0 the same pairs in the order that runs a chunk's 2^s
// queries back to back on one XCD (sweep_coord, bbq_device.h); block = kChunkRows/64 waves: wave w handles tile w of its chunk (one
// row per lane)
// SB = bits per stored field: 1 = packed 1-bit rows (QB bit-planes of the query), 2 / 4 / 8 = multi-bit rows (QB = 4: query values
// <= 15, QB = 8: any)
// Accept: empty - the unfiltered sweep, exactly the kernel it was - or one `const uint64_t *`, the accept bitset of a filtered search
// (FILT; sparse modes only).  accept[tile] is the tile's accept word (bit l = lane l's row, bbq_filter.cpp): the wave reads it once
// through a wave-uniform address; a wave whose word is 0 issues no load of its tile at all, and a lane whose bit is clear is not a
// valid row - it gathers no exact corrections, lists nothing and raises no NaN flag.  The end of the chunk (count word, flood tier,
// append path) is the same for both.  (One kernel template and a parameter pack rather than a shared __device__ body under two
// kernels: inlined through a function the unfiltered instantiations came out with other instruction schedules.)
// RS (MODE 2 only, chosen by the launch iff its view carries IndexView::row_sums): the row's popcount / code sum is not counted here - it is
// the same for every query, segment and call - but loaded from the side array with the tile's other loads; the popcount loop and the
// multi-bit dot run without their sum chain.  The value is what that chain returns, so the bound and the score are the same bits.
// DG (RS, 1-bit rows and a 4-plane query only, chosen by the launch iff ScanArgs::qdigits_at is set as well): the digit form - the workgroup
// stages the query's kDigitMasks ternary digit masks per chunk instead of its four bit-planes, and qcDist comes out of three popcount
// chains and the row's sum (tile_digit_dot).  The same integer, so everything behind it is the same bits.
// TPW (the unfiltered DG twins of tiles_twin alone, chosen by the launch from its tiles_per_wave): tiles per wave - the workgroup has
// kTilesPerChunk / TPW waves and wave w sweeps TPW consecutive tiles of the chunk (sweep_wave_tiles, above).  1: one tile per wave, the kernel as it was.
template <int QB, int W, int MODE, int SB = 1, bool RS = false, bool DG = false, int TPW = 1, class... Accept>
__global__ __launch_bounds__(kChunkRows / TPW) void bbq_scan_kernel(const ScanArgs a, const Accept... accept_arg) {
  constexpr bool FILT = sizeof...(Accept) > 0;
  static_assert(wave_tiles_are_exact(TPW) && (TPW == 1 || (DG && !FILT && MODE == 2 && W > 0)), "several tiles per wave: the unfiltered digit form of a compile-time width");
  static_assert(sizeof...(Accept) <= 1 && !(FILT && (MODE & 1)), "at most the accept bitset, and a filtered sweep is sparse");
  static_assert(!RS || (MODE & 3) == 2, "row sums are read by the sparse sweep of the compact layout alone");
  static_assert(!DG || (RS && SB == 1 && QB == 4), "the digit form: a 4-plane query against 1-bit rows whose popcounts are at hand");
  const uint64_t *__restrict__ accept = nullptr;
  if constexpr (FILT) accept = (accept_arg, ...);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NT = kChunkRows / TPW;  // the workgroup's threads
  constexpr bool DENSE = (MODE & 1) != 0;
  constexpr bool COMPACT = (MODE & 2) != 0;
  constexpr int QU = DG ? kDigitMasks : query_units_per_chunk(QB, SB);  // 16-byte units staged per chunk of a row
  const int w16 = W > 0 ? W : a.idx.geom.w16;
  u32x4 *s_planes = reinterpret_cast<u32x4 *>(smem);
  uint64_t *s_ent = reinterpret_cast<uint64_t *>(smem + (size_t)w16 * QU * 16);
  // with a flood tier every passing row of the chunk is staged (it may have to move to the overflow area as a whole)
  const uint32_t stage_cap = DENSE ? 0u : ((a.ovf || a.append_lists) ? (uint32_t)kChunkRows : (uint32_t)a.cap);
  uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_ent + stage_cap);

  // which chunk for which query: the one map of the launch (sweep_coord); a workgroup of the grid's padding has nothing to do
  const SweepCoord wg = sweep_coord(blockIdx.x, blockIdx.y, a.l2_shift);
  // It leaves in front of the first barrier, not here: with a return in the entry block the compiler of this build (ROCm 7.2) allocated
  // bbq_scan_kernel<8, 0, 0, 4> 68 vector registers instead of 41, one wave of occupancy less.  To check again: build bbq_kernels.hip and
  // bbq_filter_kernels.hip with -Rpass-analysis=kernel-resource-usage before and after moving the return, and compare VGPRs / Occupancy
  // of every bbq_scan_kernel instantiation.  Until then it reads what query 0 would (its accept word only if the tile exists): in bounds, never used
  const bool idle = wg.chunk_local >= a.n_chunks || wg.query >= a.n_queries;  // workgroup-uniform
  const int q = idle ? 0 : wg.query;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;

  // Several tiles per wave: the wave's tiles, the NaN vote and the end of the chunk, then out.  (A block of its own in front of the kernel's
  // body, which stays the text it was: with the body inside an else the one-tile instantiations came out of this build's compiler with
  // other scalar code and, 66 of them, two more vector instructions per wave.  For the same reason the end of the chunk is written out
  // twice, here through sweep_chunk_end: called from the body below, the unfiltered instantiations get other schedules.)
  if constexpr (TPW > 1) {
    bool nan_seen = false;
    uint32_t n_def;
    uint32_t *s_def = deferred_list(s_ent, s_cnt, stage_cap);
    if (!sweep_wave_tiles<W, TPW, NT>(a, wg, idle, q, s_planes, s_def, s_cnt, n_def)) return;
    sweep_deferred_exact<W, TPW, NT>(a, wg, q, s_def, s_ent, s_cnt, stage_cap, n_def, nan_seen);
    if (__any(nan_seen) && lane == 0) atomicOr(a.flags + q, kFlagNaN);
    sweep_chunk_end<NT>(a, wg, q, s_ent, s_cnt);
    return;
  }

  // the tile's accept word first: its address depends on the workgroup's chunk and the wave number alone, so the scalar load travels while the
  // planes are staged and is there when the barrier opens (behind the barrier every wave paid its latency in front of its first HBM request)
  uint64_t aw = 0;
  if constexpr (FILT) {
    const int64_t my_tile = (a.chunk_begin + wg.chunk_local) * kTilesPerChunk + __builtin_amdgcn_readfirstlane(wave);
    if (my_tile < (a.idx.n_rows + kTileRows - 1) / kTileRows) aw = accept[my_tile];
  }
  // EARLY (early_loads, above): the wave's tile loads are issued in front of the staging and the barrier.  Nothing about a tile's address depends
  // on the query, so the two memory round trips a workgroup used to pay one behind the other - the staging wave's masks, then, behind the barrier,
  // every wave's tile - travel together: the query's scalar loads, the masks' load (into registers), the tile's loads, and only then the LDS
  // write and the barrier, which waits for LDS alone.  The other order (run-time width, dense, early_loads' exceptions) stages first, as it always did.
  constexpr bool EARLY = early_loads<FILT, QB, W, MODE, SB, RS, DG>();
  const u32x4 *__restrict__ gp = reinterpret_cast<const u32x4 *>(a.qplanes) + (DG ? (size_t)a.qdigits_at : 0) + (size_t)q * w16 * QU;
  if constexpr (!EARLY) {  // stage the query bit-planes (DG: its digit masks) once per workgroup
    for (int i = tid; i < w16 * QU; i += NT) s_planes[i] = gp[i];
    if (!DENSE && tid == 0) *s_cnt = 0;
  }
  // (the query's uniforms stay in front of the tile's loads in the source: behind load_tile's compiler barriers they became vector loads)
  const QueryParams p = a.qparams[q];
  const Threshold th = DENSE ? Threshold{0u, 0u} : a.theta[q];  // (one 8-byte scalar load: the key and its z image)
  const uint32_t theta = th.key;
  if constexpr (!EARLY) {
    if (idle) return;
    __syncthreads();
  }

  const int64_t chunk = a.chunk_begin + wg.chunk_local;
  const int64_t n_tiles = (a.idx.n_rows + kTileRows - 1) / kTileRows;
  const int64_t tile = chunk * kTilesPerChunk + wave;
  bool nan_seen = false;
  // wave-uniform.  (An idle workgroup of the early order has not left yet, and its chunk may well exist in the index: it loads nothing.)
  // The early order decides it on the scalar unit, from the wave number as a scalar: its two arms below must be the two arms of a scalar
  // branch, each ending in its own wait, and not two masked stretches of one path that the compiler could see skipped both.
  bool has_tile;
  if constexpr (EARLY) has_tile = !idle && chunk * kTilesPerChunk + __builtin_amdgcn_readfirstlane(wave) < n_tiles && (!FILT || aw != 0);
  else has_tile = tile < n_tiles && (!FILT || aw != 0);

  // the tile's registers: in the early order they are loaded in front of the barrier and used behind it
  constexpr int CORR = !COMPACT ? 2 : (DENSE ? 0 : 1);
  f64x2 lu = {0.0, 0.0};
  double xadd = 0.0, x1 = 0.0;
  uint32_t cw;
  float aadd;
  uint32_t qc, ones;
  // (the early order leaves them unset: a wave without a tile never reads them, and set to zero here every wave of the early order paid
  // two dozen moves - the tile's registers with them - in front of its loads, where the compiler put the no-tile path's values)
  if constexpr (!EARLY) { cw = 0; aadd = 0.0f; ones = 0; }
  u32x4 c[W > 0 ? W : 1];
  (void)c;
  if constexpr (EARLY) {
    static_assert(W * QU <= NT, "one staging pass: every unit of the query has a thread");
    // The masks' load and the LDS write stand in BOTH arms of this scalar branch - in the arm with a tile the load at the head of whichever
    // arm load_tile takes - so that the masks are the oldest load in flight on every path and in flight nowhere else.  The loads return in
    // order, so the staging threads wait for the masks and for nothing of the tile (vmcnt = the tile's loads), and the registers the masks
    // came in are known to be free behind the barrier.  Loaded in front of the branch and written behind it, the compiler's count at the
    // join was the no-tile arm's: vmcnt(0), the whole tile, in front of the LDS write and once more behind the barrier, for every wave.
    // (The staging registers are set and read under one condition; initialised, the streamed arm copied and waited for them at once.)
    if (has_tile) {
      u32x4 staged;
      auto load_masks = [&]() { if (tid < W * QU) staged = gp[tid]; };
      const uint8_t *__restrict__ tp = a.idx.tiles + tile * (int64_t)a.idx.geom.tile_stride;
      const int64_t row = tile * kTileRows + lane;
      const bool resident = chunk_is_resident(chunk, a.idx);
      // (the row's sum as the aligned pair of 16-bit entries it lies in - rows and lanes have the same parity, the side array covers whole
      // tiles - and the lane's half picked behind the barrier: loaded as 16 bits, the value was widened here, in an instruction that waited
      // for all but the tile's last load in front of the barrier)
      if constexpr (RS) load_tile<W, CORR, true>(tp, lane, false, resident, a.idx.nt_delta, c, cw, lu, xadd, x1,
                                                 reinterpret_cast<const uint32_t *>(a.idx.row_sums + (row & ~(int64_t)1)), &ones, load_masks);
      else load_tile<W, CORR, false>(tp, lane, a.idx.geom.has_x1 != 0, resident, a.idx.nt_delta, c, cw, lu, xadd, x1, (const uint16_t *)nullptr, nullptr, load_masks);
      // with the tile's loads, not behind the barrier: there it waited for the whole tile first
      if constexpr (COMPACT) aadd = tile_add_bound(a.idx, tile, p.sim);
      if (tid < W * QU) s_planes[tid] = staged;
      asm volatile("; staged with the tile's loads in flight" ::: "memory");  // (the arms do not end alike: no common tail to merge)
    } else {
      u32x4 staged;
      if (tid < W * QU) staged = gp[tid];
      if (tid < W * QU) s_planes[tid] = staged;
      asm volatile("; staged without a tile" ::: "memory");
    }
    if (tid == 0) *s_cnt = 0;
    if (idle) return;
    __syncthreads();  // LDS only: a wave that staged nothing passes it with its tile's loads in flight
  }

  if (has_tile) {
    const uint8_t *__restrict__ tp = a.idx.tiles + tile * (int64_t)a.idx.geom.tile_stride;
    const uint8_t *__restrict__ cr = tp + tile_corr_offset(w16);
    const int64_t row = tile * kTileRows + lane;
    const bool valid = row < a.idx.n_rows && (!FILT || ((aw >> lane) & 1ull) != 0);

    // every load of the tile is issued up front: the row's code chunks and its corrections
    if constexpr (W > 0) {
      if constexpr (!EARLY) {
        const bool resident = chunk_is_resident(chunk, a.idx);
        if constexpr (RS) load_tile<W, CORR, true>(tp, lane, false, resident, a.idx.nt_delta, c, cw, lu, xadd, x1, a.idx.row_sums + row, &ones);
        else load_tile<W, CORR>(tp, lane, a.idx.geom.has_x1 != 0, resident, a.idx.nt_delta, c, cw, lu, xadd, x1);
        if constexpr (COMPACT && DENSE) exact_corrections<true>(a.idx.exact, row, lu, xadd);
        if constexpr (COMPACT && !DENSE) aadd = tile_add_bound(a.idx, tile, p.sim);
      }
      if constexpr (DG) qc = tile_digit_dot<W>(c, s_planes, EARLY ? 0u : ones, p.digit_k);
      else if constexpr (SB == 1) qc = tile_popcounts<QB, W, !RS>(c, s_planes, ones);
      else tile_dot_multibit<QB, W, SB, !RS>(c, s_planes, qc, ones);
      if constexpr (EARLY && RS) {
        // the lane's half of the pair, picked BEHIND the dot product and kept there: the pair is the tile's last load but one, and scheduled
        // in front of the popcounts the pick made them wait for the whole tile instead of counting the chunks down as they arrive
        __builtin_amdgcn_sched_barrier(0);
        ones = __builtin_amdgcn_ubfe(ones, (uint32_t)(lane & 1) << 4, 16u);
        if constexpr (DG) qc += ones << 2;  // digit_dot's 4 * ones: u32 arithmetic, the same integer in either order
      }
    } else {  // a row width without a compiled kernel: streamed chunk by chunk
      if constexpr (!COMPACT) {
        lu = BBQ_STREAM_LOAD(reinterpret_cast<const f64x2 *>(cr) + lane);
        xadd = BBQ_STREAM_LOAD(reinterpret_cast<const double *>(cr + kCorrAddOffset) + lane);
        if (a.idx.geom.has_x1) x1 = BBQ_STREAM_LOAD(reinterpret_cast<const double *>(cr + kCorrSumOffset) + lane);
      } else if constexpr (DENSE) {
        exact_corrections<true>(a.idx.exact, row, lu, xadd);
      } else {
        cw = BBQ_STREAM_LOAD(reinterpret_cast<const uint32_t *>(cr) + lane);
        aadd = tile_add_bound(a.idx, tile, p.sim);
        if constexpr (RS) ones = BBQ_STREAM_LOAD(a.idx.row_sums + row);
      }
      if constexpr (DG) qc = tile_digit_dot_any(tp, lane, w16, s_planes, ones, p.digit_k);
      else if constexpr (SB == 1) qc = tile_popcounts_any<QB, !RS>(tp, lane, w16, s_planes, ones);
      else tile_dot_multibit_any<QB, SB, !RS>(tp, lane, w16, s_planes, qc, ones);
    }
    // quantizedComponentSum of a freshly quantized row is its popcount / component sum (RS: converted where a double is needed, below)
    if constexpr (!RS) if (!a.idx.geom.has_x1) x1 = (double)ones;

    bool need_exact = true;
    if constexpr (COMPACT && !DENSE) {
      // the f32 form of the bound wherever the query allows it - except in the one instantiation (filtered, 2-bit rows of 16 chunks, query
      // values above 15) that it cost a wave of occupancy: 92 -> 98 vector registers with it, whatever its place in the code
      constexpr bool F32_BOUND = !(FILT && SB == 2 && QB == 8 && W == 16);
      if constexpr (RS) {  // the f32 form takes the integer; the sum becomes a double only inside the f64 form and for the exact score
        if constexpr (F32_BOUND) need_exact = p.fast_bound ? fast_bound_passes(valid, qc, cw, aadd, ones, p, th) : f64_bound_passes(valid, qc, cw, aadd, (double)ones, p, theta);
        else need_exact = f64_bound_passes(valid, qc, cw, aadd, (double)ones, p, theta);
      } else if constexpr (F32_BOUND) need_exact = compact_bound_passes(valid, qc, cw, aadd, ones, x1, p, th);
      else need_exact = f64_bound_passes(valid, qc, cw, aadd, x1, p, theta);
      if (need_exact) exact_corrections(a.idx.exact, row, lu, xadd);
    }
    if (need_exact) {
      if constexpr (RS) x1 = (double)ones;
      const double s64 = score_f64((double)qc, lu.x, lu.y, xadd, x1, p);
      const float s32 = (float)s64;
      const uint32_t bits = __float_as_uint(s32);
      if (valid && (s32 != s32)) nan_seen = true;
      if constexpr (DENSE) {
        if (valid) {
          const int64_t o = (int64_t)q * a.dense_stride + (row - a.chunk_begin * kChunkRows);
          if (a.dense_score32) a.dense_score32[o] = s32;
          if (a.dense_qcdist) a.dense_qcdist[o] = (int32_t)qc;
          if (a.dense_score64) a.dense_score64[o] = s64;
        }
      } else if (valid && (s32 == s32) && key_of_bits(bits) > theta) {
        const uint32_t slot = atomicAdd(s_cnt, 1u);
        if (slot < stage_cap) s_ent[slot] = candidate_entry(a.row_id_base + row, s32);
      }
    }
  }
  if (__any(nan_seen) && lane == 0) atomicOr(a.flags + q, kFlagNaN);

  if constexpr (!DENSE) {
    __syncthreads();
    if (a.append_lists) {  // workgroup-uniform
      const uint32_t cnt = *s_cnt;
      if (cnt == 0) return;
      __syncthreads();  // everyone has read *s_cnt: it takes the reserved offset
      append_to_list<NT>(s_ent, cnt, a.append_counts + (size_t)q * kAppendStride, a.append_base[2 * q], a.append_lists + (size_t)q * a.append_cap,
                         a.append_cap, a.flags + q, s_cnt);
      return;
    }
    uint32_t cnt = *s_cnt;
    uint64_t *__restrict__ slot0 = a.entries + ((size_t)q * a.n_chunks + wg.chunk_local) * (size_t)a.cap;
    uint64_t *__restrict__ out = slot0;
    uint32_t count_word = cnt;
    if (cnt > (uint32_t)a.cap) {  // workgroup-uniform
      bool parked = false;
      if (a.ovf) {
        // flood (e.g. rows stored cluster by cluster and this is the query's cluster): one block of the query's overflow
        // area takes the whole chunk, so the list stays row-ordered and the query stays on the sparse path
        __syncthreads();  // everyone has read *s_cnt
        if (tid == 0) *s_cnt = atomicAdd(a.ovf_counts + q, cnt);
        __syncthreads();
        const uint32_t off = *s_cnt;
        if ((uint64_t)off + cnt <= (uint64_t)a.ovf_cap) {
          out = a.ovf + (size_t)q * a.ovf_cap + off;
          count_word = kCountRedirect | cnt;
          if (tid == 0) slot0[0] = off;
          parked = true;
        }
      }
      if (!parked) {
        if (tid == 0) atomicOr(a.flags + q, kFlagOverflow);
        cnt = min(cnt, (uint32_t)a.cap);
        count_word = cnt;
      }
    }
    write_ranked(s_ent, cnt, out, tid, NT);
    if (tid == 0) a.counts[(size_t)q * a.n_chunks + wg.chunk_local] = count_word;
  }
}

// ---------------------------------------------------------------------------------------------------
// dispatch over the instantiations: FILT selects the kernel family, `accept` is its accept bitset (null without)

// The instantiations that keep counting the sum although the launch carries the row sums: their RS twin came out of this build's compiler
// with a wave of occupancy less than they have (docs/dropped.md, "row sums"; F32_BOUND above is the precedent).  To check again: build both
// kernel files with -Rpass-analysis=kernel-resource-usage and compare each RS instantiation's Occupancy with its twin's.
template <bool FILT, int QB, int W, int SB>
constexpr bool row_sums_twin() {
  if (SB == 1 && W == 12 && (QB == 1 || (QB == 8 && FILT))) return false;
  if (SB == 4 && (W == 12 || W == 16) && (QB == 8 || FILT)) return false;
  return true;
}

// The RS instantiations of a 4-plane query against 1-bit rows that have a digit twin (DG): those whose twin keeps at least its occupancy -
// all of them do - AND was measured faster than the plane form on the device (Measurement; docs/dropped.md, "digit planes"):
// 6, 8 and 12 chunks unfiltered, 6 chunks filtered.  One chunk (dim <= 128) gained nothing outside the run-to-run spread; the run-time
// width and the filtered sweeps of 8 and 12 chunks were not measured.
// To check again: as for row_sums_twin, each DG instantiation's Occupancy against its RS twin's, then an A/B of the width on one device.
template <bool FILT, int QB, int W, int SB>
constexpr bool digit_twin() {
  if (SB != 1 || QB != 4 || !row_sums_twin<FILT, QB, W, SB>()) return false;
  return W == 6 || (!FILT && (W == 8 || W == 12));
}

// The DG instantiations that have twins with several tiles per wave (TPW 2, 4 and 8): the unfiltered ones of 6, 8 and 12 chunks.  At all three
// W * kDigitMasks <= 64, so even a workgroup of one wave stages its query in one pass.  The filtered family keeps one tile per wave: its
// has-a-tile test needs an accept word per tile.  Which TPW a launch takes by default is decided per width from measurements, on the host
// (tiles_per_wave_for, bbq_core.cpp).  To check again: scripts/scan_resources.py - each twin without scratch and with no fewer waves per SIMD
// than its TPW = 1 twin - then an A/B of the width on one device.
template <bool FILT, int QB, int W, int SB>
constexpr bool tiles_twin() {
  return !FILT && digit_twin<FILT, QB, W, SB>() && (W == 6 || W == 8 || W == 12);
}
template <int QB, int W, int MODE, int SB, int TPW>
static void launch_tiles_twin(const ScanArgs &a, dim3 grid, size_t smem, hipStream_t s) {
  hipLaunchKernelGGL((bbq_scan_kernel<QB, W, MODE, SB, true, true, TPW>), grid, dim3(kChunkRows / TPW, 1, 1), smem, s, a);
}

// tiles_per_wave: 1, 2, 4 or 8 - a host-side parameter of the launch, not a kernel argument (ScanArgs keeps its size): it selects the TPW twin
// where the launch has one (tiles_twin, and the digit twin's own conditions) and is ignored everywhere else.  Same grid; the block is
// kChunkRows / TPW threads; the same dynamic LDS with the flood tier or in the append mode, and 2 KB more - the twins' deferred list
// (deferred_list_bytes) - without either.
template <bool FILT, int QB, int W, int MODE, int SB = 1>
static hipError_t launch_scan_t(const ScanArgs &args, const uint64_t *accept, int n_queries, int n_chunks, hipStream_t s, int tiles_per_wave = 1) {
  ScanArgs a = args;  // the map's parameters: what the kernel decodes its block index with is what the grid below is built from
  a.n_chunks = n_chunks;
  a.n_queries = n_queries;
  a.l2_shift = (MODE & 1) ? 0 : sweep_shift_for(args.l2_shift, n_queries, n_chunks);  // a dense launch writes every row: nothing to co-schedule for
  const int w16 = W > 0 ? W : a.idx.geom.w16;
  const size_t smem_out = ((MODE & 1) ? 0 : (size_t)((a.ovf || a.append_lists) ? kChunkRows : a.cap) * 8) + 16;
  const size_t smem = (size_t)w16 * query_units_per_chunk(QB, SB) * 16 + smem_out;
  dim3 grid(sweep_grid_x(n_chunks, a.l2_shift), sweep_grid_y(n_queries, a.l2_shift), 1), block(kChunkRows, 1, 1);
  if constexpr ((MODE & 3) == 2 && digit_twin<FILT, QB, W, SB>()) {
    if (a.idx.row_sums && a.qdigits_at > 0) {  // ... and the caller staged the digit masks: three planes instead of four
      const size_t smem_dg = (size_t)w16 * kDigitMasks * 16 + smem_out;
      if constexpr (tiles_twin<FILT, QB, W, SB>()) {
        // (a cap of kChunkRows without either is the whole chunk as well: deferred_list tests the staged entries, as here)
        const size_t smem_tw = smem_dg + deferred_list_bytes(a.ovf || a.append_lists || a.cap == kChunkRows);
        switch (tiles_per_wave) {
          case 2: launch_tiles_twin<QB, W, MODE, SB, 2>(a, grid, smem_tw, s); return hipGetLastError();
          case 4: launch_tiles_twin<QB, W, MODE, SB, 4>(a, grid, smem_tw, s); return hipGetLastError();
          case 8: launch_tiles_twin<QB, W, MODE, SB, 8>(a, grid, smem_tw, s); return hipGetLastError();
          default: break;
        }
      }
      if constexpr (FILT) hipLaunchKernelGGL((bbq_scan_kernel<QB, W, MODE, SB, true, true, 1, const uint64_t *>), grid, block, smem_dg, s, a, accept);
      else hipLaunchKernelGGL((bbq_scan_kernel<QB, W, MODE, SB, true, true>), grid, block, smem_dg, s, a);
      return hipGetLastError();
    }
  }
  if constexpr ((MODE & 3) == 2 && row_sums_twin<FILT, QB, W, SB>()) {
    if (a.idx.row_sums) {  // the launch's view carries the row sums: the sweep that reads them
      if constexpr (FILT) hipLaunchKernelGGL((bbq_scan_kernel<QB, W, MODE, SB, true, false, 1, const uint64_t *>), grid, block, smem, s, a, accept);
      else hipLaunchKernelGGL((bbq_scan_kernel<QB, W, MODE, SB, true>), grid, block, smem, s, a);
      return hipGetLastError();
    }
  }
  if constexpr (FILT) hipLaunchKernelGGL((bbq_scan_kernel<QB, W, MODE, SB, false, false, 1, const uint64_t *>), grid, block, smem, s, a, accept);
  else hipLaunchKernelGGL((bbq_scan_kernel<QB, W, MODE, SB>), grid, block, smem, s, a);
  return hipGetLastError();
}

// multi-bit rows: compile-time widths for 768-d / 1024-d at 2 bits (12 / 16 chunks; 16 is also 512-d at 4 bits), runtime loop otherwise
template <bool FILT, int QB, int MODE, int SB>
static hipError_t launch_scan_mb_w(const ScanArgs &a, const uint64_t *accept, int nq, int nc, hipStream_t s) {
  switch (a.idx.geom.w16) {
    case 12: return launch_scan_t<FILT, QB, 12, MODE, SB>(a, accept, nq, nc, s);
    case 16: return launch_scan_t<FILT, QB, 16, MODE, SB>(a, accept, nq, nc, s);
    default: return launch_scan_t<FILT, QB, 0, MODE, SB>(a, accept, nq, nc, s);
  }
}
template <bool FILT, int MODE>
static hipError_t launch_scan_mb(const ScanArgs &a, const uint64_t *accept, int planes, int nq, int nc, hipStream_t s) {
  switch (a.idx.geom.store_bits) {
    case 2: return planes > 4 ? launch_scan_mb_w<FILT, 8, MODE, 2>(a, accept, nq, nc, s) : launch_scan_mb_w<FILT, 4, MODE, 2>(a, accept, nq, nc, s);
    case 4: return planes > 4 ? launch_scan_mb_w<FILT, 8, MODE, 4>(a, accept, nq, nc, s) : launch_scan_mb_w<FILT, 4, MODE, 4>(a, accept, nq, nc, s);
    case 8: return launch_scan_t<FILT, 8, 0, MODE, 8>(a, accept, nq, nc, s);
    default: return hipErrorInvalidValue;
  }
}

template <bool FILT, int QB, int MODE>
static hipError_t launch_scan_w(const ScanArgs &a, const uint64_t *accept, int nq, int nc, hipStream_t s, int tpw = 1) {
  switch (a.idx.geom.w16) {
    case 1: return launch_scan_t<FILT, QB, 1, MODE>(a, accept, nq, nc, s, tpw);    // dim <= 128
    case 6: return launch_scan_t<FILT, QB, 6, MODE>(a, accept, nq, nc, s, tpw);    // dim 768
    case 8: return launch_scan_t<FILT, QB, 8, MODE>(a, accept, nq, nc, s, tpw);    // dim 1024
    case 12: return launch_scan_t<FILT, QB, 12, MODE>(a, accept, nq, nc, s, tpw);  // dim 1536
    default: return launch_scan_t<FILT, QB, 0, MODE>(a, accept, nq, nc, s, tpw);
  }
}

template <bool FILT, int MODE>
static hipError_t launch_scan_q(const ScanArgs &a, const uint64_t *accept, int planes, int nq, int nc, hipStream_t s, int tpw = 1) {
  switch (planes) {
    case 1: return launch_scan_w<FILT, 1, MODE>(a, accept, nq, nc, s, tpw);
    case 2: return launch_scan_w<FILT, 2, MODE>(a, accept, nq, nc, s, tpw);
    case 4: return launch_scan_w<FILT, 4, MODE>(a, accept, nq, nc, s, tpw);
    default: return launch_scan_w<FILT, 8, MODE>(a, accept, nq, nc, s, tpw);
  }
}

}  // namespace bbq
