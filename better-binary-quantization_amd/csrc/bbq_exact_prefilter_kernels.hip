// bbq_exact_prefilter_kernels.hip - exact search (gfx950): the prefilter in front of the f64 chains, and the compaction behind it.
//
// Prefilter pass.  The f64 chain of bbq_exact_score_kernel decides almost nothing: of a million rows about k can be in a query's
// answer.  This pass computes every (query, row) dot product in f32 on the matrix cores and turns it, with the f32 sums of squares
// of both, into an interval that is proved to hold c(query, row) (exact_side / exact_interval, bbq_device.h): what leaves the pass
// is the pair's lower end as a key - which the unchanged select pass folds into the k-th largest lower bound L - and its upper end.
// The split of the work: a workgroup is four waves and 256 rows against one block of up to 64 queries; a wave is the 64 rows of
// one accept word and owns a 64 x 64 tile of dot products, four accumulators of v_mfma_f32_32x32x2_f32 - A = 32 queries, B = 32
// rows, so that a lane's accumulator registers are ONE row against sixteen queries and a half-wave's store of one register is 256
// contiguous bytes of a key row.  Rows and queries pass through LDS 32 columns at a stage: a lane loads 16-byte pieces, eight lanes
// one 128-byte row piece, into registers, the registers are written to LDS behind the barrier, and the next stage's loads are issued
// before this stage's MFMAs.  In LDS a row or query takes 36 words, so a lane's operands of four MFMA steps are one ds_read_b128:
// the lower half-wave feeds columns 8 t .. 8 t + 3 of column group t to steps 0 .. 3, the upper half-wave columns 8 t + 4 .. 8 t + 7 -
// the order of a dot product's terms is free, only A and B have to agree.  The lane that feeds a row's value squares it into an f32
// accumulator; the two half-waves' sums joined are the row's sum of squares.  Columns beyond dim are zeros; a width that is no
// multiple of 4 loads its pieces word by word.  A wave without an accepted row loads, multiplies and writes nothing.
//
// Compaction pass.  One workgroup per query walks the slab's upper ends behind the select pass, four rows a thread, and appends the
// rows that may still be in the answer - upper end at or above L - to the query's survivor list by a prefix sum over the workgroup:
// in row order, whatever order the waves run in.
#include <hip/hip_runtime.h>
#include "bbq_device.h"
#include "bbq_launch.h"

#pragma clang fp contract(off)

namespace bbq {

namespace {

constexpr int QP = kExactPreQueries, CH = kExactPreCols, LS = kExactPreStride;
constexpr int kPreThreads = 64 * kExactPreWaves;
constexpr int kPieces = CH / 4;                         // 16-byte pieces of a staged row
constexpr int kRowLoads = kPieces;                      // pieces a lane loads of its wave's 64 rows per stage
constexpr int kQueryLoads = QP * kPieces / kPreThreads; // ... of the block's queries
constexpr int kCompactThreads = 1024;
constexpr int kCompactTile = 4 * kCompactThreads;
static_assert(kPieces == 8 && kQueryLoads * kPreThreads == QP * kPieces && LS % 4 == 0, "a lane's piece is (index / 8, index % 8)");
static_assert(QP == 64, "two MFMA blocks of 32 queries");

typedef float f32x4p __attribute__((ext_vector_type(4)));
typedef float f32x16p __attribute__((ext_vector_type(16)));
typedef unsigned long long u64x2p __attribute__((ext_vector_type(2)));

// the piece of four columns from `col` on of the vector at p; beyond dim: zeros
template <bool ALIGNED>
__device__ __forceinline__ f32x4p load_piece(const float *__restrict__ p, int col, int dim) {
  f32x4p v = {0.f, 0.f, 0.f, 0.f};
  if constexpr (ALIGNED) {  // dim is a multiple of 4: a piece lies inside the vector or outside
    if (col < dim) v = *reinterpret_cast<const f32x4p *>(p + col);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (col + i < dim) v[i] = p[col + i];
  }
  return v;
}

// grid = (tiles of kExactPreRows rows of the slab, blocks of QP queries of the sub-batch)
template <int SIM, bool ALIGNED>
__global__ __launch_bounds__(kPreThreads) void bbq_exact_prefilter_kernel(const ExactPrefilterArgs a) {
  __shared__ __attribute__((aligned(16))) float s_rows[kExactPreWaves][64 * LS];
  __shared__ __attribute__((aligned(16))) float s_q[QP * LS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r0 = a.row0 + (int64_t)blockIdx.x * kExactPreRows + wave * 64;
  // the slab ends with the rows or on a multiple of the tile: a wave beyond the rows has no accept word to read
  const unsigned long long word = r0 < a.n ? exact_accept_word(a.accept, a.n, r0 >> 6) : 0ull;
  if (!__syncthreads_or(word != 0ull)) return;
  const bool live = word != 0ull;  // wave-uniform
  const int q0 = (int)blockIdx.y * QP;
  const int n_q = min(QP, a.n_queries - q0);
  const bool two = n_q > 32;
  const int dim = a.dim;

  // lane -> piece (row it * 8 + lane / 8, columns 4 (lane % 8) ..) of the wave's rows; a row beyond the rows shadows the last row, so
  // every address stays in bounds - its accept bit is clear
  const int pc = (lane & 7) * 4;
  const float *rp[kRowLoads];
#pragma unroll
  for (int it = 0; it < kRowLoads; ++it) rp[it] = a.vecs + min(r0 + it * 8 + (lane >> 3), a.n - 1) * dim;
  // thread -> piece (query it * 32 + tid / 8, the same columns) of the block's queries; a slot behind the queries is zeros
  const float *qp[kQueryLoads];
#pragma unroll
  for (int it = 0; it < kQueryLoads; ++it) {
    const int qi = it * (kPreThreads / 8) + (tid >> 3);
    qp[it] = qi < n_q ? a.queries + (int64_t)(q0 + qi) * dim : nullptr;
  }
  f32x4p nr[kRowLoads], nq[kQueryLoads];
  auto fetch = [&](int col0) {
    if (live) {
#pragma unroll
      for (int it = 0; it < kRowLoads; ++it) nr[it] = load_piece<ALIGNED>(rp[it], col0 + pc, dim);
    }
#pragma unroll
    for (int it = 0; it < kQueryLoads; ++it) nq[it] = qp[it] ? load_piece<ALIGNED>(qp[it], col0 + pc, dim) : f32x4p{0.f, 0.f, 0.f, 0.f};
  };
  fetch(0);

  f32x16p acc[2][2];  // [query block][row block]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[i >> 1][i & 1][j] = 0.f;
  float sq0 = 0.f, sq1 = 0.f;
  // lane -> operand (vector lane % 32 of a block, columns 4 (lane / 32) .. of a column group)
  const int on = (lane & 31) * LS + (lane >> 5) * 4;
  float *my_rows = s_rows[wave];

  for (int col0 = 0; col0 < dim; col0 += CH) {
    if (live) {
#pragma unroll
      for (int it = 0; it < kRowLoads; ++it) *reinterpret_cast<f32x4p *>(my_rows + (it * 8 + (lane >> 3)) * LS + pc) = nr[it];
    }
#pragma unroll
    for (int it = 0; it < kQueryLoads; ++it) *reinterpret_cast<f32x4p *>(s_q + (it * (kPreThreads / 8) + (tid >> 3)) * LS + pc) = nq[it];
    __syncthreads();
    if (col0 + CH < dim) fetch(col0 + CH);
    if (live) {
      const int groups = (min(CH, dim - col0) + 7) >> 3;  // column groups of 8 that hold a column
      for (int t = 0; t < groups; ++t) {
        const f32x4p b0 = *reinterpret_cast<const f32x4p *>(my_rows + on + t * 8);
        const f32x4p b1 = *reinterpret_cast<const f32x4p *>(my_rows + on + 32 * LS + t * 8);
        const f32x4p a0 = *reinterpret_cast<const f32x4p *>(s_q + on + t * 8);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[i], b0[i], acc[0][0], 0, 0, 0);
          acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[i], b1[i], acc[0][1], 0, 0, 0);
          sq0 = __builtin_fmaf(b0[i], b0[i], sq0);
          sq1 = __builtin_fmaf(b1[i], b1[i], sq1);
        }
        if (two) {
          const f32x4p a1 = *reinterpret_cast<const f32x4p *>(s_q + on + 32 * LS + t * 8);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[i], b0[i], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[i], b1[i], acc[1][1], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }
  if (!live) return;

  // the lane's two rows: lane % 32 of each row block, their sums of squares the two half-waves' joined
  sq0 += __shfl_xor(sq0, 32, 64);
  sq1 += __shfl_xor(sq1, 32, 64);
  const ExactSide rs[2] = {exact_side(dim, sq0), exact_side(dim, sq1)};
  const int64_t at = (r0 - a.row0) + (lane & 31);
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
    if (mb * 32 < n_q) {  // wave-uniform
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int qi = mb * 32 + (j & 3) + 8 * (j >> 2) + 4 * (lane >> 5);  // the accumulator's row: register j of this half-wave
        if (qi < n_q) {
          const ExactSide qs = a.sides[q0 + qi];
          const size_t key_row = (size_t)(q0 + qi) * (size_t)a.stride;
#pragma unroll
          for (int nb = 0; nb < 2; ++nb) {
            double lo, hi;
            exact_interval(dim, SIM, (double)acc[mb][nb][j], qs, rs[nb], &lo, &hi);
            const bool accepted = (word >> (nb * 32 + (lane & 31))) & 1ull;
            const size_t o = key_row + (size_t)(at + nb * 32);
            a.lo_keys[o] = accepted ? true_key((unsigned long long)__double_as_longlong(lo), lo != lo) : 0ull;
            a.hi_keys[o] = true_key((unsigned long long)__double_as_longlong(hi), false);
          }
        }
      }
    }
  }
}

// grid = the sub-batch's queries
__global__ __launch_bounds__(kCompactThreads) void bbq_exact_compact_kernel(const ExactCompactArgs a) {
  __shared__ int s_wcnt[2][kCompactThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t q = blockIdx.x;
  // the k-th largest lower bound so far; 0: the list is short, every accepted row passes.  Uniform, as cnt is
  const unsigned long long cut = a.list_count[q] >= a.kk ? a.list_keys[q * (size_t)a.kk + (size_t)(a.kk - 1)] : 0ull;
  const unsigned long long *__restrict__ hi = a.hi_keys + q * (size_t)a.stride;
  int32_t *out = a.surv_rows + q * (size_t)a.cap;
  int cnt = a.surv_count[q], par = 0;
  for (int p0 = 0; p0 < a.rows; p0 += kCompactTile) {
    const int p = p0 + tid * 4;
    unsigned pass = 0;
    if (p < a.rows) {
      const int64_t r = a.row0 + p;  // a multiple of 4: the four rows share an accept word
      const unsigned m4 = (unsigned)(exact_accept_word(a.accept, a.n, r >> 6) >> (r & 63)) & 0xfu;
      if (m4) {  // the prefilter has written the keys of this word's rows
        const u64x2p k01 = *reinterpret_cast<const u64x2p *>(hi + p), k23 = *reinterpret_cast<const u64x2p *>(hi + p + 2);
        pass = m4 & ((k01.x >= cut ? 1u : 0u) | (k01.y >= cut ? 2u : 0u) | (k23.x >= cut ? 4u : 0u) | (k23.y >= cut ? 8u : 0u));
      }
    }
    const int c = __popc(pass);
    int incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(incl, (unsigned)d, 64);
      if (lane >= d) incl += o;
    }
    if (lane == 63) s_wcnt[par][wave] = incl;
    __syncthreads();
    int total = 0, before = 0;
#pragma unroll
    for (int w = 0; w < kCompactThreads / 64; ++w) {
      const int v = s_wcnt[par][w];
      total += v;
      if (w < wave) before += v;
    }
    par ^= 1;  // the next tile's counts go to the other row: no second barrier
    int at = cnt + before + incl - c;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if ((pass >> j) & 1u) {
        if (at < a.cap) out[at] = (int32_t)(a.row0 + p + j);
        ++at;
      }
    }
    cnt = min(cnt + total, 0x40000000);  // beyond the capacity only the fact is kept
  }
  if (tid == 0) a.surv_count[q] = cnt;
}

template <int SIM>
void launch_prefilter_t(const ExactPrefilterArgs &a, dim3 grid, hipStream_t s) {
  // 16-byte pieces need rows that start on 16 bytes
  if ((a.dim & 3) == 0 && (reinterpret_cast<uintptr_t>(a.vecs) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.queries) & 15) == 0)
    hipLaunchKernelGGL((bbq_exact_prefilter_kernel<SIM, true>), grid, dim3(kPreThreads, 1, 1), 0, s, a);
  else
    hipLaunchKernelGGL((bbq_exact_prefilter_kernel<SIM, false>), grid, dim3(kPreThreads, 1, 1), 0, s, a);
}

}  // namespace

hipError_t launch_exact_prefilter(const ExactPrefilterArgs &a, int64_t rows, hipStream_t s) {
  if (rows <= 0 || a.n_queries <= 0) return hipSuccess;
  if (!a.vecs || !a.queries || !a.sides || !a.lo_keys || !a.hi_keys || !exact_prefilter_serves(a.sim)) return hipErrorInvalidValue;
  if (a.dim <= 0 || a.row0 < 0 || (a.row0 % kExactPreRows) || a.row0 + rows > a.n || rows > a.stride || (a.stride & 63)) return hipErrorInvalidValue;
  const int64_t tiles = (rows + kExactPreRows - 1) / kExactPreRows, blocks = (a.n_queries + QP - 1) / QP;
  // a tile's waves that hold a row write whole words of keys: the rows rounded up to 64 fit the key rows
  if (tiles > 0x7fffffffll || blocks > 65535 || (rows + 63) / 64 * 64 > a.stride) return hipErrorInvalidValue;
  const dim3 grid((unsigned)tiles, (unsigned)blocks, 1);
  if (a.sim == 1) launch_prefilter_t<1>(a, grid, s);
  else launch_prefilter_t<2>(a, grid, s);
  return hipGetLastError();
}

hipError_t launch_exact_compact(const ExactCompactArgs &a, int n_queries, hipStream_t s) {
  if (n_queries <= 0 || a.rows <= 0) return hipSuccess;
  if (!a.hi_keys || !a.list_keys || !a.list_count || !a.surv_rows || !a.surv_count) return hipErrorInvalidValue;
  if (a.kk < 1 || a.cap < 1 || a.rows > a.stride || (a.stride & 3) || a.row0 < 0 || (a.row0 & 63) || a.row0 + a.rows > a.n) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bbq_exact_compact_kernel, dim3((unsigned)n_queries), dim3(kCompactThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace bbq
