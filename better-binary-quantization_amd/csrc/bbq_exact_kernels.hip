// bbq_exact_kernels.hip - exact search (gfx950): bbq_vectors_search_batch, the true top-k of raw queries over the resident fp32 rows.
//
// Score pass.  c(q, r) = computeSimilarity (reference src/vectorSimilarity.ts:14-126) for every (query of a block, row of a slab).  The
// arithmetic is bbq_maxsim_rerank_kernel's, and so are its bit-exactness rules (the top of bbq_maxsim_rerank_kernels.hip): every (query,
// row) is one sequential f64 chain in index order, COSINE's and MAXIMUM_INNER_PRODUCT's `dp += a * b` an explicit fma of an exact
// product, EUCLIDEAN's three operations kept apart, no contraction in this file; na per query comes precomputed (the same chain, once
// instead of once per row), nb is a chain of the lane's own.  v_mfma_f64 is no option: it adds four products before it rounds.  What
// differs is where the rows come from: they are contiguous, a lane is row row0 + 64 * blockIdx.x + lane, a wave the 64 rows of one
// accept word - no list, no search.  The wave streams its rows 32 columns at a time through LDS (each wave load covers two 128-byte row
// pieces, row stride padded to 33 words), the next stage's loads issued before the current stage's chains; the block's queries, widened
// to f64 by the host and laid a column's values side by side, are copied into LDS a stage at a time and read as 16-byte broadcasts.  A
// lane keeps one chain per query of the block in registers (64 VGPRs at 32 queries).  A row is read once per 32 queries: 8 multiply-adds
// per byte at 768 columns - the pass is bound by f64 issue and the LDS, not by HBM.
//
// Select pass.  One workgroup per query folds the slab's keys into the query's running list (ExactSelectArgs, bbq_device.h).  A thread
// tests four consecutive keys against the list's last key; what passes is compacted behind the list in LDS by a prefix sum over the
// workgroup - no atomic, so the arrival order cannot matter - and list and candidates are sorted together, bitonic, by (key descending,
// row ascending), which no two rows share: the first kk are the new list.  While the list is short of kk every accepted row passes and
// the list is closed as soon as kk rows are there; behind that a slab whose keys lie below the cut costs its read and one barrier per
// 4096 rows.  Rows stored in ascending score pass every test: then every second tile is sorted in, which is slow and exact.
#include <hip/hip_runtime.h>
#include "bbq_device.h"
#include "bbq_launch.h"

#pragma clang fp contract(off)

namespace bbq {

namespace {

constexpr int kExCols = 32;                  // columns per stage
constexpr int kExLoads = 64 * kExCols / 64;  // loads per lane per stage (= 32)
constexpr int QB = kExactQueryBlock;
constexpr int QG = kMaxSimRerankTokenGroup;
constexpr int kExactScoreThreads = 64;
static_assert(QB % QG == 0 && QB == kMaxSimTokenBlock, "a block is whole query groups, staged as a token block is");
static_assert(kExactSelectTile + kExactSelectMax <= kExactSelectSlots, "a tile of candidates fits behind a full list");

// wave-uniform read-only data (a query's na): the constant address space makes a load with a uniform address a scalar load
typedef const double __attribute__((address_space(4))) ScalarF64;
typedef double f64x2_t __attribute__((ext_vector_type(2)));
typedef unsigned long long u64x2_t __attribute__((ext_vector_type(2)));

// the chains of one stage: nc columns of the lane's row against the block's n_q queries, both staged in LDS - the row at the lane's
// own address (stride 33 words: conflict-free), the query value at one address for the whole wave (a broadcast), a group of QG
// queries at a time: a block pays for the groups it has.  qv: [column][tp8 * QG] f64
template <int SIM>
__device__ __forceinline__ void stage_chains(double (&acc)[QB], double &nb, const float *row, const double *qv, int nc, int tp8, int n_q) {
  for (int j = 0; j < nc; ++j) {
    const double bv = (double)row[j];
    if constexpr (SIM == 1) nb = __builtin_fma(bv, bv, nb);  // nb += bv * bv: an exact product
    const double *qk = qv + ((j * tp8) << 3);  // 64-byte aligned: the reads can be 16 bytes wide
#pragma unroll
    for (int g = 0; g < QB / QG; ++g) {
      if (g * QG < n_q) {  // wave-uniform
#pragma unroll
        for (int u = g * QG; u < (g + 1) * QG; ++u) {
          const double av = qk[u];
          if constexpr (SIM == 0) {  // EUCLIDEAN :38-70
            const double diff = av - bv;
            acc[u] += diff * diff;
          } else {  // COSINE :73-101, MAXIMUM_INNER_PRODUCT :108-118
            acc[u] = __builtin_fma(av, bv, acc[u]);
          }
        }
      }
    }
  }
}

// grid = (waves of 64 rows of the slab, query blocks of the sub-batch)
template <int SIM>
__global__ __launch_bounds__(kExactScoreThreads) void bbq_exact_score_kernel(const ExactScoreArgs a) {
  const int64_t r0 = a.row0 + (int64_t)blockIdx.x * 64;  // < a.n: the grid ends with the rows
  const unsigned long long word = exact_accept_word(a.accept, a.n, r0 >> 6);
  if (word == 0ull) return;  // a wave with no accepted row loads nothing, and the select pass reads nothing of it
  const int q0 = (int)blockIdx.y * QB;
  const int n_q = min(QB, a.n_queries - q0);
  const int tp = (n_q + QG - 1) / QG * QG;  // the block's slots
  const int lane = threadIdx.x;
  const int dim = a.dim;
  __shared__ float s_rows[64][kExCols + 1];
  __shared__ __attribute__((aligned(16))) double s_q[kExCols * QB];  // [column of the stage][tp]
  __shared__ int64_t s_base[64];

  const bool accepted = (word >> lane) & 1ull;
  // a lane beyond the rows shadows the last row, so every address stays in bounds; its bit is clear
  const int64_t r = min(r0 + lane, a.n - 1);
  s_base[lane] = r * dim;
  __syncthreads();
  // lane -> (row it * 2 + lane / 32, column lane % 32) of the stage
  const int lc = lane & 31, lr = lane >> 5;
  float nxt[kExLoads];
  auto fetch = [&](int col0) {
    const bool in = col0 + lc < dim;
#pragma unroll
    for (int it = 0; it < kExLoads; ++it) nxt[it] = in ? a.vecs[s_base[it * 2 + lr] + col0 + lc] : 0.f;
  };
  fetch(0);
  double acc[QB];
#pragma unroll
  for (int t = 0; t < QB; ++t) acc[t] = 0.0;
  double nb = 0.0;
  const double *__restrict__ qv = a.queries + (int64_t)q0 * dim;  // 64-byte aligned: q0 and tp are multiples of QG
  for (int col0 = 0; col0 < dim; col0 += kExCols) {
#pragma unroll
    for (int it = 0; it < kExLoads; ++it) s_rows[it * 2 + lr][lc] = nxt[it];
    const int nc = min(kExCols, dim - col0);
    {  // the stage's query values: nc * tp f64, contiguous, copied 16 bytes a lane at a time
      const f64x2_t *__restrict__ gq = reinterpret_cast<const f64x2_t *>(qv + (int64_t)col0 * tp);
      f64x2_t *sq = reinterpret_cast<f64x2_t *>(s_q);
      for (int i = lane; i < nc * (tp / 2); i += 64) sq[i] = gq[i];
    }
    __syncthreads();
    if (col0 + kExCols < dim) fetch(col0 + kExCols);
    stage_chains<SIM>(acc, nb, s_rows[lane], s_q, nc, tp / QG, n_q);
    __syncthreads();
  }

  double snb = 0.0;
  if constexpr (SIM == 1) snb = sqrt(nb);
  unsigned long long *__restrict__ out = a.keys + (size_t)q0 * (size_t)a.stride + (size_t)(r0 - a.row0) + (size_t)lane;
#pragma unroll
  for (int t = 0; t < QB; ++t) {
    if (t < n_q) {  // wave-uniform
      double c;
      if constexpr (SIM == 1) {
        const double na = ((ScalarF64 *)a.na)[q0 + t];
        c = (na == 0 || nb == 0) ? 0.0 : acc[t] / (sqrt(na) * snb);
      } else if constexpr (SIM == 0) {
        c = 1.0 / (1.0 + sqrt(acc[t]));
      } else {
        c = acc[t];
      }
      out[(size_t)t * (size_t)a.stride] = accepted ? true_key((unsigned long long)__double_as_longlong(c), c != c) : 0ull;
    }
  }
}

// is (kb, rb) ranked in front of (ka, ra)?
__device__ __forceinline__ bool ranks_first(unsigned long long kb, int32_t rb, unsigned long long ka, int32_t ra) {
  return kb > ka || (kb == ka && rb < ra);
}

// grid = the sub-batch's queries; dynamic LDS: kExactSelectLdsBytes
__global__ __launch_bounds__(kExactSelectThreads) void bbq_exact_select_kernel(const ExactSelectArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
  unsigned long long *s_key = reinterpret_cast<unsigned long long *>(s_mem);                 // [kExactSelectSlots]
  int32_t *s_row = reinterpret_cast<int32_t *>(s_mem + (size_t)kExactSelectSlots * 8);       // [kExactSelectSlots]
  __shared__ int s_wcnt[2][kExactSelectThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kk = a.kk;
  const unsigned long long *__restrict__ keys = a.keys + (size_t)blockIdx.x * (size_t)a.stride;
  unsigned long long *lk = a.list_keys + (size_t)blockIdx.x * (size_t)kk;
  int32_t *lrow = a.list_rows + (size_t)blockIdx.x * (size_t)kk;

  // everything below that steers a branch or a barrier is the same in every thread: cnt, ncand, total, thr
  int cnt = min(max(a.list_count[blockIdx.x], 0), kk);
  for (int i = tid; i < cnt; i += kExactSelectThreads) {
    s_key[i] = lk[i];
    s_row[i] = lrow[i];
  }
  __syncthreads();
  int ncand = 0, par = 0;
  bool dirty = false;
  unsigned long long thr = cnt == kk ? s_key[kk - 1] : 0ull;  // what a key has to beat; 0: every accepted row (its key is >= 1)

  // list [0, cnt) and candidates [cnt, cnt + ncand) sorted together, the best kk kept
  auto merge = [&]() {
    const int m = cnt + ncand;
    int np2 = 1;
    while (np2 < m) np2 <<= 1;
    for (int i = m + tid; i < np2; i += kExactSelectThreads) {
      s_key[i] = 0ull;
      s_row[i] = 0x7fffffff;
    }
    __syncthreads();
    for (int k2 = 2; k2 <= np2; k2 <<= 1) {
      for (int j = k2 >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < np2; i += kExactSelectThreads) {
          const int l = i ^ j;
          if (l > i) {
            const bool up = (i & k2) == 0;  // this run comes out best first
            const unsigned long long ka = s_key[i], kb = s_key[l];
            const int32_t ra = s_row[i], rb = s_row[l];
            if (ranks_first(kb, rb, ka, ra) == up && !(ka == kb && ra == rb)) {
              s_key[i] = kb; s_row[i] = rb;
              s_key[l] = ka; s_row[l] = ra;
            }
          }
        }
        __syncthreads();
      }
    }
    cnt = min(kk, m);
    ncand = 0;
    thr = cnt == kk ? s_key[kk - 1] : 0ull;
    dirty = true;
  };

  for (int p0 = 0; p0 < a.rows; p0 += kExactSelectTile) {
    const int p = p0 + tid * 4;
    unsigned long long k4[4] = {0ull, 0ull, 0ull, 0ull};
    if (p < a.rows) {
      const int64_t r = a.row0 + p;  // a multiple of 4: the four rows share an accept word
      const unsigned m4 = (unsigned)(exact_accept_word(a.accept, a.n, r >> 6) >> (r & 63)) & 0xfu;
      if (m4) {  // the score pass has written the keys of this word's rows
        const u64x2_t lo = *reinterpret_cast<const u64x2_t *>(keys + p), hi = *reinterpret_cast<const u64x2_t *>(keys + p + 2);
        k4[0] = (m4 & 1u) ? lo.x : 0ull;
        k4[1] = (m4 & 2u) ? lo.y : 0ull;
        k4[2] = (m4 & 4u) ? hi.x : 0ull;
        k4[3] = (m4 & 8u) ? hi.y : 0ull;
      }
    }
    int c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) c += k4[j] > thr ? 1 : 0;
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
    for (int w = 0; w < kExactSelectThreads / 64; ++w) {
      const int v = s_wcnt[par][w];
      total += v;
      if (w < wave) before += v;
    }
    par ^= 1;  // the next tile's counts go to the other row: no second barrier
    if (total == 0) continue;
    int at = cnt + ncand + before + incl - c;  // < kExactSelectSlots: a tile starts with room for all of it
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (k4[j] > thr) {
        s_key[at] = k4[j];
        s_row[at] = (int32_t)(a.row0 + p + j);
        ++at;
      }
    }
    ncand += total;
    // close a short list as soon as kk rows are there - the test needs its last key - and make room for the next tile
    if ((cnt < kk && cnt + ncand >= kk) || cnt + ncand + kExactSelectTile > kExactSelectSlots) {
      __syncthreads();
      merge();
    }
  }
  if (ncand > 0) {
    __syncthreads();
    merge();
  }
  if (!dirty) return;
  for (int i = tid; i < cnt; i += kExactSelectThreads) {
    lk[i] = s_key[i];
    lrow[i] = s_row[i];
  }
  if (tid == 0) a.list_count[blockIdx.x] = cnt;
}

}  // namespace

hipError_t launch_exact_score(const ExactScoreArgs &a, int64_t rows, hipStream_t s) {
  if (rows <= 0 || a.n_queries <= 0) return hipSuccess;
  if (!a.vecs || !a.queries || !a.keys || (a.sim == 1 && !a.na)) return hipErrorInvalidValue;
  if (a.dim <= 0 || a.row0 < 0 || (a.row0 & 63) || a.row0 + rows > a.n || rows > a.stride) return hipErrorInvalidValue;
  const int64_t waves = (rows + 63) / 64, blocks = (a.n_queries + QB - 1) / QB;
  if (waves > 0x7fffffffll || blocks > 65535 || waves * 64 > a.stride) return hipErrorInvalidValue;
  const dim3 grid((unsigned)waves, (unsigned)blocks, 1), block(kExactScoreThreads, 1, 1);
  switch (a.sim) {
    case 0: hipLaunchKernelGGL(bbq_exact_score_kernel<0>, grid, block, 0, s, a); break;
    case 1: hipLaunchKernelGGL(bbq_exact_score_kernel<1>, grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL(bbq_exact_score_kernel<2>, grid, block, 0, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_exact_select(const ExactSelectArgs &a, int n_queries, hipStream_t s) {
  if (n_queries <= 0 || a.rows <= 0) return hipSuccess;
  if (!a.keys || !a.list_keys || !a.list_rows || !a.list_count) return hipErrorInvalidValue;
  if (a.kk < 1 || a.kk > kExactSelectMax || a.rows > a.stride || (a.stride & 3) || a.row0 < 0 || (a.row0 & 63) || a.row0 + a.rows > a.n)
    return hipErrorInvalidValue;
  static hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(bbq_exact_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               kExactSelectLdsBytes);  // once per process: more than the 64 KB a launch gets by default
  if (attr != hipSuccess) return attr;
  hipLaunchKernelGGL(bbq_exact_select_kernel, dim3((unsigned)n_queries), dim3(kExactSelectThreads), kExactSelectLdsBytes, s, a);
  return hipGetLastError();
}

}  // namespace bbq
