// bbq_maxsim_rerank_kernels.hip - exact MaxSim rerank of candidate groups (gfx950): bbq_rerank_maxsim_groups_batch.
//
// T = M_0 + M_1 + ... of include/bbq.h: M_t the greatest computeSimilarity (reference src/vectorSimilarity.ts:14-126) of token t against
// the accepted fp32 rows of a candidate group.  The score pass takes its rows as bbq_maxsim_cand_kernel does - a lane is one row of the
// query's EXPANDED rows and finds its candidate by binary search over the MaxSimCand records, once per token block - and its arithmetic
// as bbq_rerank_kernel does: the reference accumulates in f64 in index order, so every (token, row) is one sequential chain.  A lane
// keeps one chain per token of the block in registers (64 VGPRs at 32 tokens) and the row is gathered ONCE per token block, 32 columns
// at a time through LDS (each wave load covers two 128-byte row pieces, row stride padded to 33 words), the next stage's loads issued
// before the current stage's chains.  The token values are the same in every lane: the host has widened them to f64 and laid a column's
// tokens side by side (MaxSimRerankArgs, bbq_device.h), a stage's are one contiguous piece that the wave copies into LDS, and the chains
// read them as broadcasts, 16 bytes a read - no conversion per multiply-add.  HBM traffic is the candidates' rows once per block; the
// work is tokens x rows x dim v_fma_f64, and what feeds them is the LDS: one 16-byte broadcast per two of them.
//
// Bit-exactness.  The file is compiled without contraction.  COSINE's and MAXIMUM_INNER_PRODUCT's `dp += a * b` is issued as an explicit
// fma: a and b are f32 values widened to f64, so their product has at most 24 + 24 = 48 significant bits and an exponent in
// [-298, 254] - it is exact in f64 (53 bits, exponents -1022 .. 1023, no underflow), and where a or b is not finite both forms give the
// same Inf or NaN.  a * b rounds to itself, so dp + round(a * b) and fma(a, b, dp) round the same real number once: the same bits.
// EUCLIDEAN's diff = a - b is not exact and diff * diff is rounded before the add: three operations, as the reference has them.
// COSINE's na (the token's squared norm) and nb (the row's) are chains of their own, independent of dp: nb is kept per lane, na comes
// precomputed per token (MaxSimRerankArgs::na), the same chain evaluated once instead of once per row.
//
// The maximum over the rows of a candidate is taken on the monotone 64-bit key of the f64 bits (true_key: a rejected row's is 0, a
// NaN's the lowest non-zero), by the six-step segmented maximum over the lanes of one candidate; a candidate wholly inside the wave is
// stored plainly into rep[token][entry], one that a wave's edge cuts - a workgroup is one wave - is raised with the 64-bit atomicMax
// into the cleared rep: an integer maximum does not depend on the order of its operands, so the result is the same on every run.
// There is no floating-point atomic.  The accumulate pass decodes the keys and adds a block's tokens in ascending order.
#include <hip/hip_runtime.h>
#include "bbq_device.h"
#include "bbq_launch.h"

#pragma clang fp contract(off)

namespace bbq {

namespace {

constexpr int kMrCols = 32;                  // columns per stage
constexpr int kMrLoads = 64 * kMrCols / 64;  // loads per lane per stage (= 32)
constexpr int TB = kMaxSimTokenBlock;
constexpr int TG = kMaxSimRerankTokenGroup;
constexpr int kTrueAccThreads = 256;
static_assert(kMaxSimRerankThreads == 64 && TB % TG == 0, "a workgroup is one wave; a block is whole token groups");

// wave-uniform read-only data (a token's na): the constant address space makes a load with a uniform address a scalar load
typedef const double __attribute__((address_space(4))) ScalarF64;
typedef double f64x2_t __attribute__((ext_vector_type(2)));

// the chains of one stage: nc columns of the lane's row against the block's n_tok tokens, both staged in LDS - the row at the lane's
// own address (stride 33 words: conflict-free), the token at one address for the whole wave (a broadcast), a group of TG tokens at a
// time: a query pays for the groups it has.  tok: [column][tp8 * TG] f64
template <int SIM>
__device__ __forceinline__ void stage_chains(double (&acc)[TB], double &nb, const float *row, const double *tok, int nc, int tp8, int n_tok) {
  for (int j = 0; j < nc; ++j) {
    const double bv = (double)row[j];
    if constexpr (SIM == 1) nb = __builtin_fma(bv, bv, nb);  // nb += bv * bv: an exact product, see above
    const double *tk = tok + ((j * tp8) << 3);  // 64-byte aligned: the reads can be 16 bytes wide
#pragma unroll
    for (int g = 0; g < TB / TG; ++g) {
      if (g * TG < n_tok) {  // wave-uniform
#pragma unroll
        for (int u = g * TG; u < (g + 1) * TG; ++u) {
          const double av = tk[u];
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

// grid = (pieces of 64 expanded rows of the longest list of the launch, the block's queries)
template <int SIM, bool FILT>
__global__ __launch_bounds__(kMaxSimRerankThreads) void bbq_maxsim_rerank_kernel(const MaxSimRerankArgs a) {
  const MaxSimQuery mq = a.queries[blockIdx.y];
  const MaxSimCandQuery cq = a.cq[mq.query];
  const int64_t x0 = (int64_t)blockIdx.x * kMaxSimRerankThreads;
  if (x0 >= cq.total) return;  // workgroup-uniform: this piece lies beyond the query's expanded rows
  const int n_tok = mq.n_tok < TB ? mq.n_tok : TB;
  const int tp = (n_tok + TG - 1) / TG * TG;  // the block's slots
  const int lane = threadIdx.x;
  const int dim = a.dim;
  __shared__ float s_rows[64][kMrCols + 1];
  __shared__ __attribute__((aligned(16))) double s_tok[kMrCols * TB];  // [column of the stage][tp]
  __shared__ int64_t s_base[64];

  // the lane's expanded row and its candidate: the last record at or in front of it.  A lane beyond the list shadows the list's last
  // row, so every address stays in bounds; it is a segment of its own whose key is 0
  const int64_t x = x0 + lane;
  const bool valid = x < cq.total;
  const uint32_t xc = (uint32_t)(valid ? x : (int64_t)cq.total - 1);
  const MaxSimCand *__restrict__ recs = a.recs + cq.rec_first;
  int e = 0;
  {
    int hi = cq.n_cand - 1;
    while (e < hi) {
      const int mid = (e + hi + 1) >> 1;
      if (recs[mid].pos <= xc) e = mid;
      else hi = mid - 1;
    }
  }
  const MaxSimCand rc = recs[e];
  const uint32_t next_pos = recs[e + 1].pos;  // the terminator's for the last candidate
  const int64_t r = (int64_t)rc.first_row + (xc - rc.pos);
  bool accepted = valid;
  if constexpr (FILT) accepted = valid && ((a.accept[r >> 6] >> (r & 63)) & 1ull);
  if (__ballot(accepted) == 0ull) return;  // a wave with no accepted row loads nothing

  // the lane's segment: the lanes of its candidate inside this wave
  const uint64_t heads = __ballot(!valid || xc == rc.pos) | 1ull;
  const int head = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));  // the first lane of this lane's segment
  const bool is_end = valid && (lane == 63 || ((heads >> (lane + 1)) & 1ull));
  const bool whole = (int64_t)rc.pos >= x0 && (int64_t)next_pos <= x0 + 64;  // no other wave of the launch sees this entry

  s_base[lane] = r * dim;
  __syncthreads();
  // lane -> (row it * 2 + lane / 32, column lane % 32) of the stage
  const int lc = lane & 31, lr = lane >> 5;
  float nxt[kMrLoads];
  auto fetch = [&](int col0) {
    const bool in = col0 + lc < dim;
#pragma unroll
    for (int it = 0; it < kMrLoads; ++it) nxt[it] = in ? a.vecs[s_base[it * 2 + lr] + col0 + lc] : 0.f;
  };
  fetch(0);
  double acc[TB];
#pragma unroll
  for (int t = 0; t < TB; ++t) acc[t] = 0.0;
  double nb = 0.0;
  const double *__restrict__ tok = a.tokens + (int64_t)mq.vec_first * dim;  // 64-byte aligned: vec_first and tp are multiples of TG
  for (int col0 = 0; col0 < dim; col0 += kMrCols) {
#pragma unroll
    for (int it = 0; it < kMrLoads; ++it) s_rows[it * 2 + lr][lc] = nxt[it];
    const int nc = min(kMrCols, dim - col0);
    {  // the stage's tokens: nc * tp f64, contiguous, copied 16 bytes a lane at a time
      const f64x2_t *__restrict__ gt = reinterpret_cast<const f64x2_t *>(tok + (int64_t)col0 * tp);
      f64x2_t *st = reinterpret_cast<f64x2_t *>(s_tok);
      for (int i = lane; i < nc * (tp / 2); i += 64) st[i] = gt[i];
    }
    __syncthreads();
    if (col0 + kMrCols < dim) fetch(col0 + kMrCols);
    stage_chains<SIM>(acc, nb, s_rows[lane], s_tok, nc, tp / TG, n_tok);
    __syncthreads();
  }

  double snb = 0.0;
  if constexpr (SIM == 1) snb = sqrt(nb);
  unsigned long long *__restrict__ rep = a.rep + (size_t)mq.vec_first * (size_t)a.stride + (size_t)e;  // token 0 of the block; token t: + t * stride
#pragma unroll
  for (int t = 0; t < TB; ++t) {
    if (t < n_tok) {  // wave-uniform
      double c;
      if constexpr (SIM == 1) {
        const double na = ((ScalarF64 *)a.na)[mq.vec_first + t];
        c = (na == 0 || nb == 0) ? 0.0 : acc[t] / (sqrt(na) * snb);
      } else if constexpr (SIM == 0) {
        c = 1.0 / (1.0 + sqrt(acc[t]));
      } else {
        c = acc[t];
      }
      unsigned long long key = accepted ? true_key((unsigned long long)__double_as_longlong(c), c != c) : 0ull;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(key, (unsigned)d, 64);
        if (lane - d >= head && o > key) key = o;
      }
      if (is_end && key != 0ull) {
        unsigned long long *dst = rep + (size_t)t * (size_t)a.stride;
        if (whole) *dst = key;
        else atomicMax(dst, key);
      }
    }
  }
}

// grid = (pieces of kTrueAccThreads entries, the block's queries)
__global__ __launch_bounds__(kTrueAccThreads) void bbq_maxsim_true_accumulate_kernel(const MaxSimTrueAccArgs a) {
  const int64_t slot = (int64_t)blockIdx.x * kTrueAccThreads + threadIdx.x;
  if (slot >= a.stride) return;
  const MaxSimQuery mq = a.queries[blockIdx.y];
  const unsigned long long *__restrict__ k = a.rep + (size_t)mq.vec_first * (size_t)a.stride + slot;
  const size_t at = (size_t)mq.query * (size_t)a.stride + slot;
  int t = 0;
  double acc;
  if (mq.flags & kMaxSimFirst) {
    acc = __longlong_as_double((long long)true_key_bits(k[0]));  // from M_0, not from 0.0
    t = 1;
  } else {
    acc = a.acc[at];
  }
  for (; t < mq.n_tok; ++t) acc = acc + __longlong_as_double((long long)true_key_bits(k[(size_t)t * (size_t)a.stride]));
  if ((mq.flags & kMaxSimLast) && acc != acc) acc = __longlong_as_double((long long)kTrueNaNBits);
  a.acc[at] = acc;
}

template <int SIM>
void launch_rerank_t(const MaxSimRerankArgs &a, dim3 grid, hipStream_t s) {
  if (a.accept) hipLaunchKernelGGL((bbq_maxsim_rerank_kernel<SIM, true>), grid, dim3(kMaxSimRerankThreads, 1, 1), 0, s, a);
  else hipLaunchKernelGGL((bbq_maxsim_rerank_kernel<SIM, false>), grid, dim3(kMaxSimRerankThreads, 1, 1), 0, s, a);
}

}  // namespace

hipError_t launch_maxsim_rerank_score(const MaxSimRerankArgs &a, int n_queries, int64_t longest, hipStream_t s) {
  if (n_queries <= 0 || longest <= 0) return hipSuccess;
  if (n_queries > 65535 || longest > kMaxSimCandMaxRows || a.dim <= 0) return hipErrorInvalidValue;  // grid.y; grid.x
  if (!a.vecs || !a.tokens || !a.queries || !a.cq || !a.recs || !a.rep || a.stride <= 0 || (a.sim == 1 && !a.na)) return hipErrorInvalidValue;
  dim3 grid((unsigned)((longest + kMaxSimRerankThreads - 1) / kMaxSimRerankThreads), (unsigned)n_queries, 1);
  switch (a.sim) {
    case 0: launch_rerank_t<0>(a, grid, s); break;
    case 1: launch_rerank_t<1>(a, grid, s); break;
    case 2: launch_rerank_t<2>(a, grid, s); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_maxsim_true_accumulate(const MaxSimTrueAccArgs &a, int n_queries, hipStream_t s) {
  if (n_queries <= 0 || a.stride <= 0) return hipSuccess;
  const int64_t blocks = (a.stride + kTrueAccThreads - 1) / kTrueAccThreads;
  if (n_queries > 65535 || blocks > 0x7fffffffll) return hipErrorInvalidValue;
  if (!a.rep || !a.queries || !a.acc) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bbq_maxsim_true_accumulate_kernel, dim3((unsigned)blocks, n_queries, 1), dim3(kTrueAccThreads, 1, 1), 0, s, a);
  return hipGetLastError();
}

}  // namespace bbq
