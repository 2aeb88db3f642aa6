// bbq_build.cpp - quantizeVectors on the device and the index in place (kernels: bbq_build_kernels.hip)
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <string>
#include "bbq_host.h"

using namespace bbq;

extern "C" {

int bbq_index_build(const float *vectors, int64_t n, int32_t dim, int32_t sim, double lambda, int32_t iters, int32_t device,
                    bbq_index **out, float *centroid, uint8_t *codes, double *corr, int64_t *bad_row, int32_t *bad_col) {
  return bbq_index_build_bits(vectors, n, dim, sim, 1, lambda, iters, device, out, centroid, codes, corr, bad_row, bad_col);
}

// quantizeVectors on the device + index in place (bbq_build_kernels.hip)
int bbq_index_build_bits(const float *vectors, int64_t n, int32_t dim, int32_t sim, int32_t index_bits, double lambda, int32_t iters,
                         int32_t device, bbq_index **out, float *centroid, uint8_t *codes, double *corr, int64_t *bad_row, int32_t *bad_col) {
  return bbq_index_build_opts(vectors, n, dim, sim, index_bits, lambda, iters, device, nullptr, out, centroid, codes, corr, bad_row, bad_col);
}

int bbq_index_build_opts(const float *vectors, int64_t n, int32_t dim, int32_t sim, int32_t index_bits, double lambda, int32_t iters,
                         int32_t device, const bbq_index_options *opts, bbq_index **out, float *centroid, uint8_t *codes, double *corr,
                         int64_t *bad_row, int32_t *bad_col) {
  clear_error();
  if (!out) return fail(BBQ_ERR_INVALID_ARG, "bbq_index_build: out is null");
  *out = nullptr;
  if (index_bits < 1 || index_bits > 8) return fail(BBQ_ERR_INVALID_ARG, "indexBits必须在1-8之间");
  if (check_options(opts) != BBQ_OK) return BBQ_ERR_INVALID_ARG;
  if (!dim_supported(dim, dim == 1 ? 1 : store_bits_of(index_bits)))
    return fail(BBQ_ERR_UNSUPPORTED, "dimension %d at indexBits %d: the integer dot product would not fit 31 bits", dim, index_bits);
  if (n == 0) return fail(BBQ_ERR_EMPTY, "向量集合不能为空");
  if (n < 0 || dim <= 0 || !vectors || !centroid) return fail(BBQ_ERR_INVALID_ARG, "输入向量不能为空");
  if (sim < 0 || sim > 2) return fail(BBQ_ERR_INVALID_ARG, "不支持的相似性函数: %d", sim);
  if (iters < 0 || lambda != lambda) return fail(BBQ_ERR_INVALID_ARG, "bad lambda/iters");
  if (n > 0xFFFFFFFFll) return fail(BBQ_ERR_UNSUPPORTED, "more than 2^32 rows");
  DeviceCtx *ctx = nullptr;
  int rc = open_device(device, &ctx);
  if (rc != BBQ_OK) return rc;
  std::lock_guard<std::mutex> lk(ctx->mu);
  hipStream_t st = ctx->aux_stream;
  DevBuf<float> d_vT4, d_cen;
  rc = stage_vectors(ctx, vectors, n, dim, sim, d_vT4, bad_row, bad_col);
  if (rc != BBQ_OK) return rc;
  if (d_cen.alloc((size_t)(dim + 3) / 4 * 4) != hipSuccess) { (void)hipGetLastError(); return fail(BBQ_ERR_OOM, "no device memory for the centroid"); }
  HIPCHK(launch_build_centroid(d_vT4, n, dim, tiles_of(n) * kTileRows, d_cen, st));  // :214
  HIPCHK(hipMemcpyAsync(centroid, d_cen, (size_t)dim * 4, hipMemcpyDeviceToHost, st));
  // every exit below that does not hand the index out retires it through destroy_unlocked (the context mutex is held)
  std::unique_ptr<bbq_index, void (*)(bbq_index *)> ix(new bbq_index(), destroy_unlocked);
  rc = attach_index(ix.get(), ctx, device, dim, index_bits);
  if (rc != BBQ_OK) return rc;
  ix->want_compact = want_compact_of(opts);
  // the index is empty and its rows are an append to it.  No explicit sums: a freshly quantized 1-bit row's component sum IS its
  // popcount (multi-bit rows are asked, and the layout decided again, on their way into the tiles)
  decide_layout(ix.get());
  rc = quantize_into(ix.get(), d_vT4, n, d_cen, sim, lambda, iters, Sums::kDecide, codes, corr);
  if (rc != BBQ_OK) return rc;
  ix->centroid_dp = bbq_centroid_dp(centroid, dim);  // getCentroidDP(undefined), :113-121 (the device has completed: the centroid is there)
  *out = ix.release();
  return BBQ_OK;
}

}  // extern "C"
