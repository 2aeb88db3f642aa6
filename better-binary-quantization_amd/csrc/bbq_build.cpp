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

  const int64_t npad = (n + kTileRows - 1) / kTileRows * kTileRows;
  const int dim4 = (dim + 3) / 4;
  DevBuf<float> d_in, d_vT4, d_cen;
  DevBuf<unsigned long long> d_bad;
  DevBuf<double> d_corr;
  DevBuf<uint8_t> d_codes;
  // every exit below that does not hand the index out retires it through destroy_unlocked (the context mutex is held)
  std::unique_ptr<bbq_index, void (*)(bbq_index *)> ix(new bbq_index(), destroy_unlocked);
  ix->device = device;
  HIPCHK(d_in.alloc((size_t)n * dim));
  HIPCHK(d_vT4.alloc((size_t)dim4 * npad * 4));
  HIPCHK(hipMemcpyAsync(d_in, vectors, (size_t)n * dim * 4, hipMemcpyHostToDevice, st));
  HIPCHK(launch_build_transpose(d_in, n, dim, npad, d_vT4, st));
  HIPCHK(hipStreamSynchronize(st));
  d_in.reset();  // the peak footprint of a build: the transposed copy alone from here on
  if (sim == BBQ_COSINE) HIPCHK(launch_build_normalize(d_vT4, n, dim, npad, st));  // src/binaryQuantizationFormat.ts:174-176
  // :196-211 NaN / Infinity validation on the processed vectors, first offender in row-major order
  unsigned long long bad = ~0ull;
  HIPCHK(d_bad.alloc(1));
  HIPCHK(hipMemcpyAsync(d_bad, &bad, 8, hipMemcpyHostToDevice, st));
  HIPCHK(launch_build_validate(d_vT4, n, dim, npad, d_bad, st));
  HIPCHK(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (bad != ~0ull) {
    const int64_t r = (int64_t)(bad / (unsigned long long)dim);
    const int c = (int)(bad % (unsigned long long)dim);
    float v = 0;
    HIPCHK(hipMemcpy(&v, d_vT4 + ((size_t)(c / 4) * npad + r) * 4 + (c & 3), 4, hipMemcpyDeviceToHost));
    if (bad_row) *bad_row = r;
    if (bad_col) *bad_col = c;
    if (v != v) return fail(BBQ_ERR_NAN_INPUT, "向量 %lld 位置 %d 包含NaN值", (long long)r, c);
    return fail(BBQ_ERR_INF_INPUT, "向量 %lld 位置 %d 包含Infinity值", (long long)r, c);
  }
  HIPCHK(d_cen.alloc((size_t)dim4 * 4));
  HIPCHK(launch_build_centroid(d_vT4, n, dim, npad, d_cen, st));  // :214
  HIPCHK(hipMemcpyAsync(centroid, d_cen, (size_t)dim * 4, hipMemcpyDeviceToHost, st));

  rc = attach_index(ix.get(), ctx, device, dim, index_bits);
  if (rc != BBQ_OK) return rc;
  ix->n_rows = n;
  ix->row_base = 0;
  ix->want_compact = want_compact_of(opts);
  if (index_bits > 1) {
    // more than one bit: the kernel leaves what the reference keeps for such an index - one byte per dimension - and the corrections
    // in device memory; the tile records are built from there exactly as bbq_index_create builds them from host rows
    HIPCHK(d_codes.alloc((size_t)n * dim));
    HIPCHK(d_corr.alloc((size_t)n * 4));
    HIPCHK(launch_build_quantize_bits(d_vT4, n, dim, npad, d_cen, sim, lambda, iters, index_bits, d_codes, d_corr, st));  // :221-249
    HIPCHK(hipStreamSynchronize(st));
    d_vT4.reset();  // before the tile records are allocated
    ix->centroid_dp = bbq_centroid_dp(centroid, dim);
    rc = storage_from_device_rows(ix.get(), ix->main, d_codes, d_corr, n, 0, true);
    if (rc == BBQ_OK && corr && hipMemcpy(corr, d_corr, (size_t)n * 32, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(BBQ_ERR_HIP, "bbq_index_build: copy of the corrections failed");
    if (rc == BBQ_OK && codes && hipMemcpy(codes, d_codes, (size_t)n * dim, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(BBQ_ERR_HIP, "bbq_index_build: copy of the codes failed");
    if (rc != BBQ_OK) return rc;
    *out = ix.release();
    return BBQ_OK;
  }
  ix->has_x1 = 0;  // a freshly quantized 1-bit row's component sum IS its popcount
  ix->layout = ix->want_compact ? kLayoutCompact : kLayoutInline;
  ix->tile_stride = tile_stride_of(ix->w16, ix->layout, 0);
  ix->bytes_per_row = ix->tile_stride / kTileRows;
  Storage &sto = ix->main;
  const int64_t n_tiles = npad / kTileRows;
  HIPCHK(sto.d_tiles.alloc((size_t)n_tiles * ix->tile_stride));
  if (ix->layout == kLayoutCompact) HIPCHK(sto.d_exact.alloc((size_t)compact_side_bytes(n_tiles) / 8));
  sto.cap_tiles = n_tiles;
  if (corr) HIPCHK(d_corr.alloc((size_t)n * 4));
  HIPCHK(launch_build_quantize1(d_vT4, n, dim, npad, d_cen, sim, lambda, iters, sto.d_tiles, sto.d_exact, d_corr, ix->w16, ix->tile_stride,
                              ix->layout, st));  // :221-249
  if (ix->layout == kLayoutCompact) HIPCHK(launch_tile_add_range(sto.d_exact, n, const_cast<float *>(add_range_of(sto.d_exact, n_tiles)), st));
  if (corr) HIPCHK(hipMemcpyAsync(corr, d_corr, (size_t)n * 32, hipMemcpyDeviceToHost, st));
  if (codes) {
    HIPCHK(d_codes.alloc((size_t)n * ix->pb));
    HIPCHK(launch_build_untile(sto.d_tiles, n, ix->pb, ix->w16, ix->tile_stride, d_codes, st));
    HIPCHK(hipMemcpyAsync(codes, d_codes, (size_t)n * ix->pb, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  set_storage_view(ix.get(), sto, n, 0);
  ix->centroid_dp = bbq_centroid_dp(centroid, dim);  // getCentroidDP(undefined), :113-121
  *out = ix.release();
  return BBQ_OK;
}

}  // extern "C"
