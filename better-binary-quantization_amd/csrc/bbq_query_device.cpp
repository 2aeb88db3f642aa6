// bbq_query_device.cpp - raw fp32 queries quantized on the device (bbq_query_kernels.hip): bbq_quantize_queries_device, and the option
// device_queries, under which bbq_search_raw_batch prepares its queries here instead of on host threads (bbq_core.cpp)
#include <string.h>
#include "bbq_host.h"

using namespace bbq;

namespace {

constexpr int32_t kSubBatch = 4096;  // queries per upload, launch and download

// one sub-batch's arrays inside the context's scratch, each on a 16-byte boundary
struct Layout {
  size_t queries, centroid, qquant, qcorr, status, bytes;
  Layout(int32_t nq, int32_t dim) {
    queries = 0;
    centroid = align16(queries + (size_t)nq * dim * sizeof(float));
    qquant = align16(centroid + (size_t)dim * sizeof(float));
    qcorr = align16(qquant + (size_t)nq * dim);
    status = align16(qcorr + (size_t)nq * 4 * sizeof(double));
    bytes = align16(status + (size_t)nq * sizeof(uint32_t));
  }
};

}  // namespace

bool bbq::device_queries_for_call(const bbq_index *ix) {
  return ix->opt_device_queries == 1 && !ix->multi && !ix->has_pilot && ix->row_base == 0 && ix->geom.dim <= kQueryQuantMaxDim;
}

bool bbq::set_device_queries_option(bbq_index *ix, const char *name, int64_t v, int *rc) {
  if (strcmp(name, "device_queries") != 0) return false;
  if (v < -1 || v > 1) {
    *rc = fail(BBQ_ERR_INVALID_ARG, "bbq_set_option: unknown option or value out of range: %s=%lld", name, (long long)v);
  } else {
    ix->opt_device_queries = (int)v;
    *rc = BBQ_OK;
  }
  return true;
}

extern "C" {

int bbq_quantize_queries_device(bbq_index *ix, int32_t n, const float *queries, const float *centroid, int32_t sim, int32_t query_bits,
                                double lambda, int32_t iters, uint8_t *qquant, double *qcorr, int32_t *bad_query) {
  clear_error();
  if (bad_query) *bad_query = -1;
  if (n < 0) return fail(BBQ_ERR_INVALID_ARG, "n < 0");
  if (n == 0) return BBQ_OK;
  // the quantizer's own checks first (a handle's dimension is positive: without a handle the other arguments are still looked at)
  const int32_t dim = ix ? ix->geom.dim : 1;
  int rc = check_quantizer_args(queries, centroid, dim, sim, query_bits, lambda, iters);
  if (rc != BBQ_OK) return rc;
  if (!qquant || !qcorr) return fail(BBQ_ERR_INVALID_ARG, "null output");
  if (!ix) return fail(BBQ_ERR_INVALID_ARG, "bbq_quantize_queries_device: index handle is null");
  if (ix->multi) return fail(BBQ_ERR_UNSUPPORTED, "bbq_quantize_queries_device is not supported on a multi-device index");
  if (ix->has_pilot || ix->row_base != 0) return fail(BBQ_ERR_UNSUPPORTED, "bbq_quantize_queries_device is not supported on a row shard");
  if (dim > kQueryQuantMaxDim)
    return fail(BBQ_ERR_UNSUPPORTED, "bbq_quantize_queries_device: %d dimensions; a query's working vector lives in one workgroup's LDS, which holds at most %d",
                dim, kQueryQuantMaxDim);
  std::lock_guard<std::mutex> lk(ix->ctx->mu);
  HIPCHK(hipSetDevice(ix->device));
  DeviceCtx *ctx = ix->ctx;
  hipStream_t st = ctx->aux_stream;
  const Layout lay(std::min(n, kSubBatch), dim);
  rc = reserve_scratch(ctx->d_query_quant, lay.bytes, "bbq_quantize_queries_device");
  if (rc != BBQ_OK) return rc;
  uint8_t *base = ctx->d_query_quant;
  QueryQuantArgs a{};
  a.queries = reinterpret_cast<const float *>(base + lay.queries);
  a.centroid = reinterpret_cast<const float *>(base + lay.centroid);
  a.qquant = base + lay.qquant;
  a.qcorr = reinterpret_cast<double *>(base + lay.qcorr);
  a.status = reinterpret_cast<uint32_t *>(base + lay.status);
  a.lambda = lambda;
  a.dim = dim;
  a.sim = sim;
  a.bits = query_bits;
  a.iters = iters;
  std::vector<uint32_t> status((size_t)n);
  HIPCHK(hipMemcpyAsync(base + lay.centroid, centroid, (size_t)dim * sizeof(float), hipMemcpyHostToDevice, st));
  // the sub-batches follow each other on the stream through the one scratch: an upload waits for the launch in front of it
  for (int32_t q0 = 0; q0 < n; q0 += kSubBatch) {
    const int32_t nq = std::min(kSubBatch, n - q0);
    HIPCHK(hipMemcpyAsync(base + lay.queries, queries + (size_t)q0 * dim, (size_t)nq * dim * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(launch_quantize_queries(a, nq, st));
    HIPCHK(hipMemcpyAsync(qquant + (size_t)q0 * dim, a.qquant, (size_t)nq * dim, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(qcorr + (size_t)q0 * 4, a.qcorr, (size_t)nq * 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(status.data() + q0, a.status, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  for (int32_t i = 0; i < n; ++i) {
    if (status[(size_t)i] == 0) continue;
    // the lowest bad query of the call: its code and message are the host function's, produced on this thread
    if (bad_query) *bad_query = i;
    rc = bbq_quantize_query(queries + (size_t)i * dim, dim, centroid, sim, query_bits, lambda, iters, qquant + (size_t)i * dim, qcorr + (size_t)i * 4);
    return rc != BBQ_OK ? rc : fail(BBQ_ERR_INVALID_ARG, "query quantization failed");
  }
  return BBQ_OK;
}

}  // extern "C"
