// bbq_filter_kernels.hip - the filtered instantiations of the per-query sweep (bbq_scan_body.h, FILT = true): the sparse modes of
// every QB / W / SB form the unfiltered kernel has, in a translation unit of their own so that the two families compile side by side.
#include <hip/hip_runtime.h>
#include "bbq_device.h"
#include "bbq_kernel_common.h"
#include "bbq_launch.h"
#include "bbq_scan_body.h"

#pragma clang fp contract(off)

namespace bbq {

hipError_t launch_scan_filtered(const ScanArgs &a, const uint64_t *accept, int planes, int n_queries, int n_chunks, hipStream_t s) {
  if (n_chunks <= 0 || n_queries <= 0) return hipSuccess;
  if (!accept) return hipErrorInvalidValue;
  const bool compact = a.idx.geom.layout == kLayoutCompact;
  if (a.idx.geom.store_bits > 1)
    return compact ? launch_scan_mb<true, 2>(a, accept, planes, n_queries, n_chunks, s) : launch_scan_mb<true, 0>(a, accept, planes, n_queries, n_chunks, s);
  return compact ? launch_scan_q<true, 2>(a, accept, planes, n_queries, n_chunks, s) : launch_scan_q<true, 0>(a, accept, planes, n_queries, n_chunks, s);
}

}  // namespace bbq
