// bbq_search.h - what the search-side translation units share on top of bbq_host.h: the context of one call, and the functions
// that cross a file boundary (their comments stand at the definitions).
#pragma once
#include "bbq_host.h"

#pragma GCC visibility push(hidden)  // internal: none of this joins the library's dynamic symbols
namespace bbq {

struct BatchCtx {
  bbq_index *ix;
  const uint8_t *qquant;
  const double *qcorr;
  int planes, one_bit, sim;
  int64_t k;
  int maxq = 255;  // largest quantized query value of the call (the MFMA sweep needs <= 127)
};

// outputs of a sharded scan: the per-query lists live in the index's own buffers and (optionally) the shard-local answers go straight
// into the caller's device memory (bbq_shard_scan_begin)
struct ExtOut {
  uint64_t *lists = nullptr;     // [nq of the batch][list_cap], this sub-batch's first row
  int64_t list_cap = 0;
  int32_t *counts = nullptr;     // [nq][2]
  uint64_t *answers = nullptr;   // this sub-batch's first row of the caller's [n_queries][answers_stride], or null
  int64_t answers_stride = 0;
};

// ---- bbq_query.cpp
int max_value(const uint8_t *q, int64_t count);
int64_t query_data_bytes(const bbq_index *ix, int planes);
int planes_of_call(const bbq_index *ix, const uint8_t *q, int64_t count, int one_bit);
void fill_query(const bbq_index *ix, uint8_t *planes_dst, QueryParams *pp, const uint8_t *q, const double *qc, int planes,
                int one_bit, int sim);
void fill_query_mfma(const bbq_index *ix, uint8_t *dst, int q_in_batch, const uint8_t *q);
void fill_query_mfma_fp(const bbq_index *ix, uint8_t *dst, int q_in_batch, const uint8_t *q, int scale8);
bool mfma_query_ok(const QueryParams &p);
int validate_query_args(const bbq_index *ix, int32_t nq, const uint8_t *qquant, const double *qcorr, int32_t query_bits,
                        int32_t sim, int64_t k, bool values_pending = false);

// ---- bbq_core.cpp
int effective_batch(const bbq_index *ix, int64_t n_queries = 0);
void build_plan(bbq_index *ix, int64_t k, int64_t final_k = 0, bool latency = false);
int ensure_slot(bbq_index *ix, Slot &s, int nq, bool own_lists);
FinalizeArgs slot_finalize_args(const Slot &s, uint64_t *lists, int32_t *list_counts, int64_t list_cap, bool appended, int64_t k);
int enqueue_subbatch(const BatchCtx &c, Slot &s, int64_t q_first, int nq, const ExtOut *ext);
void account_timing(bbq_index *ix, Slot &s);
int begin_replay(const BatchCtx &c, Slot &s, int32_t *out_idx, float *out_score, int64_t *out_n);
int finish_replay(const BatchCtx &c, Slot &s, int32_t *out_idx, float *out_score, int64_t *out_n);
int drain(bbq_index *ix);
// ---- bbq_latency.cpp: *done = false with BBQ_OK sends the call on to the next, more general path
int search_latency_presampled(const BatchCtx &c, const BatchCtx &cs, int32_t *out_idx, float *out_score, int64_t *out_n, bool *done);
int search_latency_chain(const BatchCtx &c, const BatchCtx &cs, int32_t *out_idx, float *out_score, int64_t *out_n, bool *done);
// ---- bbq_dense.cpp
int dense_search_one(const BatchCtx &c, int64_t qi, int32_t *out_idx, float *out_score, int64_t *out_n);

}  // namespace bbq
#pragma GCC visibility pop
