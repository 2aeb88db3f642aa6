// bbq_search.h - what the search-side translation units share on top of bbq_host.h: the one object of a call, and the functions
// that cross a file boundary (their comments stand at the definitions).
#pragma once
#include <functional>
#include "bbq_host.h"

// The accept set of a filtered search (bbq_filter.cpp): read-only after creation, so any number of calls and threads may share it.
struct bbq_filter {
  int device = 0;
  bbq::DeviceCtx *ctx = nullptr;
  int64_t n_rows = 0;                // rows of the index it was made for
  int64_t count = 0;                 // |A|
  bbq::DevBuf<uint64_t> d_bits;      // [ceil(n_rows / 64)] word t = tile t, bit l = lane l; bits at and beyond n_rows are clear
  std::vector<uint64_t> h_bits;      // the same on the host: the dense path offers the accepted rows from it
  std::vector<int32_t> cum;          // [chunks + 1] accepted rows in the chunks before chunk c: what the accepted-space plan is cut by
  int64_t first_chunk = -1, last_chunk = -1;  // the first and the last chunk that holds an accepted row (-1: none)
};

// A group set (include/bbq.h, bbq_group.cpp): read-only after creation, so any number of calls and threads may share it.  It keeps its
// own copy of the filter's words: the filter may go before it does.
struct bbq_groups {
  int device = 0;
  bbq::DeviceCtx *ctx = nullptr;
  int64_t n_rows = 0;    // rows of the index it was made for
  int64_t n_groups = 0;
  int64_t live = 0;      // L
  bool filtered = false;
  std::vector<int64_t> offsets;        // [n_groups + 1] the caller's
  std::vector<int32_t> slot;           // [n_groups] a group's rank among the live groups or -1: what a candidate list is checked against (bbq_maxsim_groups.cpp)
  bbq::DevBuf<uint64_t> d_words;       // [tiles + 1] starts, then - filtered - [tiles] accept
  bbq::DevBuf<uint32_t> d_index;       // [tiles + 1] first_group, then [non-empty groups + 1] slot
  bbq::DevBuf<int32_t> d_live_group;   // [max(L, 1)] the group number of every slot: what the MaxSim search answers with (bbq_maxsim.cpp)
  int64_t n_nonempty = 0;
};

// The original fp32 rows resident on one GPU (bbq_rerank.cpp): what the exact rerank calls score against.
struct bbq_vectors {
  int device = 0;
  bbq::DeviceCtx *ctx = nullptr;
  bbq::DevBuf<float> d;      // [cap][dim], the first n rows in use (bbq_vectors_append grows it like the index grows)
  int64_t n = 0;
  int32_t dim = 0;
  // grow-only staging for bbq_rerank_scores
  bbq::DevBuf<float> d_q;
  bbq::DevBuf<int64_t> d_off;
  bbq::DevBuf<int32_t> d_rows;
  bbq::DevBuf<double> d_out;
  // grow-only staging for bbq_vectors_search_batch (bbq_exact.cpp): a sub-batch's queries, running lists and slab keys on the device,
  // the staged queries and the returned lists on the host
  bbq::DevBuf<uint8_t> d_exact;
  bbq::PinnedBuf<uint8_t> h_exact_in, h_exact_out;
  int64_t opt_exact_slab_rows = 0;  // rows scored between two select passes; 0: what the scratch budget gives (bbq_exact.cpp)
};

#pragma GCC visibility push(hidden)  // internal: none of this joins the library's dynamic symbols
namespace bbq {

// One search call: the queries, how they are scored, its two ranks and its plan.  Every function below takes it; a step that runs with
// another sweep share (finish_replay's re-sweep) passes a copy.
struct SearchCall {
  bbq_index *ix;
  const uint8_t *qquant;
  const double *qcorr;
  int planes, one_bit, sim;
  int64_t k_out;               // the caller's k: strides the outputs, sizes the replayed heap
  int64_t k_dev = 0;           // the rank the device selects thresholds with: min(k, rows), + 1 when the device selects the answer itself
  int maxq = 255;              // largest quantized query value of the call (the MFMA sweep needs <= 127)
  int share;                   // queries per row load of the sparse sweeps of this enqueue: the index's sweep_share unless a step overrides it
  const Plan *plan = nullptr;  // the call's segment plan; null in a call that only takes the dense path
  // a filtered call (bbq_search_filtered_batch): only rows of `filter` exist for it, so n_eff = |A| stands wherever the unfiltered
  // call bounds a rank by the rows of the index (k_dev, the plan's final_k, the replayed heap)
  const bbq_filter *filter = nullptr;
  int64_t n_eff = 0;
  SearchCall(bbq_index *ix, const uint8_t *qquant, const double *qcorr, int planes, int32_t query_bits, int32_t sim, int64_t k)
      : ix(ix), qquant(qquant), qcorr(qcorr), planes(planes), one_bit(query_bits == 1 ? 1 : 0), sim(sim), k_out(k), share(ix->opt_share) {}
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
// the digit masks of a 4-plane query against a 1-bit index ([w16][kDigitMasks] 16-byte masks -> digits_dst) and their K -> pp->digit_k
int64_t digit_bytes_per_query_w(int w16);
void fill_query_digits(const bbq_index *ix, uint8_t *digits_dst, QueryParams *pp, const uint8_t *q);
// the sub-batch's queries once more as matrix-core operands + group maxima behind the `bytes` already staged in h_qbuf
struct MfmaStage { bool fp; int scale8; size_t off_qbytes, off_qmax, bytes; };
MfmaStage stage_queries_mfma(const SearchCall &c, uint8_t *h_qbuf, const QueryParams *hq, int64_t q_first, int nq, size_t bytes);
bool mfma_query_ok(const QueryParams &p);
// the f32 images of *pp's score uniforms and whether the f32 bound may use them (QueryParams::fast_bound)
void fast_bound_images(QueryParams *pp, double x1max, double qcmax, bool enable);
int validate_query_args(const bbq_index *ix, int32_t nq, const uint8_t *qquant, const double *qcorr, int32_t query_bits,
                        int32_t sim, int64_t k, bool values_pending = false);

// ---- bbq_core.cpp
int effective_batch(const bbq_index *ix, int64_t n_queries = 0);
// ScanArgs::l2_shift of a per-query sparse sweep: log2 of the queries co-scheduled per chunk (option l2_share)
int l2_share_shift(const bbq_index *ix);
// does a per-query sparse sweep of this index read the rows' component sums from the side array (option row_sums)?
bool row_sums_for_launch(const bbq_index *ix);
// the view a launch over the whole main storage gets, with that decision applied.  Context mutex held by the caller
inline IndexView main_launch_view(bbq_index *ix) {
  IndexView v = launch_view(ix, ix->main).view;
  v.row_sums = row_sums_for_launch(ix) ? ix->main.view.row_sums : nullptr;
  return v;
}
// does a call with `planes` bit-planes stage the digit masks for its per-query sparse sweeps (option digit_planes)?
bool digit_planes_for_call(const bbq_index *ix, int planes);
// tiles per wave of the per-query sparse sweeps of an index (option tiles_per_wave): what launch_scan takes
int tiles_per_wave_for(const bbq_index *ix);
Plan build_plan(const bbq_index *ix, int64_t k, int64_t final_k = 0, bool latency = false);
Plan build_filtered_plan(const bbq_index *ix, const bbq_filter &f, int64_t k, int64_t final_k, bool latency);
int ensure_slot(const SearchCall &c, Slot &s, int nq, bool own_lists);
FinalizeArgs slot_finalize_args(const Slot &s, uint64_t *lists, int32_t *list_counts, int64_t list_cap, bool appended, int64_t k);
int enqueue_subbatch(const SearchCall &c, Slot &s, int64_t q_first, int nq, const ExtOut *ext);
void account_timing(bbq_index *ix, Slot &s);
int begin_replay(const SearchCall &c, Slot &s, int32_t *out_idx, float *out_score, int64_t *out_n);
int finish_replay(const SearchCall &c, Slot &s, int32_t *out_idx, float *out_score, int64_t *out_n);
int replay_listed_query(const SearchCall &c, Slot &s, uint32_t listed, uint32_t flags, int32_t *out_idx, float *out_score, int64_t *out_n);
int drain(bbq_index *ix);
// ---- bbq_latency.cpp: *done = false with BBQ_OK sends the call on to the next, more general path
int search_latency_presampled(const SearchCall &c, int32_t *out_idx, float *out_score, int64_t *out_n, bool *done);
int search_latency_chain(const SearchCall &c, int32_t *out_idx, float *out_score, int64_t *out_n, bool *done);
// ---- bbq_compact.cpp: the map of a compaction by `f` - its accept words as they are on the device, and the ranks of its tiles
// uploaded into d_rank (BBQ_ERR_OOM).  Context mutex held, device current; returns with the ranks on the device.
int stage_compact_map(const bbq_filter *f, DevBuf<uint32_t> &d_rank, CompactMap *map);
// ---- bbq_update.cpp: the entries of an update block that take effect - positions into the block, ascending by ord, one per distinct
// ord (its last occurrence); an ord outside [0, n_rows) is BBQ_ERR_INVALID_ARG.  Host only.  stage_winners uploads the block's ords
// and the winner list (BBQ_ERR_OOM), enqueued on `s`.
int update_winners(const int32_t *ords, int64_t n, int64_t n_rows, std::vector<int64_t> &pos);
int stage_winners(hipStream_t s, const int32_t *ords, int64_t n, const std::vector<int64_t> &pos, DevBuf<int32_t> &d_ords, DevBuf<int64_t> &d_pos);
// ---- bbq_select.cpp: how a sub-batch of the span, grouped and MaxSim searches ends.  The device has scored every row (representative,
// sum) of every query into one array, selected k of them for the queries with a block, and the blocks are on the host: each block is
// proven (prove_selected, bbq_replay.cpp) and unpacked, and the reference's heap replayed over the scores of every other query.
struct SelectQuery {
  int64_t len;    // its scores; 0: it answers with nothing, status 0
  int64_t first;  // they start here in the score array; the sub-batch's scores are [0, sum of len)
  int32_t block;  // its answer block among those brought back, or -1: the device did not select
};
struct SelectTail {
  const SelectQuery *queries;
  int nq;
  const float *d_scores;    // the sub-batch's scores on the device ...
  const uint32_t *d_ords;   // ... and the row (group) behind each, or null: `walk` knows them
  const uint64_t *back;     // [blocks][out_stride] the answer blocks, on the host
  float *h_scores;          // host room for the scores ...
  uint32_t *h_ords;         // ... and the ords: touched only where a heap is replayed
  int64_t k;
  size_t out_stride;
  hipStream_t stream;       // idle on entry and on return
  int threads;              // option replay_threads
  int32_t *out_tag;         // the outputs, from the sub-batch's first query on: [nq][k] out_idx or out_group, ...
  float *out_score;
  int64_t *out_n;
  uint8_t *out_status;      // ... or null
};
// without an ord array: offers query s's rows to the heap in visiting order, scores[i] the score of the i-th
using RowWalk = std::function<void(int64_t s, const float *scores, HeapReplay &hr)>;
int finish_selected(const SelectTail &t, const RowWalk &walk = nullptr);
// ---- bbq_group.cpp: what a group set can be made for, and searched on - a single-device root index; and the score pass's arguments
// that follow from an index and a group set of it: the launch view, the set's tables, L, the chunks and the L2 share (the queries and
// rep are the sub-batch's).  Context mutex held by the caller
int check_group_index(const bbq_index *ix);
GroupScoreArgs group_score_args(bbq_index *ix, const bbq_groups *gs);
// ---- bbq_maxsim.cpp: the token block [t0, t0 + kMaxSimTokenBlock) of the sub-batch of nq queries from query q0 of the call on, staged:
// a MaxSimQuery for every query s of the sub-batch that has the block and takes_part(s), in query order -> h_mq (*n_mq of them), and
// its token vectors behind one another as queries of a score pass -> h_qdata (qb bytes each) / h_qparams.  Returns the vectors staged
struct MaxSimTokens { const int64_t *voff; const uint8_t *qquant; const double *qcorr; int planes, one_bit, sim; };  // of the call
int32_t stage_maxsim_token_block(const bbq_index *ix, const MaxSimTokens &tk, int64_t q0, int nq, int64_t t0, const std::function<bool(int)> &takes_part,
                                 uint8_t *h_qdata, size_t qb, QueryParams *h_qparams, MaxSimQuery *h_mq, int *n_mq);
// ---- bbq_maxsim_groups.cpp: the checks of a MaxSim call's token offsets and candidate lists, in the wording of `fn`, and the records
// of a sub-batch's lists.  check_maxsim_cand_lists: every group of every list is a live group of gs, the first offender named, at most
// kMaxSimCandMaxRows expanded rows a query; *longest = the longest list.  stage_maxsim_cand_records: coff = the sub-batch's first query's
// entry of the call's offsets; one record per candidate and a terminator per query -> h_rec, the queries -> h_cq; returns the most
// expanded rows of any query
int check_maxsim_vec_offsets(const char *fn, int32_t n_queries, const int64_t *vec_offsets);
int check_maxsim_cand_offsets(const char *fn, int32_t n_queries, const int64_t *cand_offsets);
int check_maxsim_cand_lists(const char *fn, const bbq_groups *gs, int32_t n_queries, const int64_t *coff, const int32_t *cand, int64_t *longest);
int64_t stage_maxsim_cand_records(const bbq_groups *gs, int nq, const int64_t *coff, const int32_t *cand, MaxSimCandQuery *h_cq, MaxSimCand *h_rec);
// ---- bbq_rerank.cpp: a candidate's true score and its position in the candidate list; the two selectors of the rerank recipes
struct Ranked { double score; int32_t pos; };
void rerank_select(int32_t selector, int64_t k, const double *t, int64_t cnt, std::vector<Ranked> &r);
// ---- bbq_maxsim_rerank.cpp: bbq_rerank_maxsim_groups_batch behind its argument checks, under a scratch budget of scratch_mb MiB
int rerank_maxsim_groups(const char *fn, bbq_vectors *v, const bbq_groups *gs, int32_t n_queries, const int64_t *voff, const float *queries, int32_t true_sim,
                         const int64_t *coff, const int32_t *cand, double *out, int scratch_mb);
// ---- bbq_dense.cpp
int dense_search_one(const SearchCall &c, int64_t qi, int32_t *out_idx, float *out_score, int64_t *out_n);

}  // namespace bbq
#pragma GCC visibility pop
