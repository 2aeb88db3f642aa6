// bbq_select.cpp - the tail of a sub-batch of the span search (plain and filtered, bbq_span.cpp), the grouped search (bbq_group.cpp)
// and the MaxSim search (bbq_maxsim.cpp): what the device selected, what the host must replay.  The decision about one answer block
// is prove_selected and the heap is HeapReplay (both bbq_replay.cpp, host only); the copies and the waits are here.
#include "bbq_search.h"

using namespace bbq;

int bbq::finish_selected(const SelectTail &t, const RowWalk &walk) {
  const int64_t k = t.k;
  // what the device selected: exactly k above the cut and no NaN - sorted by descending score; two equal scores among them, or one
  // equal to the cut, and the heap's history decides: replayed like the queries the device did not select for
  std::vector<int64_t> replay;  // the queries of the sub-batch whose heap the host replays
  std::vector<uint64_t> ent;
  int64_t n_scores = 0, replay_rows = 0;
  for (int s = 0; s < t.nq; ++s) {
    const SelectQuery &q = t.queries[s];
    n_scores += q.len;
    if (q.len == 0) {
      t.out_n[s] = 0;
      if (t.out_status) t.out_status[s] = 0;
      continue;
    }
    const bool proven = q.block >= 0 && prove_selected(t.back + (size_t)q.block * t.out_stride, k, ent);
    if (proven) {
      unpack_entries(ent.data(), k, t.out_tag + s * k, t.out_score + s * k);
      t.out_n[s] = k;
    } else {
      replay.push_back(s);
      replay_rows += q.len;
    }
    if (t.out_status) t.out_status[s] = proven ? 0 : 1;
  }
  if (replay.empty()) return BBQ_OK;

  // the reference loop (src/binaryQuantizationFormat.ts:383-411) over the query's rows in visiting order: the literal heap of min(k, rows)
  // (their scores - and ords - come back query by query, or in one copy where they are at least half of the sub-batch's: a filter
  // that leaves a query no more than k rows does so for most queries of a call, and a copy costs more than its few hundred bytes)
  auto bring_back = [&](int64_t first, int64_t rows) {
    hipError_t e = hipMemcpyAsync(t.h_scores + first, t.d_scores + first, (size_t)rows * 4, hipMemcpyDeviceToHost, t.stream);
    if (e == hipSuccess && t.d_ords) e = hipMemcpyAsync(t.h_ords + first, t.d_ords + first, (size_t)rows * 4, hipMemcpyDeviceToHost, t.stream);
    return e;
  };
  if (2 * replay_rows >= n_scores) {
    HIPCHK(bring_back(0, n_scores));
  } else {
    for (int64_t s : replay) HIPCHK(bring_back(t.queries[s].first, t.queries[s].len));
  }
  HIPCHK(hipStreamSynchronize(t.stream));
  for_each_index(replay_rows < 4096 ? 1 : t.threads, (int64_t)replay.size(), [&](int64_t i) {
    const int64_t s = replay[(size_t)i];
    const SelectQuery &q = t.queries[s];
    const float *sc = t.h_scores + q.first;
    HeapReplay hr(k, q.len);
    if (t.d_ords) {  // the rows as the device wrote them: what it wrote is what is checked
      const uint32_t *od = t.h_ords + q.first;
      for (int64_t r = 0; r < q.len; ++r) hr.offer(sc[r], (int32_t)od[r]);
    } else {
      walk(s, sc, hr);
    }
    t.out_n[s] = hr.finish(t.out_tag + s * k, t.out_score + s * k);
  });
  return BBQ_OK;
}
