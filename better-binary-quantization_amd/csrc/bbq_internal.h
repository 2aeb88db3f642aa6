// bbq_internal.h - host-side internals of libbbq shared between translation units
#pragma once
#include <stdint.h>
#include <algorithm>
#include <string>
#include <thread>
#include <vector>
#include "../../include/bbq.h"
#include "bbq_entry.h"

namespace bbq {

int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
void clear_error();

// Exact replay of the reference's top-k loop (src/binaryQuantizationFormat.ts:383-411, src/minHeap.ts:9-130).
// Feed rows in ascending global row order; rows that are skipped must be rows that cannot change the
// reference heap (DESIGN.md "Exact top-k").
class HeapReplay {
 public:
  HeapReplay(int64_t k, int64_t n_total);
  inline void offer(float score, int32_t row) {
    const double s = (double)score;
    if ((int64_t)heap_.size() < k2_) {
      push(s, row);
    } else if (k2_ > 0 && s > heap_[0].score) {
      pop();
      push(s, row);
    }
  }
  // pops everything (ascending) and writes it reversed = descending, like topKResults.reverse()
  int64_t finish(int32_t *out_idx, float *out_score);
  // the same heap keyed by an f64 (the rerank selector's trueScore, src/topKSelector.ts:40-66); drain pops ascending
  inline void offer64(double s, int32_t tag) {
    if ((int64_t)heap_.size() < k2_) {
      push(s, tag);
    } else if (k2_ > 0 && s > heap_[0].score) {
      pop();
      push(s, tag);
    }
  }
  int64_t drain_ascending(int32_t *out_tag, double *out_score);
  int64_t mutations() const { return mutations_; }

 private:
  struct Item { double score; int32_t index; };
  void push(double s, int32_t row);
  Item pop();
  std::vector<Item> heap_;
  int64_t k2_;
  int64_t mutations_ = 0;
};

// fn(i) for every i of [0, n) on at most T threads, thread t taking t, t + T, ...; T <= 1 or n <= 1: on the calling thread.  What the
// calls write must be disjoint - then how the indices are dealt changes no result.  When threads pay is the caller's decision.
template <class Fn>
void for_each_index(int64_t T, int64_t n, Fn fn) {
  T = std::min(T, n);
  if (T <= 1) {
    for (int64_t i = 0; i < n; ++i) fn(i);
    return;
  }
  std::vector<std::thread> th;
  for (int64_t t = 0; t < T; ++t)
    th.emplace_back([=] { for (int64_t i = t; i < n; i += T) fn(i); });
  for (std::thread &x : th) x.join();
}

// One answer block of the select pass (SpanSelectArgs::out, bbq_device.h): {scores above the cut | NaN seen << 32}, the cut's f32 bits,
// then the entries.  Proven - the reference's heap returns exactly these k, by descending score - when there are exactly k above the cut,
// no NaN, no two of them score equal and the k-th does not equal the cut; otherwise the heap's history decides and the caller replays
// it.  ent: the k entries by descending score when proven, scratch otherwise.
bool prove_selected(const uint64_t *blk, int64_t k, std::vector<uint64_t> &ent);

// The reference loop (src/binaryQuantizationFormat.ts:383-411) over each of n_lists lists IN THE ORDER GIVEN: the literal heap of
// min(k, length) over (scores[i], tags[i]), i in [offsets[q], offsets[q + 1]) -> out_tag / out_score [q][k], out_n[q].  An empty list
// or k == 0 answers 0.  On `threads` threads once the lists hold 4096 entries.
void replay_lists(int32_t n_lists, const int64_t *offsets, const int32_t *tags, const float *scores, int64_t k, int threads, int32_t *out_tag,
                  float *out_score, int64_t *out_n);

}  // namespace bbq
