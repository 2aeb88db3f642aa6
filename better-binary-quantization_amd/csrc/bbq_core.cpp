// bbq_core.cpp - segment plan, slot workspace, pipelined search (enqueue, collection, host replay), C ABI (see include/bbq.h).
//
// Search of one query = a short sequence of launches over row SEGMENTS of the index:
//   segment 0   rows [0, s0)           dense: every f32 score is written; the finalize kernel lists all of
//                                      them (the reference heap is still filling / changing fast here) and
//                                      selects theta_1 = k-th largest key
//   segment j   rows [b_j, b_{j+1})    sparse: rows with key > theta_j go to per-chunk candidate slots; the
//                                      finalize kernel compacts them into the list and selects theta_{j+1}
// theta_j only depends on rows before b_j, so it is a lower bound of the reference heap's minimum while the
// reference walks segment j: rows at or below it can never enter the heap (bbq_replay.cpp).
// Queries are processed in sub-batches (grid.y = queries, each query sweeps the index on its own), and
// sub-batches are pipelined over NSLOT streams so the host replay of one overlaps the scan of the next.
#include <math.h>
#include <string.h>
#include <memory>
#include "bbq_search.h"
#include "bbq_workqueue.h"

using namespace bbq;

namespace {

// Host worker pool for the heap replays: persistent threads (spawning per sub-batch cost more than the replay itself
// once sweeps are shared), fed while the device already works on the next sub-batches.
WorkQueue &replay_pool() {
  static WorkQueue *p = new WorkQueue();  // intentionally never destroyed: workers may outlive static destructors
  return *p;
}

// Raw queries of bbq_search_raw_batch being quantized on host threads, chunk by chunk, while the sub-batches in front are already
// on the device: the quantizer (~15 us per 768-d query and core) never stands in front of a sweep except for the first chunk.
struct RawFeed {
  const float *queries = nullptr, *centroid = nullptr;
  int32_t n = 0, dim = 0, sim = 0, qb = 0, iters = 0, chunk = 8;  // small chunks: the first sub-batch waits for its own queries only (8 x ~15 us)
  double lambda = 0;
  uint8_t *qq = nullptr;
  double *qc = nullptr;
  std::unique_ptr<std::atomic<int>[]> ready;  // per chunk: 0 pending, 1 done, 2 failed
  std::atomic<int> next{0};
  std::vector<std::thread> threads;
  int n_chunks() const { return (n + chunk - 1) / chunk; }
  void start(int n_threads) {
    ready.reset(new std::atomic<int>[(size_t)n_chunks()]);
    for (int i = 0; i < n_chunks(); ++i) ready[(size_t)i].store(0);
    const int T = std::max(1, std::min(n_threads, n_chunks()));
    auto work = [this] {
      for (;;) {
        const int ci = next.fetch_add(1);
        if (ci >= n_chunks()) return;
        int state = 1;
        for (int i = ci * chunk; i < std::min(n, (ci + 1) * chunk); ++i)
          if (bbq_quantize_query(queries + (size_t)i * dim, dim, centroid, sim, qb, lambda, iters, qq + (size_t)i * dim, qc + (size_t)i * 4) != BBQ_OK) {
            state = 2;
            break;
          }
        ready[(size_t)ci].store(state, std::memory_order_release);
      }
    };
    for (int t = 0; t < T; ++t) threads.emplace_back(work);
  }
  // blocks until queries [first, first + count) are quantized; on a failed query returns its index through *bad
  int wait(int64_t first, int count, int32_t *bad) {
    for (int ci = (int)(first / chunk); ci <= (int)((first + count - 1) / chunk); ++ci) {
      int st;
      while ((st = ready[(size_t)ci].load(std::memory_order_acquire)) == 0) std::this_thread::yield();
      if (st == 2) {
        // which query, and its message on THIS thread (the worker's is thread-local)
        for (int i = ci * chunk; i < std::min(n, (ci + 1) * chunk); ++i) {
          const int rc = bbq_quantize_query(queries + (size_t)i * dim, dim, centroid, sim, qb, lambda, iters, qq + (size_t)i * dim, qc + (size_t)i * 4);
          if (rc != BBQ_OK) { if (bad) *bad = i; return rc; }
        }
        return fail(BBQ_ERR_INVALID_ARG, "query quantization failed");
      }
    }
    return BBQ_OK;
  }
  void join() {
    next.store(1 << 30);
    for (auto &t : threads) t.join();
    threads.clear();
  }
  ~RawFeed() { join(); }
};

}  // namespace

namespace bbq {

// queries per launch sequence (sub-batch).  The largest sweep of a sub-batch should run for about a millisecond: shorter ones pay the
// device's dependent-launch gaps and their own ramp (1.25 M rows x 2048 queries: 52.5 K q/s with 32 per sub-batch, 56.5 K with 64,
// 57 K with 96-128; at 10 M rows 32 is as good as 64 and needs half the workspace - also with the launch's queries co-scheduled per chunk,
// l2_share_shift() below, where the sweep is bound by vector issue: 11.20-11.21 K q/s with 32, 11.33-11.34 K with 64).  A call should also be cut into at least four
// sub-batches where it can: the first sub-batch's small segments run alone on the device and only the later ones hide theirs behind
// another sub-batch's large sweep (1 M rows x 256 queries per call: 0.849 of the roofline end to end with 2 x 128, 0.855 with 4 x 64)
int effective_batch(const bbq_index *ix, int64_t n_queries) {
  if (ix->opt_batch > 0) return ix->opt_batch;
  const int64_t rows = ix->main.view.n_rows;
  int q = rows >= 6000000 ? 32 : rows >= 2500000 ? 64 : 128;
  while (n_queries > 0 && q > 32 && n_queries < 4 * (int64_t)q) q >>= 1;
  // the sweep on the matrix cores serves two groups of 32 queries per tile load (bbq_mfma_kernels.hip): 64 queries per launch chain
  if (ix->opt_share == 32 && q < 64 && (n_queries == 0 || n_queries > 32)) q = 64;
  return q;
}

// queries co-scheduled per chunk in a per-query sparse sweep (option l2_share; the launch caps it by its query count).  An explicit value
// is taken as it is.  Automatic: kL2ShareAuto - except with resident_mb 0, the "no reuse across queries" mode that bench.py's strict
// roofline figure is measured in: there every byte of every sweep has to come from HBM, so the launch keeps the plain order, in which
// two queries' reads of a chunk lie a whole sweep apart.  Measured at 10 M x 768, 256 queries per call, 32 per launch, one box, alternating
// (K q/s): 1: 7.60-7.61, 2: 9.07-9.11, 4: 10.22-10.27, 8: 10.76-10.77, 16: 11.01-11.03, 32: 11.20-11.21 - as many as a launch has.
constexpr int kL2ShareAuto = 32;
int l2_share_shift(const bbq_index *ix) {
  int p = ix->opt_l2_share;
  if (p < 0) p = ix->opt_resident_mb == 0 ? 1 : kL2ShareAuto;
  int s = 0;
  while ((1 << (s + 1)) <= p) ++s;
  return s;
}

// whether a per-query sparse sweep reads a row's component sum from the row_sums side array (where the storage has one) instead of counting
// it (option row_sums).  An explicit 0 or 1 is taken as it is.  Automatic: yes - except with resident_mb 0, where every byte of every sweep
// comes from HBM: there 2 B/row more cost time and the count is free, and the launch stays the one it was.
bool row_sums_for_launch(const bbq_index *ix) { return ix->opt_row_sums < 0 ? ix->opt_resident_mb != 0 : ix->opt_row_sums != 0; }

// whether a call stages the digit masks of its queries next to their bit-planes (option digit_planes; 1 and -1 are the same): a 4-plane
// query against 1-bit rows whose sparse sweeps read the row sums.  The launch takes the digit twin where both are there and the twin
// exists (launch_scan_t); with resident_mb 0 the automatic row_sums is off and the launch stays the one it was.
bool digit_planes_for_call(const bbq_index *ix, int planes) {
  return ix->opt_digit_planes != 0 && ix->geom.store_bits == 1 && planes == 4 && row_sums_for_launch(ix) && row_sums_fit(ix->geom);
}

// tiles a wave of a per-query sparse sweep takes one after the other (option tiles_per_wave; the launch ignores it wherever it has no such
// twin, launch_scan_t).  An explicit 1, 2, 4 or 8 is taken as it is.  Automatic: per row width, the fastest value that passed BOTH tests -
// its twin comes out of the compiler without scratch and with no fewer waves per SIMD than the one-tile kernel (scripts/scan_resources.py),
// and its slowest run was faster than the parent's fastest by more than the parent's own spread (Measurement) - and 1 where
// none did.  With the exact path behind the tile loop (sweep_deferred_exact) and the tile loop's loads through buffer descriptors
// (sweep_wave_tiles, bbq_scan_body.h) every twin holds 88-90 scalar registers and:
// 768-d: 8 (50 vector registers, 8 waves like the one-tile kernel; 2 and 4 tiles: 51, 8 waves, measured slower).  1024-d: 8 (58
// registers, 8 waves like the one-tile kernel, 1.6 % above 4 tiles' fastest run, 5 x their spread; 2 and 4 tiles: 59 / 8).
// 1536-d: 1 - every twin reports 6 waves against the one-tile kernel's 7 (75 / 75 / 74 registers against 68) although each was
// measured faster: docs/dropped.md, "tiles per wave".
int tiles_per_wave_for(const bbq_index *ix) {
  if (ix->opt_tiles_per_wave > 0) return ix->opt_tiles_per_wave;
  switch (ix->geom.w16) {
    case 6: return 8;
    case 8: return 8;
    default: return 1;
  }
}

// ------------------------------------------------------------------------------------------------ plan

static int cap_for(int64_t k, int64_t rows_before) {
  const double lam = (double)k * kChunkRows / (double)std::max<int64_t>(rows_before, 1);
  int64_t c = (int64_t)ceil(lam + 8.0 * sqrt(lam) + 16.0);
  c = (c + 7) / 8 * 8;
  return (int)std::min<int64_t>(std::max<int64_t>(c, 16), kChunkRows);
}

// have_theta: a threshold derived from earlier rows (the pilot replica) already exists when this storage starts;
// otherwise the storage's own first rows form the dense segment (for a shard without a replica that gives
// thresholds from the shard's local prefix: weaker than global ones, still valid)
static void add_storage_segments(const bbq_index *ix, Plan &p, int storage, const Storage &st, int64_t rows_before, bool have_theta,
                          bool emit, double &expected) {
  const int64_t R = st.view.n_rows;
  if (R <= 0) return;
  int64_t b = 0;
  if (!have_theta) {
    rows_before = 0;
    const int64_t rows = std::min(p.s0, R);
    p.segs.push_back(Segment{storage, 0, (rows + kChunkRows - 1) / kChunkRows, rows, true, emit, true, false, 0});
    expected += (double)rows;
    b = rows;
  }
  while (b < R) {
    // the threshold of a segment comes from every row seen before it (pilot replica + this storage's earlier
    // segments); the next boundary multiplies that count by `growth`, so every segment emits ~k*(growth-1) candidates
    const int64_t before = rows_before + b;
    int64_t e = R;
    const int64_t nb = (before * p.growth - rows_before) / kChunkRows * kChunkRows;
    if (before > 0 && nb > b && nb <= R / 2) e = nb;
    const int cap = cap_for(p.k, before);
    const int64_t rows = e - b;
    p.segs.push_back(Segment{storage, b / kChunkRows, (rows + kChunkRows - 1) / kChunkRows, rows, false, emit, true, false, cap});
    expected += (double)p.k * (double)rows / (double)before;
    b = e;
  }
}

// what a plan is built from before its segments: the ranks, the growth and the size of the first segment
static Plan start_plan(const bbq_index *ix, int64_t k, int64_t final_k, bool latency) {
  Plan p;
  p.k = k;
  p.final_k = final_k;
  p.growth = latency ? ix->opt_latency_growth : ix->opt_growth;
  p.latency = latency;
  p.s0 = std::max<int64_t>(ix->opt_s0, (4 * k + kChunkRows - 1) / kChunkRows * kChunkRows);
  p.s0 = std::min<int64_t>(p.s0, 8192);
  return p;
}

// ... and what follows from its segments: the workspace sizes, the dominant and the big sweeps, the list and flood capacities.
// listed_whole: rows that are listed whatever they score (the first segment); expected_emit: those + the expected sparse candidates
static void size_plan(const bbq_index *ix, Plan &p, int64_t listed_whole, double expected_emit) {
  if (!p.segs.empty()) p.segs.back().need_theta = false;
  int64_t best = -1;
  for (size_t i = 0; i < p.segs.size(); ++i) {
    Segment &s = p.segs[i];
    if (!s.dense) {
      p.max_slots = std::max(p.max_slots, s.n_chunks * (int64_t)s.cap);
      p.max_chunks = std::max(p.max_chunks, s.n_chunks);
    }
    if (best < 0 || s.rows > p.segs[best].rows) best = (int64_t)i;
  }
  if (best >= 0) p.segs[best].dominant = true;
  for (Segment &sg : p.segs) sg.big = best >= 0 && sg.rows * 32 >= p.segs[best].rows && sg.rows >= 65536;
  // list capacity: everything listed whole + 4x the expected sparse candidates + slack
  const double sparse = std::max(0.0, expected_emit - (double)listed_whole);
  p.list_cap = listed_whole + (int64_t)(4.0 * sparse) + 4096;
  p.list_cap = (p.list_cap + 1023) / 1024 * 1024;
  // per query; bounded so that the overflow areas of one pipeline slot stay within 512 MB however many queries a sub-batch has
  p.flood_cap = std::min<int64_t>(ix->opt_flood, (ix->main.view.n_rows + 1023) / 1024 * 1024);
  if (p.flood_cap > 0)
    p.flood_cap = std::min<int64_t>(p.flood_cap, std::max<int64_t>(16384, ((64ll << 20) / std::max(32, effective_batch(ix))) / 1024 * 1024));
}

// k: the rank the device selects thresholds with; final_k > 0: k == final_k + 1 and the last finalize launch selects the answer.
// A value of its inputs and the index's options: the call that asked for it owns it.
Plan build_plan(const bbq_index *ix, int64_t k, int64_t final_k, bool latency) {
  Plan p = start_plan(ix, k, final_k, latency);
  double expected_emit = 0, dummy = 0;
  if (ix->has_pilot) {
    add_storage_segments(ix, p, 0, ix->pilot, 0, false, false, dummy);
    add_storage_segments(ix, p, 1, ix->main, ix->pilot.view.n_rows, true, true, expected_emit);
  } else {
    add_storage_segments(ix, p, 1, ix->main, 0, false, true, expected_emit);
  }
  int64_t dense_rows = 0;
  for (const Segment &s : p.segs)
    if (s.emit && s.dense) dense_rows += s.rows;
  size_plan(ix, p, dense_rows, expected_emit);
  return p;
}

// The plan of a filtered call lives in ACCEPTED-ROW space: a threshold is an order statistic over the accepted rows seen so far and only
// tightens at a segment boundary, so the boundaries are set by accepted rows seen (the filter's cumulative counts per chunk), not by
// rows swept - cut by rows, a filter whose rows cluster at the end of the index would meet them all in one last segment with a
// threshold from next to nothing.  The sweep starts at the first chunk with an accepted row and stops after the last; the first
// segment ends where s0 accepted rows have been seen, every later boundary where the accepted count has grown `growth`-fold (while
// that is within half of |A|, the unfiltered plan's R/2 rule).  The first segment runs SPARSE with the zeroed threshold (every key of
// a non-NaN score is > 0, bbq_entry.h): a dense first segment would bring rejected rows into the running top keys.  Expected
// candidates per chunk are k * accepted_in_chunk / accepted_before <= k * kChunkRows / accepted_before: cap_for carries over with
// that substitution, and no chunk can list more than the accepted rows it holds.
Plan build_filtered_plan(const bbq_index *ix, const bbq_filter &f, int64_t k, int64_t final_k, bool latency) {
  Plan p = start_plan(ix, k, final_k, latency);
  if (f.count == 0) return p;
  const std::vector<int32_t> &cum = f.cum;
  const int64_t end = f.last_chunk + 1, R = ix->main.view.n_rows;
  // the first chunk boundary at which `acc` accepted rows have been seen
  auto chunk_where = [&cum](int64_t acc) { return (int64_t)(std::lower_bound(cum.begin(), cum.end(), acc) - cum.begin()); };
  auto add = [&](int64_t b, int64_t e, int cap_bound) {
    int32_t most = 0;
    for (int64_t c = b; c < e; ++c) most = std::max(most, cum[(size_t)c + 1] - cum[(size_t)c]);
    const int cap = std::min(cap_bound, std::max(16, (most + 7) / 8 * 8));
    p.segs.push_back(Segment{1, b, e - b, std::min(e * kChunkRows, R) - b * kChunkRows, false, true, true, false, cap});
  };
  int64_t b = f.first_chunk;
  int64_t e = std::min(std::max(chunk_where(p.s0), b + 1), end);
  add(b, e, kChunkRows);
  const int64_t first_listed = cum[(size_t)e];
  double expected_emit = (double)first_listed;
  for (b = e; b < end; b = e) {
    const int64_t before = cum[(size_t)b];
    const int64_t nb = chunk_where(before * p.growth);
    e = (nb > b && nb < end && cum[(size_t)nb] <= f.count / 2) ? nb : end;
    add(b, e, cap_for(p.k, before));
    expected_emit += (double)p.k * (double)(cum[(size_t)e] - before) / (double)before;
  }
  size_plan(ix, p, first_listed, expected_emit);
  return p;
}

// ------------------------------------------------------------------------------------------------ slots

static int64_t qbuf_bytes_per_query(const bbq_index *ix) { return qbuf_bytes_per_query_w(ix->geom.w16); }

int ensure_slot(const SearchCall &c, Slot &s, int nq, bool own_lists) {
  const bbq_index *ix = c.ix;
  const Plan &p = *c.plan;
  const int64_t qb = qbuf_bytes_per_query(ix);
  const int64_t hprefix = std::min<int64_t>(p.list_cap, 16384);
  const bool ok = s.q_cap >= nq && s.qbuf_bytes >= qb && s.chunks_cap >= p.max_chunks && s.slots_cap >= p.max_slots &&
                  s.dense_cap >= p.s0 && s.list_cap >= p.list_cap + (own_lists ? p.flood_cap : 0) && s.k_cap >= p.k && s.hprefix >= hprefix &&
                  s.flood_cap >= p.flood_cap && s.final_stride >= p.final_k + 2 &&
                  (!own_lists || s.d_lists != nullptr);
  if (ok) return BBQ_OK;
  // grow-only in every dimension: a process that alternates between call shapes (single queries use another segment plan than
  // batches, k varies) would otherwise free and allocate the workspace at every switch - each time sized for the plan at hand and
  // therefore too small for the other one (milliseconds per switch).  Every buffer grows on its own: one that is large enough stays
  own_lists = own_lists || s.d_lists != nullptr;
  const int Q = std::max((std::max(nq, effective_batch(ix)) + 31) / 32 * 32, s.q_cap);  // multiple of 32: the MFMA query layout is per group of 32
  const bool valid = s.q_cap > 0;
  s.q_cap = 0;  // the capacities below describe the buffers only once all of them are in place: a call after a failure grows again
  s.qbuf_bytes = std::max(s.qbuf_bytes, qb);
  s.chunks_cap = std::max<int64_t>(s.chunks_cap, std::max<int64_t>(p.max_chunks, 1));
  s.slots_cap = std::max<int64_t>(s.slots_cap, std::max<int64_t>(p.max_slots, 1));
  s.dense_cap = std::max<int64_t>(s.dense_cap, p.s0);
  s.flood_cap = std::max<int64_t>(s.flood_cap, p.flood_cap);
  s.list_cap = std::max<int64_t>(s.list_cap, p.list_cap + (own_lists ? s.flood_cap : 0));  // own lists can take a flood; external ones are the caller's size
  s.k_cap = std::max<int64_t>(s.k_cap, std::max<int64_t>(p.k, 1));
  s.hprefix = std::max<int64_t>(s.hprefix, hprefix);
  s.final_stride = std::max<int64_t>(s.final_stride, std::max<int64_t>(p.final_k, 126) + 2);
  // theta | flags | topk_counts | list_counts | ovf_counts | append_counts live in one control block in front of the staged queries: the copy that
  // brings a sub-batch's queries also resets them (the host twin's control part stays zero)
  const int64_t ctrl_bytes = ((int64_t)Q * (28 + 4 * kAppendStride) + 255) / 256 * 256;  // the append counters sit one per 128-byte line (kAppendStride)
  const size_t block = (size_t)(ctrl_bytes + Q * s.qbuf_bytes);
  if (!valid || s.d_block.size() < block) {  // (the control layout depends on Q alone, and a larger Q is a larger block)
    s.ctrl_bytes = ctrl_bytes;
    HIPCHK(s.d_block.alloc(block));
    s.ctrl_clean = false;
    HIPCHK(s.h_block.alloc(block));
    memset(s.h_block, 0, (size_t)s.ctrl_bytes);
    s.d_qbuf = s.d_block + s.ctrl_bytes;
    s.h_qbuf = s.h_block + s.ctrl_bytes;
    // (all-zero bytes are the reset state of every one of them: a zeroed Threshold is {key 0, z image -inf}, bbq_device.h)
    s.d_theta = reinterpret_cast<Threshold *>(s.d_block.get());
    uint32_t *words = reinterpret_cast<uint32_t *>(s.d_block.get());
    s.d_flags = words + 2 * (size_t)Q;
    s.d_topk_counts = reinterpret_cast<int32_t *>(words + 3 * (size_t)Q);
    s.d_list_counts = reinterpret_cast<int32_t *>(words + 4 * (size_t)Q);
    s.d_ovf_counts = words + 6 * (size_t)Q;
    s.d_append_counts = words + 7 * (size_t)Q;
  }
  if (s.flood_cap > 0) HIPCHK(s.d_ovf.reserve((size_t)(Q * s.flood_cap)));
  HIPCHK(s.d_counts.reserve((size_t)(Q * s.chunks_cap)));
  HIPCHK(s.d_topk.reserve((size_t)(Q * s.k_cap)));
  HIPCHK(s.h_list_counts.reserve((size_t)Q * 2));
  HIPCHK(s.d_entries.reserve((size_t)(Q * s.slots_cap)));
  HIPCHK(s.d_dense0.reserve((size_t)(Q * s.dense_cap)));
  if (own_lists) {
    HIPCHK(s.d_lists.reserve((size_t)(Q * s.list_cap)));
    HIPCHK(s.h_lists.reserve((size_t)(Q * s.hprefix)));
  }
  HIPCHK(s.d_final.reserve((size_t)(Q * s.final_stride)));
  HIPCHK(s.h_final.reserve((size_t)(Q * s.final_stride)));
  s.q_cap = Q;
  return BBQ_OK;
}

// ------------------------------------------------------------------------------------------------ enqueue / complete

// the FinalizeArgs fields every finalize launch takes from its slot: the query lists (a sharded scan's are the caller's), their
// counters (the append counters only behind a sweep that appended), the running top-k keys, the threshold, the flags and the rank
FinalizeArgs slot_finalize_args(const Slot &s, uint64_t *lists, int32_t *list_counts, int64_t list_cap, bool appended, int64_t k) {
  FinalizeArgs f{};
  f.append_counts = appended ? s.d_append_counts : nullptr;
  f.lists = lists;
  f.list_counts = list_counts;
  f.list_cap = list_cap;
  f.topk_keys = s.d_topk;
  f.topk_counts = s.d_topk_counts;
  f.theta = s.d_theta;
  f.flags = s.d_flags;
  f.k = (int32_t)k;
  return f;
}

// the ScanArgs of segment g for the slot's sub-batch of nq queries (the caller adds the append mode)
static ScanArgs segment_scan_args(const Plan &p, const Slot &s, const Segment &g, const Storage &sto, const IndexView &view, int nq, int64_t qb) {
  ScanArgs a{};
  a.idx = view;
  a.qplanes = reinterpret_cast<const uint4 *>(s.d_qbuf);
  a.qparams = reinterpret_cast<const QueryParams *>(s.d_qbuf + (size_t)nq * qb);
  a.chunk_begin = g.chunk_begin;
  a.row_id_base = sto.row_id_base;
  a.theta = s.d_theta;
  a.counts = s.d_counts;
  a.entries = s.d_entries;
  a.flags = s.d_flags;
  a.cap = g.cap;
  a.n_chunks = (int32_t)g.n_chunks;
  // the slot's area may be larger than this plan asks for (slots are shared and grow-only): the plan's size governs
  a.ovf = p.flood_cap > 0 ? s.d_ovf : nullptr;
  a.ovf_counts = s.d_ovf_counts;
  a.ovf_cap = (int32_t)p.flood_cap;
  a.dense_score32 = g.dense ? s.d_dense0 : nullptr;
  a.dense_stride = s.dense_cap;
  return a;
}

// ... and of the finalize launch behind that sweep (the caller adds where a last segment leaves its answer)
static FinalizeArgs segment_finalize_args(FinalizeArgs f, const Slot &s, const Segment &g, const ScanArgs &a) {
  f.counts = s.d_counts;
  f.entries = s.d_entries;
  f.dense_score32 = s.d_dense0;
  f.dense_stride = s.dense_cap;
  f.dense_rows = g.dense ? (int32_t)g.rows : 0;
  f.dense_row_id_base = a.row_id_base + g.chunk_begin * kChunkRows;
  f.n_chunks = (int32_t)g.n_chunks;
  f.cap = g.cap;
  f.ovf = a.ovf;
  f.ovf_cap = a.ovf_cap;
  f.emit = g.emit ? 1 : 0;
  f.need_theta = g.need_theta ? 1 : 0;
  return f;
}

int enqueue_subbatch(const SearchCall &c, Slot &s, int64_t q_first, int nq, const ExtOut *ext) {
  bbq_index *ix = c.ix;
  const Plan &p = *c.plan;
  const int64_t qb = query_data_bytes(ix, c.planes);
  QueryParams *hq = reinterpret_cast<QueryParams *>(s.h_qbuf + (size_t)nq * qb);
  for (int i = 0; i < nq; ++i)
    fill_query(ix, s.h_qbuf + (size_t)i * qb, hq + i, c.qquant + (size_t)(q_first + i) * ix->geom.dim, c.qcorr + (size_t)(q_first + i) * 4,
               c.planes, c.one_bit, c.sim);
  size_t bytes = (size_t)nq * qb + (size_t)nq * sizeof(QueryParams);
  // the matrix-core shared sweep appends its candidates to the lists, so it runs only where they are this slot's own
  // (a filtered call with sweep_share 32 as well: its kernels take the filter's accept words)
  bool use_mfma = !ext && c.share == 32 && c.maxq <= 127 && ix->geom.store_bits == 1;
  for (int i = 0; i < nq && use_mfma; ++i) use_mfma = mfma_query_ok(hq[i]);
  const MfmaStage ms = use_mfma ? stage_queries_mfma(c, s.h_qbuf, hq, q_first, nq, bytes) : MfmaStage{};
  if (use_mfma) bytes = ms.bytes;
  // the digit masks of a 4-plane query behind everything else: the per-query sparse sweeps take them where they have a digit twin
  int32_t qdigits_at = 0;  // in 16-byte units behind the planes (ScanArgs::qdigits_at)
  // (only where every sparse segment is a per-query sweep: a call with sweep_share 4 / 8 sweeps shared, and a segment of it that falls
  // back to the per-query sweep runs planes)
  if (!use_mfma && c.share == 1 && digit_planes_for_call(ix, c.planes)) {
    const size_t db = (size_t)digit_bytes_per_query_w(ix->geom.w16);
    for (int i = 0; i < nq; ++i) fill_query_digits(ix, s.h_qbuf + bytes + (size_t)i * db, hq + i, c.qquant + (size_t)(q_first + i) * ix->geom.dim);
    qdigits_at = (int32_t)(bytes / 16);
    bytes += (size_t)nq * db;
  }
  hipStream_t st = s.stream;
  HIPCHK(hipMemcpyAsync(s.d_block, s.h_block, (size_t)s.ctrl_bytes + bytes, hipMemcpyHostToDevice, st));  // control words := 0, queries
  s.ctrl_clean = false;
  uint64_t *d_lists = ext ? ext->lists : s.d_lists.get();
  const int64_t list_cap = ext ? ext->list_cap : s.list_cap;
  int32_t *d_list_counts = ext ? ext->counts : s.d_list_counts;
  if (ext) HIPCHK(hipMemsetAsync(ext->counts, 0, (size_t)nq * 8, st));
  // a shard without rows (and without a pilot replica) launches nothing that would write its answer blocks: all-zero blocks say
  // "nothing listed, no cut, no flags", which is what bbq_merge_answers expects of such a shard
  if (ext && ext->answers && p.segs.empty())
    HIPCHK(hipMemsetAsync(ext->answers, 0, ((size_t)(nq - 1) * (size_t)ext->answers_stride + (size_t)c.k_dev + 2) * 8, st));

  const bool use_final = !ext && p.final_k > 0 && !p.segs.empty();
  // few queries: the sparse launches append their candidates to the list themselves (ScanArgs::append_lists)
  const bool append = use_final && p.latency && !ix->has_pilot && c.share == 1;
  Slot::InFlight &fl = s.fl;
  fl.appended = append || use_mfma;
  fl.timed = false;
  int64_t resident = 0;  // of one query's sweep over all segments
  for (const Segment &g : p.segs) {
    const Storage &sto = g.storage == 0 ? ix->pilot : ix->main;
    const bool last = &g == &p.segs.back();
    const LaunchView lv = launch_view(ix, sto, g.chunk_begin, g.n_chunks);
    resident += lv.resident_bytes;
    ScanArgs a = segment_scan_args(p, s, g, sto, lv.view, nq, qb);
    a.l2_shift = l2_share_shift(ix);  // (read by the per-query sweep alone, and only by its sparse launches)
    a.idx.row_sums = row_sums_for_launch(ix) ? sto.view.row_sums : nullptr;  // (likewise; null where the storage has none)
    a.qdigits_at = qdigits_at;                                               // (likewise; 0: the plane form)
    const bool append_here = !g.dense && ((append && (ix->opt_append_last || !last)) || use_mfma);
    if (append_here) {
      a.append_lists = d_lists;
      a.append_base = d_list_counts;
      a.append_counts = s.d_append_counts;
      a.append_cap = list_cap;
    }
    // how this segment is swept, decided once: on the matrix cores, shared between c.share queries, or (neither) every query on its own
    // A filtered plan has no dense first segment: its first segment runs with the zeroed threshold, and the matrix-core kernel flags
    // a query without a usable threshold as overflowed.  So a filtered segment is swept there only behind k_dev accepted rows (the
    // finalize launches behind them have left a threshold of that rank); the others, always the first, stay on the per-query filtered
    // sweep, which appends to the same lists.
    const bool theta_ready = !c.filter || c.filter->cum[(size_t)g.chunk_begin] >= c.k_dev;
    const bool on_mfma = use_mfma && !g.dense && theta_ready && mfma_sweep_supported(a);
    const bool shared = !on_mfma && !g.dense && !c.filter && c.share > 1 && shared_sweep_supported(a, c.share);
    const int my_slot = (int)(&s - ix->slots);
    // one big sweep at a time on the device - for the memory-bound sweeps, which share the Infinity Cache's budget.  The chains of the
    // matrix-core sweep are issue-bound and run side by side: serialised, the finalize launch and the launch gaps between a chain's two
    // large sweeps were idle time (128 -> 138 K q/s at 10 M x 768)
    const bool chained = g.big && !on_mfma;
    if (chained && ix->ctx->last_big_slot >= 0 && ix->ctx->last_big_slot != my_slot)
      HIPCHK(hipStreamWaitEvent(st, ix->slots[ix->ctx->last_big_slot].ev_big, 0));
    if (g.dominant) HIPCHK(hipEventRecord(s.ev0, st));
    if (on_mfma && c.filter)
      HIPCHK(launch_scan_mfma_filtered(a, c.filter->d_bits, s.d_qbuf + ms.off_qbytes, reinterpret_cast<const float *>(s.d_qbuf + ms.off_qmax),
                                       ms.fp ? ms.scale8 / 8.0f : 0.0f, nq, (int)g.n_chunks, st));
    else if (on_mfma)
      HIPCHK(launch_scan_mfma(a, s.d_qbuf + ms.off_qbytes, reinterpret_cast<const float *>(s.d_qbuf + ms.off_qmax), ms.fp ? ms.scale8 / 8.0f : 0.0f, nq, (int)g.n_chunks, st));
    else if (shared)
      HIPCHK(launch_scan_shared(a, c.planes, c.share, nq, (int)g.n_chunks, st));
    else if (c.filter)  // (its plan has sparse segments only; sweep_share 4 / 8 never reach a filtered call, 32 falls back to here)
      HIPCHK(launch_scan_filtered(a, c.filter->d_bits, c.planes, nq, (int)g.n_chunks, st));
    else
      HIPCHK(launch_scan(a, c.planes, g.dense, nq, (int)g.n_chunks, st, c.share == 1 ? tiles_per_wave_for(ix) : 1));
    if (chained) {
      HIPCHK(hipEventRecord(s.ev_big, st));
      ix->ctx->last_big_slot = my_slot;
    }
    if (g.dominant) {
      HIPCHK(hipEventRecord(s.ev1, st));
      fl.timed = true;
      fl.timed_rows = g.rows * nq;
      // a shared sweep reads each row once for `share` queries
      const int share = on_mfma ? mfma_queries_per_tile_load(a, nq, ms.fp) : shared ? c.share : 1;
      // the matrix-core sweep reads the codes and the EXACT corrections (compact layout: 24 of the side array's 32 B per row instead of
      // the tile's 4-byte word), once per 32 queries
      const int64_t row_bytes = !on_mfma ? (int64_t)bytes_per_row_of(ix->geom)
                                : sto.view.geom.layout == kLayoutCompact ? (int64_t)sto.view.geom.w16 * 16 + 24 : (int64_t)sto.view.geom.tile_stride / kTileRows;
      fl.timed_bytes = g.rows * ((nq + share - 1) / share) * row_bytes;
    }
    FinalizeArgs f = segment_finalize_args(slot_finalize_args(s, d_lists, d_list_counts, list_cap, append_here, c.k_dev), s, g, a);
    f.qparams = a.qparams;  // the thresholds it writes carry their z images (store_threshold)
    if (last && p.final_k > 0 && (use_final || (ext && ext->answers))) {  // the answer: to the slot, or a shard's to its caller
      f.final_out = use_final ? s.d_final.get() : ext->answers;
      f.final_stride = (int32_t)(use_final ? s.final_stride : ext->answers_stride);
      f.final_k = (int32_t)p.final_k;
      f.final_shard = use_final ? 0 : 1;
    }
    HIPCHK(launch_finalize(f, nq, st));
  }
  ix->stats.resident_bytes = resident;
  fl.final_used = use_final;
  if (!ext) {
    if (use_final) {
      // the answer itself (header + k entries per query, one copy) instead of the candidate list: the list is fetched only for a
      // query whose answer the device could not prove (ties), see begin_replay
      if (nq == 1 || p.final_k + 2 == s.final_stride)
        HIPCHK(hipMemcpyAsync(s.h_final, s.d_final, ((size_t)(nq - 1) * s.final_stride + (size_t)p.final_k + 2) * 8, hipMemcpyDeviceToHost, st));
      else
        HIPCHK(hipMemcpy2DAsync(s.h_final, (size_t)s.final_stride * 8, s.d_final, (size_t)s.final_stride * 8, (size_t)(p.final_k + 2) * 8, (size_t)nq,
                                hipMemcpyDeviceToHost, st));
    } else {
      HIPCHK(hipMemcpyAsync(s.h_list_counts, s.d_list_counts, (size_t)nq * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpy2DAsync(s.h_lists, (size_t)s.hprefix * 8, s.d_lists, (size_t)s.list_cap * 8, (size_t)s.hprefix * 8, (size_t)nq,
                              hipMemcpyDeviceToHost, st));
    }
  }
  HIPCHK(hipEventRecord(s.ev_done, st));
  fl.busy = true;
  fl.nq = nq;
  fl.q_first = q_first;
  return BBQ_OK;
}

void account_timing(bbq_index *ix, Slot &s) {
  float ms = 0;
  if (!s.fl.timed || hipEventElapsedTime(&ms, s.ev0, s.ev1) != hipSuccess) return;
  ix->stats.last_scan_ms = ms;
  ix->stats.last_scan_rows = s.fl.timed_rows;
  ix->stats.last_scan_bytes = s.fl.timed_bytes;
  ix->stats.total_scan_ms += ms;
  ix->stats.total_scan_bytes += s.fl.timed_bytes;
  ix->stats.total_scan_launches += 1;
}

// ------------------------------------------------------------------------------------------------ collection, step by step

// step 0: the per-query collection state of a sub-batch of nq queries, the first of which is query q_first of the call
static void open_collection(Slot &s, int nq, int64_t q_first) {
  Slot::InFlight &fl = s.fl;
  fl.nq = nq;
  fl.q_first = q_first;
  fl.dense_q.clear();
  fl.tails.assign((size_t)nq, std::vector<uint64_t>());
  fl.host_cnt.assign((size_t)nq, 0);
  fl.host_replay.assign((size_t)nq, 0);
}

// step 1: what the device said about query i: entries listed, flags (non-zero: it could not bound the query, which goes to
// finish_replay's dense handling) and whether the host has to replay its heap over the list
static void set_verdict(bbq_index *ix, Slot &s, int i, uint32_t listed, uint32_t flags, bool replay) {
  s.h_list_counts[2 * i] = (int32_t)listed;
  s.h_list_counts[2 * i + 1] = (int32_t)flags;
  if (flags != 0) s.fl.dense_q.push_back(i);
  else if (replay) { s.fl.host_replay[(size_t)i] = 1; ix->stats.host_replays += 1; }
}

// ... for a sub-batch: from the header slots of the answer blocks (which carry what the two small copies used to bring), or from the
// copied counters - without the final selection every bounded query is replayed
static void read_verdicts(bbq_index *ix, Slot &s) {
  for (int i = 0; i < s.fl.nq; ++i)
    if (s.fl.final_used) {
      const AnswerHeader h(s.h_final + (size_t)i * s.final_stride);
      set_verdict(ix, s, i, h.listed, h.flags, h.needs_replay != 0);
    } else {
      set_verdict(ix, s, i, (uint32_t)s.h_list_counts[2 * i], (uint32_t)s.h_list_counts[2 * i + 1], true);
    }
}

// step 2: the lists of the queries to replay into the pinned h_lists rows.  prefix_on_host: the enqueue-time copy brought the first
// hprefix entries; otherwise (the device was to answer and could not: equal scores) the whole list is fetched - with ONE batch of
// asynchronous copies on the slot's stream (a synchronous pageable copy per query on the null stream stalled every other slot:
// duplicated vectors make such queries common)
static int fetch_lists(Slot &s, bool prefix_on_host) {
  Slot::InFlight &fl = s.fl;
  bool fetched = false;
  for (int i = 0; i < fl.nq; ++i) {
    if (!fl.host_replay[(size_t)i]) continue;
    const int64_t cnt = s.h_list_counts[2 * i], have = std::min<int64_t>(cnt, s.hprefix);
    if (!prefix_on_host && cnt > 0) {
      HIPCHK(hipMemcpyAsync(s.h_lists + (size_t)i * s.hprefix, s.d_lists + (size_t)i * s.list_cap, (size_t)have * 8, hipMemcpyDeviceToHost, s.stream));
      fetched = true;
    }
    fl.host_cnt[(size_t)i] = have;
    if (cnt > have) {  // rare (a flood): the rest of a list longer than the pinned row
      fl.tails[(size_t)i].resize((size_t)(cnt - have));
      HIPCHK(hipMemcpyAsync(fl.tails[(size_t)i].data(), s.d_lists + (size_t)i * s.list_cap + have, (size_t)(cnt - have) * 8, hipMemcpyDeviceToHost, s.stream));
      fetched = true;
    }
  }
  if (fetched) HIPCHK(hipStreamSynchronize(s.stream));
  return BBQ_OK;
}

// step 3: append mode leaves the entries of a segment in arrival order: the reference loop wants them by row (entries order like rows)
static void order_lists_by_row(Slot &s) {
  Slot::InFlight &fl = s.fl;
  for (int i = 0; i < fl.nq; ++i) {
    if (fl.host_cnt[(size_t)i] == 0 && fl.tails[(size_t)i].empty()) continue;
    uint64_t *l = s.h_lists + (size_t)i * s.hprefix;
    std::vector<uint64_t> &t = fl.tails[(size_t)i];
    if (t.empty()) {
      std::sort(l, l + fl.host_cnt[(size_t)i]);
    } else {  // list longer than the pinned row: sort the whole of it in the tail vector
      t.insert(t.begin(), l, l + fl.host_cnt[(size_t)i]);
      fl.host_cnt[(size_t)i] = 0;
      std::sort(t.begin(), t.end());
    }
  }
}

// step 4: queries the last finalize launch answered: the sorted rows are the result
static void take_device_answers(const SearchCall &c, Slot &s, int32_t *out_idx, float *out_score, int64_t *out_n) {
  for (int i = 0; i < s.fl.nq; ++i) {
    if (s.h_list_counts[2 * i + 1] != 0 || s.fl.host_replay[(size_t)i]) continue;
    const uint64_t *block = s.h_final + (size_t)i * s.final_stride;
    const int64_t qi = s.fl.q_first + i, m = AnswerHeader(block).count;
    unpack_entries(block + 2, m, out_idx + qi * c.k_out, out_score + qi * c.k_out);
    out_n[qi] = m;
  }
}

// step 5: the heap replays, on the pool when replay_threads > 1; finish_replay waits for them
static void schedule_replays(const SearchCall &c, Slot &s, int32_t *out_idx, float *out_score, int64_t *out_n) {
  const int64_t k = c.k_out, n_total = c.filter ? c.n_eff : c.ix->main.row_id_base + c.ix->main.view.n_rows;
  Slot *sp = &s;
  auto replay_range = [sp, k, n_total, out_idx, out_score, out_n](int lo, int hi) {
    Slot &s = *sp;
    for (int i = lo; i < hi; ++i) {
      if (!s.fl.host_replay[(size_t)i]) continue;
      HeapReplay hr(k, n_total);
      const uint64_t *l = s.h_lists + (size_t)i * s.hprefix;
      for (int64_t j = 0; j < s.fl.host_cnt[(size_t)i]; ++j) hr.offer(entry_score(l[j]), (int32_t)entry_row(l[j]));
      for (uint64_t e : s.fl.tails[(size_t)i]) hr.offer(entry_score(e), (int32_t)entry_row(e));
      const int64_t qi = s.fl.q_first + i;
      out_n[qi] = hr.finish(out_idx + qi * k, out_score + qi * k);
    }
  };
  const int nq = s.fl.nq, n_replay = (int)std::count(s.fl.host_replay.begin(), s.fl.host_replay.end(), 1);
  const int T = std::min(c.ix->opt_replay_threads, n_replay);
  s.fl.replaying = true;
  if (T == 1) replay_range(0, nq);
  if (T <= 1) return;  // nothing to replay, or replayed on this thread
  replay_pool().ensure(c.ix->opt_replay_threads);
  const int jobs = std::min(nq, T * 2);  // a few more jobs than threads: uneven lists balance out
  s.fl.pending.store(jobs);
  for (int t = 0; t < jobs; ++t) {
    const int lo = (int)((int64_t)nq * t / jobs), hi = (int)((int64_t)nq * (t + 1) / jobs);
    replay_pool().post([sp, replay_range, lo, hi] {
      replay_range(lo, hi);
      sp->fl.pending.fetch_sub(1, std::memory_order_release);
    });
  }
}

// device work of the slot's sub-batch is done: collect it and start the heap replays
int begin_replay(const SearchCall &c, Slot &s, int32_t *out_idx, float *out_score, int64_t *out_n) {
  HIPCHK(hipEventSynchronize(s.ev_done));
  s.fl.busy = false;
  account_timing(c.ix, s);
  open_collection(s, s.fl.nq, s.fl.q_first);
  read_verdicts(c.ix, s);
  int rc = fetch_lists(s, !s.fl.final_used);
  if (rc != BBQ_OK) return rc;
  if (s.fl.appended) order_lists_by_row(s);
  if (s.fl.final_used) take_device_answers(c, s, out_idx, out_score, out_n);
  schedule_replays(c, s, out_idx, out_score, out_n);
  return BBQ_OK;
}

// The call's one query (query 0) whose complete, unordered list sits in s.d_lists and whose answer a latency chain could not prove
// ({listed, flags}: what its answer header said; nothing of the slot is in flight): the collection steps it needs, to the end.
int replay_listed_query(const SearchCall &c, Slot &s, uint32_t listed, uint32_t flags, int32_t *out_idx, float *out_score, int64_t *out_n) {
  open_collection(s, 1, 0);
  set_verdict(c.ix, s, 0, listed, flags, true);
  int rc = fetch_lists(s, false);
  if (rc != BBQ_OK) return rc;
  order_lists_by_row(s);
  schedule_replays(c, s, out_idx, out_score, out_n);
  return finish_replay(c, s, out_idx, out_score, out_n);
}

// waits for the slot's replays, then serves the queries the device could not bound (dense path)
int finish_replay(const SearchCall &c, Slot &s, int32_t *out_idx, float *out_score, int64_t *out_n) {
  bbq_index *ix = c.ix;
  Slot::InFlight &fl = s.fl;
  auto wait_replays = [&fl] {
    while (fl.pending.load(std::memory_order_acquire) > 0) std::this_thread::yield();
    fl.replaying = false;
  };
  wait_replays();
  for (int i = 0; i < fl.nq; ++i)
    if (s.h_list_counts[2 * i + 1] == 0) ix->stats.candidates += s.h_list_counts[2 * i];
  if (fl.dense_q.empty()) return BBQ_OK;
  // queries the device could not bound.  The shared sweeps have no flood tier: a query whose candidate slots overflowed
  // there first gets one sweep of its own (slot s is free again at this point) before it pays for the dense path.
  const std::vector<int> flagged = fl.dense_q;
  std::vector<uint32_t> why;
  for (int i : flagged) why.push_back((uint32_t)s.h_list_counts[2 * i + 1]);
  const int64_t first = fl.q_first;
  fl.dense_q.clear();
  for (size_t j = 0; j < flagged.size(); ++j) {
    const int64_t qi = first + flagged[j];
    if (c.share > 1 && c.plan->flood_cap > 0 && why[j] == kFlagOverflow) {
      SearchCall alone = c;
      alone.share = 1;
      int rc = enqueue_subbatch(alone, s, qi, 1, nullptr);
      if (rc == BBQ_OK) rc = begin_replay(alone, s, out_idx, out_score, out_n);
      if (rc != BBQ_OK) return rc;
      wait_replays();
      const bool solved = fl.dense_q.empty();
      fl.dense_q.clear();
      if (solved) {
        ix->stats.candidates += s.h_list_counts[0];
        continue;
      }
    }
    int rc = dense_search_one(c, qi, out_idx + qi * c.k_out, out_score + qi * c.k_out, out_n + qi);
    if (rc != BBQ_OK) return rc;
  }
  return BBQ_OK;
}

// brings a slot back to "free": collect + replay + wait, whatever is still outstanding
static int reclaim_slot(const SearchCall &c, Slot &s, int32_t *out_idx, float *out_score, int64_t *out_n) {
  int rc = BBQ_OK;
  if (s.fl.busy) rc = begin_replay(c, s, out_idx, out_score, out_n);
  if (rc == BBQ_OK && s.fl.replaying) rc = finish_replay(c, s, out_idx, out_score, out_n);
  return rc;
}

int drain(bbq_index *ix) {
  for (int i = 0; i < kMaxSlots; ++i)
    if (ix->slots[i].stream) HIPCHK(hipStreamSynchronize(ix->slots[i].stream));
  return BBQ_OK;
}

// candidates, dense_fallbacks and host_replays count per call
static void reset_call_stats(bbq_index *ix) { ix->stats.candidates = ix->stats.dense_fallbacks = ix->stats.host_replays = 0; }

}  // namespace bbq

// bbq_search_batch, and - with `feed` - bbq_search_raw_batch: the quantized queries of a sub-batch are waited for right before it is
// enqueued; with `flt` - bbq_search_filtered_batch: the same call over the accepted rows only, on the pipelined per-query sweep or,
// with sweep_share 32, on the matrix-core sweep's filtered kernels behind the first k accepted rows (enqueue_subbatch).  The
// single-query chains and the VALU shared sweep (sweep_share 4 / 8) take no filter: such a call sweeps per query
static int search_batch_impl(bbq_index *ix, int32_t n_queries, const uint8_t *qquant, const double *qcorr, int32_t query_bits,
                             int32_t sim, int64_t k, int32_t *out_idx, float *out_score, int64_t *out_n, RawFeed *feed, int32_t *bad_query,
                             const bbq_filter *flt = nullptr) {
  int rc = validate_query_args(ix, n_queries, qquant, qcorr, query_bits, sim, k, feed != nullptr);
  if (rc != BBQ_OK) return rc;
  // a filter is checked against the index before anything returns: k == 0 does not excuse a filter of another index
  if (flt && ix->multi) return fail(BBQ_ERR_UNSUPPORTED, "filtered search is not supported on a multi-device index");
  if (flt && (ix->has_pilot || ix->row_base != 0))
    return fail(BBQ_ERR_UNSUPPORTED, "filtered search is not supported on a row shard or an index with a pilot replica");
  if (flt && (flt->device != ix->device || flt->n_rows != ix->n_rows))
    return fail(BBQ_ERR_INVALID_ARG, "the filter was made for an index of %lld rows on device %d, this one has %lld rows on device %d",
                (long long)flt->n_rows, flt->device, (long long)ix->n_rows, ix->device);
  if (n_queries > 0 && !out_n) return fail(BBQ_ERR_INVALID_ARG, "out_n is null");
  for (int32_t i = 0; i < n_queries; ++i) out_n[i] = 0;
  if (k == 0 || n_queries == 0) return BBQ_OK;  // src/binaryQuantizationFormat.ts:332-334
  if (!out_idx || !out_score) return fail(BBQ_ERR_INVALID_ARG, "output arrays are null");
  if (ix->multi) {
    reset_call_stats(ix);
    if (ix->n_rows == 0) return BBQ_OK;
    return multi_search_batch(ix, n_queries, qquant, qcorr, query_bits, sim, k, out_idx, out_score, out_n);
  }
  if (ix->has_pilot || ix->row_base != 0)
    return fail(BBQ_ERR_INVALID_ARG, "bbq_search on a non-root shard: use bbq_shard_scan + bbq_replay");
  std::lock_guard<std::mutex> lk(ix->ctx->mu);
  HIPCHK(hipSetDevice(ix->device));
  rc = settle_shard_slots(ix->ctx, nullptr);  // an asynchronous sharded scan on this device may have left slots busy
  if (rc != BBQ_OK) return rc;
  reset_call_stats(ix);
  const int64_t n_eff = flt ? flt->count : ix->n_rows;  // the rows that exist for this call
  if (n_eff == 0) return BBQ_OK;

  SearchCall c(ix, qquant, qcorr, 0, query_bits, sim, k);
  if (flt) {
    c.filter = flt;
    c.n_eff = n_eff;
    if (c.share != 32) c.share = 1;
  }
  if (feed) {  // the values are still being produced: the kernel variant follows from the bit width they are quantized to
    const int pq = query_bits <= 1 ? 1 : query_bits <= 2 ? 2 : query_bits <= 4 ? 4 : 8;
    c.planes = ix->geom.store_bits == 1 ? pq : ix->geom.store_bits == 8 ? 8 : (query_bits <= 4 ? 4 : 8);
    c.maxq = (1 << query_bits) - 1;
  } else {
    c.planes = planes_of_call(ix, qquant, (int64_t)n_queries * ix->geom.dim, query_bits == 1);
    c.maxq = c.planes <= 4 ? 15 : max_value(qquant, (int64_t)n_queries * ix->geom.dim);
  }
  const int64_t keff = std::min<int64_t>(k, n_eff);
  if (keff > kMaxFastK || ix->opt_force_dense) {
    for (int32_t i = 0; i < n_queries; ++i) {
      if (feed && (rc = feed->wait(i, 1, bad_query)) != BBQ_OK) return rc;
      rc = dense_search_one(c, i, out_idx + (int64_t)i * k, out_score + (int64_t)i * k, out_n + i);
      if (rc != BBQ_OK) return rc;
    }
    return BBQ_OK;
  }
  // thresholds are order statistics of rank min(k, N): selecting with a larger k would be wrong.  Up to kFinalSelectMax the device
  // runs with rank keff + 1 and the last finalize launch selects and sorts the answer itself (FinalizeArgs::final_out); the host
  // replays the heap only for queries with equal scores in or at the edge of their answer
  const int64_t final_k = (keff <= kFinalSelectMax && ix->opt_device_select) ? keff : 0;
  c.k_dev = final_k > 0 ? keff + 1 : keff;
  const bool latency = final_k > 0 && n_queries <= ix->opt_latency_queries;
  const Plan plan = flt ? build_filtered_plan(ix, *flt, c.k_dev, final_k, latency) : build_plan(ix, c.k_dev, final_k, latency);
  c.plan = &plan;
  if (n_queries == 1 && plan.latency && !feed && !flt) {
    bool done = false;
    rc = search_latency_presampled(c, out_idx, out_score, out_n, &done);
    if (rc != BBQ_OK || done) return rc;
    rc = search_latency_chain(c, out_idx, out_score, out_n, &done);
    if (rc != BBQ_OK || done) return rc;
  }
  const int Q = effective_batch(ix, n_queries);
  const int nslots = std::min(std::max(1, ix->opt_slots), kMaxSlots);
  const int64_t nsub = ((int64_t)n_queries + Q - 1) / Q;
  auto fail_out = [&](int code) {
    for (int i = 0; i < kMaxSlots; ++i)  // never leave pool jobs pointing at a caller's buffers
      while (ix->slots[i].fl.pending.load(std::memory_order_acquire) > 0) std::this_thread::yield();
    drain(ix);
    for (int i = 0; i < kMaxSlots; ++i) ix->slots[i].fl.reset();
    return code;
  };
  for (int64_t i = 0; i < nsub; ++i) {
    Slot &s = ix->slots[i % nslots];
    rc = reclaim_slot(c, s, out_idx, out_score, out_n);
    if (rc != BBQ_OK) return fail_out(rc);
    const int nq = (int)std::min<int64_t>(Q, n_queries - i * Q);
    rc = ensure_slot(c, s, nq, true);
    if (rc != BBQ_OK) return fail_out(rc);
    if (feed && (rc = feed->wait(i * Q, nq, bad_query)) != BBQ_OK) return fail_out(rc);
    rc = enqueue_subbatch(c, s, i * Q, nq, nullptr);
    if (rc != BBQ_OK) return fail_out(rc);
    // hand finished sub-batches to the replay workers as early as possible (their slot is needed again soon)
    for (int j = 0; j < nslots; ++j) {
      Slot &t = ix->slots[j];
      if (&t != &s && t.fl.busy && hipEventQuery(t.ev_done) == hipSuccess) {
        rc = begin_replay(c, t, out_idx, out_score, out_n);
        if (rc != BBQ_OK) return fail_out(rc);
      }
    }
  }
  for (int64_t i = std::max<int64_t>(0, nsub - nslots); i < nsub; ++i) {  // oldest first
    rc = reclaim_slot(c, ix->slots[i % nslots], out_idx, out_score, out_n);
    if (rc != BBQ_OK) return fail_out(rc);
  }
  return BBQ_OK;
}

extern "C" {

int bbq_search_batch(bbq_index *ix, int32_t n_queries, const uint8_t *qquant, const double *qcorr, int32_t query_bits,
                     int32_t sim, int64_t k, int32_t *out_idx, float *out_score, int64_t *out_n) {
  clear_error();
  return search_batch_impl(ix, n_queries, qquant, qcorr, query_bits, sim, k, out_idx, out_score, out_n, nullptr, nullptr);
}

int bbq_search_filtered_batch(bbq_index *ix, const bbq_filter *f, int32_t n_queries, const uint8_t *qquant, const double *qcorr,
                              int32_t query_bits, int32_t sim, int64_t k, int32_t *out_idx, float *out_score, int64_t *out_n) {
  clear_error();
  if (!f) return fail(BBQ_ERR_INVALID_ARG, "bbq_search_filtered_batch: the filter is null");
  return search_batch_impl(ix, n_queries, qquant, qcorr, query_bits, sim, k, out_idx, out_score, out_n, nullptr, nullptr, f);
}

int bbq_search_raw_batch(bbq_index *ix, int32_t n_queries, const float *queries, const float *centroid, int32_t sim, int32_t query_bits,
                         double lambda, int32_t iters, int32_t n_threads, int64_t k, int32_t *out_idx, float *out_score, int64_t *out_n,
                         uint8_t *qquant_out, double *qcorr_out, int32_t *bad_query) {
  clear_error();
  if (bad_query) *bad_query = -1;
  if (!ix) return fail(BBQ_ERR_INVALID_ARG, "目标向量集合不能为空");
  if (n_queries < 0) return fail(BBQ_ERR_INVALID_ARG, "n_queries < 0");
  if (n_queries > 0 && (!queries || !centroid)) return fail(BBQ_ERR_INVALID_ARG, "查询向量不能为空");
  if (k < 0) return fail(BBQ_ERR_NEGATIVE_K, "k值不能为负数");
  if (query_bits < 1 || query_bits > 8) return fail(BBQ_ERR_INVALID_ARG, "queryBits必须在1-8之间");
  if (n_queries == 0) return BBQ_OK;
  const int dim = ix->geom.dim;
  std::vector<uint8_t> own_q;
  std::vector<double> own_c;
  uint8_t *qq = qquant_out;
  double *qc = qcorr_out;
  if (!qq) { own_q.resize((size_t)n_queries * dim); qq = own_q.data(); }
  if (!qc) { own_c.resize((size_t)n_queries * 4); qc = own_c.data(); }
  const int T = n_threads > 0 ? n_threads : default_host_threads();
  // few queries, k == 0 (the quantizer's errors still surface, as in the reference's order of checks) or a multi-device handle
  // (its rounds take whole arrays): quantize first, then search
  if (n_queries <= 64 || k == 0 || ix->multi) {
    int rc = bbq_quantize_queries(queries, n_queries, dim, centroid, sim, query_bits, lambda, iters, T, qq, qc, bad_query);
    if (rc != BBQ_OK) return rc;
    return search_batch_impl(ix, n_queries, qq, qc, query_bits, sim, k, out_idx, out_score, out_n, nullptr, nullptr);
  }
  RawFeed feed;
  feed.queries = queries; feed.centroid = centroid; feed.n = n_queries; feed.dim = dim; feed.sim = sim; feed.qb = query_bits;
  feed.lambda = lambda; feed.iters = iters; feed.qq = qq; feed.qc = qc;
  // the argument checks of the quantizer, once, on this thread (the workers would only report "failed")
  {
    int rc = bbq_quantize_query(queries, dim, centroid, sim, query_bits, lambda, iters, qq, qc);
    if (rc != BBQ_OK) { if (bad_query) *bad_query = 0; return rc; }
  }
  feed.start(T);
  int rc = search_batch_impl(ix, n_queries, qq, qc, query_bits, sim, k, out_idx, out_score, out_n, &feed, bad_query);
  feed.join();
  return rc;
}

int bbq_search(bbq_index *ix, const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim, int64_t k,
               int32_t *out_idx, float *out_score, int64_t *out_n) {
  return bbq_search_batch(ix, 1, qquant, qcorr, query_bits, sim, k, out_idx, out_score, out_n);
}

}  // extern "C"
