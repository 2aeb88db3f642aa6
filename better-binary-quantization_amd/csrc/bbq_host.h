// bbq_host.h - host-side internals of libbbq shared by its translation units: the device-resident index object, the
// per-device context (streams, events, per-slot workspace) and the helpers every entry point needs.
//   bbq_index.cpp    device context, index creation from rows, cache budget of a launch, statistics, options
//   bbq_core.cpp     segment plan, slot workspace, pipelined batch search: enqueue, collection in steps, host replay (shares bbq_search.h - the SearchCall - with the next four)
//   bbq_query.cpp    query staging    bbq_latency.cpp  single-query chains    bbq_dense.cpp  dense path, bbq_score_rows
//   bbq_shard.cpp    scan of one shard of a row-sharded index (bbq_shard_scan*)
//   bbq_multi.cpp    one index over several devices of a process
//   bbq_append.cpp   the one path that writes rows into an index - creation and build are appends to an empty one - and the entry
//                    points that grow an index in place (bbq_index_append*, bbq_index_reserve)
//   bbq_compact.cpp  rows taken out of an index on the device (bbq_index_compact, bbq_index_remove_rows, bbq_filter_kept_rows)
//   bbq_update.cpp   rows of an index replaced in place (bbq_index_update*, bbq_update_winners)
//   bbq_build.cpp    quantizeVectors on the device (bbq_index_build)
//   bbq_gather.cpp   scoring and ranking chosen rows (bbq_score_ords*, bbq_search_ords_batch)
//   bbq_range.cpp    range search: every row at or above a threshold (bbq_range_key, bbq_count_range_batch, bbq_search_range_batch)
//   bbq_span.cpp     span search: the k best rows of per-query row spans (bbq_search_spans_batch, bbq_search_spans_filtered_batch)
//   bbq_group.cpp    grouped search: the k best groups of rows by their best row (bbq_groups_*, bbq_search_grouped_batch)
//   bbq_maxsim.cpp   MaxSim search: the k best groups by the sum of their best rows over a query's token vectors (bbq_search_maxsim_batch)
//   bbq_select.cpp   what the three above end with: the device's selected answers proven, the rest replayed on the host (finish_selected)
//   bbq_maxsim_groups.cpp, bbq_maxsim_rerank.cpp   MaxSim over chosen groups, quantized and exact (bbq_*_maxsim_groups_batch, bbq_search_maxsim_rerank_batch)
//   bbq_rerank.cpp   oversample + exact rerank (bbq_vectors_*, bbq_rerank_scores, bbq_search_rerank_batch)
//   bbq_exact.cpp    exact search over the fp32 rows (bbq_true_topk, bbq_vectors_search_batch, bbq_vectors_set_option)
//   bbq_persist.cpp  on-disk format (bbq_index_save / load / file_info / export)
// bbq_entry.h is the codec of the 64-bit entries, keys and answer headers; bbq_workqueue.h the host threads' job queue.
// HIP memory and events are held in the owning types of bbq_mem.h: what a struct below owns goes with it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <atomic>
#include <algorithm>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "bbq_internal.h"
#include "bbq_launch.h"
#include "bbq_mem.h"

#define HIPCHK(expr)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) return fail(BBQ_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

namespace bbq {

constexpr int kMaxSlots = 4;
constexpr int64_t kMaxFastK = 4096;  // beyond this the dense path is used: the finalize kernel selects thresholds among at most 12288 keys (running top-k + new), and with k close to that the thresholds get too weak to pay (k = 4096: 4 ms per 10 M-row query, dense path 16 ms, k = 6000 on the sparse path 23 ms)

struct Storage {
  DevBuf<uint8_t> d_tiles;
  DevBuf<double> d_exact;     // kLayoutCompact: exact corrections, gathered for the rows whose bound passes; the per-tile
                              // additive-correction ranges (view.add_range) and, where they exist, the rows' component sums
                              // (view.row_sums) live behind them in the same allocation
  int64_t cap_tiles = 0;      // tiles both allocations hold (>= the tiles in use; more after bbq_index_reserve / an append that grew):
                              // exact[] takes cap_tiles * 64 rows, add_range[] starts behind THAT, wherever the rows end, and
                              // row_sums[] behind add_range[]'s cap_tiles entries
  IndexView view{};
  int64_t row_id_base = 0;
  int64_t n_chunks() const { return (view.n_rows + kChunkRows - 1) / kChunkRows; }
};

struct Segment {
  int storage;  // 0 = pilot replica, 1 = main
  int64_t chunk_begin, n_chunks, rows;
  bool dense, emit, need_theta, dominant;
  int cap;
  bool big = false;  // large sweeps of different sub-batches are serialised through an event chain
};

// the segments of one call and the sizes that follow from them: built per call (build_plan) and handed on through its SearchCall
struct Plan {
  int64_t k = 0;          // the rank the device selects thresholds with
  std::vector<Segment> segs;
  int64_t s0 = 0;
  int64_t list_cap = 0;
  int64_t flood_cap = 0;  // per-query entries of the flood tier (overflow area + list headroom); 0: none
  int64_t max_slots = 0;  // max over sparse segments of n_chunks*cap
  int64_t max_chunks = 0;
  int64_t final_k = 0;    // > 0: the plan runs with k = final_k + 1 and the last finalize launch selects the answer itself
  int growth = 0;         // segment growth the plan was built with
  bool latency = false;   // plan of a call with few queries: latency_growth, candidates appended to the list by the scan launches
};

struct Slot {
  hipStream_t stream = nullptr;
  Event ev0, ev1, ev_done, ev_big;
  // capacities the buffers below hold (grow-only maxima over the plans seen; kernels take them as strides and limits)
  int q_cap = 0;
  int64_t qbuf_bytes = 0, chunks_cap = 0, slots_cap = 0, dense_cap = 0, list_cap = 0, k_cap = 0, hprefix = 0, flood_cap = 0;
  // one device block [control words of the sub-batch | staged queries] and its pinned host twin whose control part stays zero: ONE
  // host-to-device copy resets the thresholds / counters and brings the queries (d_theta.. and d_qbuf point into it)
  DevBuf<uint8_t> d_block;
  PinnedBuf<uint8_t> h_block;
  int64_t ctrl_bytes = 0;
  // views into d_block / h_block, derived again whenever the block is reallocated (ensure_slot)
  uint8_t *d_qbuf = nullptr, *h_qbuf = nullptr;
  Threshold *d_theta = nullptr;
  uint32_t *d_flags = nullptr, *d_append_counts = nullptr, *d_ovf_counts = nullptr;
  int32_t *d_topk_counts = nullptr, *d_list_counts = nullptr;
  DevBuf<uint32_t> d_counts, d_topk;
  PinnedBuf<int32_t> h_list_counts;
  DevBuf<uint64_t> d_entries, d_lists, d_ovf;
  PinnedBuf<uint64_t> h_lists;
  DevBuf<float> d_dense0;
  // final selection on the device (FinalizeArgs::final_out): the sorted answer + {count, needs-host-replay} per query
  DevBuf<uint64_t> d_final;  // [q_cap][final_stride]: 2 header slots + the answer per query
  PinnedBuf<uint64_t> h_final;
  int64_t final_stride = 0;
  // what is in flight on the slot (everything above is workspace).  busy: device work enqueued, not yet collected; replaying: host replay jobs outstanding
  struct InFlight {
    bool busy = false, replaying = false, timed = false;
    bool appended = false;    // the lists are unordered inside their segments (append mode)
    bool final_used = false;  // enqueued with the final selection (the list prefix was NOT copied to the host)
    std::atomic<int> pending{0};
    int nq = 0;               // queries of the sub-batch ...
    int64_t q_first = 0;      // ... from this query of the call on
    // collection (begin_replay): per query, does the host replay its heap; entries of query i in its h_lists row (the rest, if any, in
    // tails[i]); the queries the device could not bound
    std::vector<uint8_t> host_replay;
    std::vector<int64_t> host_cnt;
    std::vector<std::vector<uint64_t>> tails;
    std::vector<int> dense_q;
    int64_t timed_rows = 0, timed_bytes = 0;  // timed: of the dominant sweep between ev0 and ev1
    // non-null: the sub-batch belongs to an asynchronous sharded scan of that index (bbq_shard_scan_begin); nothing is to be collected
    // from it but the timing.  Such slots stay busy ACROSS API calls: every entry point that uses the slots settles them first.
    bbq_index *shard_owner = nullptr;
    void reset() { busy = replaying = appended = final_used = timed = false; nq = 0; dense_q.clear(); shard_owner = nullptr; }  // no job pending
  } fl;
  // the control words are all zero (the latency chain leaves them so and expects them so; every other use of the slot dirties them
  // and resets them with its own host-to-device copy)
  bool ctrl_clean = false;
};

// Per-device context shared by every index on that device: streams, events and the per-slot workspace are expensive
// to create (~10 ms per index with hipStreamCreate/Destroy) and quickSearch builds a fresh index on every call
// (src/index.ts:109), so they live for the process.  One API call at a time per device (mutex).
struct DeviceCtx {
  std::mutex mu;
  Slot slots[kMaxSlots];
  hipStream_t aux_stream = nullptr;   // dense path / bbq_score_rows / index build: never touches an in-flight slot
  DevBuf<uint8_t> d_aux_qbuf;
  DevBuf<uint32_t> d_aux_flags;
  DevBuf<uint8_t> d_gather;          // grow-only scratch of bbq_score_ords* (bbq_gather.cpp): one launch's offsets, queries, ords and outputs
  DevBuf<uint8_t> d_range;           // grow-only scratch of a range search's sub-batch (bbq_range.cpp): queries, thresholds, per-chunk counts and lists
  DevBuf<uint8_t> d_span;            // grow-only scratch of a span search's sub-batch (bbq_span.cpp): queries, span tables, work items, answer blocks, scores;
                                     // of a grouped search's (bbq_group.cpp): queries, answer blocks, the representatives' keys, scores and ords; and of
                                     // the MaxSim calls' (bbq_maxsim*.cpp).  What bbq_select.cpp's finish_selected brings scores and ords back from
  int last_big_slot = -1;             // slot whose ev_big marks the end of the most recently enqueued big sweep
  // latency path (bbq_latency_kernels.hip): the answer of a single-query call lands in mapped, coherent host memory and the host
  // polls a sequence word behind it: [0] sequence, [8 ..) header + entries
  PinnedBuf<uint64_t> h_lat{hipHostMallocMapped | hipHostMallocCoherent};
  uint64_t *d_lat = nullptr;          // h_lat as the device sees it
  uint64_t lat_seq = 0;
  DevBuf<uint32_t> d_pre_keys;        // [kLatPreKeys] per-wave top keys of the pre-sampled threshold
  // the indexes that launched sweeps on this device lately share its Infinity Cache (launch_view, bbq_index.cpp); under `mu`
  struct CacheUser { const void *index; int64_t bytes; uint64_t tick; };
  std::vector<CacheUser> cache_users;
  // only ever runs for a context that get_ctx could not finish: a published one lives until the process ends
  ~DeviceCtx() {
    for (Slot &s : slots)
      if (s.stream) (void)hipStreamDestroy(s.stream);
    if (aux_stream) (void)hipStreamDestroy(aux_stream);
  }
};
constexpr int kLatAnswerOffset = 8;   // words in front of the answer block inside DeviceCtx::h_lat

// per query: bit-planes (up to 8) + int8 values in MFMA fragment order + score uniforms + group maxima
int64_t qbuf_bytes_per_query_w(int w16);
// returns the (lazily created, never destroyed) context of a device; call with hipSetDevice(device) done
int get_ctx(int device, DeviceCtx **out);
int ensure_aux_qbuf(DeviceCtx *c, int64_t bytes);
// where the next array of a scratch layout starts: the 16-byte boundary at or behind byte b
inline size_t align16(size_t b) { return (b + 15) / 16 * 16; }
// a context's grow-only scratch holds `bytes`, or BBQ_ERR_OOM in the words of `what` - before anything is written to the caller's arrays
inline int reserve_scratch(DevBuf<uint8_t> &scratch, size_t bytes, const char *what) {
  const hipError_t e = scratch.reserve(bytes);
  if (e == hipSuccess) return BBQ_OK;
  (void)hipGetLastError();
  return fail(BBQ_ERR_OOM, "%s: %zu bytes of scratch: %s", what, bytes, hipGetErrorString(e));
}
// default number of host threads (heap replays, query quantization): half the cores, at most 16
inline int default_host_threads() { return (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency() / 2)); }
// bytes of the compact layout's side arrays for n_tiles tiles: exact corrections + add ranges (an allocation: n_tiles = its capacity;
// a file: the tiles in use, the two parts back to back)
inline int64_t compact_side_bytes(int64_t n_tiles) { return n_tiles * kTileRows * 32 + n_tiles * 8; }
inline const float *add_range_of(const double *d_exact, int64_t cap_tiles) {
  return d_exact ? reinterpret_cast<const float *>(d_exact + cap_tiles * kTileRows * 4) : nullptr;
}
// the rows' component sums, uint16 per row, behind the cap_tiles add ranges (8 bytes each: compact_side_bytes(cap_tiles) from the
// start) - a derived array that no file holds; null where the geometry has none (row_sums_fit)
inline int64_t row_sums_bytes(const TileGeom &g, int64_t n_tiles) { return row_sums_fit(g) ? n_tiles * kTileRows * 2 : 0; }
inline const uint16_t *row_sums_of(const double *d_exact, int64_t cap_tiles, const TileGeom &g) {
  return d_exact && row_sums_fit(g) ? reinterpret_cast<const uint16_t *>(reinterpret_cast<const uint8_t *>(d_exact) + compact_side_bytes(cap_tiles)) : nullptr;
}
// bytes of a compact storage's side allocation for cap_tiles tiles
inline int64_t compact_alloc_bytes(const TileGeom &g, int64_t cap_tiles) { return compact_side_bytes(cap_tiles) + row_sums_bytes(g, cap_tiles); }

}  // namespace bbq

namespace bbq { struct MultiState; }

struct bbq_index {
  bbq::MultiState *multi = nullptr;  // non-null: this handle is a row-sharded index over several devices (bbq_multi.cpp); it owns no
                                     // storage itself and every entry point dispatches to the shards
  int device = 0;
  bbq::DeviceCtx *ctx = nullptr;
  bbq::Slot *slots = nullptr;  // = ctx->slots
  bbq::TileGeom geom{};  // of every tile record of the index: each storage's view holds a copy (set_storage_view)
  int32_t want_compact = 1, index_bits = 1;  // geom.store_bits follows from index_bits (set_index_geometry)
  int64_t n_rows = 0, row_base = 0;
  double centroid_dp = 0;
  bool has_pilot = false;
  bbq::Storage pilot, main;
  bbq::DevBuf<float> d_dense_all;
  // bbq_shard_scan_begin / _wait: per-query lists before packing, two sets (two batches may be in flight) and their tickets
  struct ShardSet {
    bbq::DevBuf<uint64_t> d_lists;
    bbq::DevBuf<int32_t> d_counts;  // [q_cap][2] + the packed total (int64) behind them
    int64_t q_cap = 0, list_cap = 0;
    bbq::Event done;                // recorded behind the packing of the batch
    bbq::PinnedBuf<int64_t> h_total;
    int64_t packed_cap = 0;
  } shard_set[2];
  int64_t shard_begun = 0, shard_waited = 0;  // batches begun / waited for: ticket t uses set t & 1
  // options
  int opt_batch = 0 /* 0: by index size, effective_batch() */, opt_slots = 3, opt_growth = 8, opt_force_dense = 0, opt_share = 1, opt_device_select = 1;
  // a call with few queries is latency-bound: every segment costs a dependent scan + finalize launch pair (~15-20 us), so such calls
  // walk the index in fewer, faster-growing segments (more candidates per query - the device selects the answer itself anyway)
  int opt_latency_queries = 4, opt_latency_growth = 64;
  int opt_resident_interleave = 1;  // the resident chunks of a launch are spread over its range (of every 64 chunks the first n) instead of being its head
  int opt_resident_mb = -1;  // MiB of its row range that ONE sweep launch loads with the default cache policy, so that they stay in the Infinity
                             // Cache from one query's sweep to the next (launch_view(), bbq_index.cpp); -1: this index's share of kResidentAutoBytes
  int opt_l2_share = -1;  // queries whose workgroups sweep one chunk back to back on one XCD, so that all but the first read it through that
                          // XCD's L2 (sweep_coord, bbq_device.h): 1 off, 2..32, -1: l2_share_shift()'s choice (bbq_core.cpp)
  int opt_row_sums = -1;  // the per-query sparse sweep reads a row's component sum from the row_sums side array instead of counting it:
                          // 0 never, 1 wherever the array exists, -1: row_sums_for_launch()'s choice (bbq_core.cpp)
  int opt_tiles_per_wave = -1;  // tiles a wave of the per-query sparse sweep takes one after the other where the launch has such a twin: 1, 2, 4, 8;
                                // -1: per row width, the fastest value whose kernel keeps the one-tile kernel's waves - 8 at 6 chunks, 4 at 8 (tiles_per_wave_for, bbq_core.cpp)
  int opt_digit_planes = -1;  // a 4-plane query against 1-bit rows is swept in three ternary digit planes wherever the sweep reads the row sums
                              // and has a digit twin: 0 never, 1 and -1 wherever it can (digit_planes_for_call, bbq_core.cpp)
  int opt_group_scratch_mb = 256;  // MiB of scratch a grouped search's sub-batch may take for its representatives, 16 B per live group and
                                   // query (bbq_group.cpp): as many queries per score launch as fit, at least one
  int opt_maxsim_fused = -1;  // the MaxSim search's score pass: 1 the fused kernel wherever it exists, 0 the grouped search's kernel per token
                              // vector, -1 what was measured faster (bbq_maxsim.cpp).  The answers are the same either way
  int opt_fast_bound = 1;  // 1: the compact layout's score bound in f32 against the threshold's z image wherever the query's f32 images allow it
                           // (fast_bound_images, bbq_query.cpp); 0: always the f64 bound.  The answers are the same either way
  int opt_latency_presample = 1;  // ... and on large indexes get their threshold from per-wave top keys of a prefix (two small launches) instead of two scan / finalize pairs
  int opt_latency_fused = 1;  // single-query calls take the three-launch latency path (bbq_latency_kernels.hip) when the index shape has one
  int opt_append_last = 1;  // append mode also for the last (largest) segment: its finalize launch gets cheaper, its sweep slower (one
                            // atomic per workgroup with candidates); measured at 10 M x 768: 0.250 ms per call with, 0.263 without
  // host threads replaying the heaps of one sub-batch: half the cores, at most 8 (a batch of 32 answers 1.4x sooner than with 1)
  int opt_replay_threads = bbq::default_host_threads();
  int64_t opt_s0 = 4096;
  // flood tier: candidates one query may pile up beyond the planned list (rows stored cluster by cluster make the
  // query's own cluster beat a threshold that was derived from other clusters) before it has to take the dense path
  int64_t opt_flood = 262144;
  bbq_stats stats{};
};

namespace bbq {
// corrections layout asked for at creation: an explicit option wins, the environment variable only speaks for callers that passed none
inline int want_compact_of(const bbq_index_options *opts) {
  if (opts && opts->size >= (int32_t)sizeof(bbq_index_options) && opts->corrections != BBQ_CORRECTIONS_DEFAULT)
    return opts->corrections == BBQ_CORRECTIONS_INLINE ? 0 : 1;
  const char *e = getenv("BBQ_COMPACT_CORRECTIONS");
  return (e && e[0] == '0') ? 0 : 1;
}
inline int check_options(const bbq_index_options *opts) {
  if (!opts) return BBQ_OK;
  if (opts->size < (int32_t)sizeof(bbq_index_options)) return fail(BBQ_ERR_INVALID_ARG, "bbq_index_options.size is %d, this library expects at least %d", opts->size, (int)sizeof(bbq_index_options));
  if (opts->corrections < BBQ_CORRECTIONS_DEFAULT || opts->corrections > BBQ_CORRECTIONS_COMPACT) return fail(BBQ_ERR_INVALID_ARG, "bbq_index_options.corrections out of range: %d", opts->corrections);
  return BBQ_OK;
}
// the integer dot product of one row must fit 31 bits: dim * 255 for packed 1-bit rows (query values <= 255), dim * 255 * 255 for multi-bit fields
inline bool dim_supported(int64_t dim, int store_bits) { return dim * 255 * (store_bits > 1 ? 255 : 1) <= 0x7fffffffll; }
#pragma GCC visibility push(hidden)  // bbq_index.cpp, for the other units only (not among the library's dynamic symbols)
// what an entry point that takes a device number does first: BBQ_ERR_NO_DEVICE without a usable device (require_devices), the range
// check (check_device), then the device made current and its context (open_device)
int require_devices(int *ndev);
int check_device(int device);
int open_device(int device, DeviceCtx **ctx);
// dim, index_bits and what follows from them: store_bits, w16
void set_index_geometry(bbq_index *ix, int32_t dim, int32_t index_bits);
// a new index on its device: the geometry, the context and its slots, the auxiliary query buffer grown to this index's queries
int attach_index(bbq_index *ix, DeviceCtx *ctx, int device, int32_t dim, int32_t index_bits);
// The view a launch gets: the stored view + which chunks it loads cache-resident, and the bytes of them (the caller that sweeps the index
// sums them into bbq_stats.resident_bytes).  Context mutex held by the caller.
struct LaunchView { IndexView view; int64_t resident_bytes; };
LaunchView launch_view(bbq_index *ix, const Storage &sto, int64_t chunk_begin = 0, int64_t n_chunks = -1);
#pragma GCC visibility pop
// retires what the device still runs for the index and deletes it (its members release their memory); the device context (streams,
// workspace) stays.  Call with the context mutex held.
void destroy_unlocked(bbq_index *ix);
// the view of a storage whose buffers (and cap_tiles) are in place: its rows + the geometry of the index (layout, tile_stride, has_x1 decided)
inline void set_storage_view(const bbq_index *ix, Storage &st, int64_t n_rows, int64_t row_id_base) {
  st.row_id_base = row_id_base;
  st.view.n_rows = n_rows;
  st.view.geom = ix->geom;
  st.view.tiles = st.d_tiles;
  st.view.exact = st.d_exact;
  st.view.add_range = add_range_of(st.d_exact, st.cap_tiles);
  st.view.row_sums = row_sums_of(st.d_exact, st.cap_tiles, ix->geom);
}
// bytes per row as the caller hands them over and gets them back: packed bits, or one byte per dimension for a multi-bit index
inline int64_t caller_row_bytes(const bbq_index *ix) { return ix->geom.store_bits > 1 ? ix->geom.dim : pb_of(ix->geom); }
inline int64_t tiles_of(int64_t rows) { return (rows + kTileRows - 1) / kTileRows; }
// compact corrections (4 B/row streamed + exact and add-range side arrays) need the implicit component sum; otherwise inline
inline void decide_layout(bbq_index *ix) {
  ix->geom.layout = (ix->want_compact && !ix->geom.has_x1) ? kLayoutCompact : kLayoutInline;
  ix->geom.tile_stride = tile_stride_of(ix->geom.w16, ix->geom.layout, ix->geom.has_x1);
}

// ---- bbq_append.cpp: the one path that writes rows into a storage.  A creation, a build and a load are appends to an empty storage;
// all of it runs on the context's aux_stream with the context mutex held and the device current.
#pragma GCC visibility push(hidden)
// Room for `need_tiles` tiles of a storage.  While they fit its capacity nothing happens and the rows are written in place; otherwise
// larger buffers are allocated HERE and the tiles in use copied over device to device - the storage itself only changes in commit(),
// so a failure on the way costs nothing but these buffers.
struct Room {
  DevBuf<uint8_t> tiles;
  DevBuf<double> exact;
  int64_t cap_tiles = 0;
  bool grown = false;
  uint8_t *d_tiles = nullptr;   // where the rows are written
  double *d_exact = nullptr;
  float *d_add_range = nullptr;
  uint16_t *d_row_sums = nullptr;  // null: the geometry has none
};
// where the build kernels write the rows that go into `r`, and the scratch tile set quantize_into's explicit-sums branch packs codes
// into: inline records of the index's row width without a component sum (a freshly quantized row's sum is its popcount)
inline TileDest tile_dest(const bbq_index *ix, const Room &r) { return TileDest{r.d_tiles, r.d_exact, ix->geom}; }
inline TileDest scratch_tile_dest(const bbq_index *ix, uint8_t *tiles) {
  TileGeom g = ix->geom;
  g.layout = kLayoutInline;
  g.has_x1 = 0;
  g.tile_stride = tile_stride_of(g.w16, g.layout, g.has_x1);
  return TileDest{tiles, nullptr, g};
}
// what can be written to: a single-device root index without a pilot replica that stays below 2^32 rows with n more (the scope of the
// filters); `who` names the entry point in the message
int check_append_index(const bbq_index *ix, int64_t n, const char *who);
// the index made quiet: nothing of it in flight on the device (BBQ_ERR_INVALID_ARG while a bbq_shard_scan_begin batch has not been
// waited for).  Context mutex held, device current.
int quiesce(bbq_index *ix, const char *who);
// the one function that allocates tile records: d_tiles and, for the compact layout, the side arrays for `cap` tiles (BBQ_ERR_OOM)
int alloc_tiles(const bbq_index *ix, int64_t cap, DevBuf<uint8_t> &tiles, DevBuf<double> &exact);
// what every write of the rows [row0, total) into `room` ends with: the touched tiles' add ranges and row sums (compact layout), then
// the device has completed and the rows may be committed
int finish_rows(const bbq_index *ix, const Room &room, int64_t row0, int64_t total);
// geometric: half as much again as the capacity, at least what is needed (an empty storage gets exactly what is needed); otherwise
// exactly what is needed.  BBQ_ERR_OOM without device memory.
int make_room(bbq_index *ix, Storage &st, int64_t need_tiles, Room &r, bool geometric = true);
// the rows (or the reservation) published: called after the device has completed everything that wrote them and everything that read
// the old buffers, which are released here.  The rows of the main storage are the rows of the index.
void commit(bbq_index *ix, Storage &st, Room &r, int64_t n_rows);
// What rows mean for an index that stores no explicit component sums when a row's sum is not its popcount / code sum.  kDecide (a
// creation, whose layout is still open): the index stores the sums from now on, and the layout follows.  kRequire (an append): the
// rows are refused with BBQ_ERR_UNSUPPORTED, as are multi-bit codes not below 2^indexBits, before anything is written.  A storage
// that holds neither rows nor room decides whatever the mode: nothing would have to be re-tiled.
enum class Sums { kDecide, kRequire };
// n rows in host memory, in the caller's shape -> device scratch (BBQ_ERR_OOM); the copies are enqueued on the aux stream
int stage_rows(const bbq_index *ix, const uint8_t *codes, const double *corr, int64_t n, DevBuf<uint8_t> &d_codes, DevBuf<double> &d_corr);
// staged rows asked what `mode` says about their component sums and, for multi-bit rows under kRequire, whether every code is below
// 2^indexBits (BBQ_ERR_INVALID_ARG).  Nothing of the index is written; returns with the device done.
int check_device_rows(bbq_index *ix, const uint8_t *d_codes, const double *d_corr, int64_t n, Sums mode);
// n rows in host memory, in the caller's shape, become the rows behind those `st` holds
int append_host_rows(bbq_index *ix, Storage &st, const uint8_t *codes, const double *corr, int64_t n, Sums mode);
// n fp32 rows -> d_vT4, the [ceil(dim/4)][tiles_of(n) * 64] float4 transposed copy, normalized for COSINE and validated: the first NaN
// / Infinity in row-major order is BBQ_ERR_NAN_INPUT / BBQ_ERR_INF_INPUT with its position in *bad_row, *bad_col (when non-null)
int stage_vectors(DeviceCtx *ctx, const float *vectors, int64_t n, int32_t dim, int32_t sim, DevBuf<float> &d_vT4, int64_t *bad_row, int32_t *bad_col);
// the n staged vectors quantized against d_cen into device scratch in the caller's shape (d_codes [n][caller_row_bytes], d_corr [n][4]),
// without touching the index: what quantize_into hands to the row-major path and what an update scatters.  codes_out / corr_out
// (optional) get all n rows.  Releases d_vT4.  1-bit rows go through a scratch tile set (launch_build_quantize1 + launch_build_untile).
int quantize_staged(bbq_index *ix, DevBuf<float> &d_vT4, int64_t n, const float *d_cen, int32_t sim, double lambda, int32_t iters,
                    DevBuf<uint8_t> &d_codes, DevBuf<double> &d_corr, uint8_t *codes_out, double *corr_out);
// the n staged vectors quantized against d_cen become the rows behind those the main storage holds; codes_out / corr_out (optional) get
// them in the caller's shape.  Releases d_vT4 as soon as it has been read where more memory is needed behind it.
int quantize_into(bbq_index *ix, DevBuf<float> &d_vT4, int64_t n, const float *d_cen, int32_t sim, double lambda, int32_t iters, Sums mode,
                  uint8_t *codes_out, double *corr_out);
#pragma GCC visibility pop
// waits for the slots an asynchronous sharded scan has left busy on this device (all, or only `owner`'s) and books their timing.
// Context mutex held by the caller.
int settle_shard_slots(DeviceCtx *ctx, bbq_index *owner);
// every f32 score of one query on this (single-device) index, to host memory [n_rows]
int dense_scores_host(bbq_index *ix, const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim, float *out);
// multi-device index (bbq_multi.cpp): what the entry points of a handle with ix->multi != nullptr dispatch to
void multi_destroy(bbq_index *ix);
int multi_search_batch(bbq_index *ix, int32_t n_queries, const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim,
                       int64_t k, int32_t *out_idx, float *out_score, int64_t *out_n);
int multi_score_rows(bbq_index *ix, const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim, int64_t row_begin,
                     int64_t row_count, int32_t *out_qcdist, double *out_score64, float *out_score32);
int multi_score_ords(bbq_index *ix, int32_t n_queries, const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim,
                     const int64_t *offsets, const int32_t *ords, int32_t *out_qcdist, double *out_score64, float *out_score32);
int multi_export(bbq_index *ix, uint8_t *codes, double *corr);
int multi_set_option(bbq_index *ix, const char *name, int64_t v);
int multi_get_stats(bbq_index *ix, bbq_stats *out);
// persistence of a multi-device index: every shard as an ordinary file pair + a manifest (bbq_persist.cpp / bbq_multi.cpp)
int multi_save(bbq_index *ix, const char *prefix, const float *centroid, int32_t sim);
int multi_assemble(bbq_index *const *shards, const int32_t *devices, int32_t n_shards, int32_t dim, int32_t index_bits, int64_t n_rows,
                   double centroid_dp, bbq_index **out);
int write_manifest(const char *prefix, int32_t n_shards, const int64_t *bounds, int32_t dim, int32_t index_bits, int32_t sim, int64_t n_rows,
                   double centroid_dp, int64_t pilot_rows, const float *centroid);
std::string shard_file_prefix(const char *prefix, int s);
int multi_reset_stats(bbq_index *ix);
}  // namespace bbq
