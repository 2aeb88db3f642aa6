// bbq_index.cpp - the per-device context and the index object: creation from rows (written by bbq_append.cpp's path), the
// Infinity-Cache budget of a launch (launch_view), statistics, options.
#include <string.h>
#include <chrono>
#include <memory>
#include "bbq_host.h"

using namespace bbq;

namespace bbq {

std::mutex g_ctx_mu;
DeviceCtx *g_ctx[64] = {nullptr};

// returns the (lazily created, never destroyed) context of a device; call with hipSetDevice(device) done
int get_ctx(int device, DeviceCtx **out) {
  std::lock_guard<std::mutex> lk(g_ctx_mu);
  if (device < 0 || device >= 64) return fail(BBQ_ERR_INVALID_ARG, "device %d out of range", device);
  if (!g_ctx[device]) {
    std::unique_ptr<DeviceCtx> c(new DeviceCtx());  // a context that cannot be completed is taken down again
    for (int i = 0; i < kMaxSlots; ++i) {
      HIPCHK(hipStreamCreateWithFlags(&c->slots[i].stream, hipStreamNonBlocking));
      HIPCHK(c->slots[i].ev0.create());
      HIPCHK(c->slots[i].ev1.create());
      HIPCHK(c->slots[i].ev_done.create(hipEventDisableTiming));
      HIPCHK(c->slots[i].ev_big.create(hipEventDisableTiming));
    }
    HIPCHK(hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking));
    HIPCHK(c->d_aux_flags.alloc(1));
    HIPCHK(hipMemset(c->d_aux_flags, 0, 4));
    HIPCHK(c->h_lat.alloc((size_t)(kLatAnswerOffset + kFinalSelectMax + 8)));
    memset(c->h_lat, 0, c->h_lat.size() * 8);
    HIPCHK(hipHostGetDevicePointer((void **)&c->d_lat, c->h_lat, 0));
    HIPCHK(c->d_pre_keys.alloc((size_t)kLatPreKeys));
    g_ctx[device] = c.release();  // published: from here on it is never destroyed (no HIP call may run at process exit)
  }
  *out = g_ctx[device];
  return BBQ_OK;
}

int ensure_aux_qbuf(DeviceCtx *c, int64_t bytes) {
  HIPCHK(c->d_aux_qbuf.reserve((size_t)bytes));
  return BBQ_OK;
}

int require_devices(int *ndev) {
  *ndev = 0;
  if (hipGetDeviceCount(ndev) != hipSuccess || *ndev <= 0)
    return fail(BBQ_ERR_NO_DEVICE, "no HIP device available: libbbq has no CPU fallback (hipGetDeviceCount found %d)", *ndev);
  return BBQ_OK;
}

int check_device(int device) {
  int ndev = 0;
  const int rc = require_devices(&ndev);
  if (rc != BBQ_OK) return rc;
  if (device < 0 || device >= ndev) return fail(BBQ_ERR_INVALID_ARG, "device %d out of range (0..%d)", device, ndev - 1);
  return BBQ_OK;
}

int open_device(int device, DeviceCtx **ctx) {
  const int rc = check_device(device);
  if (rc != BBQ_OK) return rc;
  HIPCHK(hipSetDevice(device));  // before get_ctx: a new context creates its streams on the current device
  return get_ctx(device, ctx);
}

void set_index_geometry(bbq_index *ix, int32_t dim, int32_t index_bits) {
  ix->geom.dim = dim;
  ix->index_bits = index_bits;
  // a multi-bit index of dimension 1 is the one shape the reference's BATCH scorer accepts (the unpacked byte is read as a
  // packed row, src/batchDotProduct.ts:425-433): it is stored and scored as the packed 1-bit row it is taken for
  ix->geom.store_bits = dim == 1 ? 1 : store_bits_of(index_bits);
  ix->geom.w16 = (pb_of(ix->geom) + 15) / 16;
}

int attach_index(bbq_index *ix, DeviceCtx *ctx, int device, int32_t dim, int32_t index_bits) {
  set_index_geometry(ix, dim, index_bits);
  ix->device = device;
  ix->ctx = ctx;
  ix->slots = ctx->slots;
  return ensure_aux_qbuf(ctx, qbuf_bytes_per_query_w(ix->geom.w16));
}

// The view a launch gets: the stored view + which chunks it loads cache-resident.  The indexes that have launched sweeps on the device
// lately (kCacheWindow) share its 256 MiB Infinity Cache in proportion to their sizes (resident_mb >= 0: that many MiB per launch,
// whatever else is there).  Called with the device context locked.
constexpr int64_t kResidentAutoBytes = 224ll << 20;  // per launch; measured: 192 / 224 / 240 MiB within noise of each other at 10 M x 768, a resident set of 248 MiB gains nothing
constexpr uint64_t kCacheWindow = 100'000'000;  // ns: an index that has launched nothing for 0.1 s is not competing for the cache
static int64_t cache_sharers_bytes(bbq_index *ix, int64_t own) {
  DeviceCtx *c = ix->ctx;
  if (!c) return own;
  const uint64_t now = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
  int64_t all = 0;
  bool found = false;
  for (size_t i = 0; i < c->cache_users.size();) {
    DeviceCtx::CacheUser &u = c->cache_users[i];
    if (u.index == ix) { u.bytes = own; u.tick = now; found = true; }
    if (now - u.tick > kCacheWindow) { c->cache_users.erase(c->cache_users.begin() + (long)i); continue; }
    all += u.bytes;
    ++i;
  }
  if (!found) { c->cache_users.push_back({ix, own, now}); all += own; }
  return all;
}
// One launch sweeps chunks [chunk_begin, chunk_begin + n_chunks) of `sto` once per query of its sub-batch, back to back: what it can
// keep in the cache is a part of ITS range (the launches of a sub-batch run one after the other, each over its own rows).
LaunchView launch_view(bbq_index *ix, const Storage &sto, int64_t chunk_begin, int64_t n_chunks) {
  IndexView v = sto.view;
  v.row_sums = nullptr;  // carried only by the launches of the per-query sparse sweep that are to read it (row_sums_for_launch)
  const int64_t all_chunks = sto.n_chunks();
  if (n_chunks < 0) n_chunks = all_chunks - chunk_begin;
  const int64_t chunk_bytes = (int64_t)kTilesPerChunk * v.geom.tile_stride;
  const int64_t own = ix->main.n_chunks() * (int64_t)kTilesPerChunk * ix->main.view.geom.tile_stride;
  const int64_t all = std::max<int64_t>(1, cache_sharers_bytes(ix, own));
  const int64_t budget = ix->opt_resident_mb >= 0 ? ((int64_t)ix->opt_resident_mb << 20)
                                            : (int64_t)((double)kResidentAutoBytes * ((double)own / (double)all));
  int64_t fit = std::min(n_chunks, budget / std::max<int64_t>(1, chunk_bytes));  // chunks of this launch's range that stay resident
  // an index only a little larger than the budget: its launches are short and overlap (the small ones of the next sub-batch run beside
  // the large one), so their resident sets must fit TOGETHER - the same share of every launch's range
  if (own > budget && own <= budget + budget / 4 && ix->opt_resident_mb < 0) fit = std::min(n_chunks, (int64_t)((double)n_chunks * (double)budget / (double)own));
  int64_t resident_chunks;
  if (fit >= n_chunks) {  // everything this launch reads
    v.resident_share = -1;
    v.resident_tiles = (chunk_begin + n_chunks) * kTilesPerChunk;
    resident_chunks = n_chunks;
  } else if (ix->opt_resident_interleave && n_chunks >= 64) {  // of every 64 chunks the first `share`: cache and HBM deliver side by side
    v.resident_share = fit * 64 / n_chunks;  // rounded down: never more than the budget
    v.resident_tiles = 0;
    resident_chunks = n_chunks * v.resident_share / 64;
  } else {  // the first chunks of the range
    v.resident_share = -1;
    v.resident_tiles = (chunk_begin + fit) * kTilesPerChunk;
    resident_chunks = fit;
  }
  return LaunchView{v, resident_chunks * chunk_bytes};
}

// retires what the device still runs for the index, then deletes it: its storages, dense scores and shard sets go with it.  The
// device context (streams, workspace) stays
void destroy_unlocked(bbq_index *ix) {
  if (!ix) return;
  (void)hipSetDevice(ix->device);
  if (ix->ctx)
    for (size_t i = 0; i < ix->ctx->cache_users.size(); ++i)
      if (ix->ctx->cache_users[i].index == ix) { ix->ctx->cache_users.erase(ix->ctx->cache_users.begin() + (long)i); break; }
  if (ix->ctx) (void)settle_shard_slots(ix->ctx, ix);  // sub-batches of an asynchronous scan that was never waited for
  for (bbq_index::ShardSet &set : ix->shard_set)
    if (set.done) (void)hipEventSynchronize(set.done);  // a batch whose packing was never waited for
  delete ix;
}

}  // namespace bbq

// ================================================================================================ C ABI

extern "C" {

int bbq_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int bbq_index_create_shard(const uint8_t *codes, const double *corr, int64_t n_rows, int32_t dim, int32_t index_bits,
                           double centroid_dp, int64_t row_base, const uint8_t *pilot_codes, const double *pilot_corr,
                           int64_t n_pilot, int32_t device, bbq_index **out) {
  return bbq_index_create_shard_opts(codes, corr, n_rows, dim, index_bits, centroid_dp, row_base, pilot_codes, pilot_corr, n_pilot, device, nullptr, out);
}

int bbq_index_create_shard_opts(const uint8_t *codes, const double *corr, int64_t n_rows, int32_t dim, int32_t index_bits,
                                double centroid_dp, int64_t row_base, const uint8_t *pilot_codes, const double *pilot_corr,
                                int64_t n_pilot, int32_t device, const bbq_index_options *opts, bbq_index **out) {
  clear_error();
  if (!out) return fail(BBQ_ERR_INVALID_ARG, "bbq_index_create: out is null");
  *out = nullptr;
  if (n_rows < 0 || dim <= 0 || row_base < 0 || n_pilot < 0) return fail(BBQ_ERR_INVALID_ARG, "bbq_index_create: bad size");
  if (n_rows > 0 && (!codes || !corr)) return fail(BBQ_ERR_INVALID_ARG, "目标向量集合不能为空");
  if (index_bits < 1 || index_bits > 8) return fail(BBQ_ERR_INVALID_ARG, "indexBits必须在1-8之间");
  if (check_options(opts) != BBQ_OK) return BBQ_ERR_INVALID_ARG;
  if (!dim_supported(dim, dim == 1 ? 1 : store_bits_of(index_bits)))
    return fail(BBQ_ERR_UNSUPPORTED, "dimension %d at indexBits %d: the integer dot product would not fit 31 bits", dim, index_bits);
  if (n_pilot > 0 && (!pilot_codes || !pilot_corr)) return fail(BBQ_ERR_INVALID_ARG, "pilot arrays are null");
  if (n_pilot > 0 && row_base == 0) return fail(BBQ_ERR_INVALID_ARG, "the shard that owns row 0 takes no pilot replica");
  if (n_pilot > 0 && n_pilot > row_base) return fail(BBQ_ERR_INVALID_ARG, "pilot rows must precede the shard (n_pilot <= row_base)");
  if (n_pilot > 0 && n_pilot != row_base && n_pilot % kChunkRows != 0)
    return fail(BBQ_ERR_INVALID_ARG, "n_pilot must be a multiple of %d", kChunkRows);
  if (row_base + n_rows > 0xFFFFFFFFll) return fail(BBQ_ERR_UNSUPPORTED, "more than 2^32 rows");
  DeviceCtx *ctx = nullptr;
  int rc = open_device(device, &ctx);
  if (rc != BBQ_OK) return rc;

  std::unique_ptr<bbq_index> ix(new bbq_index());
  ix->row_base = row_base;
  ix->centroid_dp = centroid_dp;
  ix->has_pilot = n_pilot > 0;
  ix->want_compact = want_compact_of(opts);
  std::lock_guard<std::mutex> lk(ctx->mu);
  rc = attach_index(ix.get(), ctx, device, dim, index_bits);
  if (rc != BBQ_OK) return rc;
  // each storage is an append to an empty one.  Whether the index stores explicit component sums is decided once, over pilot and main
  ix->main.row_id_base = row_base;
  if (ix->has_pilot) rc = append_host_rows(ix.get(), ix->pilot, pilot_codes, pilot_corr, n_pilot, Sums::kDecide);
  const int had = ix->geom.has_x1;
  if (rc == BBQ_OK) rc = append_host_rows(ix.get(), ix->main, codes, corr, n_rows, Sums::kDecide);
  if (rc == BBQ_OK && ix->has_pilot && ix->geom.has_x1 != had) {  // main needs explicit sums but pilot was built without: rebuild the pilot
    ix->pilot = Storage();
    rc = append_host_rows(ix.get(), ix->pilot, pilot_codes, pilot_corr, n_pilot, Sums::kDecide);
  }
  if (rc != BBQ_OK) { destroy_unlocked(ix.release()); return rc; }
  *out = ix.release();
  return BBQ_OK;
}

int bbq_index_create(const uint8_t *codes, const double *corr, int64_t n_rows, int32_t dim, int32_t index_bits,
                     double centroid_dp, int32_t device, bbq_index **out) {
  return bbq_index_create_shard(codes, corr, n_rows, dim, index_bits, centroid_dp, 0, nullptr, nullptr, 0, device, out);
}

void bbq_index_destroy(bbq_index *ix) {
  if (!ix) return;
  if (ix->multi) { multi_destroy(ix); return; }
  if (ix->ctx) {
    std::lock_guard<std::mutex> lk(ix->ctx->mu);
    destroy_unlocked(ix);
  } else {
    destroy_unlocked(ix);
  }
}

int64_t bbq_index_size(const bbq_index *ix) { return ix ? ix->n_rows : 0; }
int32_t bbq_index_dimension(const bbq_index *ix) { return ix ? ix->geom.dim : 0; }
int32_t bbq_index_bytes_per_row(const bbq_index *ix) { return ix ? bytes_per_row_of(ix->geom) : 0; }
int32_t bbq_index_bits(const bbq_index *ix) { return ix ? ix->index_bits : 0; }

int bbq_get_stats(bbq_index *ix, bbq_stats *out) {
  if (!ix || !out) return fail(BBQ_ERR_INVALID_ARG, "bbq_get_stats: null");
  if (ix->multi) return multi_get_stats(ix, out);
  if (ix->ctx) {
    std::lock_guard<std::mutex> lk(ix->ctx->mu);
    int prev = -1;  // a getter must not change the calling thread's current device
    (void)hipGetDevice(&prev);
    HIPCHK(hipSetDevice(ix->device));
    int rc = settle_shard_slots(ix->ctx, ix);  // timings of an asynchronous scan are booked when its slots are retired
    if (prev >= 0 && prev != ix->device) (void)hipSetDevice(prev);
    if (rc != BBQ_OK) return rc;
    *out = ix->stats;
    return BBQ_OK;
  }
  *out = ix->stats;
  return BBQ_OK;
}
int bbq_reset_stats(bbq_index *ix) {
  if (!ix) return fail(BBQ_ERR_INVALID_ARG, "bbq_reset_stats: null");
  if (ix->multi) return multi_reset_stats(ix);
  ix->stats = bbq_stats{};
  return BBQ_OK;
}

int bbq_set_option(bbq_index *ix, const char *name, int64_t v) {
  if (!ix || !name) return fail(BBQ_ERR_INVALID_ARG, "bbq_set_option: null");
  if (ix->multi) return multi_set_option(ix, name, v);
  const std::string n(name);
  if (n == "batch_queries" && v >= 0 && v <= 1024) ix->opt_batch = (int)v;  // 0: by index size
  else if (n == "pipeline_slots" && v >= 1 && v <= kMaxSlots) ix->opt_slots = (int)v;
  else if (n == "segment_growth" && v >= 2 && v <= 1024) ix->opt_growth = (int)v;
  else if (n == "first_segment_rows" && v >= 1024 && v <= 8192 && v % kChunkRows == 0) ix->opt_s0 = v;
  else if (n == "resident_interleave" && (v == 0 || v == 1)) ix->opt_resident_interleave = (int)v;
  else if (n == "resident_mb" && v >= -1 && v <= 1 << 20) ix->opt_resident_mb = (int)v;
  else if (n == "l2_share" && (v == -1 || (v >= 1 && v <= 32 && (v & (v - 1)) == 0))) ix->opt_l2_share = (int)v;
  else if (n == "fast_bound" && (v == 0 || v == 1)) ix->opt_fast_bound = (int)v;
  else if (n == "row_sums" && v >= -1 && v <= 1) ix->opt_row_sums = (int)v;
  else if (n == "group_scratch_mb" && v >= 1 && v <= 8192) ix->opt_group_scratch_mb = (int)v;
  else if (n == "maxsim_fused" && v >= -1 && v <= 1) ix->opt_maxsim_fused = (int)v;
  else if (n == "digit_planes" && v >= -1 && v <= 1) ix->opt_digit_planes = (int)v;
  else if (n == "tiles_per_wave" && (v == -1 || v == 1 || v == 2 || v == 4 || v == 8)) ix->opt_tiles_per_wave = (int)v;
  else if (n == "replay_threads" && v >= 1 && v <= 256) ix->opt_replay_threads = (int)v;
  else if (n == "force_dense" && (v == 0 || v == 1)) ix->opt_force_dense = (int)v;
  else if (n == "device_select" && (v == 0 || v == 1)) ix->opt_device_select = (int)v;
  else if (n == "latency_queries" && v >= 0 && v <= 1024) ix->opt_latency_queries = (int)v;
  else if (n == "append_last" && (v == 0 || v == 1)) ix->opt_append_last = (int)v;
  else if (n == "latency_fused" && (v == 0 || v == 1)) ix->opt_latency_fused = (int)v;
  else if (n == "latency_presample" && (v == 0 || v == 1)) ix->opt_latency_presample = (int)v;
  else if (n == "latency_growth" && v >= 2 && v <= 4096) ix->opt_latency_growth = (int)v;
  else if (n == "sweep_share" && (v == 1 || v == 4 || v == 8 || v == 32)) ix->opt_share = (int)v;
  else if (n == "flood_rows" && v >= 0 && v <= (1 << 24)) ix->opt_flood = (v + 1023) / 1024 * 1024;
  else return fail(BBQ_ERR_INVALID_ARG, "bbq_set_option: unknown option or value out of range: %s=%lld", name, (long long)v);
  return BBQ_OK;
}

}  // extern "C"
