"""What bbq_stats.candidates must be after a search call, as a function of the oracle's f32 scores and the call's segment plan - and the
recipe of rows, queries and plans the count is held to.  Numpy and the CPU oracle; nothing here touches a device.
tests/test_candidate_model_cpu.py holds the model to brute force and the recipe to its conditions; tests/test_gpu_candidate_count.py
asserts `stats()["candidates"] == model` for every sweep, with no tolerance.

The answers of a search have k witnesses per query.  The candidate count has one per row above every running threshold: a bound that
rejects a row it must not reject lowers it, a threshold that is stale, late or of the wrong rank raises it.

Everything is in KEY space (key_of_bits, bbq_entry.h): an unsigned image of the f32 score bits that orders like the score, +0 above -0.

  * segmented sweeps (bbq_search_batch, every form): the dense first segment lists its rows; behind a segment that ends at row e the
    threshold is the k_dev-th largest key of rows [0, e) (0 while fewer rows were seen: bbq_finalize_kernel's need_theta block, "M <
    a.k"); a sparse segment lists the rows with key > threshold (exact_key_passes, bbq_kernel_common.h);
  * filtered calls: the same over the accepted rows, on the segments of bbq_filter_plan, the first of them sparse against threshold 0;
  * the pre-sampled single query (search_latency_presampled, bbq_latency.cpp): one threshold from the per-wave top keys of a prefix, one
    list, and the finalize kernel's `ok` chain decides whether that list answers - otherwise the segmented chain's count;
  * a query with a NaN score is flagged and takes the dense path: n rows (|A| under a filter) and one dense fallback
    (dense_search_one, bbq_dense.cpp).

Rules the model takes from the source where the source says otherwise than one would guess:
  * the pre-sampled list answers while it holds at most kFinalizeKeyCap = 12288 entries - not fewer: the only size test of the `ok`
    chain is "m_new <= (uint32_t)kFinalizeKeyCap - tcount" (bbq_finalize_kernel, bbq_kernels.hip) with tcount 0 on a clean slot, and a
    slot's own list is never shorter than that (ensure_slot, bbq_core.cpp: list_cap + flood_cap, flood_cap >= 16384 at these sizes);
  * a list of at most k2 entries proves nothing on that path unless it has exactly k2 ("r.count != (uint32_t)k2", bbq_latency.cpp).

The model REFUSES (Refused) what is not a function of the scores alone: a segment that is not the last and brings more new keys than the
finalize kernel's LDS holds beside the running top keys ("m_use = min(m_new, kFinalizeKeyCap - tcount)": the threshold is then taken over
the entries that fit - in append mode whichever arrived first).  An index with a pilot replica and a multi-device handle are not this
model's either: tests/shard_model.py models a row shard's scan - its lists, its cut and its answer block - and the handle built on it."""
import collections
import functools

import numpy as np

import call_walk as W
import orclib as O
import range_hostile as H
from test_gpu_fast_bound import _queries

F32 = np.float32
TILE, CHUNK = 64, 512
CDP = H.CDP
K_FINALIZE_KEY_CAP = 12288      # kFinalizeKeyCap, bbq_device.h
DENSE_SEGMENT_MAX = 8192        # start_plan, bbq_core.cpp
KEY_PLUS_ZERO = 0x80000000
KEY_PLUS_INF = 0xFF800000
SIMS = (0, 1, 2)
KS = (1, 10, 100)


class Refused(Exception):
    """the count of this call is not a function of the scores and the plan alone"""


def keys_of(s32):
    """key_of_bits (bbq_entry.h) of f32 scores: uint32, ordered like the scores; +0 and -0 differ"""
    b = np.ascontiguousarray(s32, F32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def scores_of_keys(keys):
    k = np.asarray(keys, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(F32)


def kth_largest(keys, k):
    """the k-th largest of the keys, 0 while there are fewer than k"""
    if len(keys) < k:
        return 0
    return int(np.partition(keys, len(keys) - k)[len(keys) - k])


Count = collections.namedtuple("Count", "count split thetas path flagged")      # split: entries listed per segment; thetas: behind each


def k_dev_of(k, n_eff, device_select=1):
    """search_batch_impl, bbq_core.cpp: "c.k_dev = final_k > 0 ? keff + 1 : keff", final_k = keff up to kFinalSelectMax with device_select"""
    keff = min(k, n_eff)
    return keff + 1 if (device_select and keff <= W.K_FINAL_SELECT_MAX) else keff


def segments_of(n, k_dev, first_segment_rows, growth):
    """[(first row, rows, dense)] of an unfiltered call: call_walk.plan_segments, which takes k and plans for k + 1"""
    return W.plan_segments(n, k_dev - 1, first_segment_rows, growth)


def filtered_segments_of(mask, k_dev, first_segment_rows, growth):
    """[(first row, rows, False)] of a filtered call, from bbq_filter_plan's chunks"""
    from bbqlib import capi
    n = len(mask)
    return [(b * CHUNK, min((b + c) * CHUNK, n) - b * CHUNK, False) for b, c, _ in capi.filter_plan(mask, k_dev, first_segment_rows, growth)]


def segmented(s32, segs, k_dev, mask=None):
    """the list a segmented sweep leaves for one query: Count.  s32: the oracle's f32 scores of all rows; mask: the accepted rows"""
    s32 = np.asarray(s32, F32)
    acc = np.ones(len(s32), bool) if mask is None else np.asarray(mask, bool)
    if np.isnan(s32[acc]).any():      # kFlagNaN -> dense_search_one: "stats.candidates += c.filter ? c.n_eff : n"
        return Count(int(acc.sum()), (), (), "dense", True)
    keys = keys_of(s32)
    theta, split, thetas, seen = 0, [], [], np.zeros(0, np.uint32)
    for i, (b, rows, dense) in enumerate(segs):
        if dense and (i != 0 or b != 0 or rows > DENSE_SEGMENT_MAX or mask is not None):
            raise Refused("a dense segment that is not the first, or beyond %d rows" % DENSE_SEGMENT_MAX)
        here = keys[b:b + rows][acc[b:b + rows]]
        listed = len(here) if dense else int((here > theta).sum())
        last = i + 1 == len(segs)
        if not last and listed > K_FINALIZE_KEY_CAP - min(len(seen), k_dev):
            raise Refused("segment %d lists %d entries: more than the threshold selection holds beside %d running keys" % (i, listed, min(len(seen), k_dev)))
        split.append(listed)
        seen = np.concatenate([seen, here])
        theta = kth_largest(seen, k_dev)      # (rows at or below the old threshold cannot be among the k_dev largest: the same statistic)
        thetas.append(theta)
    return Count(sum(split), tuple(split), tuple(thetas), "segments", False)


def presampled(s32, k):
    """the pre-sampled attempt of a single query: (entries listed, does the list answer, threshold), None where the call declines"""
    s32 = np.asarray(s32, F32)
    n = len(s32)
    plan = W.presample_plan(n, k)
    if plan is None:
        return None
    P, per_wave, n_keys = plan
    k2 = min(k, n)
    keys = keys_of(s32)
    if np.isnan(s32[:P]).any():       # bbq_lat_pre_kernel flags the query: "r.flags != 0"
        return 0, False, 0
    waves = np.sort(keys[:P].reshape(-1, TILE), axis=1)[:, TILE - per_wave:]      # the per_wave largest of each wave, duplicates kept
    assert waves.size == n_keys
    theta = kth_largest(waves.ravel(), k2 + 2)
    if np.isnan(s32).any():
        return 0, False, theta
    above = keys[keys > theta]
    listed = len(above)
    if listed > K_FINALIZE_KEY_CAP:   # "m_new <= (uint32_t)kFinalizeKeyCap - tcount"
        return listed, False, theta
    if listed <= k2:                  # take_all: "r.count != (uint32_t)k2"
        sel, edge = above, None
        if listed != k2:
            return listed, False, theta
    else:
        th1 = kth_largest(above, k2 + 1)
        sel, edge = above[above > th1], th1
        if len(sel) != k2:            # "n_sel == (uint32_t)k2"
            return listed, False, theta
    f = scores_of_keys(sel)
    ties = len(np.unique(f)) != len(f) or (edge is not None and (f == scores_of_keys([edge])[0]).any())      # as floats: +0 == -0
    return listed, not ties, theta


def option(opts, name):
    v = opts.get(name)
    return dict(W.OPTIONS)[name][0] if v is None else v


def search_count(fam, scores, k, opts, mask=None, pilot_rows=0, devices=1):
    """the model of ONE call of bbq_search_batch / bbq_search_filtered_batch with these queries (scores: one f32 array per query) on
    an index of family `fam` under the options `opts` ({name: value}, the library's defaults elsewhere): [Count per query]"""
    if pilot_rows or devices != 1:
        raise Refused("an index with a pilot replica, or a multi-device handle: out of scope")
    nq, n = len(scores), len(scores[0])
    n_eff = n if mask is None else int(np.asarray(mask).sum())
    kd = k_dev_of(k, n_eff, option(opts, "device_select"))
    if min(k, n_eff) > W.K_MAX_FAST_K or option(opts, "force_dense"):
        raise Refused("the dense path")
    latency = kd > min(k, n_eff) and nq <= option(opts, "latency_queries")
    growth = option(opts, "latency_growth") if latency else option(opts, "segment_growth")
    fsr = option(opts, "first_segment_rows")
    if mask is not None:
        segs = filtered_segments_of(mask, kd, fsr, growth)
        return [segmented(s, segs, kd, mask) for s in scores]
    segs = segments_of(n, kd, fsr, growth)
    if nq == 1:
        member = W.Member(fam.name, fam.dim, fam.index_bits, 0, fam.query_bits, n, True, None, None, 0, 0)
        if W.single_query_path(member, n, k, opts) == "presampled":
            pre = presampled(scores[0], k)
            if pre is not None and pre[1]:
                return [Count(pre[0], (pre[0],), (pre[2],), "presampled", False)]
    return [segmented(s, segs, kd) for s in scores]


def describe(counts):
    """the failure message's part: per query the count, the path and the split over the segments"""
    return "; ".join("q%d %d %s %s" % (q, c.count, c.path, list(c.split)) for q, c in enumerate(counts))


# ------------------------------------------------------------------------------------------------ the recipe

Family = collections.namedtuple("Family", "name dim index_bits query_bits n")
FAMILIES = (Family("w1", 96, 1, 4, 8192 + 37),              # the fixed width 1
            Family("generic", 200, 1, 4, 8192 + 37),        # the run-time width
            Family("w6", 768, 1, 4, 20480 + 37),            # the row_sums arm, the tiles_per_wave twins, digit planes, the latency kernels
            Family("w8", 1024, 1, 4, 8192 + 37),
            Family("w12", 1536, 1, 4, 8192 + 37),
            Family("multibit", 256, 2, 4, 4096 + 37),       # code sums as x1
            Family("long", 768, 1, 4, 262144 + 512 + 37))   # the pre-sampled chain
BY_NAME = {f.name: f for f in FAMILIES}
LONG = BY_NAME["long"]
LONG_SIMS = (0, 1)                                          # EUCLIDEAN and COSINE
ROW_KINDS = ("ordinary", "hostile")
PLAN = {"first_segment_rows": 1024, "segment_growth": 2, "latency_growth": 2}      # every index but `long`, which keeps the defaults
SEEDS = {}                                                  # a family whose default seed misses a condition of the CPU test gets another


def plan_of(fam):
    return {} if fam.name == "long" else dict(PLAN)


def _seed(fam):
    return SEEDS.get(fam.name, 9500 + 10 * FAMILIES.index(fam))


# The hostile kind, by tile: ordinary, hostile and mixed tiles in turn, and ONE tile each whose additive range is +inf, -inf and 1e300
# (+inf as f32) and one with non-finite intervals - all behind the dense first segment, where the sweep's bound is what lists a row, one
# in every sparse segment of the plan 1024 x 2.  One of each and no more: a row with additionalCorrection +inf or 1e300 scores +inf under
# COSINE and MAXIMUM_INNER_PRODUCT, and k_dev rows at +inf end every threshold there.  No NaN: a NaN score flags the query, which then
# leaves the sparse path (the NaN case has a test of its own).  So of range_hostile's LU_LANES the NaN lane stays out, and the others
# are clipped to +-1e200: an interval end that is infinite as f64 makes every score of its row NaN (the oracle multiplies the width by
# zero terms), and 1e300 does under the query x 1e60; +-1e200 is still infinite as f32, which is what the tile record holds, and every
# product with these queries stays finite as f64.
PLANT_TILES = {"add_pinf": 18, "lu_nonfinite": 27, "add_ninf": 37, "add_1e300": 70}      # segments 1, 1, 2 and 3 of the plan 1024 x 2
EUC_INF_ROW = 20 * TILE + 33
LU_LANES = tuple((lane, col, float(np.clip(v, -1e200, 1e200))) for lane, col, v in H.LU_LANES if not np.isnan(v))


def plant_tiles(fam):
    """{kind: tile} of the family's planted tiles; a family without tile 70 (multibit) has its 1e300 tile in the last segment it has"""
    tiles = (fam.n + TILE - 1) // TILE
    return {kind: t if t < tiles - 1 else 52 for kind, t in PLANT_TILES.items()}


def tile_kinds(fam):
    tiles = (fam.n + TILE - 1) // TILE
    kinds = [H.CYCLE[t % 3] for t in range(tiles)]
    assert kinds[EUC_INF_ROW // TILE] == "mixed"
    for kind, t in plant_tiles(fam).items():
        kinds[t] = kind
    kinds[-1] = "last"
    return tuple(kinds)


@functools.lru_cache(maxsize=None)
def queries(fam, sim, query_bits=None):
    """six queries per similarity as range_hostile.queries builds them: two ordinary, two with the interval x 30, one each x 1e60 and
    x 1e-60 (no f32 images: they keep the f64 bound)"""
    qb = query_bits or fam.query_bits
    qq, qc = _queries(_seed(fam) + 1 + sim + 100 * (qb != fam.query_bits) * qb, 6, fam.dim, qb)
    qc[2:4, :2] *= 30.0
    qc[4, :2] *= 1e60
    qc[5, :2] *= 1e-60
    for a in (qq, qc):
        a.setflags(write=False)
    return qq, qc


@functools.lru_cache(maxsize=None)
def rows(fam, kind):
    """(codes, corr [n, 4]) of the family's ordinary or hostile rows: seeded, read-only"""
    seed, n = _seed(fam), fam.n
    codes, corr = H._ordinary(seed, n, fam)
    if kind == "hostile":
        hcodes, hcorr = H._hostile_rows(seed + 7, n, fam)
        rng = np.random.default_rng(seed + 8)
        hostile = np.zeros(n, bool)
        kinds = tile_kinds(fam)
        for t, tk in enumerate(kinds):
            r = np.arange(t * TILE, min((t + 1) * TILE, n))
            if tk == "hostile":
                hostile[r] = True
            elif tk == "mixed":
                hostile[r] = rng.random(len(r)) < 0.5
            elif tk == "last":
                hostile[r[-1]] = True       # a hostile last lane
        codes[hostile], corr[hostile] = hcodes[hostile], hcorr[hostile]
        for t, tk in enumerate(kinds):
            if tk in H.ADD_PLANTS:
                corr[t * TILE + H.PLANT_LANE, 2] = H.ADD_PLANTS[tk]
            elif tk == "lu_nonfinite":
                for lane, col, v in LU_LANES:
                    corr[t * TILE + lane, col] = v
        corr[EUC_INF_ROW, :3] = 0.0, 0.0, H._euclidean_inf_add(queries(fam, 0)[1][0, 2])      # EUCLIDEAN query 0 scores it +inf
        assert (corr[:, 3] == H.code_sums(codes, fam.index_bits)).all()
    else:
        assert kind == "ordinary"
    for a in (codes, corr):
        a.setflags(write=False)
    return codes, corr


def ordinary_rows(fam, n, salt=0):
    """(codes, corr) of n ordinary rows of the family's shape under its seed + salt: for a recipe that needs more rows than the family has"""
    return H._ordinary(_seed(fam) + salt, n, fam._replace(n=n))


def score(fam, codes, corr, qq, qc, sim, query_bits=None):
    """the oracle's f32 scores of one query over these rows"""
    return O.score_all(codes, corr, fam.dim, qq, qc, query_bits or fam.query_bits, sim, CDP, ib=fam.index_bits)[2]


@functools.lru_cache(maxsize=None)
def scores(fam, kind, sim, query_bits=None):
    """per query the oracle's f32 scores over rows(fam, kind): computed once, read-only"""
    codes, corr = rows(fam, kind)
    qq, qc = queries(fam, sim, query_bits)
    out = tuple(score(fam, codes, corr, qq[q], qc[q], sim, query_bits) for q in range(len(qq)))
    for s in out:
        s.setflags(write=False)
    return out


def accept_sets(fam):
    """a random half; and whole tiles cleared: the first, a plant tile, a chunk's first tile and the ragged last tile"""
    n = fam.n
    cleared = np.ones(n, bool)
    for t in (0, PLANT_TILES["add_pinf"], 3 * CHUNK // TILE, (n - 1) // TILE):
        cleared[t * TILE:(t + 1) * TILE] = False
    return {"a random half": np.random.default_rng(_seed(fam) + 9).random(n) < 0.5, "whole tiles cleared": cleared}


# ------------------------------------------------------------------------------------------------ `long`: the planted ties
TIE_COPIES_AT = (100, 900, 1700, 2500, 3300, 3900)      # inside the first 4000 rows; k + 2 of them take the best row's place


@functools.lru_cache(maxsize=None)
def long_tied(sim, k):
    """(codes, corr, f32 scores of query 0) of `long`'s ordinary rows with k + 2 copies of query 0's best row inside the first 4000 rows:
    the sample's threshold is the best score itself, nothing lies above it, and the call falls through to the segmented chain"""
    assert k + 2 <= len(TIE_COPIES_AT)
    codes, corr = (a.copy() for a in rows(LONG, "ordinary"))
    best = int(np.argmax(scores(LONG, "ordinary", sim)[0]))
    at = np.array(TIE_COPIES_AT[:k + 2])
    codes[at], corr[at] = codes[best], corr[best]
    qq, qc = queries(LONG, sim)
    s = score(LONG, codes, corr, qq[0], qc[0], sim)
    for a in (codes, corr, s):
        a.setflags(write=False)
    return codes, corr, s
