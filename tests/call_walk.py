"""Seeded random walks of calls of every kind over several live indexes on ONE device, and what each of them is there to reach.  Pure
numpy: no device, no library - tests/test_call_walk_cpu.py asserts what the default walks cover, tests/test_gpu_call_walk.py plays them
and holds every answer to the oracle.

What the walks are after is the state a device context (DeviceCtx, bbq_host.h) carries from one call into the next, whatever index the
next call is made on: the pipeline slots' grow-only buffers and the capacities the kernels take as strides, Slot::ctrl_clean, the
latency answer block and its sequence word, sub-batches of an asynchronous sharded scan that stay busy across API calls, the scratch
d_span / d_range / d_gather and the staging inside bbq_vectors, the cache bookkeeping and the options.  So the members of the CAST live
for a whole walk, a step names a member and a kind of call, and a walk is made of five things, shuffled block by block:

  * the TRANSITIONS: short fixed sequences the code marks as delicate - each entry's comment names the line it stems from;
  * the option sequences: [a call, set_option, the same call] for every listed value of the options of this walk (OPTIONS, dealt to
    the seeds in turn); the last value stays in force for the rest of the walk, or until a block that is about a chain resets it;
  * the member tour: one call of every kind a member admits (ADMITS), dealt to the seeds in turn;
  * the in-flight tour: a shard batch begun, calls of other kinds, the batch collected - every kind, dealt to the seeds in turn;
  * FREE_STEPS freely drawn steps, about a quarter of the walk.

A step is a dict: "kind", "member", "via" (the block it came from) and the kind's own shape parameters, all concrete except what depends
on scores (a range threshold is given as a rank).  describe(step) prints one as a line: the listing up to a failing step replays it.

The cast.  The single-query chains exist for rows of 6, 8 and 12 16-byte chunks only (latency_path_supported,
bbq_latency_kernels.hip): a 64-dimensional index never runs either of them.  So `long`, the member that is there for the pre-sampled
chain, is 768-dimensional - 6 chunks, the narrowest width that has the chains - and `ties`, at 64 dimensions, is where single-query calls
take the general path by themselves."""
import zlib
from collections import namedtuple

import numpy as np

TILE, CHUNK = 64, 512
K_FINAL_SELECT_MAX = 1024     # kFinalSelectMax, bbq_device.h: the largest k the finalize launch selects and sorts itself
K_MAX_FAST_K = 4096           # kMaxFastK, bbq_host.h: beyond it the dense path
K_LAT_PRE_KEYS = 12288        # kLatPreKeys, bbq_device.h
PRESAMPLE_MIN_ROWS = 262144   # search_latency_presampled, bbq_latency.cpp: "N < 262144"
LATENCY_W16 = (6, 8, 12)      # latency_path_supported, bbq_latency_kernels.hip
TOKEN_BLOCK = 32              # kMaxSimTokenBlock (bbq_maxsim_token_block); the GPU test asserts it
EUCLIDEAN, COSINE, MAXIMUM_INNER_PRODUCT = 0, 1, 2
DEFAULT_SEEDS = 3             # BBQ_CALL_WALK_SEEDS asks for more
FREE_STEPS = 60               # freely drawn steps a walk adds to its blocks: about a quarter of its steps

# source: "seeded" rows made by the GPU test's recipe, "synthetic" codes and corrections drawn directly (no fp32 rows), or a golden
# fixture; rows: the slice of the source the member holds; pilot: rows of the source in front of it that it carries as a replica
Member = namedtuple("Member", "name dim ib sim qb n0 compact source rows pilot pool")
CAST = {
    # digit planes, tiles-per-wave 8, row_sums, the fused MaxSim kernel, sweep_share 32 with 70 queries, the filtered matrix-core sweep,
    # and - six chunks wide - the segmented single-query chain
    "wide": Member("wide", 768, 1, COSINE, 4, 6200, True, "seeded", None, 0, 48),
    # equal scores in and at the edge of every answer
    "ties": Member("ties", 64, 1, COSINE, 4, 3000, False, "ties_cos_qb4", None, 0, 48),
    "multi": Member("multi", 96, 4, EUCLIDEAN, 4, 200, True, "ib4_96d_euc_qb4", None, 0, 16),
    # the smallest index the pre-sampled chain runs on; queries 0..2 of its pool have their best row several times
    "long": Member("long", 768, 1, MAXIMUM_INNER_PRODUCT, 4, PRESAMPLE_MIN_ROWS + CHUNK, True, "synthetic", None, 0, 8),
    # a non-root shard over the second half of ties' rows with a pilot replica of the first 1024, and the root shard in front of it
    "shard": Member("shard", 64, 1, COSINE, 4, 1500, False, "ties_cos_qb4", (1500, 3000), 1024, 48),
    "root": Member("root", 64, 1, COSINE, 4, 1500, False, "ties_cos_qb4", (0, 1500), 0, 48),
}
TIED_QUERIES = 3              # of `long`: pool queries 0..2
WITH_VECTORS = "wide"         # the member that has its fp32 rows on the device beside it (B.Vectors)
APPEND_POOL = {"ties": 3000, "multi": 200}    # members that grow: appended rows are drawn from the fixture's rows, with replacement
MAX_ROWS = {"ties": 6000, "multi": 1500}

KINDS = ("search", "search_batch", "search_filtered_batch", "search_raw_batch", "range", "search_spans", "search_spans_filtered",
         "search_grouped", "search_maxsim", "maxsim_groups", "rerank", "maxsim_rerank", "score_rows", "score_ords", "search_ords",
         "shard_scan", "shard_begin", "shard_wait", "set_option", "stats", "reset_stats", "refused", "recreate", "append", "save")
READ_ONLY = tuple(k for k in KINDS if k not in ("append", "recreate", "set_option", "shard_scan", "shard_begin", "shard_wait", "save", "reset_stats"))
D_SPAN_USERS = ("search_spans", "search_spans_filtered", "search_grouped", "search_maxsim", "maxsim_groups", "maxsim_rerank")   # bbq_host.h, DeviceCtx::d_span

_ROOT_KINDS = ("search", "search_batch", "search_filtered_batch", "search_raw_batch", "range", "search_spans", "search_spans_filtered", "search_grouped",
               "search_maxsim", "maxsim_groups", "score_rows", "score_ords", "search_ords", "set_option", "stats", "reset_stats", "refused", "recreate", "save")
ADMITS = {
    "wide": _ROOT_KINDS + ("rerank", "maxsim_rerank"),
    "ties": _ROOT_KINDS + ("append",),
    "multi": _ROOT_KINDS + ("append",),
    # 25 MB of rows: the calls that walk all of them for every query stay few, and no group set
    "long": ("search", "search_batch", "search_filtered_batch", "range", "search_spans", "score_ords", "stats", "set_option", "refused"),
    "shard": ("shard_scan", "shard_begin", "shard_wait", "stats", "set_option", "recreate", "save", "refused"),
    # the root shard is an ordinary index: it searches, and a batch of its own may be in flight when it is asked to append
    "root": ("search", "search_batch", "shard_scan", "shard_begin", "shard_wait", "stats", "recreate", "refused"),
}

# include/bbq.h, bbq_set_option: (name, the values a walk sets - the first is the default, None where the default depends on the host)
OPTIONS = (
    ("batch_queries", (0, 32, 7)), ("pipeline_slots", (3, 1, 4)), ("segment_growth", (8, 2, 64)), ("first_segment_rows", (4096, 1024, 8192)),
    ("resident_mb", (-1, 0, 16)), ("resident_interleave", (1, 0)), ("l2_share", (-1, 1, 4)), ("row_sums", (-1, 0, 1)), ("digit_planes", (-1, 0, 1)),
    ("tiles_per_wave", (-1, 1, 2, 4, 8)), ("group_scratch_mb", (256, 1)), ("maxsim_fused", (-1, 0, 1)), ("fast_bound", (1, 0)),
    ("replay_threads", (None, 1, 4)), ("flood_rows", (262144, 1 << 20)), ("force_dense", (0, 1)), ("sweep_share", (1, 4, 8, 32)),
    ("device_select", (1, 0)), ("latency_queries", (4, 0, 1)), ("latency_growth", (64, 2, 4096)), ("append_last", (1, 0)),
    ("latency_fused", (1, 0)), ("latency_presample", (1, 0)),
)
# the call an option is set in front of and behind: (member, kind, shape overrides)
OPTION_CALLS = {
    "batch_queries": ("ties", "search_batch", {"nq": 70, "k": 10}), "pipeline_slots": ("wide", "search_batch", {"nq": 130, "k": 10}),
    "segment_growth": ("wide", "search_batch", {"nq": 5, "k": 10}), "first_segment_rows": ("wide", "search_batch", {"nq": 5, "k": 100}),
    "resident_mb": ("wide", "search_batch", {"nq": 33, "k": 10}), "resident_interleave": ("wide", "search_batch", {"nq": 5, "k": 10}),
    "l2_share": ("wide", "search_batch", {"nq": 33, "k": 10}), "row_sums": ("wide", "search_batch", {"nq": 5, "k": 10}),
    "digit_planes": ("wide", "search_batch", {"nq": 5, "k": 10}), "tiles_per_wave": ("wide", "search_batch", {"nq": 5, "k": 100}),
    "group_scratch_mb": ("wide", "search_grouped", {"nq": 33}), "maxsim_fused": ("wide", "search_maxsim", {}),
    "fast_bound": ("wide", "search_batch", {"nq": 5, "k": 10}), "replay_threads": ("ties", "search_batch", {"nq": 33, "k": 100}),
    "flood_rows": ("ties", "search_batch", {"nq": 5, "k": 10}), "force_dense": ("multi", "search_batch", {"nq": 5, "k": 10}),
    "sweep_share": ("wide", "search_batch", {"nq": 70, "k": 10}), "device_select": ("ties", "search_batch", {"nq": 5, "k": 10}),
    "latency_queries": ("wide", "search_batch", {"nq": 2, "k": 10}), "latency_growth": ("wide", "search", {"k": 10}),
    "append_last": ("wide", "search", {"k": 10}), "latency_fused": ("wide", "search", {"k": 100}), "latency_presample": ("long", "search", {"k": 10}),
}

# a call that must fail before any launch: (what, the member it is made on, the documented code's name in capi)
REFUSALS = (
    ("filter_of_another_size", "ties", "ERR_INVALID_ARG"),        # search_batch_impl, bbq_core.cpp: "the filter was made for an index of ..."
    ("negative_k", "wide", "ERR_NEGATIVE_K"),                     # validate_query_args, bbq_query.cpp
    ("search_on_a_shard", "shard", "ERR_INVALID_ARG"),            # search_batch_impl: "bbq_search on a non-root shard"
    ("group_outside_the_set", "ties", "ERR_INVALID_ARG"),         # check_maxsim_cand_lists, bbq_maxsim_groups.cpp
    ("rerank_row_out_of_range", "wide", "ERR_INVALID_ARG"),       # bbq_rerank_scores, bbq_rerank.cpp
    ("wait_with_nothing_in_flight", "shard", "ERR_INVALID_ARG"),  # bbq_shard_scan_wait, bbq_shard.cpp: "no batch in flight"
    ("third_begin", "shard", "ERR_INVALID_ARG"),                  # bbq_shard_scan_begin, bbq_shard.cpp: "two batches are already in flight"
    ("append_with_unwaited_batch", "root", "ERR_INVALID_ARG"),    # include/bbq.h, append section
)



def refusals_of(member):
    """the refusals that can be asked of a member: its own, and a negative k of every member that searches"""
    return [w for w, mem, _ in REFUSALS if mem == member or (w == "negative_k" and "search_batch" in ADMITS[member])]


NQS = (1, 2, 5, 33, 70, 130)
RAGGED = (1, 2, 0, 63, 64, 65, 0, 7, 20, 3, 130)   # the sizes a ragged group set cycles through


def tiles_of(rows):
    return (int(rows) + TILE - 1) // TILE


def w16_of(dim, ib=1):
    """16-byte chunks of a packed 1-bit row (TileGeom::w16)"""
    return (dim * ib + 127) // 128


def mask_of(member, n, which):
    """the accept mask of a member's "sparse" (2 %) or "dense" (90 %) filter at n rows; row 0 is always accepted"""
    rng = np.random.default_rng([zlib.crc32(member.encode()), int(n), 0 if which == "sparse" else 1])
    m = rng.random(n) < (0.02 if which == "sparse" else 0.9)
    m[0] = True
    return m


def offsets_of(n):
    """ragged groups over n rows: RAGGED over and over, the last group cut at n"""
    off, i = [0], 0
    while off[-1] < n:
        off.append(min(n, off[-1] + RAGGED[i % len(RAGGED)]))
        i += 1
    return np.array(off, np.int64)


def group_mask(member, n, which):
    """the rows that exist for a member's group set: all of them ("ragged"), or the dense filter's ("filtered")"""
    return np.ones(n, bool) if which == "ragged" else mask_of(member, n, "dense")


def live_groups(off, mask):
    has = np.add.reduceat(np.concatenate([mask, [False]]).astype(np.int64), np.minimum(off[:-1], len(mask)))
    return np.flatnonzero((np.diff(off) > 0) & (has > 0)).astype(np.int64)


def queries_of(step, pool):
    """the pool queries of a step: q0, q0 + 1, ... modulo the pool"""
    return (int(step["q0"]) + np.arange(int(step["nq"]))) % pool


def tokens_of(step, pool):
    """per query of a MaxSim step the pool vectors that are its tokens"""
    return [(int(t0) + np.arange(int(cnt))) % pool for t0, cnt in step["tokens"]]


# ---------------------------------------------------------------------------------------------------- the host rules the cast leans on
def digit_planes_apply(m, filtered=False, row_sums=-1, digit_planes=-1, resident_mb=-1):
    """digit_planes_for_call + row_sums_for_launch (bbq_core.cpp), row_sums_fit (bbq_device.h) and digit_twin (bbq_scan_body.h) at 4 planes"""
    reads_sums = (resident_mb != 0) if row_sums < 0 else row_sums != 0
    fits = m.compact and m.dim * ((1 << m.ib) - 1) <= 65535
    w = w16_of(m.dim)
    twin = m.ib == 1 and (w == 6 or (not filtered and w in (8, 12)))
    return digit_planes != 0 and m.ib == 1 and m.qb in (3, 4) and reads_sums and fits and twin


def tiles_per_wave_of(m, option=-1):
    """tiles_per_wave_for (bbq_core.cpp); tiles_twin (bbq_scan_body.h): unfiltered, 6, 8 or 12 chunks"""
    if not digit_planes_apply(m) or w16_of(m.dim) not in (6, 8, 12):
        return 1
    return option if option > 0 else {6: 8, 8: 8}.get(w16_of(m.dim), 1)


def latency_supported(m):
    """latency_path_supported (bbq_latency_kernels.hip) for a query of 4 planes: kLatPlaneMax = 96 is not reached at these widths"""
    return m.ib == 1 and w16_of(m.dim) in LATENCY_W16


def presample_plan(n, k):
    """search_latency_presampled (bbq_latency.cpp): (P, per_wave, n_keys) of a call it takes, None where it declines"""
    k2 = min(k, n)
    if k2 < 1 or k2 > K_FINAL_SELECT_MAX or n < PRESAMPLE_MIN_ROWS:
        return None
    P = max(((k2 + 2) * n // 6000 + CHUNK - 1) // CHUNK * CHUNK, 8192)
    if P > n // 4:
        return None
    per_wave = 1 if P // TILE >= 8 * (k2 + 2) else 4
    if P // TILE * per_wave > K_LAT_PRE_KEYS:
        per_wave = 1
    n_keys = P // TILE * per_wave
    if n_keys > K_LAT_PRE_KEYS or n_keys < k2 + 2:
        return None
    return P, per_wave, n_keys


def plan_segments(n, k, first_segment_rows=4096, growth=64):
    """build_plan + add_storage_segments (bbq_core.cpp) of an unfiltered call on an index without a pilot replica, k_dev = k + 1:
    [(first row, rows, dense)]"""
    kd = min(k, n) + 1
    s0 = min(max(first_segment_rows, (4 * kd + CHUNK - 1) // CHUNK * CHUNK), 8192)
    rows = min(s0, n)
    segs, b = [(0, rows, True)], rows
    while b < n:
        e, nb = n, b * growth // CHUNK * CHUNK
        if b > 0 and nb > b and nb <= n // 2:
            e = nb
        segs.append((b, e - b, False))
        b = e
    return segs


def matrix_core_sweep(m, n_eff, k, opts, query_bits=None):
    """does a batch search sweep on the matrix cores?  enqueue_subbatch (bbq_core.cpp): "use_mfma = !ext && c.share == 32 && c.maxq <= 127
    && ix->geom.store_bits == 1", every query's score uniforms finite (mfma_query_ok, bbq_query.cpp: any query quantized from finite
    values); search_batch_impl: not on the dense path, maxq 15 for a query of at most four planes or 2^query_bits - 1 with a feed"""
    o = lambda name, default: default if opts.get(name) is None else opts[name]
    maxq = 15 if (query_bits or m.qb) <= 4 else 255
    return o("sweep_share", 1) == 32 and maxq <= 127 and m.ib == 1 and not o("force_dense", 0) and min(k, n_eff) <= K_MAX_FAST_K


def single_query_path(m, n, k, opts):
    """which way bbq_search_batch takes ONE query (search_batch_impl, bbq_core.cpp): "dense", "presampled", "chain" or "general".
    "presampled" is where the call starts: a query the chain cannot prove goes on to "chain\""""
    o = lambda name, default: default if opts.get(name) is None else opts[name]
    keff = min(k, n)
    if keff > K_MAX_FAST_K or o("force_dense", 0):
        return "dense"
    latency = keff <= K_FINAL_SELECT_MAX and o("device_select", 1) and 1 <= o("latency_queries", 4)
    if not latency or not o("latency_fused", 1) or o("sweep_share", 1) != 1 or m.pilot or not latency_supported(m):
        return "general"
    if o("latency_presample", 1) and presample_plan(n, k) is not None:
        return "presampled"
    segs = plan_segments(n, k, o("first_segment_rows", 4096), o("latency_growth", 64))
    return "chain" if o("append_last", 1) and segs[0][2] and not any(d for _, _, d in segs[1:]) else "general"


# ---------------------------------------------------------------------------------------------------- the draws
class State:
    """what a walk knows of the cast while it draws: sizes, the rows of the members that grow, options in force, batches in flight"""

    def __init__(self):
        self.n = {name: m.n0 for name, m in CAST.items()}
        self.src = {name: np.arange(n, dtype=np.int64) for name, n in APPEND_POOL.items()}
        self.options = {name: {} for name in CAST}
        self.inflight = {name: [] for name in CAST}

    def in_flight(self):
        return sum(len(v) for v in self.inflight.values())


class _Draw:
    def __init__(self, rng, seed):
        self.rng, self.seed, self.st = rng, seed, State()

    def pick(self, options):
        return options[int(self.rng.integers(len(options)))]

    def q0(self, member):
        return int(self.rng.integers(CAST[member].pool))

    def ks(self, member, extra=()):
        n = self.st.n[member]
        ks = [1, 10, 100, K_FINAL_SELECT_MAX, K_FINAL_SELECT_MAX + 1]
        if member != "long":          # `long`: every heap of the oracle and every dense answer walks 262 656 rows, so k stays within 1025
            ks += [K_MAX_FAST_K, K_MAX_FAST_K + 1, n, n + 3]
        return ks + list(extra)

    def spans(self, n, limit):
        """the spans of one query: ascending, disjoint; none, one row, everything, tile and chunk edges, random pieces"""
        rng = self.rng
        shape = self.pick(["none", "one_row", "everything", "edges", "random", "random", "random"])
        if shape == "none":
            return np.zeros((0, 2), np.int64)
        if shape == "one_row":
            r = int(rng.integers(n))
            return np.array([[r, r + 1]], np.int64)
        if shape == "everything" and n <= limit:
            return np.array([[0, n]], np.int64)
        if shape == "edges":
            cuts = sorted({c for c in (0, 1, 63, 64, 65, 511, 512, 513, 1024, n) if c <= n})
        else:
            lo = int(rng.integers(0, max(1, n - limit)))
            cuts = sorted({int(c) for c in rng.integers(lo, min(n, lo + limit) + 1, 2 * int(rng.integers(1, 4)))})
        pairs = [(a, b) for a, b in zip(cuts[::2], cuts[1::2])]
        return np.array(pairs, np.int64).reshape(-1, 2)

    def tokens(self, member, nq):
        pool = CAST[member].pool
        return [(int(self.rng.integers(pool)), int(self.pick([1, TOKEN_BLOCK, TOKEN_BLOCK + 1]))) for _ in range(nq)]

    def cand_lists(self, member, groups, nq):
        n = self.st.n[member]
        live = live_groups(offsets_of(n), group_mask(member, n, groups))
        out = []
        for _ in range(nq):
            shape = self.pick(["none", "one", "some_with_duplicates", "some_with_duplicates", "every_live_group"])
            if shape == "none":
                out.append(np.zeros(0, np.int64))
            elif shape == "one":
                out.append(live[[int(self.rng.integers(len(live)))]])
            elif shape == "every_live_group" and len(live) <= 300:
                out.append(live[::-1].copy())
            else:
                some = live[self.rng.integers(0, len(live), int(self.rng.integers(2, 12)))]
                out.append(np.concatenate([some, some[:2]]))
        return out

    def step(self, kind, member, via="free", **over):
        """one step of `kind` on `member`, its shape drawn from the kind's edge sets; `over` fixes what a block needs fixed"""
        st, rng, m, n = self.st, self.rng, CAST[member], self.st.n[member]
        s = {"kind": kind, "member": member, "via": via}
        if kind == "search":
            s.update(q0=self.q0(member), nq=1, k=self.pick([1, 10, 100, K_FINAL_SELECT_MAX, K_FINAL_SELECT_MAX + 1]))
        elif kind == "search_batch":
            s.update(q0=self.q0(member), nq=self.pick(NQS), k=self.pick(self.ks(member)))
        elif kind == "search_filtered_batch":
            s.update(q0=self.q0(member), nq=self.pick([1, 5, 33, 70]), filter=self.pick(["sparse", "dense"]))
            count = int(mask_of(member, n, s["filter"]).sum())
            s["k"] = self.pick([1, 10, 100, K_FINAL_SELECT_MAX + 1] if member == "long" else [1, 10, 100, count, count + 3])
        elif kind == "search_raw_batch":
            s.update(q0=self.q0(member), nq=self.pick([5, 70]), k=self.pick([1, 10, 100]))     # 70: beyond 64 raw queries, the feed
        elif kind == "range":
            nq = self.pick([1, 5, 33])
            ranks = [0, 9, 999, -1] if member == "long" else [0, 9, n // 2, n - 1, -1]       # -1: a threshold no row reaches
            s.update(q0=self.q0(member), nq=nq, filter=self.pick([None, "sparse", "dense"]), ranks=[int(self.pick(ranks)) for _ in range(nq)])
        elif kind in ("search_spans", "search_spans_filtered"):
            nq = self.pick([1, 5, 33])
            limit = 20000 if member == "long" else n
            s.update(q0=self.q0(member), nq=nq, k=self.pick([1, 10, 100, K_FINAL_SELECT_MAX] + ([] if member == "long" else [K_MAX_FAST_K, K_MAX_FAST_K + 1])), spans=[self.spans(n, limit) for _ in range(nq)])
            if kind == "search_spans_filtered":
                s["filter"] = self.pick(["sparse", "dense"])
        elif kind == "search_grouped":
            s.update(q0=self.q0(member), nq=self.pick([1, 5, 33]), groups=self.pick(["ragged", "filtered"]))
            L = len(live_groups(offsets_of(n), group_mask(member, n, s["groups"])))
            s["k"] = self.pick([1, 10, L, L + 1])
        elif kind == "search_maxsim":
            s.update(tokens=self.tokens(member, self.pick([1, 2, 3])), k=self.pick([1, 10]), groups=self.pick(["ragged", "filtered"]))
        elif kind == "maxsim_groups":
            nq = self.pick([1, 2, 3])
            s.update(tokens=self.tokens(member, nq), groups=self.pick(["ragged", "filtered"]), k=self.pick([1, 3, 40]))
            s["cand"] = self.cand_lists(member, s["groups"], nq)
        elif kind == "rerank":
            shape = self.pick(["long_lists", "one_row", "mixed"])
            nq = {"long_lists": 3, "one_row": 1, "mixed": 5}[shape]
            lens = {"long_lists": [1500, 700, 64], "one_row": [1], "mixed": [0, 1, 65, 4, 200]}[shape]
            s.update(shape=shape, q0=self.q0(member), nq=nq, rows=[rng.integers(0, n, c).astype(np.int32) for c in lens],
                     true_sim=int(self.pick([0, 1, 2])), k=10, factor=int(self.pick([1, 3])), selector=int(self.pick([0, 1])))
        elif kind == "maxsim_rerank":
            nq = self.pick([1, 2])
            s.update(tokens=self.tokens(member, nq), groups=self.pick(["ragged", "filtered"]), true_sim=int(self.pick([0, 1, 2])), k=3, factor=2,
                     selector=int(self.pick([0, 1])))
            live = live_groups(offsets_of(n), group_mask(member, n, s["groups"]))
            s["cand"] = [np.concatenate([c, c[:1]]) for c in (live[rng.integers(0, len(live), int(rng.integers(1, 7)))] for _ in range(nq))]
        elif kind == "score_rows":
            s.update(q0=self.q0(member), nq=1)
        elif kind == "score_ords":
            s.update(q0=self.q0(member), nq=1, ords=rng.integers(0, n, self.pick([1, 150, 5000])).astype(np.int32))
        elif kind == "search_ords":
            nq = self.pick([1, 5])
            lists = [rng.integers(0, n, self.pick([0, 1, 65, 700])).astype(np.int32) for _ in range(nq)]
            s.update(q0=self.q0(member), nq=nq, lists=lists, k=self.pick([1, 10, max(len(l) for l in lists) + 1]))
        elif kind in ("shard_scan", "shard_begin"):
            s.update(q0=self.q0(member), nq=self.pick([1, 5, 33]), k=self.pick([1, 10, 100]))
        elif kind == "set_option":
            name, values = self.pick([o for o in OPTIONS if o[0] != "force_dense"])   # (a free draw never ends a member's sweeps for good)
            s.update(option=name, value=self.pick([v for v in values if v is not None and v != st.options[member].get(name, values[0])]))
        elif kind == "refused":
            what = over.get("what") or self.pick([w for w in refusals_of(member) if self.refusable(w)])
            s.update(what=what, code=dict((w, c) for w, _, c in REFUSALS)[what], q0=self.q0(member))
        elif kind == "append":
            s["rows"] = rng.integers(0, APPEND_POOL[member], self.pick([1, 100, 513])).astype(np.int64)
        elif kind not in ("shard_wait", "stats", "reset_stats", "recreate", "save"):
            raise ValueError(kind)
        s.update(over)
        return s

    def refusable(self, what):
        """the refusals that need something in flight exist only then"""
        st = self.st
        if what == "third_begin":
            return len(st.inflight["shard"]) == 2
        if what == "append_with_unwaited_batch":
            return len(st.inflight["root"]) > 0
        if what == "wait_with_nothing_in_flight":
            return len(st.inflight["shard"]) == 0
        return True

    def admissible(self, kind, member):
        st = self.st
        if kind not in ADMITS[member]:
            return False
        if kind == "shard_begin":
            return len(st.inflight[member]) < 2
        if kind == "shard_wait":
            return len(st.inflight[member]) > 0
        if kind == "shard_scan":     # begin + wait, and waits are taken in begin order: the synchronous form is for an idle index
            return len(st.inflight[member]) == 0
        if kind == "append":
            return st.n[member] + 513 <= MAX_ROWS[member]
        if kind == "refused":
            return any(self.refusable(w) for w in refusals_of(member))
        return True

    def done(self, s):
        """the state behind a step"""
        st, kind, member = self.st, s["kind"], s["member"]
        if kind == "shard_begin":
            st.inflight[member].append(dict(s))
        elif kind == "shard_wait":
            st.inflight[member].pop(0)
        elif kind == "recreate":           # a new index: default options, nothing in flight, the rows it had
            st.inflight[member], st.options[member] = [], {}
        elif kind == "set_option":
            st.options[member][s["option"]] = s["value"]
        elif kind == "append":
            st.src[member] = np.concatenate([st.src[member], s["rows"]])
            st.n[member] = len(st.src[member])
        return s


# ---------------------------------------------------------------------------------------------------- the delicate transitions
# name -> the (kind, member) pairs of its steps, in order; member None: drawn.  A step of a transition repeats the call of the step named
# by "same" where the point is the same call again.
TRANSITIONS = {
    # enqueue_subbatch dirties the slot's control words (bbq_core.cpp, "s.ctrl_clean = false" behind its copy); prepare_latency_slot
    # (bbq_latency.cpp) clears them only when the flag says so
    "general_then_latency": (("search_batch", "wide"), ("search", "wide")),
    "latency_then_general_then_latency": (("search", "wide"), ("search_batch", "wide"), ("search", "wide")),
    # search_latency_presampled hands a query it cannot prove to search_latency_chain on the same slot ("r.count != (uint32_t)k2", bbq_latency.cpp);
    # both raise ctx->lat_seq and read ctx->h_lat, which the next index's chain shares
    "presampled_unproven_then_chain_then_another_index": (("search", "long"), ("search", "wide"), ("search", "long")),
    # Slot::q_cap, list_cap, k_cap, final_stride only grow (ensure_slot, bbq_core.cpp; bbq_host.h "grow-only maxima over the plans seen")
    "large_strides_then_small_call": (("search_batch", "wide"), ("search_batch", "long"), ("search_batch", "ties")),
    # ensure_slot derives the views into d_block again only when the block is reallocated (bbq_host.h, Slot::d_qbuf ...)
    "wide_ties_wide": (("search_batch", "wide"), ("search_batch", "ties"), ("search_batch", "wide")),
    # sub-batches of bbq_shard_scan_begin stay busy across API calls (Slot::InFlight::shard_owner, bbq_host.h); every entry point settles
    # them in its own way: settle_shard_slots in search_batch_impl (bbq_core.cpp), bbq_get_stats, bbq_index_save, bbq_index_destroy
    "begin_then_search_elsewhere": (("shard_begin", "shard"), ("search_batch", "wide"), ("shard_wait", "shard")),
    "begin_then_search_on_the_root_twin": (("shard_begin", "shard"), ("search_batch", "root"), ("shard_wait", "shard")),
    "begin_then_stats": (("shard_begin", "shard"), ("stats", "shard"), ("shard_wait", "shard")),
    "begin_then_save": (("shard_begin", "shard"), ("save", "shard"), ("shard_wait", "shard")),
    "begin_then_recreate_the_owner": (("shard_begin", "shard"), ("recreate", "shard"), ("shard_scan", "shard")),
    # two batches in alternating ShardSets (bbq_index::shard_set, shard_begun / shard_waited, bbq_host.h)
    "begin_begin_wait_wait": (("shard_begin", "shard"), ("shard_begin", "shard"), ("shard_wait", "shard"), ("shard_wait", "shard")),
    "begin_on_both_shards": (("shard_begin", "shard"), ("shard_begin", "root"), ("shard_wait", "root"), ("shard_wait", "shard")),
    # the grow-only staging inside bbq_vectors (bbq_rerank.cpp)
    "long_rerank_then_one_row": (("rerank", "wide"), ("rerank", "wide")),
    # sweep_share 32 on `wide`: the shared sweep on the matrix cores ("bool use_mfma = ...", enqueue_subbatch, bbq_core.cpp) with 70 queries -
    # two groups of 32 and a ragged third, 64 queries per launch chain (effective_batch) -, its filtered kernels (search_batch_impl keeps
    # c.share for a filter only at 32), the raw feed beyond 64 queries, and a k beyond kFinalSelectMax, where the host replays every list
    # the matrix-core sweep appended.  The option stays in force behind the block: `wide` sweeps shared until a chain's block resets it
    "matrix_core_sweeps": (("set_option", "wide"), ("search_batch", "wide"), ("search_filtered_batch", "wide"), ("search_raw_batch", "wide"),
                           ("search_batch", "wide"), ("search_filtered_batch", "wide")),
}
_FIXED = {   # the shapes a transition needs fixed
    "general_then_latency": ({"nq": 5, "k": 10}, {"k": 10}),
    "latency_then_general_then_latency": ({"k": 100}, {"nq": 33, "k": 100}, {"same": 0}),
    "presampled_unproven_then_chain_then_another_index": ({"q0": 0, "k": 10}, {"k": 10}, {"q0": TIED_QUERIES, "k": 10}),
    "large_strides_then_small_call": ({"nq": 130, "k": K_MAX_FAST_K}, {"nq": 1, "k": 1}, {"nq": 1, "k": 1}),
    "wide_ties_wide": ({"nq": 33, "k": 100}, {"nq": 70, "k": K_FINAL_SELECT_MAX}, {"same": 0}),
    "long_rerank_then_one_row": ({"shape": "long_lists"}, {"shape": "one_row"}),
    "matrix_core_sweeps": ({"option": "sweep_share", "value": 32}, {"nq": 70, "k": 10}, {"nq": 70, "k": 100, "filter": "dense"}, {"nq": 70, "k": 10},
                           {"nq": 130, "k": K_FINAL_SELECT_MAX + 1}, {"nq": 33, "k": 10, "filter": "sparse"}),
}


def _shaped(d, kind, member, via, fixed):
    """a step of a block: `fixed` overrides what the draw chose; a rerank's shape is re-drawn to the one asked for"""
    fixed = dict(fixed)
    if kind == "rerank" and "shape" in fixed:
        for _ in range(64):
            s = d.step(kind, member, via)
            if s["shape"] == fixed["shape"]:
                return s
    s = d.step(kind, member, via)
    s.update({k: v for k, v in fixed.items() if k != "same"})
    return s


LATENCY_OPTIONS = ("force_dense", "device_select", "latency_queries", "latency_fused", "latency_presample", "append_last", "sweep_share",
                   "first_segment_rows", "latency_growth")


def _restore(d, member, via, k):
    """set_option steps that take a member's single-query calls back onto their chain - the pre-sampled one on `long`, the segmented one
    elsewhere: a transition that is about a chain must reach it whatever an earlier block of the walk has set.  Only the options that
    keep the call off the chain are reset - each is tried alone against the defaults of the others - and the rest stay in force"""
    out, m, n = [], CAST[member], d.st.n[member]
    want = "presampled" if presample_plan(n, k) is not None and latency_supported(m) else "chain"
    for name in LATENCY_OPTIONS:
        default = dict(OPTIONS)[name][0]
        value = d.st.options[member].get(name, default)
        if value != default and single_query_path(m, n, k, {name: value}) != want:
            out.append(d.done(d.step("set_option", member, via, option=name, value=default)))
    assert single_query_path(m, n, k, d.st.options[member]) == want
    return out


def _transition(d, name):
    """the steps of a transition; in front of them (via "<name>:pre") what it takes to start from the state it is about: a member whose
    chains it names back on the default latency options, a shard it begins a batch on idle"""
    out = []
    fixed = _FIXED.get(name, ({},) * len(TRANSITIONS[name]))
    for member in sorted({m for k, m in TRANSITIONS[name] if k == "search"}):
        ks = [fx["k"] for (kind, mem), fx in zip(TRANSITIONS[name], fixed) if kind == "search" and mem == member and "k" in fx]
        out += _restore(d, member, name + ":pre", max(ks))
    for member in sorted({m for k, m in TRANSITIONS[name] if k == "shard_begin"}):
        while d.st.inflight[member]:
            out.append(d.done(d.step("shard_wait", member, name + ":pre")))
    if name == "matrix_core_sweeps" and d.st.options["wide"].get("force_dense", 0):
        out.append(d.done(d.step("set_option", "wide", name + ":pre", option="force_dense", value=0)))
    body = []
    for (kind, member), fx in zip(TRANSITIONS[name], fixed):
        if "same" in fx:
            s = dict(body[fx["same"]])
        else:
            s = _shaped(d, kind, member, name, fx)
        body.append(d.done(s))
    return out + body


def _euler_circuit(rng, nodes):
    """every ordered pair of `nodes`, a node with itself included, as consecutive entries of one closed walk (Hierholzer)"""
    left = {a: [nodes[int(i)] for i in rng.permutation(len(nodes))] for a in nodes}
    stack, out = [nodes[int(rng.integers(len(nodes)))]], []
    while stack:
        a = stack[-1]
        if left[a]:
            stack.append(left[a].pop())
        else:
            out.append(stack.pop())
    return out[::-1]


def _d_span_pairs(d):
    """each ordered pair of the six users of DeviceCtx::d_span (bbq_host.h): span, filtered span, grouped, MaxSim, MaxSim over groups and
    the exact MaxSim rerank share one grow-only scratch and one way back for scores and ords (finish_selected, bbq_select.cpp)"""
    out = []
    for kind in _euler_circuit(d.rng, list(D_SPAN_USERS)):
        member = d.pick([m for m in ("wide", "ties", "multi") if kind in ADMITS[m]])
        out.append(d.done(d.step(kind, member, "d_span_pairs")))
    return out


def _refused_between(d, what, member):
    """a refused call between two identical calls: a refusal launches nothing and leaves nothing behind (clear_error / fail, bbq_index.cpp)"""
    out = []
    if what == "third_begin":
        while len(d.st.inflight["shard"]) < 2:
            out.append(d.done(d.step("shard_begin", "shard", "refused_between")))
    elif what == "append_with_unwaited_batch" and not d.st.inflight["root"]:
        out.append(d.done(d.step("shard_begin", "root", "refused_between")))
    elif what == "wait_with_nothing_in_flight":
        while d.st.inflight["shard"]:
            out.append(d.done(d.step("shard_wait", "shard", "refused_between")))
    target = member if "search_batch" in ADMITS[member] else "ties"
    call = d.step("search_batch", target, "refused_between", nq=5, k=10)
    out.append(d.done(call))
    out.append(d.done(d.step("refused", member, "refused_between", what=what)))
    out.append(d.done(dict(call)))
    while d.st.inflight["root"]:
        out.append(d.done(d.step("shard_wait", "root", "refused_between")))
    return out


def _option_block(d, name):
    """[the call, set_option, the same call] for EVERY value of the option other than the one in force, in the listed order turned by
    the seed: an option is promised "never a different answer" (include/bbq.h, bbq_set_option).  The last value stays in force"""
    member, kind, fx = OPTION_CALLS[name]
    values = dict(OPTIONS)[name]
    via = "option:" + name
    call = _shaped(d, kind, member, via, fx)
    now = d.st.options[member].get(name, values[0])
    todo = [v for v in values if v is not None and v != now]
    turn = (d.seed // DEFAULT_SEEDS) % len(todo)
    out = [d.done(call)]
    for value in todo[turn:] + todo[:turn]:
        out += [d.done(d.step("set_option", member, via, option=name, value=value)), d.done(dict(call))]
    if name == "force_dense":     # ... and back, so that the member's later steps sweep again
        out.append(d.done(d.step("set_option", member, via, option=name, value=0)))
    return out


def _inflight_block(d, kinds):
    """a batch begun on the shard, calls of `kinds`, the batch collected (a recreate of the owner collects nothing: the batch is gone)"""
    out = []
    while len(d.st.inflight["shard"]) == 2:
        out.append(d.done(d.step("shard_wait", "shard", "inflight_tour")))
    out.append(d.done(d.step("shard_begin", "shard", "inflight_tour")))
    for kind in kinds:
        members = [m for m in CAST if d.admissible(kind, m)]
        if kind == "shard_wait":      # the other shard's batch is collected while this one's stays in flight
            if not d.st.inflight["root"]:
                out.append(d.done(d.step("shard_begin", "root", "inflight_tour")))
            members = ["root"]
        if kind == "shard_scan":      # on the other shard, idle: the synchronous form while this one's batch is in flight
            while d.st.inflight["root"]:
                out.append(d.done(d.step("shard_wait", "root", "inflight_tour")))
            members = ["root"]
        if not members:
            continue
        out.append(d.done(d.step(kind, d.pick(members), "inflight_tour")))
    while d.st.inflight["shard"]:
        out.append(d.done(d.step("shard_wait", "shard", "inflight_tour")))
    return out


def walk(seed):
    """the steps of one walk (about 250): the blocks described in the module's docstring in a shuffled order, FREE_STEPS freely drawn
    steps between them, and at the end whatever is still in flight collected"""
    rng = np.random.default_rng([seed, 20240])
    d = _Draw(rng, seed)
    turn = seed % DEFAULT_SEEDS
    blocks = [("transition", name) for name in TRANSITIONS] + [("d_span_pairs", None)]
    blocks += [("option", name) for i, (name, _) in enumerate(OPTIONS) if i % DEFAULT_SEEDS == turn]
    blocks += [("refused", r) for i, r in enumerate(REFUSALS) if i % DEFAULT_SEEDS == turn]
    pairs = [(member, kind) for member in CAST for kind in ADMITS[member]]
    blocks += [("call", p) for i, p in enumerate(pairs) if i % DEFAULT_SEEDS == turn]
    tour = [k for i, k in enumerate(KINDS) if i % DEFAULT_SEEDS == turn and k != "shard_begin"]
    blocks += [("inflight", tuple(tour[i:i + 3])) for i in range(0, len(tour), 3)]
    blocks += [("free", None)] * FREE_STEPS
    out = []
    for i in rng.permutation(len(blocks)):
        what, arg = blocks[int(i)]
        if what == "transition":
            out += _transition(d, arg)
        elif what == "d_span_pairs":
            out += _d_span_pairs(d)
        elif what == "option":
            out += _option_block(d, arg)
        elif what == "refused":
            out += _refused_between(d, arg[0], arg[1])
        elif what == "inflight":
            out += _inflight_block(d, arg)
        else:
            if what == "call":
                member, kind = arg
            else:
                member = d.pick(list(CAST))
                kind = d.pick(list(ADMITS[member]))
            pre = []
            if kind == "shard_wait" and not d.st.inflight[member]:
                pre = [d.done(d.step("shard_begin", member, what))]
            if kind == "shard_begin" and len(d.st.inflight[member]) == 2:
                pre = [d.done(d.step("shard_wait", member, what))]
            while kind == "shard_scan" and d.st.inflight[member]:
                pre.append(d.done(d.step("shard_wait", member, what)))
            if kind == "refused" and member == "root" and not d.admissible(kind, member):     # its refusal needs a batch of its own in flight
                pre = [d.done(d.step("shard_begin", member, what))]
            if not d.admissible(kind, member):
                continue
            over = {}
            if what == "call" and kind == "search_batch":     # the member tour's batch searches take the k values beside the two limits
                n = d.st.n[member]
                over["k"] = {"wide": K_FINAL_SELECT_MAX + 1, "ties": K_MAX_FAST_K + 1, "multi": n + 3, "long": K_FINAL_SELECT_MAX + 1, "root": n}[member]
            out += pre + [d.done(d.step(kind, member, what, **over))]
    for member in CAST:
        while d.st.inflight[member]:
            out.append(d.done(d.step("shard_wait", member, "closing")))
    return out


def read_only_walk(seed, member="ties", steps=30):
    """the steps of one thread of the shared-handles test: read-only kinds on `member` alone, refusals among them"""
    rng = np.random.default_rng([seed, 20241])
    d = _Draw(rng, seed)
    kinds = [k for k in READ_ONLY if k in ADMITS[member] and k != "stats"]
    out = []
    for i in range(steps):
        kind = kinds[int(rng.integers(len(kinds)))] if i >= len(kinds) else kinds[i]
        if kind == "refused":
            out.append(d.step(kind, member, "threads", what=d.pick(["filter_of_another_size", "group_outside_the_set"])))
        else:
            out.append(d.step(kind, member, "threads"))
    return out


def replay(steps):
    """the State behind every step of a walk, for the checks: yields (step, options in force on its member, batches in flight in all)"""
    d = _Draw(np.random.default_rng(0), 0)
    for s in steps:
        before = (dict(d.st.options[s["member"]]), d.st.in_flight(), d.st.n[s["member"]])
        d.done(s)
        yield s, before


def describe(step):
    """one line that lets a failure be replayed as a fixed sequence"""
    def short(a):
        a = np.asarray(a).ravel().tolist()
        return str(a) if len(a) <= 10 else "[%s, ... %d entries ..., %s]" % (", ".join(map(str, a[:5])), len(a), ", ".join(map(str, a[-2:])))

    parts = [step["kind"], "on", step["member"]]
    for key in ("what", "option", "value", "shape", "q0", "nq", "k", "filter", "groups", "tokens", "ranks", "true_sim", "factor", "selector"):
        if key in step:
            parts.append("%s=%s" % (key, step[key]))
    for key in ("spans", "cand", "lists", "rows"):
        if key in step:
            v = step[key]
            parts.append("%s=%s" % (key, short(v) if isinstance(v, np.ndarray) else "[" + "; ".join(short(x) for x in v) + "]"))
    if "ords" in step:
        parts.append("ords=" + short(step["ords"]))
    parts.append("(%s)" % step["via"])
    return " ".join(parts)
