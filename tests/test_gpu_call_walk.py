"""GPU: one device context held to the oracle over seeded random walks of mixed calls (tests/call_walk.py).  The members of the cast -
five indexes of different geometry, a shard with a pilot replica among them, a bbq_vectors, filters and group sets - live on device 0
for a whole walk; a step is one call of one kind on one member, and after EVERY step the answer is compared with the oracle's: indices,
score bits, order, counts and statuses, bit for bit (canon32, canon64), no tolerances.  Expected values come from the oracle alone -
O.score_all and O.true_similarity, the numpy models of the MaxSim calls, O.heap_topk and O.rerank_select - computed once per member and
query pool and shared by the walks; the comparisons are the existing helpers' (Oracle.check_search, assert_spans, assert_filtered,
assert_grouped, assert_maxsim, assert_lists, assert_range).  A failure names seed, step, the step's line (call_walk.describe), the
options in force and what is in flight: the listing up to there replays it as a fixed sequence.  A BBQ_ERR_HIP from any call ends the
whole pytest session and closes no handle (test_gpu_mutation_walk.located).

Statistics are checked where include/bbq.h defines them as "of the last call": after bbq_search_batch, bbq_search_filtered_batch and
bbq_search_raw_batch dense_fallbacks is the number of queries on the dense path - every query under force_dense or k > 4096
(dense_search_one books one each, bbq_dense.cpp), none otherwise: no pool has a NaN score - and host_replays is the number of queries
under device_select 0 or k > 1024, and 0 where the oracle says every answer's k + 1 best scores are pairwise different.  `candidates` is
not asserted: it sums the lengths of the device's candidate lists, which follow from thresholds that the finalize launches of one
sub-batch derive in stream order - deterministic for one call as far as the code shows - but under sweep_share the lists also hold what
a shared sweep's survivor queues let through, and a query that overflowed there is swept again alone: nothing in include/bbq.h pins
the figure, so a walk would only pin today's plan.

Two more tests take the promises of include/bbq.h that need threads: filters, group sets and an index shared by four threads of
read-only walks with a thread-local bbq_last_error, and searches beside appends.  The ctypes calls release the interpreter lock -
capi.lib() loads libbbq with ctypes.CDLL, not PyDLL - so the threads do meet inside the library.  Each runs its work on one thread first
and joins the threads with a limit of max(60 s, 20 x that time); a thread still alive then ends the session without another call."""
import functools
import os
import threading
import time
import zlib

import numpy as np
import pytest

import call_walk as W
import orclib as O
import maxsim_model as MM
import maxsim_rerank_model as MR
import test_groups_cpu as GC
import test_gpu_spans as GS
import test_gpu_spans_filtered as GF
import test_gpu_grouped as GG
import test_gpu_maxsim as GM
import test_gpu_maxsim_groups as GMG
import test_gpu_range as GR
from bbqlib import bbq_amd as B, capi
from test_gpu_append import Oracle, canon32, canon64, check_export, make_index
from test_gpu_mutation_walk import located, refused
from test_gpu_update import needs_sums

pytestmark = pytest.mark.gpu

SEEDS = tuple(range(int(os.environ.get("BBQ_CALL_WALK_SEEDS", str(W.DEFAULT_SEEDS)))))
LAM, ITERS = 0.1, 5


# ---------------------------------------------------------------------------------------------------- the sources of rows
class Source:
    """the rows a member (or several) is cut from, a pool of queries, and the oracle's scores of every row for every pool query:
    computed once per session, shared, never written to"""

    def __init__(self, name, dim, ib, sim, qb, pool):
        self.name, self.dim, self.ib, self.sim, self.qb = name, dim, ib, sim, qb
        seed = zlib.crc32(name.encode()) & 0xffff
        if name == "seeded":
            n = W.CAST["wide"].n0
            base = O.mulberry32(seed, n * dim).reshape(n, dim).copy()
            base[n - 10:] = base[100:110]          # ten rows twice: equal scores wherever both copies reach an answer
            self.base = base
            self.codes, self.corr, self.cen = O.build_index(base, sim, LAM, ITERS, ib=ib)
            raw = O.mulberry32(seed + 1, pool * dim).reshape(pool, dim)
        elif name == "synthetic":
            n = W.CAST["long"].n0
            rng = np.random.default_rng(seed)
            self.base = None
            self.codes = rng.integers(0, 256, (n, dim // 8), dtype=np.uint8)
            a = rng.uniform(0.05, 0.15, n)
            pop = np.unpackbits(self.codes, axis=1).sum(axis=1).astype(np.float64)
            self.corr = np.ascontiguousarray(np.stack([-a, a * rng.uniform(0.8, 1.2, n), rng.uniform(0.5, 1.5, n), pop], axis=1))
            self.cen = (rng.standard_normal(dim) * 0.05).astype(np.float32)
            raw = rng.standard_normal((pool, dim)).astype(np.float32)
        else:
            g = O.load_golden(name)
            assert (O.SIMS[g["sim"]], g["dim"], g["ib"], g["qb"], g["lambda"], g["iters"]) == (sim, dim, ib, qb, LAM, ITERS)
            self.base, gq = O.golden_inputs(g)
            self.codes, self.corr, self.cen = O.build_index(self.base, sim, LAM, ITERS, ib=ib)
            raw = np.concatenate([gq, O.mulberry32(seed + 1, (pool - len(gq)) * dim).reshape(-1, dim)]).astype(np.float32)
        self.n, self.cdp, self.raw = self.codes.shape[0], O.centroid_dp(self.cen), np.ascontiguousarray(raw, np.float32)
        qs = [B.quantize_query(q, self.cen, sim, qb, LAM, ITERS) for q in self.raw]
        self.qq, self.qc = np.stack([a for a, _ in qs]), np.stack([b for _, b in qs])
        score = lambda p: O.score_all(self.codes, self.corr, dim, self.qq[p], self.qc[p], qb, sim, self.cdp, ib=ib)
        self.scores = [score(p) for p in range(pool)]
        if name == "synthetic":                  # queries 0..2: the best row three more times, once inside the pre-sampled prefix
            for p in range(W.TIED_QUERIES):
                best = int(np.argmax(self.scores[p][2]))
                for dst in (7 + p, n // 2 + p, n - 1 - p):
                    self.codes[dst], self.corr[dst] = self.codes[best], self.corr[best]
                    for s in self.scores:
                        for arr in s:
                            arr[dst] = arr[best]
        assert not needs_sums(self.codes[:4096], self.corr[:4096], ib)
        assert np.isfinite(self.qc).all()        # finite score uniforms: what mfma_query_ok (bbq_query.cpp) asks of a query
        for s in self.scores:
            assert not np.isnan(s[2]).any()      # what the dense_fallbacks rule of this file rests on
            for arr in s:
                arr.setflags(write=False)
        for arr in (self.codes, self.corr, self.qq, self.qc, self.raw):
            arr.setflags(write=False)
        self._true = {}

    def true(self, p, rows, true_sim):
        """computeSimilarity of raw pool query p and the fp32 rows `rows`, f64, from the oracle; every pair computed once"""
        out = np.zeros(len(rows), np.float64)
        for i, r in enumerate(np.asarray(rows, np.int64)):
            key = (int(p), int(r), int(true_sim))
            if key not in self._true:
                self._true[key] = O.true_similarity(self.raw[p:p + 1], self.base[r:r + 1], true_sim)[0, 0]
            out[i] = self._true[key]
        return out


@functools.lru_cache(maxsize=None)
def source(name):
    m = next(m for m in W.CAST.values() if m.source == name)
    return Source(name, m.dim, m.ib, m.sim, m.qb, m.pool)


class View(Oracle):
    """Oracle over the rows a member holds now, for a list of pool queries; the heaps are the member's, shared between the steps"""

    def __init__(self, live, pqs):
        src = live.src_of
        self.sim, self.qb, self.n = src.sim, src.qb, live.n
        self.qq, self.qc = np.ascontiguousarray(src.qq[pqs]), np.ascontiguousarray(src.qc[pqs])
        self.pqs, self.live = pqs, live
        self.scores = [live.scores(p) for p in pqs]

    def topk(self, qi, k):
        return self.live.topk(int(self.pqs[qi]), k)


# ---------------------------------------------------------------------------------------------------- a live member
class Live:
    """one member of the cast on the device: its index, what hangs on it, the rows it holds (`rows` into its source), its options"""

    def __init__(self, name, tmp):
        self.name, self.m, self.tmp = name, W.CAST[name], tmp
        self.src_of = source(self.m.source)
        lo, hi = self.m.rows or (0, self.m.n0)
        self.rows = np.arange(lo, hi, dtype=np.int64)
        self.whole = self.m.rows is None and name not in W.APPEND_POOL     # the member IS its source: no gather per query
        self.options, self.inflight = {}, []
        self.ix = self.dv = None
        self.filters, self.groups, self.masks = {}, {}, {}
        self._scores, self._heaps = {}, {}
        self.create()

    @property
    def n(self):
        return len(self.rows)

    def create(self):
        m, s = self.m, self.src_of
        codes, corr = s.codes[self.rows], s.corr[self.rows]
        if m.pilot:
            self.ix = B.Index(codes, corr, m.dim, s.cdp, index_bits=m.ib, row_base=int(self.rows[0]), pilot_codes=s.codes[:m.pilot], pilot_corr=s.corr[:m.pilot],
                              corrections="compact" if m.compact else "inline")
        else:
            self.ix = make_index(codes, corr, m.dim, s.cdp, m.compact, m.ib)
        if self.name == W.WITH_VECTORS and self.dv is None:
            self.dv = B.Vectors(s.base[self.rows])
        self.options, self.inflight = {}, []
        self.hang()

    def unhang(self):
        for h in list(self.groups.values()) + list(self.filters.values()):
            h.close()
        self.filters, self.groups, self.masks = {}, {}, {}

    def hang(self):
        """the filters and group sets of the index as it is now (a filter is made for one size)"""
        self.unhang()
        if "search_filtered_batch" not in W.ADMITS[self.name]:
            return
        n = self.n
        for which in ("sparse", "dense"):
            self.masks[which] = W.mask_of(self.name, n, which)
            self.filters[which] = capi.Filter(self.ix, self.masks[which])
            assert self.filters[which].count == int(self.masks[which].sum())
        if "search_grouped" in W.ADMITS[self.name]:
            self.off = W.offsets_of(n)
            self.masks["ragged"], self.masks["filtered"] = W.group_mask(self.name, n, "ragged"), self.masks["dense"]
            self.groups["ragged"] = capi.Groups(self.ix, self.off)
            self.groups["filtered"] = capi.Groups(self.ix, self.off, self.filters["dense"])

    def close(self):
        self.unhang()
        for h in (self.ix, self.dv):
            if h is not None:
                h.close()

    def scores(self, p):
        """(qcdist, f64 score, f32 score) of every row the member holds, for pool query p"""
        if self.whole:
            return self.src_of.scores[p]
        if p not in self._scores:
            self._scores[p] = tuple(a[self.rows] for a in self.src_of.scores[p])
        return self._scores[p]

    def s32(self, p):
        return self.scores(p)[2]

    def topk(self, p, k):
        if (p, k) not in self._heaps:
            self._heaps[(p, k)] = O.heap_topk(self.s32(p), k)
        return self._heaps[(p, k)]

    def grew(self, rows):
        self.rows = np.concatenate([self.rows, rows])
        self._scores, self._heaps = {}, {}
        self.hang()

    def opt(self, name):
        default = dict(W.OPTIONS)[name][0]
        return self.options.get(name, default)


def provable(s32, k):
    """the device's own selection stands: more rows than k, k within kFinalSelectMax, the k + 1 best scores pairwise different"""
    s = np.asarray(s32, np.float32)
    if not (1 <= k <= W.K_FINAL_SELECT_MAX and len(s) > k):
        return False
    top = np.sort(s)[::-1][:k + 1]
    return not (top[:-1] == top[1:]).any()


# ---------------------------------------------------------------------------------------------------- a walk on the device
class Play:
    def __init__(self, seed, tmp, steps=None, members=None):
        self.seed, self.tmp = seed, tmp
        self.steps = W.walk(seed) if steps is None else steps
        self.live = {name: Live(name, tmp) for name in (members or W.CAST)}
        self.transitions = set()
        self.stats_are_mine = True     # no other thread calls the indexes of this walk
        self.stat_checks = {"dense": 0, "all replayed": 0, "all proven": 0, "ties: replays not pinned": 0}

    def close(self):
        for lv in self.live.values():
            lv.close()

    def msg(self, i):
        s = self.steps[i]
        lv = self.live[s["member"]]
        flight = {name: len(l.inflight) for name, l in self.live.items() if l.inflight}
        return "seed %d step %d of %d: %s\noptions in force on %s: %s; in flight: %s" % (self.seed, i, len(self.steps) - 1, W.describe(s), s["member"],
                                                                                        lv.options or "defaults", flight or "nothing")

    # ------------------------------------------------------------------------------------------------ searches
    def check_stats(self, lv, nq, k, scores_of_queries):
        """candidates is left alone (the module's docstring says why)"""
        if not self.stats_are_mine:
            return
        st = lv.ix.stats()
        n_eff = len(scores_of_queries[0])
        keff = min(k, n_eff)
        if keff > W.K_MAX_FAST_K or lv.opt("force_dense"):
            assert (st["dense_fallbacks"], st["host_replays"]) == (nq, 0), "dense path: %s" % st
            self.stat_checks["dense"] += 1
            return
        assert st["dense_fallbacks"] == 0, "no query of this call has a score the device cannot bound: %s" % st
        if keff > W.K_FINAL_SELECT_MAX or not lv.opt("device_select"):
            assert st["host_replays"] == nq, "the host replays every query: %s" % st
            self.stat_checks["all replayed"] += 1
        elif all(provable(s, keff) for s in scores_of_queries):
            assert st["host_replays"] == 0, "every answer's k + 1 best scores are pairwise different: %s" % st
            self.stat_checks["all proven"] += 1
        else:
            assert 0 <= st["host_replays"] <= nq, st
            self.stat_checks["ties: replays not pinned"] += 1

    def search_batch(self, lv, s, msg):
        pqs = W.queries_of(s, lv.m.pool)
        View(lv, pqs).check_search(lv.ix, [s["k"]], msg)
        self.check_stats(lv, len(pqs), s["k"], [lv.s32(p) for p in pqs])

    def search(self, lv, s, msg):
        """the single-query entry point itself, bbq_search, and then bbq_search_batch with the same one query"""
        src, k, p = lv.src_of, s["k"], int(W.queries_of(s, lv.m.pool)[0])
        qq, qc = np.ascontiguousarray(src.qq[p]), np.ascontiguousarray(src.qc[p])
        idx, sc, cnt = np.zeros(k, np.int32), np.zeros(k, np.float32), np.zeros(1, np.int64)
        capi._chk(capi.lib().bbq_search(lv.ix._h, capi._ptr(qq), capi._ptr(qc), src.qb, src.sim, k, capi._ptr(idx), capi._ptr(sc), capi._ptr(cnt)))
        wi, ws = lv.topk(p, k)
        assert cnt[0] == len(wi), msg
        np.testing.assert_array_equal(idx[:cnt[0]], wi, err_msg=msg + ": bbq_search")
        np.testing.assert_array_equal(canon32(sc[:cnt[0]]), canon32(ws), err_msg=msg + ": bbq_search")
        self.check_stats(lv, 1, k, [lv.s32(p)])
        self.search_batch(lv, s, msg)

    def search_filtered_batch(self, lv, s, msg):
        pqs, k, src = W.queries_of(s, lv.m.pool), s["k"], lv.src_of
        acc = np.flatnonzero(lv.masks[s["filter"]])
        idx, sc, cnt = lv.ix.search_filtered_batch(src.qq[pqs], src.qc[pqs], src.qb, src.sim, k, lv.filters[s["filter"]])
        for qi, p in enumerate(pqs):
            pos, ws = O.heap_topk(lv.s32(p)[acc], k)
            assert cnt[qi] == len(pos), "%s q%d" % (msg, qi)
            np.testing.assert_array_equal(idx[qi, :cnt[qi]], acc[pos], err_msg="%s q%d" % (msg, qi))
            np.testing.assert_array_equal(canon32(sc[qi, :cnt[qi]]), canon32(ws), err_msg="%s q%d" % (msg, qi))
        self.check_stats(lv, len(pqs), k, [lv.s32(p)[acc] for p in pqs])

    def search_raw_batch(self, lv, s, msg):
        pqs, k, src = W.queries_of(s, lv.m.pool), s["k"], lv.src_of
        idx, sc, cnt, qq, qc = lv.ix.search_raw_batch(src.raw[pqs], src.cen, src.sim, src.qb, k, LAM, ITERS, want_quantized=True)
        np.testing.assert_array_equal(qq, src.qq[pqs], err_msg=msg + ": quantized queries")
        np.testing.assert_array_equal(canon64(qc), canon64(src.qc[pqs]), err_msg=msg + ": query corrections")
        for qi, p in enumerate(pqs):
            wi, ws = lv.topk(int(p), k)
            assert cnt[qi] == len(wi), "%s q%d" % (msg, qi)
            np.testing.assert_array_equal(idx[qi, :cnt[qi]], wi, err_msg="%s q%d" % (msg, qi))
            np.testing.assert_array_equal(canon32(sc[qi, :cnt[qi]]), canon32(ws), err_msg="%s q%d" % (msg, qi))
        self.check_stats(lv, len(pqs), k, [lv.s32(p) for p in pqs])

    def range(self, lv, s, msg):
        pqs, src = W.queries_of(s, lv.m.pool), lv.src_of
        mask = lv.masks[s["filter"]] if s["filter"] else None
        ths = []
        for p, rank in zip(pqs, s["ranks"]):
            v = np.sort(lv.s32(p) if mask is None else lv.s32(p)[mask])[::-1]
            ths.append(np.nextafter(v[0], np.float32(np.inf)) if rank < 0 else v[min(rank, len(v) - 1)])
        GR.assert_range(lv.ix, src.qq[pqs], src.qc[pqs], src.qb, src.sim, np.array(ths, np.float32), [lv.s32(p) for p in pqs], msg,
                        lv.filters[s["filter"]] if s["filter"] else None, mask)

    def search_spans(self, lv, s, msg):
        pqs, src = W.queries_of(s, lv.m.pool), lv.src_of
        GS.assert_spans(lv.ix, src.qq[pqs], src.qc[pqs], src.qb, src.sim, s["k"], s["spans"], [lv.s32(p) for p in pqs], msg)

    def search_spans_filtered(self, lv, s, msg):
        pqs, src = W.queries_of(s, lv.m.pool), lv.src_of
        GF.assert_filtered(lv.ix, lv.filters[s["filter"]], lv.masks[s["filter"]], src.qq[pqs], src.qc[pqs], src.qb, src.sim, s["k"], s["spans"],
                           [lv.s32(p) for p in pqs], msg)

    def search_grouped(self, lv, s, msg):
        pqs, src = W.queries_of(s, lv.m.pool), lv.src_of
        GG.assert_grouped(lv.ix, lv.groups[s["groups"]], lv.off, lv.masks[s["groups"]], src.qq[pqs], src.qc[pqs], src.qb, src.sim, s["k"],
                          [lv.s32(p) for p in pqs], msg)

    def _tokens(self, lv, s):
        """(pool vectors of all tokens, [(first, last)] per query, the model's representatives [vectors, L] and live groups)"""
        toks = W.tokens_of(s, lv.m.pool)
        flat = np.concatenate(toks)
        cuts = np.concatenate([[0], np.cumsum([len(t) for t in toks])])
        spans = [(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]
        rep, live = MM.rep_scores([lv.s32(int(p)) for p in flat], lv.off, lv.masks[s["groups"]])
        return flat, spans, rep, live

    def search_maxsim(self, lv, s, msg):
        src = lv.src_of
        flat, spans, rep, live = self._tokens(lv, s)
        GM.assert_maxsim(lv.ix, lv.groups[s["groups"]], rep, live, src.qq[flat], src.qc[flat], spans, src.qb, src.sim, s["k"], msg)
        lv.ix.set_option("maxsim_fused", lv.opt("maxsim_fused"))     # assert_maxsim runs both values and leaves -1: the walk's value again

    def maxsim_groups(self, lv, s, msg):
        src = lv.src_of
        flat, spans, rep, live = self._tokens(lv, s)
        GMG.assert_lists(lv.ix, lv.groups[s["groups"]], rep, live, src.qq[flat], src.qc[flat], spans, s["cand"], src.qb, src.sim, msg, ks=(s["k"], None))

    def rerank(self, lv, s, msg):
        pqs, src, k, factor = W.queries_of(s, lv.m.pool), lv.src_of, s["k"], s["factor"]
        got = lv.dv.rerank_scores(src.raw[pqs], s["rows"], s["true_sim"])
        for qi, p in enumerate(pqs):
            np.testing.assert_array_equal(canon64(got[qi]), canon64(src.true(p, lv.rows[s["rows"][qi]], s["true_sim"])), err_msg="%s rerank_scores q%d" % (msg, qi))
        idx, qs, ts, cnt = B.search_rerank_batch(lv.ix, lv.dv, src.raw[pqs], src.qq[pqs], src.qc[pqs], src.qb, src.sim, k, factor, s["selector"], 1)
        for qi, p in enumerate(pqs):
            cand, csc = lv.topk(int(p), k * factor)
            true = src.true(p, lv.rows[cand], 1)
            pos = O.rerank_select(true, k, "sort" if s["selector"] else "heap")
            np.testing.assert_array_equal(idx[qi, :cnt[qi]], cand[pos], err_msg="%s search_rerank q%d" % (msg, qi))
            np.testing.assert_array_equal(canon32(qs[qi, :cnt[qi]]), canon32(csc[pos]), err_msg="%s search_rerank q%d" % (msg, qi))
            np.testing.assert_array_equal(canon64(ts[qi, :cnt[qi]]), canon64(true[pos]), err_msg="%s search_rerank q%d" % (msg, qi))

    def _true_maxsim(self, lv, s, toks, cand):
        """the model's exact MaxSim score of every candidate group of a query (maxsim_rerank_model over the oracle's similarities)"""
        src, mask = lv.src_of, lv.masks[s["groups"]]
        uniq, inv = np.unique(np.asarray(cand, np.int64), return_inverse=True)
        rep = np.zeros((len(toks), len(uniq)), np.float64)
        for i, g in enumerate(uniq):
            rows = np.arange(lv.off[g], lv.off[g + 1])
            rows = rows[mask[rows]]
            for t, p in enumerate(toks):
                rep[t, i] = MR.group_max(src.true(int(p), lv.rows[rows], s["true_sim"]))
        return MR.reduce_true(rep)[inv] if len(uniq) else np.zeros(0, np.float64)

    def maxsim_rerank(self, lv, s, msg):
        src, groups = lv.src_of, lv.groups[s["groups"]]
        toks = W.tokens_of(s, lv.m.pool)
        raw = [src.raw[t] for t in toks]
        got, coff = lv.dv.rerank_maxsim_groups_batch(raw, groups, s["cand"], s["true_sim"])
        for q, (t, cand) in enumerate(zip(toks, s["cand"])):
            np.testing.assert_array_equal(MR.bits(got[coff[q]:coff[q + 1]]), MR.bits(self._true_maxsim(lv, s, t, cand)), err_msg="%s rerank_maxsim_groups q%d" % (msg, q))
        k, factor, how = s["k"], s["factor"], "sort" if s["selector"] else "heap"
        tok = [(src.qq[t], src.qc[t]) for t in toks]
        res = capi.search_maxsim_rerank_batch(lv.ix, lv.dv, groups, raw, tok, src.qb, src.sim, k, factor, s["selector"], s["true_sim"])
        for q, t in enumerate(toks):
            rep, live = MM.rep_scores([lv.s32(int(p)) for p in t], lv.off, lv.masks[s["groups"]])
            S = MM.reduce(rep)
            oi, osc = O.heap_topk(S, k * factor)
            first = live[oi]
            true = self._true_maxsim(lv, s, t, first)
            pos = O.rerank_select(true, k, how)
            w = "%s search_maxsim_rerank q%d" % (msg, q)
            np.testing.assert_array_equal(res[q][0], first[pos], err_msg=w + ": groups")
            np.testing.assert_array_equal(canon32(res[q][1]), canon32(osc[pos]), err_msg=w + ": quantized scores")
            np.testing.assert_array_equal(MR.bits(res[q][2]), MR.bits(true[pos]), err_msg=w + ": true scores")

    def score_rows(self, lv, s, msg):
        View(lv, W.queries_of(s, lv.m.pool)).check_score_rows(lv.ix, msg)

    def score_ords(self, lv, s, msg):
        p, src, ords = int(W.queries_of(s, lv.m.pool)[0]), lv.src_of, s["ords"]
        d, s64, s32 = lv.ix.score_ords(src.qq[p], src.qc[p], src.qb, src.sim, ords)
        od, o64, o32 = lv.scores(p)
        np.testing.assert_array_equal(d, od[ords], err_msg=msg)
        np.testing.assert_array_equal(canon64(s64), canon64(o64[ords]), err_msg=msg)
        np.testing.assert_array_equal(canon32(s32), canon32(o32[ords]), err_msg=msg)

    def search_ords(self, lv, s, msg):
        pqs, src, k = W.queries_of(s, lv.m.pool), lv.src_of, s["k"]
        res = lv.ix.search_ords_batch(src.qq[pqs], src.qc[pqs], src.qb, src.sim, k, s["lists"])
        for qi, (p, lst) in enumerate(zip(pqs, s["lists"])):
            pos, ws = O.heap_topk(lv.s32(p)[lst], k)
            np.testing.assert_array_equal(res[qi][0], lst[pos], err_msg="%s q%d" % (msg, qi))
            np.testing.assert_array_equal(canon32(res[qi][1]), canon32(ws), err_msg="%s q%d" % (msg, qi))

    # ------------------------------------------------------------------------------------------------ sharded scans
    def begin(self, lv, s, wait):
        import torch
        pqs, src, k = W.queries_of(s, lv.m.pool), lv.src_of, s["k"]
        nq, stride = len(pqs), k + 3
        cap = max(int(lv.ix.shard_list_cap(k)), 1) * nq
        b = {"pqs": pqs, "k": k, "cap": cap, "stride": stride,
             "packed": torch.zeros(cap, dtype=torch.int64, device="cuda"), "off": torch.zeros(nq + 1, dtype=torch.int64, device="cuda"),
             "flags": torch.zeros(nq, dtype=torch.int32, device="cuda"), "ans": None}
        args = (src.qq[pqs], src.qc[pqs], src.qb, src.sim, k, b["packed"].data_ptr(), cap, b["off"].data_ptr(), b["flags"].data_ptr())
        if wait:
            b["total"] = lv.ix.shard_scan(*args)
        else:
            b["ans"] = torch.full((nq * stride,), -1, dtype=torch.int64, device="cuda")     # garbage the scan has to overwrite
            lv.ix.shard_scan_begin(*args, b["ans"].data_ptr(), stride)
        return b

    def collected(self, lv, b, msg):
        """a batch's packed lists replay, with the rows in front of the shard, to the oracle's heaps over all rows; its answer blocks
        merge with the oracle's blocks of the rows in front to the same"""
        src, k, pqs = lv.src_of, b["k"], b["pqs"]
        nq, lo, hi = len(pqs), int(lv.rows[0]), int(lv.rows[-1]) + 1
        flags, off = b["flags"].cpu().numpy(), b["off"].cpu().numpy()
        assert not flags.any(), msg + ": no query of this pool has a NaN score"
        assert off[nq] == b["total"], msg
        packed = b["packed"][:b["total"]].cpu().numpy().view(np.uint64)
        rows = (packed >> np.uint64(32)).astype(np.int64)
        assert ((rows >= lo) & (rows < hi)).all(), msg + ": a packed entry outside the shard's rows"
        front_p, front_o, front_b = [], [0], []
        for p in pqs:                  # the rows in front of the shard, from the oracle: every row listed (a superset is a valid list)
            s32 = src.scores[p][2][:lo]
            front_p.append((np.arange(lo, dtype=np.uint64) << np.uint64(32)) | s32.view(np.uint32).astype(np.uint64))
            front_o.append(front_o[-1] + lo)
            key = GC.rank_keys(s32)
            cut = int(np.sort(key)[::-1][k]) if lo > k else 0
            above = np.flatnonzero(key > cut)
            above = above[np.argsort(-key[above], kind="stable")]
            blk = np.zeros(b["stride"], np.uint64)
            blk[0], blk[1], blk[2] = lo, len(above), cut
            blk[3:3 + len(above)] = (above.astype(np.uint64) << np.uint64(32)) | s32[above].view(np.uint32).astype(np.uint64)
            front_b.append(blk)
        sources_p = ([np.concatenate(front_p)] if lo else []) + [packed]
        sources_o = ([np.array(front_o, np.int64)] if lo else []) + [off]
        idx, sc, cnt = B.replay_batch(sources_p, sources_o, nq, hi, k)
        want = [O.heap_topk(src.scores[p][2][:hi], k) for p in pqs]
        for qi, (wi, ws) in enumerate(want):
            np.testing.assert_array_equal(idx[qi, :cnt[qi]], wi, err_msg="%s: replayed lists q%d" % (msg, qi))
            np.testing.assert_array_equal(canon32(sc[qi, :cnt[qi]]), canon32(ws), err_msg="%s: replayed lists q%d" % (msg, qi))
        if b["ans"] is None:
            return
        blk = b["ans"].cpu().numpy().view(np.uint64).reshape(nq, b["stride"])
        np.testing.assert_array_equal(blk[:, 0] & np.uint64(0xffffffff), np.diff(off).astype(np.uint64), err_msg=msg + ": entries listed")
        assert not (blk[:, 0] >> np.uint64(32)).any(), msg + ": flags in an answer block"
        idx, sc, cnt, status = B.merge_answers(([np.stack(front_b)] if lo else []) + [blk], nq, hi, k)
        assert (status != 2).all(), msg
        for qi in np.flatnonzero(status == 0):
            wi, ws = want[qi]
            np.testing.assert_array_equal(idx[qi, :cnt[qi]], wi, err_msg="%s: merged answers q%d" % (msg, qi))
            np.testing.assert_array_equal(canon32(sc[qi, :cnt[qi]]), canon32(ws), err_msg="%s: merged answers q%d" % (msg, qi))

    # ------------------------------------------------------------------------------------------------ refusals
    def refuse(self, lv, s, msg):
        src, what, code = lv.src_of, s["what"], getattr(capi, s["code"])
        p = int(s["q0"]) % lv.m.pool
        one = (src.qq[p:p + 1], src.qc[p:p + 1], src.qb, src.sim)
        if what == "filter_of_another_size":
            other = self.live["multi"].filters["dense"] if "multi" in self.live else self.foreign_filter
            call = lambda: lv.ix.search_filtered_batch(*one, 3, other)
        elif what == "negative_k":
            call = lambda: lv.ix.search_batch(*one, -1)
        elif what == "search_on_a_shard":
            call = lambda: lv.ix.search_batch(*one, 3)
        elif what == "group_outside_the_set":
            tok = [(src.qq[p:p + 1], src.qc[p:p + 1])]
            call = lambda: lv.ix.search_maxsim_groups_batch(tok, src.qb, src.sim, 3, lv.groups["ragged"], [np.array([0, len(lv.off) - 1], np.int64)])
        elif what == "rerank_row_out_of_range":
            call = lambda: lv.dv.rerank_scores(src.raw[p:p + 1], [np.array([0, lv.n], np.int32)], 1)
        elif what == "wait_with_nothing_in_flight":
            assert not lv.inflight
            call = lv.ix.shard_scan_wait
        elif what == "third_begin":
            assert len(lv.inflight) == 2
            call = lambda: self.begin(lv, {"q0": p, "nq": 1, "k": 3}, False)
        elif what == "append_with_unwaited_batch":
            assert lv.inflight
            call = lambda: lv.ix.append_rows(src.codes[:5], src.corr[:5])
        else:
            raise ValueError(what)
        refused(call, code, msg)
        assert lv.ix.n == lv.n == capi.lib().bbq_index_size(lv.ix._h), msg

    # ------------------------------------------------------------------------------------------------ one step
    def step(self, i):
        s, msg = self.steps[i], self.msg(i)
        lv, kind = self.live[s["member"]], s["kind"]
        if kind in ("search", "search_batch", "search_filtered_batch", "search_raw_batch", "range", "search_spans", "search_spans_filtered", "search_grouped",
                      "search_maxsim", "maxsim_groups", "rerank", "maxsim_rerank", "score_rows", "score_ords", "search_ords"):
            getattr(self, kind)(lv, s, msg)
        elif kind == "shard_scan":
            assert not lv.inflight, msg         # begin + wait, and waits are taken in begin order: the walk draws it on an idle member
            self.collected(lv, self.begin(lv, s, True), msg)
        elif kind == "shard_begin":
            lv.inflight.append(self.begin(lv, s, False))
        elif kind == "shard_wait":
            b = lv.inflight.pop(0)
            b["total"] = lv.ix.shard_scan_wait()
            self.collected(lv, b, msg)
        elif kind == "set_option":
            lv.ix.set_option(s["option"], s["value"])
            lv.options[s["option"]] = s["value"]
        elif kind == "stats":
            st = lv.ix.stats()
            assert min(st["candidates"], st["dense_fallbacks"], st["host_replays"], st["total_scan_launches"]) >= 0, msg
        elif kind == "reset_stats":
            lv.ix.reset_stats()
            st = lv.ix.stats()
            assert (st["total_scan_ms"], st["total_scan_bytes"], st["total_scan_launches"]) == (0, 0, 0), "%s: %s" % (msg, st)
        elif kind == "refused":
            self.refuse(lv, s, msg)
        elif kind == "recreate":                # with whatever it has in flight: the batches are gone with it
            lv.unhang()
            lv.ix.close()
            lv.create()
        elif kind == "append":
            src = lv.src_of
            lv.ix.append_rows(src.codes[s["rows"]], src.corr[s["rows"]])
            lv.grew(s["rows"])
            assert lv.ix.n == lv.n, msg
        elif kind == "save":
            src, prefix = lv.src_of, str(self.tmp / ("saved_%s" % lv.name))
            lv.ix.save(prefix, src.cen, src.sim)
            info = B.file_info(prefix)
            assert (info["n_rows"], info["dim"], info["row_base"]) == (lv.n, lv.m.dim, int(lv.rows[0])), msg
        else:
            raise ValueError(kind)

    def run(self):
        prev = None
        for i, s in enumerate(self.steps):
            with located(self.msg(i)):
                self.step(i)
            if prev is not None:
                self.transitions.add((prev, s["kind"]))
            prev = s["kind"]
        assert not any(lv.inflight for lv in self.live.values())


def played(play):
    try:
        play.run()
    except BaseException as e:
        if not isinstance(e, pytest.exit.Exception):    # after a HIP error nothing more touches the device, not even a close
            play.close()
        raise
    play.close()


def test_the_token_block_is_the_walks():
    assert capi.maxsim_token_block() == W.TOKEN_BLOCK


@pytest.mark.parametrize("seed", SEEDS)
def test_walk_of_mixed_calls_equals_the_oracle(seed, tmp_path):
    t0 = time.perf_counter()
    for name in {m.source for m in W.CAST.values()}:
        source(name)
    t1 = time.perf_counter()
    play = Play(seed, tmp_path)
    played(play)
    print("call walk seed %d: %d steps, %d distinct transitions between kinds, %.2f s (the oracle's pools: %.2f s before it); statistics held: %s"
          % (seed, len(play.steps), len(play.transitions), time.perf_counter() - t1, t1 - t0, play.stat_checks))


# ---------------------------------------------------------------------------------------------------- threads
def joined(threads, limit, what):
    """the threads end within the limit, or the session does without another call on the device"""
    deadline = time.monotonic() + limit
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    if any(t.is_alive() for t in threads):
        pytest.exit("%s: a thread is still inside the library after %.0f s - a hang; its cause is to be read from the code" % (what, limit), returncode=3)


class Thread(threading.Thread):
    def __init__(self, fn):
        super().__init__(daemon=True)
        self.fn, self.error = fn, None

    def run(self):
        try:
            self.fn()
        except BaseException as e:          # handed to the test's thread
            self.error = e


def raise_first(threads):
    for t in threads:
        if isinstance(t.error, pytest.exit.Exception):
            raise t.error
    for t in threads:
        if t.error is not None:
            raise t.error


class SharedPlay(Play):
    """a thread's read-only walk: its own index for most steps, and handles shared with the other threads for every fourth"""

    def __init__(self, seed, tmp, shared):
        super().__init__(seed, tmp, steps=W.read_only_walk(seed), members=("ties",))
        self.own, self.shared = self.live["ties"], shared
        self.foreign_filter = shared.foreign

    def step(self, i):
        s = self.steps[i]
        self.live["ties"] = self.shared if i % 4 == 3 and s["kind"] != "search_maxsim" else self.own     # (assert_maxsim sets an option)
        self.stats_are_mine = self.live["ties"] is self.own      # "of the last call": on a shared index that may be another thread's
        try:
            super().step(i)
            if s["kind"] != "refused":
                assert capi.lib().bbq_last_error() in (None, b""), "%s: another thread's refusal shows here: %r" % (self.msg(i), capi.lib().bbq_last_error())
        finally:
            self.live["ties"] = self.own


def test_threads_share_read_only_handles(tmp_path):
    """four threads, a read-only walk each: every answer the oracle's, and a thread's bbq_last_error is its own"""
    source("ties_cos_qb4")
    shared = Live("ties", tmp_path)
    small = B.Index(shared.src_of.codes[:100], shared.src_of.corr[:100], 64, shared.src_of.cdp)
    shared.foreign = capi.Filter(small, np.ones(100, bool))
    plays = [SharedPlay(seed, tmp_path, shared) for seed in range(4)]

    def close_all():
        for p in plays:
            p.close()
        shared.foreign.close()
        small.close()
        shared.close()

    try:
        t0 = time.perf_counter()
        for p in plays:                      # the same work on one thread first: its time sets the limit
            p.run()
        T = time.perf_counter() - t0
        threads = [Thread(p.run) for p in plays]
        t0 = time.perf_counter()
        for t in threads:
            t.start()
        joined(threads, max(60.0, 20 * T), "shared read-only handles")
        print("shared handles: %.2f s on one thread, %.2f s on four" % (T, time.perf_counter() - t0))
        raise_first(threads)
    except BaseException as e:
        if not isinstance(e, pytest.exit.Exception):
            close_all()
        raise
    close_all()


def test_search_beside_append(tmp_path):
    """one thread appends 6 blocks of 100 rows to an index of 2 000 while another searches it 40 times: every call's answers are the
    oracle's over the first 2 000 + 100 j rows for one j, the same for its five queries, and j never decreases.  The appending thread
    hands block j over once 5 (j + 1) searches have come back, so the appends fall among the searches and not before or behind them;
    which j a later search sees is the scheduler's business and is printed, not asserted"""
    src = source("ties_cos_qb4")
    N0, BLOCK, M, CALLS, NQ, K = 2000, 100, 6, 40, 5, 10
    pqs = np.arange(NQ)
    # the fixture is 40 vectors many times each, so a block of later copies changes no answer: the rows go in by query 0's score,
    # ascending - every block then brings scores above all that came before it, and every state answers differently
    total = N0 + BLOCK * M
    order = np.argsort(src.scores[0][2][:total], kind="stable")
    codes, corr = np.ascontiguousarray(src.codes[order]), np.ascontiguousarray(src.corr[order])
    s32 = [src.scores[p][2][order] for p in pqs]
    want = [[O.heap_topk(s32[p][:N0 + BLOCK * j], K) for p in pqs] for j in range(M + 1)]

    def j_of(idx, sc, cnt):
        for j in range(M + 1):
            if all(cnt[q] == K and np.array_equal(idx[q], want[j][q][0]) and np.array_equal(canon32(sc[q]), canon32(want[j][q][1])) for q in range(NQ)):
                return j
        return None

    states = {b"".join(w[0].tobytes() + w[1].tobytes() for w in want[j]) for j in range(M + 1)}
    assert len(states) == M + 1, "the appended blocks hardly change the answers: the searches could not tell the states apart"

    EVERY = 5      # searches between two appends: block j goes in once 5 (j + 1) searches have come back, while the next ones run

    def work(ix, seen, threaded):
        gates = [threading.Event() for _ in range(M)]

        def append():
            for j in range(M):
                assert gates[j].wait(60.0), "the searches stand still"
                ix.append_rows(codes[N0 + BLOCK * j:N0 + BLOCK * (j + 1)], corr[N0 + BLOCK * j:N0 + BLOCK * (j + 1)])

        def search():
            for i in range(CALLS):
                seen.append(ix.search_batch(src.qq[pqs], src.qc[pqs], src.qb, src.sim, K))
                if (i + 1) % EVERY == 0 and (i + 1) // EVERY <= M:
                    gates[(i + 1) // EVERY - 1].set()

        if not threaded:
            search()
            append()
            return []
        threads = [Thread(append), Thread(search)]
        for t in threads:
            t.start()
        return threads

    ix = make_index(codes[:N0], corr[:N0], 64, src.cdp, False)
    twin = None
    try:
        with located("search beside append"):
            first = make_index(codes[:N0], corr[:N0], 64, src.cdp, False)
            try:
                t0 = time.perf_counter()
                work(first, [], False)
                T = time.perf_counter() - t0
            finally:
                first.close()
            seen = []
            threads = work(ix, seen, True)
            joined(threads, max(60.0, 20 * T), "search beside append")
            raise_first(threads)
            js = [j_of(*r) for r in seen]
            assert len(js) == CALLS and None not in js, "a call's answers are no single state of the index: %s" % js
            assert js == sorted(js), "the index went back in time: %s" % js
            assert js[:EVERY] == [0] * EVERY, "no block had been handed over when these came back: %s" % js
            print("search beside append: the searches saw j = %s" % js)
            n = N0 + BLOCK * M
            assert ix.n == n == capi.lib().bbq_index_size(ix._h)
            check_export(ix, codes[:n], corr[:n], "after the appends")
            twin = make_index(codes[:n], corr[:n], 64, src.cdp, False)
            a, b = ix.search_batch(src.qq[pqs], src.qc[pqs], src.qb, src.sim, K), twin.search_batch(src.qq[pqs], src.qc[pqs], src.qb, src.sim, K)
            assert j_of(*a) == M and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    except BaseException as e:
        if not isinstance(e, pytest.exit.Exception):
            ix.close()
            if twin is not None:
                twin.close()
        raise
    ix.close()
    twin.close()
