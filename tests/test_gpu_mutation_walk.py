"""GPU: a mutated index held to a row-list model over seeded random walks of its mutations (tests/mutation_walk.py): appends, updates,
compactions, reserves, save + load and refused calls in one sequence, because each of them leaves state - capacity slack, the padding
lanes of a partial last tile, per-tile add ranges, the record format - that only a LATER, different mutation can trip over.
include/bbq.h promises that after any mutation the index is indistinguishable from one created whole over the resulting rows.  So
after EVERY step the library is held against the model (size, capacity, record format) and against a twin created whole over
pool[model.src]: export, the bytes of both files, bbq_score_rows, every search entry point against the oracle's heaps, filters made
before the step, bbq_score_ords, and - on every fifth step and the last - the other sweep variants and a sharded scan.  The fp32 side
of the rerank recipe (bbq_vectors_*) takes every step alongside.  Bit-exact (canon32, canon64): no tolerances.  The rows of a walk
are drawn from a pool with replacement, so tied scores are everywhere.  A failure names flavour, layout, seed, step and operation:
the steps up to there, printed by mutation_walk.describe, replay it as a fixed sequence.  tests/test_mutation_walk_cpu.py asserts
what the default walks cover.
A BBQ_ERR_HIP from any call means the device itself has failed: the file then ends the WHOLE pytest session (pytest.exit) and does
not even close its handles, so that nothing more is started on a device in that state - every later test file is cancelled with it.
A flavour whose scores hold NaN (edge_dim1) has every query flagged by the sharded scan, as include/bbq.h says ("could not bound the
query ... must be scored densely"); those queries are then answered on the dense path and compared with the oracle's heap there."""
import contextlib
import functools
import os

import numpy as np
import pytest

import mutation_walk as M
import orclib as O
from bbqlib import bbq_amd as B, capi
from test_gpu_append import Oracle, canon32, canon64, check_export, file_bytes, make_index
from test_gpu_compact import RowSet, row_set
from test_gpu_update import needs_sums

pytestmark = pytest.mark.gpu

SEEDS = tuple(range(int(os.environ.get("BBQ_WALK_SEEDS", str(M.DEFAULT_SEEDS)))))
VARIANTS = ({"force_dense": 1}, {"sweep_share": 4}, {"sweep_share": 32}, {"device_select": 0}, {"first_segment_rows": 1024, "segment_growth": 2})
RESET = {"force_dense": 0, "sweep_share": 1, "device_select": 1, "first_segment_rows": 4096, "segment_growth": 8}
WITH_VECTORS = "seeded_1000x129"   # the flavour whose walks carry a B.Vectors alongside, under both layouts


class SumsRowSet(RowSet):
    """the seeded pool with a handful of rows whose quantizedComponentSum is not their popcount: an index created over one of them
    stores explicit sums, takes any row and keeps storing them"""

    def __init__(self, odd_rows):
        plain = row_set("seeded_1000x129")
        self.__dict__.update(plain.__dict__)
        self.corr = plain.corr.copy()
        self.corr[list(odd_rows), 3] += 2.0
        self.orc = Oracle(self.codes, self.corr, self.dim, self.cen, self.sim, self.qb, self.queries, self.ib, self.lam, self.iters)


@functools.lru_cache(maxsize=None)
def pool(flavour):
    """the rows a flavour's walks draw from and the oracle's scores of all of them: computed once, shared, never written to"""
    fl = M.FLAVOURS[flavour]
    rs = SumsRowSet(fl.odd_rows) if fl.odd_rows else row_set(fl.pool)
    assert (rs.dim, rs.ib, rs.sim) == (fl.dim, fl.ib, fl.sim)
    assert needs_sums(rs.codes, rs.corr, rs.ib) == bool(fl.odd_rows)
    return rs


@contextlib.contextmanager
def located(msg):
    """whatever fails inside names the walk and the step"""
    try:
        yield
    except (AssertionError, B.BBQError) as e:
        if isinstance(e, B.BBQError) and e.code == capi.ERR_HIP:   # the device has failed: nothing more is started on it
            pytest.exit("%s\nHIP error: %s" % (msg, e), returncode=3)
        raise AssertionError("%s\n%s: %s" % (msg, type(e).__name__, e)) from e


def refused(call, code, msg):
    """the call is refused with this code; a call that goes through fails with the walk and the step in its message, as every failure"""
    try:
        call()
    except B.BBQError as e:
        if e.code == capi.ERR_HIP:
            raise
        assert e.code == code, "%s: refused with %d (%s), not %d" % (msg, e.code, e, code)
        return e
    raise AssertionError("%s: the call was not refused (BBQError %d expected)" % (msg, code))


class Walk:
    """one index - and, for one flavour, its fp32 side - taken through the steps of a walk"""

    def __init__(self, flavour, compact, seed, tmp_path):
        self.flavour, self.compact, self.seed, self.tmp = flavour, compact, seed, tmp_path
        self.rs, self.fl = pool(flavour), M.FLAVOURS[flavour]
        self.steps = M.walk(seed, self.rs.n, flavour)
        self.ix = self.dv = self.model = None
        self.codes = self.corr = None   # the rows the index holds, as they were handed over or as the device made them
        self.files = None               # the files of the index after the latest step

    def close(self):
        for h in (self.ix, self.dv):
            if h is not None:
                h.close()

    def msg(self, i):
        return "%s compact=%s seed %d step %d of %d: %s" % (self.flavour, self.compact, self.seed, i, len(self.steps) - 1, M.describe(self.steps[i]))

    def raw(self, rows):
        rs = self.rs
        return np.ascontiguousarray(rs.base[rows]), rs.cen, rs.sim, rs.lam, rs.iters

    def from_raw(self, got, rows, msg):
        """codes_out / corr_out of a raw block: pool row j's fp32 row quantized against the pool's centroid IS pool row j"""
        np.testing.assert_array_equal(got[0], self.rs.codes[rows], err_msg=msg + ": codes_out")
        np.testing.assert_array_equal(canon64(got[1]), canon64(self.rs.corr[rows]), err_msg=msg + ": corr_out")
        return got

    # ---------------------------------------------------------------------------------------------- the operations
    def create(self, step):
        rs, rows = self.rs, step["rows"]
        self.codes, self.corr = rs.codes[rows].copy(), rs.corr[rows].copy()
        self.ix = make_index(self.codes, self.corr, rs.dim, rs.cdp, self.compact, rs.ib)
        self.model = M.IndexModel(rows, needs_sums(rs.codes, rs.corr, rs.ib))
        if self.flavour == WITH_VECTORS:
            self.dv = B.Vectors(rs.base[rows].reshape(len(rows), rs.dim))

    def mutate(self, step, msg):
        rs, ix, dv, op = self.rs, self.ix, self.dv, step["op"]
        if op in ("append_rows", "append"):
            rows = step["rows"]
            if op == "append_rows":
                new = rs.codes[rows], rs.corr[rows]
                ix.append_rows(*new)
            else:
                new = self.from_raw(ix.append(*self.raw(rows)), rows, msg)
            self.codes, self.corr = np.concatenate([self.codes, new[0]]), np.concatenate([self.corr, new[1]])
            if dv is not None:
                dv.append(rs.base[rows].reshape(len(rows), rs.dim))
        elif op in ("update_rows", "update"):
            ords, frm = step["ords"], step["frm"]
            if op == "update_rows":
                new = rs.codes[frm], rs.corr[frm]
                ix.update_rows(ords, *new)
            else:
                new = self.from_raw(ix.update(ords, *self.raw(frm)), frm, msg)   # all rows of the block, duplicate losers included
            for i, o in enumerate(ords):   # applied in order: the last of equal ords wins
                self.codes[o], self.corr[o] = new[0][i], new[1][i]
            if dv is not None:
                dv.update(ords, rs.base[frm].reshape(len(frm), rs.dim))
        elif op in ("compact", "remove_rows"):
            n = ix.n
            mask = step["mask"] if op == "compact" else ~np.isin(np.arange(n), step["rows"])
            with capi.Filter(ix, mask) as flt:   # made before the index changes: the fp32 side follows by the same filter
                assert flt.count == int(mask.sum()), msg
                if op == "compact":
                    ix.compact(flt)
                else:
                    ix.remove_rows(step["rows"])
                if dv is not None:
                    dv.compact(flt)
            self.codes, self.corr = self.codes[mask], self.corr[mask]
        elif op == "reserve":
            ix.reserve(step["rows"])
        elif op == "save_load":
            prefix = str(self.tmp / "reload")
            ix.save(prefix, rs.cen, rs.sim)
            ix.close()
            self.ix, cen, info = B.Index.load(prefix)
            np.testing.assert_array_equal(cen.view(np.uint32), rs.cen.view(np.uint32), err_msg=msg)
            assert info["n_rows"] == len(self.codes), msg
        else:
            self.refuse(step, msg)
        M.apply(self.model, step)

    def refuse(self, step, msg):
        """a call the library must refuse, with the code and the position include/bbq.h states"""
        rs, ix, op, via, rows = self.rs, self.ix, step["op"], step["via"], step["rows"]
        if op in ("fail_nan", "fail_inf"):
            block, cen, sim, lam, iters = self.raw(rows)
            r, c = step["bad"]
            block[r, c] = step["value"]
            call = (lambda: ix.append(block, cen, sim, lam, iters)) if via == "append" else (lambda: ix.update(step["ords"], block, cen, sim, lam, iters))
            # COSINE validates the normalised rows: the row's norm is NaN, and with it its first value
            want = (capi.ERR_NAN_INPUT, r, 0) if sim == capi.COSINE else (capi.ERR_NAN_INPUT if op == "fail_nan" else capi.ERR_INF_INPUT, r, c)
            e = refused(call, want[0], msg)
            assert (e.bad_row, e.bad_col) == want[1:], "%s: reported at (%d, %d)" % (msg, e.bad_row, e.bad_col)
        elif op == "fail_ord":
            ords = step["ords"]
            call = {"update_rows": lambda: ix.update_rows(ords, rs.codes[rows], rs.corr[rows]), "update": lambda: ix.update(ords, *self.raw(rows)),
                    "remove_rows": lambda: ix.remove_rows(ords)}[via]
            refused(call, capi.ERR_INVALID_ARG, msg)
        else:
            codes, corr = rs.codes[rows].copy(), rs.corr[rows].copy()
            if op == "fail_code":   # 2^indexBits, and the sum stays the code sum: only the range is wrong
                r, d = step["bad"]
                corr[r, 3] += (1 << rs.ib) - float(codes[r, d])
                codes[r, d] = 1 << rs.ib
            else:
                corr[step["bad"][0], 3] += 1.0
            call = (lambda: ix.append_rows(codes, corr)) if via == "append_rows" else (lambda: ix.update_rows(step["ords"], codes, corr))
            refused(call, capi.ERR_INVALID_ARG if op == "fail_code" else capi.ERR_UNSUPPORTED, msg)

    # ---------------------------------------------------------------------------------------------- the checks
    def searches(self, ix, orc, msg):
        n = orc.n
        if n == 0:
            idx, sc, cnt = ix.search_batch(orc.qq, orc.qc, orc.qb, orc.sim, 5)
            assert (cnt == 0).all(), msg
        else:
            orc.check_search(ix, sorted({1, 10, 100, n, n + 5}), msg, single=True)

    def filtered(self, flt, acc, orc, msg):
        """a filter that still fits answers over the rows as they are now"""
        ix = self.ix
        assert flt.count == len(acc), msg
        for k in sorted({1, 10, len(acc) + 5}):
            idx, sc, cnt = ix.search_filtered_batch(orc.qq, orc.qc, orc.qb, orc.sim, k, flt)
            for qi in range(len(orc.qq)):
                pos, ws = O.heap_topk(orc.scores[qi][2][acc], k)
                assert cnt[qi] == len(pos), "%s filtered q%d k=%d" % (msg, qi, k)
                np.testing.assert_array_equal(idx[qi, :cnt[qi]], acc[pos], err_msg="%s filtered q%d k=%d" % (msg, qi, k))
                np.testing.assert_array_equal(canon32(sc[qi, :cnt[qi]]), canon32(ws), err_msg="%s filtered q%d k=%d" % (msg, qi, k))

    def shard_scan(self, orc, msg):
        import torch
        ix, n, k, nq = self.ix, orc.n, 10, len(orc.qq)
        cap = int(ix.shard_list_cap(k)) * nq
        d_packed = torch.zeros(cap, dtype=torch.int64, device="cuda")
        d_off = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
        d_flags = torch.zeros(nq, dtype=torch.int32, device="cuda")
        total = ix.shard_scan(orc.qq, orc.qc, orc.qb, orc.sim, k, d_packed.data_ptr(), cap, d_off.data_ptr(), d_flags.data_ptr())
        # a query with a NaN score cannot be bounded: the shard flags it and carries no entries for it (include/bbq.h), every other
        # query's list replays to the oracle's heap
        flags, off = d_flags.cpu().numpy(), d_off.cpu().numpy()
        nan = np.array([bool(np.isnan(orc.scores[qi][2]).any()) for qi in range(nq)])
        np.testing.assert_array_equal(flags != 0, nan, err_msg=msg + ": shard scan flags")
        assert (np.diff(off)[nan] == 0).all(), msg + ": a flagged query carries entries"
        idx, sc, cnt = B.replay_batch([d_packed[:total].cpu().numpy().view(np.uint64)], [off], nq, n, k)
        for qi in np.flatnonzero(~nan):
            wi, ws = orc.topk(qi, k)
            np.testing.assert_array_equal(idx[qi, :cnt[qi]], wi, err_msg="%s shard scan q%d" % (msg, qi))
            np.testing.assert_array_equal(canon32(sc[qi, :cnt[qi]]), canon32(ws), err_msg="%s shard scan q%d" % (msg, qi))
        if nan.any():   # a flagged query must be scored densely: do that, and compare what comes back
            ix.set_option("force_dense", 1)
            try:
                idx, sc, cnt = ix.search_batch(orc.qq, orc.qc, orc.qb, orc.sim, k)
            finally:
                ix.set_option("force_dense", RESET["force_dense"])
            for qi in np.flatnonzero(nan):
                wi, ws = orc.topk(qi, k)
                np.testing.assert_array_equal(idx[qi, :cnt[qi]], wi, err_msg="%s flagged q%d scored densely" % (msg, qi))
                np.testing.assert_array_equal(canon32(sc[qi, :cnt[qi]]), canon32(ws), err_msg="%s flagged q%d scored densely" % (msg, qi))

    def check(self, i, msg, refusal, extra, last):
        rs, ix, m = self.rs, self.ix, self.model
        src, n = m.src, m.size
        rng = np.random.default_rng([self.seed, i])
        # 1, 2: size and capacity
        assert ix.n == n == capi.lib().bbq_index_size(ix._h), "%s: size %d, the model has %d" % (msg, capi.lib().bbq_index_size(ix._h), n)
        assert ix.capacity == m.capacity, "%s: capacity %d, the model has %d" % (msg, ix.capacity, m.capacity)
        np.testing.assert_array_equal(self.codes, rs.codes[src], err_msg=msg)
        np.testing.assert_array_equal(canon64(self.corr), canon64(rs.corr[src]), err_msg=msg)
        # the twin: created whole over pool[src] (the rows as the device made them where it made them: they equal the pool's up to
        # the bits of a NaN, which a file keeps as they are)
        twin = make_index(self.codes, self.corr, rs.dim, rs.cdp, self.compact, rs.ib)
        whole_dv = None
        try:
            assert twin.capacity == M.tiles_of(n) * M.TILE, msg
            # 3: the record format is never re-decided
            same_format = not m.stores_sums or needs_sums(self.codes, self.corr, rs.ib)
            if same_format:
                assert ix.bytes_per_row == twin.bytes_per_row, "%s: %d bytes per row, the twin has %d" % (msg, ix.bytes_per_row, twin.bytes_per_row)
            else:
                assert ix.bytes_per_row > twin.bytes_per_row, msg
            # 4, 5: export and files; spare capacity must not show, and a refused call has changed nothing
            check_export(ix, rs.codes[src], rs.corr[src], msg)
            files = file_bytes(ix, str(self.tmp / "walked"), rs.cen, rs.sim)
            if same_format:
                want = file_bytes(twin, str(self.tmp / "twin"), rs.cen, rs.sim)
                assert files[1] == want[1], msg + ": the .vemb file is not the twin's"
                assert files[0] == want[0], msg + ": the .veb file is not the twin's"
            if refusal:
                assert files == self.files, msg + ": the files are not those from before the refused call"
            self.files = files
            # 6: scores and every search entry point against the oracle
            orc = rs.oracle_over(src)
            if n > 0:
                orc.check_score_rows(ix, msg)
            self.searches(ix, orc, msg)
            # 8: chosen rows, shuffled and with repeats
            if n > 0:
                ords = rng.integers(0, n, 150).astype(np.int32)
                for qi in range(len(orc.qq)):
                    d, s64, s32 = ix.score_ords(orc.qq[qi], orc.qc[qi], rs.qb, rs.sim, ords)
                    od, o64, o32 = orc.scores[qi]
                    np.testing.assert_array_equal(d, od[ords], err_msg=msg + ": score_ords")
                    np.testing.assert_array_equal(canon64(s64), canon64(o64[ords]), err_msg=msg + ": score_ords")
                    np.testing.assert_array_equal(canon32(s32), canon32(o32[ords]), err_msg=msg + ": score_ords")
            if extra and n > 0:
                for opts in VARIANTS:
                    for k_, v in opts.items():
                        ix.set_option(k_, v)
                    self.searches(ix, orc, "%s %s" % (msg, opts))
                    for k_ in opts:
                        ix.set_option(k_, RESET[k_])
                self.shard_scan(orc, msg)
            # the fp32 side in step
            if self.dv is not None:
                dv, queries = self.dv, rs.queries
                assert dv.n == n == capi.lib().bbq_vectors_size(dv._h), msg
                whole_dv = B.Vectors(rs.base[src].reshape(n, rs.dim))
                lists = [np.array([0, n - 1, n // 2, 0], np.int32) if n else np.zeros(0, np.int32), rng.integers(0, max(n, 1), 70 if n else 0).astype(np.int32)]
                lists = (lists + [np.zeros(0, np.int32)] * len(queries))[:len(queries)]
                for true_sim in (0, 1, 2):
                    for qi, (x, y) in enumerate(zip(dv.rerank_scores(queries, lists, true_sim), whole_dv.rerank_scores(queries, lists, true_sim))):
                        np.testing.assert_array_equal(canon64(x), canon64(y), err_msg="%s rerank_scores sim %d q%d" % (msg, true_sim, qi))
                if last and n > 0:
                    for selector in (0, 1):
                        got = B.search_rerank_batch(ix, dv, queries, orc.qq, orc.qc, rs.qb, rs.sim, 10, 5, selector, 1)
                        want = B.search_rerank_batch(twin, whole_dv, queries, orc.qq, orc.qc, rs.qb, rs.sim, 10, 5, selector, 1)
                        for a, b in zip(got, want):
                            np.testing.assert_array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8), err_msg="%s rerank selector %d" % (msg, selector))
        finally:
            twin.close()
            if whole_dv is not None:
                whole_dv.close()
        return orc

    def run(self):
        self.create(self.steps[0])
        with located(self.msg(0)):
            self.check(0, self.msg(0), False, False, False)
        for i in range(1, len(self.steps)):
            step, msg = self.steps[i], self.msg(i)
            with located(msg):
                n_before, ix_before = self.model.size, self.ix
                rng = np.random.default_rng([self.seed, i, 7])
                old = old_mask = None
                if n_before > 0:   # 7: a filter made before the step
                    old_mask = rng.random(n_before) < 0.5
                    old_mask[[0, n_before - 1]] = [True, rng.random() < 0.5]
                    old = capi.Filter(self.ix, old_mask)
                try:
                    self.mutate(step, msg)
                    last = i == len(self.steps) - 1
                    orc = self.check(i, msg, step["op"] in M.FAIL_KINDS, i % 5 == 0 or last, last)
                    if old is not None and self.ix is ix_before:
                        if self.model.size == n_before:    # the size is what the filter was made for: it still means the same ords
                            self.filtered(old, np.flatnonzero(old_mask), orc, msg + ": a filter made before")
                        else:                              # made for another size: refused, and nothing changes
                            refused(lambda: self.ix.search_filtered_batch(orc.qq, orc.qc, self.rs.qb, self.rs.sim, 3, old), capi.ERR_INVALID_ARG, msg)
                            assert capi.lib().bbq_index_compact(self.ix._h, old._h) == capi.ERR_INVALID_ARG, msg
                            assert self.ix.n == self.model.size == capi.lib().bbq_index_size(self.ix._h), msg
                finally:
                    if old is not None:
                        old.close()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("flavour", M.FLAVOURS)
def test_walk_equals_created_whole(flavour, compact, seed, tmp_path):
    w = Walk(flavour, compact, seed, tmp_path)
    try:
        w.run()
    except BaseException as e:
        if not isinstance(e, pytest.exit.Exception):   # after a HIP error nothing more touches the device, not even a close
            w.close()
        raise
    w.close()
