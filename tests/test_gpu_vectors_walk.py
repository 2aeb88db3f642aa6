"""GPU: the device-resident fp32 row store (bbq_vectors_*) held to a row-list model over seeded walks of its mutations
(tests/vectors_walk.py): appends that fit the capacity and appends that move the rows, updates, compactions by every mask shape and
refused calls in one sequence on one handle, at the widths on both sides of every path of the copy kernels.  Every exact entry point
reads these rows and promises computeSimilarity bit for bit, so after EVERY step

  1. the size is the model's - after a refused call too;
  2. every element of every row is read back: under MAXIMUM_INNER_PRODUCT the score of the one-hot query e_j against a finite row is
     float64(row[j]) + 0.0 (tests/test_vectors_walk_cpu.py holds the ORACLE to that), so rerank_scores of the dim one-hot queries
     over all rows must be pool[src].T widened, bit for bit - a failure names row and column;
  3. the same matrix comes back through the exact search, k = n, un-permuted by the rows it returns, which must be a permutation of
     all rows - with slabs of 256 rows and with automatic slabs, at up to 64 columns a step that move on with the steps;
  4. four random queries and the zero query under all three similarities: rerank_scores over all rows against the oracle's
     computeSimilarity, search_batch(k = 10) against tests/exact_model.py.

On the last step a twin created whole over pool[src] answers 2 to 4 byte for byte, and at the widths 65 and 768 the exact MaxSim
rerank over a small group layout equals the twin's.  Bit-exact: no tolerances.  A failure names width, seed, step and operation; the
steps up to there, printed by vectors_walk.describe, replay it as a fixed sequence.
A BBQ_ERR_HIP from any call means the device itself has failed: the file then ends the WHOLE pytest session (pytest.exit) and does not
even close its handles, so that nothing more is started on a device in that state."""
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest

import exact_model as EM
import orclib as O
import vectors_walk as W
from bbqlib import bbq_amd as B, capi

pytestmark = pytest.mark.gpu

SEEDS = tuple(range(int(os.environ.get("BBQ_VECTORS_WALK_SEEDS", str(W.DEFAULT_SEEDS)))))
SLABS = (256, 0)
MIP = O.SIMS["MAXIMUM_INNER_PRODUCT"]
INDEX_DIM, INDEX_ROWS = 64, W.MAX_ROWS + 2 * W.TILE


@functools.lru_cache(maxsize=None)
def _index_rows():
    rng = np.random.default_rng(7)
    codes, corr, cen = B.quantize_vectors(rng.standard_normal((INDEX_ROWS, INDEX_DIM)).astype(np.float32), 1)
    return codes, corr, B.centroid_dp(cen)


@functools.lru_cache(maxsize=32)
def _index(n):
    """an index of n rows: filters and groups hang on it - its dimension and rows are not the handle's"""
    codes, corr, cdp = _index_rows()
    return B.Index(codes[:n], corr[:n], INDEX_DIM, cdp)


def _filter(n, mask, padding=0):
    """a filter for n rows from the accept words themselves, the bits beyond the last row set where `padding` says so: they are ignored"""
    words = capi.pack_mask(mask)
    if padding and n % 64:
        words[-1] |= np.uint64(0xffffffffffffffff) << np.uint64(n % 64)
    h = C.c_void_p()
    capi._chk(capi.lib().bbq_filter_create(_index(n)._h, capi._ptr(words), words.shape[0], C.byref(h)))
    flt = capi.Filter.__new__(capi.Filter)
    flt._h = h
    assert flt.count == int(np.asarray(mask).sum())
    return flt


class Width:
    """what the walks of one width share: the pool, the queries, the oracle's scores of every pool row - computed once, never written to"""

    def __init__(self, pool, seed):
        self.pool, self.dim = pool, pool.shape[1]
        rng = np.random.default_rng([31, self.dim, seed])
        self.queries = np.concatenate([rng.standard_normal((4, self.dim)), np.zeros((1, self.dim))]).astype(np.float32)
        self.scores = [EM.scores(self.queries, pool, sim) for sim in (0, 1, 2)]
        self.onehot = np.eye(self.dim, dtype=np.float32)
        if np.isfinite(pool).all():
            self.elements = np.ascontiguousarray(pool.T.astype(np.float64) + 0.0)   # [dim, pool rows]: what e_j reads back
            self.elements.setflags(write=False)
        for a in (self.queries, self.onehot):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def width(dim):
    return Width(W.pool(dim), 0)


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
    try:
        call()
    except B.BBQError as e:
        if e.code == capi.ERR_HIP:
            raise
        assert e.code == code, "%s: refused with %d (%s), not %d" % (msg, e.code, e, code)
        return
    raise AssertionError("%s: the call was not refused (BBQError %d expected)" % (msg, code))


def same_bits(got, want, msg, name_cell=None):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, "%s: shape %s, not %s" % (msg, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    if len(bad):
        at = tuple(int(v) for v in bad[0])
        where = name_cell(at) if name_cell else "at %s" % (at,)
        raise AssertionError("%s: %d of %d values differ, the first %s: got %r (0x%016x), the model has %r (0x%016x)" % (
            msg, len(bad), got.size, where, got[at], int(got.view(np.uint64)[at]), want[at], int(want.view(np.uint64)[at])))


# ---------------------------------------------------------------------------------------------- what a handle answers
def read_back(V, wd):
    """check 2's question: every element of every row, [dim, n]"""
    every = np.arange(V.n, dtype=np.int32)
    return np.stack(V.rerank_scores(wd.onehot, [every] * wd.dim, MIP)).reshape(wd.dim, V.n)


def read_back_exact(V, wd, cols, slab):
    """check 3's question: the columns `cols` of every row through the exact search - (rows, scores, counts)"""
    V.set_option("exact_slab_rows", slab)
    try:
        return V.search_batch(wd.onehot[cols], V.n, MIP)
    finally:
        V.set_option("exact_slab_rows", 0)


def unpermuted(ans, n, msg):
    idx, out, cnt = ans
    assert (cnt == n).all() and idx.shape == out.shape == (len(cnt), n), "%s: counts %s, not %d" % (msg, sorted(set(cnt.tolist())), n)
    assert (np.sort(idx, axis=1) == np.arange(n)).all(), msg + ": the returned rows are not a permutation of all rows"
    m = np.empty(out.shape, np.float64)
    np.put_along_axis(m, idx.astype(np.int64), out, axis=1)
    return m


def fixed_queries(V, wd):
    """check 4's questions: [(name, array)]"""
    every = np.arange(V.n, dtype=np.int32)
    out = []
    for sim in (0, 1, 2):
        out.append(("rerank_scores sim %d" % sim, np.stack(V.rerank_scores(wd.queries, [every] * len(wd.queries), sim)).reshape(len(wd.queries), V.n)))
        for name, a in zip(("rows", "scores", "counts"), V.search_batch(wd.queries, 10, sim)):
            out.append(("search_batch k 10 sim %d %s" % (sim, name), a))
    return out


def check_fixed_queries(answers, wd, src, msg):
    n, a = len(src), dict(answers)
    for sim in (0, 1, 2):
        c = np.ascontiguousarray(wd.scores[sim][:, src])
        got = a["rerank_scores sim %d" % sim]
        assert EM.canon64(got).tolist() == EM.canon64(c).tolist(), "%s: rerank_scores under similarity %d is not the oracle's computeSimilarity" % (msg, sim)
        idx, out, cnt = (a["search_batch k 10 sim %d %s" % (sim, name)] for name in ("rows", "scores", "counts"))
        for q in range(len(wd.queries)):
            rows, bits = EM.topk(c[q], 10)
            w = "%s: search_batch k 10, similarity %d, query %d" % (msg, sim, q)
            assert cnt[q] == len(rows) == min(10, n), w + ": count"
            assert idx[q, :cnt[q]].tolist() == rows.tolist(), w + ": rows"
            assert out[q, :cnt[q]].view(np.uint64).tolist() == bits.tolist(), w + ": score bits"


def check_handle(V, wd, src, cols, msg):
    """checks 1 to 4 of one handle against the model; returns everything it answered, for the twin"""
    n = len(src)
    assert V.n == n == capi.lib().bbq_vectors_size(V._h), "%s: size %d, the model has %d" % (msg, capi.lib().bbq_vectors_size(V._h), n)
    want = wd.elements[:, src]
    answers = [("read-back", read_back(V, wd))]
    same_bits(answers[0][1], want, msg + ": read-back through rerank_scores",
              lambda at: "row %d column %d (pool row %d)" % (at[1], at[0], src[at[1]]))
    if n <= 4096:
        for slab in SLABS:
            ans = read_back_exact(V, wd, cols, slab)
            answers += [("exact slab %d %s" % (slab, name), a) for name, a in zip(("rows", "scores", "counts"), ans)]
            w = "%s: read-back through search_batch, k = n, exact_slab_rows %d" % (msg, slab)
            same_bits(unpermuted(ans, n, w), want[cols], w, lambda at: "row %d column %d (pool row %d)" % (at[1], cols[at[0]], src[at[1]]))
    fixed = fixed_queries(V, wd)
    check_fixed_queries(fixed, wd, src, msg)
    return answers + fixed


def maxsim_groups(V, wd, n):
    """the exact MaxSim rerank over a small fixed layout of four groups: the first rows, a run across tile edges, the rest but one, the last row"""
    off = np.array([0, 3, n // 2, n - 1, n], np.int64)
    with capi.Groups(_index(n), off) as groups:
        out = []
        for sim in (0, 1, 2):
            sc, coff = V.rerank_maxsim_groups_batch([wd.queries[:2], wd.queries[2:5]], groups, [np.array([0, 3, 2, 1, 0]), np.array([2, 1])], sim)
            out.append(sc.copy())
    return out


# ---------------------------------------------------------------------------------------------- the walk
def play(dv, step, wd, model, msg):
    """one step on the handle, and on the model"""
    pool, op, n = wd.pool, step["op"], model.size
    if op == "append":
        dv.append(pool[step["rows"]].reshape(len(step["rows"]), wd.dim))
    elif op == "update":
        dv.update(step["ords"], pool[step["frm"]].reshape(len(step["frm"]), wd.dim))
    elif op == "compact":
        flt = _filter(n, step["mask"], step["padding"])   # the accept words as the caller hands them over
        try:
            dv.compact(flt)
        finally:
            flt.close()
    elif op == "refuse_update":
        refused(lambda: dv.update(step["ords"], pool[step["frm"]].reshape(len(step["frm"]), wd.dim)), capi.ERR_INVALID_ARG, msg)
    elif op == "refuse_compact":
        other = step["bad"][0]
        flt = _filter(other, np.arange(other) % 2 == 0)
        try:
            refused(lambda: dv.compact(flt), capi.ERR_INVALID_ARG, msg)
        finally:
            flt.close()
    elif op == "refuse_append":
        refused(lambda: dv.append(np.ones((len(step["rows"]), step["bad"][0]), np.float32)), capi.ERR_DIM_MISMATCH, msg)
    else:
        raise ValueError(op)
    W.apply(model, step)


def run_walk(dim, seed, steps=None, holder=None):
    wd = width(dim)
    steps = W.walk(seed, dim) if steps is None else steps
    holder = {} if holder is None else holder
    model = W.VectorsModel(steps[0]["rows"])
    dv = holder["dv"] = B.Vectors(wd.pool[steps[0]["rows"]].reshape(len(steps[0]["rows"]), dim))
    answers = None
    for i, step in enumerate(steps):
        msg = "dim %d seed %d step %d of %d: %s" % (dim, seed, i, len(steps) - 1, W.describe(step))
        with located(msg):
            if i > 0:
                play(dv, step, wd, model, msg)
            answers = check_handle(dv, wd, model.src, W.exact_columns(seed, i, dim), msg)
    # the last step: a twin created whole over the resulting rows answers byte for byte
    msg = "dim %d seed %d after the last step" % (dim, seed)
    with located(msg):
        n, cols = model.size, W.exact_columns(seed, len(steps) - 1, dim)
        twin = holder["twin"] = B.Vectors(wd.pool[model.src].reshape(n, dim))
        theirs = check_handle(twin, wd, model.src, cols, msg + ": the twin")
        assert [name for name, _ in answers] == [name for name, _ in theirs]
        for (name, a), (_, b) in zip(answers, theirs):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), "%s: %s is not the twin's" % (msg, name)
        if dim in (65, 768):
            for sim, (a, b) in enumerate(zip(maxsim_groups(dv, wd, n), maxsim_groups(twin, wd, n))):
                assert a.tobytes() == b.tobytes(), "%s: rerank_maxsim_groups_batch under similarity %d is not the twin's" % (msg, sim)
    return model


def with_handles(fn):
    """run fn(holder); close what it opened - unless the device has failed: then nothing touches it, not even a close"""
    holder = {}
    try:
        fn(holder)
    except BaseException as e:
        if isinstance(e, pytest.exit.Exception):
            raise
        for h in holder.values():
            h.close()
        raise
    for h in holder.values():
        h.close()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("dim", W.WIDTHS)
def test_walk_equals_created_whole(dim, seed):
    with_handles(lambda holder: run_walk(dim, seed, holder=holder))


# ---------------------------------------------------------------------------------------------- rows that are not finite
@functools.lru_cache(maxsize=None)
def non_finite(dim):
    """the pool of a width with six rows behind it that a read-back cannot see through: NaN and +-Infinity among ordinary values, in the
    first and the last column, and a row of nothing but NaN"""
    rng = np.random.default_rng([32, dim])
    extra = rng.standard_normal((6, dim)).astype(np.float32)
    extra[0, 0] = np.nan
    extra[1, dim - 1] = np.nan
    extra[2, dim // 2] = np.inf
    extra[3, dim - 1] = -np.inf
    extra[4, 0], extra[4, dim - 1] = np.inf, -np.inf
    extra[5] = np.nan
    pool = np.concatenate([W.pool(dim), extra])
    pool.setflags(write=False)
    return Width(pool, 1)


@pytest.mark.parametrize("dim", [33, 260])
def test_non_finite_rows_arrive_where_the_model_says(dim):
    """NaN, +-Infinity and a whole-NaN row through one append, one update and one compaction, seen through check 4 alone: the copy paths
    carry them as they carry every other row"""
    wd = non_finite(dim)
    p, bad = wd.pool, np.arange(len(wd.pool) - 6, len(wd.pool))
    assert not np.isfinite(p[bad]).all(axis=1).any() and np.isnan(p[bad[5]]).all()
    rng = np.random.default_rng([33, dim])

    def body(holder):
        model = W.VectorsModel(rng.integers(0, W.N_NORMAL, 300))
        dv = holder["dv"] = B.Vectors(p[model.src])

        def check(msg):
            with located("dim %d, non-finite rows, %s" % (dim, msg)):
                assert dv.n == model.size == capi.lib().bbq_vectors_size(dv._h)
                for sim in (0, 1, 2):
                    assert np.isnan(wd.scores[sim][:, model.src]).any() == (msg != "created")
                check_fixed_queries(fixed_queries(dv, wd), wd, model.src, msg)

        check("created")
        rows = np.concatenate([rng.integers(0, W.N_NORMAL, 100), bad, rng.integers(0, W.N_NORMAL, 94)])   # across the old end's tile and beyond
        dv.append(p[rows])
        model.append(rows)
        check("after the append")
        ords = np.array([0, 63, 64, 299, 300, 499, 405, 64, 0], np.int64)   # row 405 held the whole-NaN row; rows 0 and 64 are named twice
        frm = np.array([bad[0], bad[1], bad[2], bad[3], 7, bad[4], 8, bad[5], 9], np.int64)
        dv.update(ords, p[frm])
        model.update(ords, frm)
        assert model.src[64] == bad[5] and model.src[0] == 9
        check("after the update")
        mask = rng.random(500) < 0.5
        mask[[63, 64, 299, 499]] = True
        mask[[400, 401, 402]] = False
        flt = _filter(500, mask, 1)
        try:
            dv.compact(flt)
        finally:
            flt.close()
        model.compact(mask)
        assert np.isin(bad[[1, 5, 3, 4]], model.src).all()
        check("after the compaction")

    with_handles(body)
