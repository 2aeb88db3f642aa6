"""GPU: bbq_stats.candidates of every sparse search held to the model of tests/candidate_model.py - an exact function of the oracle's f32
scores and the call's segment plan - with no tolerance, beside the answers themselves (O.heap_topk, bit for bit) and dense_fallbacks.

The answers have k witnesses per query for the code most likely to be subtly wrong: the score bounds that decide which rows reach the
exact path, and the running thresholds they are tested against.  A bound that rejects a row above the running threshold shows in the
answer only if that row is still among the best k at the end; a threshold that is stale, late or of the wrong rank shows nowhere, it
only lists more rows.  The count makes every row above every running threshold a witness, in both directions.

Every check names in its failure message which of the three assertions failed, the model's count per query and its split over the
segments.  tests/test_candidate_model_cpu.py holds the model to brute force and the recipe to its conditions.

A BBQ_ERR_HIP from any call ends the whole pytest session (test_gpu_mutation_walk.located)."""
import collections
import contextlib

import numpy as np
import pytest

import call_walk as W
import candidate_model as M
import orclib as O
from bbqlib import bbq_amd as B, capi
from test_gpu_fast_bound import bits32
from test_gpu_mutation_walk import located

pytestmark = pytest.mark.gpu

LAYOUTS = ("compact", "inline")
SHORT = tuple(f for f in M.FAMILIES if f.name != "long")
LATENCY = tuple(M.BY_NAME[n] for n in ("w6", "w8", "w12"))
EIGHT = (0, 1, 2, 3, 4, 5, 0, 1)           # more than latency_queries: the chunk-slot mode
PAIRS = ((0, 1), (2, 3), (4, 5))           # at most latency_queries: the append mode
TALLY = collections.defaultdict(lambda: [0, 0])      # family -> [calls compared, model candidates]

_held = {}
_heaps = {}


class Held:
    """an open index and the options in force on it, which the model reads"""

    def __init__(self, fam, layout, codes, corr):
        self.fam, self.layout = fam, layout
        self.ix = B.Index(codes, corr, fam.dim, M.CDP, index_bits=fam.index_bits, corrections=layout)
        self.opts = {}
        for name, value in M.plan_of(fam).items():
            self.set(name, value)

    def set(self, name, value):
        self.ix.set_option(name, value)
        self.opts[name] = value

    @contextlib.contextmanager
    def options(self, **values):
        before = {name: M.option(self.opts, name) for name in values}
        try:
            for name, value in values.items():
                self.set(name, value)
            yield self
        finally:
            for name, value in before.items():      # (host state only)
                self.set(name, value)


def held(fam, kind, layout):
    if (fam, kind, layout) not in _held:
        _held[fam, kind, layout] = Held(fam, layout, *M.rows(fam, kind))
    return _held[fam, kind, layout]


@pytest.fixture(scope="module", autouse=True)
def _close_and_tally():
    yield
    for h in _held.values():
        h.ix.close()
    _held.clear()
    for name, (calls, cand) in TALLY.items():
        print("candidate count: family %s: %d calls compared, %d model candidates" % (name, calls, cand))


def want(s32, k, mask, key):
    """the oracle's answer; key: what names these scores for good (None: not kept)"""
    if key is not None and (key, k) in _heaps:
        return _heaps[key, k]
    if mask is None:
        out = O.heap_topk(s32, k)
    else:
        acc = np.flatnonzero(mask)
        pos, sc = O.heap_topk(s32[acc], k)
        out = acc[pos].astype(np.int32), sc
    if key is not None:
        _heaps[key, k] = out
    return out


def check(h, scores, qq, qc, qb, sim, k, msg, keys=None, mask=None, flt=None):
    """ONE call: the answers, dense_fallbacks and candidates against the oracle and the model; returns the model's counts"""
    model = M.search_count(h.fam, scores, k, h.opts, mask)
    with located(msg):
        if flt is None:
            idx, sc, cnt = h.ix.search_batch(qq, qc, qb, sim, k)
        else:
            idx, sc, cnt = h.ix.search_filtered_batch(qq, qc, qb, sim, k, flt)
        st = h.ix.stats()
    bad = []
    for q, s in enumerate(scores):
        wi, ws = want(s, k, mask, None if keys is None else keys[q])
        if cnt[q] != len(wi) or (idx[q, :cnt[q]] != wi).any() or (bits32(sc[q, :cnt[q]]) != bits32(ws)).any():
            bad.append("ANSWER of query %d: rows %s, the oracle's %s" % (q, idx[q, :cnt[q]][:12], wi[:12]))
    flagged = sum(c.flagged for c in model)
    if st["dense_fallbacks"] != flagged:
        bad.append("DENSE_FALLBACKS %d, the model's %d" % (st["dense_fallbacks"], flagged))
    total = sum(c.count for c in model)
    if st["candidates"] != total:
        bad.append("CANDIDATES %d, the model's %d (%+d): %s" % (st["candidates"], total, st["candidates"] - total, M.describe(model)))
    assert not bad, "%s, k %d, options %s\n%s" % (msg, k, h.opts, "\n".join(bad))
    TALLY[h.fam.name][0] += 1
    TALLY[h.fam.name][1] += total
    return model


def call(h, kind, sim, which, k, msg, qb=None, **kw):
    """check() of the recipe's queries `which` (indices into the six) on the held index of `kind`"""
    qq, qc = M.queries(h.fam, sim, qb)
    sc = M.scores(h.fam, kind, sim, qb)
    which = list(which)
    mask_key = kw.pop("mask_key", None)
    keys = [(h.fam.name, kind, sim, qb, q, mask_key) for q in which]
    return check(h, [sc[q] for q in which], qq[which], qc[which], qb or h.fam.query_bits, sim, k, "%s %s %s sim %d %s" % (h.fam.name, kind, h.layout, sim, msg),
                 keys=keys, **kw)


CELLS = [(f, kind) for f in SHORT for kind in M.ROW_KINDS]
CELL_IDS = ["%s-%s" % (f.name, kind) for f, kind in CELLS]


@pytest.mark.parametrize("fam,kind", CELLS, ids=CELL_IDS)
def test_per_query_sweep(fam, kind):
    """the pipelined per-query sweep in chunk-slot mode (8 queries) and in append mode (2), both layouts, both forms of the bound"""
    for layout in LAYOUTS:
        h = held(fam, kind, layout)
        for fast in (1, 0):
            with h.options(fast_bound=fast):
                for sim in M.SIMS:
                    for k in M.KS:
                        call(h, kind, sim, EIGHT, k, "8 queries")
                        for pair in PAIRS:
                            call(h, kind, sim, pair, k, "queries %s, append mode" % (pair,))


@pytest.mark.parametrize("fam", [M.BY_NAME["w6"], M.BY_NAME["w8"]], ids=["w6", "w8"])
@pytest.mark.parametrize("kind", M.ROW_KINDS)
def test_tiles_per_wave_and_digit_planes(fam, kind):
    h = held(fam, kind, "compact")
    for tiles in (1, 2, 4, 8):
        for planes in (1, 0):
            with h.options(tiles_per_wave=tiles, digit_planes=planes):
                for sim in M.SIMS:
                    for k in M.KS:
                        call(h, kind, sim, EIGHT, k, "8 queries")
                        call(h, kind, sim, PAIRS[1], k, "append mode")


@pytest.mark.parametrize("kind", M.ROW_KINDS)
def test_host_selected_answers(kind):
    """device_select 0: the thresholds have rank k, not k + 1, and the model's count moves with it"""
    fam = M.BY_NAME["w6"]
    for layout in LAYOUTS:
        h = held(fam, kind, layout)
        for sim in M.SIMS:
            for k in M.KS:
                on = call(h, kind, sim, EIGHT, k, "8 queries")
                with h.options(device_select=0):
                    off = call(h, kind, sim, EIGHT, k, "8 queries")
                    call(h, kind, sim, PAIRS[0], k, "2 queries")
                if kind == "ordinary" and k > 1:
                    assert sum(c.count for c in off) < sum(c.count for c in on)


@pytest.mark.parametrize("kind", M.ROW_KINDS)
def test_shared_sweeps(kind):
    """sweep_share 4 and 8 on w6; 32 - the matrix cores - on w6, w8 and w12 with 70 queries of 4 bits (the FP form) and of 7 (int8):
    the four queries with f32 images in one call, which sweeps on the matrix cores, and all six in another, which must not
    (mfma_query_ok, bbq_query.cpp) and lists the same rows; a multi-bit index falls back quietly"""
    w6 = M.BY_NAME["w6"]
    for layout in LAYOUTS:
        h = held(w6, kind, layout)
        for share in (4, 8):
            with h.options(sweep_share=share):
                for sim in M.SIMS:
                    for k in M.KS:
                        call(h, kind, sim, EIGHT, k, "8 queries")
    seventy4, seventy6 = [i % 4 for i in range(70)], [i % 6 for i in range(70)]
    for fam in LATENCY:
        for layout in LAYOUTS:
            h = held(fam, kind, layout)
            with h.options(sweep_share=32):
                for qb in (None, 7):
                    for sim in M.SIMS:
                        for k in (10, 100):
                            call(h, kind, sim, seventy4, k, "70 queries of 4", qb=qb)
                            st = h.ix.stats()
                            assert st["last_scan_bytes"] != st["last_scan_rows"] * h.ix.bytes_per_row, "not on the matrix cores"
                        call(h, kind, sim, seventy6, 10, "70 queries of 6", qb=qb)
    h = held(M.BY_NAME["multibit"], kind, "compact")
    with h.options(sweep_share=32):
        for sim in M.SIMS:
            call(h, kind, sim, seventy6, 10, "70 queries")


@pytest.mark.parametrize("fam", LATENCY, ids=[f.name for f in LATENCY])
@pytest.mark.parametrize("kind", M.ROW_KINDS)
def test_single_query_chain(fam, kind):
    """the segmented chain of ONE query at 1, 2, 4 and 8 query bits: every bbq_lat_scan_kernel instantiation.  Below 262144 rows
    latency_presample changes nothing"""
    for layout in LAYOUTS:
        h = held(fam, kind, layout)
        assert W.single_query_path(W.Member(fam.name, fam.dim, 1, 0, 4, fam.n, True, None, None, 0, 0), fam.n, 10, h.opts) == "chain"
        for presample in (1, 0):
            with h.options(latency_presample=presample):
                for qb in (1, 2, None, 8):
                    for sim in M.SIMS:
                        for q in range(6):
                            for k in (M.KS if qb is None else (10,)):
                                call(h, kind, sim, [q], k, "one query, %s bits" % (qb or 4), qb=qb)


@pytest.mark.parametrize("sim", M.LONG_SIMS)
@pytest.mark.parametrize("kind", M.ROW_KINDS)
def test_presampled_chain(kind, sim):
    """`long`: the count says which path answered - the pre-sampled list or, behind it, the segmented chain; they differ by thousands"""
    fam = M.LONG
    paths = collections.Counter()
    for layout in LAYOUTS:
        h = held(fam, kind, layout)
        for k in (1, 10, 100, 500):
            for q in range(6):
                launches = h.ix.stats()["total_scan_launches"]
                model = call(h, kind, sim, [q], k, "one query")
                paths[model[0].path] += 1
                assert h.ix.stats()["total_scan_launches"] == launches, "the general path ran"
        with h.options(latency_presample=0):
            for q in range(6):
                assert call(h, kind, sim, [q], 10, "one query")[0].path == "segments"
    assert paths["segments"] > 0 and (paths["presampled"] > 0 or (kind, sim) == ("hostile", 1))      # (hostile COSINE: several rows at +inf tie in every answer)


@pytest.mark.parametrize("sim", M.LONG_SIMS)
def test_presampled_chain_planted_ties(sim):
    """k + 2 copies of the best row in the sampled prefix: the threshold is the best score, the list is empty, the chain answers"""
    fam = M.LONG
    for k in (1, 4):
        codes, corr, s = M.long_tied(sim, k)
        qq, qc = M.queries(fam, sim)
        for layout in LAYOUTS:
            h = Held(fam, layout, codes, corr)
            try:
                model = check(h, [s], qq[:1], qc[:1], fam.query_bits, sim, k, "long tied %s sim %d" % (layout, sim))
                assert model[0].path == "segments" and h.ix.stats()["host_replays"] == 1
            finally:
                h.ix.close()


@pytest.mark.parametrize("fam", [M.BY_NAME["w1"], M.BY_NAME["w6"]], ids=["w1", "w6"])
@pytest.mark.parametrize("kind", M.ROW_KINDS)
def test_filtered(fam, kind):
    """two masks on the pipelined sweep, and on w6 with sweep_share 32: the matrix-core kernels behind k_dev accepted rows"""
    for layout in LAYOUTS:
        h = held(fam, kind, layout)
        for label, mask in M.accept_sets(fam).items():
            with capi.Filter(h.ix, mask) as flt:
                for share in ((1, 32) if fam.name == "w6" else (1,)):
                    with h.options(sweep_share=share):
                        for sim in M.SIMS:
                            for k in M.KS:
                                which = [i % 4 for i in range(70)] if share == 32 else EIGHT
                                call(h, kind, sim, which, k, label, mask=mask, flt=flt, mask_key=label)
                                if share == 1:
                                    call(h, kind, sim, PAIRS[2], k, label + ", append mode", mask=mask, flt=flt, mask_key=label)


def test_after_mutation():
    """w6 compact, hostile kind.  update_rows gives a row of an ordinary tile an additionalCorrection of 1e300 - its tile must stop
    rejecting - and makes the planted +inf row ordinary - its tile must start; then an append of 100 rows crosses the ragged tile.
    Each count is the model's over the rows the index then holds"""
    fam = M.BY_NAME["w6"]
    codes, corr = (a.copy() for a in M.rows(fam, "hostile"))
    kinds = M.tile_kinds(fam)
    t_ord = 21
    assert kinds[t_ord] == "ordinary" and t_ord * M.TILE >= 1024
    ords = np.array([t_ord * M.TILE + 50, M.PLANT_TILES["add_pinf"] * M.TILE + M.H.PLANT_LANE], np.int32)
    assert corr[ords[1], 2] == np.inf
    ncodes, ncorr = M.H._ordinary(77, 2, fam)
    ncorr[0, 2] = 1e300
    acodes, acorr = M.H._ordinary(78, 100, fam)
    h = Held(fam, "compact", codes, corr)
    try:
        def everything(msg):
            for sim in M.SIMS:
                qq, qc = M.queries(fam, sim)
                sc = [M.score(fam, codes, corr, qq[q], qc[q], sim) for q in range(6)]
                assert not any(np.isnan(s).any() for s in sc)
                h.fam = fam._replace(n=len(codes))
                for k in (10, 100):
                    check(h, [sc[q] for q in EIGHT], qq[list(EIGHT)], qc[list(EIGHT)], fam.query_bits, sim, k, "w6 %s sim %d, 8 queries" % (msg, sim))
                    check(h, sc[:2], qq[:2], qc[:2], fam.query_bits, sim, k, "w6 %s sim %d, append mode" % (msg, sim))
                    check(h, sc[:1], qq[:1], qc[:1], fam.query_bits, sim, k, "w6 %s sim %d, one query" % (msg, sim))
        with located("update"):
            h.ix.update_rows(ords, ncodes, ncorr)
        codes[ords], corr[ords] = ncodes, ncorr
        everything("after the update")
        with located("append"):
            h.ix.append_rows(acodes, acorr)
        codes, corr = np.concatenate([codes, acodes]), np.concatenate([corr, acorr])
        assert len(codes) // M.TILE > fam.n // M.TILE
        everything("after the append")
    finally:
        h.ix.close()


def test_nan_flags_the_query():
    """one NaN correction behind the first segment: every query is flagged, counts every row and falls back - on the batch path, in
    append mode, on the segmented single-query chain and on the pre-sampled one"""
    for fam, row in ((M.BY_NAME["w6"], 5000), (M.LONG, 100000)):
        codes, corr = M.rows(fam, "ordinary")
        corr = corr.copy()
        corr[row, 2] = np.nan
        sim = 1
        qq, qc = M.queries(fam, sim)
        nqs = (8, 2, 1) if fam.name == "w6" else (1,)
        sc = [M.score(fam, codes, corr, qq[q], qc[q], sim) for q in range(2)]
        assert all(np.isnan(s[row]) and np.isnan(s).sum() == 1 for s in sc)
        h = Held(fam, "compact", codes, corr)
        try:
            for nq in nqs:
                which = [i % 2 for i in range(nq)]
                model = check(h, [sc[q] for q in which], qq[which], qc[which], fam.query_bits, sim, 10, "%s with a NaN row, %d queries" % (fam.name, nq))
                st = h.ix.stats()
                assert all(c.flagged for c in model) and st["candidates"] == nq * fam.n and st["dense_fallbacks"] == nq
        finally:
            h.ix.close()
