"""GPU: the count pass of the range search on the matrix-core shared sweep - bbq_count_range_batch / bbq_search_range_batch under
sweep_share 32 (bbq_range_mfma_kernel).  Every comparison is exact: counts, offsets, ascending ords and f32 score bits equal range_answer
over the oracle's f32 scores, and equal the bytes the same handle returns under sweep_share 1 (the per-query count).  The kernel flags
the queries it cannot count - no positive finite interval width, a key below every score, a full survivor queue - and the host counts
those per query inside the same sub-batch, so a call mixes both; `selective` holds each call to inputs of which the kernel itself decides
at least half: a query whose passing rows in any one 64-row tile are at most 4 fills at most its share (1 / 32) of the 128-entry queue.

Rows per chunk: 512.  The shapes the kernel can go wrong at: a ragged last tile, a chunk whose last waves have no tile, one and two
groups of 32 queries per workgroup and a ragged third group in a second workgroup row, the four compiled widths, the FP form at S = 1,
1/2, 1/4 (query values <= 3, 7, 15) and the int8 form (<= 127), and two chunks per workgroup (more than 512 workgroups' worth)."""
import functools

import numpy as np
import pytest

import orclib as O
import range_hostile as H
from test_gpu_range import bits
from test_range_key_cpu import range_answer
from bbqlib import bbq_amd as B, capi

pytestmark = pytest.mark.gpu

LAYOUTS = ("compact", "inline")
TILE = 64


def selective(gold, ths, mask=None):
    """queries whose threshold the survivor queue holds: at most 4 passing rows in any tile (module docstring)"""
    out = []
    for q, (g, t) in enumerate(zip(gold, ths)):
        p = np.zeros(-(-len(g) // TILE) * TILE, bool)
        w = range_answer(g, t)
        p[w if mask is None else w[mask[w]]] = True
        out.append(p.reshape(-1, TILE).sum(axis=1).max() <= 4)
    return np.array(out)


def run(ix, qb, sim, qq, qc, ths, gold, msg, flt=None, mask=None):
    """search and count under sweep_share 32 held to range_answer, then under sweep_share 1: the same bytes"""
    want = [range_answer(g, t) for g, t in zip(gold, ths)]
    if mask is not None:
        want = [w[mask[w]] for w in want]
    sizes = [len(w) for w in want]
    got = []
    try:
        for share in (32, 1):
            ix.set_option("sweep_share", share)
            idx, sc, off = ix.search_range_batch(qq, qc, qb, sim, ths, flt)
            cnt = ix.count_range_batch(qq, qc, qb, sim, ths, flt)
            got.append((idx.tobytes(), bits(sc).tobytes(), off.tobytes(), cnt.tobytes()))
            if share == 1:
                break
            np.testing.assert_array_equal(cnt, sizes, err_msg=msg + ": counts")
            np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(sizes)]), err_msg=msg + ": offsets")
            for q, w in enumerate(want):
                sl = slice(off[q], off[q + 1])
                np.testing.assert_array_equal(idx[sl], w, err_msg="%s: query %d threshold %r" % (msg, q, ths[q]))
                np.testing.assert_array_equal(bits(sc[sl]), bits(gold[q][w]), err_msg="%s: query %d: score bits" % (msg, q))
        assert got[0] == got[1], msg + ": sweep_share 32 and 1 differ"
    finally:
        ix.set_option("sweep_share", 32)


@functools.lru_cache(maxsize=None)
def case(dim, qb, n, nq, sim=1):
    """seeded rows through the product's quantizer, nq queries that are noisy copies of rows, the oracle's f32 scores: read-only"""
    rng = np.random.default_rng(7000 + dim + 10 * qb)
    base = rng.standard_normal((n, dim)).astype(np.float32)
    queries = (base[rng.permutation(n)[:nq]] + 0.5 * rng.standard_normal((nq, dim))).astype(np.float32)
    codes, corr, cen = B.quantize_vectors(base, sim, 1)
    cdp = B.centroid_dp(cen)
    qq, qc = B.quantize_queries(queries, cen, sim, qb)
    gold = [O.score_all(codes, corr, dim, qq[q], qc[q], qb, sim, cdp)[2] for q in range(nq)]
    return codes, corr, cdp, qq, qc, gold


def kth(gold, k):
    return np.array([np.sort(g)[-k] for g in gold], np.float32)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_count_ran_on_the_matrix_cores(layout):
    """64 queries at 768-d: the call reports a sweep that loads every tile once for 64 (or 32) queries; under sweep_share 1 it reports
    nothing, as before"""
    dim, qb, nq, sim = 768, 4, 64, 1
    codes, corr, cdp, qq, qc, gold = case(dim, qb, 2 * 512 + 64 + 37, nq)
    ths = kth(gold, 10)
    ix = B.Index(codes, corr, dim, cdp, corrections=layout)
    try:
        row_bytes = 16 * 6 + 24 if layout == "compact" else ix.bytes_per_row
        ix.reset_stats()
        ix.set_option("sweep_share", 32)
        cnt = ix.count_range_batch(qq, qc, qb, sim, ths)
        np.testing.assert_array_equal(cnt, [len(range_answer(g, t)) for g, t in zip(gold, ths)])
        st = ix.stats()
        print("sweep_share 32: last_scan_rows %d last_scan_bytes %d" % (st["last_scan_rows"], st["last_scan_bytes"]))
        assert st["last_scan_rows"] > 0 and st["last_scan_rows"] % 64 == 0
        assert st["last_scan_bytes"] in [(st["last_scan_rows"] // 64) * ((64 + S - 1) // S) * row_bytes for S in (64, 32)]
        ix.reset_stats()
        ix.set_option("sweep_share", 1)
        np.testing.assert_array_equal(ix.count_range_batch(qq, qc, qb, sim, ths), cnt)
        assert ix.stats()["last_scan_rows"] == 0
    finally:
        ix.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("sim", H.SIMS)
@pytest.mark.parametrize("name", ("main", "wide"))
def test_the_hostile_recipe(name, sim, layout):
    """H.pairs in one call: ordinary queries beside queries outside the f32 images (flagged by the host), thresholds of edge floats,
    +-inf and the queries' own scores (the prologue's flag, the overflow, exact equality); main also under H.accept_sets.  The table is
    H.pairs as it stands: 36 to 39 of its 120 eligible pairs are selective (the others pass hundreds of rows and are counted per query),
    so this case asserts a quarter where the other cases assert half"""
    fam = H.BY_NAME[name]
    qqs, qcs, ths, who = H.pairs(fam, sim)
    per_query = [s[2] for s in H.scores(fam, sim)]
    gold = [per_query[q] for q in who]
    eligible = who < 4             # queries 4 and 5 (intervals x 1e60, x 1e-60) are not mfma_query_ok
    codes, corr = H.rows(fam)
    ix = B.Index(codes, corr, fam.dim, H.CDP, index_bits=fam.index_bits, corrections=layout)
    try:
        sel = selective(gold, ths)
        print("%s sim %d: %d of %d eligible pairs are selective" % (name, sim, sel[eligible].sum(), eligible.sum()))
        assert 4 * sel[eligible].sum() >= eligible.sum()
        run(ix, fam.query_bits, sim, qqs, qcs, ths, gold, "%s sim %d %s" % (name, sim, layout))
        for label, mask in (H.accept_sets(fam).items() if name == "main" else ()):
            assert 4 * selective(gold, ths, mask=mask)[eligible].sum() >= eligible.sum()
            with capi.Filter(ix, mask) as flt:
                run(ix, fam.query_bits, sim, qqs, qcs, ths, gold, "%s sim %d %s, %s" % (name, sim, layout, label), flt, mask)
    finally:
        ix.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dim,qb", [(64, 2), (700, 3), (1024, 4), (1536, 7), (64, 7), (1536, 4)])
def test_forms_and_widths(dim, qb, layout):
    """W = 1, a ragged 6, 8, 12; S = 1, 1/2, 1/4 and int8 by the call's largest query value; 1, 9, 33 and 70 queries (a call of fewer
    than 8 queries keeps the per-query count: 9 is the one-group launch); thresholds at the 10th
    best score, and one query of each call at its median: only that query overflows the queue and is counted per query"""
    n, sim = 2 * 256 + 64 + 37, 1
    codes, corr, cdp, qq, qc, gold = case(dim, qb, n, 70)
    assert int(qq.max()) <= {2: 3, 3: 7, 4: 15, 7: 127}[qb] and int(qq.max()) > {2: 1, 3: 3, 4: 7, 7: 15}[qb]      # the form meant
    ix = B.Index(codes, corr, dim, cdp, corrections=layout)
    try:
        for nq in (1, 9, 33, 70):
            ths = kth(gold[:nq], 10)
            if nq > 1:
                ths[nq // 2] = np.median(gold[nq // 2])
            sel = selective(gold[:nq], ths)
            assert 2 * sel.sum() >= nq and (nq == 1 or not sel[nq // 2])
            run(ix, qb, sim, qq[:nq], qc[:nq], ths, gold[:nq], "%d-d qb %d %s, %d queries" % (dim, qb, layout, nq))
    finally:
        ix.close()


@pytest.mark.parametrize("n", (600 * 256 + 100, 600 * 512 + 100))
def test_several_chunks_per_workgroup(n):
    """64-d, 33 queries (two groups in one workgroup row): 301 and 601 chunks of 512 rows - the launch gives a workgroup one chunk up to
    512 of them and two beyond, so the second size is the one that walks; unfiltered, and under a filter that clears a run of whole
    chunks in the middle (the walk skips them)"""
    dim, qb, nq, sim = 64, 4, 33, 1
    codes, corr, cdp, qq, qc, gold = case(dim, qb, n, nq)
    ths = kth(gold, 10)
    mask = np.ones(n, bool)
    mask[100 * 512 + 64:107 * 512] = False
    ix = B.Index(codes, corr, dim, cdp, corrections="compact")
    try:
        assert selective(gold, ths).all()
        run(ix, qb, sim, qq, qc, ths, gold, "%d rows" % n)
        with capi.Filter(ix, mask) as flt:
            run(ix, qb, sim, qq, qc, ths, gold, "%d rows, chunks cleared" % n, flt, mask)
    finally:
        ix.close()
