"""GPU: the MaxSim search's score pass on the matrix cores (maxsim_fused 2) against the model of tests/maxsim_model.py, bit for bit -
groups, score bits, order, counts and out_status - and beside maxsim_fused 1, whose bytes it must give.  One index of 1 080 rows (two
chunks and a 56-row last tile) per width, similarity and corrections layout; one group layout that holds every shape the kernel's
two-register segmented maximum can meet; one call with a query of 1, 31, 32, 33 and 70 tokens (empty lanes of a block, the block edge,
the f64 carry across blocks).  Hostile rows stand in single-row groups and inside larger ones."""
import functools

import numpy as np
import pytest

import orclib as O
import maxsim_model as M
from test_gpu_score_ords import canon32
from bbqlib import bbq_amd as B, capi

pytestmark = pytest.mark.gpu

N = 1080
TOKENS = (1, 31, 32, 33, 70)
SPANS = [(int(a), int(a + t)) for a, t in zip(np.cumsum((0,) + TOKENS[:-1]), TOKENS)]
# single rows; a group ending at row 31 of a tile and one beginning at its row 32; rows 30..33 of tile 1; all of tile 2; groups across a
# tile edge (250..259), three tiles (320..499) and a chunk edge (500..519); single rows over the second chunk edge; the last tile's rest
OFFSETS = np.array(list(range(11)) + [32, 40, 64, 94, 98, 128, 192, 250, 260, 320, 500, 520, 1000] + list(range(1001, 1031)) + [N], np.int64)


def _masks():
    m = {"all": np.ones(N, bool), "random_half": np.random.default_rng(5).random(N) < 0.5}
    for name, rejected in (("lower_half_out", list(range(64, 96)) + list(range(128, 160))),     # rows 0..31 of tiles 1 and 2
                           ("tile_out", range(256, 320)),                                       # all of tile 4
                           ("dead_groups", [5] + list(range(94, 98)))):                         # a single row's group and the seam's
        m[name] = np.ones(N, bool)
        m[name][list(rejected)] = False
    return m


@functools.lru_cache(maxsize=None)
def _case(dim, sim, qb=4):
    """rows, token vectors and the oracle's f32 score of every (vector, row); computed once, read-only"""
    rng = np.random.default_rng(1000 * dim + sim)
    codes, corr, cen = B.quantize_vectors(rng.standard_normal((N, dim)).astype(np.float32), sim)
    corr = corr.copy()
    corr[[3, 60], 1] = corr[[3, 60], 0]                    # zero interval width: a single row, a row inside a group
    corr[[7, 130], 1] = corr[[7, 130], 0] - 0.01           # negative width
    corr[[9, 300], 2] = 3e38
    corr[[1002, 330], 1] = 1e300
    corr[[1004, 95], 2] = np.nan                           # a NaN score: a single row, and a row of the seam's group
    cdp = B.centroid_dp(cen)
    qq, qc = B.quantize_queries(rng.standard_normal((sum(TOKENS), dim)).astype(np.float32), cen, sim, qb)
    s32 = [O.score_all(codes, corr, dim, qq[i], qc[i], qb, sim, cdp)[2] for i in range(len(qq))] if qb == 4 else None
    for a in (codes, corr):
        a.setflags(write=False)
    return codes, corr, cdp, qq, qc, s32


@functools.lru_cache(maxsize=None)
def _want(dim, sim, mname, k):
    rep, live = M.rep_scores(_case(dim, sim)[5], OFFSETS, _masks()[mname])
    out = []
    for a, b in SPANS:
        S = M.reduce(rep[a:b])
        oi, osc = O.heap_topk(S, k)
        out.append((live[oi].astype(np.int32), osc, M.SC.expected_status(S, k)))
    return out, len(live)


def _answers(ix, groups, qq, qc, qb, sim, k):
    """the call under maxsim_fused 1 and 2: [(answers, statuses)]"""
    seen = []
    for fused in (1, 2):
        ix.set_option("maxsim_fused", fused)
        seen.append(ix.search_maxsim_batch([(qq[a:b], qc[a:b]) for a, b in SPANS], qb, sim, k, groups))
    ix.set_option("maxsim_fused", -1)
    (r1, s1), (r2, s2) = seen
    assert s1.tobytes() == s2.tobytes() and all(u.tobytes() == v.tobytes() for x, y in zip(r1, r2) for u, v in zip(x, y)), "1 and 2 differ"
    return seen


def _groups(ix, mask):
    if mask.all():
        return capi.Groups(ix, OFFSETS)
    with capi.Filter(ix, mask) as flt:
        return capi.Groups(ix, OFFSETS, flt)


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("sim", [0, 1, 2])
@pytest.mark.parametrize("dim", [768, 700, 1000, 1500])
def test_against_the_model(dim, sim, compact):
    codes, corr, cdp, qq, qc, _ = _case(dim, sim)
    ix = B.Index(codes, corr, dim, cdp, corrections="compact" if compact else "inline")
    try:
        for mname, mask in _masks().items():
            with _groups(ix, mask) as groups:
                for k in (7, N):
                    want, L = _want(dim, sim, mname, k)
                    assert groups.live == L
                    for fused, (res, status) in zip((1, 2), _answers(ix, groups, qq, qc, 4, sim, k)):
                        for q, (wg, ws, wst) in enumerate(want):
                            where = "%s k=%d fused=%d query %d" % (mname, k, fused, q)
                            np.testing.assert_array_equal(res[q][0], wg, err_msg=where + ": groups")
                            np.testing.assert_array_equal(canon32(res[q][1]), canon32(ws), err_msg=where + ": score bits")
                            assert status[q] == wst, where + ": status"
    finally:
        ix.close()


@pytest.mark.parametrize("dim,qb", [(64, 4), (768, 8)])
def test_off_shape_answers_as_fused_1(dim, qb):
    """no matrix-core kernel for a 64-d index or a call with query values above 15: 2 does what 1 does"""
    codes, corr, cdp, qq, qc, _ = _case(dim, 1, qb)
    assert qb == 4 or qq.max() > 15
    ix = B.Index(codes, corr, dim, cdp)
    try:
        with capi.Groups(ix, OFFSETS) as groups:
            (res, _), _ = _answers(ix, groups, qq, qc, qb, 1, 7)
            assert all(len(r[0]) == 7 for r in res)
    finally:
        ix.close()


def test_refusals():
    codes, corr, cdp, _, _, _ = _case(64, 1)
    ix = B.Index(codes, corr, 64, cdp)
    try:
        for bad in (3, -2):
            with pytest.raises(capi.BBQError) as e:
                ix.set_option("maxsim_fused", bad)
            assert e.value.code == capi.ERR_INVALID_ARG
    finally:
        ix.close()
