"""GPU: the shared end of the span, filtered span, grouped and MaxSim searches (finish_selected, bbq_select.cpp) - every branch of it
through each of its four callers, every answer held to the oracle's heap by the callers' own helpers: indices, score bits, out_n and the
status of tests/test_spans_cpu.py's rule.  The branches: a query without rows; a query the device selected for and proved; one it
selected for and could not prove (equal scores); one it did not select for (no more rows than k); the scores of the replayed queries
brought back query by query (they are less than half of the call's) or in one copy; the heaps on one thread or on several (at least
4 096 replayed rows and option replay_threads > 1).  Each test asserts how many statuses the oracle expects to be 1, so it cannot pass
while a branch goes unvisited.  4 000 rows of 64 dimensions - the narrowest compiled width - and 8 queries a call."""
import functools

import numpy as np
import pytest

import orclib as O
import maxsim_model as M
import test_spans_cpu as SC
import test_spans_filtered_cpu as FC
import test_gpu_spans as GS               # assert_spans
import test_gpu_spans_filtered as GF      # assert_filtered
import test_gpu_grouped as GG             # assert_grouped
import test_gpu_maxsim as GM              # assert_maxsim
from bbqlib import bbq_amd as B, capi

pytestmark = pytest.mark.gpu

N, DIM, NQ, SEED = 4000, 64, 8, 319
SIM, QB = 1, 4
K_SPAN = 3000                             # below the select pass's limit of 4 096
SHORT, LONG = 3000, 3500                  # rows of a query the device does not select for (L <= k), and of one it does
K_GROUP = 10
THREADS = (1, 4)
SINGLETONS = np.arange(N + 1, dtype=np.int64)
EVERYTHING = np.ones(N, bool)
DUP_AT = N - 16                           # where the copies of best rows go: rows [DUP_AT, N)


@functools.lru_cache(maxsize=None)
def _mask():
    """accepts about 90 % of the rows; read-only"""
    m = np.random.default_rng(SEED + 1).random(N) < 0.9
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _base():
    """the seeded index, NQ query vectors for the span and grouped searches and 2 NQ token vectors - two per MaxSim query - with every
    vector's per-row oracle scores; computed once, read-only.  Of 3 500 scores of 64-dimensional rows the 3 001 largest are pairwise
    different for about every second query only, so query q is the first vector of a seeded pool that the device can prove an answer
    for wherever a case below makes it a long query, with and without the filter; the token vectors 8 .. 15 are the next of the pool"""
    rng = np.random.default_rng(SEED)
    base = rng.standard_normal((N, DIM)).astype(np.float32)
    pool = rng.standard_normal((128, DIM)).astype(np.float32)
    codes, corr, cen = B.quantize_vectors(base, SIM)
    cdp = B.centroid_dp(cen)
    pq, pc = B.quantize_queries(pool, cen, SIM, QB)
    visits = [[] for _ in range(NQ)]                         # per query: the row sets it must be provable over
    for case, short in SPAN_CASES.items():
        for mask in (None, _mask()):
            lists, _ = _span_lists(case, mask)
            for q in range(NQ):
                if q != 3 and q not in short:
                    visits[q].append(SC.expand(lists[q]) if mask is None else FC.accepted(mask, lists[q]))
    chosen, s32, nxt = [], [], 0
    while len(chosen) < 2 * NQ:
        sc = O.score_all(codes, corr, DIM, pq[nxt], pc[nxt], QB, SIM, cdp)[2]
        if len(chosen) >= NQ or all(SC.expected_status(sc[rows], K_SPAN) == 0 for rows in visits[len(chosen)]):
            chosen.append(nxt)
            s32.append(sc)
        nxt += 1
    qq, qc = np.ascontiguousarray(pq[chosen]), np.ascontiguousarray(pc[chosen])
    for a in (codes, corr):
        a.setflags(write=False)
    return codes, corr, cdp, qq, qc, s32


def _scores(codes, corr):
    _, _, cdp, qq, qc, _ = _base()
    return [O.score_all(codes, corr, DIM, qq[i], qc[i], QB, SIM, cdp)[2] for i in range(2 * NQ)]


TOKENS = [(2 * i, 2 * i + 2) for i in range(NQ)]          # MaxSim query i: token vectors 2 i and 2 i + 1


@functools.lru_cache(maxsize=None)
def _tied(n_tied):
    """the index with, for each of the first n_tied queries, its best row copied to a row of its own at the end - once the grouped
    search's best row (the best score of vector q) and once the MaxSim search's (the best sum of query q's two tokens): with groups of
    one row the two best representatives, or sums, of such a query are equal, and the device cannot prove its answer"""
    codes, corr, _, _, _, s32 = _base()
    codes, corr = codes.copy(), corr.copy()
    at = DUP_AT
    for q in range(n_tied):
        S = M.reduce(np.stack([s32[t] for t in range(*TOKENS[q])]))
        for best in (int(np.argmax(s32[q][:DUP_AT])), int(np.argmax(S[:DUP_AT]))):
            codes[at], corr[at] = codes[best], corr[best]
            at += 1
    assert at <= N
    for a in (codes, corr):
        a.setflags(write=False)
    return codes, corr, _scores(codes, corr)


SPAN_CASES = {"two_replayed_query_by_query": (1, 6), "five_replayed_in_one_copy": (0, 1, 4, 5, 7)}


def _span_lists(case, mask=None):
    """(8 span lists, the short queries): query 3 has no span; a short query holds exactly SHORT rows - accepted rows under a mask -
    and the others LONG rows, in two pieces q rows apart (query 0: adjacent) so that a replay walks more than one span"""
    short = SPAN_CASES[case]
    acc = np.concatenate([[0], np.cumsum(EVERYTHING if mask is None else mask)])       # accepted rows in front of row r
    lists = []
    for q in range(NQ):
        if q == 3:
            lists.append(SC.spans_of([]))
            continue
        b = 7 + 41 * q
        mid = b + 1000 + 64 * q
        again = mid + q
        if q in short:                                                                 # the first e that completes SHORT rows
            e = int(np.searchsorted(acc, acc[again] + SHORT - (acc[mid] - acc[b])))
        else:
            e = again + LONG - (mid - b)
        lists.append(SC.spans_of([(b, mid), (again, e)]))
        assert SC.spans_are_valid(lists[-1], N)
    return lists, short


@pytest.mark.parametrize("case", SPAN_CASES)
def test_span_search(case):
    codes, corr, cdp, qq, qc, s32 = _base()
    lists, short = _span_lists(case)
    visited = [s32[q][SC.expand(lists[q])] for q in range(NQ)]
    assert [len(v) for v in visited] == [0 if q == 3 else SHORT if q in short else LONG for q in range(NQ)]
    want = [SC.expected_status(v, K_SPAN) for v in visited]
    assert want == [1 if q in short else 0 for q in range(NQ)]                          # only the short ones are replayed
    replayed, total = SHORT * len(short), sum(len(v) for v in visited)
    assert replayed >= 4096 and (2 * replayed >= total) == (case == "five_replayed_in_one_copy")
    ix = B.Index(codes, corr, DIM, cdp)
    try:
        for threads in THREADS:
            ix.set_option("replay_threads", threads)
            status = GS.assert_spans(ix, qq[:NQ], qc[:NQ], QB, SIM, K_SPAN, lists, s32[:NQ], "%s, %d threads" % (case, threads))
            assert status.tolist() == want
    finally:
        ix.close()


@pytest.mark.parametrize("case", SPAN_CASES)
def test_filtered_span_search(case):
    codes, corr, cdp, qq, qc, s32 = _base()
    mask = _mask()
    assert 0.88 * N < mask.sum() < 0.92 * N
    lists, short = _span_lists(case, mask)
    visited = [s32[q][FC.accepted(mask, lists[q])] for q in range(NQ)]
    assert all(len(visited[q]) == SHORT for q in short) and all(len(visited[q]) > K_SPAN for q in range(NQ) if q != 3 and q not in short)
    want = [SC.expected_status(v, K_SPAN) for v in visited]
    assert want == [1 if q in short else 0 for q in range(NQ)]
    replayed, total = SHORT * len(short), sum(len(v) for v in visited)
    assert replayed >= 4096 and (2 * replayed >= total) == (case == "five_replayed_in_one_copy")
    ix = B.Index(codes, corr, DIM, cdp)
    try:
        with capi.Filter(ix, mask) as flt:
            for threads in THREADS:
                ix.set_option("replay_threads", threads)
                _, status = GF.assert_filtered(ix, flt, mask, qq[:NQ], qc[:NQ], QB, SIM, K_SPAN, lists, s32[:NQ], "%s, %d threads" % (case, threads))
                assert status.tolist() == want
    finally:
        ix.close()


def _maxsim_want(s32):
    rep, live = M.rep_scores(s32, SINGLETONS, EVERYTHING)
    return rep, live, [SC.expected_status(M.reduce(rep[a:b]), K_GROUP) for a, b in TOKENS]


@pytest.mark.parametrize("n_tied", [2, 6])
def test_grouped_and_maxsim_search(n_tied):
    """groups of one row, L = 4 000, k = 10: the first n_tied queries' two best are equal - replayed, 4 000 rows each, query by query
    where they are two of eight and in one copy where they are six - and the others' are proven"""
    _, _, cdp, qq, qc, _ = _base()
    codes, corr, s32 = _tied(n_tied)
    want = [SC.expected_status(s32[q], K_GROUP) for q in range(NQ)]
    assert want == [1] * n_tied + [0] * (NQ - n_tied)
    rep, live, want_maxsim = _maxsim_want(s32)
    assert want_maxsim == want
    assert n_tied * N >= 4096 and (2 * n_tied >= NQ) == (n_tied == 6)
    ix = B.Index(codes, corr, DIM, cdp)
    try:
        with capi.Groups(ix, SINGLETONS) as groups:
            assert groups.live == N
            for threads in THREADS:
                ix.set_option("replay_threads", threads)
                _, status = GG.assert_grouped(ix, groups, SINGLETONS, EVERYTHING, qq[:NQ], qc[:NQ], QB, SIM, K_GROUP, s32[:NQ], "%d tied, %d threads" % (n_tied, threads))
                assert status.tolist() == want
                _, status = GM.assert_maxsim(ix, groups, rep, live, qq, qc, TOKENS, QB, SIM, K_GROUP, "%d tied, %d threads" % (n_tied, threads))
                assert status.tolist() == want
    finally:
        ix.close()


def test_interleaved_on_one_index():
    """the four callers take turns on one index: they share one scratch, which only grows, and one stream"""
    _, _, cdp, qq, qc, _ = _base()
    codes, corr, s32 = _tied(2)
    mask = _mask()
    rep, live, _ = _maxsim_want(s32)
    plain, _ = _span_lists("two_replayed_query_by_query")
    filtered, _ = _span_lists("five_replayed_in_one_copy", mask)
    ix = B.Index(codes, corr, DIM, cdp)
    try:
        ix.set_option("replay_threads", 4)
        with capi.Filter(ix, mask) as flt, capi.Groups(ix, SINGLETONS) as groups:
            for turn in range(2):
                GG.assert_grouped(ix, groups, SINGLETONS, EVERYTHING, qq[:NQ], qc[:NQ], QB, SIM, K_GROUP, s32[:NQ], "turn %d" % turn)
                GS.assert_spans(ix, qq[:NQ], qc[:NQ], QB, SIM, K_SPAN, plain, s32[:NQ], "turn %d" % turn)
                GM.assert_maxsim(ix, groups, rep, live, qq, qc, TOKENS, QB, SIM, K_GROUP, "turn %d" % turn)
                GF.assert_filtered(ix, flt, mask, qq[:NQ], qc[:NQ], QB, SIM, K_SPAN, filtered, s32[:NQ], "turn %d" % turn)
                GS.assert_spans(ix, qq[:NQ], qc[:NQ], QB, SIM, 5, plain, s32[:NQ], "turn %d, k = 5" % turn)
    finally:
        ix.close()
