"""GPU: filtered search (bbq_filter_*, bbq_search_filtered_batch) against the oracle.  The contract: the answer is what the
reference's searchNearestNeighbors loop returns when it visits only the accepted ords, ascending, each with its original ord and f32
score, heap size min(k, |A|) - so the expected value is the oracle's heap over scores[flatnonzero(mask)], mapped back to ords.
Bit-exact: indices, f32 score bits and order, ties included; no tolerances, nothing skipped for ties."""
import numpy as np
import pytest

import orclib as O
from bbqlib import bbq_amd as B, capi

pytestmark = pytest.mark.gpu


def canon32(a):
    a = np.array(a, np.float32)
    a[np.isnan(a)] = np.nan
    return a.view(np.uint32)


def _reference_accepts(name):
    return not any("per_row_error" in rec for rec in O.load_golden(name)["queries"])


_WANTED = ("ties_", "m_768d_", "m_100d_", "big_20000x128_cos", "big_50000x768_cos", "big_30000x1536_mip", "big_20000x1024_euc_qb8",
           "ib2_", "ib4_", "ib8_", "edge_n1", "edge_dim1")
CASES = [n for n in O.golden_names() if n.startswith(_WANTED) and _reference_accepts(n)]


def expected(s32, mask, k):
    """the oracle recipe: the heap over the accepted rows' scores in ascending ord, positions mapped back to ords"""
    acc = np.flatnonzero(mask)
    pos, sc = O.heap_topk(s32[acc], k)
    return acc[pos].astype(np.int32), sc


def assert_same(got, want, msg):
    np.testing.assert_array_equal(got[0], want[0], err_msg=msg)
    np.testing.assert_array_equal(canon32(got[1]), canon32(want[1]), err_msg=msg)


def masks_for(n, top10, seed):
    """the masks of the issue, by name; k0 = 10 stands for "k" in the masks that are sized by it"""
    rng = np.random.default_rng(seed)
    k0 = min(10, n)
    m = {"ones": np.ones(n, bool), "zeros": np.zeros(n, bool)}
    m["one_row"] = np.zeros(n, bool)
    m["one_row"][n // 2] = True
    m["random_50"] = rng.random(n) < 0.5
    m["random_1"] = rng.random(n) < 0.01
    m["first_half"] = np.arange(n) < n // 2
    m["last_10pct"] = np.arange(n) >= n - max(n // 10, 1)
    m["every_64th"] = np.arange(n) % 64 == 0
    for name, cnt in (("exactly_k", k0), ("k_minus_1", k0 - 1)):
        m[name] = np.zeros(n, bool)
        m[name][rng.choice(n, cnt, replace=False)] = True
    m["not_top10"] = np.ones(n, bool)
    m["not_top10"][top10] = False
    return m


def _case_index(g, compact):
    sim = O.SIMS[g["sim"]]
    base, queries = O.golden_inputs(g)
    codes, corr, cen = B.quantize_vectors(base, sim, g["ib"], g["lambda"], g["iters"])
    cdp = B.centroid_dp(cen)
    ix = B.Index(codes, corr, g["dim"], cdp, corrections="compact" if compact else "inline", index_bits=g["ib"])
    return sim, queries, codes, corr, cen, cdp, ix


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_golden_filtered(name, compact):
    g = O.load_golden(name)
    sim, queries, codes, corr, cen, cdp, ix = _case_index(g, compact)
    n, qb = g["n"], g["qb"]
    try:
        prepared = []
        for qi, rec in enumerate(g["queries"]):
            qq, qc = B.quantize_query(queries[qi], cen, sim, qb, g["lambda"], g["iters"])
            _, _, s32 = O.score_all(codes, corr, g["dim"], qq, qc, qb, sim, cdp, ib=g["ib"])
            prepared.append((qq, qc, s32, rec))
        top10 = O.heap_topk(prepared[0][2], 10)[0]
        for mname, mask in masks_for(n, top10, 11).items():
            with capi.Filter(ix, mask) as flt:
                a = int(mask.sum())
                assert flt.count == a
                for qi, (qq, qc, s32, rec) in enumerate(prepared):
                    for k in sorted({1, 10, 100, a, a + 5}):
                        got = ix.search_filtered(qq, qc, qb, sim, k, flt)
                        assert len(got[0]) == min(k, a)
                        assert_same(got, expected(s32, mask, k), "%s %s q%d k=%d" % (name, mname, qi, k))
                    if mname == "ones":  # ... which must also be the reference's recorded answers
                        for tk in rec["topk"]:
                            idx, sc = ix.search_filtered(qq, qc, qb, sim, tk["k"], flt)
                            np.testing.assert_array_equal(idx, O.dec(tk["idx_i32"], "<i4"), err_msg="%s q%d k=%d" % (name, qi, tk["k"]))
                            np.testing.assert_array_equal(canon32(sc), canon32(O.dec(tk["score_f32"], "<f4")))
                    if mname == "not_top10" and qi == 0 and n > 10:
                        assert not set(ix.search_filtered(qq, qc, qb, sim, 10, flt)[0]) & set(top10), "the answer did not change"
    finally:
        ix.close()


@pytest.mark.parametrize("name", ["big_20000x128_cos", "big_20000x1024_euc_qb8"])
def test_large_k_takes_the_dense_path(name):
    g = O.load_golden(name)
    sim, queries, codes, corr, cen, cdp, ix = _case_index(g, True)
    try:
        qq, qc = B.quantize_query(queries[0], cen, sim, g["qb"], g["lambda"], g["iters"])
        _, _, s32 = O.score_all(codes, corr, g["dim"], qq, qc, g["qb"], sim, cdp)
        mask = np.random.default_rng(3).random(g["n"]) < 0.5
        with capi.Filter(ix, mask) as flt:
            assert_same(ix.search_filtered(qq, qc, g["qb"], sim, 5000, flt), expected(s32, mask, 5000), name)
            assert ix.stats()["dense_fallbacks"] == 1
    finally:
        ix.close()


def _planted_ties(sim=1, qb=4):
    """rows duplicated so that equal scores sit inside and exactly at the edge of the accepted answer, while the rejected rows are
    copies of the query's best rows: strictly higher scores that must not show"""
    rng = np.random.default_rng(21)
    n, dim, k = 6000, 128, 40
    base = rng.standard_normal((n, dim)).astype(np.float32)
    query = rng.standard_normal(dim).astype(np.float32)
    codes, corr, cen = B.quantize_vectors(base, sim)
    cdp = B.centroid_dp(cen)
    qq, qc = B.quantize_query(query, cen, sim, qb)
    _, _, s32 = O.score_all(codes, corr, dim, qq, qc, qb, sim, cdp)
    order = np.argsort(-s32.astype(np.float64), kind="stable")
    best, rest = order[:40], order[40:]
    mask = np.ones(n, bool)
    mask[best] = False  # rejected: the 40 best rows ...
    spots = rng.choice(rest[200:], 60, replace=False)
    # ... and, accepted, 12 copies of rest[5] (equal scores inside the answer: ranks 5..17 of the accepted rows) and 18 of rest[19]
    # (ranks 31..49: rank k = 40 cuts through them), scattered over the index
    for r in spots[:12]:
        codes[r], corr[r] = codes[rest[5]], corr[rest[5]]
    for r in spots[12:30]:
        codes[r], corr[r] = codes[rest[19]], corr[rest[19]]
    for r in spots[30:]:  # more rejected rows with strictly higher scores, spread over the index
        codes[r], corr[r] = codes[best[0]], corr[best[0]]
        mask[r] = False
    _, _, s32 = O.score_all(codes, corr, dim, qq, qc, qb, sim, cdp)
    return codes, corr, dim, cdp, qq, qc, s32, mask, k


@pytest.mark.parametrize("compact", [True, False])
def test_planted_ties_among_accepted_rows(compact):
    codes, corr, dim, cdp, qq, qc, s32, mask, k = _planted_ties()
    acc_scores = np.sort(s32[mask])[::-1]
    assert acc_scores[k - 1] == acc_scores[k] and acc_scores[5] == acc_scores[6], "the plant did not produce ties in and at the edge"
    assert s32[~mask].min() > acc_scores[0], "a rejected row does not beat every accepted one"
    ix = B.Index(codes, corr, dim, cdp, corrections="compact" if compact else "inline")
    try:
        with capi.Filter(ix, mask) as flt:
            for opts in ({}, {"first_segment_rows": 1024, "segment_growth": 2}, {"device_select": 0}, {"force_dense": 1}):
                for name, v in opts.items():
                    ix.set_option(name, v)
                for kk in (k - 1, k, k + 1, 5, 6, 31, 32, 50, 200):
                    assert_same(ix.search_filtered(qq, qc, 4, 1, kk, flt), expected(s32, mask, kk), "planted ties k=%d %r" % (kk, opts))
    finally:
        ix.close()


def _random_index(n, dim, nq, seed, sim=1, qb=4):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((n, dim)).astype(np.float32)
    queries = rng.standard_normal((nq, dim)).astype(np.float32)
    codes, corr, cen = B.quantize_vectors(base, sim)
    cdp = B.centroid_dp(cen)
    qq, qc = B.quantize_queries(queries, cen, sim, qb)
    s32 = [O.score_all(codes, corr, dim, qq[i], qc[i], qb, sim, cdp)[2] for i in range(nq)]
    return codes, corr, cdp, qq, qc, s32


def test_batch_equals_single_calls_and_options_do_not_change_the_answer():
    n, dim, nq, k, sim, qb = 30000, 256, 70, 100, 1, 4
    codes, corr, cdp, qq, qc, s32 = _random_index(n, dim, nq, 5)
    mask = np.random.default_rng(6).random(n) < 0.3
    ix = B.Index(codes, corr, dim, cdp)
    try:
        with capi.Filter(ix, mask) as flt:
            idx, sc, cnt = ix.search_filtered_batch(qq, qc, qb, sim, k, flt)
            for i in range(nq):
                want = expected(s32[i], mask, k)
                assert_same((idx[i, :cnt[i]], sc[i, :cnt[i]]), want, "batch q%d" % i)
                assert_same(ix.search_filtered(qq[i], qc[i], qb, sim, k, flt), want, "single q%d" % i)
            defaults = {"device_select": 1, "force_dense": 0, "sweep_share": 1, "latency_queries": 4, "pipeline_slots": 3, "flood_rows": 262144}
            for name, v in (("device_select", 0), ("force_dense", 1), ("sweep_share", 32), ("latency_queries", 0), ("pipeline_slots", 1),
                            ("pipeline_slots", 3), ("flood_rows", 0)):
                ix.set_option(name, v)
                for nq_call in (2, nq):  # a call of few queries (the latency plan) and a pipelined one
                    i2, s2, c2 = ix.search_filtered_batch(qq[:nq_call], qc[:nq_call], qb, sim, k, flt)
                    np.testing.assert_array_equal(c2, cnt[:nq_call])
                    np.testing.assert_array_equal(i2, idx[:nq_call], err_msg="%s=%d" % (name, v))
                    np.testing.assert_array_equal(canon32(s2), canon32(sc[:nq_call]))
                ix.set_option(name, defaults[name])
    finally:
        ix.close()


def test_bitset_rows_and_shuffled_rows_make_the_same_filter():
    n, dim, nq, k = 20000, 128, 3, 50
    codes, corr, cdp, qq, qc, s32 = _random_index(n, dim, nq, 8)
    rng = np.random.default_rng(9)
    mask = rng.random(n) < 0.2
    rows = np.flatnonzero(mask).astype(np.int32)
    shuffled = rng.permutation(np.concatenate([rows, rows[::3], rows[:5]])).astype(np.int32)
    ix = B.Index(codes, corr, dim, cdp)
    try:
        answers = []
        for src in (mask, rows, shuffled):
            with capi.Filter(ix, src) as flt:
                assert flt.count == rows.shape[0]
                answers.append(ix.search_filtered_batch(qq, qc, 4, 1, k, flt))
        for i in range(nq):
            assert_same((answers[0][0][i], answers[0][1][i]), expected(s32[i], mask, k), "q%d" % i)
        for other in answers[1:]:
            np.testing.assert_array_equal(other[0], answers[0][0])
            np.testing.assert_array_equal(canon32(other[1]), canon32(answers[0][1]))
    finally:
        ix.close()


def test_argument_errors_on_the_device():
    n, dim = 1000, 64
    codes, corr, cdp, qq, qc, _ = _random_index(n, dim, 1, 12)
    ix = B.Index(codes, corr, dim, cdp)
    other = B.Index(codes[:900], corr[:900], dim, cdp)
    multi = B.Index.create_multi(codes, corr, dim, cdp, [0, 0], pilot_rows=0)
    try:
        L = capi.lib()
        words = capi.pack_mask(np.ones(n, bool))
        h = capi.C.c_void_p()
        assert L.bbq_filter_create(ix._h, words.ctypes.data, words.shape[0] + 1, capi.C.byref(h)) == capi.ERR_INVALID_ARG
        assert b"n_words" in L.bbq_last_error()
        with pytest.raises(B.BBQError) as e:
            capi.Filter(ix, np.array([0, n], np.int32))
        assert e.value.code == capi.ERR_INVALID_ARG
        # bits at and beyond n_rows are ignored
        words[-1] = np.uint64(0xFFFFFFFFFFFFFFFF)
        assert L.bbq_filter_create(ix._h, words.ctypes.data, words.shape[0], capi.C.byref(h)) == 0
        assert L.bbq_filter_count(h) == n
        L.bbq_filter_destroy(h)
        with capi.Filter(ix, np.ones(n, bool)) as flt:
            with pytest.raises(B.BBQError) as e:  # a filter of an index of another size
                other.search_filtered(qq[0], qc[0], 4, 1, 5, flt)
            assert e.value.code == capi.ERR_INVALID_ARG
            with pytest.raises(B.BBQError) as e:
                ix.search_filtered(qq[0], qc[0], 4, 1, -1, flt)
            assert e.value.code == capi.ERR_NEGATIVE_K
            assert len(ix.search_filtered(qq[0], qc[0], 4, 1, 0, flt)[0]) == 0
            with pytest.raises(B.BBQError) as e:  # a multi-device handle (all shards on device 0): out of scope, and it says so
                multi.search_filtered(qq[0], qc[0], 4, 1, 5, flt)
            assert e.value.code == capi.ERR_UNSUPPORTED and "multi-device" in str(e.value)
        with pytest.raises(B.BBQError) as e:
            capi.Filter(multi, np.ones(n, bool))
        assert e.value.code == capi.ERR_UNSUPPORTED and "multi-device" in str(e.value)
        with capi.Filter(ix, np.ones(n, bool)) as flt:  # k == 0 does not excuse a filter that does not belong to the index
            for wrong, code in ((other, capi.ERR_INVALID_ARG), (multi, capi.ERR_UNSUPPORTED)):
                with pytest.raises(B.BBQError) as e:
                    wrong.search_filtered(qq[0], qc[0], 4, 1, 0, flt)
                assert e.value.code == code
    finally:
        ix.close()
        other.close()
        multi.close()


def test_shards_and_pilot_replicas_are_unsupported():
    """a non-root shard and an index with a pilot replica: no filter can be made for them, and none of another index is taken"""
    n, dim = 4096, 64
    codes, corr, cdp, qq, qc, _ = _random_index(n, dim, 1, 13)
    root = B.Index(codes[:2048], corr[:2048], dim, cdp)
    shard = B.Index(codes[2048:], corr[2048:], dim, cdp, row_base=2048)
    piloted = B.Index(codes[2048:], corr[2048:], dim, cdp, row_base=2048, pilot_codes=codes[:1024], pilot_corr=corr[:1024])
    try:
        with capi.Filter(root, np.ones(2048, bool)) as flt:  # same size, same device: only the kind of index is wrong
            for ix in (shard, piloted):
                with pytest.raises(B.BBQError) as e:
                    capi.Filter(ix, np.ones(2048, bool))
                assert e.value.code == capi.ERR_UNSUPPORTED and "shard" in str(e.value)
                with pytest.raises(B.BBQError) as e:
                    capi.Filter(ix, np.arange(10, dtype=np.int32))
                assert e.value.code == capi.ERR_UNSUPPORTED
                with pytest.raises(B.BBQError) as e:
                    ix.search_filtered(qq[0], qc[0], 4, 1, 5, flt)
                assert e.value.code == capi.ERR_UNSUPPORTED and "shard" in str(e.value)
    finally:
        root.close()
        shard.close()
        piloted.close()


def test_at_size_2m_rows():
    """2 M x 768 synthetic rows, k = 100, 8 queries: every mask against the oracle; the accepted-space plan keeps the random and the
    clustered masks on the sparse path"""
    import bench
    n, dim, k, nq, sim, qb = 2_000_000, 768, 100, 8, 1, 4
    codes, corr = bench.synth_rows(1, 0, n, dim // 8)
    cen = bench.synth_centroid(dim)
    cdp = float(B.centroid_dp(cen))
    qq, qc = bench.synth_queries(3, nq, dim, qb)
    s32 = [O.score_all(codes, corr, dim, qq[i], qc[i], qb, sim, cdp)[2] for i in range(nq)]
    rng = np.random.default_rng(17)
    masks = {"random_50": rng.random(n) < 0.5, "random_1": rng.random(n) < 0.01, "last_10pct": np.arange(n) >= n - n // 10}
    masks["rows_1000"] = np.zeros(n, bool)
    masks["rows_1000"][rng.choice(n, 1000, replace=False)] = True
    ix = B.Index(codes, corr, dim, cdp)
    try:
        for mname, mask in masks.items():
            with capi.Filter(ix, mask) as flt:
                idx, sc, cnt = ix.search_filtered_batch(qq, qc, qb, sim, k, flt)
                st = ix.stats()
                print("at size: %s |A|=%d dense_fallbacks=%d host_replays=%d candidates=%d" % (mname, flt.count, st["dense_fallbacks"], st["host_replays"], st["candidates"]))
                for i in range(nq):
                    assert_same((idx[i, :cnt[i]], sc[i, :cnt[i]]), expected(s32[i], mask, k), "%s q%d" % (mname, i))
                if mname != "rows_1000":
                    assert st["dense_fallbacks"] == 0, "%s fell to the dense path" % mname
    finally:
        ix.close()
