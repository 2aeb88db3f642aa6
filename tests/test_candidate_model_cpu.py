"""CPU: the candidate-count model of tests/candidate_model.py - what tests/test_gpu_candidate_count.py holds bbq_stats.candidates to -
against brute force, its recipe against the conditions that make the count a witness, and the host rules it restates against their
source lines.

What "finite threshold" is asked of.  The hostile kind plants one row with additionalCorrection +inf and one with 1e300, and both score
+inf under COSINE and MAXIMUM_INNER_PRODUCT: with k = 1 (k_dev = 2) two such rows end every threshold at the key of +inf, whatever the
seed.  So the condition "four of six queries end with a finite threshold above the key of +0" is asserted for every (family, kind,
similarity) at k = 10 and 100, and at k = 1 wherever fewer than k_dev = 2 rows score +inf - the ordinary kind, and the hostile kind
under EUCLIDEAN; the hostile k = 1 cells under the other two similarities are where a threshold that has reached +inf must list nothing."""
import os

import numpy as np
import pytest

import call_walk as W
import candidate_model as M
import orclib as O

CSRC = os.path.join(O.ROOT, "better-binary-quantization_amd", "csrc")
SHORT = [f for f in M.FAMILIES if f.name != "long"]
CELLS = [(f, kind) for f in SHORT for kind in M.ROW_KINDS]
CELL_IDS = ["%s-%s" % (f.name, kind) for f, kind in CELLS]


def _source(name):
    with open(os.path.join(CSRC, name), encoding="utf-8") as f:
        return f.read()


def _finite(theta):
    return M.KEY_PLUS_ZERO < theta < M.KEY_PLUS_INF


@pytest.mark.parametrize("fam,kind", CELLS, ids=CELL_IDS)
def test_the_recipe_meets_its_conditions(fam, kind):
    for sim in M.SIMS:
        sc = M.scores(fam, kind, sim)
        assert len(sc) == 6 and not any(np.isnan(s).any() for s in sc), "a NaN score"
        infs = max(sorted(int((s == np.inf).sum()) for s in sc)[:4])       # of the four queries with the fewest
        for k in M.KS:
            counts = M.search_count(fam, [sc[i % 6] for i in range(8)], k, M.plan_of(fam))[:6]
            for a in (0, 2, 4):       # append mode: the same lists, and no refusal
                assert M.search_count(fam, sc[a:a + 2], k, M.plan_of(fam)) == counts[a:a + 2]
            assert all(c.path == "segments" and not c.flagged for c in counts)
            assert all(len(c.split) >= 3 for c in counts), "fewer than two thresholds"
            assert all(c.split[0] == 1024 for c in counts)
            assert all(list(c.thetas) == sorted(c.thetas) for c in counts)
            if infs < M.k_dev_of(k, fam.n):
                assert sum(_finite(c.thetas[-1]) for c in counts) >= 4, (sim, k, [c.thetas[-1] for c in counts])
                for seg in range(1, len(counts[0].split)):
                    assert any(c.split[seg] > 0 for c in counts), "sparse segment %d lists nothing for any query (sim %d, k %d)" % (seg, sim, k)
            else:
                assert kind == "hostile" and k == 1 and sim != 0
    if kind == "hostile":       # the plants lie behind the dense first segment, in three sparse segments of the plan (two where it has two)
        segs = M.segments_of(fam.n, 11, 1024, 2)
        where = {name: next(i for i, (b, rows, _) in enumerate(segs) if b <= t * M.TILE < b + rows) for name, t in M.plant_tiles(fam).items()}
        assert min(where.values()) >= 1 and len(set(where.values())) == min(3, len(segs) - 1), where
        codes, corr = M.rows(fam, kind)
        with np.errstate(over="ignore"):
            f32 = corr.astype(np.float32)
        assert np.isinf(f32[:, :2]).any() and np.isfinite(corr[:, :2]).all()          # intervals that are non-finite as the tile holds them
        assert (corr[:, 2] == np.inf).sum() == 1 and (corr[:, 2] == -np.inf).sum() == 1 and (corr[:, 2] == 1e300).sum() == 1
        assert np.isinf(M.scores(fam, kind, 0)[0][M.EUC_INF_ROW])                     # the EUCLIDEAN +inf row


def _brute(keys, segs, k_dev, acc):
    """per segment: the threshold recomputed from scratch by sorting every accepted key in front of it"""
    out = []
    for b, rows, dense in segs:
        before = sorted((int(x) for x in keys[:b][acc[:b]]), reverse=True)
        theta = before[k_dev - 1] if len(before) >= k_dev else 0
        here = keys[b:b + rows][acc[b:b + rows]]
        out.append(len(here) if dense else sum(1 for x in here if int(x) > theta))
    return out


@pytest.mark.parametrize("kind", M.ROW_KINDS)
def test_against_brute_force_on_a_slice(kind):
    fam, n = M.BY_NAME["w6"], 3000
    rng = np.random.default_rng(5)
    masks = {"none": None, "half": rng.random(n) < 0.5, "tiles": np.r_[np.zeros(64, bool), np.ones(n - 64 - 56, bool), np.zeros(56, bool)]}
    for sim in M.SIMS:
        for q, s in enumerate(M.scores(fam, kind, sim)):
            s, keys = s[:n], M.keys_of(s[:n])
            for k in M.KS:
                for select in (1, 0):
                    for name, mask in masks.items():
                        opts = dict(M.PLAN, device_select=select)
                        got = M.search_count(fam, [s] * 8, k, opts, mask)[q % 8]
                        n_eff = n if mask is None else int(mask.sum())
                        kd = min(k, n_eff) + select
                        segs = M.segments_of(n, kd, 1024, 2) if mask is None else M.filtered_segments_of(mask, kd, 1024, 2)
                        want = _brute(keys, segs, kd, np.ones(n, bool) if mask is None else mask)
                        assert list(got.split) == want and got.count == sum(want), (sim, q, k, select, name)
                        # every row of the oracle's answer is listed
                        acc = np.arange(n) if mask is None else np.flatnonzero(mask)
                        top = acc[O.heap_topk(s[acc], k)[0]]
                        seg_of = np.searchsorted([b for b, _, _ in segs], top, side="right") - 1
                        theta_before = np.array([0] + list(got.thetas))[seg_of]
                        assert ((keys[top] > theta_before) | (seg_of == 0)).all(), "a row of the answer is not listed"


def test_one_score_moves_the_count_by_one():
    fam = M.BY_NAME["w6"]
    s = np.array(M.scores(fam, "ordinary", 1)[0])
    base = M.search_count(fam, [s] * 8, 10, M.PLAN)[0]
    segs = M.segments_of(fam.n, 11, 1024, 2)
    keys = M.keys_of(s)
    moved = 0
    for i in range(1, len(segs)):
        b, rows, _ = segs[i]
        lo, hi = base.thetas[i - 1], base.thetas[i]
        if hi - lo < 2:
            continue
        seg = np.arange(b, b + rows)
        # listed, and below the segment's own threshold: lowering it to the old threshold changes no later threshold
        listed = seg[(keys[seg] > lo) & (keys[seg] < hi)]
        if len(listed):
            t = s.copy()
            t[listed[0]] = M.scores_of_keys([lo])[0]
            assert M.search_count(fam, [t] * 8, 10, M.PLAN)[0].count == base.count - 1
            moved += 1
        unlisted = seg[keys[seg] <= lo]
        t = s.copy()
        t[unlisted[0]] = M.scores_of_keys([lo + 1])[0]
        assert M.search_count(fam, [t] * 8, 10, M.PLAN)[0].count == base.count + 1
        moved += 1
    assert moved >= 4


def test_refusals_and_flags():
    fam = M.BY_NAME["w1"]
    s = np.array(M.scores(fam, "ordinary", 1)[0])
    t = s.copy()
    t[5000] = np.nan
    c = M.search_count(fam, [t, s], 10, M.PLAN)
    assert c[0].flagged and c[0].count == fam.n and not c[1].flagged
    mask = np.arange(fam.n) % 2 == 0
    assert M.search_count(fam, [t, s], 10, M.PLAN, mask)[0].count == mask.sum() and not M.search_count(fam, [t], 10, M.PLAN, ~mask)[0].flagged
    rising = np.arange(40000, dtype=np.float32)          # every row above every threshold: a second segment of 14000 new keys
    with pytest.raises(M.Refused):
        M.segmented(rising, [(0, 8192, True), (8192, 14000, False), (22192, 40000 - 22192, False)], 11)
    assert M.segmented(rising, [(0, 8192, True), (8192, 40000 - 8192, False)], 11).count == 40000      # ... the last segment selects no threshold
    with pytest.raises(M.Refused):
        M.search_count(fam, [s], 5000, M.PLAN)
    for out_of_scope in ({"pilot_rows": 1024}, {"devices": 2}):
        with pytest.raises(M.Refused):
            M.search_count(fam, [s], 10, M.PLAN, **out_of_scope)


def test_keys():
    f = np.array([-np.inf, -1.0, -0.0, 0.0, 1e-45, 1.0, np.inf], np.float32)
    keys = M.keys_of(f)
    assert (np.diff(keys.astype(np.int64)) > 0).all() and keys[3] == M.KEY_PLUS_ZERO and keys[-1] == M.KEY_PLUS_INF
    assert M.scores_of_keys(keys).view(np.uint32).tolist() == f.view(np.uint32).tolist()
    assert M.kth_largest(keys, 2) == keys[-2] and M.kth_largest(keys, 8) == 0


# ------------------------------------------------------------------------------------------------ `long`
@pytest.mark.parametrize("sim", M.LONG_SIMS)
def test_long_takes_both_paths(sim):
    fam = M.LONG
    assert W.presample_plan(fam.n, 10)[1] == 1 and W.presample_plan(fam.n, 100)[1] == 4 and W.presample_plan(fam.n, 500)[1] == 4
    paths = {}
    for kind in M.ROW_KINDS:
        sc = M.scores(fam, kind, sim)
        assert not any(np.isnan(s).any() for s in sc)
        for k in (1, 10, 100, 500):
            for q, s in enumerate(sc):
                c = M.search_count(fam, [s], k, {})[0]
                pre = M.presampled(s, k)
                chain = M.segmented(s, M.segments_of(fam.n, k + 1, 4096, 64), k + 1)
                assert c.count == (pre[0] if pre[1] else chain.count) and c.path == ("presampled" if pre[1] else "segments")
                assert abs(pre[0] - chain.count) > 1000, "the two paths' counts are too close to tell them apart"
                # with latency_presample 0 the chain answers
                assert M.search_count(fam, [s], k, {"latency_presample": 0})[0].count == chain.count
                paths.setdefault((kind, k), []).append(c.path)
    for k in (1, 10):       # the two ordinary queries and the two with the interval x 30 are answered from the pre-sampled list
        assert paths["ordinary", k][:4] == ["presampled"] * 4
    assert any("segments" in p for p in paths.values())
    for k in (1, 4):        # k + 2 copies of the best row inside the first 4000 rows
        _, _, s = M.long_tied(sim, k)
        pre = M.presampled(s, k)
        assert pre[0] == 0 and not pre[1]
        c = M.search_count(fam, [s], k, {})[0]
        assert c.path == "segments" and c.count == 4096 and c.split == (4096, 0)


# ------------------------------------------------------------------------------------------------ the rules, in their sources
def test_the_rules_are_the_sources():
    core, kernels, device, latency = _source("bbq_core.cpp"), _source("bbq_kernels.hip"), _source("bbq_device.h"), _source("bbq_latency.cpp")
    assert "c.k_dev = final_k > 0 ? keff + 1 : keff;" in core
    assert "const int64_t final_k = (keff <= kFinalSelectMax && ix->opt_device_select) ? keff : 0;" in core
    assert "const bool latency = final_k > 0 && n_queries <= ix->opt_latency_queries;" in core
    assert "p.growth = latency ? ix->opt_latency_growth : ix->opt_growth;" in core
    assert "p.s0 = std::min<int64_t>(p.s0, %d);" % M.DENSE_SEGMENT_MAX in core
    assert "constexpr int kFinalizeKeyCap = %d;" % M.K_FINALIZE_KEY_CAP in device
    assert M.DENSE_SEGMENT_MAX < M.K_FINALIZE_KEY_CAP == W.K_LAT_PRE_KEYS
    # the threshold: the k-th largest of the new keys and the running top keys, 0 while fewer were seen; over the keys that fit
    assert "const uint32_t m_use = min(m_new, (uint32_t)kFinalizeKeyCap - tcount);" in kernels
    assert "if (M < (uint32_t)a.k) {" in kernels
    assert "const uint32_t th = block_select_kth_largest(s_keys, M, (uint32_t)a.k, s_hist, s_wave, s_misc + 8);" in kernels
    assert "return valid && (s32 == s32) && key_of_bits(__float_as_uint(s32)) > theta;" in _source("bbq_kernel_common.h")
    assert "return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }" in _source("bbq_entry.h")
    # the pre-sampled chain: the rank, what its list must hold to answer, and what sends the call on
    assert "HIPCHK(launch_lat_select(ctx->d_pre_keys, (int)n_keys, (int)(k2 + 2), s.d_theta, a.p, st));" in latency
    assert "m_new <= (uint32_t)kFinalizeKeyCap - tcount && a.k == k2 + 1;" in kernels
    assert "ok = shard ? (n_sel <= (uint32_t)k2) : take_all ? (n_sel == (uint32_t)total) : (n_sel == (uint32_t)k2);" in kernels
    assert "if (!shard && (same > 1u || (!take_all && fx == fth))) s_misc[3] = 1;" in kernels
    assert "if (r.flags != 0 || r.needs_replay != 0 || r.count != (uint32_t)k2) return BBQ_OK;" in latency
    assert "if (lane == __ffsll((long long)holders) - 1) key = 0;" in _source("bbq_latency_kernels.hip")       # ONE holder retires: duplicates stay
    # the three places that add to the count, the dense path's, and the reset per call
    assert "ix->stats.candidates += h.listed;" in latency
    assert "if (s.h_list_counts[2 * i + 1] == 0) ix->stats.candidates += s.h_list_counts[2 * i];" in core
    assert "ix->stats.candidates += s.h_list_counts[0];" in core
    assert core.count("stats.candidates +=") == 2 and latency.count("stats.candidates +=") == 1
    assert "ix->stats.candidates += c.filter ? c.n_eff : n;" in _source("bbq_dense.cpp")
    assert "static void reset_call_stats(bbq_index *ix) { ix->stats.candidates = ix->stats.dense_fallbacks = ix->stats.host_replays = 0; }" in core
    assert core.count("reset_call_stats(ix);") == 2
    # the plan of call_walk.plan_segments is the unfiltered plan with k_dev = k + 1
    assert M.segments_of(20517, 11, 1024, 2) == W.plan_segments(20517, 10, 1024, 2)
