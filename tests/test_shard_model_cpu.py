"""CPU: tests/shard_model.py held to brute force, its recipe to the conditions it is meant to reach, and the host rules it restates to
their source lines.  The device is held to the model in tests/test_gpu_shard_model.py."""
import collections
import os

import numpy as np
import pytest

import call_walk as W
import candidate_model as M
import orclib as O
import shard_model as S
from bbqlib import capi as B

CSRC = os.path.join(O.ROOT, "better-binary-quantization_amd", "csrc")
GRID, TINY = S.grid_cases(), S.tiny_cases()
REACHED = collections.Counter()      # filled by the parametrised tests below, read by the last test of the file


def _source(name):
    with open(os.path.join(CSRC, name), encoding="utf-8") as f:
        return f.read()


def model_of(data, shard, q, k, answers=True, opts=S.OPTS, fam=None, subset=False):
    ps, ow = S.shard_scores(data, shard, q)
    kd = k + 1 if answers else k
    segs = S.shard_segments(len(ps), len(ow), kd, opts["first_segment_rows"], opts["segment_growth"])
    return S.scan_model(ps, ow, shard.r0, k, answers, opts, S.planned_list_cap(segs, kd), fam, subset)


def plans_agree(shard, k, opts=S.OPTS):
    """do the ranks k and k + 1 plan the same segments on this shard?"""
    a, b = ([g[:5] for g in S.shard_segments(len(shard.pilot), shard.r1 - shard.r0, kd, opts["first_segment_rows"], opts["segment_growth"])] for kd in (k, k + 1))
    return a == b


def brute_list(data, shard, q, k_dev, opts=S.OPTS):
    """the list by its definition, row sets and sorts only: per segment of the plan, the rows seen BEFORE it give the threshold"""
    s = data.scores[q]
    keys = M.keys_of(s)
    segs = S.shard_segments(len(shard.pilot), shard.r1 - shard.r0, k_dev, opts["first_segment_rows"], opts["segment_growth"])
    seen, out = [], []
    for g in segs:
        ids = (shard.pilot if g.storage == 0 else np.arange(shard.r0, shard.r1))[g.first:g.first + g.rows]
        before = np.sort(keys[np.array(seen, np.int64)])[::-1] if seen else np.zeros(0, np.uint32)
        theta = int(before[k_dev - 1]) if len(before) >= k_dev else 0
        if g.emit:
            out += [int(r) for r in ids if g.dense or keys[r] > theta]
        seen += ids.tolist()
    return out


def check_case(data, shards, ks, fam, tag):
    """every property of the model that brute force can state, for every k and every query of a case: no query is left out"""
    n = data.n
    for k in ks:
        blocks = [[] for _ in shards]
        lists = [[] for _ in shards]
        for q in range(len(data.scores)):
            s = data.scores[q]
            nan = bool(np.isnan(s).any())
            keys = M.keys_of(s)
            models = [model_of(data, sh, q, k, fam=fam) for sh in shards]
            for si, (sh, m) in enumerate(zip(shards, models)):
                assert m.exact, "%s: only the floods may leave the exact model" % tag
                blocks[si].append(m.block)
                lists[si].append((m.rows.astype(np.uint64) << np.uint64(32)) | m.bits.astype(np.uint64))
                listed, flags, cnt, unproven, cut = S.header(m.block)
                REACHED["flag reason: " + (m.reasons[0].split(":")[0] if m.reasons else "none")] += 1
                if flags:
                    assert unproven == 1 and cnt == 0 and cut == 0
                    continue
                assert not nan or not (np.isnan(s[sh.pilot]).any() or np.isnan(s[sh.r0:sh.r1]).any())
                assert m.rows.tolist() == brute_list(data, sh, q, k + 1), "%s k %d q %d shard %d: the list" % (tag, k, q, si)
                assert (m.bits == s[m.rows].view(np.uint32)).all()
                assert listed == len(m.rows) and unproven == 0, "%s: nothing of the grid overflows a buffer" % tag
                REACHED["branch " + m.branch] += 1
                REACHED["cut 0"] += cut == 0
                REACHED["fewer than k own rows above the cut: the replica holds the others"] += (not m.take_all and m.n_sel < k and m.pilot_above > 0)
                seen_ids = np.concatenate([sh.pilot, np.arange(sh.r0, sh.r1)])
                REACHED["rows seen " + ("< k" if len(seen_ids) < k else "== k" if len(seen_ids) == k else "== k + 1" if len(seen_ids) == k + 1 else "> k + 1")] += 1
                assert m.take_all == (len(seen_ids) <= k) and m.seen == len(seen_ids)
                if not nan:
                    assert cut <= M.kth_largest(keys, k + 1), "%s: a cut above the global statistic" % tag
                    assert cut == M.kth_largest(keys[seen_ids], k + 1)
                    if len(sh.pilot) == 0 or (sh.pilot == np.arange(len(sh.pilot))).all():      # the layouts the numpy block of the merge test covers
                        ref = S.shard_block(s, keys, sh.r0, sh.r1, len(sh.pilot), k, k + 3)
                        assert (m.block[1:] == ref[1:3 + cnt]).all(), "%s k %d q %d shard %d: the block" % (tag, k, q, si)
            status = S.merge_model([m.block for m in models], s, k)
            REACHED["status %d" % status] += 1
            if not any(m.flags for m in models):
                cut = max(m.cut for m in models)
                ents = np.concatenate([m.block[3:] for m in models])
                above = np.flatnonzero(keys > cut)
                got = (ents >> np.uint64(32)).astype(np.int64)
                assert len(set(got.tolist())) == len(got) and sorted(got[keys[got] > cut].tolist()) == above.tolist(), \
                    "%s k %d q %d: the union of the entries does not hold every row above max(cut)" % (tag, k, q)
        # the host merge and the host replay over the model's words: the library's own status is the model's, its answers the oracle's
        stride = k + 3
        host = [np.stack([np.concatenate([b, np.zeros(stride - len(b), np.uint64)]) for b in bl]) for bl in blocks]
        nq = len(data.scores)
        idx, sc, cnt, status = B.merge_answers(host, nq, n, k, 1)
        offs = [np.concatenate([[0], np.cumsum([0 if S.header(blocks[si][q])[1] else len(l) for q, l in enumerate(ls)])]).astype(np.int64)
                for si, ls in enumerate(lists)]
        packed = [np.concatenate([l for q, l in enumerate(ls) if not S.header(blocks[si][q])[1]] + [np.zeros(0, np.uint64)]) for si, ls in enumerate(lists)]
        ri, rs, rc = B.replay_batch(packed, offs, nq, n, k, 1)
        for q in range(nq):
            want = S.merge_model([bl[q] for bl in blocks], data.scores[q], k)
            assert status[q] == want, "%s k %d q %d: bbq_merge_answers says %d, the model %d" % (tag, k, q, status[q], want)
            if want == 2:
                continue
            oi, osc = O.heap_topk(data.scores[q], k)
            if want == 0:
                assert cnt[q] == len(oi) and (idx[q, :cnt[q]] == oi).all() and (sc[q, :cnt[q]].view(np.uint32) == osc.view(np.uint32)).all()
            assert rc[q] == len(oi) and (ri[q, :rc[q]] == oi).all() and (rs[q, :rc[q]].view(np.uint32) == osc.view(np.uint32)).all(), \
                "%s k %d q %d: the lists do not replay to the oracle's answer" % (tag, k, q)


@pytest.mark.parametrize("case", GRID, ids=[c.name for c in GRID])
def test_grid_model_against_brute_force(case):
    data = S.case_data(case)
    check_case(data, data.shards, S.KS_ANSWERS, case.fam, case.name)


@pytest.mark.parametrize("case", TINY, ids=[c.name for c in TINY])
def test_tiny_model_against_brute_force(case):
    data = S.case_data(case)
    check_case(data, data.shards, S.TINY_KS, case.fam, case.name)


@pytest.mark.parametrize("case", S.SPECIAL, ids=[c.name for c in S.SPECIAL])
def test_special_model_against_brute_force(case):
    data = S.case_data(case)
    check_case(data, data.shards, (S.TIE_K,) if case.variant == "ties" else (10, 100), case.fam, case.name)
    flagged = [[model_of(data, sh, q, 10).flags for q in range(6)] for sh in data.shards]
    if case.variant == "nan own":
        assert flagged == [[0] * 6, [S.FLAG_NAN] * 6]
    elif case.variant == "nan pilot":      # the root owns the row, the shard behind it sees it in its replica only
        assert flagged == [[S.FLAG_NAN] * 6] * 2 and all("pilot" in model_of(data, data.shards[1], q, 10).reasons[0] for q in range(6))
    elif case.variant == "nan query":
        assert [[bool(f) for f in fl] for fl in flagged] == [[q == S.NAN_QUERY for q in range(6)]] * 2
    else:
        assert S.merge_model([model_of(data, sh, 0, S.TIE_K).block for sh in data.shards], data.scores[0], S.TIE_K) == 1
        top = np.sort(data.scores[0])[::-1][:S.TIE_K + 2]
        assert len(np.unique(top)) == 1, "k + 2 copies of the best row"


def test_lists_only_scans_are_subsets_where_both_ranks_plan_the_same_segments():
    """rank k lists are subsets of the rank k + 1 lists of the same k where the two plans agree; where 4 k and 4 (k + 1) round to other
    first segments a row meets a threshold of other rows in each plan and neither list holds the other.  Both kinds are met; the
    lists-only k of the recipe stay exact"""
    met = collections.Counter()
    for case in (GRID[0], GRID[1], GRID[4], next(c for c in GRID if c.name == "w6-ordinary-no_replica")):
        data = S.case_data(case)
        for sh in data.shards:
            for q in range(6):
                a, b = model_of(data, sh, q, 1024, answers=False), model_of(data, sh, q, 1024, answers=True)
                assert a.block is None and a.rows.tolist() == brute_list(data, sh, q, 1024)
                subset = set(a.rows.tolist()) <= set(b.rows.tolist())
                assert subset or not plans_agree(sh, 1024), "%s shard [%d, %d) query %d" % (case.name, sh.r0, sh.r1, q)
                met["agree" if plans_agree(sh, 1024) else "differ, subset" if subset else "differ, no subset"] += 1
                for k in S.KS_LISTS:
                    m = model_of(data, sh, q, k, answers=False)
                    assert m.exact and not m.flags and m.rows.tolist() == brute_list(data, sh, q, k)
    assert met["agree"] and met["differ, no subset"], met


def test_hostile_plants_fall_in_the_replica_the_first_and_the_last_segment():
    fam = S.W1
    n, shards = S.layouts(fam)["whole prefix"]
    sh = shards[1]
    segs = [g for g in S.shard_segments(len(sh.pilot), sh.r1 - sh.r0, 11, 1024, 2) if g.emit]
    tiles = M.plant_tiles(fam)
    at = {kind: t * M.TILE for kind, t in tiles.items()}      # (the tile's first row: the tiles are 64 rows, the segments thousands)
    assert at["add_pinf"] < sh.r0                                                                    # in the replica
    assert segs[0].first <= at["lu_nonfinite"] - sh.r0 < segs[0].first + segs[0].rows                # in the shard's first segment
    assert segs[-1].first <= at["add_1e300"] - sh.r0                                                 # in its last


# ------------------------------------------------------------------------------------------------ the floods
def flood_case(which):
    sh = S.flood_shards(which)[1]
    data = S.flood_data("mid" if which == "mid" else "inner")
    return data._replace(scores=tuple(s[:sh.r1] for s in data.scores), n=sh.r1), sh


def test_floods_reach_every_kind_and_every_flag_reason():
    k = S.FLOOD_K
    for which in ("last", "inner", "mid"):
        sub, sh = flood_case(which)
        plan = S.shard_segments(len(sh.pilot), sh.r1 - sh.r0, k + 1, 1024, 2)
        own = [g for g in plan if g.emit]
        assert len(own) == (3 if which == "last" else 4)
        for q, src in enumerate(S.FLOOD_QUERIES):
            m = model_of(sub, sh, q, k, fam=S.W1)
            if src != 0:
                assert m.exact and m.ok and not m.flags and max(m.split) < 2000, "query %d floods" % src
                continue
            assert not m.flags, m.reasons
            dev = model_of(sub, sh, q, k, fam=S.W1, subset=True)      # what the keys that fit give
            if which == "last":      # (a) only the LAST own segment exceeds the key buffer: modelled completely - unproven, no cut, the list whole
                assert m.exact and max(m.split[:-1]) <= S.KEY_CAP - (k + 1) < m.split[-1]
                assert m.why_not == "m_new > kFinalizeKeyCap - tcount" and S.header(m.block)[2:] == (0, 1, 0)
                assert S.header(m.block)[0] == len(m.rows) > S.planned_list_cap(plan, k + 1)
                continue
            # (b) a segment that is NOT the last does: the invariants only
            assert not m.exact and not dev.exact and max(m.split[:-1]) > S.KEY_CAP - (k + 1) and m.ok
            assert set(m.rows.tolist()) <= set(dev.rows.tolist())
            if which == "inner":     # the best of the segment fall off: more than k own rows above the subset's statistic, unproven
                assert dev.why_not == "n_sel > k2" and dev.n_sel == 21 and S.header(dev.block)[2:] == (0, 1, 0)
            else:                    # ranks 15, 14, 11, 10 fall off: a PROVEN block whose cut lies below the true one
                assert dev.ok and 0 < dev.cut < m.cut and m.n_sel == 3 and dev.n_sel == 5 <= k and dev.split[-1] == 0
                ranked = np.sort(M.keys_of(np.concatenate(S.shard_scores(sub, sh, q))))[::-1]
                assert (m.cut, dev.cut) == (int(ranked[10]), int(ranked[12])) and dev.pilot_above == S.MID_REPLICA_RANKS
        # every source of kFlagOverflow, from the flooding query: no flood tier (flood_rows 0; the shared sweep of sweep_share 4), the
        # over-full chunks beyond a small tier, and the list beyond its own capacity
        for opts, reasons in ((dict(S.OPTS, flood_rows=0), ["no flood tier"]), (dict(S.OPTS, sweep_share=4), ["no flood tier"]),
                              (dict(S.OPTS, flood_rows=1024), ["over the list's", "over the flood tier's 1024"])):
            m0 = model_of(sub, sh, 0, k, opts=opts, fam=S.W1)
            assert m0.flags == S.FLAG_OVERFLOW and S.header(m0.block)[1:] == (S.FLAG_OVERFLOW, 0, 1, 0)
            for r in reasons:
                assert any(r in x for x in m0.reasons), (which, opts, m0.reasons)
            assert not any(model_of(sub, sh, q, k, opts=opts, fam=S.W1).flags for q in (1, 3, 5)), "a query that does not flood is flagged"
        assert S.shared_sweep(S.W1, dict(S.OPTS, sweep_share=4), 32) and S.shared_sweep(S.W1, dict(S.OPTS, sweep_share=8), 32)
        assert not S.shared_sweep(S.W1, dict(S.OPTS, sweep_share=32), 32) and not S.shared_sweep(S.W1, S.OPTS, 32)
    # the smallest sizes: one own row fewer and the condition is gone
    for which, fewer in (("last", 1), ("inner", 2)):
        sub, sh = flood_case(which)
        sh = sh._replace(r1=sh.r1 - fewer)
        sub = sub._replace(scores=tuple(s[:sh.r1] for s in sub.scores), n=sh.r1)
        m = model_of(sub, sh, 0, k, fam=S.W1)
        assert m.exact and (which == "inner" or m.ok or m.split[-1] <= S.KEY_CAP - (k + 1))


def test_a_flood_shard_lists_exactly_the_advertised_capacity():
    sh, cap = S.flood_shard_at_capacity()
    data = S.flood_data()
    sub = data._replace(scores=tuple(s[:sh.r1] for s in data.scores), n=sh.r1)
    lengths = [len(model_of(sub, sh, q, S.FLOOD_K, fam=S.W1).rows) for q in (0, 2, 1)]      # FLOOD_QUERIES: query 0 twice, then one that does not flood
    assert lengths[:2] == [cap, cap] and lengths[2] < cap // 4
    flags, off, total, oom = S.pack_model(lengths, [0, 0, 0], cap, 2 * cap)      # the squeeze round runs and drops nothing: "c > advertised_cap"
    assert not flags.any() and total == sum(lengths) and oom


def test_exact_is_false_only_for_the_non_last_floods():
    """the cap that keeps the suite honest: everything but the flooding query of the `inner` and `mid` layouts is modelled completely (the grid, the
    tiny shards and the special cases assert m.exact per model in check_case)"""
    for which in ("last", "inner", "mid"):
        sub, sh = flood_case(which)
        got = [model_of(sub, sh, q, S.FLOOD_K, fam=S.W1).exact for q in range(len(S.FLOOD_QUERIES))]
        assert got == [not (which != "last" and src == 0) for src in S.FLOOD_QUERIES]
        root = S.flood_shards(which)[0]
        assert all(model_of(sub, root, q, S.FLOOD_K, fam=S.W1).exact for q in range(len(S.FLOOD_QUERIES)))


def test_pack_model_squeezes_only_when_the_sum_does_not_fit():
    cap = 5120
    lengths, flags = [40000, 900, 40000, 1100, 5120, 5121], [0, 0, 0, 0, 0, 0]
    f, off, total, oom = S.pack_model(lengths, flags, cap, 1 << 20)            # generous: nothing is dropped
    assert not f.any() and total == sum(lengths) and not oom
    f, off, total, oom = S.pack_model(lengths, flags, cap, 6 * cap)            # the sum does not fit: exactly the lists over the advertised capacity go
    assert f.tolist() == [1, 0, 1, 0, 0, 1] and total == 900 + 1100 + 5120 and not oom and np.diff(off).tolist() == [0, 900, 0, 1100, 5120, 0]
    f, off, total, oom = S.pack_model(lengths, flags, cap, 7000)               # smaller than nq x cap and still not fitting
    assert oom and total == 7120
    f, off, total, oom = S.pack_model(lengths, [0, 2, 0, 0, 0, 0], cap, 6 * cap)
    assert f.tolist() == [1, 2, 1, 0, 0, 1] and total == 1100 + 5120
    f, off, total, oom = S.pack_model([cap] * 6, flags, cap, 6 * cap)          # every list exactly at the capacity fits
    assert not f.any() and total == 6 * cap and not oom


# ------------------------------------------------------------------------------------------------ the plan
def test_the_plan_without_a_replica_is_call_walks_and_with_one_covers_both_storages():
    for n in (1, 63, 511, 512, 513, 1024, 1025, 4133, 8229, 20517, 46117, 100000):
        for k in (1, 10, 100, 1024, 4096):
            for fsr, growth in ((1024, 2), (4096, 8), (8192, 64)):
                got = [(g.first, g.rows, g.dense) for g in S.shard_segments(0, n, k + 1, fsr, growth)]
                assert got == W.plan_segments(n, k, fsr, growth) or n < k, (n, k, fsr, growth)
                if n < k:      # (plan_segments clamps k to n, a shard scan does not: one dense segment either way)
                    assert got == [(0, n, True)]
    for P in (512, 1024, 1237, 3072, 4096):
        for R in (1, 65, 513, 4133, 19280, 43008):
            for k_dev in (2, 11, 1025):
                segs = S.shard_segments(P, R, k_dev, 1024, 2)
                pilot, own = [g for g in segs if g.storage == 0], [g for g in segs if g.storage == 1]
                assert segs == pilot + own and not any(g.emit for g in pilot) and all(g.emit and not g.dense for g in own)
                assert pilot[0].dense and not any(g.dense for g in pilot[1:])
                for part, rows in ((pilot, P), (own, R)):
                    assert part[0].first == 0 and sum(g.rows for g in part) == rows
                    assert all(a.first + a.rows == b.first and b.first % 512 == 0 for a, b in zip(part, part[1:]))
                assert [g.before for g in own] == [P + g.first for g in own]
                for a in own[:-1]:      # a boundary multiplies the rows seen by the growth (to the chunk) and stays within half the storage
                    end = a.first + a.rows
                    assert end == ((P + a.first) * 2 - P) // 512 * 512 and end <= R // 2


def test_the_rules_are_the_sources():
    core, kernels, shard, multi, device = (_source(n) for n in ("bbq_core.cpp", "bbq_kernels.hip", "bbq_shard.cpp", "bbq_multi.cpp", "bbq_device.h"))
    # the plan
    assert "add_storage_segments(ix, p, 0, ix->pilot, 0, false, false, dummy);" in core
    assert "add_storage_segments(ix, p, 1, ix->main, ix->pilot.view.n_rows, true, true, expected_emit);" in core
    assert "const int64_t nb = (before * p.growth - rows_before) / kChunkRows * kChunkRows;" in core
    assert "if (before > 0 && nb > b && nb <= R / 2) e = nb;" in core
    assert "if (!p.segs.empty()) p.segs.back().need_theta = false;" in core
    assert "p.list_cap = listed_whole + (int64_t)(4.0 * sparse) + 4096;" in core
    assert "p.flood_cap = std::min<int64_t>(ix->opt_flood, (ix->main.view.n_rows + 1023) / 1024 * 1024);" in core
    assert "const double lam = (double)k * kChunkRows / (double)std::max<int64_t>(rows_before, 1);" in core
    # the rank, the scan's own list capacity, the two-in-flight rule, what is refused
    assert "c.k_dev = answers ? k + 1 : k;" in shard
    assert "const Plan plan = build_plan(ix, c.k_dev, answers ? k : 0);" in shard
    assert "const int64_t list_cap = plan.list_cap + std::min<int64_t>(plan.flood_cap, 65536);" in shard
    assert "if (ix->shard_begun - ix->shard_waited >= 2) return fail(BBQ_ERR_INVALID_ARG," in shard
    assert "if (ix->shard_begun == ix->shard_waited) return fail(BBQ_ERR_INVALID_ARG," in shard
    assert "if (total > set->packed_cap) return fail(BBQ_ERR_OOM," in shard
    assert "if (k == 0 || k > kMaxFastK) return fail(BBQ_ERR_UNSUPPORTED," in shard and "if (dev_answers && k > kFinalSelectMax)" in shard
    assert "return (keff <= kFinalSelectMax ? build_plan(ix, keff + 1, keff) : build_plan(ix, keff)).list_cap;" in shard
    assert "bool use_mfma = !ext && c.share == 32 && c.maxq <= 127 && ix->geom.store_bits == 1;" in core
    assert "f.final_shard = use_final ? 0 : 1;" in core
    # the flags
    assert "if (base + m_new > a.list_cap) flags |= kFlagOverflow;" in kernels
    assert "if ((uint64_t)off + cnt <= (uint64_t)a.ovf_cap) {" in _source("bbq_scan_body.h")
    assert "constexpr uint32_t kFlagOverflow = 1u;" in device and "constexpr uint32_t kFlagNaN = 2u;" in device
    assert (S.FLAG_OVERFLOW, S.FLAG_NAN, S.KEY_CAP) == (1, 2, 12288) and "constexpr int kFinalizeKeyCap = 12288;" in device
    # the `ok` chain, shard-mode take_all, the cut in slot 2
    assert "bool ok = f_all == 0 && a.emit && total <= a.list_cap && k2 >= 1 && k2 <= kFinalSelectMax && k2 + hdr_slots <= a.final_stride &&" in kernels
    assert "m_new <= (uint32_t)kFinalizeKeyCap - tcount && a.k == k2 + 1;" in kernels
    assert "const bool take_all = shard ? (m_new + tcount < (uint32_t)(k2 + 1)) : (total <= (int64_t)k2);" in kernels
    assert "} else if (M <= 2048u) {" in kernels
    assert "th1 = block_select_kth_largest(s_keys, M, (uint32_t)(k2 + 1), s_hist, s_wave, s_misc + 8);" in kernels
    assert "ok = shard ? (n_sel <= (uint32_t)k2) : take_all ? (n_sel == (uint32_t)total) : (n_sel == (uint32_t)k2);" in kernels
    assert "if (shard) hdr[2] = (ok && !take_all) ? (uint64_t)th1 : 0ull;" in kernels
    assert "s_sel[slot] = ((uint64_t)key << 32) | (ent[u] >> 32);" in kernels and "rank += y > x ? 1u : 0u;" in kernels
    # the squeeze
    assert "if (!f && squeeze && (int64_t)c > advertised_cap) f = (int32_t)kFlagOverflow;" in kernels
    assert "if ((int64_t)s_base <= packed_cap) break;" in kernels
    # the multi-device handle: its shards, and the three figures of its statistics that are functions of the model
    assert "if (r0 > 0) P = pilot_rows >= r0 ? r0 : pilot_rows / kChunkRows * kChunkRows;" in multi
    assert "for (int s = 0; s < S; ++s) ix->stats.candidates += AnswerHeader(blocks[(size_t)s] + (size_t)q * (size_t)strides[(size_t)s]).count;" in multi
    assert "ix->stats.host_replays += 1;\n          ix->stats.candidates += cand;" in multi
    assert "ix->stats.dense_fallbacks += 1;\n        ix->stats.candidates += ix->n_rows;" in multi


def test_the_recipe_reaches_what_it_is_for():
    """what the parametrised tests above have met; run on its own, it walks the w1 cases itself"""
    if not REACHED:
        for case in [c for c in GRID + TINY if c.fam is S.W1 and c.kind == "ordinary"] + list(S.SPECIAL):
            data = S.case_data(case)
            check_case(data, data.shards, S.TINY_KS if case.layout.startswith("tiny") else (10, 1024), case.fam, case.name)
    for what in ("branch count", "branch radix", "branch take_all", "cut 0", "fewer than k own rows above the cut: the replica holds the others",
                 "rows seen < k", "rows seen == k", "rows seen == k + 1", "rows seen > k + 1", "status 0", "status 1", "status 2",
                 "flag reason: none", "flag reason: a NaN score in the pilot replica", "flag reason: a NaN score in the own rows"):
        assert REACHED[what] > 0, "the recipe never reaches: %s (%s)" % (what, dict(REACHED))
