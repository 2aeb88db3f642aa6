"""CPU: what the call walks of tests/call_walk.py cover, so that tests/test_gpu_call_walk.py cannot pass while a hazard goes unvisited,
and the host rules the cast leans on, restated in call_walk and held to the source lines here: a change of a rule that decides which
kernel or which chain a member reaches fails here instead of leaving the walks on another path than their comments name.  Over the
default seeds (BBQ_CALL_WALK_SEEDS for more, never fewer than the default): every kind occurs, every listed transition occurs with the
paths it is about (the matrix-core sweeps under sweep_share 32 among them), every option takes every listed value with the same call on
both sides, every member is the target of every kind it admits,
a shard batch is in flight across a step of every kind, every refusal is made, and every walk ends with nothing in flight."""
import os
import re

import numpy as np
import pytest

import call_walk as W
import orclib as O

CSRC = os.path.join(O.ROOT, "better-binary-quantization_amd", "csrc")
SEEDS = tuple(range(max(W.DEFAULT_SEEDS, int(os.environ.get("BBQ_CALL_WALK_SEEDS", "0")))))


def _source(name):
    with open(os.path.join(CSRC, name) if not name.endswith("bbq.h") else os.path.join(O.ROOT, "include", "bbq.h"), encoding="utf-8") as f:
        return f.read()


_walks = {}


def walk(seed):
    if seed not in _walks:
        _walks[seed] = W.walk(seed)
    return _walks[seed]


def all_steps():
    return [(seed, i, s) for seed in SEEDS for i, s in enumerate(walk(seed))]


# ---------------------------------------------------------------------------------------------------- coverage
def test_walks_are_deterministic_and_describable():
    for seed in SEEDS:
        a, b = W.walk(seed), W.walk(seed)
        assert [W.describe(s) for s in a] == [W.describe(s) for s in b]
        assert 180 <= len(a) <= 300, len(a)
        assert sum(s["via"] == "free" for s in a) >= 0.2 * len(a)
        for s in a:
            assert s["kind"] in W.KINDS and s["kind"] in W.ADMITS[s["member"]], W.describe(s)
            assert "\n" not in W.describe(s)


def test_every_kind_occurs_in_every_walk_set():
    seen = {s["kind"] for _, _, s in all_steps()}
    assert seen == set(W.KINDS), set(W.KINDS) - seen


def test_every_member_is_the_target_of_every_kind_it_admits():
    seen = {(s["member"], s["kind"]) for _, _, s in all_steps()}
    want = {(m, k) for m in W.CAST for k in W.ADMITS[m]}
    assert want <= seen, sorted(want - seen)


def test_every_listed_transition_occurs_in_every_walk():
    for seed in SEEDS:
        steps = walk(seed)
        for name, pattern in W.TRANSITIONS.items():
            mine = [s for s in steps if s["via"] == name]
            assert [(s["kind"], s["member"]) for s in mine] == list(pattern), (seed, name)
            at = [i for i, s in enumerate(steps) if s["via"] == name]
            assert at == list(range(at[0], at[0] + len(at))), "%s is interrupted in walk %d" % (name, seed)


def test_the_latency_transitions_reach_the_chains_they_name():
    """with the options in force when the step is played: the general path dirties slot 0, the chains expect it clean"""
    want = {
        "general_then_latency": ["general", "chain"],
        "latency_then_general_then_latency": ["chain", "general", "chain"],
        "presampled_unproven_then_chain_then_another_index": ["presampled", "chain", "presampled"],
    }
    for seed in SEEDS:
        got = {name: [] for name in want}
        for s, (opts, _, n) in W.replay(walk(seed)):
            if s["via"] in want:
                m = W.CAST[s["member"]]
                got[s["via"]].append(W.single_query_path(m, n, s["k"], opts) if s["nq"] == 1 else "general")
        assert got == want, seed
        tied = [s for s in walk(seed) if s["via"] == "presampled_unproven_then_chain_then_another_index" and s["member"] == "long"]
        assert [s["q0"] < W.TIED_QUERIES for s in tied] == [True, False]       # the first cannot be proven and goes on to the chain


def test_every_walk_sweeps_wide_on_the_matrix_cores():
    """sweep_share 32 in force - and nothing else that would take the call off the matrix cores - for 70 queries, the filtered call, the
    raw feed and a k the host replays, in EVERY walk"""
    core = _source("bbq_core.cpp")
    assert "bool use_mfma = !ext && c.share == 32 && c.maxq <= 127 && ix->geom.store_bits == 1;" in core
    assert "for (int i = 0; i < nq && use_mfma; ++i) use_mfma = mfma_query_ok(hq[i]);" in core
    assert "if (c.share != 32) c.share = 1;" in core                                        # a filtered call keeps 32 alone
    assert "if (ix->opt_share == 32 && q < 64 && (n_queries == 0 || n_queries > 32)) q = 64;" in core
    assert "if (n_queries <= 64 || k == 0 || ix->multi) {" in core                          # the feed: more than 64 raw queries
    assert "c.maxq = (1 << query_bits) - 1;" in core and "c.maxq = c.planes <= 4 ? 15 : max_value(" in core
    assert "if (keff > kMaxFastK || ix->opt_force_dense) {" in core
    wide = W.CAST["wide"]
    for seed in SEEDS:
        seen = []
        for s, (opts, _, n) in W.replay(walk(seed)):
            if s["via"] == "matrix_core_sweeps" and s["kind"] != "set_option":
                n_eff = int(W.mask_of("wide", n, s["filter"]).sum()) if "filter" in s else n
                assert opts.get("sweep_share") == 32 and W.matrix_core_sweep(wide, n_eff, s["k"], opts), (seed, W.describe(s), opts)
                seen.append((s["kind"], s["nq"], s["k"] > W.K_FINAL_SELECT_MAX))
        assert ("search_batch", 70, False) in seen and ("search_raw_batch", 70, False) in seen and ("search_batch", 130, True) in seen, (seed, seen)
        assert {nq for kind, nq, _ in seen if kind == "search_filtered_batch"} == {70, 33}, (seed, seen)
    assert not W.matrix_core_sweep(wide, wide.n0, 10, {}) and not W.matrix_core_sweep(wide, wide.n0, 10, {"sweep_share": 4})
    assert not W.matrix_core_sweep(wide, wide.n0, 10, {"sweep_share": 32, "force_dense": 1}) and not W.matrix_core_sweep(W.CAST["multi"], 200, 10, {"sweep_share": 32})


def test_every_ordered_pair_of_the_d_span_users_occurs():
    for seed in SEEDS:
        kinds = [s["kind"] for s in walk(seed)]
        pairs = {(a, b) for a, b in zip(kinds, kinds[1:])}
        want = {(a, b) for a in W.D_SPAN_USERS for b in W.D_SPAN_USERS}
        assert want <= pairs, (seed, sorted(want - pairs))


def test_every_option_takes_two_values_around_the_same_call():
    header = _source("bbq.h")
    names = [n for n, _ in W.OPTIONS]
    for n in names:
        assert re.search(r"\b%s\b" % n, header), n
    # every name bbq_set_option knows is in the list
    known = set(re.findall(r'n == "([a-z0-9_]+)"', _source("bbq_index.cpp")))
    assert known == set(names), known ^ set(names)
    assert set(W.OPTION_CALLS) == set(names)
    values = {n: set() for n in names}
    around = set()
    for seed in SEEDS:
        steps = walk(seed)
        for (s, (opts, _, _)) in W.replay(steps):
            if s["kind"] not in ("set_option", "stats", "reset_stats", "recreate", "save", "refused"):
                for n, vals in W.OPTIONS:
                    values[n].add(opts.get(n, vals[0]))
        for a, b, c in zip(steps, steps[1:], steps[2:]):
            if b["kind"] == "set_option" and b["via"] == "option:" + b["option"] and a["member"] == b["member"] == c["member"] and W.describe(a) == W.describe(c):
                around.add(b["option"])
    assert around == set(names), set(names) - around
    for n, vals in W.OPTIONS:      # every listed value is in force for a call somewhere in the default walks
        assert values[n] >= {v for v in vals if v is not None}, (n, values[n])


def test_a_batch_is_in_flight_across_a_step_of_every_kind():
    seen = set()
    for seed in SEEDS:
        for s, (_, in_flight, _) in W.replay(walk(seed)):
            if in_flight > 0:
                seen.add(s["kind"])
    assert seen == set(W.KINDS), set(W.KINDS) - seen


def test_every_refusal_is_made_between_two_identical_calls():
    seen = set()
    for seed in SEEDS:
        steps = walk(seed)
        for a, b, c in zip(steps, steps[1:], steps[2:]):
            if b["kind"] == "refused" and b["via"] == "refused_between" and W.describe(a) == W.describe(c) and a["kind"] == "search_batch":
                seen.add(b["what"])
    assert seen == {w for w, _, _ in W.REFUSALS}, {w for w, _, _ in W.REFUSALS} - seen


def test_every_walk_ends_with_nothing_in_flight_and_within_its_limits():
    for seed in SEEDS:
        flights = {m: 0 for m in W.CAST}
        n = {name: m.n0 for name, m in W.CAST.items()}
        for s in walk(seed):
            m = s["member"]
            if s["kind"] == "shard_begin":
                flights[m] += 1
                assert flights[m] <= 2, W.describe(s)
            elif s["kind"] == "shard_wait":
                flights[m] -= 1
                assert flights[m] >= 0, W.describe(s)
            elif s["kind"] == "shard_scan":
                assert flights[m] == 0, W.describe(s)
            elif s["kind"] == "recreate":
                flights[m] = 0
            elif s["kind"] == "append":
                n[m] += len(s["rows"])
                assert n[m] <= W.MAX_ROWS[m]
            elif s["kind"] == "refused":
                assert {"third_begin": flights["shard"] == 2, "append_with_unwaited_batch": flights["root"] > 0,
                        "wait_with_nothing_in_flight": flights["shard"] == 0}.get(s["what"], True), W.describe(s)
            if "spans" in s:
                for sp in s["spans"]:
                    assert (sp[:, 0] >= 0).all() and (sp[:, 0] <= sp[:, 1]).all() and (sp[:, 1] <= n[m]).all() and (sp[1:, 0] >= sp[:-1, 1]).all(), W.describe(s)
            if m == "long" and "k" in s:
                assert s["k"] <= W.K_FINAL_SELECT_MAX + 1
        assert not any(flights.values()), (seed, flights)


def test_the_k_and_query_counts_of_the_edges_are_drawn():
    ks = {s["k"] for _, _, s in all_steps() if s["kind"] == "search_batch"}
    assert {1, 10, 100, W.K_FINAL_SELECT_MAX, W.K_FINAL_SELECT_MAX + 1, W.K_MAX_FAST_K} <= ks, ks
    assert {s["nq"] for _, _, s in all_steps() if s["kind"] == "search_batch"} >= {1, 5, 33, 70, 130}
    counts = {c for _, _, s in all_steps() if "tokens" in s for _, c in s["tokens"]}
    assert counts == {1, W.TOKEN_BLOCK, W.TOKEN_BLOCK + 1}
    assert {s["nq"] for _, _, s in all_steps() if s["kind"] == "search_raw_batch"} == {5, 70}
    assert {s["shape"] for _, _, s in all_steps() if s["kind"] == "rerank"} >= {"long_lists", "one_row"}


def test_read_only_walks_hold_read_only_kinds():
    for seed in range(4):
        steps = W.read_only_walk(seed)
        assert {s["kind"] for s in steps} <= set(W.READ_ONLY) and all(s["member"] == "ties" for s in steps)
        assert any(s["kind"] == "refused" for s in steps)
        assert {s["kind"] for s in steps} >= {"search_batch", "search_filtered_batch", "search_spans", "search_grouped", "search_maxsim", "range", "score_ords"}


# ---------------------------------------------------------------------------------------------------- the rules behind the cast
def test_the_constants_are_the_sources():
    device, host, latency = _source("bbq_device.h"), _source("bbq_host.h"), _source("bbq_latency.cpp")
    assert "constexpr int kFinalSelectMax = %d;" % W.K_FINAL_SELECT_MAX in device
    assert "constexpr int64_t kMaxFastK = %d;" % W.K_MAX_FAST_K in host
    assert "constexpr int kLatPreKeys = %d;" % W.K_LAT_PRE_KEYS in device
    assert "constexpr int kTileRows = %d;" % W.TILE in device
    assert "N < %d" % W.PRESAMPLE_MIN_ROWS in latency
    assert re.search(r"#define BBQ_CHUNK_ROWS %d\b" % W.CHUNK, device) and "BBQ_CHUNK_ROWS" not in _source("Makefile")
    assert "constexpr int kMaxSimTokenBlock = %d;" % W.TOKEN_BLOCK in device


def test_wide_reaches_digit_planes_and_eight_tiles_per_wave():
    core, body, dev = _source("bbq_core.cpp"), _source("bbq_scan_body.h"), _source("bbq_device.h")
    assert "return ix->opt_digit_planes != 0 && ix->geom.store_bits == 1 && planes == 4 && row_sums_for_launch(ix) && row_sums_fit(ix->geom);" in core
    assert "bool row_sums_for_launch(const bbq_index *ix) { return ix->opt_row_sums < 0 ? ix->opt_resident_mb != 0 : ix->opt_row_sums != 0; }" in core
    assert "return g.layout == kLayoutCompact && (int64_t)g.dim * ((1 << g.store_bits) - 1) <= 65535;" in dev
    assert "return W == 6 || (!FILT && (W == 8 || W == 12));" in body
    assert "return !FILT && digit_twin<FILT, QB, W, SB>() && (W == 6 || W == 8 || W == 12);" in body
    assert re.search(r"case 6: return 8;\s*case 8: return 8;\s*default: return 1;", core)
    wide = W.CAST["wide"]
    assert W.w16_of(wide.dim) == 6 and wide.compact and wide.qb == 4
    assert W.digit_planes_apply(wide) and W.digit_planes_apply(wide, filtered=True) and W.tiles_per_wave_of(wide) == 8
    assert not W.digit_planes_apply(wide, resident_mb=0) and W.digit_planes_apply(wide, resident_mb=0, row_sums=1) and not W.digit_planes_apply(wide, digit_planes=0)
    for other in ("ties", "multi"):
        assert not W.digit_planes_apply(W.CAST[other]) and W.tiles_per_wave_of(W.CAST[other]) == 1
    # the fused MaxSim kernel: "4 query bit-planes against 1-bit rows of 6, 8 or 12 16-byte chunks" (include/bbq.h, maxsim_fused)
    assert "4 query bit-planes against 1-bit rows of 6, 8 or 12 16-byte chunks" in _source("bbq.h")
    # sweep_share 32: 64 queries per launch chain from 33 queries on, so 70 queries are two launches, the second one ragged
    assert "if (ix->opt_share == 32 && q < 64 && (n_queries == 0 || n_queries > 32)) q = 64;" in core
    assert "bool use_mfma = !ext && c.share == 32 && c.maxq <= 127 && ix->geom.store_bits == 1;" in core


def test_the_single_query_paths_of_the_cast():
    lat, kern, core = _source("bbq_latency.cpp"), _source("bbq_latency_kernels.hip"), _source("bbq_core.cpp")
    assert "return v.geom.store_bits == 1 && (v.geom.w16 == 6 || v.geom.w16 == 8 || v.geom.w16 == 12) &&" in kern
    assert "int64_t P = ((k2 + 2) * N / 6000 + kChunkRows - 1) / kChunkRows * kChunkRows;" in lat
    assert "P = std::max<int64_t>(P, 8192);" in lat and "if (P > N / 4) return BBQ_OK;" in lat
    assert "int per_wave = (P / kTileRows >= 8 * (k2 + 2)) ? 1 : 4;" in lat and "if (P / kTileRows * per_wave > kLatPreKeys) per_wave = 1;" in lat
    assert "if (n_keys > kLatPreKeys || n_keys < k2 + 2) return BBQ_OK;" in lat
    assert "p.final_k < 1 || p.final_k > kFinalSelectMax || p.segs.empty() || !p.segs[0].dense || !latency_path_supported(ix->main.view, c.planes))" in lat
    assert "if (p.segs[i].dense || p.segs[i].storage != 1) return BBQ_OK;" in lat
    assert "const bool latency = final_k > 0 && n_queries <= ix->opt_latency_queries;" in core
    assert "if (n_queries == 1 && plan.latency && !feed && !flt) {" in core
    assert "const int64_t nb = (before * p.growth - rows_before) / kChunkRows * kChunkRows;" in core and "if (before > 0 && nb > b && nb <= R / 2) e = nb;" in core
    long, wide, ties = W.CAST["long"], W.CAST["wide"], W.CAST["ties"]
    assert long.n0 == W.PRESAMPLE_MIN_ROWS + W.CHUNK and W.latency_supported(long) and W.latency_supported(wide)
    assert not W.latency_supported(ties) and not W.latency_supported(W.CAST["multi"])       # 64 dimensions: one chunk, no chain at all
    for k in (1, 10, 100, W.K_FINAL_SELECT_MAX):                 # the k values a single-query step draws on `long`
        P, per_wave, n_keys = W.presample_plan(long.n0, k)
        assert P <= long.n0 // 4 and k + 2 <= n_keys <= W.K_LAT_PRE_KEYS, (k, P, n_keys)
        assert W.single_query_path(long, long.n0, k, {}) == "presampled"
        assert W.single_query_path(long, long.n0, k, {"latency_presample": 0}) == "chain"
        assert W.single_query_path(wide, wide.n0, k, {}) == "chain"
        assert W.single_query_path(ties, ties.n0, k, {}) == "general"
    assert W.presample_plan(long.n0 - 2 * W.CHUNK, 10) is None and W.presample_plan(long.n0, W.K_FINAL_SELECT_MAX + 1) is None
    assert W.single_query_path(long, long.n0, W.K_FINAL_SELECT_MAX + 1, {}) == "general"
    # the chain's plan: a dense first segment, sparse ones behind it
    for m in (long, wide):
        for k in (1, 10, 100, W.K_FINAL_SELECT_MAX):
            segs = W.plan_segments(m.n0, k)
            assert segs[0][2] and len(segs) >= 2 and not any(d for _, _, d in segs[1:]) and sum(r for _, r, _ in segs) == m.n0
    for opts in ({"force_dense": 1}, {"device_select": 0}, {"latency_queries": 0}, {"latency_fused": 0}, {"sweep_share": 4}):
        assert W.single_query_path(wide, wide.n0, 10, opts) in ("general", "dense")
    assert W.single_query_path(wide, wide.n0, 10, {"append_last": 0}) == "general"


def test_the_shard_and_the_fixtures_are_what_the_cast_says():
    for name in ("ties", "multi"):
        m = W.CAST[name]
        g = O.load_golden(m.source)
        assert (g["n"], g["dim"], g["ib"], g["qb"], O.SIMS[g["sim"]]) == (m.n0, m.dim, m.ib, m.qb, m.sim)
        assert W.APPEND_POOL[name] == g["n"]
    shard, root, ties = W.CAST["shard"], W.CAST["root"], W.CAST["ties"]
    assert shard.rows == (ties.n0 // 2, ties.n0) and root.rows == (0, ties.n0 // 2) and shard.pilot % 1024 == 0 and 0 < shard.pilot <= shard.rows[0]
    header = _source("bbq.h")
    assert "n_pilot a multiple of 1024, or all row_base of them" in header
    assert "two batches in flight per index" in header and "waits are taken in" in header
    shard_cpp = _source("bbq_shard.cpp")
    assert "if (ix->shard_begun - ix->shard_waited >= 2) return fail(BBQ_ERR_INVALID_ARG" in shard_cpp
    assert 'return fail(BBQ_ERR_INVALID_ARG, "bbq_shard_scan_wait: no batch in flight");' in shard_cpp
    assert 'if (k < 0) return fail(BBQ_ERR_NEGATIVE_K' in _source("bbq_query.cpp")


def test_masks_and_groups():
    for name, m in W.CAST.items():
        for which in ("sparse", "dense"):
            mask = W.mask_of(name, m.n0, which)
            assert mask[0] and mask.shape == (m.n0,) and (mask.mean() < 0.1) == (which == "sparse")
        off = W.offsets_of(m.n0)
        assert off[0] == 0 and off[-1] == m.n0 and (np.diff(off) >= 0).all() and (np.diff(off) == 0).any()
        for which in ("ragged", "filtered"):
            gm = W.group_mask(name, m.n0, which)
            live = W.live_groups(off, gm)
            want = [g for g in range(len(off) - 1) if gm[off[g]:off[g + 1]].any()]
            assert live.tolist() == want
        if m.n0 >= 1000 and "search_grouped" in W.ADMITS[name]:      # the filter leaves some of the small groups without a row
            assert len(W.live_groups(off, W.group_mask(name, m.n0, "filtered"))) < len(W.live_groups(off, W.group_mask(name, m.n0, "ragged")))
