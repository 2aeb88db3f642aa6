"""CPU: the random mutation walk itself (tests/mutation_walk.py), with no device.  A random test can go quiet and hide what it no
longer exercises, so what the DEFAULT walks - every flavour, the default seeds, the walks tests/test_gpu_mutation_walk.py plays on the
device - cover is asserted here: every operation kind and every refusable kind, and the sequences in which one mutation can be wrong
only because another came before it.  The model is held to the library's two host-only restatements, bbq_filter_kept_rows and
bbq_update_winners, on every compaction and update of those walks.  These are conditions, not measurements: when a change to the
walk breaks one, the walk's seeds or biases change, never the assertion."""
import functools

import numpy as np
import pytest

import mutation_walk as M
import orclib as O
from bbqlib import capi

SEEDS = tuple(range(M.DEFAULT_SEEDS))
APPENDS, UPDATES, COMPACTIONS = ("append_rows", "append"), ("update_rows", "update"), ("compact", "remove_rows")


def pool_n(flavour):
    pool = M.FLAVOURS[flavour].pool
    return 1000 if pool == "seeded_1000x129" else O.load_golden(pool)["n"]


@functools.lru_cache(maxsize=None)
def played(flavour, seed):
    """the walk's steps with the model's state before and after each: [(step, src before, capacity tiles before, src after)]"""
    steps = M.walk(seed, pool_n(flavour), flavour)
    assert steps[0]["op"] == "create"
    m = M.IndexModel(steps[0]["rows"], bool(M.FLAVOURS[flavour].odd_rows))
    out = []
    for step in steps[1:]:
        before, cap = m.src.copy(), m.cap_tiles
        M.apply(m, step)
        out.append((step, before, cap, m.src.copy()))
    return steps, out, m


def all_walks():
    return [(f, s) + played(f, s) for f in M.FLAVOURS for s in SEEDS]


def changes(step, before, after):
    """does the step change the rows of the index?"""
    return step["op"] in APPENDS + UPDATES + COMPACTIONS and (len(before) != len(after) or (before != after).any())


def test_the_flavours_describe_their_pools():
    for name, fl in M.FLAVOURS.items():
        if fl.pool == "seeded_1000x129":
            assert (fl.dim, fl.ib, fl.sim) == (129, 1, 1)
        else:
            g = O.load_golden(fl.pool)
            assert (fl.dim, fl.ib, fl.sim) == (g["dim"], g["ib"], O.SIMS[g["sim"]]), name
        assert all(0 <= r < pool_n(name) for r in fl.odd_rows)


@pytest.mark.parametrize("flavour", M.FLAVOURS)
def test_the_same_seed_gives_the_same_steps(flavour):
    for seed in SEEDS:
        a, b = M.walk(seed, pool_n(flavour), flavour), M.walk(seed, pool_n(flavour), flavour)
        assert len(a) == len(b) and M.STEPS + 1 <= len(a) <= M.STEPS + 2   # the creation, the steps, a closing block
        for x, y in zip(a, b):
            assert x.keys() == y.keys()
            for key in x:
                np.testing.assert_array_equal(x[key], y[key], err_msg="%s seed %d %s" % (flavour, seed, key))
    assert [M.describe(s) for s in M.walk(0, pool_n(flavour), flavour)] != [M.describe(s) for s in M.walk(1, pool_n(flavour), flavour)]


@pytest.mark.parametrize("flavour", M.FLAVOURS)
def test_every_kind_occurs(flavour):
    ops = [step["op"] for seed in SEEDS for step in played(flavour, seed)[0]]
    for kind in M.KINDS:
        assert ops.count(kind) >= 3, "%s: %s occurs %d times" % (flavour, kind, ops.count(kind))
    for kind in M.fail_kinds_of(M.FLAVOURS[flavour]):
        assert ops.count(kind) >= 1, "%s: %s never occurs" % (flavour, kind)


def test_every_failing_kind_occurs_in_every_way():
    seen = {(step["op"], step["via"]) for _, _, steps, _, _ in all_walks() for step in steps if step["op"] in M.FAIL_KINDS}
    want = {("fail_nan", "append"), ("fail_nan", "update"), ("fail_inf", "append"), ("fail_inf", "update"),
            ("fail_ord", "update_rows"), ("fail_ord", "update"), ("fail_ord", "remove_rows"),
            ("fail_code", "append_rows"), ("fail_code", "update_rows"), ("fail_sum", "append_rows"), ("fail_sum", "update_rows")}
    assert want <= seen, "never drawn: %s" % sorted(want - seen)
    # a refusal on an index that still has spare capacity, and one on an index a compaction has emptied
    slack = emptied_refusals = 0
    for _, _, _, run, _ in all_walks():
        emptied = False
        for step, before, cap, after in run:
            if step["op"] in M.FAIL_KINDS:
                slack += cap > M.tiles_of(len(before))
                emptied_refusals += emptied and len(before) == 0
            emptied = emptied or (len(before) > 0 and len(after) == 0)
    assert slack and emptied_refusals


def test_sizes_stay_inside_the_limit_and_steps_are_valid():
    for flavour, seed, steps, run, _ in all_walks():
        n_pool = pool_n(flavour)
        for step, before, cap, after in run:
            assert len(after) <= M.MAX_ROWS
            n = len(before)
            if step["op"] in M.FAIL_KINDS:
                np.testing.assert_array_equal(before, after)
                continue
            if "ords" in step:
                assert len(step["ords"]) == len(step["frm"]) and all(0 <= o < n for o in step["ords"])
            if step["op"] == "remove_rows":
                assert all(0 <= r < n for r in step["rows"])
            for key in ("frm",) + (("rows",) if step["op"] in APPENDS else ()):
                assert all(0 <= r < n_pool for r in step[key]) if key in step else True
            if step["op"] in ("append", "update"):   # a raw row never reproduces a row with an odd sum
                assert not np.isin(step["rows" if step["op"] == "append" else "frm"], M.FLAVOURS[flavour].odd_rows).any()
        if M.FLAVOURS[flavour].odd_rows:
            assert np.isin(steps[0]["rows"], M.FLAVOURS[flavour].odd_rows).any()


def test_the_sequences_that_carry_state_occur():
    seen = set()
    for flavour, seed, steps, run, _ in all_walks():
        emptied = False
        last = None           # the latest step that changed the rows: (step, src after)
        after_load = False    # a save_load with no change of the rows behind it yet
        for step, before, cap, after in run:
            op, n = step["op"], len(before)
            if op in APPENDS and len(step["rows"]):
                seen.add("append_in_place" if M.tiles_of(len(after)) <= cap else "append_reallocates")
                if len(after) == cap * M.TILE and cap > M.tiles_of(n):
                    seen.add("append_lands_on_capacity")
                if M.tiles_of(len(after)) > cap and len(after) == cap * M.TILE + 1 and n < cap * M.TILE:
                    seen.add("append_one_beyond_capacity")
                if emptied and n == 0:
                    seen.add("append_to_an_emptied_index")
                if emptied:
                    seen.add("append_after_passing_through_zero")
                if last is not None and last[0]["op"] in COMPACTIONS and len(last[1]) % M.TILE:
                    seen.add("append_after_compaction_left_a_partial_last_tile")
                if last is not None and last[0]["op"] in UPDATES and set(np.asarray(last[0]["ords"]) // M.TILE) & {(n - 1) // M.TILE} and n % M.TILE:
                    seen.add("append_into_a_last_tile_an_update_touched")
            if op in UPDATES and len(step["ords"]):
                if len(set(step["ords"].tolist())) < len(step["ords"]):
                    seen.add("update_with_a_duplicate_ord")
                if last is not None and last[0]["op"] in APPENDS and (step["ords"] < len(last[1]) - len(last[0]["rows"])).any() \
                        and (step["ords"] >= len(last[1]) - len(last[0]["rows"])).any():
                    seen.add("update_across_the_old_end_of_an_append")
                if cap > M.tiles_of(n):
                    seen.add("update_with_spare_capacity")
            if op in COMPACTIONS and len(after) != n:
                if len(after) == 0:
                    emptied = True
                if last is not None and last[0]["op"] in UPDATES:
                    removed = np.flatnonzero(~step["mask"]) if op == "compact" else np.unique(step["rows"])
                    if set(np.asarray(last[0]["ords"]) // M.TILE) & set(removed // M.TILE):
                        seen.add("compaction_after_an_update_of_the_same_tile")
                if cap > M.tiles_of(n):
                    seen.add("compaction_removes_spare_capacity")
            if op == "save_load":
                after_load = True
                if cap > M.tiles_of(n):
                    seen.add("save_with_spare_capacity")
            elif after_load and changes(step, before, after):
                seen.add("save_load_then_" + ("append" if op in APPENDS else "update" if op in UPDATES else "compaction"))
                after_load = False
            if op == "reserve" and M.tiles_of(step["rows"]) > cap:
                seen.add("reserve_grows")
            if changes(step, before, after):
                last = (step, after)
    want = {"append_in_place", "append_reallocates", "append_lands_on_capacity", "append_one_beyond_capacity", "append_to_an_emptied_index",
            "append_after_passing_through_zero", "append_after_compaction_left_a_partial_last_tile", "append_into_a_last_tile_an_update_touched",
            "update_with_a_duplicate_ord", "update_across_the_old_end_of_an_append", "update_with_spare_capacity",
            "compaction_after_an_update_of_the_same_tile", "compaction_removes_spare_capacity", "save_with_spare_capacity",
            "save_load_then_append", "save_load_then_update", "save_load_then_compaction", "reserve_grows"}
    assert want <= seen, "the default walks never reach: %s" % sorted(want - seen)


def test_every_walk_ends_with_duplicate_rows():
    for flavour, seed, _, _, m in all_walks():
        dup = m.size - len(np.unique(m.src))
        assert m.size > 0 and 10 * dup >= m.size, "%s seed %d ends with %d rows, %d of them duplicates" % (flavour, seed, m.size, dup)


def test_the_model_agrees_with_the_library_host_side():
    """IndexModel.compact against bbq_filter_kept_rows and IndexModel.update against bbq_update_winners, on every such step of the
    default walks"""
    compactions = updates = 0
    for flavour, seed, _, run, _ in all_walks():
        for step, before, _, after in run:
            n, msg = len(before), "%s seed %d %s" % (flavour, seed, M.describe(step))
            if step["op"] in COMPACTIONS:
                mask = step["mask"] if step["op"] == "compact" else ~np.isin(np.arange(n), step["rows"])
                kept = capi.kept_rows(mask)
                np.testing.assert_array_equal(after, before[kept], err_msg=msg)
                compactions += 1
            elif step["op"] in UPDATES:
                m = M.IndexModel(before, False)
                winners = m.update(step["ords"], step["frm"])
                np.testing.assert_array_equal(capi.update_winners(step["ords"], n), winners, err_msg=msg)
                want = before.copy()
                want[step["ords"][winners]] = step["frm"][winners]   # the winners alone, in any order, give the same rows
                np.testing.assert_array_equal(after, want, err_msg=msg)
                updates += 1
            elif step["op"] == "fail_ord":
                with pytest.raises(IndexError):
                    if step["via"] == "remove_rows":
                        M.IndexModel(before, False).remove(step["ords"])
                    else:
                        M.IndexModel(before, False).update(step["ords"], np.zeros(len(step["ords"]), np.int64))
                if step["via"] != "remove_rows":
                    with pytest.raises(capi.BBQError) as e:
                        capi.update_winners(step["ords"], n)
                    assert e.value.code == capi.ERR_INVALID_ARG
    assert compactions >= 6 * len(SEEDS) * 4 // 2 and updates >= 6 * len(SEEDS) * 4 // 2


def test_the_capacity_rules_on_the_figures_of_the_append_test():
    """the model on the figures tests/test_gpu_append.py::test_reserve_and_geometric_growth asserts of the library"""
    m = M.IndexModel(np.zeros(1000, np.int64), False)
    assert m.capacity == 1024
    m.reserve(500)
    assert m.capacity == 1024
    m.reserve(3000)
    assert m.capacity == 3008
    m.append(np.zeros(2008, np.int64))
    assert (m.size, m.capacity) == (3008, 3008)
    m.append(np.zeros(1, np.int64))
    assert (m.size, m.capacity) == (3009, 47 * 3 // 2 * 64)
    m.append(np.zeros(5000 - 3009, np.int64))
    assert (m.size, m.capacity) == (5000, 105 * 64)
    m.append(np.zeros(7000, np.int64))
    assert (m.size, m.capacity) == (12000, 188 * 64)
    m.compact(np.ones(12000, bool))
    assert m.capacity == 188 * 64          # every row kept: nothing changes, capacity included
    m.compact(np.arange(12000) < 65)
    assert (m.size, m.capacity) == (65, 128)
    m.reserve(1000)
    m.save_load()
    assert (m.size, m.capacity) == (65, 128)
    m.remove([64, 0, 64])
    assert (m.size, m.capacity) == (63, 64)
    m.compact(np.zeros(63, bool))
    assert (m.size, m.capacity) == (0, 0)
    m.append(np.zeros(1, np.int64))
    assert (m.size, m.capacity) == (1, 64)
