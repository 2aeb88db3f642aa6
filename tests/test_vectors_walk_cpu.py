"""CPU: the walk over the fp32 row store itself (tests/vectors_walk.py), with no device.  What the DEFAULT walks - every width, the
default seeds, the walks tests/test_gpu_vectors_walk.py plays on the device - cover is asserted here, width by width: every operation,
both kinds of append, the sequences in which one mutation can be wrong only because another came before it, every mask shape, every
column through the exact search.  These are conditions, not measurements: when a change to the walk breaks one, the walk's seeds or
deck change, never the assertion.  The model's update rule is held to the library's host-only bbq_update_winners and its compaction to
bbq_filter_kept_rows.  And the identity the device test reads rows back by is anchored to the ORACLE here: under MAXIMUM_INNER_PRODUCT
the score of a one-hot query e_j against a finite row is float64(row[j]) + 0.0, bit for bit."""
import functools

import numpy as np
import pytest

import orclib as O
import vectors_walk as W
from bbqlib import capi

SEEDS = tuple(range(W.DEFAULT_SEEDS))


@functools.lru_cache(maxsize=None)
def played(seed, dim):
    """the walk's steps with the model's state around each: [(step, src before, capacity before, src after, capacity after)]"""
    steps = W.walk(seed, dim)
    assert steps[0]["op"] == "create"
    m = W.VectorsModel(steps[0]["rows"])
    out = []
    for step in steps[1:]:
        before, cap = m.src.copy(), m.cap
        W.apply(m, step)
        out.append((step, before, cap, m.src.copy(), m.cap))
    return steps, out, m


def test_the_widths_sit_on_both_sides_of_every_path():
    w = W.WIDTHS
    assert any(d % 4 == 0 for d in w) and any(d % 4 for d in w) and min(w) < 4            # the 16-byte and the 4-byte copy
    assert {63, 65} <= set(w) and any(d > 128 and d % 4 for d in w)                        # one, two and three trips of 64 x 4 bytes
    assert {256, 260} <= set(w) and any(d > 512 and d % 4 == 0 for d in w)                 # one, two and three trips of 64 x 16 bytes
    assert any(d < 32 for d in w) and any(32 < d < 64 for d in w) and any(d > 64 for d in w)   # the readers' 32-column stage


def test_the_pool_holds_the_hostile_rows():
    for dim in W.WIDTHS:
        p = W.pool(dim)
        assert p.dtype == np.float32 and p.shape == (W.N_NORMAL + len(W.HOSTILE), dim) and not p.flags.writeable
        assert np.isfinite(p).all()
        sub = p[W.hostile_row("subnormal")]
        assert (sub != 0).all() and (np.abs(sub) < np.finfo(np.float32).tiny).all() and np.float32(2.0 ** -149) in sub
        ext = np.abs(p[W.hostile_row("extreme")])
        assert np.finfo(np.float32).tiny in ext and (dim < 2 or np.finfo(np.float32).max in ext) and (dim < 4 or ((ext > 1e-3) & (ext < 10)).any())
        assert not p[W.hostile_row("zero")].any() and not np.signbit(p[W.hostile_row("zero")]).any()
        assert not p[W.hostile_row("negative_zero")].any() and np.signbit(p[W.hostile_row("negative_zero")]).all()
        last = p[W.hostile_row("last_column")]
        assert last[dim - 1] != 0 and not last[:dim - 1].any()
        for name in ("duplicate_a", "duplicate_b", "duplicate_c"):
            assert p[W.hostile_row(name)].tobytes() == p[W.DUPLICATED].tobytes()
        assert W.pool(dim).tobytes() == p.tobytes()


@pytest.mark.parametrize("dim", W.WIDTHS)
def test_the_same_seed_gives_the_same_steps(dim):
    for seed in SEEDS:
        a, b = W.walk(seed, dim), W.walk(seed, dim)
        assert len(a) == len(b) and 20 <= len(a) <= 36, len(a)
        for x, y in zip(a, b):
            assert x.keys() == y.keys()
            for key in x:
                np.testing.assert_array_equal(x[key], y[key], err_msg="dim %d seed %d %s" % (dim, seed, key))
    assert [W.describe(s) for s in W.walk(0, dim)] != [W.describe(s) for s in W.walk(1, dim)]


@pytest.mark.parametrize("dim", W.WIDTHS)
def test_steps_are_valid_and_sizes_stay_inside_the_limit(dim):
    n_pool = W.pool(dim).shape[0]
    for seed in SEEDS:
        steps, run, m = played(seed, dim)
        assert m.size >= 200
        emptied = False
        for step, before, cap, after, cap_after in run:
            n = len(before)
            assert len(after) <= W.MAX_ROWS and cap_after >= len(after)
            for key in ("rows", "frm"):
                assert all(0 <= r < n_pool for r in step.get(key, ()))
            if step["op"] in W.REFUSALS:
                np.testing.assert_array_equal(before, after)
                assert cap_after == cap
            if step["op"] == "update":
                assert len(step["ords"]) == len(step["frm"]) and all(0 <= o < n for o in step["ords"])
            if step["op"] == "refuse_update":
                assert step["ords"][step["bad"][0]] in (-1, n)
            if step["op"] == "refuse_compact":
                assert step["bad"][0] >= 1 and step["bad"][0] != n
            if step["op"] == "refuse_append":
                assert step["bad"][0] != dim and len(step["rows"]) > 0
            if step["op"] == "compact":
                assert step["mask"].shape == (n,) and n > 0
                if step["mask"].all():
                    assert cap_after == cap
                else:
                    assert cap_after == len(after) == int(step["mask"].sum())
            if step["op"] == "append" and len(step["rows"]) and emptied and n == 0:
                emptied = False
            if step["op"] == "compact" and len(after) == 0:
                emptied = True
        assert not emptied, "keep_none is not followed by an append"


@pytest.mark.parametrize("dim", W.WIDTHS)
def test_what_the_default_walks_of_a_width_cover(dim):
    seen, shapes, padding = set(), set(), set()
    for seed in SEEDS:
        steps, run, _ = played(seed, dim)
        seen.add("create_%s" % ("empty" if len(steps[0]["rows"]) == 0 else "rows"))
        emptied_by_keep_none, previous = False, None
        for step, before, cap, after, cap_after in run:
            op, n = step["op"], len(before)
            seen.add(op)
            if op == "append":
                cnt = len(step["rows"])
                seen.add("append_%d" % cnt if cnt < 2 else "append_many")
                if cnt:
                    seen.add("append_reallocates" if n + cnt > cap else "append_in_place")
                    if n + cnt == cap and cap > n:
                        seen.add("append_fits_the_capacity_exactly")
                    if n + cnt > cap and cap > 0 and n + cnt < cap * 3 // 2:
                        seen.add("append_grows_by_half")
                    if n + cnt > cap * 3 // 2 and cap > 0:
                        seen.add("append_grows_to_what_is_needed")
                    if n == 0 and emptied_by_keep_none:
                        seen.add("append_on_an_emptied_handle")
                    if n == 0:
                        emptied_by_keep_none = False
            if op == "update" and len(step["ords"]):
                if len(set(step["ords"].tolist())) < len(step["ords"]):
                    seen.add("update_with_a_duplicate_ord")
                if previous is not None and previous[0]["op"] == "compact" and not previous[0]["mask"].all():
                    seen.add("update_directly_after_a_compaction")
                    assert cap == n, "the buffer holds exactly the kept rows"
                if cap > n:
                    seen.add("update_with_spare_capacity")
            if op == "update" and not len(step["ords"]):
                seen.add("update_of_nothing")
            if op == "compact":
                shapes.add(step["shape"])
                if n % W.TILE:
                    padding.add(step["padding"])
                if step["shape"] == "keep_none":
                    emptied_by_keep_none = True
                if step["shape"] == "first_tile_out":
                    assert not step["mask"][:W.TILE].any() and step["mask"][W.TILE:].all()
                if step["shape"] == "middle_tiles_out":
                    out_tiles = np.flatnonzero(~step["mask"].reshape(-1)[:n // W.TILE * W.TILE].reshape(-1, W.TILE).any(axis=1))
                    assert len(out_tiles) >= 3 and out_tiles[0] > 0 and (np.diff(out_tiles) == 1).all() and step["mask"][(out_tiles[-1] + 1) * W.TILE:].all()
                if step["shape"] == "only_last_row":
                    assert step["mask"].sum() == 1 and step["mask"][-1]
                if step["shape"] == "drop_row_0":
                    assert step["mask"].sum() == n - 1 and not step["mask"][0]
                if step["shape"] == "alternating":
                    assert (step["mask"] == (np.arange(n) % 2 == 1)).all()
                if cap > n:
                    seen.add("compaction_removes_spare_capacity")
            if op == "refuse_update":
                seen.add("refuse_update_ord_%s" % ("minus_1" if step["ords"][step["bad"][0]] == -1 else "n"))
            for mult in (64, 256):
                if len(after) // mult > n // mult:
                    seen.add("up_across_%d" % mult)
                if len(after) // mult < n // mult:
                    seen.add("down_across_%d" % mult)
            previous = (step, after)
    want = {"append", "update", "compact", "refuse_update", "refuse_compact", "refuse_append", "append_0", "append_1", "append_many",
            "append_reallocates", "append_in_place", "append_fits_the_capacity_exactly", "append_grows_by_half", "append_grows_to_what_is_needed",
            "append_on_an_emptied_handle", "update_with_a_duplicate_ord", "update_directly_after_a_compaction", "update_with_spare_capacity",
            "update_of_nothing", "compaction_removes_spare_capacity", "refuse_update_ord_minus_1", "refuse_update_ord_n",
            "up_across_64", "down_across_64", "up_across_256", "down_across_256"}
    assert want <= seen, "dim %d: the default walks never reach: %s" % (dim, sorted(want - seen))
    assert set(W.MASK_SHAPES) <= shapes, "dim %d: never drawn: %s" % (dim, sorted(set(W.MASK_SHAPES) - shapes))
    assert padding == {0, 1}, "dim %d: the padding bits of a partial last accept word are only ever %s" % (dim, sorted(padding))


def test_an_empty_creation_occurs():
    assert any(len(played(seed, dim)[0][0]["rows"]) == 0 for dim in W.WIDTHS for seed in SEEDS)


@pytest.mark.parametrize("dim", W.WIDTHS)
def test_the_exact_search_reads_every_column_back(dim):
    covered = set()
    for seed in SEEDS:
        steps = played(seed, dim)[0]
        for i in range(len(steps)):
            cols = W.exact_columns(seed, i, dim)
            assert len(cols) <= W.EXACT_COLUMNS and len(set(cols.tolist())) == len(cols) and 0 in cols and dim - 1 in cols
            assert cols.min() >= 0 and cols.max() < dim
            covered |= set(cols.tolist())
    assert covered == set(range(dim))


def test_the_model_agrees_with_the_library_host_side():
    """VectorsModel.update against bbq_update_winners and VectorsModel.compact against bbq_filter_kept_rows, on every such step of the
    default walks; a refused update is refused by both"""
    updates = compactions = refused = 0
    for dim in W.WIDTHS:
        for seed in SEEDS:
            for step, before, _, after, _ in played(seed, dim)[1]:
                n, msg = len(before), "dim %d seed %d %s" % (dim, seed, W.describe(step))
                if step["op"] == "update":
                    winners = W.VectorsModel(before).update(step["ords"], step["frm"])
                    np.testing.assert_array_equal(capi.update_winners(step["ords"], n), winners, err_msg=msg)
                    want = before.copy()
                    want[step["ords"][winners]] = step["frm"][winners]   # the winners alone, in any order, give the same rows
                    np.testing.assert_array_equal(after, want, err_msg=msg)
                    updates += 1
                elif step["op"] == "compact":
                    np.testing.assert_array_equal(after, before[capi.kept_rows(step["mask"])], err_msg=msg)
                    compactions += 1
                elif step["op"] == "refuse_update":
                    with pytest.raises(IndexError):
                        W.VectorsModel(before).update(step["ords"], step["frm"])
                    with pytest.raises(capi.BBQError) as e:
                        capi.update_winners(step["ords"], n)
                    assert e.value.code == capi.ERR_INVALID_ARG, msg
                    refused += 1
    assert updates >= 4 * len(W.WIDTHS) * len(SEEDS) and compactions >= W.MASKS_PER_WALK * len(W.WIDTHS) * len(SEEDS) and refused == len(W.WIDTHS) * len(SEEDS)


def test_the_capacity_rule_on_figures():
    m = W.VectorsModel(np.zeros(0, np.int64))
    assert (m.size, m.cap) == (0, 0)
    m.append(np.zeros(0, np.int64))
    assert (m.size, m.cap) == (0, 0)
    m.append(np.zeros(1, np.int64))
    assert (m.size, m.cap) == (1, 1)          # 1 * 3 / 2 is 1
    m.append(np.zeros(1, np.int64))
    assert (m.size, m.cap) == (2, 2)
    m.append(np.zeros(1, np.int64))
    assert (m.size, m.cap) == (3, 3)          # 2 * 3 / 2 is 3
    m.append(np.zeros(997, np.int64))
    assert (m.size, m.cap) == (1000, 1000)
    m.append(np.zeros(1, np.int64))
    assert (m.size, m.cap) == (1001, 1500)
    m.append(np.zeros(499, np.int64))
    assert (m.size, m.cap) == (1500, 1500)    # exactly on the capacity
    m.compact(np.ones(1500, bool))
    assert (m.size, m.cap) == (1500, 1500)
    m.append(np.zeros(1, np.int64))
    assert (m.size, m.cap) == (1501, 2250)
    m.compact(np.ones(1501, bool))
    assert (m.size, m.cap) == (1501, 2250)    # every row kept: nothing changes, the capacity included
    m.compact(np.arange(1501) < 65)
    assert (m.size, m.cap) == (65, 65)
    m.compact(np.zeros(65, bool))
    assert (m.size, m.cap) == (0, 0)
    m.append(np.zeros(7, np.int64))
    assert (m.size, m.cap) == (7, 7)


@pytest.mark.parametrize("dim", [5, 33])
def test_the_read_back_identity_holds_for_the_oracle(dim):
    """computeSimilarity(e_j, row) under MAXIMUM_INNER_PRODUCT is float64(row[j]) + 0.0 for every finite row, subnormals, -0.0 and
    +-FLT_MAX included: every other product is a zero of either sign, the chain starts at +0.0, and +0.0 + -0.0 is +0.0"""
    p = W.pool(dim)
    got = O.true_similarity(np.eye(dim, dtype=np.float32), p, O.SIMS["MAXIMUM_INNER_PRODUCT"])
    want = np.ascontiguousarray(p.T.astype(np.float64) + 0.0)
    assert not np.signbit(want[:, W.hostile_row("negative_zero")]).any()
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    assert not len(bad), "pool row %d, column %d: the oracle gives %r, the row holds %r" % (bad[0][1], bad[0][0], got[tuple(bad[0])], p[bad[0][1], bad[0][0]])
    assert (want[:, W.hostile_row("subnormal")] != 0).all()
