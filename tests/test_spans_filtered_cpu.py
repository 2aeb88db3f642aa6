"""CPU: the filtered span search's contract restated in numpy - bbq_search_spans_filtered_batch's out_status is the span search's rule
over the ACCEPTED visited rows - and, from the goldens alone, a check that the masks, span sets and k values tests/test_gpu_spans_filtered.py
runs exercise both paths: per mask the device's selection for at least half of the cases, at least one replay because of equal scores, and
10 000 cases in all."""
import functools

import numpy as np
import pytest

import test_gpu_score_ords as SO          # FIXTURES: the names alone (nothing here touches a device)
import test_spans_cpu as SC               # expand, span_sets, expected_status: shared with the unfiltered checks

MASKS = ("all", "none", "drop_every_third", "random_half", "tile_out_and_ends", "sparse_61")


@functools.lru_cache(maxsize=None)
def masks(n):
    """the row masks of an index of n rows, by name; read-only"""
    rng = np.random.default_rng(1234 + n)
    m = {"all": np.ones(n, bool), "none": np.zeros(n, bool)}
    m["drop_every_third"] = np.ones(n, bool)
    m["drop_every_third"][1::3] = False
    m["random_half"] = rng.random(n) < 0.5                    # the generator's first draw
    t = np.ones(n, bool)
    t[64:128] = False
    t[0] = False
    t[n - 1] = False
    m["tile_out_and_ends"] = t
    m["sparse_61"] = np.zeros(n, bool)
    m["sparse_61"][::61] = True
    assert tuple(m) == MASKS
    for a in m.values():
        a.setflags(write=False)
    return m


def accepted(mask, spans):
    """the rows a filtered span list visits, in visiting order"""
    rows = SC.expand(spans)
    return rows[mask[rows]]


def k_values(mask, sets):
    """one call per k: {0, 1, 3, 10, A - 1, A, A + 5} for the accepted count A of every span set"""
    ks = {0, 1, 3, 10}
    for s in sets:
        A = len(accepted(mask, s))
        ks |= {A - 1, A, A + 5}
    return sorted(k for k in ks if k >= 0)


def expected_status(scores, mask, spans, k):
    """the rule: the span search's over the scores of the accepted visited rows; a rejected row's score is never looked at"""
    return SC.expected_status(np.asarray(scores, np.float32)[accepted(mask, spans)], k)


def test_the_rule_on_small_cases():
    nan = np.nan
    s = np.array([5, nan, 4, 3, 3, 1], np.float32)
    everything = [(0, 6)]
    keep = np.array([1, 0, 1, 1, 0, 1], bool)                  # the NaN and one of the equal scores are rejected
    assert expected_status(s, keep, everything, 1) == 0 and expected_status(s, keep, everything, 3) == 0
    assert expected_status(s, keep, everything, 4) == 1        # A == k
    assert expected_status(s, np.ones(6, bool), everything, 1) == 1                                    # the NaN is accepted
    assert expected_status(s, np.array([1, 0, 1, 1, 1, 1], bool), everything, 2) == 0                  # 5, 4 | 3: no tie among the k + 1 largest
    assert expected_status(s, np.array([1, 0, 1, 1, 1, 1], bool), everything, 3) == 1                  # 5, 4, 3 | 3
    assert expected_status(s, keep, [(1, 2)], 1) == 0 and len(accepted(keep, [(1, 2)])) == 0           # nothing accepted: nothing to answer
    assert expected_status(s, keep, [(0, 1), (2, 4)], 2) == 0 and expected_status(s, keep, [(0, 1), (2, 4)], 0) == 0
    assert expected_status(s, np.zeros(6, bool), everything, 3) == 0
    np.testing.assert_array_equal(accepted(keep, [(0, 2), (3, 6)]), [0, 3, 5])
    big = np.arange(2 * SC.SELECT_MAX + 20, dtype=np.float32)
    half = np.zeros(len(big), bool)
    half[::2] = True                                           # 4106 accepted rows
    assert expected_status(big, half, [(0, len(big))], SC.SELECT_MAX) == 0 and expected_status(big, half, [(0, len(big))], SC.SELECT_MAX + 1) == 1


def test_the_masks():
    for n in (1, 2, 12, 100, 1000):
        m = masks(n)
        assert m["all"].all() and not m["none"].any()
        assert m["sparse_61"].sum() == (n + 60) // 61 and m["sparse_61"][0]
        assert not m["tile_out_and_ends"][0] and not m["tile_out_and_ends"][n - 1] and not m["tile_out_and_ends"][64:128].any()
        assert m["drop_every_third"].sum() == n - len(range(1, n, 3))
        assert all(len(a) == n for a in m.values())
    assert 400 < masks(1000)["random_half"].sum() < 600
    assert (masks(1000)["random_half"] == (np.random.default_rng(2234).random(1000) < 0.5)).all()


def test_the_golden_inputs_exercise_both_paths():
    """per mask, of the (fixture, query, span set, k) cases of the golden GPU test with A > k >= 1: how many the device answers and how
    many the host replays because of equal scores"""
    count = {name: [0, 0, 0] for name in MASKS}               # cases, device-selected, tie replays
    for fx in SO.FIXTURES:
        n, scores = SC.golden_scores(fx)
        sets = SC.span_sets(n)
        for name, mask in masks(n).items():
            ks = k_values(mask, sets)
            for s32 in scores:
                for sp in sets:
                    v = s32[accepted(mask, sp)]
                    for k in ks:
                        if len(v) > k >= 1:
                            count[name][0] += 1
                            count[name][1] += SC.expected_status(v, k) == 0
                            count[name][2] += bool(SC.tie_is_the_reason(v, k))
    print(count)
    assert count["none"] == [0, 0, 0]
    for name in MASKS:
        if name != "none":
            total, by_device, ties = count[name]
            assert 2 * by_device >= total > 0, "%s: %d of %d cases have expected status 0" % (name, by_device, total)
            assert ties >= 1, "%s: no replay because of equal scores" % name
    assert sum(c[0] for c in count.values()) >= 10000
