"""CPU: the model of MaxSim over chosen groups (tests/maxsim_groups_model.py) held to the MaxSim search's model where the two must
agree - a query whose candidates are all live groups, ascending - and the candidate lists of tests/test_gpu_maxsim_groups.py held to
what each is there to reach: a seed that stops reaching it fails here, without a device."""
import numpy as np
import pytest

import maxsim_groups_model as MG
import maxsim_model as M
import test_groups_cpu as GC
import test_spans_filtered_cpu as FC
from bbqlib import capi

N = 1300                                   # test_gpu_maxsim's index: three chunks of 512 rows, the last tile partial


def _scores(n, tokens, seed):
    """per token the f32 score of every row: seeded, with repeats (ties), a NaN and both zeros"""
    rng = np.random.default_rng(seed)
    s = rng.integers(-6, 7, (tokens, n)).astype(np.float32) / 4
    s[:, 77] = np.nan
    s[0, 5], s[0, 6] = 0.0, -0.0
    return s


def test_symbols_are_bound():
    assert {"bbq_score_maxsim_groups_batch", "bbq_search_maxsim_groups_batch"} <= set(capi.SYMBOLS)
    L = capi.lib()
    assert L.bbq_score_maxsim_groups_batch and L.bbq_search_maxsim_groups_batch
    assert hasattr(capi.Index, "score_maxsim_groups_batch") and hasattr(capi.Index, "search_maxsim_groups_batch")


@pytest.mark.parametrize("lname", ["singletons", "groups_of_65", "random_1_20", "empty_groups", "one_group"])
@pytest.mark.parametrize("mname", ["all", "random_half", "tile_out_and_ends"])
def test_all_live_groups_ascending_is_the_maxsim_search(lname, mname):
    off, mask = GC.layouts(N)[lname], FC.masks(N)[mname]
    for tokens, seed in ((1, 1), (3, 2), (33, 3)):
        s32 = _scores(N, tokens, seed)
        rep, live = M.rep_scores(s32, off, mask)
        for k in (0, 1, 3, 40, len(live), len(live) + 5):
            wg, ws, _, L = M.answer(s32, off, mask, k)
            gg, gs = MG.answer(rep, live, live, k)
            assert L == len(live)
            np.testing.assert_array_equal(gg, wg)
            assert np.asarray(gs, np.float32).tobytes() == np.asarray(ws, np.float32).tobytes()
        np.testing.assert_array_equal(MG.scores(rep, live, live).view(np.uint32), M.reduce(rep).view(np.uint32))
        assert MG.first_bad(off, mask, [live, live[::-1]]) is None


def test_the_model_on_a_small_case():
    off = np.array([0, 2, 2, 5, 6], np.int64)                      # groups: rows {0, 1}, none, {2, 3, 4}, {5}
    mask = np.array([1, 1, 1, 0, 1, 0], bool)                      # group 3's only row is rejected
    s32 = np.array([[1, 4, 9, 99, 2, 7], [3, 1, 1, 99, 8, 7]], np.float32)
    rep, live = M.rep_scores(s32, off, mask)
    assert live.tolist() == [0, 2]
    assert MG.scores(rep, live, [2, 0, 2]).tolist() == [17.0, 7.0, 17.0]          # 9 + 8, 4 + 3; the duplicate is scored again
    g, s = MG.answer(rep, live, [2, 0, 2], 2)
    assert g.tolist() == [2, 2] and s.tolist() == [17.0, 17.0]
    assert MG.answer(rep, live, [0], 5)[0].tolist() == [0] and len(MG.answer(rep, live, [], 5)[0]) == 0
    assert MG.first_bad(off, mask, [[0, 2], [2, 1]]) == (1, 1, 1)                 # an empty group
    assert MG.first_bad(off, mask, [[0, 3]]) == (0, 1, 3)                         # a group the filter empties
    assert MG.first_bad(off, mask, [[], [4]]) == (1, 0, 4) and MG.first_bad(off, mask, [[-1]]) == (0, 0, -1)
    assert MG.positions(off, [2, 0, 2]).tolist() == [0, 3, 5, 8]
    assert MG.cut_by(off, [2, 0, 2], 4) == [1] and MG.cut_by(off, [2, 0, 2], 8) == [] and MG.cut_by(off, [2, 0, 2], 3) == [2]


@pytest.mark.parametrize("lname", ["singletons", "random_1_20"])
@pytest.mark.parametrize("mname", ["all", "random_half"])
def test_the_lists_reach_the_boundaries(lname, mname):
    """exactly 64, 65, 256 and 257 expanded rows; a duplicate; a descending list"""
    off, mask = GC.layouts(N)[lname], FC.masks(N)[mname]
    _, live = M.rep_scores(_scores(N, 1, 4), off, mask)
    lists = MG.candidate_lists(off, live)
    assert set(lists) == {"ascending", "reversed", "random_dups", "one", "empty"} | {"total_%d" % t for t in MG.TOTALS}
    for t in MG.TOTALS:
        lst = lists["total_%d" % t]
        assert MG.positions(off, lst)[-1] == t and len(set(lst.tolist())) == len(lst)
    dups = lists["random_dups"]
    assert len(set(dups.tolist())) < len(dups) and max(np.bincount(dups)) >= 3
    assert (np.diff(lists["reversed"]) < 0).all() and (np.diff(lists["ascending"]) > 0).all()
    assert len(lists["one"]) == 1 and len(lists["empty"]) == 0
    assert all(MG.first_bad(off, mask, [l]) is None for l in lists.values())


def test_the_lists_reach_the_cuts():
    """a candidate cut by a wave's edge and one cut by a workgroup piece's edge, in lists the GPU test runs: random_1_20's ascending and
    reversed lists hold both, groups_of_65's every candidate but a few is cut by a wave's edge, and one_group is a single candidate of
    1 300 rows that every wave shares"""
    for lname, name in (("random_1_20", "ascending"), ("random_1_20", "reversed"), ("random_1_20", "random_dups"), ("groups_of_65", "ascending")):
        off = GC.layouts(N)[lname]
        live = np.arange(len(off) - 1)
        lst = MG.candidate_lists(off, live)[name]
        wave, piece = MG.cut_by(off, lst, MG.WAVE), MG.cut_by(off, lst, MG.PIECE)
        assert wave and piece and set(piece) <= set(wave), (lname, name)
        assert len(set(wave) - set(piece)) > 0                          # cut by a wave's edge inside a piece
    off = GC.layouts(N)["one_group"]
    assert MG.cut_by(off, [0], MG.PIECE) == [0] and MG.positions(off, [0])[-1] == N
    # a list that ends exactly on an edge cuts nothing there
    off = GC.layouts(N)["singletons"]
    assert MG.cut_by(off, np.arange(256), MG.WAVE) == []


def test_a_tie_makes_the_heap_order_differ_from_the_sorted_order():
    """the list the GPU test runs on test_gpu_maxsim's tie case - groups 2 and 4 score the same sums - in an order whose heap answer is
    not the stable sort's"""
    off = np.array([0, 64, 200, 210, 700, 710, N], np.int64)
    s32 = _scores(N, 3, 5)
    s32[:, 700:710] = s32[:, 200:210]
    rep, live = M.rep_scores(s32, off, np.ones(N, bool))
    S = M.reduce(rep)
    assert S[2].tobytes() == S[4].tobytes()
    differs = 0
    for lst, k in TIE_LISTS:
        hg, hs = MG.answer(rep, live, lst, k)
        sg, ss = MG.sorted_answer(rep, live, lst, k)
        assert sorted(canon(hs)) == sorted(canon(ss))
        differs += hg.tolist() != sg.tolist()
    assert differs > 0


TIE_LISTS = (([4, 2, 0, 1, 3, 5], 6), ([2, 4, 0, 1, 3, 5], 6), ([0, 4, 1, 2, 5, 3], 3), ([5, 4, 3, 2, 1, 0], 2), ([4, 0, 2], 3), ([2, 0, 4, 4, 2], 4))


def canon(s):
    return np.asarray(s, np.float32).view(np.uint32).tolist()
