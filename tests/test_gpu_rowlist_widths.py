"""GPU: the row-list entry points at every compiled width - bbq_score_ords, bbq_score_ords_batch, bbq_search_ords_batch,
bbq_count_range_batch, bbq_search_range_batch, bbq_search_spans_batch, bbq_search_spans_filtered_batch, bbq_search_grouped_batch and
bbq_search_maxsim_batch (unfused and fused) - over the matrix of tests/rowlist_cells.py, bit for bit against the CPU oracle's scores of
the product's own quantization and the numpy models the entry points' own tests use.  No tolerance anywhere.

One test per (cell, variant).  A cell fixes (store_bits, planes or QB, W) - rowlist_cells.compiled, which tests/test_rowlist_cells_cpu.py
holds to the launchers' switch arms - and the test asserts the plane count of the query values it sends and the layout of the index it
made; the variant fixes the rest of what selects a kernel: the corrections layout and, in the compact layout, whether the launch's view
carries the row_sums side array (default options: the arm that reads it; row_sums 0, and resident_mb 0 with an automatic row_sums: the
arm that counts).  Every call runs without a filter and under one.

A BBQ_ERR_HIP from any call ends the whole pytest session (test_gpu_mutation_walk.located): nothing more is started on a device that has
failed, not even the close of the handles."""
import contextlib
import functools

import numpy as np
import pytest

import orclib as O
import maxsim_model as M
import rowlist_cells as C
import test_spans_cpu as SC
import test_spans_filtered_cpu as FC
import test_groups_cpu as GC
import test_gpu_score_ords as SO
import test_gpu_range as GR
import test_gpu_spans as GS
import test_gpu_spans_filtered as GSF
import test_gpu_grouped as GG
import test_gpu_maxsim as GM
import test_gpu_mutation_walk as MW
from test_gpu_score_ords import canon32
from bbqlib import bbq_amd as B, capi

pytestmark = pytest.mark.gpu

VARIANTS = ("compact", "compact_row_sums_0", "compact_resident_mb_0", "inline")
OPTIONS = {"compact_row_sums_0": ("row_sums", 0), "compact_resident_mb_0": ("resident_mb", 0)}
DEFAULTS = (("row_sums", -1), ("resident_mb", -1), ("maxsim_fused", -1))
CASES = [(c, v) for c in C.CELLS for v in VARIANTS if v != "compact_resident_mb_0" or c in C.one_cell_per_w()]

_held = {}                 # the one index that is open: {(cell, layout): Index}, made once per (cell, layout) and shared by the cell's variants
_device_failed = []        # not empty: a call returned BBQ_ERR_HIP
_seen = {}                 # {W class: {variant: the span and group statuses seen}}


def _close_held():
    if not _device_failed:         # after a device failure the handles are neither closed nor dropped
        for ix in _held.values():
            ix.close()
        _held.clear()


def _index(cell, layout):
    if (cell, layout) not in _held:
        _close_held()
        codes, corr, cdp = C.case(cell)[:3]
        _held[cell, layout] = B.Index(codes, corr, cell.dim, cdp, index_bits=cell.index_bits, corrections=layout)
    return _held[cell, layout]


@pytest.fixture(scope="module", autouse=True)
def _close_the_last_index():
    yield
    _close_held()


@contextlib.contextmanager
def located(msg):
    try:
        with MW.located(msg):
            yield
    except pytest.exit.Exception:
        _device_failed.append(msg)
        raise


@functools.lru_cache(maxsize=None)
def _reps(cell, lname, filtered):
    """the MaxSim model's representative scores [tokens, L] and live groups of one (cell, layout, mask): once, read-only"""
    rep, live = M.rep_scores([s[2] for s in C.case(cell)[5]], C.group_layouts()[lname], C.accept_mask() if filtered else FC.masks(C.N)["all"])
    rep.setflags(write=False)
    return rep, live


def _check_ords(ix, cell, qq, qc, scores, mask, msg):
    qb, sim = cell.query_bits, cell.sim
    everything = C.ord_list()
    for ords in (everything, everything[mask[everything]]):                 # the list, and what a filter leaves of it
        SO._assert_entries(ix.score_ords(qq[0], qc[0], qb, sim, ords), scores[0], ords, msg + " score_ords")
        lists = [ords, ords[::-1].copy(), np.concatenate([ords, ords])]
        d, s64, s32, off = ix.score_ords_batch(qq[:3], qc[:3], qb, sim, lists)
        np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum([len(l) for l in lists])]))
        for q, l in enumerate(lists):
            sl = slice(off[q], off[q + 1])
            SO._assert_entries((d[sl], s64[sl], s32[sl]), scores[q], l, "%s score_ords_batch query %d" % (msg, q))
        for k in (1, 10, len(lists[2]) + 1):
            res = ix.search_ords_batch(qq[:3], qc[:3], qb, sim, k, lists)
            for q, l in enumerate(lists):
                oi, osc = O.heap_topk(scores[q][2][l], k)
                np.testing.assert_array_equal(res[q][0], l[oi], err_msg="%s search_ords_batch query %d k=%d" % (msg, q, k))
                np.testing.assert_array_equal(canon32(res[q][1]), canon32(osc), err_msg="%s search_ords_batch query %d k=%d: score bits" % (msg, q, k))


def _check_range(ix, cell, qq, qc, scores, flt, mask, msg):
    who = [q for q in range(C.N_SINGLE) for _ in range(4)]
    ths = np.concatenate([C.thresholds_of(scores[q][2]) for q in range(C.N_SINGLE)])
    gold = [scores[q][2] for q in who]
    for f, m in ((None, None), (flt, mask)):
        want = GR.assert_range(ix, qq[who], qc[who], cell.query_bits, cell.sim, ths, gold, msg + (" range" if f is None else " filtered range"), f, m)
        for q in range(C.N_SINGLE):
            everything, third, median, above = want[4 * q:4 * q + 4]
            assert len(everything) == (C.N if m is None else m.sum()) and len(above) == 0 and 0 < len(third) <= len(median) < len(everything)


def _check_spans(ix, cell, qq, qc, scores, flt, mask, msg):
    qb, sim = cell.query_bits, cell.sim
    qqs, qcs, lists, who = GS._pairs([(qq[q], qc[q]) for q in range(C.N_SINGLE)], C.span_lists())
    s32 = [scores[w][2] for w in who]
    everything = FC.masks(C.N)["all"]
    seen = set()
    for f, m in ((None, everything), (flt, mask)):
        ks = sorted(set(C.SPAN_KS) | {len(FC.accepted(m, sp)) + 1 for sp in C.span_lists() if len(FC.accepted(m, sp))})
        for k in ks:
            if f is None:
                seen |= set(GS.assert_spans(ix, qqs, qcs, qb, sim, k, lists, s32, msg + " spans").tolist())
            res, status = GSF.assert_filtered(ix, f, m, qqs, qcs, qb, sim, k, lists, s32, msg + (" filtered spans" if f else " spans through the filtered entry"))
            seen |= set(status.tolist())
            assert all(len(r[0]) == 0 and st == 0 for r, st, sp in zip(res, status, lists) if len(SC.expand(sp)) == 0)    # the empty span
    return seen


def _check_groups_and_maxsim(ix, cell, qq, qc, scores, mask, msg):
    qb, sim = cell.query_bits, cell.sim
    tb = capi.maxsim_token_block()
    assert tb + 1 <= C.N_QUERIES
    tokens = [(0, 1), (1, 3), (0, tb + 1)]                                  # queries of 1, 2 and token_block + 1 token vectors
    s32 = [scores[q][2] for q in range(C.N_SINGLE)]
    seen = set()
    for lname, off in C.group_layouts().items():
        for filtered, m in ((False, FC.masks(C.N)["all"]), (True, mask)):
            where = "%s %s%s" % (msg, lname, " filtered" if filtered else "")
            with GM._open(ix, off, m) as groups:
                assert groups.count == len(off) - 1 and groups.live == GC.plan(off, m)[1]
                for k in C.GROUP_KS + (groups.live + 1,):
                    _, status = GG.assert_grouped(ix, groups, off, m, qq[:C.N_SINGLE], qc[:C.N_SINGLE], qb, sim, k, s32, where + " grouped")
                    seen |= set(status.tolist())
                rep, live = _reps(cell, lname, filtered)
                for k in C.GROUP_KS:                                          # both values of maxsim_fused, byte-identical answers
                    GM.assert_maxsim(ix, groups, rep, live, qq, qc, tokens, qb, sim, k, where + " maxsim")
    return seen


@pytest.mark.parametrize("cell,variant", CASES, ids=["%s-%s" % (C.cell_id(c), v) for c, v in CASES])
def test_cell(cell, variant):
    layout = "inline" if variant == "inline" else "compact"
    sb, planes, w = C.compiled(cell)
    codes, corr, cdp, qq, qc, scores = C.case(cell)
    mask = C.accept_mask()
    msg = "%s %s <%d, %d, %d>" % (C.cell_id(cell), variant, sb, planes, w)
    # what selects the kernel, as far as the inputs decide it: the planes of the values sent, the row width, the layout
    assert all(C.planes_of_values(cell.index_bits, cell.query_bits, q) == planes for q in qq)
    w16 = C.w16_of(cell.index_bits, cell.dim)
    assert w == (w16 if w16 in (C.ONE_BIT_W if sb == 1 else C.MULTI_BIT_W if sb < 8 else ()) else 0)
    ix = _index(cell, layout)
    try:
        with located(msg):
            assert ix.bytes_per_row == 16 * w16 + (4 if layout == "compact" else 24)      # compact: 4 bytes of corrections per row; inline: 24
            if variant in OPTIONS:
                ix.set_option(*OPTIONS[variant])
            with capi.Filter(ix, mask) as flt:
                assert flt.count == mask.sum()
                _check_ords(ix, cell, qq, qc, scores, mask, msg)
                _check_range(ix, cell, qq, qc, scores, flt, mask, msg)
                seen = _check_spans(ix, cell, qq, qc, scores, flt, mask, msg)
            seen |= _check_groups_and_maxsim(ix, cell, qq, qc, scores, mask, msg)
            assert 1 in seen                                               # the ties sent a query to the heap
            _seen.setdefault(C.w_class(cell), {}).setdefault(variant, []).append(seen)
    finally:
        for name, value in DEFAULTS:                                       # (host state only: safe after a device failure too)
            ix.set_option(name, value)


def test_both_statuses_were_seen_in_every_w_class():
    """over the cells of a W class that ran, per variant: the device selected an answer and the host replayed one.  (A class none of
    whose cells ran in this session - a -k selection - has nothing to say.)"""
    for cls, by_variant in _seen.items():
        for variant, sets in by_variant.items():
            want = sum(1 for c, v in CASES if C.w_class(c) == cls and v == variant)
            if len(sets) == want:
                assert set().union(*sets) == {0, 1}, "%s %s" % (cls, variant)
