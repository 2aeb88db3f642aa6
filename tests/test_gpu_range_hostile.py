"""GPU: range search - bbq_count_range_batch, bbq_search_range_batch - over the hostile recipe of tests/range_hostile.py: tiles of
ordinary, hostile and mixed rows, tiles whose additive range is NaN or infinite, queries outside the f32 images beside ordinary ones in
one launch, and a threshold table of edge floats and the query's own scores.  In the compact layout the score bound decides the answer
with nothing behind it, so a row it wrongly rejects is missing.  Bit-exact, no tolerance: counts, offsets, ascending ords and f32 score
bits equal range_answer over the oracle's f32 scores; no NaN-scored row in any answer; fast_bound 0 (the f64 form of the bound) and
fast_bound 1 give identical bytes; the inline layout, which scores every row, gives the compact layout's ords.
tests/test_range_hostile_cpu.py shows from the bound's numpy model that these inputs reach the bound, and how often.

A BBQ_ERR_HIP from any call ends the whole pytest session (test_gpu_mutation_walk.located): nothing more is started on a device that has
failed, not even the close of the handles."""
import contextlib

import numpy as np
import pytest

import range_hostile as H
import test_gpu_mutation_walk as MW
from rowlist_cells import w16_of
from test_gpu_range import bits
from test_range_key_cpu import range_answer
from bbqlib import bbq_amd as B, capi

pytestmark = pytest.mark.gpu

LAYOUTS = ("compact", "inline")
MAIN = H.BY_NAME["main"]
CASES = [(f, s) for f in H.FAMILIES[1:] + (MAIN,) for s in H.SIMS]      # the main family last: the tests below go on with its indexes
IDS = ["%s-%s" % (f.name, ("euc", "cos", "mip")[s]) for f, s in CASES]

_held = {}                 # the indexes that are open: {(family, layout): Index} of ONE family, made once per (family, layout)
_device_failed = []        # not empty: a call returned BBQ_ERR_HIP


def _close_held():
    if not _device_failed:         # after a device failure the handles are neither closed nor dropped
        for ix in _held.values():
            ix.close()
        _held.clear()


def _make(fam, layout, codes, corr):
    ix = B.Index(codes, corr, fam.dim, H.CDP, index_bits=fam.index_bits, corrections=layout)
    assert ix.bytes_per_row == 16 * w16_of(fam.index_bits, fam.dim) + (4 if layout == "compact" else 24)      # the layout asked for
    return ix


def _index(fam, layout):
    if (fam, layout) not in _held:
        if any(f != fam for f, _ in _held):
            _close_held()
        _held[fam, layout] = _make(fam, layout, *H.rows(fam))
    return _held[fam, layout]


@pytest.fixture(scope="module", autouse=True)
def _close_the_last_indexes():
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


def answer(ix, fam, sim, qqs, qcs, ths, gold, msg, flt=None, mask=None):
    """one search and one count call for all the pairs, held to range_answer over the oracle's f32 scores (test_gpu_range.assert_range's
    assertions); returns the bytes the calls delivered"""
    idx, sc, off = ix.search_range_batch(qqs, qcs, fam.query_bits, sim, ths, flt)
    cnt = ix.count_range_batch(qqs, qcs, fam.query_bits, sim, ths, flt)
    want = [range_answer(g, t) for g, t in zip(gold, ths)]
    if mask is not None:
        want = [w[mask[w]] for w in want]
    sizes = [len(w) for w in want]
    np.testing.assert_array_equal(cnt, sizes, err_msg=msg + ": counts")
    np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(sizes)]), err_msg=msg + ": offsets")
    assert len(idx) == len(sc) == off[-1]
    assert not np.isnan(sc).any(), msg + ": a NaN score in an answer"
    for q, w in enumerate(want):
        sl = slice(off[q], off[q + 1])
        np.testing.assert_array_equal(idx[sl], w, err_msg="%s: pair %d threshold %r" % (msg, q, ths[q]))
        np.testing.assert_array_equal(bits(sc[sl]), bits(gold[q][w]), err_msg="%s: pair %d threshold %r: score bits" % (msg, q, ths[q]))
        assert not np.isnan(gold[q][idx[sl]]).any(), "%s: pair %d: a NaN-scored row in the answer" % (msg, q)
    return idx.tobytes(), bits(sc).tobytes(), off.tobytes(), cnt.tobytes()


def both_bounds(ix, run, msg):
    """run(msg) under fast_bound 1 and 0: identical bytes; the option is restored"""
    try:
        first = run(msg + " fast_bound 1")
        ix.set_option("fast_bound", 0)
        assert run(msg + " fast_bound 0") == first, msg + ": fast_bound 0 and 1 differ"
    finally:
        ix.set_option("fast_bound", 1)      # (host state only: safe after a device failure too)
    return first


def _gold(fam, sim, who):
    s = H.scores(fam, sim)
    return [s[q][2] for q in who]


@pytest.mark.parametrize("fam,sim", CASES, ids=IDS)
def test_every_pair_in_one_call(fam, sim):
    qqs, qcs, ths, who = H.pairs(fam, sim)
    gold = _gold(fam, sim, who)
    msg = "%s sim %d" % (fam.name, sim)
    with located(msg):
        compact, inline = _index(fam, "compact"), _index(fam, "inline")
        got = both_bounds(compact, lambda m: answer(compact, fam, sim, qqs, qcs, ths, gold, m), msg + " compact")
        control = answer(inline, fam, sim, qqs, qcs, ths, gold, msg + " inline")
        assert got[0] == control[0] and got[2] == control[2], msg + ": the compact layout's ords are not the inline layout's"
        assert np.frombuffer(got[2], np.int64)[-1] > fam.n          # (more than one query's worth of entries)


@pytest.mark.parametrize("sim", H.SIMS)
def test_filtered(sim):
    fam = MAIN
    qqs, qcs, ths, who = H.pairs(fam, sim)
    gold = _gold(fam, sim, who)
    with located("filtered sim %d" % sim):
        compact, inline = _index(fam, "compact"), _index(fam, "inline")
        for label, mask in H.accept_sets(fam).items():
            msg = "main sim %d, %s" % (sim, label)
            with capi.Filter(compact, mask) as flt:
                got = both_bounds(compact, lambda m: answer(compact, fam, sim, qqs, qcs, ths, gold, m, flt, mask), msg + " compact")
            with capi.Filter(inline, mask) as flt:
                control = answer(inline, fam, sim, qqs, qcs, ths, gold, msg + " inline", flt, mask)
            assert got[0] == control[0] and got[2] == control[2], msg


@pytest.mark.parametrize("sim", H.SIMS)
def test_more_pairs_than_a_sub_batch(sim):
    """the table repeated until it holds more than 1024 (query, threshold) pairs, so the call crosses the sub-batch boundary - in the
    middle of a repeat, with hostile rows on both sides"""
    fam = MAIN
    reps = 1024 // len(H.pairs(fam, sim)[2]) + 1
    qqs, qcs, ths, who = (np.concatenate([a] * reps) for a in H.pairs(fam, sim))
    assert 1024 < len(ths) < 2048 and 1024 % len(H.pairs(fam, sim)[2])
    gold = _gold(fam, sim, who)
    with located("call size sim %d" % sim):
        compact = _index(fam, "compact")
        both_bounds(compact, lambda m: answer(compact, fam, sim, qqs, qcs, ths, gold, m), "main sim %d, %d pairs" % (sim, len(ths)))


def test_after_an_update():
    """update_rows puts a row with additionalCorrection 1e300 into an ordinary tile and an ordinary row over the NaN row of the
    NaN-additive tile: bbq_tile_add_range_list_kernel rewrites both tiles' ranges - the first stops rejecting under COSINE and MIP (a stale
    maximum would lose the new row, whose score is +inf), the second starts.  Answers equal the oracle over the updated rows"""
    fam = MAIN
    ords, ncodes, ncorr, codes, corr = H.update(fam)
    with located("update"):
        ix = _make(fam, "compact", *H.rows(fam))
        try:
            ix.update_rows(ords, ncodes, ncorr)
            for sim in H.SIMS:
                qq, qc = H.queries(fam, sim)
                now = [H.score(fam, codes, corr, qq[q], qc[q], sim)[2] for q in range(len(qq))]
                if sim != 0:
                    assert now[0][ords[0]] == np.inf and np.isnan(H.scores(fam, sim)[0][2][ords[1]]) and np.isfinite(now[0][ords[1]])
                tabs = [H.thresholds_of(s) for s in now]
                who = np.repeat(np.arange(len(qq)), [len(t) for t in tabs])
                both_bounds(ix, lambda m: answer(ix, fam, sim, qq[who], qc[who], np.concatenate(tabs), [now[q] for q in who], m),
                            "main sim %d after the update" % sim)
        finally:
            if not _device_failed:
                ix.close()
