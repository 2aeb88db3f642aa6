"""GPU: bbq_search_raw_batch on the shared sweep on the matrix cores (sweep_share 32, bbq_scan_mfma_kernel) over the matrix of
tests/rawbatch_cells.py.  A raw call of more than 64 queries is the only one that reaches the sweep's FP6 x FP4 forms with S = 1/2
(queryBits 3) and S = 1 (queryBits 1 and 2) - rawbatch_cells.form_of; bbq_search_batch runs S = 1/4 for every query of at most four
planes.  Every answer is compared bit for bit with the CPU oracle's heap over its scores of the product's own quantization: ords, f32
score bits through canon32, order and counts.  No tolerance anywhere.

Every index runs with sweep_share 32, first_segment_rows 1024, segment_growth 4.  With flood_rows 0 a query the matrix-core sweep flags
has no sweep of its own to fall back to and is counted in dense_fallbacks: dense_fallbacks == 0 then says that the answers came from the
dense prefix and the matrix-core sweep's lists.  tests/test_rawbatch_cells_cpu.py holds the inputs to the conditions under which a wrong
dot product recovered from an accumulator shows in an answer.

A BBQ_ERR_HIP from any call ends the whole pytest session (test_gpu_mutation_walk.located): nothing more is started on a device that has
failed, not even the close of the handle."""
import contextlib

import numpy as np
import pytest

import orclib as O
import rawbatch_cells as C
import test_gpu_mutation_walk as MW
from test_gpu_score_ords import canon32
from bbqlib import bbq_amd as B

pytestmark = pytest.mark.gpu

MAIN = [(c, "compact") for c in C.CELLS] + [(c, "inline") for c in C.INLINE_CELLS]
MAIN.sort(key=lambda cl: C.CELLS.index(cl[0]))             # a cell's two layouts side by side
# one cell per (form, W) of the 768-d forms, and queryBits 2 at the narrowest and at a ragged widest row
SECOND_SUBBATCH = (C.Cell(768, 2, 0), C.Cell(768, 3, 1), C.Cell(768, 4, 2), C.Cell(768, 7, 0), C.Cell(100, 2, 1), C.Cell(1500, 2, 2))
EDGES = C.Cell(768, 3, 1)


@contextlib.contextmanager
def _open(cell, layout, msg, corr=None, **options):
    c = C.case(cell)
    ix = B.Index(c.codes, c.corr if corr is None else corr, cell.dim, c.cdp, corrections=layout)
    try:
        with MW.located(msg):
            for name, value in dict(C.OPTIONS, **options).items():
                ix.set_option(name, value)
            yield ix
    except pytest.exit.Exception:
        ix._h = None               # the device has failed: the handle is neither closed nor destroyed
        raise
    except BaseException:
        ix.close()
        raise
    ix.close()


def _assert_answers(res, want, msg):
    idx, sc, cnt = res[:3]
    assert len(cnt) == len(want)
    for q, (ords, scores) in enumerate(want):
        assert cnt[q] == len(ords), "%s query %d: %d answers, the oracle has %d" % (msg, q, cnt[q], len(ords))
        np.testing.assert_array_equal(idx[q, :cnt[q]], ords, err_msg="%s query %d" % (msg, q))
        np.testing.assert_array_equal(canon32(sc[q, :cnt[q]]), canon32(scores), err_msg="%s query %d: score bits" % (msg, q))


def _raw(ix, cell, k=C.K, queries=None, **kw):
    c = C.case(cell)
    return ix.search_raw_batch(c.queries if queries is None else queries, c.cen, cell.sim, cell.query_bits, k, **kw)


@pytest.mark.parametrize("cell,layout", MAIN, ids=["%s-%s" % (C.cell_id(c), l) for c, l in MAIN])
def test_raw_call_on_the_matrix_cores(cell, layout):
    """70 raw queries in one sub-batch, flood_rows 0: the form's answers are the oracle's, no query fell to the dense path, and the
    dominant launch reports the bytes of a sweep that loads every tile once per 64 or 32 queries (enqueue_subbatch's timing block).
    Then the same quantized queries through bbq_search_batch - S = 1/4 up to queryBits 4, int8 at 7, the forms the suite already runs:
    the control.  A fallback there says the cell's input is unfit (another seed in rawbatch_cells.SEEDS), one in the raw call alone
    that the form's magnitude budget is."""
    c = C.case(cell)
    form, w16 = C.form_w(cell)
    msg = "%s %s %s W %d" % (C.cell_id(cell), layout, form, w16)
    with _open(cell, layout, msg, flood_rows=0, batch_queries=128) as ix:
        assert ix.bytes_per_row == 16 * w16 + (4 if layout == "compact" else 24)
        res = _raw(ix, cell, want_quantized=True)
        np.testing.assert_array_equal(res[3], c.qq, err_msg=msg + ": the quantized queries")
        np.testing.assert_array_equal(res[4].view(np.uint64), c.qc.view(np.uint64), err_msg=msg + ": the query corrections")
        _assert_answers(res, c.want, msg + " raw")
        st = ix.stats()
        print("%s raw: dense_fallbacks %d host_replays %d candidates %d last_scan_rows %d last_scan_bytes %d"
              % (msg, st["dense_fallbacks"], st["host_replays"], st["candidates"], st["last_scan_rows"], st["last_scan_bytes"]))
        assert st["dense_fallbacks"] == 0, msg + " raw"
        assert st["last_scan_rows"] > 0 and st["last_scan_rows"] % C.NQ == 0
        rows = st["last_scan_rows"] // C.NQ
        assert rows == C.N - C.FIRST_SEGMENT                              # the one sparse segment behind the dense prefix
        row_bytes = 16 * w16 + 24 if layout == "compact" else ix.bytes_per_row
        assert st["last_scan_bytes"] in {rows * loads * row_bytes for loads in (2, 3)}, msg      # 70 queries: 64 or 32 per tile load
        _assert_answers(ix.search_batch(c.qq, c.qc, cell.query_bits, cell.sim, C.K), c.want, msg + " quantized")
        st = ix.stats()
        print("%s quantized: dense_fallbacks %d host_replays %d candidates %d" % (msg, st["dense_fallbacks"], st["host_replays"], st["candidates"]))
        assert st["dense_fallbacks"] == 0, msg + " quantized"


@pytest.mark.parametrize("cell", C.HOSTILE_CELLS, ids=C.cell_id)
def test_raw_call_hostile_rows(cell):
    """a tenth of the rows with corrections no threshold can bound - they pass every pair, so queues may overflow and a query may fall
    back (default flood_rows): the answers are the oracle's, for K and for K_DEEP - under COSINE and MAXIMUM_INNER_PRODUCT the K best
    are rows whose 3e38 saturates the score, most of them in the dense prefix; K_DEEP reaches past them"""
    h = C.hostile(cell)
    msg = "hostile %s %s" % (C.cell_id(cell), C.form_w(cell))
    with _open(cell, "compact", msg, corr=h.corr) as ix:
        for k, want in ((C.K, h.want), (C.K_DEEP, h.deep)):
            _assert_answers(_raw(ix, cell, k=k), want, "%s k = %d" % (msg, k))
            st = ix.stats()
            print("%s k = %d: dense_fallbacks %d host_replays %d" % (msg, k, st["dense_fallbacks"], st["host_replays"]))


@pytest.mark.parametrize("cell", SECOND_SUBBATCH, ids=C.cell_id)
def test_raw_call_second_subbatch(cell):
    """batch_queries 64: sub-batches of 64 and 6 queries - the second is enqueued while the first is in flight, its queries were
    quantized meanwhile, and its group is partial"""
    c = C.case(cell)
    msg = "two sub-batches %s %s" % (C.cell_id(cell), C.form_w(cell))
    with _open(cell, "compact", msg, flood_rows=0, batch_queries=64) as ix:
        for threads in (1, 7):
            _assert_answers(_raw(ix, cell, n_threads=threads), c.want, "%s, %d threads" % (msg, threads))
            assert ix.stats()["dense_fallbacks"] == 0, msg


@pytest.mark.parametrize("cell,options", [(C.Cell(768, 8, 1), {}), (C.Cell(200, 4, 2), {}), (C.Cell(768, 3, 0), {"sweep_share": 8})],
                         ids=["qb8", "200d", "sweep_share_8"])
def test_raw_call_without_a_matrix_core_form(cell, options):
    """queryBits 8 through the feed (maxq 255), a row width without an instantiation (w16 2), and sweep_share 8 - the shared VALU sweep
    with its planes chosen by the bit width: the call falls back quietly and answers as the oracle does"""
    c = C.case(cell)
    msg = "no matrix-core form: %s %s" % (C.cell_id(cell), options)
    assert C.form_of(cell.query_bits) is None or C.w16_of(cell.dim) not in C.W_CLASSES or options
    with _open(cell, "compact", msg, **options) as ix:
        _assert_answers(_raw(ix, cell), c.want, msg)


def test_raw_call_k_edges_and_refused_query():
    """768-d, queryBits 3 (S = 1/2): k = 1024, the last rank the device selects, and 1025, the first the host replays - the first
    segment grows to 4 (k + 1) rows and the matrix cores sweep what is left; k = 5000 > 4096, where the dense path waits on the feed
    query by query.  Then a NaN in query 66, inside the second sub-batch: refused with the quantizer's code, and the index answers the
    next raw call as before"""
    cell = EDGES
    c = C.case(cell)
    s32 = C.scores_of(cell)
    msg = "k edges %s %s" % (C.cell_id(cell), C.form_w(cell))
    with _open(cell, "compact", msg) as ix:
        for k in (1024, 1025, 5000):
            _assert_answers(_raw(ix, cell, k=k), [O.heap_topk(s, k) for s in s32], "%s k = %d" % (msg, k))
            st = ix.stats()
            print("%s k = %d: dense_fallbacks %d host_replays %d" % (msg, k, st["dense_fallbacks"], st["host_replays"]))
        bad = c.queries.copy()
        bad[66, 5] = np.nan
        with pytest.raises(B.BBQError) as e:
            _raw(ix, cell, queries=bad, n_threads=3)
        if e.value.code == B.capi.ERR_HIP:
            raise e.value
        assert e.value.code == B.capi.ERR_NAN_INPUT
        _assert_answers(_raw(ix, cell), c.want, msg + " after the refused call")
