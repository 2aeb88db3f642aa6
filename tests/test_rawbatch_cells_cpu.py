"""CPU: the matrix of tests/rawbatch_cells.py held to the code and to its own conditions.  form_of restates two host lines, which are
read out of the sources here, so a change of the rule that picks the matrix-core sweep's form fails here instead of leaving the GPU
cells on another form than they are named after; every form meets every row width, ragged and full, and every similarity in both
layouts; and every cell's seeded input still makes the GPU comparison bite: every query value of the bit width is staged, the answers
come from behind the dense prefix and from every place of a tile, no score is NaN, no tile overflows a wave's survivor queue and the
device's selection is what gets compared; the hostile cells have answers from behind the dense prefix too.  A cell that fails a
condition gets another seed in rawbatch_cells.SEEDS, never a weaker condition."""
import os
import re

import numpy as np
import pytest

import orclib as O
import rawbatch_cells as C

CSRC = os.path.join(O.ROOT, "better-binary-quantization_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name), encoding="utf-8") as f:
        return f.read()


def test_form_of_restates_the_host_lines():
    core, query = _source("bbq_core.cpp"), _source("bbq_query.cpp")
    # a call with a feed takes maxq from the bit width; one without takes 15 for every query of at most four planes
    m = re.search(r"if \(feed\) \{.*?\n(.*?)\n  \} else \{\n(.*?)\n  \}", core, re.S)
    assert m and "c.maxq = (1 << query_bits) - 1;" in m.group(1) and "c.maxq = c.planes <= 4 ? 15 : max_value(" in m.group(2)
    assert "m.fp = c.maxq <= 15;" in query
    assert "m.scale8 = c.maxq <= 3 ? 8 : c.maxq <= 7 ? 4 : 2;" in query
    assert "ms.fp ? ms.scale8 / 8.0f : 0.0f" in core                                   # S = scale8 / 8 is what the kernel gets
    assert "c.maxq <= 127" in core                                                    # beyond it there is no matrix-core sweep
    assert "if (n_queries <= 64 || k == 0 || ix->multi) {" in core                    # the feed: more than 64 raw queries
    assert [C.form_of(q) for q in range(1, 9)] == [("fp", 1), ("fp", 1), ("fp", 0.5), ("fp", 0.25), ("int8", 1), ("int8", 1), ("int8", 1), None]
    assert [C.form_of(q) for q in C.QUERY_BITS] == [("fp", 1), ("fp", 1), ("fp", 0.5), ("fp", 0.25), ("int8", 1)]


def test_the_first_segment_is_the_dense_prefix_the_cells_assume():
    """start_plan: s0 = min(max(first_segment_rows, 4 k_dev rounded up to whole chunks), 8192) with k_dev = K + 1 - 1024 rows for
    first_segment_rows 1024, so BEYOND = 2048 lies behind it and needs no move; add_storage_segments then gives everything behind it to
    ONE sparse segment, the dominant one (4 x 1024 is beyond half of the rows)"""
    core = _source("bbq_core.cpp")
    assert "p.s0 = std::max<int64_t>(ix->opt_s0, (4 * k + kChunkRows - 1) / kChunkRows * kChunkRows);" in core
    assert "p.s0 = std::min<int64_t>(p.s0, 8192);" in core
    assert "c.k_dev = final_k > 0 ? keff + 1 : keff;" in core
    s0 = min(max(dict(C.OPTIONS)["first_segment_rows"], (4 * (C.K + 1) + C.CHUNK - 1) // C.CHUNK * C.CHUNK), 8192)
    assert s0 == C.FIRST_SEGMENT == 1024 and C.BEYOND >= 2 * s0
    assert s0 * dict(C.OPTIONS)["segment_growth"] > C.N // 2 and C.N - s0 > s0


def test_the_shapes():
    assert C.N == 12 * C.CHUNK + 56 and C.N % C.TILE == 56
    assert C.NQ > 64 and (C.NQ + 31) // 32 == 3 and C.NQ % 32 == 6
    assert [C.w16_of(d) for d in C.DIMS] == [1, 1, 6, 6, 8, 8, 12, 12]
    assert [C.is_ragged(d) for d in C.DIMS] == [True, False] * 4
    src = C.sources(1)
    assert len(set(src.tolist())) == C.NQ and src.min() >= C.BEYOND and src.max() < C.N
    kernels = _source("bbq_mfma_kernels.hip")
    assert "constexpr int kMfmaQueueCapTwo = %d;" % C.QUEUE in kernels and "constexpr int kMfmaQueueCap = 512;" in kernels      # the smaller of the two
    assert C.FIRST_SEGMENT % C.TILE == 0 and C.BEYOND % C.TILE == 0


def test_the_matrix_covers_every_form_at_every_width():
    assert len(C.CELLS) == len(set(C.CELLS)) == 120 and set(C.SEEDS) <= set(C.CELLS)
    assert set(C.INLINE_CELLS) <= set(C.CELLS) and set(C.HOSTILE_CELLS) <= set(C.CELLS)
    assert len(C.HOSTILE_CELLS) == 40 and len({(c.dim, c.query_bits) for c in C.HOSTILE_CELLS}) == 40
    assert {(c.dim, c.query_bits) for c in C.INLINE_CELLS} == {(d, q) for d in C.DIMS for q in C.QUERY_BITS}
    forms = (("fp", 1), ("fp", 0.5), ("fp", 0.25), ("int8", 1))
    for cells, what in ((C.CELLS, "compact"), (C.INLINE_CELLS, "inline")):
        seen = {}
        for c in cells:
            seen.setdefault(C.form_w(c), {"sims": set(), "ragged": set()})
            seen[C.form_w(c)]["sims"].add(c.sim)
            seen[C.form_w(c)]["ragged"].add(C.is_ragged(c.dim))
        assert set(seen) == {(f, w) for f in forms for w in C.W_CLASSES}, what
        for fw, s in seen.items():
            assert s["sims"] == {0, 1, 2} and s["ragged"] == {True, False}, "%s %s: %s" % (what, fw, s)
    # the hostile variant: every (form, W) ragged and full and with a EUCLIDEAN cell, and all three similarities over the matrix
    assert {(C.form_w(c), C.is_ragged(c.dim)) for c in C.HOSTILE_CELLS} == {((f, w), r) for f in forms for w in C.W_CLASSES for r in (True, False)}
    assert {C.form_w(c) for c in C.HOSTILE_CELLS if c.sim == 0} == {(f, w) for f in forms for w in C.W_CLASSES}
    assert {c.sim for c in C.HOSTILE_CELLS} == {0, 1, 2}


@pytest.mark.parametrize("w16", C.W_CLASSES)
@pytest.mark.parametrize("form", [("fp", 1), ("fp", 0.5), ("fp", 0.25), ("int8", 1)], ids=["S1", "S1_2", "S1_4", "int8"])
def test_the_answers_stand_all_over_the_tiles(form, w16):
    """a survivor's dot product is recovered per register group - rows 0..31 and 32..63 of a tile - and per lane: over the cells of a
    (form, W) every one of the 64 places of a tile holds an answer, every cell has answers in both halves, and an answer stands in
    the last, 56-row tile"""
    places, in_last_tile = np.zeros(C.TILE, np.int64), 0
    for cell in C.CELLS:
        if C.form_w(cell) == (form, w16):
            ords = np.concatenate([w[0] for w in C.case(cell).want])
            here = np.bincount(ords % C.TILE, minlength=C.TILE)
            assert (here[:32] > 0).sum() >= 4 and (here[32:] > 0).sum() >= 4, "%s: %s" % (C.cell_id(cell), here.tolist())
            places += here
            in_last_tile += int((ords >= C.N // C.TILE * C.TILE).sum())
    assert (places > 0).all(), places.tolist()
    assert in_last_tile > 0


@pytest.mark.parametrize("cell", C.CELLS, ids=C.cell_id)
def test_the_cell_s_input_meets_its_conditions(cell):
    c = C.case(cell)                                                      # (asserts that no oracle score of the cell is NaN)
    top_value = (1 << cell.query_bits) - 1
    # value coverage: every value of the bit width occurs - the top FP6 code of the form's table is staged - and none beyond it
    assert c.qq.shape == (C.NQ, cell.dim) and c.queries.shape == (C.NQ, cell.dim) and c.codes.shape == (C.N, (cell.dim + 7) // 8)
    assert np.unique(c.qq).tolist() == list(range(top_value + 1))
    if C.is_ragged(cell.dim):                                             # the partly empty last 32-dimension word holds a value
        assert c.qq[:, cell.dim // 32 * 32:].any()
    # the rows are the product's: component sums are popcounts, and a ragged row's padding bits are clear
    assert (c.corr[:, 3] == np.unpackbits(c.codes, axis=1).sum(axis=1)).all()
    assert not np.unpackbits(c.codes, axis=1)[:, cell.dim:].any()
    # answers from behind the dense prefix: at least half of every query's
    assert not np.isnan(c.top).any() and c.moved < (C.N - C.BEYOND) // 4
    for q, (ords, sc) in enumerate(c.want):
        assert len(ords) == C.K and (ords >= C.BEYOND).sum() * 2 >= C.K, "query %d: %s" % (q, ords.tolist())
    # the pairs that beat their threshold fit a wave's survivor queue with a quarter of it to spare for what the pre-filter's slack lets
    # through: an overflow flag in this cell is then the sweep's doing, not the input's
    assert c.crowd <= C.QUEUE * 3 // 4, "%d pairs of one tile and group beat their thresholds" % c.crowd
    # the device selects the answer unless two of the K + 1 best scores compare equal
    untied = sum(len(np.unique(t)) == C.K + 1 for t in c.top)
    assert untied >= 60, "%d of %d queries without a tie among their %d best" % (untied, C.NQ, C.K + 1)


@pytest.mark.parametrize("cell", C.HOSTILE_CELLS, ids=C.cell_id)
def test_the_hostile_variant(cell):
    c, h = C.case(cell), C.hostile(cell)
    assert (h.corr[:, 3] == c.corr[:, 3]).all() and not h.nan             # the comparison stays exact: no NaN score
    width = h.corr[:, 1] - h.corr[:, 0]
    changed = np.flatnonzero((h.corr != c.corr).any(axis=1))
    assert len(changed) == C.N // 10 and set(h.weird.tolist()) <= set(changed.tolist())
    assert (width == 0).sum() >= 40 and (width < 0).sum() >= 40 and (h.corr[:, 1] == 1e300).sum() == 100
    assert (h.corr[:, 2] == 3.0e38).sum() == 100 and (h.corr[:, 0] == -1e-320).sum() == 100 and (np.abs(h.corr[:, 2]) > 1e3).sum() > 100
    with np.errstate(over="ignore"):
        lost = (width > 0) & (h.corr[:, 1].astype(np.float32) == h.corr[:, 0].astype(np.float32))
    assert lost.sum() >= 40
    assert (h.weird >= C.FIRST_SEGMENT).sum() > 100 and (h.weird < C.FIRST_SEGMENT).sum() > 10      # on both sides of the dense prefix
    assert all(len(w[0]) == C.K for w in h.want) and all(len(w[0]) == C.K_DEEP for w in h.deep)
    # what makes the cell bite.  EUCLIDEAN: a huge additional correction sends a score to 0, not to the top - half of every query's K
    # answers come from behind the dense prefix, with scores of their own.  The other two: the K best are rows whose 3e38 saturates the
    # score; K_DEEP reaches past them, and half of those answers come from behind the dense prefix
    behind = [w[0] >= C.FIRST_SEGMENT for w in (h.want if cell.sim == 0 else h.deep)]
    assert all(b.sum() * 2 >= len(b) for b in behind), min(int(b.sum()) for b in behind)
    if cell.sim == 0:
        assert all(len(np.unique(w[1][b])) * 2 >= C.K for w, b in zip(h.want, behind))
