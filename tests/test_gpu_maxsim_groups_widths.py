"""GPU: MaxSim over chosen groups at every compiled width - every cell of tests/rowlist_cells.py, both corrections layouts (and the
compact one without the row_sums side array), unfiltered and under the matrix's filter - bit for bit against the model of
tests/maxsim_groups_model.py over the cell's oracle scores.  One group layout (random_1_20), two queries per call - 3 tokens and one
token block + 1 - and one shuffled candidate list with a duplicate."""
import numpy as np
import pytest

import maxsim_groups_model as MG
import maxsim_model as M
import rowlist_cells as C
import test_groups_cpu as GC
import test_spans_filtered_cpu as FC
import test_gpu_maxsim as GM
import test_gpu_maxsim_groups as GMG
import test_gpu_rowlist_widths as GW      # its cached representatives of every (cell, layout, mask): computed once per process
from bbqlib import bbq_amd as B, capi

pytestmark = pytest.mark.gpu

LAYOUT = "random_1_20"
CASES = [(c, v) for c in C.CELLS for v in ("compact", "inline")]


def _list(live, seed):
    lst = np.random.default_rng(seed).permutation(np.asarray(live, np.int64))
    return np.concatenate([lst, lst[[0, len(lst) // 2]]])                   # every live group, shuffled, two of them twice


@pytest.mark.parametrize("cell,layout", CASES, ids=["%s-%s" % (C.cell_id(c), v) for c, v in CASES])
def test_cell(cell, layout):
    codes, corr, cdp, qq, qc, _ = C.case(cell)
    tb = capi.maxsim_token_block()
    assert tb + 1 <= C.N_QUERIES
    spans = [(1, 4), (0, tb + 1)]
    off = C.group_layouts()[LAYOUT]
    ix = B.Index(codes, corr, cell.dim, cdp, index_bits=cell.index_bits, corrections=layout)
    try:
        for filtered, mask in ((False, FC.masks(C.N)["all"]), (True, C.accept_mask())):
            rep, live = GW._reps(cell, LAYOUT, filtered)
            lists = [_list(live, 11), _list(live, 12)[::-1].copy()]
            assert len(MG.cut_by(off, lists[0], MG.PIECE)) > 0 and MG.positions(off, lists[0])[-1] % MG.WAVE != 0
            with GM._open(ix, off, mask) as groups:
                for row_sums in ((-1, 0) if layout == "compact" else (-1,)):
                    ix.set_option("row_sums", row_sums)
                    GMG.assert_lists(ix, groups, rep, live, qq, qc, spans, lists, cell.query_bits, cell.sim,
                                     "%s %s%s row_sums %d" % (C.cell_id(cell), layout, " filtered" if filtered else "", row_sums), ks=(3, None))
    finally:
        ix.set_option("row_sums", -1)
        ix.close()


@pytest.mark.parametrize("layout", ["compact", "inline"])
def test_a_row_too_wide_to_stage_a_whole_token_block(layout):
    """8-bit rows of 2 048 dimensions: a token's staged query data takes 2 048 + 96 bytes, 32 of them more than the 64 KiB a workgroup
    stages, so the kernel works through a token block in two passes - 30 tokens and the rest - inside the workgroup.  The recipe is
    rowlist_cells.case's, on 300 rows"""
    cell, n = C.Cell(8, 2048, 4, 0), 300
    tb = capi.maxsim_token_block()
    per_token = 16 * C.w16_of(cell.index_bits, cell.dim) + 96
    assert tb * per_token > 65536 >= per_token and 1 < 65536 // per_token < tb
    rng = np.random.default_rng(9100)
    sigma = 0.5 / np.sqrt(C.inflation(cell) * cell.dim)
    base = (sigma * rng.standard_normal((n, cell.dim))).astype(np.float32)
    queries = (base[rng.integers(0, n, tb + 1)] + 0.5 * sigma * rng.standard_normal((tb + 1, cell.dim))).astype(np.float32)
    codes, corr, cen = B.quantize_vectors(base, cell.sim, cell.index_bits)
    cdp = B.centroid_dp(cen)
    qq, qc = B.quantize_queries(queries, cen, cell.sim, cell.query_bits)
    s32 = [C.oracle_scores(cell, codes, corr, qq[i], qc[i], cdp)[2] for i in range(tb + 1)]
    off = GC.layouts(n)["random_1_20"]
    spans = [(0, tb + 1), (2, tb), (5, 7)]                                   # two passes and one more block; two passes; one
    ix = B.Index(codes, corr, cell.dim, cdp, index_bits=cell.index_bits, corrections=layout)
    try:
        for mask in (FC.masks(n)["all"], FC.masks(n)["random_half"]):
            rep, live = M.rep_scores(s32, off, mask)
            lists = [_list(live, 13), _list(live, 14)[::-1].copy(), live[:5]]
            with GM._open(ix, off, mask) as groups:
                GMG.assert_lists(ix, groups, rep, live, qq, qc, spans, lists, cell.query_bits, cell.sim, "2048-d 8-bit rows %s" % layout, ks=(3, None))
    finally:
        ix.close()
