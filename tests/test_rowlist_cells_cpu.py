"""CPU: the width matrix of tests/rowlist_cells.py held to the code and to its own conditions.  The cells' compiled() values are exactly
the (store_bits, planes or QB, W) arms of the one ladder the row-list launchers share (rowlist_ladder, csrc/bbq_rowlist.h) - read out of
that header, so a width added later without a cell fails here, and every launcher file is held to calling it and having no arm of its
own; every W class meets every similarity; and every cell's seeded input still exercises what it is there for: the plane
count its kernel is compiled for, thresholds that select some rows and leave some, span and group cases in which a tie sends a query
to the heap - and, in every W class, cases the device answers.  A cell that fails a condition gets another seed in rowlist_cells.SEEDS."""
import itertools
import os
import re

import numpy as np
import pytest

import orclib as O
import rowlist_cells as C
import test_spans_cpu as SC
import test_spans_filtered_cpu as FC
import test_groups_cpu as GC
from test_range_key_cpu import range_answer

CSRC = os.path.join(O.ROOT, "better-binary-quantization_amd", "csrc")
LAUNCHERS = ("bbq_gather_kernels.hip", "bbq_range_kernels.hip", "bbq_span_kernels.hip", "bbq_group_kernels.hip")
CAND_LAUNCHER = "bbq_maxsim_cand_kernels.hip"
FUSED_LAUNCHER = "bbq_maxsim_kernels.hip"
LADDER = "bbq_rowlist.h"

# the arms of the ladder's switches, one regular expression per shape of arm
W_ARM = re.compile(r"^\s*(?:case (\d+)|default): return f\(Int<QB>\{\}, Int<(\d+)>\{\}, Int<(1|SB)>\{\}\);")  # switch (w16), 1-bit and multi-bit
PLANES_ARM = re.compile(r"^\s*(?:case (\d+)|default): return rowlist_width<(\d+)>\(geom\.w16, f\);")          # switch (planes), 1-bit rows
QB_ARM = re.compile(r"^\s*case (\d+): return planes > 4 \? rowlist_width_mb<(\d+), (\d+), MB>\(geom\.w16, f\) : rowlist_width_mb<(\d+), (\d+), MB>\(geom\.w16, f\);")
BYTE_ARM = re.compile(r"^\s*case 8: return f\(Int<(\d+)>\{\}, Int<(\d+)>\{\}, Int<(\d+)>\{\}\);")              # 8-bit rows
FUSED_ARM = re.compile(r"^\s*(?:case (\d+)|default): return launch_maxsim_score_t<(\d+)>\(")
ANY_ARM = re.compile(r"^\s*(case \d+|default):")
NO_KERNEL = re.compile(r"^\s*(case 1:\s*$|default: return hipErrorInvalidValue;)")                   # the nested planes switch; an unknown store_bits
LADDER_CALL = re.compile(r"\browlist_ladder(<[^>(]*>)?\(")                                            # a call, with or without a policy
NO_MULTI_BIT_WIDTHS = "<MultiBitRows::kRunTimeWidth>"


def _lines(name):
    with open(os.path.join(CSRC, name), encoding="utf-8") as f:
        return f.read().splitlines()


def ladder_arms(name=LADDER):
    """every (store_bits, planes or QB, W) the ladder dispatches to; every case / default line of the header has to be one this
    parser knows, so an arm of a new shape fails here instead of going unseen"""
    w_one, w_multi, planes, qb_sb, bytes_arm = set(), set(), set(), set(), set()
    for line in _lines(name):
        if not ANY_ARM.match(line):
            continue
        m = W_ARM.match(line)
        if m:
            assert int(m.group(2)) == (int(m.group(1)) if m.group(1) else 0), line      # case N runs <.., N, ..>; default runs W = 0
            (w_one if m.group(3) == "1" else w_multi).add(int(m.group(2)))
            continue
        m = PLANES_ARM.match(line)
        if m:
            assert m.group(1) is None or m.group(1) == m.group(2), line
            planes.add(int(m.group(2)))
            continue
        m = QB_ARM.match(line)
        if m:
            assert m.group(1) == m.group(3) == m.group(5), line
            qb_sb |= {(int(m.group(3)), int(m.group(2))), (int(m.group(5)), int(m.group(4)))}
            continue
        m = BYTE_ARM.match(line)
        if m:
            bytes_arm.add((int(m.group(3)), int(m.group(1)), int(m.group(2))))
            continue
        assert NO_KERNEL.match(line), "%s: an arm this test cannot read: %s" % (name, line.strip())
    arms = {(1, p, w) for p in planes for w in w_one} | {(sb, qb, w) for sb, qb in qb_sb for w in w_multi} | bytes_arm
    assert w_one and w_multi and planes and qb_sb and bytes_arm, name
    return arms


def fused_arms():
    lines = _lines(FUSED_LAUNCHER)
    assert sum("constexpr int QB = 4;" in l for l in lines) == 1         # launch_maxsim_score_t: 4 planes, 1-bit rows
    widths = set()
    for line in lines:
        if ANY_ARM.match(line):
            m = FUSED_ARM.match(line)
            assert m, "%s: an arm this test cannot read: %s" % (FUSED_LAUNCHER, line.strip())
            assert m.group(1) is None or m.group(1) == m.group(2), line
            widths.add(int(m.group(2)))
    return {(1, 4, w) for w in widths}


def ladder_calls(name):
    """the policies of a launcher file's calls of the ladder ('' = the default: multi-bit rows have compiled widths); the file names no
    arm of its own"""
    lines = _lines(name)
    own = [l.strip() for l in lines if ANY_ARM.match(l)]
    assert not own, "%s: arms outside the ladder: %s" % (name, own)
    assert any('#include "%s"' % LADDER in l for l in lines), name
    return [m.group(1) or "" for l in lines for m in LADDER_CALL.finditer(l)]


@pytest.mark.parametrize("name", LAUNCHERS)
def test_the_cells_cover_every_arm_of_the_launcher(name):
    assert ladder_calls(name) == [""]                                    # the launcher takes the shared ladder, whole
    arms = ladder_arms()
    covered = {C.compiled(c) for c in C.CELLS}
    assert covered == arms, "without a cell: %s; cells without an arm: %s" % (sorted(arms - covered), sorted(covered - arms))
    assert len(arms) == 4 * 5 + 2 * 2 * 3 + 1


def test_the_candidate_launcher_takes_the_ladder_without_multi_bit_widths():
    assert ladder_calls(CAND_LAUNCHER) == [NO_MULTI_BIT_WIDTHS]
    # ... and the ladder gives that policy the run-time width for every multi-bit row: its switch over the compiled widths stands under the
    # other policy, which is the default
    text = "\n".join(_lines(LADDER))
    assert text.count("template <MultiBitRows MB = MultiBitRows::kCompiledWidths, class F>") == 1
    m = re.search(r"\n  if constexpr \(MB == MultiBitRows::kCompiledWidths\) \{\n    switch \(w16\) \{\n(.*?)\n    \}\n  \} else \{\n"
                  r"    return f\(Int<QB>\{\}, Int<0>\{\}, Int<SB>\{\}\);\n  \}\n\}", text, re.S)
    assert m, "rowlist_width_mb no longer has the shape this test reads"
    arms = m.group(1).splitlines()
    assert arms and all(W_ARM.match(l) and W_ARM.match(l).group(3) == "SB" for l in arms), arms
    assert sum(bool(W_ARM.match(l)) and W_ARM.match(l).group(3) == "SB" for l in _lines(LADDER)) == len(arms)   # no multi-bit arm elsewhere


def test_the_cells_cover_every_width_of_the_fused_maxsim_kernel():
    arms = fused_arms()
    covered = {C.compiled(c) for c in C.CELLS if C.fused_maxsim_exists(c)}
    assert covered == arms == {(1, 4, w) for w in C.FUSED_MAXSIM_W}


def test_the_matrix_is_the_issue_s():
    assert len(C.CELLS) == len(set(C.CELLS)) == 7 * 4 + 7 * 2
    assert set(C.SEEDS) <= set(C.CELLS)
    by_dim = {(c.index_bits, c.dim): C.compiled(c)[2] for c in C.CELLS}
    assert by_dim == {(1, 100): 1, (1, 129): 0, (1, 1600): 0, (1, 700): 6, (1, 1000): 8, (1, 1500): 12, (1, 1536): 12,
                      (2, 768): 12, (2, 1000): 16, (2, 100): 0, (4, 384): 12, (4, 500): 16, (4, 96): 0, (8, 64): 0}
    assert C.w16_of(1, 129) == 2 and C.w16_of(1, 1600) == 13
    ragged = [c for c in C.CELLS if (c.dim * C.store_bits_of(c.index_bits)) % 128]       # the last 16-byte chunk is partly padding
    assert {(c.index_bits, c.dim) for c in ragged} >= {(1, 100), (1, 129), (1, 1600), (1, 700), (1, 1000), (1, 1500), (2, 1000), (2, 100), (4, 500)}
    per_w = C.one_cell_per_w()
    assert {C.w_class(c) for c in per_w} == {C.w_class(c) for c in C.CELLS} and len(per_w) == 8
    assert all(C.fused_maxsim_exists(c) for c in per_w if C.w_class(c) in {("1-bit", w) for w in C.FUSED_MAXSIM_W})


def test_every_w_class_meets_every_similarity():
    sims = {}
    for c in C.CELLS:
        sims.setdefault(C.w_class(c), set()).add(c.sim)
    assert set(sims) == {("1-bit", w) for w in (0,) + C.ONE_BIT_W} | {("multi-bit", w) for w in (0,) + C.MULTI_BIT_W}
    assert all(s == {0, 1, 2} for s in sims.values()), sims


def test_the_shared_inputs():
    n, mask = C.N, C.accept_mask()
    assert n == 2 * C.CHUNK + 76 and n % C.TILE == 12
    assert 450 < mask.sum() < 650 and not mask[128:192].any() and mask[1088:1094].all() and not mask[1094:].any()
    assert all(mask[b:b + C.TIE_LEN].sum() >= 2 for b in C.TIE_RUNS)                  # the ties survive the filter
    ords = C.ord_list()
    assert ords[-1] == n - 1 and ords.min() == 0 and len(set(ords.tolist())) < len(ords)
    desc = ords[:14]
    assert (np.diff(desc) < 0).all()
    for edge in (64, 512, 1024, 1088):
        assert edge - 1 in desc and edge in desc
    everything, edges, empty = C.span_lists()
    assert all(SC.spans_are_valid(s, n) for s in C.span_lists())
    assert len(SC.expand(everything)) == n and len(SC.expand(empty)) == 0
    assert all(b % C.TILE and e % C.TILE for b, e in edges if e > b) and any(b == e for b, e in edges)
    assert edges[0][0] < C.CHUNK < edges[0][1] and edges[-1][0] < 2 * C.CHUNK < edges[-1][1]
    lays = C.group_layouts()
    assert tuple(lays) == C.GROUP_LAYOUTS and lays["across_two_edges"].tolist() == [0, 500, n]


def _status_cases(cell):
    """every (kind, case, filtered, k, query) of the span and group calls of a cell with the visited scores the rule looks at"""
    scores = [s[2] for s in C.case(cell)[5][:C.N_SINGLE]]
    everything = FC.masks(C.N)["all"]
    for filtered, mask in ((False, everything), (True, C.accept_mask())):
        for si, sp in enumerate(C.span_lists()):
            rows = FC.accepted(mask, sp)
            if len(rows):
                for k in C.SPAN_KS + (len(rows) + 1,):
                    for q, s32 in enumerate(scores):
                        yield ("spans", si, filtered), k, q, s32[rows]
        for lname, off in C.group_layouts().items():
            live = GC.plan(off, mask)[1]
            for q, s32 in enumerate(scores):
                v = s32[GC.representatives(s32, off, mask)[0]]
                assert len(v) == live
                for k in C.GROUP_KS + (live + 1,):
                    yield ("groups", lname, filtered), k, q, v


@pytest.mark.parametrize("cell", C.CELLS, ids=C.cell_id)
def test_the_cell_s_input_meets_its_conditions(cell):
    codes, corr, cdp, qq, qc, scores = C.case(cell)
    sb, planes, w = C.compiled(cell)
    top = (1 << cell.index_bits) - 1
    # the plane count the kernel is compiled for, from every query's values
    assert qq.shape == (C.N_QUERIES, cell.dim) and int(qq.max()) <= (1 << cell.query_bits) - 1
    for q in range(C.N_QUERIES):
        assert C.planes_of_values(cell.index_bits, cell.query_bits, qq[q]) == planes, "query %d" % q
        if sb == 1:
            m = int(np.bitwise_or.reduce(qq[q]))
            assert {1: m <= 1, 2: 1 < m <= 3, 4: 3 < m <= 15, 8: m > 15}[planes], "query %d: the OR of its values is %d" % (q, m)
        elif cell.query_bits == 8:
            assert int(qq[q].max()) > 15, "query %d" % q
    assert C.planes_of_values(cell.index_bits, cell.query_bits, qq) == planes              # and of a whole call's
    # the planted rows
    unpacked = np.unpackbits(codes, axis=1)[:, :cell.dim] if cell.index_bits == 1 else codes
    assert codes.shape == (C.N, (cell.dim + 7) // 8 if cell.index_bits == 1 else cell.dim)
    assert (unpacked[C.ZERO_ROW] == 0).all() and (unpacked[C.ONES_ROW] == top).all() and int(unpacked.max()) == top
    assert (corr[:, 3] == unpacked.sum(axis=1)).all() and corr[C.ZERO_ROW, 3] == 0 and corr[C.ONES_ROW, 3] == cell.dim * top
    a, b = C.TIE_RUNS
    for run in (codes[a:a + C.TIE_LEN], codes[b:b + C.TIE_LEN]):
        assert (run == codes[a]).all()
    assert (corr[a:a + C.TIE_LEN].view(np.uint64) == corr[b:b + C.TIE_LEN].view(np.uint64)).all()
    # no NaN anywhere, and query 0 has the tie runs at its top
    for d, s64, s32 in scores:
        assert not np.isnan(s64).any() and not np.isnan(s32).any() and len(s32) == C.N
    assert (scores[0][2] > scores[0][2][a]).sum() <= 2                    # (at most the two planted codes above them)
    assert len(np.unique(scores[0][2])) >= C.N // 3                        # not a handful of clamped values: a wrong dot product shows
    # the thresholds select at least one row and leave out at least one, with and without the filter
    mask = C.accept_mask()
    for q in range(C.N_SINGLE):
        s32 = scores[q][2]
        ths = C.thresholds_of(s32)
        assert ths[0] == -np.inf and len(range_answer(s32, ths[0])) == C.N and len(range_answer(s32, ths[3])) == 0
        for t in ths[1:3]:
            hit = range_answer(s32, t)
            assert 0 < len(hit) < C.N and 0 < mask[hit].sum() < mask.sum(), "query %d threshold %r" % (q, t)
    # every span and group case: L > k for some k, and a tie among the k + 1 best sends one query to the heap
    cases = {}
    for case, k, q, v in _status_cases(cell):
        c = cases.setdefault(case, {"beyond_k": False, "tie": False})
        c["beyond_k"] |= len(v) > k
        c["tie"] |= bool(SC.tie_is_the_reason(v, k))
    assert len(cases) == 2 * (2 + len(C.GROUP_LAYOUTS))
    for case, c in cases.items():
        assert all(c.values()), "%s: %s" % (case, c)


def test_both_statuses_occur_in_every_w_class():
    seen = {}
    for cell in C.CELLS:
        for _, k, _, v in _status_cases(cell):
            seen.setdefault(C.w_class(cell), set()).add(SC.expected_status(v, k))
    assert len(seen) == 8 and all(s == {0, 1} for s in seen.values()), seen


def test_the_resident_mb_variant_has_one_cell_per_w():
    cells = C.one_cell_per_w()
    assert sorted(C.w_class(c) for c in cells) == sorted({C.w_class(c) for c in C.CELLS})
    assert all(a != b for a, b in itertools.combinations([C.w_class(c) for c in cells], 2))
