"""The width matrix of the row-list entry points (bbq_score_ords*, bbq_search_ords_batch, bbq_*_range_batch, bbq_search_spans*_batch,
bbq_search_grouped_batch, bbq_search_maxsim_batch): which cells there are, which compiled kernel arm each one runs, and the seeded inputs
of every cell.  Numpy and the host side of the library only (the quantizer, the oracle): nothing here touches a device.
tests/test_rowlist_cells_cpu.py holds the matrix to the launchers' switch arms and the inputs to their conditions;
tests/test_gpu_rowlist_widths.py runs every cell.

A cell is (index_bits, dim, query_bits, sim).  Its kernel is fixed by compiled(cell) = (store_bits, planes or QB, W), the layout, whether
the call carries a filter, and whether the launch's view carries the row_sums side array."""
import collections
import functools

import numpy as np

import orclib as O
from bbqlib import bbq_amd as B

N = 1100                                   # two full chunks of 512 rows and a 76-row tail whose last tile holds 12 rows
CHUNK, TILE = 512, 64
TIE_RUNS = (200, 700)                      # rows [200, 210) and [700, 710) are copies of one row: query 0's best
TIE_LEN = 10
ZERO_ROW, ONES_ROW = 300, 900              # an all-zero code and an all-ones code (component sums 0 and dim * (2^bits - 1))
N_QUERIES = 33                             # token vectors per cell: the longest MaxSim query takes bbq_maxsim_token_block() + 1 = 33
N_SINGLE = 3                               # the first of them are the queries of the one-vector entry points

ONE_BIT_DIMS = (100, 129, 1600, 700, 1000, 1500, 1536)       # W 1 | run-time: w16 2 and 13 | 6 | 8 | 12, ragged and full
ONE_BIT_QUERY_BITS = (1, 2, 4, 8)
MULTI_BIT = ((2, 768), (2, 1000), (4, 384), (4, 500), (2, 100), (8, 64), (4, 96))   # per row width: W 12 and 16, then the run-time widths (8-bit rows have no other)
MULTI_BIT_QUERY_BITS = (4, 8)
ONE_BIT_W = (1, 6, 8, 12)                  # the row widths with a compiled kernel; every other width is W = 0, the run-time width
MULTI_BIT_W = (12, 16)
FUSED_MAXSIM_W = (6, 8, 12)                # the fused MaxSim kernel: 1-bit rows, 4 planes, these widths

Cell = collections.namedtuple("Cell", "index_bits dim query_bits sim")


def store_bits_of(index_bits):
    return 1 if index_bits == 1 else 2 if index_bits == 2 else 4 if index_bits <= 4 else 8


def w16_of(index_bits, dim):
    """16-byte chunks of a stored row: ceil(ceil(dim * store_bits / 8) / 16)"""
    return ((dim * store_bits_of(index_bits) + 7) // 8 + 15) // 16


def planes_of_values(index_bits, query_bits, qq):
    """what the library's planes_of_call makes of quantized query values: 1-bit rows - the bit-planes their OR needs (1 for a 1-bit
    query); 2- and 4-bit rows - QB 4 while no value exceeds 15, else 8; 8-bit rows - 8"""
    sb = store_bits_of(index_bits)
    if sb == 8:
        return 8
    if sb > 1:
        return 4 if int(np.max(qq)) <= 15 else 8
    if query_bits == 1:
        return 1
    m = int(np.bitwise_or.reduce(np.asarray(qq, np.uint8).ravel()))
    return 1 if m <= 1 else 2 if m <= 3 else 4 if m <= 15 else 8


def compiled(cell):
    """(store_bits, planes or QB, W) of the kernel the launchers pick for the cell; W = 0 is the run-time width"""
    sb = store_bits_of(cell.index_bits)
    w16 = w16_of(cell.index_bits, cell.dim)
    if sb == 1:
        return sb, cell.query_bits, w16 if w16 in ONE_BIT_W else 0
    if sb == 8:
        return sb, 8, 0
    return sb, 4 if cell.query_bits <= 4 else 8, w16 if w16 in MULTI_BIT_W else 0


def w_class(cell):
    """the classes every similarity and both statuses have to meet: 1-bit rows per W, multi-bit rows per W"""
    sb, _, w = compiled(cell)
    return ("1-bit" if sb == 1 else "multi-bit", w)


def fused_maxsim_exists(cell):
    sb, planes, w = compiled(cell)
    return sb == 1 and planes == 4 and w in FUSED_MAXSIM_W


def _cells():
    """the similarity rotates within each W class, so that every class meets all three (the order of MULTI_BIT keeps COSINE, whose
    max((1 + t) / 2, 0) clamps the rows an overstated dot product sends below -1, off the 4- and 8-bit rows at queryBits 8)"""
    plain = [(1, d, q) for d in ONE_BIT_DIMS for q in ONE_BIT_QUERY_BITS] + [(ib, d, q) for ib, d in MULTI_BIT for q in MULTI_BIT_QUERY_BITS]
    seen = collections.Counter()
    out = []
    for ib, d, q in plain:
        cls = w_class(Cell(ib, d, q, 0))
        out.append(Cell(ib, d, q, seen[cls] % 3))
        seen[cls] += 1
    return tuple(out)


CELLS = _cells()
# a cell whose default seed fails a condition of tests/test_rowlist_cells_cpu.py gets another one here (both: a threshold of a query
# whose three best rows the filter rejects, or whose median is the clamped 0.0)
SEEDS = {Cell(1, 129, 8, 0): 8000, Cell(4, 96, 4, 1): 8004}


def cell_id(cell):
    return "ib%d_%dd_qb%d_%s" % (cell.index_bits, cell.dim, cell.query_bits, ("euc", "cos", "mip")[cell.sim])


def seed_of(cell):
    return SEEDS.get(cell, 7000 + CELLS.index(cell))


def one_cell_per_w():
    """the first cell of every W class that runs the most kernels: 4 planes on 1-bit rows (the fused MaxSim kernel where it exists),
    QB 8 on multi-bit rows"""
    out = {}
    for c in CELLS:
        if c.query_bits == (4 if c.index_bits == 1 else 8):
            out.setdefault(w_class(c), c)
    return tuple(out.values())


# ------------------------------------------------------------------------------------------------ the inputs every cell shares

@functools.lru_cache(maxsize=None)
def accept_mask():
    """the filter of every filtered call: a random half that also rejects one whole tile (rows 128..191) and accepts only the first six
    rows of the last, partial tile (1088..1099)"""
    m = np.random.default_rng(4242).random(N) < 0.5
    m[128:192] = False
    m[1088:1094] = True
    m[1094:] = False
    m.setflags(write=False)
    return m


def ord_list():
    """a list that crosses rows 63/64, 511/512, 1023/1024 and 1087/1088 in descending order, holds repeats and ends on n - 1"""
    rng = np.random.default_rng(4243)
    desc = [N - 1, 1088, 1087, 1024, 1023, ONES_ROW, 705, 512, 511, ZERO_ROW, 205, 64, 63, 0]
    return np.ascontiguousarray(np.concatenate([desc, [63, 63, 1088, 205], rng.integers(0, N, 40), [N - 1]]), np.int32)


def span_lists():
    """one span over everything; spans that start and end in the middle of a tile, across both chunk edges, with an empty span between
    them; an empty span alone"""
    return [np.array(s, np.int64).reshape(-1, 2) for s in ([(0, N)], [(37, 530), (530, 530), (1000, 1097)], [(450, 450)])]


SPAN_KS = (1, 10)                          # and L + 1 of every list that visits a row
GROUP_KS = (1, 3)                          # and L + 1
GROUP_LAYOUTS = ("groups_of_65", "random_1_20", "across_two_edges")


@functools.lru_cache(maxsize=None)
def group_layouts():
    """groups of 65 rows, of 1 to 20 rows, and [0, 500) with [500, 1100) - a group over both chunk edges; read-only"""
    import test_groups_cpu as GC
    lays = dict(GC.layouts(N))
    lays.update(GC.chunk_edge_layouts(N))
    out = {k: lays[k] for k in GROUP_LAYOUTS}
    for off in out.values():
        off.setflags(write=False)
    return out


def thresholds_of(s32):
    """-inf, the 3rd-largest score, the median, and the float above the maximum"""
    srt = np.sort(np.asarray(s32, np.float32))
    return np.array([-np.inf, srt[-3], srt[len(srt) // 2], np.nextafter(srt[-1], np.float32(np.inf))], np.float32)


# ------------------------------------------------------------------------------------------------ one cell's index and expected scores

def _code_sums(codes, index_bits):
    return (np.unpackbits(codes, axis=1).sum(axis=1) if index_bits == 1 else codes.sum(axis=1, dtype=np.int64)).astype(np.float64)


def oracle_scores(cell, codes, corr, qq, qc, cdp):
    """(qcDist, f64 score, f32 score) of every row for one query: the reference's scorer, and for the multi-bit rows at queryBits 8 -
    which the reference refuses - the documented per-row 4-bit form"""
    if cell.index_bits > 1 and cell.query_bits == 8:
        return O.score_all_multibit_ext(codes, corr, cell.dim, qq, qc, cell.query_bits, cell.sim, cdp)
    return O.score_all(codes, corr, cell.dim, qq, qc, cell.query_bits, cell.sim, cdp, cell.index_bits)


def query_sources():
    """the rows the queries are noisy copies of: the one-vector queries' are rows the filter accepts, outside the tie runs and the
    planted rows; the remaining token vectors' are a seeded draw"""
    mask = accept_mask()
    taken = set(range(TIE_RUNS[0], TIE_RUNS[0] + TIE_LEN)) | set(range(TIE_RUNS[1], TIE_RUNS[1] + TIE_LEN)) | {ZERO_ROW, ONES_ROW}
    first = [next(r for r in range(start, N) if mask[r] and r not in taken) for start in (40, 600, 1050)]
    rest = np.random.default_rng(4244).integers(0, N, N_QUERIES - N_SINGLE)
    return np.concatenate([first, rest]).astype(np.int64)


def inflation(cell):
    """how far the reference's formulas overstate a dot product: the interval of a multi-bit row is not divided by its 2^bits - 1
    steps, and an 8-bit query is scaled as a 4-bit one (oracle/bbq_oracle.c, orc_score_single_row)"""
    f = ((1 << cell.index_bits) - 1) * (17 if cell.query_bits == 8 else 1)
    return f * 64 if cell.index_bits > 1 and cell.query_bits == 8 else f      # (there the formula's four terms no longer cancel either)


@functools.lru_cache(maxsize=None)
def case(cell):
    """(codes, corr, cdp, qq [33, dim], qc [33, 4], per query (qcDist, f64, f32) of every row).  Seeded zero-mean rows and queries that
    are noisy copies of some of them, both through the product's quantizer.  Their length is 1 / (2 sqrt(inflation)): short enough that
    max(1 / (1 + d), 0) never clamps an EUCLIDEAN score to 0, which would leave a bit-exact comparison little to bite on.  Then, in the
    quantized form bbq_index_create takes - which is all a kernel ever sees - the all-zero and the all-ones code at ZERO_ROW and
    ONES_ROW with their component sums (and intervals 1/64 of their donors': the codes of rows close to the centroid, which score
    inside the field and not off its scale), and query 0's best row copied over both tie runs.  Computed once, shared by every test,
    never written to"""
    rng = np.random.default_rng(seed_of(cell))
    sigma = 0.5 / np.sqrt(inflation(cell) * cell.dim)
    base = (sigma * rng.standard_normal((N, cell.dim))).astype(np.float32)
    queries = (base[query_sources()] + 0.5 * sigma * rng.standard_normal((N_QUERIES, cell.dim))).astype(np.float32)
    codes, corr, cen = B.quantize_vectors(base, cell.sim, cell.index_bits)
    cdp = B.centroid_dp(cen)
    qq, qc = B.quantize_queries(queries, cen, cell.sim, cell.query_bits)
    codes, corr = codes.copy(), corr.copy()
    top = (1 << cell.index_bits) - 1
    codes[ZERO_ROW] = 0
    codes[ONES_ROW] = np.packbits(np.ones(cell.dim, np.uint8)) if cell.index_bits == 1 else top
    for r, total in ((ZERO_ROW, 0), (ONES_ROW, cell.dim * top)):
        corr[r, 0:2] /= 64.0
        corr[r, 3] = total
    assert (corr[:, 3] == _code_sums(codes, cell.index_bits)).all()      # every row's sum is its code sum: the compact layout holds it
    s0 = oracle_scores(cell, codes, corr, qq[0], qc[0], cdp)[2].copy()
    s0[[ZERO_ROW, ONES_ROW]] = -np.inf
    best = int(np.argmax(s0))
    for b in TIE_RUNS:
        codes[b:b + TIE_LEN], corr[b:b + TIE_LEN] = codes[best], corr[best]
    scores = tuple(oracle_scores(cell, codes, corr, qq[i], qc[i], cdp) for i in range(N_QUERIES))
    for a in (codes, corr, qq, qc) + tuple(x for s in scores for x in s):
        a.setflags(write=False)
    return codes, corr, cdp, qq, qc, scores
