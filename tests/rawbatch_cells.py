"""The matrix of bbq_search_raw_batch on the matrix-core shared sweep (sweep_share 32, bbq_scan_mfma_kernel): which cells there are, which
of the sweep's forms each one runs, and the seeded inputs of every cell.  Numpy and the host side of the library only (the quantizer,
the oracle): nothing here touches a device.  tests/test_rawbatch_cells_cpu.py holds the inputs to the conditions that make the cells
bite; tests/test_gpu_rawbatch_sweeps.py runs every cell.

A cell is (dim, query_bits, sim).  The form of its sweep - FP6 x FP4 with a factor S of 1, 1/2 or 1/4 on every query value, or int8 -
is form_of(query_bits), which restates two host lines:

    search_batch_impl (csrc/bbq_core.cpp), a call with a feed:   c.maxq = (1 << query_bits) - 1;
    stage_queries_mfma (csrc/bbq_query.cpp):                     m.fp = c.maxq <= 15;  m.scale8 = c.maxq <= 3 ? 8 : c.maxq <= 7 ? 4 : 2;

(S = scale8 / 8).  A call without a feed has maxq 15 for every query of at most four planes, so S = 1/2 and S = 1 are reached through
the pipelined raw-query path alone: bbq_search_raw_batch with more than 64 queries.  If either line changes, the cells stop reaching
the forms they are named after.

The rows of a cell.  Seeded zero-mean fp32 rows through the product's quantizer, so the padding bits of a ragged row are what the
product writes and every row's quantizedComponentSum is its popcount (the compact layout holds it).  The first segment of a call with
first_segment_rows 1024 and k = 10 is max(1024, 4 (k + 1) rounded up to 512) = 1024 rows (start_plan, csrc/bbq_core.cpp): rows
[0, 1024) are listed whole, everything behind them is swept on the matrix cores.  Every query is a noisy copy of a source row at or
beyond BEYOND = 2048, as rowlist_cells.case makes them.

The order of the rows.  The reference scales every query of 2 to 8 bits as a 4-bit one, and a row's EUCLIDEAN score leans on its own
length: at most widths a score says more about the row than about its closeness to the query.  Left where they fall, a third of every
answer stands in front of BEYOND, and the rows that beat most queries' thresholds crowd single tiles - four of them in one tile are
128 (row, query) pairs for a group of 32 queries, all that a wave's survivor queue holds (QUEUE): the query is flagged and answered by
a fallback, in the raw call and in its bbq_search_batch twin alike.  No other seed mends what one query in twenty-five, or one cell in
three, fails.  So the QUANTIZED rows are put in another order, which changes no row's codes, corrections or score, and leaves the
centroid the one the quantizer returned (and the raw call gets):
  * every row among some query's K + 1 best that stands in front of BEYOND changes places with a row behind it that is nobody's;
  * the rows of [FIRST_SEGMENT, BEYOND) and of [BEYOND, N) are dealt out over the tiles of their range like cards, the rows that
    beat the most queries' thresholds first, and every tile's rows then stand at seeded places inside the tile: the sweep recovers
    a survivor's dot product per register group (rows 0..31 and 32..63 of a tile) and per lane, and the answers have to come from
    all of them, the 56-row last tile included (test_the_answers_stand_all_over_the_tiles).
A larger signal does not do instead: with NEIGHBOURS - eleven noisy copies of every source row - some queries' own source rows still
ranked in the hundreds at queryBits 2, 3 and 7, and a shorter sigma scales signal and row term alike.
A query's K best rows are then rows the matrix cores found, the threshold the dense prefix leaves is that of 1024 rows without any
query's best, and the survivors spread over the tiles (crowd_of: what test_rawbatch_cells_cpu.py holds below the queue)."""
import collections
import functools

import numpy as np

import orclib as O
from bbqlib import bbq_amd as B

N = 6200                                   # twelve chunks of 512 rows and a 56-row tail: its last tile holds 56 rows
NQ = 70                                    # more than 64 raw queries: the feed is used; three groups of 32, the last one of 6
K = 10
CHUNK, TILE = 512, 64
FIRST_SEGMENT = 1024                       # start_plan's s0 for first_segment_rows 1024 and k_dev = K + 1
BEYOND = 2048                              # the source rows, and every row of an answer, lie at or beyond this row

DIMS = (100, 128, 700, 768, 1000, 1024, 1500, 1536)          # W 1 | 6 | 8 | 12: a dimension that leaves the last 32-dimension word partly empty, one that fills the row
QUERY_BITS = (1, 2, 3, 4, 7)                                  # S = 1, 1, 1/2, then 1/4 through the feed, then int8 (maxq 127)
W_CLASSES = (1, 6, 8, 12)
SIMS = (0, 1, 2)
OPTIONS = (("sweep_share", 32), ("first_segment_rows", 1024), ("segment_growth", 4))     # of every index the GPU module opens

Cell = collections.namedtuple("Cell", "dim query_bits sim")


def w16_of(dim):
    """16-byte chunks of a stored 1-bit row"""
    return ((dim + 7) // 8 + 15) // 16


def is_ragged(dim):
    return dim % 32 != 0


def form_of(query_bits):
    """("fp", S) or ("int8", 1): the form of the matrix-core sweep a raw call of this bit width runs (None: it has none)"""
    maxq = (1 << query_bits) - 1
    if maxq > 127:
        return None
    if maxq > 15:
        return ("int8", 1)
    scale8 = 8 if maxq <= 3 else 4 if maxq <= 7 else 2
    return ("fp", scale8 / 8)


def form_w(cell):
    return form_of(cell.query_bits), w16_of(cell.dim)


CELLS = tuple(Cell(d, q, s) for d in DIMS for q in QUERY_BITS for s in SIMS)         # the compact layout runs them all


def _rotation():
    """one similarity per (dim, query_bits), rotating inside each (form, W) - and where a (form, W) has only two (dim, query_bits), the
    second one takes the third similarity as well, so that every (form, W) meets all three"""
    by_class = collections.OrderedDict()
    for d in DIMS:
        for q in QUERY_BITS:
            by_class.setdefault(form_w(Cell(d, q, 0)), []).append((d, q))
    out = []
    for pairs in by_class.values():
        for i, (d, q) in enumerate(pairs):
            out.append(Cell(d, q, i % 3))
        for s in range(len(pairs), 3):
            out.append(Cell(pairs[-1][0], pairs[-1][1], s))
    order = {c: i for i, c in enumerate(CELLS)}
    return tuple(sorted(out, key=order.get))


INLINE_CELLS = _rotation()


def _hostile_rotation():
    """one similarity per (dim, query_bits): in every (form, W) the first one is EUCLIDEAN - the similarity under which a huge
    additional correction does not saturate the best scores - and the others alternate between the two remaining ones"""
    by_class = collections.OrderedDict()
    for d in DIMS:
        for q in QUERY_BITS:
            by_class.setdefault(form_w(Cell(d, q, 0)), []).append((d, q))
    out = []
    for n, pairs in enumerate(by_class.values()):
        for i, (d, q) in enumerate(pairs):
            out.append(Cell(d, q, 0 if i % 3 == 0 else 1 + (i + n) % 2))
    order = {c: i for i, c in enumerate(CELLS)}
    return tuple(sorted(out, key=order.get))


HOSTILE_CELLS = _hostile_rotation()
K_DEEP = 200                               # the hostile cells' second k: behind the rows whose corrections saturate a score
# a cell whose default seed fails a condition of tests/test_rawbatch_cells_cpu.py gets another one here
SEEDS = {}


def cell_id(cell):
    return "%dd_qb%d_%s" % (cell.dim, cell.query_bits, ("euc", "cos", "mip")[cell.sim])


def seed_of(cell):
    """(a cell outside the matrix - the shapes without a matrix-core form - has a seed as well)"""
    return SEEDS.get(cell, 9000 + CELLS.index(cell) if cell in CELLS else 20000 + 100 * cell.dim + 3 * cell.query_bits + cell.sim)


# ------------------------------------------------------------------------------------------------ one cell's rows, queries and answers

def sources(seed):
    """the NQ rows the queries are noisy copies of: distinct rows at or beyond BEYOND"""
    return (BEYOND + np.random.default_rng(seed).permutation(N - BEYOND)[:NQ]).astype(np.int64)


def inflation(query_bits):
    """how far the reference's formulas overstate a dot product of a query of more than four bits: it is scaled as a 4-bit one
    (oracle/bbq_oracle.c; rowlist_cells.inflation)"""
    return max(1.0, ((1 << query_bits) - 1) / 15.0)


Case = collections.namedtuple("Case", "codes corr cen cdp queries qq qc top want moved crowd")
QUEUE = 128                                # survivors a wave of the matrix-core sweep holds per tile and group of 32 queries (kMfmaQueueCapTwo)


def crowd_of(s32):
    """the most (row, query) pairs of one 64-row tile behind the dense prefix and one group of 32 queries whose score beats the query's
    threshold there - the K + 1 best score of the prefix: what the sweep's survivor queue has to hold at the least"""
    s = np.asarray(s32)
    theta = np.sort(s[:, :FIRST_SEGMENT], axis=1)[:, -(K + 1)]
    above = s[:, FIRST_SEGMENT:] > theta[:, None]
    tiles = -(-above.shape[1] // TILE)
    above = np.concatenate([above, np.zeros((NQ, tiles * TILE - above.shape[1]), bool)], axis=1).reshape(NQ, tiles, TILE).sum(axis=2)
    return int(max(above[g:g + 32].sum(axis=0).max() for g in range(0, NQ, 32)))


def _score(cell, codes, corr, cdp, qq, qc):
    return [O.score_all(codes, corr, cell.dim, qq[q], qc[q], cell.query_bits, cell.sim, cdp)[2] for q in range(NQ)]


def _answers(s32, k=K):
    """per query the k + 1 best f32 scores, and (ords, scores) of the oracle's heap for k"""
    return np.array([np.sort(s)[::-1][:k + 1] for s in s32]), tuple(O.heap_topk(s, k) for s in s32)


@functools.lru_cache(maxsize=None)
def case(cell):
    """Case(codes, corr, cen, cdp, queries [NQ, dim] fp32, qq [NQ, dim], qc [NQ, 4], top [NQ, K + 1], want, moved): computed once,
    read-only, shared by both layouts.  The rows' length is that of rowlist_cells.case: short enough that max(1 / (1 + d), 0) clamps no
    EUCLIDEAN score to 0.  `moved` is the number of quantized rows that changed places with a row behind BEYOND (module docstring),
    `crowd` is crowd_of the final order"""
    rng = np.random.default_rng(seed_of(cell))
    src = sources(seed_of(cell))
    sigma = 0.5 / np.sqrt(inflation(cell.query_bits) * cell.dim)
    base = (sigma * rng.standard_normal((N, cell.dim))).astype(np.float32)
    queries = (base[src] + 0.5 * sigma * rng.standard_normal((NQ, cell.dim))).astype(np.float32)
    codes, corr, cen = B.quantize_vectors(base, cell.sim, 1)
    assert (corr[:, 3] == np.unpackbits(codes, axis=1).sum(axis=1)).all()        # every row's sum is its popcount: the compact layout holds it
    cdp = B.centroid_dp(cen)
    qq, qc = B.quantize_queries(queries, cen, cell.sim, cell.query_bits)
    s32 = _score(cell, codes, corr, cdp, qq, qc)
    assert not any(np.isnan(s).any() for s in s32), "a NaN among the oracle's scores of a benign cell"
    s32 = np.array(s32)
    # the rows among some query's K + 1 best that stand in front of BEYOND change places with rows behind it that are nobody's
    hot = np.unique(np.argsort(-s32, axis=1, kind="stable")[:, :K + 1])
    front = hot[hot < BEYOND]
    cold = rng.permutation(np.setdiff1d(np.arange(BEYOND, N), np.concatenate([hot, src])))[:len(front)]
    order = np.arange(N)
    order[front], order[cold] = cold, front
    # ... and the rows of [FIRST_SEGMENT, BEYOND) and of [BEYOND, N) are dealt out over the tiles of their range, the rows that beat the
    # most queries' thresholds first
    theta = np.sort(s32[:, order[:FIRST_SEGMENT]], axis=1)[:, -(K + 1)]
    for lo, hi in ((FIRST_SEGMENT, BEYOND), (BEYOND, N)):
        rows = order[lo:hi]
        heat = (s32[:, rows] > theta[:, None]).sum(axis=0)
        places = np.arange(lo, hi)
        places = places[np.lexsort((places // TILE, places % TILE))]          # every tile's first row, then every tile's second, ...
        order[places] = rows[np.argsort(-heat, kind="stable")]
        for t in range(lo, hi, TILE):                                         # ... each tile's rows at seeded places inside the tile
            order[t:min(t + TILE, hi)] = rng.permutation(order[t:min(t + TILE, hi)])
    codes, corr = codes[order], corr[order]
    s32 = s32[:, order]
    top, want = _answers(s32)
    crowd = crowd_of(s32)
    for a in (codes, corr, cen, queries, qq, qc, top) + tuple(x for w in want for x in w):
        a.setflags(write=False)
    return Case(codes, corr, cen, cdp, queries, qq, qc, top, want, len(front), crowd)


def scores_of(cell, corr=None):
    """every query's f32 scores of every row (not kept: the tests of one cell that need more than K answers ask for them)"""
    c = case(cell)
    return _score(cell, c.codes, c.corr if corr is None else corr, c.cdp, c.qq, c.qc)


def hostile_corrections(cell):
    """the cell's corrections with a tenth of the rows given the recipe of tests/test_gpu_filtered_mfma.py::_rows - zero, negative and
    f32-lost interval widths, 1e300, 3e38, -1e-320, additional corrections of about 1e4; corr[:, 3] stays.  Returns (corr, the rows
    no threshold can bound)"""
    rng = np.random.default_rng(seed_of(cell) + 100000)
    corr = case(cell).corr.copy()
    h = rng.choice(N, N // 10, replace=False)
    m = len(h) // 12
    scale = 10.0 ** rng.uniform(-6, 3, len(h))
    corr[h, 0] = -scale * rng.uniform(0.1, 1.0, len(h))
    corr[h, 1] = scale * rng.uniform(0.1, 1.0, len(h))
    corr[h[:m], 1] = corr[h[:m], 0]                                       # zero width
    corr[h[m:2 * m], 1] = corr[h[m:2 * m], 0] - 0.01                      # negative width
    corr[h[2 * m:3 * m], 1] = corr[h[2 * m:3 * m], 0] * (1 - 2.0 ** -30)  # a width lost in f32
    corr[h[3 * m:3 * m + 100], 1] = 1e300                                 # overflows f32
    corr[h[3 * m + 100:3 * m + 200], 2] = 3.0e38
    corr[h[3 * m + 200:3 * m + 300], 0] = -1e-320                         # f64 subnormal
    corr[h[3 * m + 300:4 * m + 300], 2] = rng.standard_normal(m) * 1e4
    assert 4 * m + 300 <= len(h)
    return corr, h[:3 * m + 300]


HostileCase = collections.namedtuple("HostileCase", "corr weird want deep nan")


@functools.lru_cache(maxsize=None)
def hostile(cell):
    """HostileCase(corr, weird rows, want for K, want for K_DEEP, whether a score is NaN) over the codes and queries of case(cell).
    Under COSINE and MAXIMUM_INNER_PRODUCT the K best of every query are rows whose additional correction of 3e38 saturates the score;
    K_DEEP reaches past them and past the rows with corrections of about 1e4, to scores that depend on the dot product"""
    c = case(cell)
    corr, weird = hostile_corrections(cell)
    assert (corr[:, 3] == c.corr[:, 3]).all()
    s32 = _score(cell, c.codes, corr, c.cdp, c.qq, c.qc)
    nan = any(bool(np.isnan(s).any()) for s in s32)
    want, deep = _answers(s32)[1], _answers(s32, K_DEEP)[1]
    for a in (corr, weird) + tuple(x for w in want + deep for x in w):
        a.setflags(write=False)
    return HostileCase(corr, weird, want, deep, nan)
