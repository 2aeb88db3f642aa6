"""A seeded walk over the mutations of the device-resident fp32 row store (bbq_vectors_*), and the model it is held to.  Pure numpy: no
device, no library.

include/bbq.h promises that a mutated handle is indistinguishable from one created whole over the resulting rows, so the whole state of a
bbq_vectors over a pool of rows is `src` (row i of the handle holds pool row src[i]).  VectorsModel restates the header's rule for every
operation and, beside it, the capacity rule of append_vectors (bbq_rerank.cpp) - the capacity cannot be observed, but the walk aims at
it: an append that fits it exactly, and one that forces a reallocation.  walk() deals a deck: every append kind, every update kind, six
of the mask shapes (a different six per seed: three consecutive seeds hold all of them), every refusable call, in a shuffled order.  A
step that needs rows the handle does not have is preceded by an append, one that would take it beyond MAX_ROWS by a compaction: a step's
"op" is always what it is.  tests/test_vectors_walk_cpu.py asserts what the default walks cover; tests/test_gpu_vectors_walk.py plays
them on the device.

The pool of a width is frozen: standard-normal rows, and hostile FINITE rows - f32 subnormals, FLT_MIN and +-FLT_MAX beside ordinary
values, zeros, -0.0, one non-zero entry in the last column, exact duplicates.  Finite, because the device test reads every element
back as the MAXIMUM_INNER_PRODUCT score of a one-hot query, float64(row[j]) + 0.0, and 0 * Infinity is a NaN.  Rows are drawn with
replacement, half of the time from a hot set that holds every hostile row."""
import numpy as np

TILE, MAX_ROWS, MIN_COMPACT_ROWS = 64, 1500, 330
DEFAULT_SEEDS = 3   # BBQ_VECTORS_WALK_SEEDS asks the device test for more
# the smallest widths on both sides of: the 16-byte and the 4-byte copy path (dim % 4), one trip and several of each copy loop (64 lanes x
# 4 bytes: 63 | 65 | 129; 64 lanes x 16 bytes: 256 | 260, and 768 is three trips), the 32-column stage of the readers (5 | 63, 65)
WIDTHS = (1, 3, 4, 5, 63, 65, 129, 256, 260, 768)
EXACT_COLUMNS = 64   # one-hot columns a step reads back through the exact search
N_NORMAL = 200
HOSTILE = ("subnormal", "extreme", "zero", "negative_zero", "last_column", "duplicate_a", "duplicate_b", "duplicate_c")
DUPLICATED = 3       # the pool row the duplicates copy

APPENDS = ("append_0", "append_1", "append_exact", "append_realloc", "append_random", "append_random")
UPDATES = ("update_duplicates", "update_shuffled", "update_edges", "update_empty")
REFUSALS = ("refuse_update", "refuse_compact", "refuse_append")
# the shapes tests/test_gpu_compact.py::masks_of names, and behind them the ones it leaves out
MASK_SHAPES = ("keep_all", "keep_none", "only_row_0", "only_last_row", "partial_last_tile", "exactly_63", "exactly_64", "exactly_65",
               "tiles_0_3_last_full_rejected", "alternating", "every_10th", "middle_block", "random_90", "random_50",
               "first_tile_out", "middle_tiles_out", "drop_row_0")
MASKS_PER_WALK = 6


def hostile_row(name):
    return N_NORMAL + HOSTILE.index(name)


def pool(dim):
    """the frozen rows of one width: float32 [N_NORMAL + len(HOSTILE), dim]"""
    rng = np.random.default_rng([20261, dim])
    p = np.zeros((N_NORMAL + len(HOSTILE), dim), np.float32)
    p[:N_NORMAL] = rng.standard_normal((N_NORMAL, dim)).astype(np.float32)
    c = np.arange(dim)
    tiny = np.float32(2.0 ** -149)
    sub = (rng.standard_normal(dim) * 1e-42).astype(np.float32)
    sub[c % 3 == 0], sub[c % 3 == 1] = tiny, -tiny
    p[hostile_row("subnormal")] = sub
    fmax, fmin = np.finfo(np.float32).max, np.finfo(np.float32).tiny
    ext = rng.standard_normal(dim).astype(np.float32)
    ext[c % 4 == 0], ext[c % 4 == 1], ext[c % 4 == 2] = fmin, fmax, -fmax
    p[hostile_row("extreme")] = ext
    p[hostile_row("negative_zero")] = np.float32(-0.0)
    p[hostile_row("last_column"), dim - 1] = np.float32(1.5)
    for name in ("duplicate_a", "duplicate_b", "duplicate_c"):
        p[hostile_row(name)] = p[DUPLICATED]
    assert np.isfinite(p).all()
    p.setflags(write=False)
    return p


def exact_columns(seed, i, dim):
    """the one-hot columns step i of a walk reads back through the exact search: column 0, column dim - 1 and a window that moves on
    with every step, so that one walk passes over every column"""
    if dim <= EXACT_COLUMNS:
        return np.arange(dim)
    w = EXACT_COLUMNS - 2
    return np.unique(np.concatenate([[0, dim - 1], (i * w + seed * (w // 2) + np.arange(w)) % dim]))


class VectorsModel:
    """a bbq_vectors over a pool of rows, as include/bbq.h describes it, and its capacity in rows as append_vectors keeps it"""

    def __init__(self, rows):
        self.src = np.array(rows, np.int64).ravel()
        self.cap = len(self.src)   # a creation is an append to an empty buffer: exactly its rows

    @property
    def size(self):
        return len(self.src)

    def append(self, rows):
        """new rows get the next ords; an append that does not fit moves the rows into max(rows needed, 1.5 x rows held)"""
        self.src = np.concatenate([self.src, np.asarray(rows, np.int64).ravel()])
        if self.cap < len(self.src):
            self.cap = max(len(self.src), self.cap * 3 // 2)

    def update(self, ords, frm):
        """applied entry by entry: the last of equal ords wins.  Returns the positions that took effect, ascending by ord."""
        last = {}
        for i, o in enumerate(ords):
            if not 0 <= int(o) < len(self.src):
                raise IndexError("ord %d outside [0, %d)" % (int(o), len(self.src)))
            self.src[int(o)] = frm[i]
            last[int(o)] = i
        return np.array([last[o] for o in sorted(last)], np.int64)

    def compact(self, mask):
        """the rows the mask accepts, in order, in a buffer of exactly that many rows; every row kept: nothing changes"""
        mask = np.asarray(mask, bool)
        assert mask.shape == self.src.shape
        if mask.all():
            return
        self.src = self.src[mask]
        self.cap = len(self.src)


def apply(model, step):
    """play one step on a model; a refused step leaves everything as it was"""
    op = step["op"]
    if op == "append":
        model.append(step["rows"])
    elif op == "update":
        model.update(step["ords"], step["frm"])
    elif op == "compact":
        model.compact(step["mask"])
    elif op not in REFUSALS:
        raise ValueError(op)


def describe(step):
    """one line that lets a failure be replayed as a fixed sequence"""
    def short(a):
        a = [int(v) for v in a]
        return str(a) if len(a) <= 12 else "[%s, ... %d entries ..., %s]" % (", ".join(map(str, a[:6])), len(a), ", ".join(map(str, a[-3:])))

    parts = [step["op"], step.get("shape", "")]
    if "ords" in step:
        parts.append("ords=" + short(step["ords"]))
    if "frm" in step:
        parts.append("from=" + short(step["frm"]))
    if "mask" in step:
        parts.append("kept=%s padding_bits=%d" % (short(np.flatnonzero(step["mask"])), step["padding"]))
    if "rows" in step:
        parts.append("rows=" + short(step["rows"]))
    if "bad" in step:
        parts.append("bad=%s" % (step["bad"],))
    return " ".join(p for p in parts if p)


def mask_of(shape, n, rng):
    """one mask over n rows; the first fourteen shapes as tests/test_gpu_compact.py::masks_of builds them"""
    r = np.arange(n)
    full, tiles = n // TILE, (n + TILE - 1) // TILE
    if shape == "keep_all":
        return np.ones(n, bool)
    if shape == "keep_none":
        return np.zeros(n, bool)
    if shape == "only_row_0":
        return r == 0
    if shape == "only_last_row":
        return r == n - 1
    if shape == "partial_last_tile":
        return r >= (n - 1) // TILE * TILE
    if shape.startswith("exactly_"):
        cnt = int(shape[8:])
        return np.isin(r, np.round(np.linspace(0, n - 1, min(cnt, n))).astype(np.int64))
    if shape == "tiles_0_3_last_full_rejected":
        return ~np.isin(r // TILE, [0, 3, full - 1])
    if shape == "alternating":
        return r % 2 == 1
    if shape == "every_10th":
        return r % 10 == 3
    if shape == "middle_block":
        return (r >= n // 3) & (r < 2 * n // 3)
    if shape == "random_90":
        return rng.random(n) < 0.9
    if shape in ("random_50", "shrink_random_50"):
        return rng.random(n) < 0.5
    if shape == "first_tile_out":       # the binary search's first rank is 0
        return r >= TILE
    if shape == "middle_tiles_out":     # a run of three to five whole tiles in front of the binary search's targets behind it
        assert tiles >= 6
        run = int(rng.integers(3, min(5, tiles - 2) + 1))
        t0 = int(rng.integers(1, tiles - run))
        return ~((r // TILE >= t0) & (r // TILE < t0 + run))
    if shape == "drop_row_0":
        return r != 0
    raise ValueError(shape)


def walk(seed, dim):
    """the steps of one walk over a handle of this width: a creation, then the deck in a shuffled order with what its items need put in
    front of them, and a closing block where the walk would end on a handful of rows"""
    rng = np.random.default_rng([seed, dim, 4711])
    pool_n = N_NORMAL + len(HOSTILE)
    hot = np.concatenate([np.arange(N_NORMAL, pool_n), rng.choice(N_NORMAL, 8, replace=False), [DUPLICATED]])

    def rows(count):
        if rng.random() < 0.5:
            return hot[rng.integers(0, len(hot), count)].astype(np.int64)
        return rng.integers(0, pool_n, count).astype(np.int64)

    shapes = [MASK_SHAPES[(seed * MASKS_PER_WALK + j) % len(MASK_SHAPES)] for j in range(MASKS_PER_WALK)]
    deck = list(APPENDS) + list(UPDATES) + list(REFUSALS) + ["compact:" + s for s in shapes]
    deck = [deck[int(i)] for i in rng.permutation(len(deck))]

    size0 = [0, 1, 63, 64, 65, 255, 256, 257, 1000][int(rng.integers(9))]
    out = [{"op": "create", "rows": rows(size0)}]
    m = VectorsModel(out[0]["rows"])
    compactions = 0

    def emit(step):
        apply(m, step)
        out.append(step)

    def append(shape, count):
        while m.size + count > MAX_ROWS:
            compact("shrink_random_50")
        emit({"op": "append", "shape": shape, "rows": rows(count)})

    def update(shape, ords):
        ords = np.array(ords, np.int64)
        emit({"op": "update", "shape": shape, "ords": ords, "frm": rows(len(ords))})

    def compact(shape):
        nonlocal compactions
        mask = np.asarray(mask_of(shape, m.size, rng), bool)
        # the bits of the last accept word beyond the last row, as the caller hands them over: set, or clear
        emit({"op": "compact", "shape": shape, "mask": mask, "padding": (seed + compactions) % 2})
        compactions += 1

    for item in deck:
        n = m.size
        if item.startswith("compact:"):
            if n < MIN_COMPACT_ROWS:
                append("refill", int(rng.integers(400, 900)))
            turn = compactions
            compact(item[8:])
            if m.size > 0 and turn % 2 == 0:   # an update of a buffer that holds exactly the kept rows
                k = m.size
                some = rng.integers(0, k, min(k, 20))
                update("after_compaction", np.concatenate([[0, k - 1], some, some[:3]]))
        elif item == "append_0":
            append(item, 0)
        elif item == "append_1":
            append(item, 1)
        elif item == "append_random":
            append(item, int(rng.integers(1, 400)))
        elif item == "append_realloc":
            if m.cap + 300 > MAX_ROWS:   # a compaction leaves a capacity of exactly the kept rows
                compact("shrink_random_50")
            append(item, m.cap - m.size + int(rng.integers(1, 300)))
        elif item == "append_exact":
            if n > 1000 or m.cap > MAX_ROWS:
                compact("shrink_random_50")
            if m.size < 4:
                append("refill", int(rng.integers(400, 900)))
            if m.cap == m.size:   # one row beyond the capacity leaves room for half as many again
                append("one_beyond_capacity", 1)
            assert m.cap > m.size
            update("with_spare_capacity", rng.integers(0, m.size, 9))
            append(item, m.cap - m.size)
            assert m.cap == m.size
        elif item in UPDATES:
            if n == 0 and item != "update_empty":
                append("refill", int(rng.integers(400, 900)))
                n = m.size
            if item == "update_duplicates":
                d = int(rng.integers(0, n))
                update(item, [0, d, n - 1, d, 1 % n, d])
            elif item == "update_shuffled":
                update(item, rng.permutation(n)[:max(1, n // 4)])
            elif item == "update_edges":
                update(item, [e for e in (0, 1, 63, 64, 65, 255, 256, 257) if e < n] + [n - 1])
            else:
                update(item, [])
        elif item == "refuse_update":   # an ord that no row has: -1, or the size
            count = int(rng.integers(1, 30))
            ords = rng.integers(0, max(n, 1), count).astype(np.int64)
            at = int(rng.integers(0, count))
            ords[at] = (-1, n)[seed % 2]
            emit({"op": item, "shape": "ord_%d_of_%d" % (ords[at], n), "ords": ords, "frm": rows(count), "bad": (at,)})
        elif item == "refuse_compact":  # a filter made for another row count
            other = n + (1, -1, TILE)[seed % 3]
            other = other if other >= 1 else n + 1
            emit({"op": item, "shape": "filter_for_%d_of_%d" % (other, n), "bad": (other,)})
        elif item == "refuse_append":   # rows of another width
            emit({"op": item, "shape": "width", "rows": rows(int(rng.integers(1, 5))), "bad": (dim + (1, 3, 4)[seed % 3],)})
        else:
            raise ValueError(item)
    if m.size < 200:   # no walk ends on a handful of rows, and none on an emptied handle
        emit({"op": "append", "shape": "closing_block", "rows": rows(257)})
    return out
