"""A seeded random walk over the mutations of a device-resident index, and the model it is held to.  Pure numpy: no device, no
library.

The model is a row list.  include/bbq.h promises that a mutated index is indistinguishable from one created whole over the resulting
rows, so the whole state of an index over a pool of rows is `src` (index row i holds pool row src[i]), its capacity in 64-row tiles
and whether its records store explicit component sums.  IndexModel restates the header's rule for every operation; walk() draws a
deterministic list of steps whose shapes are biased to the edges the single-mutation tests name (tile and chunk boundaries, the
partial last tile, duplicates, an update across the end of an append, an append that lands on the capacity and one row beyond it);
apply() plays a step on a model.  tests/test_mutation_walk_cpu.py asserts what the default walks cover; tests/test_gpu_mutation_walk.py
plays them on the device.

Rows are drawn from the pool WITH replacement, half of the time from a hot set of 24 rows: the index soon holds many copies of one
row, so exactly equal scores inside and at the edge of every answer are the norm.

One thing the walk never draws: a row whose quantizedComponentSum is not its code sum offered to an index that holds neither rows
nor room.  Such an index is the index of zero rows, and like one created over zero rows it decides its record format at its next
append, so there the row is not refused: include/bbq.h does not spell this exception out, and
tests/test_gpu_append.py::test_an_emptied_index_decides_its_format_like_one_created_over_zero_rows pins it as a fixed sequence."""
from collections import namedtuple

import numpy as np

TILE, CHUNK, MAX_ROWS, STEPS = 64, 512, 4096, 25
DEFAULT_SEEDS = 3   # per flavour; BBQ_WALK_SEEDS asks the device test for more
EDGES = (0, 1, 63, 64, 65, 511, 512, 513)
EUCLIDEAN, COSINE, MAXIMUM_INNER_PRODUCT = 0, 1, 2

KINDS = ("append_rows", "append", "update_rows", "update", "compact", "remove_rows", "reserve", "save_load")
FAIL_KINDS = ("fail_nan", "fail_inf", "fail_ord", "fail_code", "fail_sum")

# what the walk has to know of a pool: its row shape, and which of its rows carry a quantizedComponentSum that is not their code sum
# (an index created over one of them stores explicit sums; a raw row never reproduces one, so raw blocks avoid them)
Flavour = namedtuple("Flavour", "pool dim ib sim odd_rows")
FLAVOURS = {
    "seeded_1000x129": Flavour("seeded_1000x129", 129, 1, COSINE, ()),
    "ties_cos_qb4": Flavour("ties_cos_qb4", 64, 1, COSINE, ()),
    "ib2_100d_cos_qb4": Flavour("ib2_100d_cos_qb4", 100, 2, COSINE, ()),
    "ib4_96d_euc_qb4": Flavour("ib4_96d_euc_qb4", 96, 4, EUCLIDEAN, ()),
    "edge_dim1": Flavour("edge_dim1", 1, 1, MAXIMUM_INNER_PRODUCT, ()),
    "explicit_sums": Flavour("seeded_1000x129", 129, 1, COSINE, (7, 70, 200, 640, 999)),
}


def tiles_of(rows):
    return (int(rows) + TILE - 1) // TILE


def fail_kinds_of(fl):
    """the refusable kinds that exist for a flavour: an Infinity is reported as such only under EUCLIDEAN (COSINE normalises first),
    a code out of range needs multi-bit rows, and an index that stores explicit sums takes any sum"""
    kinds = ["fail_nan", "fail_ord"]
    if fl.sim == EUCLIDEAN:
        kinds.append("fail_inf")
    if fl.ib > 1:
        kinds.append("fail_code")
    if not fl.odd_rows:
        kinds.append("fail_sum")
    return tuple(k for k in FAIL_KINDS if k in kinds)


class IndexModel:
    """an index over a pool of rows, as include/bbq.h describes it"""

    def __init__(self, src, stores_sums):
        self.src = np.array(src, np.int64).ravel()
        self.cap_tiles = tiles_of(len(self.src))      # a creation allocates whole tiles of exactly its rows
        self.stores_sums = bool(stores_sums)          # decided once, at creation, and never again

    @property
    def size(self):
        return len(self.src)

    @property
    def capacity(self):
        return self.cap_tiles * TILE

    def append(self, rows):
        """new rows get the next ords; an append that does not fit moves the index into max(tiles needed, 1.5 x tiles held) tiles"""
        self.src = np.concatenate([self.src, np.asarray(rows, np.int64).ravel()])
        need = tiles_of(len(self.src))
        if need > self.cap_tiles:
            self.cap_tiles = max(need, self.cap_tiles + self.cap_tiles // 2)

    def reserve(self, rows):
        """room for exactly `rows` rows in total; never shrinks"""
        self.cap_tiles = max(self.cap_tiles, tiles_of(rows))

    def update(self, ords, frm):
        """applied entry by entry: the last of equal ords wins.  Size and capacity stay.  Returns the positions that took effect,
        ascending by ord."""
        last = {}
        for i, o in enumerate(ords):
            if not 0 <= int(o) < len(self.src):
                raise IndexError("ord %d outside [0, %d)" % (int(o), len(self.src)))
            self.src[int(o)] = frm[i]
            last[int(o)] = i
        return np.array([last[o] for o in sorted(last)], np.int64)

    def compact(self, mask):
        """the rows the mask accepts, in order, in whole tiles of exactly that many rows; every row kept: nothing changes"""
        mask = np.asarray(mask, bool)
        assert mask.shape == self.src.shape
        if mask.all():
            return
        self.src = self.src[mask]
        self.cap_tiles = tiles_of(len(self.src))

    def remove(self, rows):
        mask = np.ones(len(self.src), bool)
        for r in rows:
            if not 0 <= int(r) < len(self.src):
                raise IndexError("row %d outside [0, %d)" % (int(r), len(self.src)))
            mask[int(r)] = False
        self.compact(mask)

    def save_load(self):
        """a loaded index holds whole tiles of exactly its rows"""
        self.cap_tiles = tiles_of(len(self.src))


def apply(model, step):
    """play one step on a model; a failing step leaves everything as it was"""
    op = step["op"]
    if op in ("append_rows", "append"):
        model.append(step["rows"])
    elif op in ("update_rows", "update"):
        model.update(step["ords"], step["frm"])
    elif op == "compact":
        model.compact(step["mask"])
    elif op == "remove_rows":
        model.remove(step["rows"])
    elif op == "reserve":
        model.reserve(step["rows"])
    elif op == "save_load":
        model.save_load()
    elif op not in FAIL_KINDS:
        raise ValueError(op)


def describe(step):
    """one line that lets a failure be replayed as a fixed sequence"""
    def short(a):
        a = [int(v) for v in a]
        return str(a) if len(a) <= 12 else "[%s, ... %d entries ..., %s]" % (", ".join(map(str, a[:6])), len(a), ", ".join(map(str, a[-3:])))

    op = step["op"]
    parts = [op]
    if "shape" in step:
        parts.append(step["shape"])
    if "via" in step:
        parts.append("via " + step["via"])
    if "ords" in step:
        parts.append("ords=" + short(step["ords"]))
    if "frm" in step:
        parts.append("from=" + short(step["frm"]))
    if "mask" in step:
        parts.append("kept=" + short(np.flatnonzero(step["mask"])))
    if "rows" in step:
        parts.append("rows=" + (str(step["rows"]) if np.isscalar(step["rows"]) else short(step["rows"])))
    if "bad" in step:
        parts.append("bad=%s" % (step["bad"],))
    return " ".join(parts)


class _Draw:
    """the draws of one walk: every shape is a function of the model's state and the generator"""

    def __init__(self, rng, pool_n, fl, seed):
        self.rng, self.pool_n, self.fl, self.seed = rng, pool_n, fl, seed
        self.hot = rng.choice(pool_n, size=min(24, pool_n), replace=False)
        self.plain = np.setdiff1d(np.arange(pool_n), np.array(fl.odd_rows, np.int64))
        self.last_append = None     # (old end, rows) of the latest append, until the size changes otherwise
        self.last_updated = None    # the ords of the latest update, until another mutation follows

    def pick(self, options):
        return options[int(self.rng.integers(len(options)))]

    def pool_rows(self, count, raw=False):
        """rows of the pool with replacement, half of the time from the hot set; a raw block stays off the rows with odd sums"""
        rng = self.rng
        if rng.random() < 0.5:
            rows = self.hot[rng.integers(0, len(self.hot), count)]
        else:
            rows = rng.integers(0, self.pool_n, count)
        rows = np.asarray(rows, np.int64)
        if raw and self.fl.odd_rows:
            odd = np.isin(rows, self.fl.odd_rows)
            rows[odd] = self.plain[rng.integers(0, len(self.plain), int(odd.sum()))]
        return rows

    # ---------------------------------------------------------------------------------------------- appends
    def append_count(self, m):
        n, cap = m.size, m.capacity
        options = [("edge_%d" % c, c) for c in EDGES]
        to_tile, to_chunk = (n // TILE + 1) * TILE - n, (n // CHUNK + 1) * CHUNK - n
        options += [("to_tile_end", to_tile), ("past_tile_end", to_tile + 1), ("before_tile_end", to_tile - 1),
                    ("to_chunk_end", to_chunk), ("past_chunk_end", to_chunk + 1), ("before_chunk_end", to_chunk - 1),
                    ("random", int(self.rng.integers(1, 700))), ("random", int(self.rng.integers(1, 700)))]
        if cap > n:   # exactly on the capacity, and one row beyond it
            options += [("lands_on_capacity", cap - n)] * 3 + [("one_beyond_capacity", cap - n + 1)] * 3
        else:
            options += [("one_beyond_capacity", 1)] * 2
        if n == 0:    # an emptied index gets rows to go on with
            options = [("edge_%d" % c, c) for c in (1, 65, 513)] + [("random", int(self.rng.integers(100, 1200)))] * 3
        return self.pick(options)

    def append(self, m, op):
        shape, count = self.append_count(m)
        if m.size + count > MAX_ROWS:
            return None
        step = {"op": op, "shape": shape, "rows": self.pool_rows(count, raw=op == "append")}
        return step

    # ---------------------------------------------------------------------------------------------- updates
    def update_ords(self, m):
        n, rng = m.size, self.rng
        last_tile = (n - 1) // TILE * TILE
        options = [("row_0", [0]), ("last_row", [n - 1]), ("tile_edges", [e for e in EDGES[1:] if e < n] or [0]),
                   ("chunk_edges_from_end", [n - 1 - e for e in EDGES if e < n]),
                   ("partial_last_tile", list(range(last_tile, n))), ("every_10th", list(range(3 % n, n, 10))),
                   ("random_shuffled", list(rng.permutation(n)[:max(1, n // 4)])), ("empty", [])]
        t = int(rng.integers(0, tiles_of(n)))
        options.append(("whole_tile", list(range(t * TILE, min(n, (t + 1) * TILE)))))
        d = int(rng.integers(0, n))
        options += [("duplicates", [0, d, n - 1, d, 1 % n, d])] * 2
        some = rng.integers(0, n, 40)
        options.append(("duplicates_random", list(np.concatenate([some, some[:13][::-1]]))))
        if self.last_append is not None and self.last_append[0] > 0 and self.last_append[1] > 0:
            end, cnt = self.last_append   # across the old end, into rows that were just appended
            options += [("across_the_old_end", list(range(max(0, end - 3), min(n, end + 3))) + [end - 1])] * 4
        return self.pick(options)

    def update(self, m, op):
        shape, ords = self.update_ords(m)
        ords = np.array(ords, np.int64)
        return {"op": op, "shape": shape, "ords": ords, "frm": self.pool_rows(len(ords), raw=op == "update")}

    # ---------------------------------------------------------------------------------------------- compactions
    def compact_mask(self, m):
        n, rng = m.size, self.rng
        r = np.arange(n)
        options = [("partial_last_tile", r >= (n - 1) // TILE * TILE), ("only_last_row", r == n - 1), ("keep_none", np.zeros(n, bool)),
                   ("keep_all", np.ones(n, bool)), ("every_10th", r % 10 == 3), ("random_90", rng.random(n) < 0.9),
                   ("random_90", rng.random(n) < 0.9), ("random_50", rng.random(n) < 0.5), ("drop_row_0", r != 0), ("drop_last_row", r != n - 1)]
        for cnt in (63, 64, 65, 511, 512, 513):   # the destination's tile and chunk boundaries
            if cnt < n:
                options.append(("exactly_%d" % cnt, np.isin(r, np.round(np.linspace(0, n - 1, cnt)).astype(np.int64))))
        if n % TILE == 0 and n > 1:               # leave a partial last tile behind
            options.append(("drop_last_row", r != n - 1))
        if self.last_updated is not None and len(self.last_updated):   # rows of the tiles an update has just touched go
            drop = np.unique(self.last_updated)[::2]
            options += [("drop_updated", ~np.isin(r, drop))] * 4
        return self.pick(options)

    def compact(self, m):
        shape, mask = self.compact_mask(m)
        return {"op": "compact", "shape": shape, "mask": np.asarray(mask, bool)}

    def remove(self, m):
        n, rng = m.size, self.rng
        options = [("edges_with_duplicates", [e for e in EDGES if e < n] + [n - 1, 0, n - 1]),
                   ("random_with_duplicates", list(rng.integers(0, n, max(1, n // 8))) + [int(rng.integers(0, n))] * 2),
                   ("last_tile", list(range((n - 1) // TILE * TILE, n))), ("nothing", []), ("everything", list(rng.permutation(n)))]
        if self.last_updated is not None and len(self.last_updated):
            options += [("updated_rows", list(self.last_updated[::2]))] * 3
        shape, rows = self.pick(options)
        return {"op": "remove_rows", "shape": shape, "rows": np.array(rows, np.int64)}

    def shrink(self, m):
        """what a drawn append that would exceed MAX_ROWS becomes"""
        n = m.size
        keep = self.rng.random(n) < 0.3
        return {"op": "compact", "shape": "shrink_random_30", "mask": keep}

    # ---------------------------------------------------------------------------------------------- capacity
    def reserve(self, m):
        n, cap = m.size, m.capacity
        shape, rows = self.pick([("below_size", n // 2), ("the_capacity", cap), ("one_row_beyond", cap + 1), ("one_row_beyond", cap + 1),
                                 ("some_tiles_beyond", cap + TILE * int(self.rng.integers(1, 9))), ("a_chunk_beyond_the_size", n + CHUNK + 1)])
        return {"op": "reserve", "shape": shape, "rows": int(rows)}

    # ---------------------------------------------------------------------------------------------- refusals
    def fail(self, m, kind):
        n, rng, fl = m.size, self.rng, self.fl
        count = int(rng.integers(1, 71))
        turn = self.seed + FAIL_KINDS.index(kind)   # the ways of one kind take turns over the seeds, so none depends on luck
        by_update = n > 0 and turn % 2 == 0
        step = {"op": kind, "rows": self.pool_rows(count, raw=kind in ("fail_nan", "fail_inf"))}
        if by_update:
            step["ords"] = rng.integers(0, n, count).astype(np.int64)
        r = int(rng.integers(0, count))
        if kind in ("fail_nan", "fail_inf"):
            step["via"] = "update" if by_update else "append"
            step["bad"] = (r, int(rng.integers(0, fl.dim)))
            step["value"] = float("nan") if kind == "fail_nan" else float(self.pick([np.inf, -np.inf]))
        elif kind == "fail_ord":   # an ord equal to the size is not an append
            step["via"] = ("update_rows", "update", "remove_rows")[turn % 3]
            ords = rng.integers(0, n, count).astype(np.int64) if n > 0 else np.zeros(count, np.int64)
            ords[r] = n
            step["ords"], step["bad"] = ords, (r,)
            if step["via"] == "update":
                step["rows"] = self.pool_rows(count, raw=True)
        elif kind == "fail_code":  # a code equal to 2^indexBits; the sum stays the code sum
            step["via"] = "update_rows" if by_update else "append_rows"
            step["bad"] = (r, int(rng.integers(0, fl.dim)))
        elif kind == "fail_sum":   # a quantizedComponentSum that is not the code sum
            step["via"] = "update_rows" if by_update else "append_rows"
            step["bad"] = (r,)
        else:
            raise ValueError(kind)
        return step


def walk(seed, pool_n, flavour, steps=STEPS):
    """the steps of one walk: a creation, then `steps` operations - every kind twice, every refusable kind of the flavour once, the
    rest drawn - in a shuffled order.  An operation that needs rows on an empty index becomes an append, and a drawn append that
    would take the index beyond MAX_ROWS becomes a compaction: a step's "op" is always what it is, not what was drawn."""
    fl = FLAVOURS[flavour]
    rng = np.random.default_rng([seed, pool_n, sorted(FLAVOURS).index(flavour)])
    d = _Draw(rng, pool_n, fl, seed)
    fails = fail_kinds_of(fl)
    deck = list(KINDS) * 2 + list(fails)
    deck += [KINDS[int(i)] for i in rng.integers(0, len(KINDS), max(0, steps - len(deck)))]
    deck = [deck[int(i)] for i in rng.permutation(len(deck))]

    size0 = d.pick([0, 1, 63, 64, 65, 511, 512, 513, 1000, 1000])
    first = d.pool_rows(max(size0, 1) if fl.odd_rows else size0)
    if fl.odd_rows and not np.isin(first, fl.odd_rows).any():   # the starting index contains a row that needs explicit sums
        first[int(rng.integers(0, len(first)))] = d.pick(list(fl.odd_rows))
    out = [{"op": "create", "rows": np.array(first, np.int64)}]
    m = IndexModel(first, bool(fl.odd_rows))

    deck, at = list(deck), 0
    while at < len(deck):
        drawn, n = deck[at], m.size
        at += 1
        if drawn in FAIL_KINDS and n == 0 and (seed + FAIL_KINDS.index(drawn)) % 2 == 0 and any(k not in FAIL_KINDS for k in deck[at:]):
            deck.append(drawn)   # its turn is to go through an update, which an empty index cannot take: later
            continue
        if drawn in FAIL_KINDS:
            kind = drawn
            if kind == "fail_sum" and n == 0 and m.cap_tiles == 0:   # see the module's docstring
                kind = "fail_ord"
            step = d.fail(m, kind)
        elif drawn in ("append_rows", "append") or (n == 0 and drawn in ("update_rows", "update", "compact", "remove_rows")):
            op = drawn if drawn in ("append_rows", "append") else d.pick(["append_rows", "append"])
            step = d.append(m, op) or d.shrink(m)
        elif drawn in ("update_rows", "update"):
            step = d.update(m, drawn)
        elif drawn == "compact":
            step = d.compact(m)
        elif drawn == "remove_rows":
            step = d.remove(m)
        elif drawn == "reserve":
            step = d.reserve(m)
        else:
            step = {"op": "save_load"}
        before = m.size
        apply(m, step)
        op = step["op"]
        if op in ("append_rows", "append"):
            d.last_append, d.last_updated = (before, len(step["rows"])), None
        elif op in ("update_rows", "update"):
            d.last_updated = step["ords"] if len(step["ords"]) else d.last_updated
        elif op in ("compact", "remove_rows"):
            d.last_updated = None
            if m.size != before:
                d.last_append = None
        out.append(step)
    if m.size < 200:   # no walk ends on a handful of rows: the answers of the last step, the most checked one, have ties to order
        step = {"op": "append_rows", "shape": "closing_block", "rows": d.hot[rng.integers(0, len(d.hot), 257)].astype(np.int64)}
        apply(m, step)
        out.append(step)
    return out
