"""GPU: option row_sums - the per-query sparse sweep of a compact index reads each row's component sum from the row_sums side array
instead of counting it - changes no answer, and the side array follows every change of the rows.

The criterion everywhere: indices, f32 score BITS and counts under row_sums 1 equal those under row_sums 0, the row_sums 0 results are
heap_topk of the oracle's scores, and host_replays / dense_fallbacks do not differ between the two values.  No tolerances.

Staleness traps.  A wrong sum only moves a BOUND, and with ordinary rows a sum that was never refreshed can leave every answer
intact.  The mutation cases therefore put rows into the answer whose bound, evaluated with the sum their lane held BEFORE the mutation,
provably fails every threshold a sweep can hold - stale_rejects() restates fast_bound_passes in numpy f32 (test_bound_f32_cpu.py) and each
case asserts it, so a trap that stops being one fails loudly:
  kind A queries (lowerInterval < 0: the raw score FALLS with the row's sum) against rows that were all ones and become sparse;
  kind B queries (lowerInterval > 0: it RISES with it) against rows - or padding lanes, whose entry is 0 - that become all ones.
Where the old content of a lane is not defined (a fresh allocation: load, a new shard) there is nothing to prove and the case only holds
the answers to the oracle."""
import functools

import numpy as np
import pytest

import orclib as O
from bbqlib import bbq_amd as B, capi
from test_bound_f32_cpu import FBS, F32, bound_z, images, key_of_bits, z_image
from test_bound_math_cpu import bf16_trunc
from test_gpu_l2_share import CDP, _expected, _scores, _synthetic, bits32

pytestmark = pytest.mark.gpu


def _small_segments(ix):
    # launches of 2, 4, 8, ... chunks, each with its own chunk_begin; rows from 1024 on are swept by sparse launches
    ix.set_option("first_segment_rows", 1024)
    ix.set_option("segment_growth", 2)


def _check_row_sums(ix, run, want, values=(0, 1)):
    """run() -> (idx [nq][k], scores, counts) under each value of row_sums: the first equals `want`, the others equal the first"""
    first = first_stats = None
    for v in values:
        ix.set_option("row_sums", v)
        ix.reset_stats()
        idx, sc, cnt = run()
        st = ix.stats()
        st = (st["host_replays"], st["dense_fallbacks"])
        if first is None:
            first, first_stats = (idx, bits32(sc), cnt), st
            for q, (wi, ws) in enumerate(want):
                assert cnt[q] == len(wi), "row_sums %d, query %d" % (v, q)
                np.testing.assert_array_equal(idx[q, :cnt[q]], wi, err_msg="row_sums %d, query %d" % (v, q))
                np.testing.assert_array_equal(bits32(sc[q, :cnt[q]]), bits32(ws), err_msg="row_sums %d, query %d" % (v, q))
        else:
            np.testing.assert_array_equal(cnt, first[2], err_msg="row_sums %d" % v)
            np.testing.assert_array_equal(idx, first[0], err_msg="row_sums %d" % v)
            np.testing.assert_array_equal(bits32(sc), first[1], err_msg="row_sums %d" % v)
            assert st == first_stats, "row_sums %d: host_replays / dense_fallbacks %r, with row_sums %d %r" % (v, st, values[0], first_stats)
    ix.set_option("row_sums", -1)


# ------------------------------------------------------------------------------------------------ 1. answers, 1-bit rows
# the ragged grid of test_gpu_l2_share.py: 19 044 rows = 38 chunks, the last one partly filled, 37 queries = one launch group of 32 plus 5
RAGGED_N, RAGGED_NQ, RAGGED_K = 19_044, 37, 50


@functools.lru_cache(maxsize=None)
def _ragged(dim):
    codes, corr, qq, qc = _synthetic(dim, RAGGED_N, dim, 1, 4, RAGGED_NQ)
    for a in (codes, corr, qq, qc):
        a.setflags(write=False)
    return codes, corr, qq, qc


@functools.lru_cache(maxsize=None)
def _ragged_want(dim, sim):
    codes, corr, qq, qc = _ragged(dim)
    s32 = _scores(codes, corr, dim, qq, qc, 4, sim, 1)
    return s32, [_expected(s, RAGGED_K) for s in s32]


@pytest.mark.parametrize("sim", [0, 1, 2])
@pytest.mark.parametrize("dim", [128, 768, 100])   # W = 1, W = 6, a run-time width whose last byte is partly used
def test_ragged_grid(dim, sim):
    codes, corr, qq, qc = _ragged(dim)
    _, want = _ragged_want(dim, sim)
    ix = B.Index(codes, corr, dim, CDP, corrections="compact")
    try:
        _small_segments(ix)
        _check_row_sums(ix, lambda: ix.search_batch(qq, qc, 4, sim, RAGGED_K), want)
    finally:
        ix.close()


@pytest.mark.parametrize("nq", [1, 3])
def test_few_queries(nq):
    """calls with few queries walk the index in other segments and their sweeps append the candidates to the lists themselves: the
    same flagged kernel.  A single query: the fused latency path (which never reads the sums), then the general one"""
    codes, corr, qq, qc = _ragged(768)
    _, want = _ragged_want(768, 1)
    ix = B.Index(codes, corr, 768, CDP, corrections="compact")
    try:
        _small_segments(ix)
        for fused in (1, 0):
            ix.set_option("latency_fused", fused)
            _check_row_sums(ix, lambda: ix.search_batch(qq[:nq], qc[:nq], 4, 1, RAGGED_K), want[:nq])
    finally:
        ix.close()


def test_strict_mode_keeps_its_launch_and_its_answers():
    """resident_mb 0: automatic means the launch that counts; an explicit 1 holds whatever resident_mb says.  Answers equal."""
    codes, corr, qq, qc = _ragged(768)
    _, want = _ragged_want(768, 1)
    ix = B.Index(codes, corr, 768, CDP, corrections="compact")
    try:
        _small_segments(ix)
        ix.set_option("resident_mb", 0)
        _check_row_sums(ix, lambda: ix.search_batch(qq, qc, 4, 1, RAGGED_K), want, values=(-1, 1, 0))
        assert ix.stats()["resident_bytes"] == 0
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 2. multi-bit rows
# (dim, indexBits, queryBits, the side array exists): 2-bit 1024-d is W = 16; 8-bit 64-d fits 16 bits (64 * 255), 8-bit 300-d does not (76 500)
MULTIBIT = [(1024, 2, 4, True), (1024, 2, 8, True), (96, 4, 4, True), (64, 8, 4, True), (300, 8, 4, False)]
MB_N, MB_NQ, MB_K = 5_003, 12, 50


@functools.lru_cache(maxsize=None)
def _multibit(dim, ib, qb):
    codes, corr, qq, qc = _synthetic(dim + 7 * ib + qb, MB_N, dim, ib, qb, MB_NQ)
    s32 = _scores(codes, corr, dim, qq, qc, qb, 1, ib)
    for a in (codes, corr, qq, qc, *s32):
        a.setflags(write=False)
    return codes, corr, qq, qc, s32


@pytest.mark.parametrize("dim,ib,qb,exists", MULTIBIT)
def test_multibit_rows(dim, ib, qb, exists):
    """where the array does not exist (a sum can exceed 16 bits) row_sums 1 is accepted and the launch is the one that counts"""
    assert (dim * ((1 << ib) - 1) <= 65535) == exists
    codes, corr, qq, qc, s32 = _multibit(dim, ib, qb)
    ix = B.Index(codes, corr, dim, CDP, index_bits=ib, corrections="compact")
    try:
        _small_segments(ix)
        _check_row_sums(ix, lambda: ix.search_batch(qq, qc, qb, 1, MB_K), [_expected(s, MB_K) for s in s32])
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 3. filtered search, one per family
@pytest.mark.parametrize("family", ["1bit_768", "2bit_1024_qb8", "4bit_96", "8bit_64"])
def test_filtered_search(family):
    if family == "1bit_768":
        dim, ib, qb, k = 768, 1, 4, RAGGED_K
        codes, corr, qq, qc = _ragged(dim)
        s32, _ = _ragged_want(dim, 1)
    else:
        dim, ib, qb = {"2bit_1024_qb8": (1024, 2, 8), "4bit_96": (96, 4, 4), "8bit_64": (64, 8, 4)}[family]
        k = MB_K
        codes, corr, qq, qc, s32 = _multibit(dim, ib, qb)
    n = len(codes)
    rng = np.random.default_rng(len(family))
    mask = rng.random(n) < 0.08                     # sparse: most tiles accept a few lanes ...
    mask[(np.arange(n) // 64) % 5 == 3] = False     # ... and every fifth tile none: its wave loads nothing
    ix = B.Index(codes, corr, dim, CDP, index_bits=ib, corrections="compact")
    try:
        _small_segments(ix)
        with capi.Filter(ix, mask) as flt:
            want = [_expected(s, k, mask) for s in s32]
            _check_row_sums(ix, lambda: ix.search_filtered_batch(qq, qc, qb, 1, k, flt), want)
    finally:
        ix.close()


def test_option_validation():
    codes, corr, qq, qc = _ragged(128)
    ix = B.Index(codes[:1024], corr[:1024], 128, CDP)
    try:
        for bad in (-2, 2, 7):
            with pytest.raises(capi.BBQError) as e:
                ix.set_option("row_sums", bad)
            assert e.value.code == capi.ERR_INVALID_ARG
        for good in (-1, 0, 1):
            ix.set_option("row_sums", good)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 4. staleness traps
T_DIM, T_QB, T_SIM, T_K = 768, 4, 1, 20
T_PB = T_DIM // 8
N_A = N_B = 3   # queries of kind A, then of kind B


@functools.lru_cache(maxsize=None)
def _trap_queries():
    rng = np.random.default_rng(4242)
    nq = N_A + N_B
    qq = rng.integers(0, 1 << T_QB, size=(nq, T_DIM), dtype=np.uint8)
    qc = np.empty((nq, 4))
    qc[:N_A, 0] = -0.15 * (0.95 + 0.1 * rng.random(N_A))    # kind A: ay < 0, ly = 0.01
    qc[:N_A, 1] = 0.0
    qc[N_A:, 0] = 0.15 * (0.95 + 0.1 * rng.random(N_B))     # kind B: ay > 0, ly = 0.02
    qc[N_A:, 1] = 0.45
    qc[:, 2] = -0.0028 * rng.random(nq)
    qc[:, 3] = qq.sum(axis=1)
    qq.setflags(write=False)
    qc.setflags(write=False)
    return qq, qc


def _sums(codes):
    return np.unpackbits(codes, axis=1).sum(axis=1).astype(np.int64)


def _rows(kind, m, seed):
    """m rows of one kind: 'bg' random codes, 'ones' / 'zeros' armed rows with ordinary corrections, 'sparse_top' / 'dense_top' the rows
    an update, an append or a compaction puts in their place: 8 bits set / all ones, and a lower interval that takes them to the top of the
    kind A / kind B queries' answers"""
    rng = np.random.default_rng(seed)
    if kind == "bg":
        codes = rng.integers(0, 256, size=(m, T_PB), dtype=np.uint8)
    elif kind in ("ones", "dense_top"):
        codes = np.full((m, T_PB), 255, np.uint8)
    elif kind == "zeros":
        codes = np.zeros((m, T_PB), np.uint8)
    else:
        codes = np.zeros((m, T_PB), np.uint8)
        for r in range(m):
            codes[r, rng.choice(T_PB, 8, replace=False)] = 1 << rng.integers(0, 8, 8)
    corr = np.empty((m, 4))
    top = kind.endswith("_top")
    corr[:, 0] = (-0.2 if top else -0.04) * (0.9 + 0.2 * rng.random(m))
    corr[:, 1] = 0.04 * (0.9 + 0.2 * rng.random(m))
    corr[:, 2] = 1e-4 * (2 * rng.random(m) - 1)
    corr[:, 3] = _sums(codes)
    return codes, corr


def _cat(*parts):
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _tile_add_max(corr):
    """the tile's additive bound as the sweep takes it for COSINE: the maximum over the tile's valid rows, as f32, per row"""
    n = len(corr)
    pad = np.full((n + 63) // 64 * 64, -np.inf)
    pad[:n] = corr[:, 2]
    return np.repeat(pad.reshape(-1, 64).max(axis=1).astype(F32), 64)[:n]


def stale_rejects(codes, corr, old_sums, q):
    """per row: does the f32 bound of query q, evaluated with old_sums instead of the row's sum, fail EVERY threshold a sweep can hold -
    the z image of the lowest score any row of the index has (a threshold is the key of some row's score)?  Fused and unfused."""
    qq, qc = _trap_queries()
    d, _, s32 = O.score_all(codes, corr, T_DIM, qq[q], qc[q], T_QB, T_SIM, CDP)
    im = images(qc[q, 0], (qc[q, 1] - qc[q, 0]) * FBS, qc[q, 3], float(T_DIM), T_SIM, T_DIM, T_DIM * 15)
    assert im is not None, "the trap queries take the f32 bound"
    keys = key_of_bits(np.asarray(s32, F32).view(np.uint32))
    zth = z_image(keys, qc[q, 2], CDP, T_SIM, False).min()
    assert np.isfinite(zth)
    al, au, aadd = bf16_trunc(corr[:, 0]), bf16_trunc(corr[:, 1]), _tile_add_max(corr)
    out = np.ones(len(corr), bool)
    for fused in (True, False):
        with np.errstate(all="ignore"):
            out &= bound_z(np.asarray(d), al, au, aadd, np.maximum(old_sums, 0), im, fused) <= zth
    return out & (old_sums >= 0)


def prove_trap(codes, corr, old_sums, trapped, sparse_from=1024):
    """every trapped query has a row of its oracle answer, swept by a sparse launch (local row >= sparse_from), whose stale bound rejects it"""
    qq, qc = _trap_queries()
    for q in trapped:
        s32 = O.score_all(codes, corr, T_DIM, qq[q], qc[q], T_QB, T_SIM, CDP)[2]
        ans = _expected(s32, T_K)[0]
        hit = stale_rejects(codes, corr, old_sums, q)[ans] & (ans >= sparse_from) & (old_sums[ans] != _sums(codes[ans]))
        assert hit.any(), "query %d: no row of its answer is rejected by a stale sum - the trap is no trap any more" % q


def _want(codes, corr):
    qq, qc = _trap_queries()
    return [_expected(s, T_K) for s in _scores(codes, corr, T_DIM, qq, qc, T_QB, T_SIM, 1)]


def _check_trap_index(ix, codes, corr):
    qq, qc = _trap_queries()
    assert ix.n == len(codes)
    _check_row_sums(ix, lambda: ix.search_batch(qq, qc, T_QB, T_SIM, T_K), _want(codes, corr))


KIND_A, KIND_B = tuple(range(N_A)), tuple(range(N_A, N_A + N_B))
UNKNOWN = -1   # old content of a lane that no earlier write defined


@functools.lru_cache(maxsize=None)
def _updated():
    """3000 rows with armed rows in three tiles (the last one partly filled), and the same rows after the update that springs the traps"""
    codes, corr = _rows("bg", 3000, 1)
    codes, corr = codes.copy(), corr.copy()
    ones_at = np.r_[1100:1108, 2990:2994]
    zeros_at = np.r_[1500:1508, 2994:2998]
    codes[ones_at], corr[ones_at] = _rows("ones", len(ones_at), 2)
    codes[zeros_at], corr[zeros_at] = _rows("zeros", len(zeros_at), 3)
    ords = np.concatenate([ones_at, zeros_at]).astype(np.int32)
    new = _cat(_rows("sparse_top", len(ones_at), 4), _rows("dense_top", len(zeros_at), 5))
    after = codes.copy(), corr.copy()
    after[0][ords], after[1][ords] = new
    return (codes, corr), ords, new, after


def test_trap_update_rows():
    (codes, corr), ords, new, (codes2, corr2) = _updated()
    prove_trap(codes2, corr2, _sums(codes), KIND_A + KIND_B)
    ix = B.Index(codes, corr, T_DIM, CDP, corrections="compact")
    try:
        _small_segments(ix)
        _check_trap_index(ix, codes, corr)
        ix.update_rows(ords, *new)
        _check_trap_index(ix, codes2, corr2)
    finally:
        ix.close()


def test_trap_append_rows():
    """1000 rows, + 100 across a tile boundary (the storage grows), + 1 into a padding lane of the last tile, + 150 behind it, then enough
    to reallocate.  A padding lane's entry is 0: an all-ones row that lands there traps the kind B queries."""
    steps = [_rows("bg", 1000, 11), _rows("bg", 100, 12), _rows("dense_top", 1, 13), _cat(_rows("dense_top", 30, 14), _rows("sparse_top", 120, 15)),
             _cat(_rows("bg", 2990, 16), _rows("dense_top", 10, 17))]
    ix = B.Index(*steps[0], T_DIM, CDP, corrections="compact")
    try:
        _small_segments(ix)
        codes, corr = steps[0]
        for i, step in enumerate(steps[1:], 1):
            cap = ix.capacity
            old = np.concatenate([_sums(codes), np.zeros(len(step[0]), np.int64)])   # the lanes behind the last row held 0 ...
            codes, corr = _cat((codes, corr), step)
            old[min(cap, (len(old) - len(step[0]) + 63) // 64 * 64):] = UNKNOWN      # ... as far as the tiles in use went
            if i in (2, 3):
                assert len(codes) <= cap, "the step was meant to land in lanes the storage already holds"
                prove_trap(codes, corr, old, KIND_B)
            if i == 4:
                # the step that reallocates has to MOVE the sums.  No proof is possible for a fresh allocation's content, so rows of
                # the part that moves are first replaced by rows of the answer with extreme sums: what has to arrive in the new
                # array then differs from anything an earlier allocation of that size can have held for these lanes
                assert len(codes) > cap
                ords = np.r_[1030:1034, 1060:1064].astype(np.int32)
                new = _cat(_rows("sparse_top", 4, 18), _rows("dense_top", 4, 19))
                ix.update_rows(ords, *new)
                codes, corr = codes.copy(), corr.copy()
                codes[ords], corr[ords] = new
            ix.append_rows(*step)
            _check_trap_index(ix, codes, corr)
        assert ix.capacity > 1536, "the last step was meant to reallocate"
    finally:
        ix.close()


def test_trap_reserve_then_append():
    codes, corr = _rows("bg", 2000, 21)
    step = _cat(_rows("dense_top", 40, 22), _rows("bg", 200, 23))
    ix = B.Index(codes, corr, T_DIM, CDP, corrections="compact")
    try:
        _small_segments(ix)
        # rows of the answer with extreme sums in the part that moves (see test_trap_append_rows): the copy has to bring THESE sums
        ords = np.r_[1200:1204, 1900:1904].astype(np.int32)
        new = _cat(_rows("sparse_top", 4, 24), _rows("dense_top", 4, 25))
        ix.update_rows(ords, *new)
        codes, corr = codes.copy(), corr.copy()
        codes[ords], corr[ords] = new
        ix.reserve(5000)   # the side arrays move: the sums of the 2000 rows and the zeros behind them, to the end of tile 31
        assert ix.capacity >= 5000
        _check_trap_index(ix, codes, corr)
        old = np.concatenate([_sums(codes), np.zeros(48, np.int64), np.full(len(step[0]) - 48, UNKNOWN)])
        codes2, corr2 = _cat((codes, corr), step)
        prove_trap(codes2, corr2, old, KIND_B)
        ix.append_rows(*step)
        _check_trap_index(ix, codes2, corr2)
    finally:
        ix.close()


@pytest.mark.parametrize("how", ["remove_rows", "compact"])
def test_trap_compaction(how):
    """64 armed rows in front of 64 rows of the answer: without the armed rows the answer's rows sit in the lanes the armed rows had.
    remove_rows: all ones in front of sparse rows (kind A); compact: all zeros in front of all-ones rows (kind B)."""
    armed, top, trapped = ("ones", "sparse_top", KIND_A) if how == "remove_rows" else ("zeros", "dense_top", KIND_B)
    codes, corr = _cat(_rows("bg", 1100, 31), _rows(armed, 64, 32), _rows(top, 64, 33), _rows("bg", 1369, 34))
    drop = np.r_[1100:1164]
    keep = np.ones(len(codes), bool)
    keep[drop] = False
    codes2, corr2 = codes[keep], corr[keep]
    prove_trap(codes2, corr2, _sums(codes)[:len(codes2)], trapped)
    ix = B.Index(codes, corr, T_DIM, CDP, corrections="compact")
    try:
        _small_segments(ix)
        if how == "remove_rows":
            ix.remove_rows(drop)
        else:
            with capi.Filter(ix, keep) as flt:
                ix.compact(flt)
        _check_trap_index(ix, codes2, corr2)
    finally:
        ix.close()


def test_trap_save_load(tmp_path):
    """the array is in no file: a load derives it from the loaded codes.  (A fresh allocation: nothing to prove, the oracle decides.)"""
    (codes, corr), ords, new, (codes2, corr2) = _updated()
    cen = np.zeros(T_DIM, np.float32)
    ix = B.Index(codes, corr, T_DIM, CDP, corrections="compact")
    try:
        ix.update_rows(ords, *new)
        ix.save(str(tmp_path / "rs"), cen, T_SIM)
    finally:
        ix.close()
    ix2, _, _ = B.Index.load(str(tmp_path / "rs"))
    try:
        _small_segments(ix2)
        _check_trap_index(ix2, codes2, corr2)
    finally:
        ix2.close()


def test_trap_multi_device(tmp_path):
    """two shards on device 0 behind one handle, then the same through save -> load_multi"""
    _, _, _, (codes, corr) = _updated()
    cen = np.zeros(T_DIM, np.float32)
    mx = B.Index.create_multi(codes, corr, T_DIM, CDP, [0, 0], pilot_rows=1024, corrections="compact")
    try:
        assert mx.shards == 2
        _small_segments(mx)
        _check_trap_index(mx, codes, corr)
        mx.save(str(tmp_path / "rsm"), cen, T_SIM)
    finally:
        mx.close()
    mx2, _, _ = B.Index.load_multi(str(tmp_path / "rsm"), [0, 0])
    try:
        _small_segments(mx2)
        _check_trap_index(mx2, codes, corr)
    finally:
        mx2.close()


def test_trap_pilot_replica():
    """a row shard with a pilot replica of the global prefix (row_base, pilot_codes): both storages carry their sums.  The two shards'
    packed lists, replayed in shard order, are the oracle's answer under either value of the option"""
    import torch
    _, _, _, (codes, corr) = _updated()
    qq, qc = _trap_queries()
    nq, n, cut = len(qq), len(codes), 1536
    want = _want(codes, corr)
    shards = [B.Index(codes[:cut], corr[:cut], T_DIM, CDP, corrections="compact"),
              B.Index(codes[cut:], corr[cut:], T_DIM, CDP, row_base=cut, pilot_codes=codes[:1024], pilot_corr=corr[:1024], corrections="compact")]
    try:
        results = []
        for v in (0, 1):
            packed, offsets, stats = [], [], []
            for ix in shards:
                _small_segments(ix)
                ix.set_option("row_sums", v)
                ix.reset_stats()
                cap = int(ix.shard_list_cap(T_K)) * nq
                d_packed = torch.zeros(cap, dtype=torch.int64, device="cuda")
                d_off = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
                d_flags = torch.zeros(nq, dtype=torch.int32, device="cuda")
                total = ix.shard_scan(qq, qc, T_QB, T_SIM, T_K, d_packed.data_ptr(), cap, d_off.data_ptr(), d_flags.data_ptr())
                assert int(d_flags.abs().sum().item()) == 0
                packed.append(d_packed[:total].cpu().numpy().view(np.uint64))
                offsets.append(d_off.cpu().numpy())
                st = ix.stats()
                stats.append((st["host_replays"], st["dense_fallbacks"]))
            idx, sc, cnt = B.replay_batch(packed, offsets, nq, n, T_K, n_threads=2)
            results.append((idx, bits32(sc), cnt, stats))
        for q, (wi, ws) in enumerate(want):
            idx, sc, cnt, _ = results[0]
            assert cnt[q] == len(wi)
            np.testing.assert_array_equal(idx[q, :cnt[q]], wi, err_msg="row_sums 0, query %d" % q)
            np.testing.assert_array_equal(sc[q, :cnt[q]], bits32(ws), err_msg="row_sums 0, query %d" % q)
        for a, b in zip(results[0][:3], results[1][:3]):
            np.testing.assert_array_equal(a, b)
        assert results[0][3] == results[1][3]
    finally:
        for ix in shards:
            ix.close()
