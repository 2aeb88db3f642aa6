"""GPU: the bytes of <prefix>.veb against a restatement of the tile record.

The restatement below is written from DESIGN.md section 2 ("HBM layout", "Multi-bit indexes") and the file table of "On-disk
format" alone, in numpy, and calls nothing of the library: the library only creates, grows, builds and saves the indexes whose files
are compared.  Every comparison is byte for byte - code chunks, corrections blocks, the side section, and the padding lanes of the
last tile, which are all zero in every block."""
import struct

import numpy as np
import pytest

import orclib as O
from bbqlib import bbq_amd as B

pytestmark = pytest.mark.gpu

TILE_ROWS = 64
ROWS = (1, 63, 64, 65, 130)
# (indexBits, dim): 1-bit rows of one byte, of 17 bytes (a second, mostly padded chunk) and of w16 = 6; multi-bit fields of every width
ONE_BIT = ((1, 8), (1, 129), (1, 768))
MULTI_BIT = ((2, 5), (2, 67), (3, 33), (8, 17))
QUIET_NAN32 = 0x7FC00000


# ------------------------------------------------------------------------------------------------ the restatement

def field_bits(index_bits):
    return 1 if index_bits == 1 else 2 if index_bits <= 2 else 4 if index_bits <= 4 else 8


def stored_rows(codes, dim, index_bits):
    """[n][w16 * 16] bytes: a 1-bit row is the caller's packed bytes; a multi-bit row (one byte per dimension) is packed into fields -
    field f of dword w is dimension w * (32 / bits) + f, i.e. dimension d sits at bit d * bits of the little-endian row - and every
    row is zero-padded to 16-byte chunks"""
    n = codes.shape[0]
    bits = field_bits(index_bits)
    if bits == 1:
        rows = codes
    else:
        per = 8 // bits
        padded = np.zeros((n, (dim + per - 1) // per * per), np.uint32)
        padded[:, :dim] = codes
        rows = np.zeros((n, padded.shape[1] // per), np.uint32)
        for f in range(per):
            rows |= padded[:, f::per] << (f * bits)
        rows = rows.astype(np.uint8)
    w16 = (rows.shape[1] + 15) // 16
    out = np.zeros((n, w16 * 16), np.uint8)
    out[:, :rows.shape[1]] = rows
    return out, w16


def upper16(x):
    return np.asarray(x, np.float64).astype(np.float32).view(np.uint32) >> 16


def restate(codes, corr, dim, index_bits, compact, with_sums):
    """(tile records, side section) as bytes: what the file must hold for these rows"""
    n = codes.shape[0]
    rows, w16 = stored_rows(codes, dim, index_bits)
    n_tiles = (n + TILE_ROWS - 1) // TILE_ROWS
    npad = n_tiles * TILE_ROWS
    prow = np.zeros((npad, w16 * 16), np.uint8)
    prow[:n] = rows
    pcorr = np.zeros((npad, 4), np.float64)
    pcorr[:n] = corr
    # code chunk j of row r at (j * 64 + r) * 16
    chunks = prow.reshape(n_tiles, TILE_ROWS, w16, 16).transpose(0, 2, 1, 3).reshape(n_tiles, w16 * TILE_ROWS * 16)
    c = pcorr.reshape(n_tiles, TILE_ROWS, 4)
    if compact:
        word = (upper16(c[:, :, 0]) | (upper16(c[:, :, 1]) << 16)).astype("<u4")
        blocks = [word.view(np.uint8).reshape(n_tiles, -1)]
    else:
        blocks = [np.ascontiguousarray(c[:, :, 0:2]).view(np.uint8).reshape(n_tiles, -1),
                  np.ascontiguousarray(c[:, :, 2]).view(np.uint8).reshape(n_tiles, -1)]
        if with_sums:
            blocks.append(np.ascontiguousarray(c[:, :, 3]).view(np.uint8).reshape(n_tiles, -1))
    tiles = np.concatenate([chunks] + blocks, axis=1)
    side = b""
    if compact:
        exact = pcorr.copy()
        exact[:, 3] = 0.0
        add_range = np.zeros((n_tiles, 2), np.float32)
        for t in range(n_tiles):
            a = corr[t * TILE_ROWS:min(n, (t + 1) * TILE_ROWS), 2]
            if np.isnan(a).any():
                add_range[t].view(np.uint32)[:] = QUIET_NAN32
            else:
                add_range[t] = (np.float32(a.min()), np.float32(a.max()))
        side = exact.tobytes() + add_range.tobytes()
    return tiles.tobytes(), side


def check_file(prefix, codes, corr, dim, index_bits, compact, with_sums=False, msg=""):
    """<prefix>.veb from vectorDataOffset on is the restated tile records followed by the restated side section"""
    head = open(prefix + ".vemb", "rb").read(104)
    data_offset, = struct.unpack_from("<q", head, 24)
    tiles_bytes, exact_bytes = struct.unpack_from("<qq", head, 80)
    want_tiles, want_side = restate(codes, corr, dim, index_bits, compact, with_sums)
    assert (tiles_bytes, exact_bytes) == (len(want_tiles), len(want_side)), msg
    data = open(prefix + ".veb", "rb").read()[data_offset:]
    assert len(data) == tiles_bytes + exact_bytes, msg
    got_tiles, got_side = data[:tiles_bytes], data[tiles_bytes:]
    if got_tiles != want_tiles:
        g, w = np.frombuffer(got_tiles, np.uint8), np.frombuffer(want_tiles, np.uint8)
        at = int(np.flatnonzero(g != w)[0])
        stride = len(want_tiles) // ((codes.shape[0] + TILE_ROWS - 1) // TILE_ROWS)
        raise AssertionError("%s: tile %d differs at byte %d of its record (%d differing bytes in all)" % (msg, at // stride, at % stride, int((g != w).sum())))
    if got_side != want_side:
        g, w = np.frombuffer(got_side, np.uint8), np.frombuffer(want_side, np.uint8)
        raise AssertionError("%s: side section differs at byte %d" % (msg, int(np.flatnonzero(g != w)[0])))


# ------------------------------------------------------------------------------------------------ rows

def caller_rows(n, dim, index_bits, seed):
    """n rows as a caller hands them over, with the implied component sums (popcount / code sum)"""
    rng = np.random.default_rng(seed)
    if index_bits == 1:
        codes = rng.integers(0, 256, (n, (dim + 7) // 8), dtype=np.uint8)
        sums = np.unpackbits(codes, axis=1).sum(axis=1)
    else:
        codes = rng.integers(0, 1 << index_bits, (n, dim), dtype=np.uint8)
        sums = codes.sum(axis=1, dtype=np.int64)
    corr = np.empty((n, 4), np.float64)
    corr[:, 0] = -rng.random(n) - 0.01
    corr[:, 1] = rng.random(n) + 0.01
    corr[:, 2] = rng.standard_normal(n) * 3.0
    corr[:, 3] = sums
    return codes, corr


def saved(ix, tmp_path, dim):
    prefix = str(tmp_path / "ix")
    try:
        ix.save(prefix, np.zeros(dim, np.float32), O.SIMS["COSINE"])
    finally:
        ix.close()
    return prefix


def make(codes, corr, dim, index_bits, compact):
    return B.Index(codes, corr, dim, 0.25, index_bits=index_bits, corrections="compact" if compact else "inline")


# ------------------------------------------------------------------------------------------------ tests

@pytest.mark.parametrize("compact", [True, False], ids=["compact", "inline"])
@pytest.mark.parametrize("index_bits,dim", ONE_BIT + MULTI_BIT)
def test_created_from_rows(index_bits, dim, compact, tmp_path):
    for n in ROWS:
        codes, corr = caller_rows(n, dim, index_bits, 1000 * dim + n)
        prefix = saved(make(codes, corr, dim, index_bits, compact), tmp_path, dim)
        check_file(prefix, codes, corr, dim, index_bits, compact, msg="ib%d dim %d n %d" % (index_bits, dim, n))


@pytest.mark.parametrize("asked_compact", [True, False], ids=["compact", "inline"])
@pytest.mark.parametrize("index_bits,dim", [(1, 129), (2, 67)])
def test_explicit_sums_are_inline_with_sum(index_bits, dim, asked_compact, tmp_path):
    n = 130
    codes, corr = caller_rows(n, dim, index_bits, 77)
    corr[5, 3] += 1.0     # not the implied sum: the index stores the sums, whatever layout was asked for
    corr[129, 3] = 0.5
    prefix = saved(make(codes, corr, dim, index_bits, asked_compact), tmp_path, dim)
    check_file(prefix, codes, corr, dim, index_bits, False, with_sums=True, msg="ib%d dim %d explicit sums" % (index_bits, dim))


def test_nan_additive_correction(tmp_path):
    n, dim = 130, 129
    codes, corr = caller_rows(n, dim, 1, 78)
    corr[70, 2] = np.nan  # tile 1: both ends of its range are NaN; tiles 0 and 2 keep theirs
    prefix = saved(make(codes, corr, dim, 1, True), tmp_path, dim)
    check_file(prefix, codes, corr, dim, 1, True, msg="NaN additive")


@pytest.mark.parametrize("index_bits,dim,compact", [(1, 129, True), (2, 67, False)])
def test_grown_by_append_rows(index_bits, dim, compact, tmp_path):
    codes, corr = caller_rows(130, dim, index_bits, 79)
    ix = make(codes[:63], corr[:63], dim, index_bits, compact)
    ix.append_rows(codes[63:], corr[63:])
    assert ix.n == 130
    check_file(saved(ix, tmp_path, dim), codes, corr, dim, index_bits, compact, msg="grown 63 -> 130")


@pytest.mark.parametrize("index_bits", [1, 4])
def test_built_on_the_device(index_bits, tmp_path):
    n, dim, sim = 130, 129, O.SIMS["COSINE"]
    base = O.mulberry32(90 + index_bits, n * dim).reshape(n, dim)
    codes, corr, cen = O.build_index(base, sim, ib=index_bits)  # the oracle's rows, not rows the library handed back
    ix = B.Index.build(base, sim, index_bits=index_bits, want_host_copy=False, corrections="compact")[0]
    check_file(saved(ix, tmp_path, dim), codes, corr, dim, index_bits, True, msg="built ib%d" % index_bits)
