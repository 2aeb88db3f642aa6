"""Hostile rows and parameters for the quantizer (scalarQuantize, src/optimizedScalarQuantizer.ts:108-353): the batches, the grid of
(indexBits, lambda, iters) and the oracle's answers over them, shared by tests/test_quantizer_hostile_cpu.py (oracle, host quantizer,
reference pin) and tests/test_gpu_quantizer_hostile.py (bbq_quantize1_kernel behind build, append and update).

Every batch is deterministic, f32 and finite (validation passes).  What each is aimed at is stated - and asserted, with the oracle's
trace - in test_quantizer_hostile_cpu.py:
  mixed      every way optimizeIntervals can end, NaN intervals included
  extreme    magnitudes around 1e30 next to f32 denormals: the scaling paths of f64 division and sqrt, denormal conversions
  overflow   the f32 centroid sum and the centred values overflow under EUCLIDEAN / MAXIMUM_INNER_PRODUCT: every correction NaN
  identical  every row is the centroid: a zero centred vector, non-finite `scale`
"""
import functools

import numpy as np

import orclib as O

NS = (257, 601)                    # cross a 64-row tile and a 256-thread block, partial last tile
DIMS = (1, 2, 3, 13, 64, 131)      # dim % 4 = 1, 2, 3, 0; shorter than a float4; the 32-dimension word and the 128-dimension chunk boundary
BATCHES = ("mixed", "extreme", "overflow", "identical")
GRID = ((1, 0.1, 5), (1, 0.0, 5), (1, 1.0, 5), (2, 0.1, 5), (3, 0.0, 2), (4, 1.0, 3), (8, 0.001, 20), (4, 0.1, 0))   # (indexBits, lambda, iters)
SIM_NAMES = ("EUCLIDEAN", "COSINE", "MAXIMUM_INNER_PRODUCT")
SEED = 7

EXIT_ITERS, EXIT_SCALE, EXIT_DET, EXIT_CONVERGED, EXIT_LOSS_ROSE = range(5)   # trace[0], oracle/bbq_oracle.h


def _small_int_row(rng, dim):
    row = rng.integers(-2, 3, dim).astype(np.float32)
    if not row.any():
        row[0] = 1.0
    return row


def _mixed(rng, n, dim):
    e = n // 8
    parts = [rng.standard_normal((e, dim)),
             rng.standard_normal((e, dim)) * 10.0 ** rng.uniform(-6, 6, (e, 1)),
             rng.choice([-1.0, 1.0], (e, dim)) * 10.0 ** rng.uniform(-3, 3, (e, 1)),
             rng.integers(-2, 3, (e, dim)).astype(np.float64),
             np.zeros((e, dim)),
             np.full((e, dim), 2.5)]
    spike = np.zeros((e, dim))
    spike[np.arange(e), rng.integers(0, dim, e)] = rng.standard_normal(e) * 10.0 ** rng.integers(-3, 4, e)
    parts.append(spike)
    rest = np.concatenate(parts)
    rows = np.concatenate([rest, rest[rng.integers(0, len(rest), n - len(rest))]])
    return rows[rng.permutation(n)]


@functools.lru_cache(maxsize=None)
def batch(name, n, dim):
    """f32 [n, dim], read-only"""
    rng = np.random.default_rng([SEED, BATCHES.index(name), n, dim])
    if name == "mixed":
        rows = _mixed(rng, n, dim)
    elif name == "extreme":
        rows = rng.standard_normal((n, dim)) * 1e30
        rows[::5] = rng.standard_normal((len(rows[::5]), dim)) * 1e-42
    elif name == "overflow":
        rows = rng.choice([-3e38, 3e38, 1.0, 0.0], (n, dim))
    elif name == "identical":
        rows = np.tile(_small_int_row(rng, dim), (n, 1))
    else:
        raise KeyError(name)
    rows = np.ascontiguousarray(rows, np.float32)
    assert np.isfinite(rows).all()
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def benign(n, dim, seed=0):
    rows = np.random.default_rng([SEED, 99, n, dim, seed]).standard_normal((n, dim)).astype(np.float32)
    rows.setflags(write=False)
    return rows


def queries(name, n, dim):
    """two queries: a row of the batch (the first that is not zero, if any) and a benign one"""
    rows = batch(name, n, dim)
    nz = np.flatnonzero(rows.any(axis=1))
    return np.stack([rows[nz[0] if len(nz) else 0], benign(1, dim, 1)[0]])


@functools.lru_cache(maxsize=None)
def oracle_build(name, n, dim, sim, ib, lam, iters):
    """(codes, corr, centroid) of O.build_index over the batch, computed once and shared; read-only"""
    out = O.build_index(batch(name, n, dim), sim, lam, iters, ib)
    for a in out:
        a.setflags(write=False)
    return out


def canon32(a):
    a = np.array(a, np.float32)
    a[np.isnan(a)] = np.nan
    return a.view(np.uint32)


def canon64(a):
    a = np.array(a, np.float64)
    a[np.isnan(a)] = np.nan
    return a.view(np.uint64)


# ---------------------------------------------------------------- how the rows' optimisations ended

CLASSES = ("ran out, nothing accepted", "ran out after an accepted step", "determinant exit", "converged after an accepted step",
           "loss rose, nothing accepted", "loss rose after an accepted step", "NaN loss seen", "non-finite scale",
           "converged, nothing accepted", "NaN correction")


def classify(trace, corr):
    """rows per class of CLASSES, from quantize_trace's trace [n, 3] and corrections"""
    ex, acc, nan = trace[:, 0], trace[:, 1] > 0, trace[:, 2] != 0
    return np.array([np.sum((ex == EXIT_ITERS) & ~acc), np.sum((ex == EXIT_ITERS) & acc), np.sum(ex == EXIT_DET),
                     np.sum((ex == EXIT_CONVERGED) & acc), np.sum((ex == EXIT_LOSS_ROSE) & ~acc), np.sum((ex == EXIT_LOSS_ROSE) & acc),
                     np.sum(nan), np.sum(ex == EXIT_SCALE), np.sum((ex == EXIT_CONVERGED) & ~acc), np.sum(np.isnan(corr).any(axis=1))], np.int64)


@functools.lru_cache(maxsize=None)
def traced(name, n, dim, sim, ib, lam, iters):
    """(codes, corr, trace) of O.quantize_trace over the batch against the build's centroid"""
    cen = oracle_build(name, n, dim, sim, ib, lam, iters)[2]
    return O.quantize_trace(batch(name, n, dim), cen, sim, ib, lam, iters)


def table(rows):
    """rows: [(label, counts)] -> text"""
    head = "%-44s " % "" + " ".join("%5s" % ("c%d" % i) for i in range(len(CLASSES)))
    legend = "\n".join("  c%d = %s" % (i, c) for i, c in enumerate(CLASSES))
    return "\n".join([legend, head] + ["%-44s " % label + " ".join("%5d" % c for c in counts) for label, counts in rows])
