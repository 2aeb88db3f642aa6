"""CPU: bbq_exact_bound, the interval the exact search's prefilter prunes with, against the oracle's f64 scores with no device.  The f32
dot product and sums of squares are computed in numpy in four orders - forward, reverse, pairwise, `@` - and every interval must hold
the score, or be unknown (NaN, +Inf); on ordinary rows it must be known and about as narrow as the classical bound."""
import numpy as np
import pytest

import exact_model as EM
from bbqlib import capi

F = np.float32
ORDERS = {
    "forward": lambda p: np.cumsum(p, dtype=F)[-1],
    "reverse": lambda p: np.cumsum(p[::-1], dtype=F)[-1],
    "pairwise": lambda p: np.add.reduce(np.ascontiguousarray(p), dtype=F),
}
N_PLAIN = 24


def _rows(dim):
    rng = np.random.default_rng(4100 + dim)
    base = rng.standard_normal((N_PLAIN + 10, dim)).astype(F)
    queries = rng.standard_normal((5, dim)).astype(F)
    h = base[N_PLAIN:]
    h[0] = 1e-30
    h[1] = 1e-40
    h[2] = 3e38
    h[3, 0] = np.inf
    h[4, dim - 1] = -np.inf
    h[5, dim // 2] = np.nan
    h[6] = 0.0
    h[7] *= F(1e20)
    h[8] *= F(1e-3)
    h[9] *= F(1e-19)   # products in the denormal range
    queries[3] = 0.0
    queries[4] *= F(1e-18)
    return base, queries


@pytest.mark.parametrize("sim", [1, 2])
@pytest.mark.parametrize("dim", [1, 3, 33, 100, 768])
def test_every_interval_holds_the_oracle_score(dim, sim):
    base, queries = _rows(dim)
    c = EM.scores(queries, base, sim)
    with np.errstate(all="ignore"):
        mm = queries @ base.T
        sq_mm = [np.array([v @ v for v in m], F) for m in (queries, base)]
        for q, qv in enumerate(queries):
            for r, rv in enumerate(base):
                for name in list(ORDERS) + ["matmul"]:
                    if name == "matmul":
                        dot, qq, rr = mm[q, r], sq_mm[0][q], sq_mm[1][r]
                    else:
                        dot, qq, rr = (ORDERS[name](a * b) for a, b in ((qv, rv), (qv, qv), (rv, rv)))
                    lo, hi = capi.exact_bound(dim, sim, dot, qq, rr)
                    w = "dim %d sim %d query %d row %d %s: [%r, %r] for %r" % (dim, sim, q, r, name, lo, hi, c[q, r])
                    unknown = np.isnan(lo) and hi == np.inf
                    assert unknown or lo <= c[q, r] <= hi, w
                    assert not (lo == 0 and not np.signbit(lo)) and not (hi == 0 and np.signbit(hi)), w + ": a zero end on the wrong side"
                    if r < N_PLAIN and q < 3:
                        # ordinary pairs: known.  A side is at most g = (dim + 2) 2^-23 for the dot product and |cos| g for the norms
                        # (the bound): 4 g = 8 (dim + 2) 2^-24 in all, and a quarter more for every slop
                        scale = 1.0 if sim == 1 else float(np.linalg.norm(qv.astype(np.float64)) * np.linalg.norm(rv.astype(np.float64)))
                        assert not unknown and hi - lo <= 10 * (dim + 2) * 2.0 ** -24 * scale, w


def test_arguments():
    assert capi.lib().bbq_exact_bound(0, 1, 0.0, 1.0, 1.0, None, None) == capi.ERR_INVALID_ARG
    with pytest.raises(capi.BBQError) as e:
        capi.exact_bound(0, 1, 0.0, 1.0, 1.0)
    assert e.value.code == capi.ERR_INVALID_ARG
    with pytest.raises(capi.BBQError) as e:
        capi.exact_bound(8, 0, 0.0, 1.0, 1.0)   # EUCLIDEAN: no interval
    assert e.value.code == capi.ERR_UNSUPPORTED
    lo, hi = capi.exact_bound(8, 1, 0.5, np.inf, 1.0)
    assert np.isnan(lo) and hi == np.inf
