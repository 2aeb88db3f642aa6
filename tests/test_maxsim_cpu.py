"""CPU: bbq_maxsim_reduce - the MaxSim search's group score, the ordered f64 sum of a group's per-token representative scores rounded
once to f32 - against the numpy model (tests/maxsim_model.py), bit for bit: random values, one token (the identity, -0.0 included), a NaN
in any position, and two constructed cases that pin the precision (f64, not f32) and the order (ascending token) of the adds."""
import numpy as np
import pytest

import maxsim_model as M
from bbqlib import capi


def bits(a):
    a = np.array(a, np.float32)
    a[np.isnan(a)] = np.nan
    return a.view(np.uint32)


def test_random_values():
    rng = np.random.default_rng(20)
    for T, L in ((1, 1), (2, 7), (5, 64), (32, 1000), (67, 333)):
        rep = (rng.standard_normal((T, L)) * 10.0 ** rng.integers(-3, 4, (T, L))).astype(np.float32)
        np.testing.assert_array_equal(bits(capi.maxsim_reduce(rep)), bits(M.reduce(rep)), err_msg="T=%d L=%d" % (T, L))
    assert capi.maxsim_reduce(np.zeros((3, 0), np.float32)).shape == (0,)


def test_one_token_is_the_identity():
    rep = np.array([[1.5, -0.0, 0.0, np.inf, -np.inf, 1e-45, -3.25e38]], np.float32)
    got = capi.maxsim_reduce(rep)
    assert got.view(np.uint32).tolist() == rep[0].view(np.uint32).tolist()      # -0.0 stays -0.0: the sum starts from m_0, not from 0.0
    assert got.view(np.uint32)[1] == 0x80000000
    two = capi.maxsim_reduce(np.array([[-0.0], [-0.0]], np.float32))
    assert two.view(np.uint32)[0] == 0x80000000 and bits(M.reduce([[-0.0], [-0.0]]))[0] == 0x80000000


@pytest.mark.parametrize("T", [1, 2, 5])
def test_a_nan_in_any_position(T):
    for at in range(T):
        rep = np.arange(1, 3 * T + 1, dtype=np.float32).reshape(T, 3)
        rep[at, 1] = np.nan
        got = capi.maxsim_reduce(rep)
        assert np.isnan(got[1]) and not np.isnan(got[[0, 2]]).any()
        np.testing.assert_array_equal(bits(got), bits(M.reduce(rep)))
    inf = capi.maxsim_reduce(np.array([[np.inf], [-np.inf]], np.float32))
    assert np.isnan(inf[0])


def test_precision_and_order_are_pinned():
    # f64 against f32 accumulation: 1 + 2^-24 + 2^-24.  In f32 each half ulp is rounded away (ties to even); in f64 the sum is 1 + 2^-23
    half = np.float32(2.0 ** -24)
    rep = np.array([[1.0], [half], [half]], np.float32)
    in_f32 = np.float32(np.float32(rep[0, 0] + rep[1, 0]) + rep[2, 0])
    in_f64 = np.float32(np.float64(rep[0, 0]) + np.float64(rep[1, 0]) + np.float64(rep[2, 0]))
    assert in_f32 == np.float32(1.0) and in_f64.view(np.uint32) == np.float32(1.0).view(np.uint32) + 1        # they differ in the last bit
    got = capi.maxsim_reduce(rep)
    assert got.view(np.uint32)[0] == in_f64.view(np.uint32) == bits(M.reduce(rep))[0]
    # ascending against descending token: (1 + 2^60) - 2^60 = 0 in f64, (-2^60 + 2^60) + 1 = 1
    big = np.float32(2.0 ** 60)
    rep = np.array([[1.0], [big], [-big]], np.float32)
    ascending = np.float32((np.float64(1.0) + np.float64(big)) + np.float64(-big))
    descending = np.float32((np.float64(-big) + np.float64(big)) + np.float64(1.0))
    assert ascending == 0.0 and descending == 1.0
    got = capi.maxsim_reduce(rep)
    assert got[0] == ascending and got.view(np.uint32)[0] == bits(M.reduce(rep))[0]
    assert capi.maxsim_reduce(rep[::-1].copy())[0] == descending


def test_refusals():
    with pytest.raises(capi.BBQError) as e:
        capi.maxsim_reduce(np.zeros((0, 4), np.float32))
    assert e.value.code == capi.ERR_INVALID_ARG and "bbq_maxsim_reduce" in str(e.value)
    assert capi.lib().bbq_maxsim_reduce(None, 2, 3, None) == capi.ERR_INVALID_ARG
    assert capi.maxsim_token_block() >= 1
