"""CPU: the start value of a row that a filter REJECTS in the filtered family of the shared sweep on the matrix cores
(bbq_mfma_kernels.hip: MfmaNum<FP>::pass_none, row_constants_early with `accepted` false), restated in numpy with f32 arithmetic as
tests/test_prefilter_math_cpu.py restates the accepted rows'.  A rejected row has zero constants and K = pass_none, so its
accumulator ends at K + S * qcDist: that must stay below the bias - the pre-filter passes what ends ABOVE it - and inside the form's
binade, where the sum is exact, for the largest qcDist the form admits at every dimension the kernel is built for and every fp_scale."""
import numpy as np
import pytest

from test_prefilter_math_cpu import FORMS, fma32

F32 = np.float32

# bbq_mfma_kernels.hip MfmaNum<FP>::pass_none: pass_all mirrored at the bias, a quarter of the binade's lower end below its middle
PASS_NONE = {"int8": F32(12582912.0) - F32(2097152.0), "fp": F32(786432.0) - F32(131072.0)}
BINADE = {"int8": (F32(2.0 ** 23), F32(2.0 ** 24)), "fp": (F32(2.0 ** 19), F32(2.0 ** 20))}
DIMS = (128, 768, 1024, 1536)
# (form, S, the largest query value the form takes at that S): int8 up to 127; FP6 x FP4 with products of q / 4, q / 2 or q
# (stage_queries_mfma: the largest scale the values leave room for) - and, beyond what the host ever stages, the value 15 at EVERY scale
SCALES = [("int8", 1.0, 127), ("fp", 0.25, 15), ("fp", 0.5, 7), ("fp", 1.0, 3), ("fp", 0.5, 15), ("fp", 1.0, 15)]


def test_pass_none_mirrors_pass_all_inside_the_binade():
    for form, N in FORMS.items():
        bias, lo = F32(N["bias"]), BINADE[form][0]
        assert bias == F32(1.5) * lo
        assert F32(N["pass_all"]) - bias == bias - PASS_NONE[form] == lo / F32(4.0)
        assert lo <= PASS_NONE[form] < bias < BINADE[form][1]


@pytest.mark.parametrize("form,S,max_q", SCALES)
@pytest.mark.parametrize("dim", DIMS)
def test_no_pair_of_a_rejected_row_reaches_the_bias(form, S, max_q, dim):
    N = FORMS[form]
    bias, K = F32(N["bias"]), PASS_NONE[form]
    lo, hi = BINADE[form]
    qc = np.array([0, 1, dim * max_q // 2, dim * max_q - 1, dim * max_q], np.int64)   # every bit set against the largest query value
    if form == "int8":   # the i32 accumulator: the start value's bits + qcDist
        final_bits = np.int64(K.view(np.int32)) + qc
        final = final_bits.astype(np.int32).view(F32)
        assert (final_bits <= np.int64(bias.view(np.int32))).all() and (final_bits < np.int64(bias.view(np.int32))).all()
        assert (final.astype(np.float64) == float(K) + qc).all()                       # bits + integer IS float + integer inside [2^23, 2^24)
    else:                # the f32 accumulator: multiples of 1/16 inside one binade
        final = (np.float64(K) + S * qc).astype(F32)
        assert (final.astype(np.float64) == float(K) + S * qc).all()                   # exact
    assert (final < bias).all() and (final >= lo).all() and (final < hi).all()
    # the margin the kernel's comment derives: the largest S * qcDist is below the distance from pass_none to the bias
    assert S * dim * max_q < float(bias - K)
    # "passes" is the integer compare of the accumulator's bits against the bias's (both forms)
    assert not (final.view(np.int32) > bias.view(np.int32)).any()


@pytest.mark.parametrize("form", ["int8", "fp"])
def test_zero_row_constants_leave_the_start_value_alone(form):
    """start_values(): K x 1 first, then q0 r0 | q2 r2, q3 r3 | q1 r1 as chained f32 FMAs.  With r0 = r1 = r2 = r3 = 0 every product
    is a signed zero and K comes out bit for bit - for the extreme query constants the filtered prologue can produce: qk.x = -3.0e38
    (a threshold beyond every score, and a lane without a query), |qk.y| up to 3.0e38 (the filtered prologue's clamp of S * ay / ly,
    which mfma_query_ok admits up to 1e60 - unclamped, an infinite f32 image times zero would be NaN), |qk.z| = S |y1| and
    qk.w = S / beta up to 1e30 (mfma_query_ok's limits), in either sign."""
    K = PASS_NONE[form]
    zero = F32(0.0)
    big = [F32(-3.0e38), F32(3.0e38)]
    for S in ((1.0,) if form == "int8" else (0.25, 0.5, 1.0)):
        for q0 in (F32(-3.0e38), F32(-1.0e30), F32(1.0e30), F32(0.0)):
            for q1 in big + [F32(np.clip(-S * 1e60, -3.0e38, 3.0e38))]:
                for q2 in (F32(-S * 1e30), F32(S * 1e30)):
                    for q3 in (F32(-S * 1e30), F32(-S * 1e-30)):
                        for z in (zero, -zero):
                            init = fma32(q1, z, fma32(q3, z, fma32(q2, z, fma32(q0, z, fma32(F32(1.0), K, F32(0.0))))))
                            assert np.isfinite(init) and init.view(np.uint32) == K.view(np.uint32)
    # ... and what the clamp is for: the unclamped image is infinite, and inf x 0 is NaN - not pass_none (a quiet NaN with a clear sign
    # bit, the device's default, compares ABOVE the bias as an integer)
    with np.errstate(all="ignore"):
        unclamped = F32(-0.25 * 1e60)
        bad = (np.float64(unclamped) * 0.0 + np.float64(K)).astype(F32)
    assert np.isinf(unclamped) and np.isnan(bad)
    assert np.uint32(0x7FC00000).view(np.int32) > F32(FORMS[form]["bias"]).view(np.int32)
