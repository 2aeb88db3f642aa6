"""CPU: what bbq_quantize_queries_device and option device_queries refuse before any device is needed: the quantizer's argument checks
with its messages, then the null handle."""
import ctypes as C

import numpy as np
import pytest

from bbqlib import capi


def _call(n=2, q=True, cen=True, sim=1, qb=4, lam=0.1, iters=5, out=True, handle=None):
    a = {k: np.zeros(s, t) for k, s, t in (("q", 16, np.float32), ("cen", 8, np.float32), ("qq", 16, np.uint8), ("qc", 8, np.float64))}
    bad = C.c_int32(7)
    rc = capi.lib().bbq_quantize_queries_device(handle, n, a["q"].ctypes.data if q else None, a["cen"].ctypes.data if cen else None, sim, qb, lam,
                                                iters, a["qq"].ctypes.data if out else None, a["qc"].ctypes.data if out else None, C.byref(bad))
    return rc, bad.value, capi.lib().bbq_last_error().decode("utf-8")


@pytest.mark.parametrize("kw,text", [({}, "index handle is null"), ({"n": -1}, "n < 0"), ({"q": False}, "输入向量不能为空"), ({"cen": False}, "输入向量不能为空"),
                                     ({"sim": 3}, "不支持的相似性函数: 3"), ({"sim": -1}, "不支持的相似性函数: -1"), ({"qb": 0}, "位数必须在1-8之间"),
                                     ({"qb": 9}, "位数必须在1-8之间"), ({"iters": -1}, "bad lambda/iters"), ({"lam": float("nan")}, "bad lambda/iters"),
                                     ({"out": False}, "null output")])
def test_refused_without_a_device(kw, text):
    rc, bad, message = _call(**kw)
    assert rc == capi.ERR_INVALID_ARG and bad == -1 and text in message


def test_nothing_to_do_and_the_option():
    assert _call(n=0)[:2] == (capi.OK, -1)
    assert capi.lib().bbq_set_option(None, b"device_queries", 1) == capi.ERR_INVALID_ARG


def test_the_raw_call_hands_device_quantized_queries_on_without_a_feed():
    """bbq_search_raw_batch under device_queries 1 (csrc/bbq_core.cpp): the whole batch through the device quantizer, then search_batch_impl
    with a null feed and a null bad_query - planes, maxq and the single-query chains are bbq_search_batch's on the same bytes, which is
    what tests/call_walk.py (raw_call_prepares) and the device_queries tests of tests/test_gpu_rawbatch_sweeps.py rest on"""
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "better-binary-quantization_amd", "csrc", "bbq_core.cpp"), encoding="utf-8") as f:
        core = f.read()
    block = re.search(r"  // option device_queries: all queries through the device quantizer \(bbq_query_device\.cpp\), then the search of prepared queries\n"
                      r"  if \(device_queries_for_call\(ix\)\) \{\n"
                      r"    int rc = bbq_quantize_queries_device\(ix, n_queries, queries, centroid, sim, query_bits, lambda, iters, qq, qc, bad_query\);\n"
                      r"    if \(rc != BBQ_OK\) return rc;\n"
                      r"    return search_batch_impl\(ix, n_queries, qq, qc, query_bits, sim, k, out_idx, out_score, out_n, nullptr, nullptr\);\n"
                      r"  \}\n", core)
    assert block, "the composition of bbq_search_raw_batch under device_queries 1 has changed: the call walk's model restates it"
    assert core.index("if (device_queries_for_call(ix)) {") < core.index("if (n_queries <= 64 || k == 0 || ix->multi) {") < core.index("RawFeed feed;")
    assert "if (n_queries == 1 && plan.latency && !feed && !flt) {" in core and "if (feed) {  // the values are still being produced" in core
