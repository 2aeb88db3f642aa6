"""GPU: the filtered search of the JavaScript host (N-API addon over libbbq) under node: the three forms of `accept`, the batch
method, dispose, parity with the ctypes answers on two fixtures, and the library's message on a multi-device index (BBQ_DEVICES)."""
import base64
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from bbqlib import ROOT

CASES = ["m_768d_cos_qb4", "ties_cos_qb4"]


def _b64(a):
    return base64.b64encode(np.ascontiguousarray(a).tobytes()).decode("ascii")


def _ctypes_answers(path):
    """filtered answers through the ctypes binding (itself pinned to the oracle by tests/test_gpu_filtered.py)"""
    import orclib as O
    from bbqlib import bbq_amd as B, capi
    cases = []
    for name in CASES:
        g = O.load_golden(name)
        sim = O.SIMS[g["sim"]]
        base, queries = O.golden_inputs(g)
        codes, corr, cen = B.quantize_vectors(base, sim, g["ib"], g["lambda"], g["iters"])
        mask = np.random.default_rng(31).random(g["n"]) < 0.4
        ix = B.Index(codes, corr, g["dim"], B.centroid_dp(cen), index_bits=g["ib"])
        try:
            with capi.Filter(ix, mask) as flt:
                answers = []
                for qi in range(g["nq"]):
                    qq, qc = B.quantize_query(queries[qi], cen, sim, g["qb"], g["lambda"], g["iters"])
                    for k in (1, 10, 100):
                        idx, sc = ix.search_filtered(qq, qc, g["qb"], sim, k, flt)
                        answers.append({"q": qi, "k": k, "idx_i32": _b64(idx.astype("<i4")), "score_f32": _b64(sc.astype("<f4"))})
        finally:
            ix.close()
        cases.append({"name": name, "mask_u8": _b64(mask.astype(np.uint8)), "answers": answers})
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"cases": cases}, f)


def _node(path, env=None):
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "gpu_filtered.js"), str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600, env=env)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "0 failures" in r.stdout
    return r.stdout


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_filtered_matches_ctypes(tmp_path):
    path = tmp_path / "filtered_answers.json"
    _ctypes_answers(path)
    _node(path)


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_filtered_on_a_multi_device_index_throws_unsupported(tmp_path):
    path = tmp_path / "filtered_answers.json"
    _ctypes_answers(path)
    out = _node(path, env=dict(os.environ, BBQ_DEVICES="0,0", BBQ_PILOT_ROWS="1024"))
    assert "(sharded)" in out
