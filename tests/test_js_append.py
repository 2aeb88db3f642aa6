"""GPU: appendVectors of the JavaScript host (N-API addon over libbbq) under node: size(), the row accessors over the new ords and
searchNearestNeighbors equal the ctypes results for the same rows (themselves pinned to the oracle by tests/test_gpu_append.py);
DeviceVectors.append and reserve; a loaded index whose host copies are fetched lazily; the library's message on a multi-device index."""
import base64
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from bbqlib import ROOT

CASES = [("m_768d_cos_qb4", 130), ("ties_cos_qb4", 1001), ("ib2_100d_euc_qb4", 64)]


def _b64(a):
    return base64.b64encode(np.ascontiguousarray(a).tobytes()).decode("ascii")


def _ctypes_answers(path):
    import orclib as O
    from bbqlib import bbq_amd as B
    cases = []
    for name, cut in CASES:
        g = O.load_golden(name)
        sim = O.SIMS[g["sim"]]
        base, queries = O.golden_inputs(g)
        ix, codes, corr, cen = B.Index.build(base[:cut], sim, g["lambda"], g["iters"], index_bits=g["ib"])
        try:
            bcodes, bcorr = ix.append(base[cut:], cen, sim, g["lambda"], g["iters"])
            answers = []
            for qi in range(g["nq"]):
                qq, qc = B.quantize_query(queries[qi], cen, sim, g["qb"], g["lambda"], g["iters"])
                for k in (1, 10, 100):
                    idx, sc = ix.search(qq, qc, g["qb"], sim, k)
                    answers.append({"q": qi, "k": k, "idx_i32": _b64(idx.astype("<i4")), "score_f32": _b64(sc.astype("<f4"))})
            size = ix.n
        finally:
            ix.close()
        cases.append({"name": name, "cut": cut, "size": size, "new_codes_u8": _b64(bcodes), "new_corr_f64": _b64(bcorr.astype("<f8")), "answers": answers})
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"cases": cases}, f)


def _node(path, tmp_path, env=None):
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "gpu_append.js"), str(path), str(tmp_path)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600, env=env)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "0 failures" in r.stdout
    return r.stdout


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_append_matches_ctypes(tmp_path):
    path = tmp_path / "append_answers.json"
    _ctypes_answers(path)
    _node(path, tmp_path)


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_append_on_a_multi_device_index_throws_unsupported(tmp_path):
    path = tmp_path / "append_answers.json"
    _ctypes_answers(path)
    out = _node(path, tmp_path, env=dict(os.environ, BBQ_DEVICES="0,0", BBQ_PILOT_ROWS="1024"))
    assert "(sharded)" in out
