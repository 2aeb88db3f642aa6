"""GPU: scoring chosen rows through the JavaScript host (N-API addon over libbbq) under node: computeBatchQuantizedScores over a
scattered list with a duplicate equals per-ord calls, and searchNearestNeighborsInOrds equals the ctypes answers for the same lists
(themselves pinned to the oracle by tests/test_gpu_score_ords.py); the same with the index row-sharded behind one handle."""
import base64
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from bbqlib import ROOT

CASES = ["c1_1000x128_cos_qb4"]


def _b64(a):
    return base64.b64encode(np.ascontiguousarray(a).tobytes()).decode("ascii")


def _ctypes_answers(path):
    import orclib as O
    from bbqlib import bbq_amd as B
    cases = []
    for name in CASES:
        g = O.load_golden(name)
        sim, n = O.SIMS[g["sim"]], g["n"]
        base, queries = O.golden_inputs(g)
        codes, corr, cen = B.quantize_vectors(base, sim, g["ib"], g["lambda"], g["iters"])
        rng = np.random.default_rng(31)
        lists = [np.arange(n - 1, -1, -1), rng.integers(0, n, 300), np.array([n - 1, 0, 17, 17])]
        ix = B.Index(codes, corr, g["dim"], B.centroid_dp(cen), index_bits=g["ib"])
        answers = []
        try:
            for qi in range(g["nq"]):
                qq, qc = B.quantize_query(queries[qi], cen, sim, g["qb"], g["lambda"], g["iters"])
                for ords in lists:
                    for k in (1, 10, len(ords) + 3):
                        idx, sc = ix.search_ords_batch(qq[None, :], qc[None, :], g["qb"], sim, k, [ords])[0]
                        answers.append({"q": qi, "k": k, "ords_i32": _b64(ords.astype("<i4")), "idx_i32": _b64(idx.astype("<i4")),
                                        "score_f32": _b64(sc.astype("<f4"))})
        finally:
            ix.close()
        cases.append({"name": name, "answers": answers})
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"cases": cases}, f)


def _node(path, env=None):
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "score_ords.js"), str(path)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600, env=env)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "0 failures" in r.stdout
    return r.stdout


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_score_ords_matches_ctypes(tmp_path):
    path = tmp_path / "score_ords_answers.json"
    _ctypes_answers(path)
    _node(path)
    out = _node(path, env=dict(os.environ, BBQ_DEVICES="0,0,0", BBQ_PILOT_ROWS="512"))
    assert "(sharded)" in out
