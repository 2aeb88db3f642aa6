"""GPU: the exact MaxSim rerank through the JavaScript host (N-API addon over libbbq) under node: computeMaxSimGroupTrueScores and
getOversampledMaxSimTopK return, byte for byte, what the ctypes binding returns for the fixture's first queries taken as one query's token
vectors - which tests/test_gpu_maxsim_rerank.py holds to the model."""
import base64
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from bbqlib import ROOT

CASE = "c1_1000x128_cos_qb4"
SIM_NAMES = ["EUCLIDEAN", "COSINE", "MAXIMUM_INNER_PRODUCT"]


def _b64(a):
    return base64.b64encode(np.ascontiguousarray(a).tobytes()).decode("ascii")


def _ctypes_answers(path):
    import orclib as O
    import test_gpu_score_ords as SO
    import test_groups_cpu as GC
    from bbqlib import bbq_amd as B, capi
    g, sim, codes, corr, cdp, qs = SO._case(CASE)
    base, queries = O.golden_inputs(g)
    T = min(len(qs), 5)
    off = GC.layouts(g["n"])["random_1_20"]
    tok = [(np.stack([qs[i][0] for i in range(T)]), np.stack([qs[i][1] for i in range(T)]))]
    raw = [np.stack([queries[i] for i in range(T)]).astype(np.float32)]
    rng = np.random.default_rng(9)
    cand = rng.permutation(len(off) - 1)[:40]
    cand = np.concatenate([cand, cand[3:5]])
    ix = B.Index(codes, corr, g["dim"], cdp)
    V = capi.Vectors(base)
    try:
        with capi.Groups(ix, off) as groups:
            true = {SIM_NAMES[s]: _b64(V.rerank_maxsim_groups_batch(raw, groups, [cand], s)[0].astype("<f8")) for s in range(3)}
            recipe = []
            for k, factor in ((1, 1), (10, 3), (200, 2)):
                for selector in ("heap", "sort"):
                    grp, qsc, tsc = capi.search_maxsim_rerank_batch(ix, V, groups, raw, tok, g["qb"], sim, k, factor, 1 if selector == "sort" else 0, 1)[0]
                    recipe.append({"k": k, "factor": factor, "selector": selector, "group_i32": _b64(grp.astype("<i4")), "quant_f32": _b64(qsc.astype("<f4")),
                                   "true_f64": _b64(tsc.astype("<f8"))})
    finally:
        V.close()
        ix.close()
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"name": CASE, "tokens": T, "layout": [int(x) for x in off], "cand_i32": _b64(cand.astype("<i4")), "true_f64": true, "recipe": recipe}, f)


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_exact_maxsim_rerank_matches_the_ctypes_binding(tmp_path):
    path = tmp_path / "maxsim_rerank_answers.json"
    _ctypes_answers(path)
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "maxsim_rerank.js"), str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "0 failures" in r.stdout
