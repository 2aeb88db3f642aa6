"""GPU: the exact search through the JavaScript host (N-API addon over libbbq) under node: getTrueTopK and DeviceVectors.trueTopK return
the indices - and trueTopK the score bytes - of the model of tests/exact_model.py (the oracle's computeSimilarity and its stable
descending sort) for the README's 1000 x 128 case, for rows that tie, and with and without a RowFilter."""
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
DUPS = [[20, 7], [21, 7], [63, 7], [64, 7], [300, 7], [999, 7], [500, 499]]   # row dst becomes a copy of row src
NQ = 4


def _b64(a):
    return base64.b64encode(np.ascontiguousarray(a).tobytes()).decode("ascii")


def _model_answers(path):
    import orclib as O
    import exact_model as EM
    g = O.load_golden(CASE)
    base, queries = O.golden_inputs(g)
    base, queries = np.array(base, np.float32), np.array(queries, np.float32)[:NQ]
    tied = base.copy()
    for dst, src in DUPS:
        tied[dst] = base[src]
    tie_queries = np.concatenate([queries[:1], base[7:8]])      # the second one has the copies of row 7 on top
    mask = (np.arange(g["n"]) % 3 != 0) & ~((np.arange(g["n"]) >= 128) & (np.arange(g["n"]) < 256))
    cases = []
    for label, rows, qs, m, sims in (("plain", base, queries, None, (0, 1, 2)), ("ties", tied, tie_queries, None, (1,)), ("filtered", base, queries, mask, (1, 2)),
                                     ("ties, filtered", tied, tie_queries, mask, (1,))):
        for sim in sims:
            c = EM.scores(qs, rows, sim)
            for k in (1, 10, 100, 1005):
                want = [EM.topk(c[q], k, m) for q in range(qs.shape[0])]
                cases.append({"label": label, "sim": SIM_NAMES[sim], "k": k, "tied": label.startswith("ties"), "filtered": m is not None,
                              "idx_i32": [_b64(w[0].astype("<i4")) for w in want], "bits_u64": [_b64(w[1].astype("<u8")) for w in want]})
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"name": CASE, "dups": DUPS, "nq": NQ, "mask_u8": _b64(mask.astype(np.uint8)), "cases": cases}, f)


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_exact_search_matches_the_model(tmp_path):
    path = tmp_path / "exact_answers.json"
    _model_answers(path)
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "exact.js"), str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "0 failures" in r.stdout
