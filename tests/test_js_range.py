"""GPU: range search through the JavaScript host (N-API addon over libbbq) under node: searchRange equals the ctypes answers for the
same fixture, thresholds and filter (themselves pinned to the golden scores by tests/test_gpu_range.py), in both orders."""
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
    from bbqlib import bbq_amd as B, capi
    cases = []
    for name in CASES:
        g = O.load_golden(name)
        sim, n = O.SIMS[g["sim"]], g["n"]
        base, queries = O.golden_inputs(g)
        codes, corr, cen = B.quantize_vectors(base, sim, g["ib"], g["lambda"], g["iters"])
        mask = np.random.default_rng(41).random(n) < 0.5
        ix = B.Index(codes, corr, g["dim"], B.centroid_dp(cen), index_bits=g["ib"])
        answers = []
        try:
            with capi.Filter(ix, mask) as flt:
                for qi in range(g["nq"]):
                    qq, qc = B.quantize_query(queries[qi], cen, sim, g["qb"], g["lambda"], g["iters"])
                    s32 = np.sort(ix.score_rows(qq, qc, g["qb"], sim)[2])
                    for t in (np.float32(-np.inf), s32[n // 2], s32[-3], np.nextafter(s32[-1], np.float32(np.inf))):
                        for f in (None, flt):
                            idx, sc, _ = ix.search_range_batch(qq[None, :], qc[None, :], g["qb"], sim, [t], f)
                            by = np.argsort(-sc, kind="stable")
                            answers.append({"q": qi, "threshold_f32": _b64(np.array([t], "<f4")), "filtered": f is not None,
                                            "idx_i32": _b64(idx.astype("<i4")), "score_f32": _b64(sc.astype("<f4")),
                                            "by_score_idx_i32": _b64(idx[by].astype("<i4")), "by_score_f32": _b64(sc[by].astype("<f4"))})
        finally:
            ix.close()
        cases.append({"name": name, "mask_u8": _b64(mask.astype(np.uint8)), "answers": answers})
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"cases": cases}, f)


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_range_matches_ctypes(tmp_path):
    path = tmp_path / "range_answers.json"
    _ctypes_answers(path)
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "range.js"), str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "0 failures" in r.stdout
