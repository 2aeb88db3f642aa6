"""GPU: filtered span search through the JavaScript host (N-API addon over libbbq) under node: searchNearestNeighborsInSpansFiltered equals
the oracle's heap over the golden f32 scores of the accepted rows of each span set, as tests/test_gpu_spans_filtered.py holds the ctypes
binding to it, and equals searchNearestNeighborsFiltered when one span covers everything."""
import base64
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from bbqlib import ROOT

CASES = ["c1_1000x128_cos_qb4"]
MASKS = ["drop_every_third", "tile_out_and_ends", "sparse_61", "none"]


def _b64(a):
    return base64.b64encode(np.ascontiguousarray(a).tobytes()).decode("ascii")


def _oracle_answers(path):
    import orclib as O
    import test_spans_cpu as SC
    import test_spans_filtered_cpu as FC
    cases = []
    for name in CASES:
        n, scores = SC.golden_scores(name)
        masks = FC.masks(n)
        answers = []
        for mname in MASKS:
            for qi, s32 in enumerate(scores[:2]):
                for sp in SC.span_sets(n):
                    rows = FC.accepted(masks[mname], sp)
                    for k in sorted({1, 10, max(len(rows) - 1, 0), len(rows) + 5}):
                        oi, osc = O.heap_topk(s32[rows], k)
                        answers.append({"q": qi, "k": int(k), "mask": mname, "spans": sp.tolist(), "idx_i32": _b64(rows[oi].astype("<i4")),
                                        "score_f32": _b64(osc.astype("<f4"))})
        cases.append({"name": name, "masks": {m: _b64(masks[m].astype(np.uint8)) for m in MASKS}, "answers": answers})
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"cases": cases}, f)


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_filtered_spans_match_the_oracle(tmp_path):
    path = tmp_path / "span_filtered_answers.json"
    _oracle_answers(path)
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "spans_filtered.js"), str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "0 failures" in r.stdout
