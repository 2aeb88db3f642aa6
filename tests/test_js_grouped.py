"""GPU: grouped search through the JavaScript host (N-API addon over libbbq) under node: searchNearestNeighborsGrouped equals the oracle's
heap over the golden f32 scores of the model's representatives (tests/test_groups_cpu.py), with and without a row filter, as
tests/test_gpu_grouped.py holds the ctypes binding to it."""
import base64
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from bbqlib import ROOT

CASES = ["c1_1000x128_cos_qb4", "m_768d_cos_qb4"]
LAYOUTS = ["singletons", "one_group", "groups_of_65", "random_1_20", "empty_groups"]
MASKS = ["all", "drop_every_third", "sparse_61", "none"]


def _b64(a):
    return base64.b64encode(np.ascontiguousarray(a).tobytes()).decode("ascii")


def _oracle_answers(path):
    import orclib as O
    import test_spans_cpu as SC
    import test_spans_filtered_cpu as FC
    import test_groups_cpu as GC
    cases = []
    for name in CASES:
        n, scores = SC.golden_scores(name)
        masks, lays = FC.masks(n), GC.layouts(n)
        names = [l for l in LAYOUTS if l in lays]
        answers = []
        for lname in names:
            for mname in MASKS:
                slot, live = GC.plan(lays[lname], masks[mname])
                for qi, s32 in enumerate(scores[:2]):
                    ords, groups = GC.representatives(s32, lays[lname], masks[mname])
                    for k in sorted({1, 10, max(live - 1, 0), live + 5}):
                        oi, osc = O.heap_topk(s32[ords], k)
                        answers.append({"q": qi, "k": int(k), "layout": lname, "mask": mname, "live": live, "idx_i32": _b64(ords[oi].astype("<i4")),
                                        "group_i32": _b64(groups[oi].astype("<i4")), "score_f32": _b64(osc.astype("<f4"))})
        cases.append({"name": name, "masks": {m: _b64(masks[m].astype(np.uint8)) for m in MASKS},
                      "layouts": {l: [int(x) for x in lays[l]] for l in names}, "answers": answers})
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"cases": cases}, f)


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_grouped_search_matches_the_oracle(tmp_path):
    path = tmp_path / "grouped_answers.json"
    _oracle_answers(path)
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "grouped.js"), str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "0 failures" in r.stdout
