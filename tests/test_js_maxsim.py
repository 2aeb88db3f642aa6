"""GPU: MaxSim search through the JavaScript host (N-API addon over libbbq) under node: searchNearestNeighborsMaxSim equals the model of
tests/maxsim_model.py over the golden f32 scores of the fixture's queries taken as one query's token vectors, with and without a row
filter, as tests/test_gpu_maxsim.py holds the ctypes binding to it."""
import base64
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from bbqlib import ROOT

CASE = "c1_1000x128_cos_qb4"
LAYOUTS = ["singletons", "one_group", "groups_of_65", "random_1_20", "empty_groups"]
MASKS = ["all", "drop_every_third", "none"]


def _b64(a):
    return base64.b64encode(np.ascontiguousarray(a).tobytes()).decode("ascii")


def _model_answers(path):
    import maxsim_model as M
    import test_spans_cpu as SC
    import test_spans_filtered_cpu as FC
    import test_groups_cpu as GC
    n, scores = SC.golden_scores(CASE)
    masks, lays = FC.masks(n), GC.layouts(n)
    answers = []
    for lname in LAYOUTS:
        for mname in MASKS:
            for tokens in sorted({1, 2, len(scores)}):
                live = GC.plan(lays[lname], masks[mname])[1]
                for k in sorted({1, 10, max(live - 1, 0), live + 5}):
                    groups, sc, _, L = M.answer(scores[:tokens], lays[lname], masks[mname], k)
                    assert L == live
                    answers.append({"tokens": tokens, "k": int(k), "layout": lname, "mask": mname, "group_i32": _b64(groups.astype("<i4")),
                                    "score_f32": _b64(sc.astype("<f4"))})
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"name": CASE, "masks": {m: _b64(masks[m].astype(np.uint8)) for m in MASKS},
                   "layouts": {l: [int(x) for x in lays[l]] for l in LAYOUTS}, "answers": answers}, f)


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_maxsim_search_matches_the_model(tmp_path):
    path = tmp_path / "maxsim_answers.json"
    _model_answers(path)
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "maxsim.js"), str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "0 failures" in r.stdout
