"""GPU: MaxSim over chosen groups through the JavaScript host (N-API addon over libbbq) under node: searchNearestNeighborsMaxSimInGroups
and computeMaxSimGroupScores equal the model of tests/maxsim_groups_model.py over the golden f32 scores of the fixture's queries taken
as one query's token vectors - candidate lists ascending, shuffled and with a duplicate, with and without a row filter - as
tests/test_gpu_maxsim_groups.py holds the ctypes binding to it."""
import base64
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from bbqlib import ROOT

CASE = "c1_1000x128_cos_qb4"
LAYOUTS = ["singletons", "groups_of_65", "random_1_20", "empty_groups"]
MASKS = ["all", "drop_every_third"]


def _b64(a):
    return base64.b64encode(np.ascontiguousarray(a).tobytes()).decode("ascii")


def _model_answers(path):
    import maxsim_model as M
    import maxsim_groups_model as MG
    import test_spans_cpu as SC
    import test_spans_filtered_cpu as FC
    import test_groups_cpu as GC
    n, scores = SC.golden_scores(CASE)
    masks, lays = FC.masks(n), GC.layouts(n)
    rng = np.random.default_rng(77)
    answers = []
    for lname in LAYOUTS:
        for mname in MASKS:
            for tokens in sorted({1, len(scores)}):
                rep, live = M.rep_scores(scores[:tokens], lays[lname], masks[mname])
                shuffled = rng.permutation(live)[:50]
                lists = {"ascending": live, "shuffled": shuffled, "duplicate": np.concatenate([shuffled[:7], shuffled[2:4], shuffled[:1]])}
                for name, lst in lists.items():
                    S = MG.scores(rep, live, lst)
                    for k in sorted({1, 10, len(lst) + 5}):
                        groups, sc = MG.answer(rep, live, lst, k)
                        answers.append({"tokens": tokens, "k": int(k), "layout": lname, "mask": mname, "list": name, "cand_i32": _b64(lst.astype("<i4")),
                                        "all_f32": _b64(S.astype("<f4")), "group_i32": _b64(groups.astype("<i4")), "score_f32": _b64(sc.astype("<f4"))})
    dead = {l: int(np.flatnonzero(GC.plan(lays[l], masks["drop_every_third"])[0] < 0)[0]) for l in ("singletons", "empty_groups")}
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"name": CASE, "masks": {m: _b64(masks[m].astype(np.uint8)) for m in MASKS}, "layouts": {l: [int(x) for x in lays[l]] for l in LAYOUTS},
                   "answers": answers, "dead": dead}, f)


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_maxsim_over_chosen_groups_matches_the_model(tmp_path):
    path = tmp_path / "maxsim_groups_answers.json"
    _model_answers(path)
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "maxsim_groups.js"), str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "0 failures" in r.stdout
