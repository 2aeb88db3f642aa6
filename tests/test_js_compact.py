"""GPU: removeVectors / compactVectors of the JavaScript host (N-API addon over libbbq) under node: size(), vectorValue,
getCorrectiveTerms and searchNearestNeighbors equal the ctypes results for the index over the kept rows (themselves pinned to the oracle
by tests/test_gpu_compact.py).  The host copies are never stale: with the copies present, after loadIndex where they are absent, with
the accept set on the device alone (a RowFilter) and without a device copy; DeviceVectors.compact; a multi-device index refuses."""
import base64
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from bbqlib import ROOT

CASES = ["m_768d_cos_qb4", "ties_cos_qb4", "ib2_100d_euc_qb4"]


def _b64(a):
    return base64.b64encode(np.ascontiguousarray(a).tobytes()).decode("ascii")


def drop_and_mask(n):
    """what tests/js/gpu_compact.js does to every set: removeVectors(drop), then compactVectors(mask) over the n - 3 rows left"""
    drop = [n - 1, 0, 5, 5]
    mask = (np.arange(n - 3) * 7 + 3) % 10 < 6
    return drop, mask


def _ctypes_answers(path):
    import orclib as O
    from bbqlib import bbq_amd as B, capi
    cases = []
    for name in CASES:
        g = O.load_golden(name)
        sim = O.SIMS[g["sim"]]
        base, queries = O.golden_inputs(g)
        drop, mask = drop_and_mask(g["n"])
        ix, codes, corr, cen = B.Index.build(base, sim, g["lambda"], g["iters"], index_bits=g["ib"])
        try:
            ix.remove_rows(drop)
            after_drop = ix.n
            with capi.Filter(ix, mask) as flt:
                ix.compact(flt)
            keep = np.ones(g["n"], bool)
            keep[drop] = False
            kept = np.flatnonzero(keep)[mask]
            assert ix.n == len(kept)
            ecodes, ecorr = ix.export()
            np.testing.assert_array_equal(ecodes, codes[kept])
            answers = []
            for qi in range(g["nq"]):
                qq, qc = B.quantize_query(queries[qi], cen, sim, g["qb"], g["lambda"], g["iters"])
                for k in (1, 10, 100):
                    idx, sc = ix.search(qq, qc, g["qb"], sim, k)
                    answers.append({"q": qi, "k": k, "idx_i32": _b64(idx.astype("<i4")), "score_f32": _b64(sc.astype("<f4"))})
        finally:
            ix.close()
        cases.append({"name": name, "drop": drop, "after_drop": after_drop, "mask_u8": _b64(mask.astype(np.uint8)), "kept_i32": _b64(kept.astype("<i4")),
                      "codes_u8": _b64(ecodes), "corr_f64": _b64(ecorr.astype("<f8")), "answers": answers})
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"cases": cases}, f)


def _node(path, tmp_path, env=None):
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "gpu_compact.js"), str(path), str(tmp_path)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600, env=env)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "0 failures" in r.stdout
    return r.stdout


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_compact_matches_ctypes(tmp_path):
    path = tmp_path / "compact_answers.json"
    _ctypes_answers(path)
    _node(path, tmp_path)


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_compact_on_a_multi_device_index_throws_unsupported(tmp_path):
    path = tmp_path / "compact_answers.json"
    _ctypes_answers(path)
    out = _node(path, tmp_path, env=dict(os.environ, BBQ_DEVICES="0,0", BBQ_PILOT_ROWS="1024"))
    assert "(sharded)" in out
