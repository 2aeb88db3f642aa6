"""GPU: updateVectors of the JavaScript host (N-API addon over libbbq) under node: the row accessors over the updated ords and
searchNearestNeighbors before and after equal the ctypes results for the same rows (themselves pinned to the oracle by
tests/test_gpu_update.py); a RowFilter made before the update still serves; DeviceVectors.update; a loaded index whose host copies are
fetched lazily; the host-quantizer branch (BBQ_HOST_QUANTIZER=1) gives identical results; the library's message on a multi-device index."""
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


def _ctypes_answers(path):
    import orclib as O
    from bbqlib import bbq_amd as B, capi
    cases = []
    for name in CASES:
        g = O.load_golden(name)
        sim, n = O.SIMS[g["sim"]], g["n"]
        base, queries = O.golden_inputs(g)
        d = n // 2
        ords = [e for e in (0, 63, 64, 65, n - 1) if e < n] + [d, 1, d, 2, d]   # tile edges, and one ord three times
        frm = [(7 * o + 3 + i) % n for i, o in enumerate(ords)]
        mask = np.arange(n) % 2 == 0
        ix, codes, corr, cen = B.Index.build(base, sim, g["lambda"], g["iters"], index_bits=g["ib"])
        try:
            qs = [B.quantize_query(queries[qi], cen, sim, g["qb"], g["lambda"], g["iters"]) for qi in range(g["nq"])]

            def answers(ks, flt=None):
                out = []
                for qi, (qq, qc) in enumerate(qs):
                    for k in ks:
                        idx, sc = ix.search(qq, qc, g["qb"], sim, k) if flt is None else ix.search_filtered(qq, qc, g["qb"], sim, k, flt)
                        out.append({"q": qi, "k": k, "idx_i32": _b64(idx.astype("<i4")), "score_f32": _b64(sc.astype("<f4"))})
                return out

            before = answers((10,))
            with capi.Filter(ix, mask) as flt:   # made before the update
                bcodes, bcorr = ix.update(ords, base[frm], cen, sim, g["lambda"], g["iters"])
                filtered = answers((10,), flt) if g["ib"] == 1 else []
            after = answers((1, 10, 100))
            assert ix.n == n
        finally:
            ix.close()
        cases.append({"name": name, "ords": ords, "frm": frm, "block_codes_u8": _b64(bcodes), "block_corr_f64": _b64(bcorr.astype("<f8")),
                      "before": before, "after": after, "filtered": filtered})
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"cases": cases}, f)


def _node(path, tmp_path, env=None):
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "gpu_update.js"), str(path), str(tmp_path)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600, env=env)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "0 failures" in r.stdout
    return r.stdout


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_update_matches_ctypes(tmp_path):
    path = tmp_path / "update_answers.json"
    _ctypes_answers(path)
    _node(path, tmp_path)
    out = _node(path, tmp_path, env=dict(os.environ, BBQ_HOST_QUANTIZER="1"))
    assert "(host quantizer)" in out


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_update_on_a_multi_device_index_throws_unsupported(tmp_path):
    path = tmp_path / "update_answers.json"
    _ctypes_answers(path)
    out = _node(path, tmp_path, env=dict(os.environ, BBQ_DEVICES="0,0", BBQ_PILOT_ROWS="1024"))
    assert "(sharded)" in out
