"""bench.py --gpus N starts N real ranks by itself (fresh child processes before any GPU call) or fails - it never prints
a line that claims N GPUs while measuring fewer.  CPU: the launch path with --dry-run (no device, no
measurement).  GPU: the same path with real work, two ranks sharing the box's one GPU over gloo."""
import json
import os
import subprocess
import sys

import pytest

from bbqlib import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def _run(argv, env=None, timeout=600):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    r = subprocess.run([sys.executable, BENCH] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, env=e)
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    return r, lines


@pytest.mark.parametrize("n", [2, 3])
def test_self_launch_starts_n_ranks(n):
    r, lines = _run(["--gpus", str(n), "--dry-run"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert len(lines) == 1, lines                       # ONE JSON line on stdout, whatever the ranks chatter about
    out = json.loads(lines[0])
    assert out["n_gpus"] == n and out["ranks"] == n and out["dry_run"] is True and out["value"] is None


def test_single_gpu_needs_no_launcher():
    r, lines = _run(["--gpus", "1", "--dry-run"])
    assert r.returncode == 0 and json.loads(lines[0])["n_gpus"] == 1


def test_world_size_mismatch_is_an_error():
    r, lines = _run(["--gpus", "2", "--dry-run"], env={"WORLD_SIZE": "4", "RANK": "0"})
    assert r.returncode != 0 and not lines
    assert "refusing" in r.stderr


def test_too_few_devices_is_an_error():
    import torch
    if torch.cuda.device_count() >= 64:
        pytest.skip("64 devices visible")
    r, lines = _run(["--gpus", "64", "--no-recall"])
    assert r.returncode != 0 and not lines
    assert "HIP device(s) visible" in r.stderr


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_through_the_self_launch_path():
    r, lines = _run(["--gpus", "2", "--backend", "gloo", "--same-device", "--rows", "400000", "--steps", "2", "--warmup", "1",
                     "--batch", "64", "--full", "--no-recall", "--no-cpu-baseline"], timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["ranks"] == 2 and out["backend"] == "gloo"
    assert out["parity_full_size"] is True
    assert out["value"] > 0


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_dumps_its_last_step(tmp_path):
    """without --full the line carries the headline step alone; --dump-outputs writes the answers of the last timed step, the same
    in every run with the same arguments, and they are the oracle's"""
    import numpy as np
    import bbq_amd
    import bench
    import orclib as O
    rows, dim, k, Q, steps, warmup = 300000, 768, 100, 64, 3, 1
    argv = ["--gpus", "1", "--rows", str(rows), "--steps", str(steps), "--warmup", str(warmup), "--batch", str(Q)]
    runs = []
    for i in range(2):
        d = str(tmp_path / ("run%d" % i))
        r, lines = _run(argv + ["--dump-outputs", d])
        assert r.returncode == 0, r.stderr[-4000:]
        assert len(lines) == 1, lines
        runs.append((json.loads(lines[0]), d))
    out = runs[0][0]
    assert out["steps"] == steps and out["warmup"] == warmup and out["ms_per_step"] > 0 and out["value"] > 0
    for leg in ("latency", "batched", "raw_queries", "hbm_only", "inprocess_multi", "configs", "cpu_baseline", "parity_full_size", "recall_at_100"):
        assert leg not in out, leg
    got = {}
    for name, dtype, shape in (("indices", np.float64, (Q, k)), ("scores", np.float32, (Q, k)), ("counts", np.float64, (Q,))):
        a, b = (np.load(os.path.join(d, name + ".npy")) for _, d in runs)
        assert a.dtype == dtype and a.shape == shape, (name, a.dtype, a.shape)
        np.testing.assert_array_equal(a, b)
        got[name] = a
    # the first query of the last timed step against the oracle over the same synthetic rows
    codes, corr = bench.synth_rows(1, 0, rows, (dim + 7) // 8)
    qq, qc = bench.synth_queries(2, (warmup + steps) * Q, dim, 4)
    q0 = (warmup + steps - 1) * Q
    s32 = O.score_all(codes, corr, dim, qq[q0], qc[q0], 4, 1, float(bbq_amd.centroid_dp(bench.synth_centroid(dim))))[2]
    oi, osc = O.heap_topk(s32, k)
    np.testing.assert_array_equal(got["indices"][0], oi.astype(np.float64))
    np.testing.assert_array_equal(got["scores"][0].view(np.uint32), osc.view(np.uint32))
