"""GPU: BinaryQuantizationFormat.quantizeQueriesOnDevice through the JavaScript host (N-API addon over libbbq) under node returns the
bytes of the host quantizer (native.quantizeQueries) for one batch of the README's 1000 x 128 case, under every similarity."""
import os
import shutil
import subprocess

import pytest

from bbqlib import ROOT


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_device_queries_match_the_host():
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "device_queries.js")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "0 failures" in r.stdout
