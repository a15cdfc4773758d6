"""Y.writeMany of the Node facade (crdt_amd/js): the recorded Yjs op scripts of tests/golden/ops.json
run in lockstep through batched local ops reach the recorded states, the returned updates are what
takeLocalUpdate collects, and an observer on a written map fires once per call
(tests/js/docs_write_check.js)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node not installed")


@pytest.mark.gpu
def test_napi_write_many_on_gpu():
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "docs_write_check.js")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "napi docs write ok" in r.stdout
