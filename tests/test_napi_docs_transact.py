"""Y.transactMany of the Node facade (crdt_amd/js): the recorded Yjs op scripts of tests/golden/ops.json,
their local ops cut into chunks of at most 8 and every round's chunks issued through one call, reach
the recorded states; a type set and pushed into in one call equals the facade's own calls; the returned
updates are what takeLocalUpdate collects, and an observer on a written map fires once per call
(tests/js/docs_transact_check.js)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node not installed")


@pytest.mark.gpu
def test_napi_transact_many_on_gpu():
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "docs_transact_check.js")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "napi docs transact ok" in r.stdout
