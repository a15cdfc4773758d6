"""Y.readMany of the Node facade (crdt_amd/js): batched point reads deep-equal the per-type
getMap(name).get / .size and getArray(name).get / .length and Yjs's recorded values over a dozen small
fixture documents (tests/js/docs_read_check.js)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node not installed")


@pytest.mark.gpu
def test_napi_read_many_on_gpu():
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "docs_read_check.js")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "napi docs read ok" in r.stdout
