"""Y.rootsToJSON of the Node facade (crdt_amd/js): batched root toJSON deep-equals the per-type
getMap(name).toJSON() / getArray(name).toJSON() and Yjs's recorded values over the map and nested
fixtures (tests/js/docs_json_check.js)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node not installed")


@pytest.mark.gpu
def test_napi_roots_to_json_on_gpu():
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "docs_json_check.js")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "napi docs json ok" in r.stdout
