"""The doc-less update store of the Node facade (crdt_amd/js): Y.encodeStateVectorFromUpdate,
Y.encodeStateVectorsFromUpdates and Y.mergeUpdatesGroups against the bytes Yjs recorded in
tests/golden/merge.json and tests/golden/update_store.json (tests/js/update_store_check.js)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node not installed")


@pytest.mark.gpu
def test_napi_update_store_on_gpu():
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "update_store_check.js")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "napi update store ok" in r.stdout
