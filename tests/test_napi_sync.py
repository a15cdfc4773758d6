"""Y.encodeStatesAsUpdates of the Node facade (crdt_amd/js): batched sync replies equal the per-pair
Y.encodeStateAsUpdate and Yjs's recorded replies (tests/js/sync_check.js)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node not installed")


@pytest.mark.gpu
def test_napi_batched_sync_replies_on_gpu():
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "sync_check.js")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "napi sync ok" in r.stdout
