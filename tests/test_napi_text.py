"""Text content through the Node facade (crdt_amd/js): the hand-built ContentString cases of
tests/golden/text.json through Y.applyUpdate / Y.encodeStateAsUpdate / Y.mergeUpdates, strings split
inside a surrogate pair included (tests/js/text_check.js)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node not installed")


@pytest.mark.gpu
def test_napi_text_on_gpu():
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "text_check.js")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "napi text ok" in r.stdout
