"""Y.cachesToJSON of the Node facade (crdt_amd/js): the batched cache objects deep-equal the `c`
Yjs 13.5.16 built for every document of tests/golden/cache.json and the object crdt.js's loop
builds through the facade's own getMap / getArray / toJSON (tests/js/docs_cache_check.js)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node not installed")


@pytest.mark.gpu
def test_napi_caches_to_json_on_gpu():
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "docs_cache_check.js")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "napi docs cache ok" in r.stdout
