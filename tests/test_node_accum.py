"""MergeEngine.accumulatePatches / checkPatches of the JS host on a real MI355X (peritext_amd/node -> N-API -> ptx_accumulate_patches / ptx_check_patches) on
tests/golden/patches_mini.json: the streams the replay returns, accumulated on the device, decode to spans deep-equal to the fixture's (made by the
reference); a stream with a record out of bounds fails its own log only; checkPatches agrees on every replica."""
import json
import os
import subprocess

import pytest

import helpers as H

ADDON = os.path.join(H.ROOT, "peritext_amd", "node", "peritext_node.node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not H.have_node(), reason="node not installed"),
              pytest.mark.skipif(not os.path.exists(ADDON), reason="N-API addon not built (run __graft_entry__.build())")]


def test_accumulate_and_check_patches_through_napi():
    p = subprocess.run([H.NODE, os.path.join(H.ROOT, "tests", "node_accum_check.js"), os.path.join(H.GOLDEN, "patches_mini.json")], cwd=H.ROOT, capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["ok"] and out["logs"] >= 6
