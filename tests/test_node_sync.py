"""MergeEngine.syncMany of the JS host on a real MI355X (peritext_amd/node: encode, upload, ptx_sync_replicas, download of `more`, decodeChanges) on the
documents of tests/golden/patches_mini.json, re-dealt: per pair the Changes deep-equal to what oracle/harness.js's getMissingChanges + applyChanges apply
(tests/sync_oracle.js), in admitted order."""
import json
import os
import random
import subprocess

import pytest

import helpers as H
import sync_cases as SC

ADDON = os.path.join(H.ROOT, "peritext_amd", "node", "peritext_node.node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not H.have_node(), reason="node not installed"),
              pytest.mark.skipif(not os.path.exists(ADDON), reason="N-API addon not built (run __graft_entry__.build())")]


def test_sync_many_on_redealt_documents(tmp_path):
    gen = H._load_golden("patches_mini.json")
    rng = random.Random(9)
    docs, pairs, flat = [], [], []
    for d in gen["docs"][:6]:
        logs = []
        while len(logs) < 3:
            logs += H.redeal_logs(d["logs"], rng, 3 - len(logs))
        k = len(docs)
        docs.append(logs)
        pairs += [{"doc": k, "from": 0, "to": 1}, {"doc": k, "from": 1, "to": 0}, {"doc": k, "from": 0, "to": 2}]
        flat += [(logs[0], logs[1]), (logs[1], logs[0]), (logs[0], logs[2])]
    oracle = SC.oracle_sync(flat)
    expected = []
    for (src, _), o in zip(flat, oracle):
        assert not o["threw"]
        keyed = SC.by_key(src)
        expected.append({"applied": [keyed[(a, q)] for a, q in o["applied"]], "status": 0})
    assert sum(len(e["applied"]) for e in expected) > 20
    inp = tmp_path / "in.json"
    inp.write_text(json.dumps({"docs": docs, "pairs": pairs, "expected": expected}))
    p = subprocess.run([H.NODE, os.path.join(H.ROOT, "tests", "node_sync_check.js"), str(inp)], cwd=H.ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["ok"] and out["pairs"] == len(pairs) and out["changes"] == sum(len(e["applied"]) for e in expected)
