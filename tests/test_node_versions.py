"""MergeEngine.documentsAt of the JS host on a real MI355X (peritext_amd/node: encode, upload, ptx_batch_at_versions, merge, ptx_replay_patches_from, decode)
on the documents of tests/golden/patches_mini.json, re-dealt: every replica at the clock of another replica of its document and at prefixes of its own log,
with and without `diff`, plus a clock no replica could have had — status, effective clock, spans and patches against tests/version_oracle.js."""
import json
import os
import random
import subprocess

import pytest

import helpers as H
import version_cases as VC

ADDON = os.path.join(H.ROOT, "peritext_amd", "node", "peritext_node.node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not H.have_node(), reason="node not installed"),
              pytest.mark.skipif(not os.path.exists(ADDON), reason="N-API addon not built (run __graft_entry__.build())")]


def expected_of(logs, cuts):
    at, rest = VC.oracle_versions(logs, cuts, False), VC.oracle_versions(logs, cuts, True)
    out = []
    for a, r in zip(at, rest):
        if a["error"] is not None:
            assert a["error"]["kind"] == "Missing dependency"
            out.append({"status": 3})
        else:
            assert r["error"] is None
            out.append({"status": 0, "clock": a["clock"], "spans": a["atVersion"]["spans"] if a["atVersion"] else None, "patches": r["restPatches"]})
    return out


def test_documents_at_on_redealt_documents(tmp_path):
    gen = H._load_golden("patches_mini.json")
    rng = random.Random(9)
    docs, flat, clock_cuts, prefix_cuts = [], [], [], []
    for d in gen["docs"][:4]:
        logs = []
        while len(logs) < 3:
            logs += H.redeal_logs(d["logs"], rng, 3 - len(logs))
        k = len(docs)
        docs.append(logs)
        for s, t in ((0, 1), (1, 2), (2, 0)):
            clock_cuts.append({"doc": k, "replica": s, "clock": VC.clock_of(logs[t])})
        prefix_cuts += [{"doc": k, "replica": 0, "changes": n} for n in (0, 1, len(logs[0]) // 2, len(logs[0]) + 5)]
        flat += logs
    # a clock no replica could have had: the last change of replica 0 of the first document that waits for another actor, without that actor
    victim = next(c for c in reversed(docs[0][0]) if any(a != c["actor"] and q for a, q in c["deps"].items()))
    open_clock = dict(VC.clock_of(docs[0][0]))
    open_clock[next(a for a, q in victim["deps"].items() if a != victim["actor"] and q)] = 0
    clock_cuts.append({"doc": 0, "replica": 0, "clock": open_clock})
    first = [0]
    for logs in docs:
        first.append(first[-1] + len(logs))
    as_oracle = lambda cuts: [dict({"log": first[c["doc"]] + c["replica"]}, **{k: v for k, v in c.items() if k in ("clock", "changes")}) for c in cuts]  # noqa: E731
    expected = {"clock": expected_of(flat, as_oracle(clock_cuts)), "prefix": expected_of(flat, as_oracle(prefix_cuts))}
    assert expected["clock"][-1] == {"status": 3} and all(e["status"] == 0 for e in expected["clock"][:-1] + expected["prefix"])
    assert sum(len(e["patches"]) for e in expected["prefix"]) > 20
    inp = tmp_path / "in.json"
    inp.write_text(json.dumps({"docs": docs, "clockCuts": clock_cuts, "prefixCuts": prefix_cuts, "expected": expected}))
    p = subprocess.run([H.NODE, os.path.join(H.ROOT, "tests", "node_versions_check.js"), str(inp)], cwd=H.ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["ok"] and out["failed"] == 1 and out["checked"] == 2 * (len(clock_cuts) - 1 + len(prefix_cuts)) and out["patches"] > 20
