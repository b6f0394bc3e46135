#!/usr/bin/env python3
"""Replace all planned on the device against the host path it replaces, on one box, in one run -> profiles/replace_plan.json.

    python tools/replace_bench.py [--docs 16384] [--reps 5] [--out FILE] [--commit ID]

Workload: the view of profiles/text_view.json — the `rich4k` mix (3 replicas x 4 096 ops per document), generated and merged on the device, one resident view of
every log; the string table is the generator's 128 one-unit strings.  The pattern is the two-unit pattern of tools/view_bench.py, the replacement three elements.
Both sides run --reps times after one warm-up run, alternating; medians and ranges are reported, the runs are kept.
  plan   TextView.replace_plan: ptx_replace_plan.kernel_ms (HIP events around count, scan, positions, locate, select, the two scans, emit) and the wall time of
         the call, the copies into numpy included.
  host   what a caller does without it: TextView.find_text with every hit listed; per log a Python loop for the leftmost non-overlapping hits; the boundary test
         in numpy — every string of this table is one unit, so pre[e] == e and the test is hit_start == hit_unit and hit_end == hit_unit + m; a table with longer
         strings would need the value ids of every log downloaded first, which is NOT timed here —; the InputOperation dicts in descending order and
         wire.encode_input_ops.  kernel_ms is the find's; the wall time is the whole path's.
  agreement  Change for Change and op for op: chg_off, op_off, action, index, count and the value ids every insert points at must be equal (asserted).
A record, no threshold: tests/test_emu_replace.py and tests/test_gpu_replace.py are the acceptance."""
import argparse
import json
import os
import platform
import statistics
import subprocess
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def commit():
    try:
        return subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def side_by_side(fns, reps):
    """{name: [(wall ms, kernel ms)] per run} of `reps` rounds after one warm-up round; the sides alternate within a round.  fns: {name: callable -> kernel_ms}."""
    runs = {k: [] for k in fns}
    for rep in range(reps + 1):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            km = fn()
            if rep:
                runs[k].append(((time.perf_counter() - t0) * 1e3, km))
    return runs


def summary(runs):
    wall, km = [w for w, _ in runs], [k for _, k in runs]
    return {"call_wall_ms": round(statistics.median(wall), 3), "call_wall_ms_range": [round(min(wall), 3), round(max(wall), 3)], "call_wall_ms_runs": [round(x, 3) for x in wall],
            "kernel_ms": round(statistics.median(km), 3), "kernel_ms_range": [round(min(km), 3), round(max(km), 3)], "kernel_ms_runs": [round(x, 3) for x in km]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--commit", help="the commit measured (default: git rev-parse of the tree the tool stands in)")
    args = ap.parse_args()
    import torch

    from peritext_amd import wire
    from peritext_amd.engine import Engine
    from peritext_amd.workloads import gen_config

    if not torch.cuda.is_available():
        print("tools/replace_bench.py measures on the GPU; none is visible", file=sys.stderr)
        return 1
    cfg = gen_config("rich4k")
    R, D = cfg["replicas"], args.docs
    L = R * D
    res = {"tool": "tools/replace_bench.py", "config": "rich4k", "docs": D, "replicas": R, "ops_per_log": cfg["ops_per_log"], "logs": L, "reps": args.reps,
           "box": "%s, %s, torch %s" % (torch.cuda.get_device_name(0), platform.node() or "host", torch.__version__), "commit": args.commit or commit()}
    assert all(len(v) == 1 for v in wire.GEN_VALUES), "the host side's boundary test assumes one unit per element"
    replacement = ["<", "r", ">"]
    ids = [wire.GEN_VALUES.index(v) for v in replacement]
    # what wire.encode_input_ops reads of a batch: the tables and who is who (the ops themselves stay on the device)
    names = ["r%d" % i for i in range(R)]
    stub = types.SimpleNamespace(values=list(wire.GEN_VALUES), urls=[], keys=["text"], map_values=[], log_doc=[l // R for l in range(L)], doc_actors=[names] * D,
                                 doc_comments=[[]] * D, max_actors=R)
    actors = [names[l % R] for l in range(L)]
    with Engine(0) as eng:
        db, _ = eng.generate(R, cfg["ops_per_log"], cfg["mix"], cfg["mark_types"], D, 4)
        dr = eng.alloc_result(db)
        ds = eng.upload_strings(wire.GEN_VALUES)
        eng.merge(db, dr)
        eng.sync()
        text = eng.text(db, dr, ds, 0, 1)
        first = text.text[int(text.text_off[0]) : int(text.text_off[1])]
        needle = np.ascontiguousarray(first[10:12]).astype("<u2").tobytes().decode("utf-16-le", "surrogatepass")
        m = len(needle)
        view = eng.text_view(db, dr, ds)
        eng.free_strings(ds)
        keep = {}

        def plan():
            keep["plan"] = view.replace_plan(needle, ids, L)
            return keep["plan"].kernel_ms

        def host():
            hits = view.find_text(needle)
            off, hu, hs, he = hits.hit_off.astype(np.int64), hits.hit_unit, hits.hit_start, hits.hit_end
            whole = (hs == hu) & (he.astype(np.int64) == hu.astype(np.int64) + m)
            per_log = []
            for l in range(L):
                a, b = int(off[l]), int(off[l + 1])
                ops, limit, chosen = [], 0, []
                for k in range(a, b):
                    u = int(hu[k])
                    if u >= limit:
                        limit = u + m
                        if whole[k]:
                            chosen.append(k)
                for k in reversed(chosen):
                    s = int(hs[k])
                    ops.append({"path": ["text"], "action": "delete", "index": s, "count": int(he[k]) - s})
                    ops.append({"path": ["text"], "action": "insert", "index": s, "values": replacement})
                per_log.append([ops] if ops else [])
            keep["host"] = wire.encode_input_ops(stub, per_log, actors)
            keep["hits"] = hits
            return hits.kernel_ms

        runs = side_by_side({"plan": plan, "host": host}, args.reps)
        p, h, hits = keep["plan"], keep["host"], keep["hits"]
        for f in ("chg_off", "op_off", "action", "index", "count"):
            assert getattr(p.ops, f).tobytes() == getattr(h, f).tobytes(), "the two paths disagree on " + f
        ins = p.ops.action == 0
        assert ins.any() and all(np.array_equal(p.ops.values[p.ops.payload[ins] + i], h.values[h.payload[ins] + i]) for i in range(len(ids))), "the inserts' value ids"
        assert np.array_equal(p.n_matches, hits.n_matches) and not p.status.any()
        a, b = summary(runs["plan"]), summary(runs["host"])
        res["replace_plan"] = {"needle": needle, "replacement_elements": len(ids), "matches": int(p.n_matches.sum()), "chosen": int(p.n_chosen.sum()), "replaced": int(p.n_replaced.sum()),
                               "changes": int(p.ops.chg_off[-1]), "input_ops": int(p.ops.op_off[-1]), "plan": a, "host_find_greedy_encode": b,
                               "every_change_and_op_agree": True, "plan_kernel_ms_minus_find_kernel_ms": round(a["kernel_ms"] - b["kernel_ms"], 3),
                               "plan_call_wall_ms_is_lower": a["call_wall_ms"] < b["call_wall_ms"]}
        view.free()
        eng.free_result(dr)
        eng.free_batch(db)
    out_path = args.out or os.path.join(ROOT, "profiles", "replace_plan.json")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
