#!/usr/bin/env python3
"""Replace all APPLIED: the plan made into Changes through the host (the ops come down and go up again) against the plan left on the device, on one box, in one
run -> profiles/replace_apply.json.

    python tools/replace_apply_bench.py [--docs 16384] [--reps 5] [--out FILE] [--commit ID]

Workload: that of tools/replace_bench.py — the `rich4k` mix (3 replicas x 4 096 ops per document), generated and merged on the device, one resident view of every
log, the two-unit pattern of that tool replaced by three elements.  Both legs run --reps times after one warm-up round, alternating; medians and ranges are
reported, the runs are kept.
  A  host_ops      TextView.replace_plan (the ops come down through a pinned block and are copied into numpy) + Engine.change (ptx_change: walks every op and every
                   offset on the host, downloads every ptx_log_hdr and log_off of the base batch, uploads the ops again, sums the made rows on the host).
  B  resident_ops  TextView.replace_plan_device (status and the three count arrays come down; the ops stay) + Engine.change_device (ptx_change_device: two passes
                   on the device for all of the above, ptx_change_kernel and ptx_take_rows_kernel unchanged).
Per leg: the wall time of the two calls together and of each half, the made batch freed outside the timed region; kernel_ms is the plan half's (HIP events around
its launches, the same passes in both legs) — neither ptx_change nor ptx_change_device times its kernels.
  agreement  the two made batches of the last round are downloaded and compared column for column, status included (asserted).
A record, no threshold: tests/test_gpu_change_device.py and tests/test_gpu_replace_device.py are the acceptance.  The tool reads nothing outside the repository."""
import argparse
import json
import os
import platform
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLUMNS = ("log_off", "op_id", "ref_a", "ref_b", "payload", "action", "mark_type", "side_a", "side_b", "chg_off", "chg_hdr", "chg_env", "log_hdr")


def commit():
    try:
        return subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def stats(xs):
    return {"median": round(statistics.median(xs), 3), "range": [round(min(xs), 3), round(max(xs), 3)], "runs": [round(x, 3) for x in xs]}


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
        print("tools/replace_apply_bench.py measures on the GPU; none is visible", file=sys.stderr)
        return 1
    cfg = gen_config("rich4k")
    R, D = cfg["replicas"], args.docs
    L = R * D
    res = {"tool": "tools/replace_apply_bench.py", "config": "rich4k", "docs": D, "replicas": R, "ops_per_log": cfg["ops_per_log"], "logs": L, "reps": args.reps,
           "box": "%s, %s, torch %s" % (torch.cuda.get_device_name(0), platform.node() or "host", torch.__version__), "commit": args.commit or commit()}
    replacement = ["<", "r", ">"]
    ids = [wire.GEN_VALUES.index(v) for v in replacement]
    actor = (np.arange(L, dtype=np.uint32) % R).astype(np.uint32)  # replica r of a generated document is actor rank r
    with Engine(0) as eng:
        db, _ = eng.generate(R, cfg["ops_per_log"], cfg["mix"], cfg["mark_types"], D, 4)
        dr = eng.alloc_result(db)
        ds = eng.upload_strings(wire.GEN_VALUES)
        eng.merge(db, dr)
        eng.sync()
        text = eng.text(db, dr, ds, 0, 1)
        first = text.text[int(text.text_off[0]) : int(text.text_off[1])]
        needle = np.ascontiguousarray(first[10:12]).astype("<u2").tobytes().decode("utf-16-le", "surrogatepass")
        view = eng.text_view(db, dr, ds)
        eng.free_strings(ds)
        na = int(eng.lib.ptx_batch_max_actors(db)) or R
        keep = {}

        def leg_a():
            t0 = time.perf_counter()
            plan = view.replace_plan(needle, ids, L)
            plan.ops.actor, plan.ops.max_actors = actor, na
            t1 = time.perf_counter()
            made, status = eng.change(db, dr, plan.ops)
            t2 = time.perf_counter()
            return plan, made, status, (t1 - t0) * 1e3, (t2 - t1) * 1e3

        def leg_b():
            t0 = time.perf_counter()
            plan, h = view.replace_plan_device(needle, ids, L, actor, na)
            t1 = time.perf_counter()
            made, status = eng.change_device(db, dr, h)
            t2 = time.perf_counter()
            eng.free_input_ops(h)
            return plan, made, status, (t1 - t0) * 1e3, (t2 - t1) * 1e3

        legs = {"host_ops": leg_a, "resident_ops": leg_b}
        runs = {k: {"wall": [], "plan": [], "change": [], "kernel": []} for k in legs}
        for rep in range(args.reps + 1):
            for k, fn in legs.items():
                plan, made, status, t_plan, t_change = fn()
                if rep:
                    r = runs[k]
                    r["wall"].append(t_plan + t_change), r["plan"].append(t_plan), r["change"].append(t_change), r["kernel"].append(plan.kernel_ms)
                if rep == args.reps:
                    keep[k] = (plan, eng.download_batch(made), status.copy())
                eng.free_batch(made)
        (pa, ma, sa), (pb, mb, sb) = keep["host_ops"], keep["resident_ops"]
        assert np.array_equal(sa, sb) and (ma.n_logs, ma.n_ops, ma.max_actors) == (mb.n_logs, mb.n_ops, mb.max_actors), "the two legs disagree on the status or the sizes"
        for f in COLUMNS:
            assert getattr(ma, f).tobytes() == getattr(mb, f).tobytes(), "the two legs disagree on " + f
        assert (ma.chg_env_hi is None) == (mb.chg_env_hi is None)
        for f in ("status", "n_matches", "n_chosen", "n_replaced"):
            assert np.array_equal(getattr(pa, f), getattr(pb, f)), f
        out = {"needle": needle, "replacement_elements": len(ids), "matches": int(pa.n_matches.sum()), "replaced": int(pa.n_replaced.sum()), "changes": int(pa.ops.chg_off[-1]),
               "input_ops": int(pa.ops.op_off[-1]), "rows_made": int(ma.n_ops), "logs_not_ok": int((sa != 0).sum()), "the_made_batches_agree_column_for_column": True}
        for k in legs:
            r = runs[k]
            out[k] = {"wall_ms": stats(r["wall"]), "plan_call_wall_ms": stats(r["plan"]), "change_call_wall_ms": stats(r["change"]), "plan_kernel_ms": stats(r["kernel"]),
                      "change_kernel_ms": None}
        out["resident_slowest_wall_ms_is_under_host_fastest"] = max(runs["resident_ops"]["wall"]) < min(runs["host_ops"]["wall"])
        res["replace_apply"] = out
        view.free()
        eng.free_result(dr)
        eng.free_batch(db)
    out_path = args.out or os.path.join(ROOT, "profiles", "replace_apply.json")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
