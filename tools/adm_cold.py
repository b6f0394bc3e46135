#!/usr/bin/env python3
"""What the admission marks cost where they save nothing: the FIRST merge of a freshly generated batch (every log walked, every mark written) and the steady
merges of a PTX_FLAG_READMIT context (every log walked every time, the marks ignored), beside the steady merges of a context that keeps marks.  One build, one
process; run it once per build on the same box (--lib: another build of the library, e.g. the parent commit's, whose plain merges are the yardstick — it knows
no marks, so its three figures are a first merge and two times its steady merges).
    python tools/adm_cold.py [--lib PATH] [--docs 8192] [--repeats 5] [--iters 10]
Per repeat a NEW batch is generated (other device addresses, zeroed marks); a throw-away batch is merged first so that no figure holds the process's start-up.
Prints one JSON line: the per-repeat milliseconds (ptx_merge_timed: HIP events on the context's stream) and their medians."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from peritext_amd import abi, workloads  # noqa: E402
from peritext_amd.engine import Engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--config", default="config4")
    ap.add_argument("--docs", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    lib = args.lib and (args.lib if os.path.isabs(args.lib) else os.path.join(ROOT, args.lib))
    g = workloads.gen_config(args.config)
    first, steady, readmit = [], [], []
    with Engine(0, flags=abi.FLAG_NO_ELEM_RANK, lib_path=lib) as e, Engine(0, flags=abi.FLAG_NO_ELEM_RANK | abi.FLAG_READMIT, lib_path=lib) as f:
        kernel = None
        for rep in range(args.repeats + 1):
            db, _ = e.generate(g["replicas"], g["ops_per_log"], g["mix"], g["mark_types"], args.docs, 2024 + rep, list_cap=2048)
            dr, dr2 = e.alloc_result(db), f.alloc_result(db)
            t_first = e.merge_timed(db, dr, 1)
            t_steady = e.merge_timed(db, dr, args.iters) / args.iters
            t_readmit = f.merge_timed(db, dr2, args.iters) / args.iters
            assert int(e.download_logs(dr, e.n_logs(db))["status"].max()) == 0 and int(f.download_logs(dr2, e.n_logs(db))["status"].max()) == 0
            kernel = e.batch_kernel_name(db)
            f.free_result(dr2)
            e.free_result(dr)
            e.free_batch(db)
            if rep:  # (the first batch is the warm-up)
                first.append(t_first)
                steady.append(t_steady)
                readmit.append(t_readmit)
    r4 = lambda xs: [round(x, 4) for x in xs]  # noqa: E731
    print("ADM_COLD " + json.dumps({"build": os.path.basename(lib or "libperitext_hip.so"), "config": args.config, "docs": args.docs, "kernel": kernel, "iters": args.iters,
                                    "first_merge_ms": r4(first), "steady_ms": r4(steady), "readmit_steady_ms": r4(readmit),
                                    "median": {"first_merge_ms": round(statistics.median(first), 4), "steady_ms": round(statistics.median(steady), 4),
                                               "readmit_steady_ms": round(statistics.median(readmit), 4)}}), flush=True)


if __name__ == "__main__":
    main()
