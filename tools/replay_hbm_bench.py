#!/usr/bin/env python3
"""Measurements of the HBM-state patch replay (ptx_replay_kernel_hbm) on the GPU -> profiles/replay_hbm_state.json.

    python tools/replay_hbm_bench.py [--out profiles/replay_hbm_state.json]

Every step runs in a child process of its own under `timeout` (a step that faults or hangs ends the run: nothing more is started on the GPU after a failure):
  scaling_typed      replay kernel_ms of an append-only typed document of 100 000 and of 200 000 elements
  scaling_scattered  the same for "scattered typing" logs (tests/replay_hbm_docs.scattered_typing_log) of 110 000 and 220 000 ops
                     -> T(2n) / T(n): linear work gives 2, a pass over the document per op gives 4; the structure is right below 3
  cost               one 60 000-element document (fits the LDS) through the LDS build and through the HBM-state kernel (PTX_FLAG_REPLAY_HBM_STATE), alternated in
                     one process, and the same at the router's boundary (78 000 elements: the largest round size whose state still fits 160 KB)
Every replay is checked: status 0 and one record per row (such logs carry no marks)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEPS = (("scaling_typed", 420), ("scaling_scattered", 420), ("cost", 420))
REPS = 5


def _replays(eng, batch, reps):
    """kernel_ms of `reps` replays of a one-log batch (merged once), each checked."""
    db = eng.upload(batch)
    dr = eng.alloc_result(db)
    try:
        eng.merge(db, dr)
        out = []
        for _ in range(reps):
            pat = eng.replay_patches(db, dr)
            rows = int(batch.log_off[1] - batch.log_off[0])
            assert int(pat.logs["status"][0]) == 0 and int(pat.logs["n_patches"][0]) == rows, (pat.logs, rows)
            out.append((pat.kernel_ms, pat.hbm_logs))
        return out
    finally:
        eng.free_result(dr)
        eng.free_batch(db)


def _scaling(make, sizes):
    from peritext_amd import wire
    from peritext_amd.engine import Engine

    res = {}
    with Engine(0) as eng:
        for n in sizes:
            batch = wire.encode_docs([[make(n)]])
            runs = _replays(eng, batch, REPS)
            assert all(h == 1 for _, h in runs), "beyond the LDS: the HBM-state kernel"
            res[str(n)] = {"rows": int(batch.log_off[1]), "elements": int(batch.log_hdr["n_ins"][0]), "kernel_ms": [round(ms, 3) for ms, _ in runs],
                           "median_ms": round(statistics.median(ms for ms, _ in runs), 3)}
    a, b = (res[str(n)]["median_ms"] for n in sizes)
    res["ratio_T2n_over_Tn"] = round(b / a, 3)
    assert b / a < 3.0, "T(2n) / T(n) = %.2f: a per-op pass over the document is left somewhere" % (b / a)
    return res


def step(name):
    import replay_hbm_docs as D
    from peritext_amd import abi, wire
    from peritext_amd.engine import Engine

    if name == "scaling_typed":
        return _scaling(D.typed_log, (100000, 200000))
    if name == "scaling_scattered":
        return _scaling(lambda n: D.scattered_typing_log(n, 7), (110000, 220000))
    if name == "cost":
        res = {}
        with Engine(0) as lds, Engine(0, flags=abi.FLAG_REPLAY_HBM_STATE) as hbm:
            for n in (60000, 78000):
                batch = wire.encode_docs([[D.typed_log(n)]])
                a, b = [], []
                for _ in range(REPS):  # alternated
                    (ms, h), = _replays(lds, batch, 1)
                    assert h == 0, "fits the LDS: the wide build"
                    a.append(ms)
                    (ms, h), = _replays(hbm, batch, 1)
                    assert h == 1
                    b.append(ms)
                res[str(n)] = {"lds_kernel_ms": [round(x, 3) for x in a], "hbm_kernel_ms": [round(x, 3) for x in b],
                               "ratio_hbm_over_lds": round(statistics.median(b) / statistics.median(a), 3)}
        return res
    raise SystemExit("unknown step " + name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_hbm_state.json"))
    ap.add_argument("--step")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(step(args.step)))
        return 0
    result = {"tool": "tools/replay_hbm_bench.py", "repeats": REPS}
    for name, limit in STEPS:  # (the chain: a failed step ends it)
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name], cwd=ROOT, capture_output=True, text=True)
        if p.returncode != 0:
            print("step %s failed (exit %d):\n%s\n%s" % (name, p.returncode, p.stdout[-2000:], p.stderr[-4000:]), file=sys.stderr)
            return 1
        result[name] = json.loads(p.stdout.strip().splitlines()[-1])
        print(name, json.dumps(result[name]), flush=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
