#!/usr/bin/env python3
"""Measurements of ptx_check_patches (the fuzzer's patch assertion on the device, peritext_amd/csrc/accum_core.h) on the GPU -> profiles/accum_check.json.

    python tools/accum_profile.py [--out profiles/accum_check.json]

Every step runs in a child process of its own under `timeout` (a step that faults or hangs ends the run: nothing more is started on the GPU after a failure):
  config4   config #4 made by ptx_generate, 2 048 documents x 3 replicas x 4 096 ops, merged
  rich4k    the `rich` mix at 4 096 ops per log (documents that keep ~2 000 characters), 512 documents
Per step:
  replay_patches   ptx_replay_patches' kernel_ms and the call's wall time (records downloaded: what a host had to do before)
  check_patches    REPS calls of ptx_check_patches: the HIP-event time of its two kernels (replay, accumulate: ptx_check_patches_ms) and the call's wall time;
                   every log must agree with the merge
  host_way_scaled  the way of making the same check before this entry point existed — replay, download, wire.decode_patches and tests/helpers.py
                   accumulate_patches against the decoded spans — timed on the first 8 documents and SCALED to the step's documents (labelled as scaled)
No figure is asserted: the speed of this kernel had never been measured."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEPS = (("config4", 2048, 500), ("rich4k", 512, 500))
REPS = 3
HOST_DOCS = 8
SEED = 20260


def step(name, docs):
    import helpers as H
    from peritext_amd import wire, workloads
    from peritext_amd.engine import Engine

    g = workloads.gen_config(name)
    gen_args = (g["replicas"], g["ops_per_log"], g["mix"], g["mark_types"])
    out = {"docs": docs, "replicas": g["replicas"], "ops_per_log": g["ops_per_log"]}
    with Engine(0) as e:
        db, info = e.generate(*gen_args, docs, SEED)
        dr = e.alloc_result(db)
        try:
            e.merge(db, dr)
            e.sync()
            out["logs"], out["ops"] = e.n_logs(db), e.n_ops(db)
            t0 = time.perf_counter()
            pat = e.replay_patches(db, dr)
            out["replay_patches"] = {"kernel_ms": round(pat.kernel_ms, 3), "wall_ms": round(1e3 * (time.perf_counter() - t0), 3), "records": int(pat.logs["n_patches"].sum()),
                                     "record_bytes_downloaded": 16 * int(pat.logs["n_patches"].sum())}
            del pat
            runs = []
            for _ in range(REPS):
                t0 = time.perf_counter()
                rows, bad = e.check_patches(db, dr)
                wall = 1e3 * (time.perf_counter() - t0)
                rms, ams = e.check_patches_ms()
                assert bad == 0 and (rows["status"] == 0).all() and (rows["agrees"] == 1).all(), (bad, rows[:4])
                runs.append({"replay_kernel_ms": round(rms, 3), "accum_kernel_ms": round(ams, 3), "wall_ms": round(wall, 3)})
            out["check_patches"] = {"runs": runs, "median_accum_kernel_ms": statistics.median(r["accum_kernel_ms"] for r in runs),
                                    "median_wall_ms": statistics.median(r["wall_ms"] for r in runs), "bytes_device_to_host": 88 * out["logs"] + 8}
        finally:
            e.free_result(dr)
            e.free_batch(db)
        # the host's way, on the first HOST_DOCS documents
        hb, hinfo = e.generate(*gen_args, HOST_DOCS, SEED)
        hr = e.alloc_result(hb)
        try:
            e.merge(hb, hr)
            e.sync()
            actors, comments, log_doc = wire.generated_tables(HOST_DOCS, g["replicas"], hinfo["n_comments"])
            t0 = time.perf_counter()
            batch = e.download_batch(hb, wire.GEN_VALUES, wire.GEN_URLS, log_doc, actors, comments)
            res = e.download(hb, hr)
            pat = e.replay_patches(hb, hr)
            for log in range(batch.n_logs):
                got = H.accumulate_patches(wire.decode_patches(batch, pat, log, with_rows=True))
                assert H.norm_spans(got) == H.norm_spans(wire.decode_spans(batch, res, log)), log
            wall = 1e3 * (time.perf_counter() - t0)
            out["host_way_scaled"] = {"measured_docs": HOST_DOCS, "measured_wall_ms": round(wall, 1), "scaled_to_docs": docs, "scaled_wall_ms": round(wall * docs / HOST_DOCS, 1),
                                      "note": "SCALED linearly from %d documents, not measured at %d" % (HOST_DOCS, docs)}
        finally:
            e.free_result(hr)
            e.free_batch(hb)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accum_check.json"))
    ap.add_argument("--step")
    ap.add_argument("--docs", type=int, default=0)
    args = ap.parse_args()
    if args.step:
        print(json.dumps(step(args.step, args.docs)))
        return 0
    result = {"tool": "tools/accum_profile.py", "repeats": REPS}
    for name, docs, limit in STEPS:  # (the chain: a failed step ends it)
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, "--docs", str(docs)], cwd=ROOT, capture_output=True, text=True)
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
