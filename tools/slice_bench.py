#!/usr/bin/env python3
"""Text of element ranges of resident documents cut on the device against the only path the parent commit has — download the text, slice it on the host — on one
box, in one run -> profiles/text_slices.json.

    python tools/slice_bench.py [--docs 16384] [--reps 5] [--context 16] [--out FILE] [--commit ID]

Workload: the batch of profiles/text_assembly.json and profiles/find_text.json — the `rich4k` mix (3 replicas x 4 096 ops per document), generated and merged on
the device; the string table is the generator's 128 one-unit strings.  Every side runs --reps times after one warm-up run; medians are reported, the runs are kept.
  snippets   (a) the listed hits of find_bench's two-unit pattern, each widened by --context elements on both sides (the subtraction saturated at 0, nothing
             else clamped by the caller): Engine.text_slices_flat — ptx_slices.kernel_ms (HIP events around every launch of the call: lengths, offset scan, plan,
             its scan, assemble, prefix, bounds, output scan, copy, span emit), the wall time of the call (the upload of the ranges, its three waits, the download
             and the copy into numpy included) and the bytes that come down.
  whole      (b) one slice per log that covers the whole log: the worst case for the copy pass, which then moves every unit the assemble pass has just written.
             The result must be Engine.text's buffer byte for byte (asserted).  kernel_ms beyond the text passes' own is what plan, prefix, bounds, scans, copy
             and span emit cost together; the API has no finer clock.
  host       (c) the parent's path in the same run: Engine.text (the download of the whole text) + numpy slicing of the downloaded buffer into the same snippets
             (one fancy-indexing gather; one unit per element in this batch, so element indexes are unit offsets).  One thread.
Both sides must agree on every snippet (checked).  A record, no threshold: tests/test_emu_slices.py and tests/test_gpu_slices.py are the acceptance."""
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


def commit():
    try:
        return subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def timed(fn, reps):
    """(median ms, [ms per run]) of `reps` runs after one warm-up."""
    fn()
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        runs.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(runs), [round(x, 3) for x in runs]


def spread(runs):
    return round(max(runs) - min(runs), 3)


def host_slices(text, slice_off, start, end):
    """The snippets cut from a downloaded wire.Text, back to back: (unit_off, units).  One unit per element."""
    log = np.repeat(np.arange(len(slice_off) - 1), np.diff(slice_off).astype(np.int64))
    nv = np.diff(text.text_off).astype(np.int64)[log]
    a, b = np.minimum(start.astype(np.int64), nv), np.minimum(end.astype(np.int64), nv)
    b = np.maximum(a, b)
    lens = b - a
    off = np.concatenate([[0], np.cumsum(lens)])
    src = text.text_off[log].astype(np.int64) + a
    idx = np.repeat(src - off[:-1], lens) + np.arange(int(off[-1]))
    return off, text.text[idx]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--context", type=int, default=16)
    ap.add_argument("--out")
    ap.add_argument("--commit", help="the commit measured (default: git rev-parse of the tree the tool stands in)")
    args = ap.parse_args()
    import torch

    from peritext_amd import wire
    from peritext_amd.engine import Engine
    from peritext_amd.workloads import gen_config

    if not torch.cuda.is_available():
        print("tools/slice_bench.py measures on the GPU; none is visible", file=sys.stderr)
        return 1
    cfg = gen_config("rich4k")
    R, D = cfg["replicas"], args.docs
    L = R * D
    res = {"tool": "tools/slice_bench.py", "config": "rich4k", "docs": D, "replicas": R, "ops_per_log": cfg["ops_per_log"], "logs": L, "reps": args.reps, "context": args.context,
           "box": "%s, %s, torch %s" % (torch.cuda.get_device_name(0), platform.node() or "host", torch.__version__), "commit": args.commit or commit()}
    with Engine(0) as eng:
        db, info = eng.generate(R, cfg["ops_per_log"], cfg["mix"], cfg["mark_types"], D, 4)
        dr = eng.alloc_result(db)
        ds = eng.upload_strings(wire.GEN_VALUES)
        eng.merge(db, dr)
        eng.sync()
        text = eng.text(db, dr, ds)
        units = int(text.text_off[-1])
        assert not text.status.any() and units == int(eng.download_logs(dr, L)["n_visible"].sum()), "one unit per element"
        res["text_units"], res["text_bytes"] = units, 2 * units
        first = text.text[int(text.text_off[0]) : int(text.text_off[1])]
        needle = np.ascontiguousarray(first[10:12]).astype("<u2").tobytes().decode("utf-16-le", "surrogatepass")
        hits = eng.find_text(db, dr, ds, needle)
        # (c) the parent's only path: the text comes down, the host slices it
        tks = []
        tw, tw_runs = timed(lambda: tks.append(eng.text(db, dr, ds).kernel_ms), args.reps)
        text_k = statistics.median(tks[1:])
        # (a) the listed hits, widened
        c = args.context
        s_off = hits.hit_off.astype(np.uint64)
        s_start = np.where(hits.hit_start >= c, hits.hit_start - c, 0).astype(np.uint32)
        s_end = (hits.hit_end.astype(np.uint64) + c).clip(max=0xFFFFFFFF).astype(np.uint32)
        kms = []

        def dev(off, start, end):
            r = eng.text_slices_flat(db, dr, ds, off, start, end)
            kms.append(r.kernel_ms)
            return r

        wall, wall_runs = timed(lambda: dev(s_off, s_start, s_end), args.reps)
        k_a = kms[1 : 1 + args.reps]
        got = dev(s_off, s_start, s_end)
        hs, hs_runs = timed(lambda: host_slices(text, s_off, s_start, s_end), args.reps)
        h_off, h_units = host_slices(text, s_off, s_start, s_end)
        assert np.array_equal(h_off, got.unit_off.astype(np.int64)) and np.array_equal(h_units, got.text), "device and host disagree on the snippets"
        ns, nu, nr = len(got.elem_start), int(got.unit_off[-1]), int(got.sspan_off[-1])
        down = 4 * L + 8 * ns + 16 * (ns + 1) + 2 * nu + 12 * nr
        res["snippets"] = {"needle": needle, "slices": ns, "units": nu, "span_rows": nr, "mean_units_per_slice": round(nu / max(ns, 1), 2),
                           "device": {"kernel_ms": round(statistics.median(k_a), 3), "kernel_ms_runs": [round(x, 3) for x in k_a], "kernel_ms_spread": spread(k_a),
                                      "kernel_ms_beyond_text_passes": round(statistics.median(k_a) - text_k, 3), "call_wall_ms": round(wall, 3), "call_wall_ms_runs": wall_runs,
                                      "call_wall_ms_spread": spread(wall_runs), "bytes_uploaded": 8 * (L + 1) + 8 * ns, "bytes_downloaded": down},
                           "host": {"engine_text_call_wall_ms": round(tw, 3), "engine_text_call_wall_ms_runs": tw_runs, "bytes_downloaded": 2 * units + 16 * (L + 1) + 4 * L,
                                    "numpy_slicing_ms": round(hs, 3), "numpy_slicing_ms_runs": hs_runs, "text_download_plus_slicing_ms": round(tw + hs, 3)},
                           "device_path_is_faster": wall < tw + hs}
        # (b) one slice per log, the whole log: the copy pass moves all of the text once more
        w_off = np.arange(L + 1, dtype=np.uint64)
        w_start, w_end = np.zeros(L, np.uint32), np.full(L, 0xFFFFFFFF, np.uint32)
        del kms[:]
        wwall, wwall_runs = timed(lambda: dev(w_off, w_start, w_end), args.reps)
        k_b = kms[1 : 1 + args.reps]
        whole = dev(w_off, w_start, w_end)
        assert whole.text.tobytes() == text.text.tobytes() and np.array_equal(whole.unit_off, text.text_off), "one slice per log returns Engine.text's buffer byte for byte"
        same_spans = bool(np.array_equal(whole.sspan_off, text.span_off) and np.array_equal(whole.sspan_unit, text.span_unit))  # (equal unless a log has spans and no element)
        beyond = statistics.median(k_b) - text_k
        res["whole_logs"] = {"slices": L, "units": units, "span_rows": int(whole.sspan_off[-1]), "span_offsets_equal_engine_text": same_spans,
                             "device": {"kernel_ms": round(statistics.median(k_b), 3), "kernel_ms_runs": [round(x, 3) for x in k_b], "kernel_ms_spread": spread(k_b),
                                        "text_passes_kernel_ms": round(text_k, 3), "kernel_ms_beyond_text_passes": round(beyond, 3),
                                        "copy_bytes_read_plus_written": 4 * units, "beyond_text_passes_gbps_of_the_copy_alone": round(4 * units / (beyond * 1e-3) / 1e9, 1),
                                        "prefix_block_bytes": 4 * (units + L), "call_wall_ms": round(wwall, 3), "call_wall_ms_runs": wwall_runs},
                             "host": {"engine_text_call_wall_ms": round(tw, 3)}, "device_path_is_faster": wwall < tw}
        eng.free_strings(ds)
        eng.free_result(dr)
        eng.free_batch(db)
    out_path = args.out or os.path.join(ROOT, "profiles", "text_slices.json")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
