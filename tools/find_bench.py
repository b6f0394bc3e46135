#!/usr/bin/env python3
"""Find in resident documents' text on the device against the only path the parent commit has — download the text, search it on the host — on one box, in one
run -> profiles/find_text.json.

    python tools/find_bench.py [--docs 16384] [--reps 5] [--out FILE] [--commit ID]

Workload: the batch of profiles/text_assembly.json — the `rich4k` mix (3 replicas x 4 096 ops per document), generated and merged on the device; the string table
is the generator's 128 one-unit strings.  Every side runs --reps times after one warm-up run; medians are reported, the runs are kept.
  device     Engine.find_text over the whole batch for a two-unit and a sixteen-unit pattern taken from the first log's own text: ptx_matches.kernel_ms (HIP
             events around every launch of the call: lengths, offset scan, assemble, count, hit scan, emit), the wall time of the call (its three waits, the
             download of the hits and the copy into numpy included), and the same for a count-only call (max_hits_per_log = 0).
  host       Engine.text (61 ms of it are the download of the text) + a numpy search of the downloaded buffer: candidates by the pattern's first two units over the
             whole buffer, verified unit by unit, attributed to logs by text_off and dropped where they cross a log's end.  One thread.
Both sides must agree on every log's count and on the hit units (checked).  A record, no threshold: tests/test_emu_find.py and tests/test_gpu_find.py are the
acceptance."""
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


def host_search(text, pat):
    """(count per log, hit units per log back to back) of a downloaded wire.Text: every position, overlapping ones included, none across a log's end."""
    t, m = text.text, len(pat)
    if len(t) < m:
        return np.zeros(len(text.status), np.int64), np.zeros(0, np.int64)
    ok = t[: len(t) - m + 1] == pat[0]
    for i in range(1, m):
        ok &= t[i : len(t) - m + 1 + i] == pat[i]
    p = np.flatnonzero(ok)
    log = np.searchsorted(text.text_off, p, side="right") - 1
    keep = p + m <= text.text_off[log + 1].astype(np.int64)
    p, log = p[keep], log[keep]
    return np.bincount(log, minlength=len(text.status)), p - text.text_off[log].astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--commit", help="the commit measured (default: git rev-parse of the tree the tool stands in)")
    args = ap.parse_args()
    import torch

    from peritext_amd import abi, wire
    from peritext_amd.engine import Engine
    from peritext_amd.workloads import gen_config

    if not torch.cuda.is_available():
        print("tools/find_bench.py measures on the GPU; none is visible", file=sys.stderr)
        return 1
    cfg = gen_config("rich4k")
    R, D = cfg["replicas"], args.docs
    L = R * D
    res = {"tool": "tools/find_bench.py", "config": "rich4k", "docs": D, "replicas": R, "ops_per_log": cfg["ops_per_log"], "logs": L, "reps": args.reps,
           "box": "%s, %s, torch %s" % (torch.cuda.get_device_name(0), platform.node() or "host", torch.__version__), "commit": args.commit or commit()}
    with Engine(0) as eng:
        db, info = eng.generate(R, cfg["ops_per_log"], cfg["mix"], cfg["mark_types"], D, 4)
        dr = eng.alloc_result(db)
        ds = eng.upload_strings(wire.GEN_VALUES)
        eng.merge(db, dr)
        eng.sync()
        text = eng.text(db, dr, ds)
        units = int(text.text_off[-1])
        assert not text.status.any() and units == int(eng.download_logs(dr, L)["n_visible"].sum()), "one unit per element: the traffic figures below count elements as units"
        res["text_units"], res["text_bytes"] = units, 2 * units
        first = text.text[int(text.text_off[0]) : int(text.text_off[1])]
        # the parent's only path: the text comes down, the host searches it
        tks = []
        tw, tw_runs = timed(lambda: tks.append(eng.text(db, dr, ds).kernel_ms), args.reps)
        text_k = statistics.median(tks[1:])  # the text passes alone, in this run: what a find call's kernel_ms holds beyond them is the search
        res["host"] = {"engine_text_call_wall_ms": round(tw, 3), "engine_text_call_wall_ms_runs": tw_runs, "text_passes_kernel_ms": round(text_k, 3)}
        for name, m in (("pattern_2_units", 2), ("pattern_16_units", 16)):
            pat = np.ascontiguousarray(first[10 : 10 + m]).astype(np.uint16)
            needle = pat.astype("<u2").tobytes().decode("utf-16-le", "surrogatepass")
            kms = []

            def dev(cap=0xFFFFFFFF):
                r = eng.find_text(db, dr, ds, needle, max_hits_per_log=cap)
                kms.append(r.kernel_ms)
                return r

            wall, wall_runs = timed(dev, args.reps)
            k_all = kms[1 : 1 + args.reps]
            del kms[:]
            cwall, cwall_runs = timed(lambda: dev(0), args.reps)
            k_cnt = kms[1 : 1 + args.reps]
            got = dev()
            sw, sw_runs = timed(lambda: host_search(text, pat), args.reps)
            counts, hit_units = host_search(text, pat)
            assert np.array_equal(counts, got.n_matches.astype(np.int64)) and np.array_equal(hit_units, got.hit_unit.astype(np.int64)), "device and host disagree"
            nh = int(got.hit_off[-1])
            # what the search passes move by their algorithm.  count: every log's text once + a halo of m - 1 units per step.  emit, only in logs with a listed hit:
            # the text again up to the step of the last listed hit, the value ids and two table offsets per element of the tiles up to the one that holds its last
            # unit, three words per hit written and hit_unit read back by both cursors
            S, T = abi.FIND_STEP, abi.TEXT_TILE
            lens = np.diff(text.text_off).astype(np.int64)
            steps = np.where(lens >= m, (lens - m + 1 + S - 1) // S, 0)
            count_bytes = int(2 * lens[lens >= m].sum() + 2 * (m - 1) * steps.sum())
            has = np.flatnonzero(np.diff(got.hit_off) > 0)
            last = got.hit_off[has + 1].astype(np.int64) - 1
            walked = np.minimum(lens[has], (got.hit_unit[last].astype(np.int64) // S + 1) * S + m - 1)
            tiles = (got.hit_end[last].astype(np.int64) - 1) // T + 1
            emit_bytes = int(2 * walked.sum() + 2 * (m - 1) * ((walked + S - 1) // S).sum() + np.minimum(lens[has], tiles * T).sum() * (4 + 16) + nh * 4 * 5)
            moved = count_bytes + emit_bytes
            search_ms = statistics.median(k_all) - text_k
            res[name] = {"needle": needle, "matches": int(got.n_matches.sum()), "logs_with_a_match": int((got.n_matches > 0).sum()), "listed_hits": nh,
                         "device": {"kernel_ms": round(statistics.median(k_all), 3), "kernel_ms_runs": [round(x, 3) for x in k_all], "call_wall_ms": round(wall, 3), "call_wall_ms_runs": wall_runs,
                                    "count_only_kernel_ms": round(statistics.median(k_cnt), 3), "count_only_call_wall_ms": round(cwall, 3), "count_only_call_wall_ms_runs": cwall_runs,
                                    "hit_bytes_downloaded": 12 * nh, "search_passes_kernel_ms": round(search_ms, 3), "count_pass_bytes": count_bytes, "emit_pass_bytes": emit_bytes,
                                    "search_passes_gbps": round(moved / (search_ms * 1e-3) / 1e9, 1),
                                    "count_pass_gbps": round(count_bytes / ((statistics.median(k_cnt) - text_k) * 1e-3) / 1e9, 1)},
                         "host": {"numpy_search_ms": round(sw, 3), "numpy_search_ms_runs": sw_runs, "text_download_plus_search_ms": round(tw + sw, 3)},
                         "device_path_is_faster": wall < tw + sw, "count_only_is_faster": cwall < tw + sw}
        eng.free_strings(ds)
        eng.free_result(dr)
        eng.free_batch(db)
    out_path = args.out or os.path.join(ROOT, "profiles", "find_text.json")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
