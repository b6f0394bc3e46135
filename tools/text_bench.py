#!/usr/bin/env python3
"""Document text assembled on the device against the host joins it replaces, on one box -> profiles/text_assembly.json.

    python tools/text_bench.py [--docs 16384] [--reps 5] [--py-logs 128] [--js-logs 8192] [--out FILE] [--commit ID]

Workload: the `rich4k` mix (3 replicas x 4 096 ops per document at 55 % inserts: documents that keep ~1 900 characters), generated and merged on the device;
the string table is the generator's 128 one-unit strings.  Every side runs --reps times after one warm-up run; medians are reported, the runs are kept.
  device       Engine.text over the whole batch: ptx_text.kernel_ms (HIP events around the length + offset-scan and the assemble launches) and the wall time
               of the call, download into pinned memory and the copy into numpy included.  `assemble_gbps` = the bytes the two passes move by their
               algorithm (value ids twice, the two table offsets per element twice, the units read and written, span rows and span_unit) over kernel_ms; the
               128-entry table stays in cache, so this is no HBM figure; `compulsory_gbps` counts only what no cache can serve (the ids once per pass, the text written,
               the span rows and span_unit).
  host_python  wire.decode_spans — the parent's path: one string-table lookup and one concatenation per visible element — over the first --py-logs logs of
               the SAME downloaded result, against wire.decode_spans_text over the same logs (one slice per span); scaled to the batch by visible elements.
  host_js      peritext_amd/node decodeSpans against decodeSpansText over the first --js-logs logs of the same result (tools/text_bench_decode.js, one node
               thread), scaled likewise.
The device path is compared with the host join, never with itself; both must return the same spans (checked on the Python sample, and in node on its own).
A record, no threshold: tests/test_emu_text.py and tests/test_gpu_text.py are the acceptance."""
import argparse
import json
import os
import platform
import shutil
import statistics
import subprocess
import sys
import tempfile
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--py-logs", type=int, default=128)
    ap.add_argument("--js-logs", type=int, default=8192)
    ap.add_argument("--out")
    ap.add_argument("--commit", help="the commit measured (default: git rev-parse of the tree the tool stands in)")
    args = ap.parse_args()
    import torch

    from peritext_amd import wire
    from peritext_amd.engine import Engine
    from peritext_amd.workloads import gen_config

    if not torch.cuda.is_available():
        print("tools/text_bench.py measures on the GPU; none is visible", file=sys.stderr)
        return 1
    cfg = gen_config("rich4k")
    R, D = cfg["replicas"], args.docs
    L = R * D
    res = {"tool": "tools/text_bench.py", "config": "rich4k", "docs": D, "replicas": R, "ops_per_log": cfg["ops_per_log"], "logs": L, "reps": args.reps,
           "box": "%s, %s, torch %s" % (torch.cuda.get_device_name(0), platform.node() or "host", torch.__version__), "commit": args.commit or commit()}
    with Engine(0) as eng:
        db, info = eng.generate(R, cfg["ops_per_log"], cfg["mix"], cfg["mark_types"], D, 4)
        dr = eng.alloc_result(db)
        ds = eng.upload_strings(wire.GEN_VALUES)
        eng.merge(db, dr)
        eng.sync()
        logs = eng.download_logs(dr, L)
        assert not logs["status"].any()
        nv, ns = int(logs["n_visible"].sum()), int(logs["n_spans"].sum())
        res["visible_elements"], res["spans"], res["visible_per_log"] = nv, ns, round(nv / L, 1)
        res["merge_ms"] = round(eng.merge_timed(db, dr, 3) / 3, 3)
        # ---- device ----
        kms = []

        def dev():
            t = eng.text(db, dr, ds)
            kms.append(t.kernel_ms)
            return t

        wall, wall_runs = timed(dev, args.reps)
        text = dev()
        units = int(text.text_off[-1])
        assert units == nv and not text.status.any()
        k = statistics.median(kms[1 : 1 + args.reps])
        moved = 2 * nv * (4 + 16) + 2 * units + 2 * units + ns * (8 + 4)
        compulsory = 2 * nv * 4 + 2 * units + ns * (8 + 4)  # what cannot come from a cache: the value ids (once per pass), the text written, span rows and span_unit
        res["device"] = {"kernel_ms": round(k, 3), "kernel_ms_runs": [round(x, 3) for x in kms[1 : 1 + args.reps]], "call_wall_ms": round(wall, 3), "call_wall_ms_runs": wall_runs,
                         "text_bytes": 2 * units, "bytes_moved_by_the_algorithm": moved, "assemble_gbps": round(moved / (k * 1e-3) / 1e9, 1),
                         "bytes_moved_per_text_byte": round(moved / (2 * units), 2), "compulsory_bytes": compulsory, "compulsory_gbps": round(compulsory / (k * 1e-3) / 1e9, 1),
                         "compulsory_bytes_per_text_byte": round(compulsory / (2 * units), 2)}
        # ---- host, Python: the parent's decoder over the same downloaded rows ----
        n_py = min(args.py_logs, L)
        actors_t, comments_t, log_doc_t = wire.generated_tables(D, R, info["n_comments"])
        sub = eng.download_range(db, dr, 0, n_py)
        sub_text = eng.text(db, dr, ds, 0, n_py)

        class Tables:  # what the decoders read of a batch: the string tables (the op columns of 5 x 10^7 rows stay on the device)
            values, urls, log_doc, doc_comments = wire.GEN_VALUES, wire.GEN_URLS, log_doc_t, comments_t

        tb = Tables
        join_ms, join_runs = timed(lambda: [wire.decode_spans(tb, sub, l) for l in range(n_py)], args.reps)
        slice_ms, slice_runs = timed(lambda: [wire.decode_spans_text(tb, sub, sub_text, l) for l in range(n_py)], args.reps)
        for l in range(min(n_py, 16)):
            assert wire.decode_spans(tb, sub, l) == wire.decode_spans_text(tb, sub, sub_text, l), l
        nv_py = int(sub.value_off[-1])
        res["host_python"] = {"logs": n_py, "visible_elements": nv_py, "decode_spans_join_ms": round(join_ms, 3), "decode_spans_join_ms_runs": join_runs,
                              "decode_spans_text_slice_ms": round(slice_ms, 3), "decode_spans_text_slice_ms_runs": slice_runs,
                              "join_ms_scaled_to_batch": round(join_ms * nv / max(nv_py, 1), 1), "slice_ms_scaled_to_batch": round(slice_ms * nv / max(nv_py, 1), 1)}
        # ---- host, node: decodeSpans against decodeSpansText over the same rows ----
        node = shutil.which("node")
        n_js = min(args.js_logs, L)
        if node:
            js = eng.download_range(db, dr, 0, n_js)
            js_text = eng.text(db, dr, ds, 0, n_js)
            with tempfile.TemporaryDirectory() as td:
                for name, a in (("logs", js.logs), ("values", js.values), ("spans", js.spans), ("cintervals", js.cintervals), ("valueOff", js.value_off), ("spanOff", js.span_off),
                                ("cintOff", js.cint_off), ("text", js_text.text), ("textOff", js_text.text_off), ("textStatus", js_text.status), ("spanUnit", js_text.span_unit)):
                    np.ascontiguousarray(a).tofile(os.path.join(td, name + ".bin"))
                with open(os.path.join(td, "meta.json"), "w") as f:
                    json.dump({"nLogs": n_js, "replicas": R, "nComments": [int(x) for x in info["n_comments"][: (n_js + R - 1) // R]], "reps": args.reps}, f)
                p = subprocess.run([node, os.path.join(ROOT, "tools", "text_bench_decode.js"), td], capture_output=True, text=True, timeout=900)
                if p.returncode != 0:
                    raise RuntimeError("tools/text_bench_decode.js failed:\n%s\n%s" % (p.stdout[-2000:], p.stderr[-2000:]))
                out = json.loads(p.stdout.strip().splitlines()[-1])
            nv_js = int(js.value_off[-1])
            out["join_ms_scaled_to_batch"] = round(out["decode_spans_join_ms"] * nv / max(nv_js, 1), 1)
            out["slice_ms_scaled_to_batch"] = round(out["decode_spans_text_slice_ms"] * nv / max(nv_js, 1), 1)
            out["visible_elements"] = nv_js
            res["host_js"] = out
        else:
            res["host_js"] = "not measured: node is not installed"
        # the comparison the issue asks for, stated plainly: the device call (kernels + download) + one slice per span against one lookup per element
        d_py = res["device"]["call_wall_ms"] + res["host_python"]["slice_ms_scaled_to_batch"]
        res["python_end_to_end_ms"] = {"device_text_plus_slices": round(d_py, 1), "host_join": res["host_python"]["join_ms_scaled_to_batch"],
                                       "device_path_is_faster": d_py < res["host_python"]["join_ms_scaled_to_batch"]}
        if isinstance(res["host_js"], dict):
            d_js = res["device"]["call_wall_ms"] + res["host_js"]["slice_ms_scaled_to_batch"]
            res["js_end_to_end_ms"] = {"device_text_plus_slices": round(d_js, 1), "host_join": res["host_js"]["join_ms_scaled_to_batch"],
                                       "device_path_is_faster": d_js < res["host_js"]["join_ms_scaled_to_batch"]}
        eng.free_strings(ds)
        eng.free_result(dr)
        eng.free_batch(db)
    out_path = args.out or os.path.join(ROOT, "profiles", "text_assembly.json")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
