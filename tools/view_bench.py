#!/usr/bin/env python3
"""A resident text view against the per-call paths it replaces, on one box, in one run -> profiles/text_view.json.

    python tools/view_bench.py [--docs 16384] [--reps 5] [--context 16] [--out FILE] [--commit ID]

Workload: the batch of profiles/text_assembly.json, find_text.json and text_slices.json — the `rich4k` mix (3 replicas x 4 096 ops per document), generated and
merged on the device; the string table is the generator's 128 one-unit strings.  Every side runs --reps times after one warm-up run, the two sides of a
comparison alternating; medians and ranges are reported, the runs are kept.
  create     Engine.text_view over the whole batch: ptx_view_desc.kernel_ms (HIP events around lengths, scan, plan, scan, assemble, prefix), the wall time of the
             call (two hipMalloc of the view's own blocks included) and the bytes held.  Freed after every run: hipFree is inside the next run's wall time.
  find       the two-unit and the sixteen-unit pattern of tools/find_bench.py through TextView.find_text against Engine.find_text: kernel_ms and call wall time.
  snippets   TextView.find_snippets with --context elements on both sides against the parent's path: Engine.find_text, the windows widened on the host with
             numpy, Engine.text_slices_flat.  kernel_ms (the parent's: both calls' summed) and wall time.
  agreement  every field of the hits and every unit, row and bound of the snippets must be equal between the two paths (asserted), and match_unit must point
             at the pattern in every snippet (asserted).
A record, no threshold: tests/test_emu_view.py and tests/test_gpu_view.py are the acceptance."""
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
    ap.add_argument("--context", type=int, default=16)
    ap.add_argument("--out")
    ap.add_argument("--commit", help="the commit measured (default: git rev-parse of the tree the tool stands in)")
    args = ap.parse_args()
    import torch

    from peritext_amd import wire
    from peritext_amd.engine import Engine
    from peritext_amd.workloads import gen_config

    if not torch.cuda.is_available():
        print("tools/view_bench.py measures on the GPU; none is visible", file=sys.stderr)
        return 1
    cfg = gen_config("rich4k")
    R, D, c = cfg["replicas"], args.docs, args.context
    L = R * D
    res = {"tool": "tools/view_bench.py", "config": "rich4k", "docs": D, "replicas": R, "ops_per_log": cfg["ops_per_log"], "logs": L, "reps": args.reps, "context": c,
           "box": "%s, %s, torch %s" % (torch.cuda.get_device_name(0), platform.node() or "host", torch.__version__), "commit": args.commit or commit()}
    with Engine(0) as eng:
        db, _ = eng.generate(R, cfg["ops_per_log"], cfg["mix"], cfg["mark_types"], D, 4)
        dr = eng.alloc_result(db)
        ds = eng.upload_strings(wire.GEN_VALUES)
        eng.merge(db, dr)
        eng.sync()
        text = eng.text(db, dr, ds, 0, 1)
        first = text.text[int(text.text_off[0]) : int(text.text_off[1])]

        # 1. creation
        def create():
            v = eng.text_view(db, dr, ds)
            km = v.info()["kernel_ms"]
            v.free()
            return km

        res["create"] = summary(side_by_side({"create": create}, args.reps)["create"])
        view = eng.text_view(db, dr, ds)
        info = view.info()
        res["create"].update({"bytes_held": info["bytes"], "text_units": info["n_units"], "text_bytes": 2 * info["n_units"], "prefix_words": info["n_prefix_words"],
                              "prefix_bytes": 4 * info["n_prefix_words"]})
        # 2. find, view against twin
        for name, m in (("pattern_2_units", 2), ("pattern_16_units", 16)):
            needle = np.ascontiguousarray(first[10 : 10 + m]).astype("<u2").tobytes().decode("utf-16-le", "surrogatepass")
            runs = side_by_side({"view": lambda: view.find_text(needle).kernel_ms, "twin": lambda: eng.find_text(db, dr, ds, needle).kernel_ms}, args.reps)
            a, b = view.find_text(needle), eng.find_text(db, dr, ds, needle)
            for f in ("status", "n_matches", "hit_off", "hit_unit", "hit_start", "hit_end"):
                assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), "view and twin disagree on " + f
            v, t = summary(runs["view"]), summary(runs["twin"])
            res["find_" + name] = {"needle": needle, "matches": int(a.n_matches.sum()), "listed_hits": int(a.hit_off[-1]), "view": v, "twin": t,
                                   "view_kernel_ms_is_lower": v["kernel_ms"] < t["kernel_ms"], "view_call_wall_ms_is_lower": v["call_wall_ms"] < t["call_wall_ms"]}
        # 3. snippets of +- context elements, view against find -> widen on the host -> slices
        needle = np.ascontiguousarray(first[10:12]).astype("<u2").tobytes().decode("utf-16-le", "surrogatepass")
        keep = {}

        def parent():
            hits = eng.find_text(db, dr, ds, needle)
            start = np.where(hits.hit_start >= c, hits.hit_start - c, 0).astype(np.uint32)
            end = (hits.hit_end.astype(np.uint64) + c).clip(max=0xFFFFFFFF).astype(np.uint32)
            cut = eng.text_slices_flat(db, dr, ds, hits.hit_off.astype(np.uint64), start, end)
            keep["parent"] = (hits, cut)
            return hits.kernel_ms + cut.kernel_ms

        def resident():
            keep["view"] = view.find_snippets(needle, c, c)
            return keep["view"].kernel_ms

        runs = side_by_side({"view": resident, "parent": parent}, args.reps)
        s, (hits, cut) = keep["view"], keep["parent"]
        for f in ("status", "n_matches", "hit_off", "hit_unit", "hit_start", "hit_end"):
            assert getattr(s.matches(), f).tobytes() == getattr(hits, f).tobytes(), "the two paths disagree on " + f
        for f in ("elem_start", "elem_end", "unit_off", "text", "sspan_off", "sspans", "sspan_unit"):
            assert getattr(s, f).tobytes() == getattr(cut, f).tobytes(), "the two paths disagree on " + f
        at = s.unit_off[:-1].astype(np.int64) + s.match_unit.astype(np.int64)
        pat = np.frombuffer(needle.encode("utf-16-le"), "<u2")
        assert all(np.array_equal(s.text[at + i], np.full(len(at), pat[i])) for i in range(len(pat))), "match_unit points at the pattern in every snippet"
        ns, nu, nr = len(s.elem_start), int(s.unit_off[-1]), int(s.sspan_off[-1])
        v, p = summary(runs["view"]), summary(runs["parent"])
        res["snippets"] = {"needle": needle, "snippets": ns, "units": nu, "span_rows": nr, "view": v, "parent_find_widen_slices": p,
                           "parent_bytes_uploaded_between_its_calls": 8 * (L + 1) + 8 * ns, "view_bytes_uploaded": 2 * len(pat),
                           "every_hit_and_every_snippet_unit_agree": True, "view_kernel_ms_is_lower": v["kernel_ms"] < p["kernel_ms"],
                           "view_call_wall_ms_is_lower": v["call_wall_ms"] < p["call_wall_ms"]}
        view.free()
        eng.free_strings(ds)
        eng.free_result(dr)
        eng.free_batch(db)
    out_path = args.out or os.path.join(ROOT, "profiles", "text_view.json")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
