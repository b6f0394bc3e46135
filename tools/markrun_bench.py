#!/usr/bin/env python3
"""Queries by format on a resident text view against the host path they replace, on one box, in one run -> profiles/mark_queries.json.

    python tools/markrun_bench.py [--docs 16384] [--reps 5] [--out FILE] [--commit ID]

Workload: the batch of profiles/text_view.json — the `rich4k` mix (3 replicas x 4 096 ops per document), generated and merged on the device, one resident view of
all of it.  Every side runs --reps times after one warm-up run, the two sides of a comparison alternating; medians and ranges are reported, the runs are kept.
  mark_runs      strong, any link, any comment through TextView.mark_runs against the host path: Engine.download_range of the whole batch (spans, cintervals and
                 the value ids the units need), the runs coalesced with numpy over all logs at once, their units from a cumulative sum of the strings' lengths
  mark_snippets  any comment with +-0 and +-16 elements through TextView.mark_snippets against: the same download and coalescing, the windows widened with numpy,
                 TextView.text_slices_flat
  find_in_marks  "5d" inside strong through TextView.find_in_marks against: the same download and coalescing, TextView.find_text, a numpy filter
  agreement      both sides must agree on every run, every unit, every snippet unit and row, and every hit (asserted)
kernel_ms is what the library's calls report (HIP events around their launches); the host side's is the sum over its calls, and Engine.download_range reports
none — its gather kernels are inside its wall time only.  A record, no threshold: tests/test_emu_markruns.py and tests/test_gpu_markruns.py are the acceptance."""
import argparse
import json
import os
import platform
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from view_bench import commit, side_by_side, summary  # noqa: E402


def host_runs(rows, mark_type, ident, table_len, abi):
    """(run_off, start, end, id, unit, len) of every log of a downloaded range, coalesced with numpy over all logs at once."""
    n = len(rows.logs)
    nv = (rows.value_off[1:] - rows.value_off[:-1]).astype(np.int64)
    cs = np.concatenate([[0], np.cumsum(table_len[rows.values], dtype=np.int64)])  # units before every element of the range
    if mark_type == abi.MARK_COMMENT:
        c = rows.cintervals
        log = np.repeat(np.arange(n), (rows.cint_off[1:] - rows.cint_off[:-1]).astype(np.int64))
        keep = np.ones(len(c), bool) if ident == abi.MARK_ANY_ID else c["id"] == ident
        log, start, end, rid = log[keep], c["start"][keep].astype(np.int64), c["end"][keep].astype(np.int64), c["id"][keep]
    else:
        sp = rows.spans
        cnt = (rows.span_off[1:] - rows.span_off[:-1]).astype(np.int64)
        row_log = np.repeat(np.arange(n), cnt)
        attr, st = sp["attr"].astype(np.uint32), sp["start"].astype(np.int64)
        flag = {abi.MARK_STRONG: abi.ATTR_STRONG, abi.MARK_EM: abi.ATTR_EM, abi.MARK_LINK: abi.ATTR_LINK}[mark_type]
        key = attr & np.uint32(abi.ATTR_ID_MASK) if mark_type == abi.MARK_LINK else np.zeros(len(sp), np.uint32)
        m = (attr & np.uint32(flag)) != 0
        if mark_type == abi.MARK_LINK and ident != abi.MARK_ANY_ID:
            m &= key == np.uint32(ident)
        joined = m[1:] & m[:-1] & (key[1:] == key[:-1]) & (row_log[1:] == row_log[:-1])
        first = m & ~np.concatenate([[False], joined])
        last = m & ~np.concatenate([joined, [False]])
        nxt = np.concatenate([st[1:], [0]])
        is_log_end = np.concatenate([row_log[1:] != row_log[:-1], [True]])
        nxt[is_log_end] = nv[row_log[is_log_end]]
        log, start, end, rid = row_log[first], st[first], nxt[last], key[first]
    base = rows.value_off[:-1].astype(np.int64)[log]
    unit = cs[base + start] - cs[base]
    length = cs[base + end] - cs[base + start]
    run_off = np.concatenate([[0], np.cumsum(np.bincount(log, minlength=n))]).astype(np.uint64)
    return run_off, start.astype(np.uint32), end.astype(np.uint32), rid.astype(np.uint32), unit.astype(np.uint32), length.astype(np.uint32)


def same_runs(got, host):
    for f, h in zip(("run_off", "run_start", "run_end", "run_id", "run_unit", "run_len"), host):
        assert getattr(got, f).tobytes() == h.astype(getattr(got, f).dtype).tobytes(), "the two paths disagree on " + f


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
        print("tools/markrun_bench.py measures on the GPU; none is visible", file=sys.stderr)
        return 1
    cfg = gen_config("rich4k")
    R, D = cfg["replicas"], args.docs
    L = R * D
    res = {"tool": "tools/markrun_bench.py", "config": "rich4k", "docs": D, "replicas": R, "ops_per_log": cfg["ops_per_log"], "logs": L, "reps": args.reps,
           "box": "%s, %s, torch %s" % (torch.cuda.get_device_name(0), platform.node() or "host", torch.__version__), "commit": args.commit or commit()}
    table_len = np.array([len(v.encode("utf-16-le")) // 2 for v in wire.GEN_VALUES], dtype=np.int64)
    with Engine(0) as eng:
        db, _ = eng.generate(R, cfg["ops_per_log"], cfg["mix"], cfg["mark_types"], D, 4)
        dr = eng.alloc_result(db)
        ds = eng.upload_strings(wire.GEN_VALUES)
        eng.merge(db, dr)
        eng.sync()
        view = eng.text_view(db, dr, ds)
        eng.free_strings(ds)
        keep = {}

        def host(mark_type, ident):
            rows = eng.download_range(db, dr, 0, L)
            return host_runs(rows, mark_type, ident, table_len, abi)

        # 1. the runs
        for name, mt in (("strong", abi.MARK_STRONG), ("any_link", abi.MARK_LINK), ("any_comment", abi.MARK_COMMENT)):
            def device():
                keep["d"] = view.mark_runs(mt)
                return keep["d"].kernel_ms

            def parent():
                keep["h"] = host(mt, abi.MARK_ANY_ID)
                return 0.0

            runs = side_by_side({"view": device, "host": parent}, args.reps)
            same_runs(keep["d"], keep["h"])
            v, h = summary(runs["view"]), summary(runs["host"])
            h["kernel_ms_note"] = "Engine.download_range reports no kernel time"
            res["mark_runs_" + name] = {"runs": int(keep["d"].run_off[-1]), "view": v, "host_download_coalesce": h, "every_run_and_unit_agrees": True,
                                        "view_call_wall_ms_is_lower": v["call_wall_ms"] < h["call_wall_ms"], "wall_ratio_host_over_view": round(h["call_wall_ms"] / v["call_wall_ms"], 2)}
        # 2. every comment with its text
        for c in (0, 16):
            def device():
                keep["d"] = view.mark_snippets(abi.MARK_COMMENT, before=c, after=c)
                return keep["d"].kernel_ms

            def parent():
                off, start, end, rid, unit, length = host(abi.MARK_COMMENT, abi.MARK_ANY_ID)
                ws = np.where(start >= c, start - c, 0).astype(np.uint32)
                we = (end.astype(np.uint64) + c).clip(max=0xFFFFFFFF).astype(np.uint32)
                cut = view.text_slices_flat(off, ws, we)
                keep["h"] = ((off, start, end, rid, unit, length), cut)
                return cut.kernel_ms

            runs = side_by_side({"view": device, "host": parent}, args.reps)
            s, (hr, cut) = keep["d"], keep["h"]
            same_runs(s.runs(), hr)
            for f in ("elem_start", "elem_end", "unit_off", "text", "sspan_off", "sspans", "sspan_unit"):
                assert getattr(s, f).tobytes() == getattr(cut, f).tobytes(), "the two paths disagree on " + f
            v, h = summary(runs["view"]), summary(runs["host"])
            h["kernel_ms_note"] = "TextView.text_slices_flat only: Engine.download_range reports no kernel time"
            res["mark_snippets_any_comment_context_%d" % c] = {"snippets": len(s.elem_start), "units": int(s.unit_off[-1]), "span_rows": int(s.sspan_off[-1]), "view": v,
                                                               "host_download_coalesce_slices": h, "every_run_unit_and_row_agrees": True,
                                                               "view_call_wall_ms_is_lower": v["call_wall_ms"] < h["call_wall_ms"],
                                                               "wall_ratio_host_over_view": round(h["call_wall_ms"] / v["call_wall_ms"], 2)}
        # 3. a find inside strong
        needle = "5d"

        def device():
            keep["d"] = view.find_in_marks(needle, abi.MARK_STRONG)
            return keep["d"].kernel_ms

        def parent():
            off, start, end, _, _, _ = host(abi.MARK_STRONG, abi.MARK_ANY_ID)
            m = view.find_text(needle)
            hit_log = np.repeat(np.arange(L, dtype=np.int64), (m.hit_off[1:] - m.hit_off[:-1]).astype(np.int64))
            run_log = np.repeat(np.arange(L, dtype=np.int64), (off[1:] - off[:-1]).astype(np.int64))
            at = np.searchsorted((run_log << 32) | start.astype(np.int64), (hit_log << 32) | m.hit_start.astype(np.int64), side="right") - 1  # the last run with (log, start) <= the hit's
            ok = at >= 0
            at = np.maximum(at, 0)
            ok &= (run_log[at] == hit_log) & (m.hit_end <= end[at]) if len(start) else False
            kept_off = np.concatenate([[0], np.cumsum(np.bincount(hit_log[ok], minlength=L))]).astype(np.uint64)
            keep["h"] = (kept_off, m.hit_unit[ok], m.hit_start[ok], m.hit_end[ok], int(m.hit_off[-1]))
            return m.kernel_ms

        runs = side_by_side({"view": device, "host": parent}, args.reps)
        g, (koff, ku, ks, ke, nall) = keep["d"], keep["h"]
        assert g.hit_off.tobytes() == koff.tobytes() and g.hit_unit.tobytes() == ku.tobytes() and g.hit_start.tobytes() == ks.tobytes() and g.hit_end.tobytes() == ke.tobytes()
        assert np.array_equal(g.n_matches.astype(np.uint64), koff[1:] - koff[:-1])
        v, h = summary(runs["view"]), summary(runs["host"])
        h["kernel_ms_note"] = "TextView.find_text only: Engine.download_range reports no kernel time"
        res["find_in_marks_5d_strong"] = {"needle": needle, "matches_in_the_view": nall, "contained": int(g.hit_off[-1]), "view": v, "host_download_coalesce_find_filter": h,
                                          "every_hit_agrees": True, "view_call_wall_ms_is_lower": v["call_wall_ms"] < h["call_wall_ms"],
                                          "wall_ratio_host_over_view": round(h["call_wall_ms"] / v["call_wall_ms"], 2)}
        view.free()
        eng.free_result(dr)
        eng.free_batch(db)
    out_path = args.out or os.path.join(ROOT, "profiles", "mark_queries.json")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
