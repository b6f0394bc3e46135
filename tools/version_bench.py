#!/usr/bin/env python3
"""Resident logs cut at past versions on the device against the host path it replaces, on one box -> profiles/versions_<docs>_docs.json.

    python tools/version_bench.py [--docs 8192] [--host-docs 64] [--cuts 8] [--out FILE]

Workload: a config-#4 batch (3 replicas x 4 096 ops per document, generated on the device); the replica-0 log of every document is cut at --cuts evenly
spaced prefixes of its changes in ONE call (the history strip of a scrubber), then the cut logs are merged.
  device  ptx_batch_at_versions (synchronises) + ptx_merge + ptx_sync, wall time, median of --reps runs
  host    ptx_batch_download of the batch; the prefixes taken in Python (numpy index arithmetic over the columns and the envelope); ptx_batch_upload of the
          re-encoded logs; the same merge.  Filter, upload and merge run on the first --host-docs documents and are scaled to the batch (the cut logs of
          the whole batch are gigabytes of host memory); the download is the whole batch's, as the host path needs it.
The two paths must deliver the same logs (checked column by column on the documents the host path ran on).  A record, no threshold: the parity tests are
the acceptance (tests/test_emu_versions.py, tests/test_gpu_versions.py)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_prefixes(b, src, ks):
    """wire.Batch whose log c holds the first ks[c] changes of log src[c] of the downloaded batch `b`."""
    from peritext_amd import abi, wire

    es = abi.env_stride(b.max_actors)
    row_of_chg = np.concatenate([[0], np.cumsum(b.chg_nops.astype(np.int64))])
    keep_c, keep_r, log_off, chg_off = [], [], [0], [0]
    for s, k in zip(src, ks):
        c0 = int(b.chg_off[s])
        c1 = min(c0 + int(k), int(b.chg_off[s + 1]))
        keep_c.append(np.arange(c0, c1))
        keep_r.append(np.arange(row_of_chg[c0], row_of_chg[c1]))
        chg_off.append(chg_off[-1] + c1 - c0)
        log_off.append(log_off[-1] + int(row_of_chg[c1] - row_of_chg[c0]))
    kc, kr = np.concatenate(keep_c), np.concatenate(keep_r)
    env = b.chg_env.reshape(-1, es)[kc].reshape(-1)
    return wire.Batch(np.asarray(log_off, np.uint64), b.op_id[kr], b.ref_a[kr], b.ref_b[kr], b.payload[kr], b.action[kr], b.mark_type[kr], b.side_a[kr], b.side_b[kr],
                      np.asarray(chg_off, np.uint64), b.chg_hdr[kc], env, b.max_actors, None, b.values, b.urls, [b.log_doc[int(s)] for s in src], b.doc_actors, b.doc_comments)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=8192)
    ap.add_argument("--host-docs", type=int, default=64)
    ap.add_argument("--cuts", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    from peritext_amd import wire
    from peritext_amd.engine import Engine
    from peritext_amd.workloads import gen_config

    cfg = gen_config("config4")
    R, D, K = cfg["replicas"], args.docs, args.cuts
    res = {"tool": "tools/version_bench.py", "config": "config4", "docs": D, "replicas": R, "ops_per_log": cfg["ops_per_log"], "cuts_per_log": K, "reps": args.reps}
    with Engine(0) as eng:
        db, info = eng.generate(R, cfg["ops_per_log"], cfg["mix"], cfg["mark_types"], D, 4)
        actors_t, comments_t, log_doc_t = wire.generated_tables(D, R, info["n_comments"])
        tables = (wire.GEN_VALUES, wire.GEN_URLS, log_doc_t, actors_t, comments_t)
        # ---- host: the download first (it also tells both paths where the prefixes stand) ----
        t0 = time.perf_counter()
        host = eng.download_batch(db, *tables)
        t_down = (time.perf_counter() - t0) * 1e3
        n_chg = np.diff(host.chg_off.astype(np.int64))
        src = np.repeat(np.arange(D, dtype=np.uint32) * R, K)
        ks = np.concatenate([[(n_chg[d * R] * (j + 1)) // K for j in range(K)] for d in range(D)]).astype(np.uint32)
        res["changes_in_batch"], res["rows_in_batch"], res["cuts"] = int(host.chg_off[-1]), int(host.n_ops), len(src)
        # ---- device ----
        t_cut, t_merge = [], []
        cut_h = dr = None
        for _ in range(args.reps + 1):  # (the first run warms the block pool)
            if dr is not None:
                eng.free_result(dr)
            if cut_h is not None:
                eng.free_batch(cut_h)
            t0 = time.perf_counter()
            cut_h, status, n_kept, first_row, _ = eng.at_versions(db, src, prefix=ks)
            t1 = time.perf_counter()
            dr = eng.alloc_result(cut_h)
            eng.merge(cut_h, dr)
            eng.sync()
            t2 = time.perf_counter()
            t_cut.append((t1 - t0) * 1e3)
            t_merge.append((t2 - t1) * 1e3)
        assert not status.any() and np.array_equal(n_kept, ks)
        res["cut_changes"], res["cut_rows"] = eng.n_changes(cut_h), eng.n_ops(cut_h)
        res["device"] = {"at_versions_ms": round(statistics.median(t_cut[1:]), 3), "merge_ms": round(statistics.median(t_merge[1:]), 3),
                         "total_ms": round(statistics.median([a + b for a, b in zip(t_cut[1:], t_merge[1:])]), 3)}
        eng.free_result(dr)
        # ---- host, on the first documents: filter, upload, merge ----
        n_host = min(args.host_docs, D)
        m = n_host * K
        t0 = time.perf_counter()
        cut_host = host_prefixes(host, src[:m], ks[:m])
        t_filter = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        up_h = eng.upload(cut_host)
        t_up = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        dr = eng.alloc_result(up_h)
        eng.merge(up_h, dr)
        eng.sync()
        t_hmerge = (time.perf_counter() - t0) * 1e3
        host_res = eng.download(up_h, dr)
        eng.free_result(dr)
        eng.free_batch(up_h)
        # both deliver the same logs: the device's cut of the same documents, column by column, and the same merged documents
        chk_h, _, _, _, _ = eng.at_versions(db, src[:m], prefix=ks[:m])
        got = eng.download_batch(chk_h, wire.GEN_VALUES, wire.GEN_URLS, cut_host.log_doc, actors_t, comments_t)
        for name in ("log_off", "op_id", "ref_a", "ref_b", "payload", "action", "mark_type", "side_a", "side_b", "chg_off", "chg_hdr", "chg_env"):
            assert np.array_equal(getattr(got, name), getattr(cut_host, name)), "the device's cut logs differ from the host path's in %s" % name
        dr = eng.alloc_result(chk_h)
        eng.merge(chk_h, dr)
        eng.sync()
        dev_res = eng.download(chk_h, dr)
        assert not dev_res.logs["status"].any() and np.array_equal(dev_res.logs["digest"], host_res.logs["digest"]), "the merged cut logs differ"
        eng.free_result(dr)
        eng.free_batch(chk_h)
        scale = D / n_host
        res["host"] = {"batch_download_ms": round(t_down, 3), "docs": n_host, "python_filter_ms": round(t_filter, 3), "batch_upload_ms": round(t_up, 3), "merge_ms": round(t_hmerge, 3),
                       "filter_upload_merge_ms_scaled_to_batch": round((t_filter + t_up + t_hmerge) * scale, 1), "total_ms": round(t_down + (t_filter + t_up + t_hmerge) * scale, 1)}
        res["same_logs_checked_on_docs"] = n_host
        eng.free_batch(cut_h)
        eng.free_batch(db)
    out = args.out or os.path.join(ROOT, "profiles", "versions_%d_docs.json" % D)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
