#!/usr/bin/env python3
"""The sync of replica logs on the device against the host path it replaces, on one box -> profiles/sync_replicas_<docs>_docs.json.

    python tools/sync_bench.py [--docs 8192] [--host-docs 16] [--out FILE]

Workload: a config-#4 batch (3 replicas x 4 096 ops per document, generated on the device); replica 1 of every document is cut back to the first half of
its log (a prefix of an application order is causally closed), then every replica 1 pulls from replica 0.
  device  ptx_sync_replicas + ptx_batch_append_device, wall time of the two calls (both synchronise), median of --reps runs
  host    ptx_batch_download of the batch; the reference's getMissingChanges + applyChanges loop restated in Python over the envelope columns (run on the first
          --host-docs documents and scaled to the batch: a host loop of microseconds per attempt, and half a config-#4 log takes far more attempts than the reference's guard allows: both paths run with the guard lifted, max_attempts = 0); ptx_batch_append of the re-encoded rows
The two paths must deliver the same changes in the same order (checked on the documents the host loop ran on).  A record, no threshold: the parity tests are the
acceptance (tests/test_emu_sync.py, tests/test_gpu_sync.py)."""
import argparse
import collections
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cut_replica_one(b, replicas):
    """The batch with log 1 of every document cut back to the first half of its changes."""
    from peritext_amd import abi, wire

    L, es = b.n_logs, abi.env_stride(b.max_actors)
    nops = b.chg_nops.astype(np.int64)
    row_of_chg = np.concatenate([[0], np.cumsum(nops)])
    keep_c, keep_r, log_off, chg_off = [], [], [0], [0]
    for l in range(L):
        c0, c1 = int(b.chg_off[l]), int(b.chg_off[l + 1])
        if l % replicas == 1:
            c1 = c0 + (c1 - c0) // 2
        keep_c.append(np.arange(c0, c1))
        keep_r.append(np.arange(row_of_chg[c0], row_of_chg[c1]))
        chg_off.append(chg_off[-1] + c1 - c0)
        log_off.append(log_off[-1] + int(row_of_chg[c1] - row_of_chg[c0]))
    kc, kr = np.concatenate(keep_c), np.concatenate(keep_r)
    env = b.chg_env.reshape(-1, es)[kc].reshape(-1)
    return wire.Batch(np.asarray(log_off, np.uint64), b.op_id[kr], b.ref_a[kr], b.ref_b[kr], b.payload[kr], b.action[kr], b.mark_type[kr], b.side_a[kr], b.side_b[kr],
                      np.asarray(chg_off, np.uint64), b.chg_hdr[kc], env, b.max_actors, None, b.values, b.urls, b.log_doc, b.doc_actors, b.doc_comments)


def host_sync(b, s, t):
    """getMissingChanges + applyChanges (reference/test/merge.ts:4-38) over the envelope columns of a downloaded batch: the source's change indices (relative to
    its log) in the order the target applies them, and the attempts the loop made."""
    actor, seq, deps = b.chg_actor, b.chg_seq, b.chg_deps
    s0, s1, t0, t1 = (int(x) for x in (b.chg_off[s], b.chg_off[s + 1], b.chg_off[t], b.chg_off[t + 1]))
    clock, order_of = {}, {}
    for c in range(t0, t1):
        clock[int(actor[c])] = max(clock.get(int(actor[c]), 0), int(seq[c]))
    for c in range(s0, s1):
        order_of.setdefault(int(actor[c]), []).append(c)
    queue = collections.deque(c for a, cs in order_of.items() for c in cs if int(seq[c]) > clock.get(a, 0))
    out, attempts = [], 0
    while queue:
        c = queue.popleft()
        a = int(actor[c])
        ok = int(seq[c]) == clock.get(a, 0) + 1 and all(clock.get(k, 0) >= int(d) for k, d in enumerate(deps[c]) if d)
        if ok:
            clock[a] = int(seq[c])
            out.append(c - s0)
        else:
            queue.append(c)
        attempts += 1  # (no guard: half a config-#4 log takes far more than the reference's 10 001 attempts — both paths run unbounded)
    return out, attempts


def rows_of(b, log, chgs):
    """wire columns of the given changes (indices relative to the log) of one log, in that order."""
    c0 = int(b.chg_off[log])
    nops = b.chg_nops.astype(np.int64)
    first = int(b.log_off[log]) + np.concatenate([[0], np.cumsum(nops[c0:int(b.chg_off[log + 1])])])
    rows = np.concatenate([np.arange(first[c], first[c + 1]) for c in chgs] + [np.zeros(0, np.int64)]).astype(np.int64)
    return rows, np.asarray(chgs, np.int64) + c0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=8192)
    ap.add_argument("--host-docs", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    from peritext_amd import wire
    from peritext_amd.engine import Engine
    from peritext_amd.workloads import gen_config

    cfg = gen_config("config4")
    R, D = cfg["replicas"], args.docs
    res = {"tool": "tools/sync_bench.py", "config": "config4", "docs": D, "replicas": R, "ops_per_log": cfg["ops_per_log"], "reps": args.reps}
    with Engine(0) as eng:
        gen_h, info = eng.generate(R, cfg["ops_per_log"], cfg["mix"], cfg["mark_types"], D, 4)
        actors_t, comments_t, log_doc_t = wire.generated_tables(D, R, info["n_comments"])
        full = eng.download_batch(gen_h, wire.GEN_VALUES, wire.GEN_URLS, log_doc_t, actors_t, comments_t)
        eng.free_batch(gen_h)
        base = cut_replica_one(full, R)
        del full
        db = eng.upload(base)
        pairs = [(d * R, d * R + 1) for d in range(D)]
        res["changes_in_batch"], res["rows_in_batch"] = int(base.chg_off[-1]), int(base.n_ops)
        # ---- device ----
        t_sync, t_app = [], []
        more_h = grown_h = None
        for _ in range(args.reps + 1):  # (the first run warms the block pool)
            for h in (more_h, grown_h):
                if h is not None:
                    eng.free_batch(h)
            t0 = time.perf_counter()
            more_h, status = eng.sync_replicas(db, pairs, max_attempts=0)
            t1 = time.perf_counter()
            grown_h = eng.append_device(db, more_h)
            t2 = time.perf_counter()
            t_sync.append((t1 - t0) * 1e3)
            t_app.append((t2 - t1) * 1e3)
        assert not status.any()
        res["delivered_changes"], res["delivered_rows"] = eng.n_changes(more_h), eng.n_ops(more_h)
        res["device"] = {"sync_replicas_ms": round(statistics.median(t_sync[1:]), 3), "append_device_ms": round(statistics.median(t_app[1:]), 3),
                         "total_ms": round(statistics.median([a + b for a, b in zip(t_sync[1:], t_app[1:])]), 3)}
        more = eng.download_batch(more_h, wire.GEN_VALUES, wire.GEN_URLS, log_doc_t, actors_t, comments_t)
        # ---- host ----
        t0 = time.perf_counter()
        host = eng.download_batch(db, wire.GEN_VALUES, wire.GEN_URLS, log_doc_t, actors_t, comments_t)
        t_down = (time.perf_counter() - t0) * 1e3
        n_host = min(args.host_docs, D)
        t0 = time.perf_counter()
        synced = [host_sync(host, d * R, d * R + 1) for d in range(n_host)]
        t_loop = (time.perf_counter() - t0) * 1e3
        res["attempts_per_pair_mean"] = round(statistics.mean(a for _, a in synced), 1)
        for d, (order, _) in enumerate(synced):  # the same changes in the same order
            t = d * R + 1
            _, chgs = rows_of(host, d * R, order)
            assert np.array_equal(more.chg_hdr[int(more.chg_off[t]):int(more.chg_off[t + 1])], host.chg_hdr[chgs]), "document %d" % d
            assert np.array_equal(more.chg_seq[int(more.chg_off[t]):int(more.chg_off[t + 1])], host.chg_seq[chgs]), "document %d" % d
        # the re-encode of what was chosen + ptx_batch_append (`more` stands in for the rows the host loop chose: the same rows)
        t0 = time.perf_counter()
        h2 = eng.append(db, more)
        t_append = (time.perf_counter() - t0) * 1e3
        eng.free_batch(h2)
        res["host"] = {"batch_download_ms": round(t_down, 3), "python_loop_docs": n_host, "python_loop_ms": round(t_loop, 3), "python_loop_ms_scaled_to_batch": round(t_loop * D / n_host, 1),
                       "batch_append_ms": round(t_append, 3), "total_ms": round(t_down + t_loop * D / n_host + t_append, 1)}
        for h in (more_h, grown_h, db):
            eng.free_batch(h)
    out = args.out or os.path.join(ROOT, "profiles", "sync_replicas_%d_docs.json" % D)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
