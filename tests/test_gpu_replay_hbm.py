"""ptx_replay_patches on documents whose replay state does not fit one CU's LDS (ptx_replay_kernel_hbm, replay_hbm_core.h) — through ctypes and the C ABI on a
real MI355X: two such documents beside ordinary ones in one batch, record for record against the oracle; every log of the reference-made fixtures forced
through the HBM-state kernel (PTX_FLAG_REPLAY_HBM_STATE); tail streams; the patches of Changes made by ptx_change on such a document; and the JS host's
getPatches() on a 100 000-character replica.  The oracle runs ONCE for the module (replay_hbm_docs.expected, about two minutes)."""
import json
import os
import subprocess
import time

import numpy as np
import pytest

import helpers as H
import replay_hbm_docs as D
from peritext_amd import abi, wire

pytestmark = pytest.mark.gpu

ADDON = os.path.join(H.ROOT, "peritext_amd", "node", "peritext_node.node")
needs_node = pytest.mark.skipif(not H.have_node(), reason="node not installed")
needs_addon = pytest.mark.skipif(not os.path.exists(ADDON), reason="N-API addon not built (run __graft_entry__.build())")
_T0 = time.time()


def _load(name):
    with open(os.path.join(H.GOLDEN, name)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from peritext_amd.engine import Engine

    e = Engine(0)  # raises if libperitext_hip.so is missing or no gfx950 is visible: no fallback
    yield e
    e.close()
    print("\ntest_gpu_replay_hbm.py: %.0f s of wall time" % (time.time() - _T0))


@pytest.fixture(scope="module")
def big(eng):
    """The logs of ptxgen_mini.json plus docs A and B in ONE batch (the mini documents first: link urls get their ids in a batch-wide table in the order they are
    met, so the mini logs' records carry the ids they carry in a batch of their own); merged and replayed once with the default flags; the oracle's streams of A
    and B.  "at": the log index of A (B follows)."""
    mini = _load("ptxgen_mini.json")
    mini_docs = [d["logs"] for d in mini["docs"]]
    batch = wire.encode_docs(mini_docs + D.docs())
    db = eng.upload(batch)
    dr = eng.alloc_result(db)
    try:
        eng.merge(db, dr)
        res = eng.download(db, dr)
        pat = eng.replay_patches(db, dr)
        yield {"batch": batch, "db": db, "dr": dr, "res": res, "pat": pat, "mini_docs": mini_docs, "at": batch.n_logs - 2, "expected": D.expected() if H.have_node() else None}
    finally:
        eng.free_result(dr)
        eng.free_batch(db)


def _canonical(rec):
    """The records of one log with the comment ids of one insert patch (kind INSERT_COMMENT, emitted through an atomic counter) in id order."""
    is_c = rec["kind"] == abi.PATCH_INSERT_COMMENT
    start = np.arange(len(rec))
    start[is_c] = 0
    start = np.maximum.accumulate(start)
    return rec[np.lexsort((np.where(is_c, rec["a"], 0), is_c, start))]


@needs_node
def test_large_documents_beside_ordinary_ones_in_one_batch(eng, big):
    """[A], [B] and the mini logs, default flags: all statuses 0; A and B — beyond the LDS: PTX_ERR_CAPACITY before this kernel existed — match the oracle record
    for record and are the two logs the HBM-state kernel took; the mini logs take the ordinary launch, shaped by them alone, and give the records a replay
    of the mini batch alone gives (byte-equal up to the order of the comment records of one insert, which an atomic counter decides); one launch of each."""
    batch, pat, at = big["batch"], big["pat"], big["at"]
    assert (big["res"].logs["status"] == 0).all()
    assert [D.lds_working_set(batch, l) > 160 * 1024 for l in range(batch.n_logs)] == [False] * at + [True, True]
    assert (pat.logs["status"] == 0).all(), pat.logs
    assert pat.hbm_logs == 2 and pat.launches == 1 and pat.kernel_ms > 0
    exp = big["expected"]
    assert [int(x) for x in pat.logs["n_patches"][at:]] == [len(exp[0][0]["patches"]), len(exp[1][0]["patches"])]
    for log in range(2):  # every record of both logs
        got = H.norm_patches(wire.decode_patches(batch, pat, at + log))
        want = H.norm_patches(exp[log][0]["patches"])
        assert len(got) == len(want)
        for i, (x, y) in enumerate(zip(got, want)):
            assert x == y, "log %d patch %d: %r != %r" % (log, i, x, y)
    alone_batch = wire.encode_docs(big["mini_docs"])
    db = eng.upload(alone_batch)
    dr = eng.alloc_result(db)
    try:
        eng.merge(db, dr)
        alone = eng.replay_patches(db, dr)
    finally:
        eng.free_result(dr)
        eng.free_batch(db)
    assert alone.hbm_logs == 0 and alone.launches == 1 and (alone.logs["status"] == 0).all()
    assert alone_batch.n_logs == at and np.array_equal(alone.logs, pat.logs[:at])
    for l in range(at):
        assert np.array_equal(_canonical(D.stream(pat, l)), _canonical(D.stream(alone, l))), l


@pytest.mark.parametrize("names", [("patches_mini.json", None), ("patches_rich_300.json", None), ("ptxgen_config5_8192.json", "patches_config5_8192.json")])
def test_every_log_forced_through_the_hbm_state_kernel(names):
    """PTX_FLAG_REPLAY_HBM_STATE on the reference-made fixtures: every patch of every replica log, in order, deep-equal; every log counted in hbm_logs."""
    from peritext_amd.engine import Engine

    g = _load(names[0])
    p = _load(names[1]) if names[1] else g
    assert p["impl"] == "ref"
    batch = wire.encode_docs([d["logs"] for d in g["docs"]])
    with Engine(0, flags=abi.FLAG_REPLAY_HBM_STATE) as e:
        db = e.upload(batch)
        dr = e.alloc_result(db)
        try:
            e.merge(db, dr)
            pat = e.replay_patches(db, dr)
        finally:
            e.free_result(dr)
            e.free_batch(db)
    assert pat.hbm_logs == batch.n_logs and pat.launches == 1 and pat.kernel_ms > 0
    assert H.check_patch_streams(batch, pat, [d["expected"] for d in p["docs"]]) == batch.n_logs
    assert np.array_equal(pat.patch_off[1:] - pat.patch_off[:-1], np.where(pat.logs["status"] == 0, pat.logs["n_patches"], 0).astype(pat.patch_off.dtype))  # packed to exact offsets


def test_tail_streams_of_large_documents(eng, big):
    """ptx_replay_patches_from: the records of the last 500 rows of A and of B are exactly the last records of their whole streams."""
    batch, whole, at = big["batch"], big["pat"], big["at"]
    rows = np.diff(batch.log_off.astype(np.int64))
    first = np.where(np.arange(batch.n_logs) >= at, rows - 500, rows)  # (the mini logs: nothing asked for)
    tail = eng.replay_patches(big["db"], big["dr"], first_row=first)
    assert (tail.logs["status"] == 0).all() and tail.hbm_logs == 2
    for log in (at, at + 1):
        a = D.stream(whole, log)
        want = a[a["row"] >= first[log]]
        assert len(want) >= 500 and np.array_equal(D.stream(tail, log), want), log
    assert (tail.logs["n_patches"][:at] == 0).all()


def test_patches_of_changes_made_on_a_large_document(eng, big):
    """ptx_change on docs A and B (a delete on A; two inserts and a delete on B), the made Changes appended on the device, merged, and replayed from the old row
    counts: the records are those of the three / one ops at the indices asked for (doc B carries no marks: its inserts have none)."""
    batch, res, at = big["batch"], big["res"], big["at"]
    V = [int(res.logs["n_visible"][at]), int(res.logs["n_visible"][at + 1])]
    calls = [[] for _ in range(batch.n_logs)]
    calls[at] = [[{"path": ["text"], "action": "delete", "index": 5, "count": 1}]]
    calls[at + 1] = [[{"path": ["text"], "action": "insert", "index": V[1] - 10, "values": ["x", "y"]}, {"path": ["text"], "action": "delete", "index": V[1] // 2, "count": 1}]]
    actors = [log[0]["actor"] for logs in big["mini_docs"] for log in logs] + ["doc1", "doc1"]
    made_db = after = dr2 = None
    try:
        made_db, status = eng.change(big["db"], big["dr"], wire.encode_input_ops(batch, calls, actors))
        assert not status.any()
        after = eng.append_device(big["db"], made_db)
        dr2 = eng.alloc_result(after)
        eng.merge(after, dr2)
        logs2 = eng.download_logs(dr2, batch.n_logs)
        assert (logs2["status"] == 0).all() and int(logs2["n_visible"][at]) == V[0] - 1 and int(logs2["n_visible"][at + 1]) == V[1] + 2 - 1
        rows0 = np.diff(batch.log_off.astype(np.int64))
        pat = eng.replay_patches(after, dr2, first_row=rows0)
        assert (pat.logs["status"] == 0).all() and pat.hbm_logs == 2
        a, b = D.stream(pat, at), D.stream(pat, at + 1)
        r0, r1 = int(rows0[at]), int(rows0[at + 1])
        assert a.tolist() == [(r0, abi.PATCH_DELETE, 5, 1)]
        assert b.tolist() == [(r1, abi.PATCH_INSERT, V[1] - 10, 0), (r1 + 1, abi.PATCH_INSERT, V[1] - 9, 0), (r1 + 2, abi.PATCH_DELETE, V[1] // 2, 1)]
        assert (pat.logs["n_patches"][:at] == 0).all()
    finally:
        if dr2 is not None:
            eng.free_result(dr2)
        for h in (after, made_db):
            if h is not None:
                eng.free_batch(h)


@needs_node
@needs_addon
def test_node_host_get_patches_on_a_100000_character_replica():
    """The JS host imposes no size limit of its own on the patch path: a replica handle that receives one Change typing 100 000 characters (a replay working set
    of 200 KB) returns the makeList patch and 100 000 inserts, patch k at index k - 1 (tests/node_replay_hbm_check.js)."""
    p = subprocess.run([H.NODE, os.path.join(H.ROOT, "tests", "node_replay_hbm_check.js"), "100000"], cwd=H.ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert json.loads(p.stdout.strip().splitlines()[-1]) == {"ok": True, "patches": 100001}
