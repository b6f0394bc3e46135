"""Logs beyond one CU's LDS on the GPU (VERDICT r2 "missing" #3 / next #7): the library routes them to ptx_merge_big_kernel (biglog_core.h: working set in HBM
scratch, 32-bit indices, one 1 024-thread workgroup per log) inside the SAME ptx_merge call that merges the ordinary logs of the batch through the LDS kernel.
A 100 000-op insert/delete document (the reference's arrays have no bound: reference/src/micromerge.ts:614-672) and all-marks documents of 20 000 and 40 000 ops,
against the oracle; a failing large log names the reference's error and the failing row."""
import copy
import dataclasses
import json
import os

import numpy as np
import pytest

import helpers as H
from peritext_amd import abi, wire

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch  # (first, like the other GPU suites: torch brings its own HIP runtime, which must be the one the process initialises)

    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from peritext_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def _load(name):
    with open(os.path.join(H.GOLDEN, name)) as f:
        return json.load(f)


@pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")
def test_large_logs_beside_ordinary_ones(eng):
    small = _load("ptxgen_config4_600.json")
    essay = H.oracle_gen("config2", 1, 77, 100000, 1)          # 100 000 ops: ~64 000 list elements, beyond the LDS kernel's 16-bit element index
    marks40 = H.synthetic_marks_log(6000, 34000, 9)            # 40 001 rows of which 34 000 mark ops: mark lists alone beyond one CU's LDS
    marks20 = H.synthetic_marks_log(4000, 16000, 5)            # 20 001 rows: the LDS kernel holds it with a CU to itself
    exp_marks = H.oracle_apply([[marks40], [marks20]], no_patches=True, timeout=1200)
    docs = [d["logs"] for d in small["docs"]] + [essay["docs"][0]["logs"], [marks40], [marks20]]
    expected = [e for d in small["docs"] for e in d["expected"]] + [essay["docs"][0]["expected"][0], exp_marks[0][0], exp_marks[1][0]]
    batch = wire.encode_docs(docs)
    db = eng.upload(batch)
    dr = eng.alloc_result(db)
    try:
        for _ in range(2):  # the scratch of the large logs is reused from merge to merge
            eng.merge(db, dr)
        res = eng.download(db, dr)
    finally:
        eng.free_result(dr)
        eng.free_batch(db)
    assert (res.logs["status"] == 0).all()
    for log, exp in enumerate(expected):
        H.check_log(batch, res, log, exp)
    n_small = sum(len(d["logs"]) for d in small["docs"])
    lds = res.logs["reserved"][:, 0]
    assert (lds[:n_small] > 0).all() and lds[n_small] == 0 and lds[n_small + 1] == 0  # the two largest took the HBM-staged kernel (it reports no LDS figure)
    assert int(res.logs["n_elems"][n_small]) > 32766 and int(res.logs["n_ops"][n_small + 1]) == 40000
    # every replica of the ordinary documents still converges, and the launch shape of the LDS kernel is the ordinary logs' own (not the CU maximum)
    dg = res.logs["digest"][:n_small].reshape(-1, 3, 2)
    assert (dg == dg[:, :1, :]).all()
    # on a runtime without cooperative launch (played by PTX_NO_COOPERATIVE) the logs of 16 384 rows and more are merged by one workgroup of the
    # HBM-staged kernel each — the same results, never a failed batch
    os.environ["PTX_NO_COOPERATIVE"] = "1"
    try:
        db = eng.upload(batch)
        dr = eng.alloc_result(db)
        try:
            eng.merge(db, dr)
            res2 = eng.download(db, dr)
        finally:
            eng.free_result(dr)
            eng.free_batch(db)
    finally:
        del os.environ["PTX_NO_COOPERATIVE"]
    assert (res2.logs["status"] == 0).all() and (res2.logs["digest"] == res.logs["digest"]).all() and (res2.logs["n_spans"] == res.logs["n_spans"]).all()


@pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")
def test_a_failing_large_log_names_the_error_and_the_row(eng):
    essay = H.oracle_gen("config2", 1, 77, 100000, 1)["docs"][0]["logs"][0]
    bad = copy.deepcopy(essay)
    c = len(bad) * 2 // 3
    op = next(o for o in bad[c]["ops"] if o["action"] == "del" or o.get("insert"))
    op["elemId"] = "999999@zz"  # an element nobody inserted: RangeError("List element not found"), micromerge.ts:752
    row = sum(len(ch["ops"]) for ch in bad[:c]) + bad[c]["ops"].index(op)
    dropped = copy.deepcopy(essay)
    del dropped[len(dropped) // 2]  # a change is missing: the next change of that actor fails the seq check (single actor: micromerge.ts:501-504)
    row2 = sum(len(ch["ops"]) for ch in dropped[: len(dropped) // 2])
    batch = wire.encode_docs([[bad], [dropped], [essay]], extra_actors=[["zz"], [], []])
    res = eng.apply_materialize(batch)
    assert [int(x) for x in res.logs["status"]] == [abi.ERR_ELEM_NOT_FOUND, abi.ERR_SEQ_GAP, 0]
    assert int(res.logs["reserved"][0, 1]) == row and int(res.logs["reserved"][1, 1]) == row2


@pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")
def test_long_log_of_several_actors_whose_values_stay_narrow(eng):
    """ADVICE r4 (medium), GPU twin: 2 actors x 33 000 one-op changes — more than 65 533 changes, no value near 65 535, hence no wide column: admitted by the
    HBM-staged kernel (round 4: PTX_ERR_CAPACITY); so is a resident log that two narrow parts make this long (ptx_batch_append_device)."""
    import copy

    from test_emu_biglog import _typed_log

    a = _typed_log(33000)
    b = _typed_log(33000, actor="b", first_ctr=33001, make_list=False, deps_of=lambda k: {"a": 33000})
    far = copy.deepcopy(b)
    far[10]["deps"] = {"a": 33001}
    docs = [[a + b], [a + far]]
    batch = wire.encode_docs(docs)
    assert batch.chg_env_hi is None
    exp = H.oracle_apply(docs, no_patches=True, timeout=900)
    res = eng.apply_materialize(batch)
    assert int(res.logs["status"][0]) == 0 and int(res.logs["n_visible"][0]) == 65999
    H.check_log(batch, res, 0, exp[0][0])
    assert int(res.logs["status"][1]) == abi.ERR_MISSING_DEP and int(res.logs["reserved"][1, 1]) == 33010
    # two narrow parts (40 000 + 26 000 changes) appended on the device cross the 65 533-change line of the LDS kernel's admission
    one = wire.encode_docs([docs[0]])
    head, tail = wire.split_batch(one, [40000])
    head, tail = dataclasses.replace(head, chg_env_hi=None), dataclasses.replace(tail, chg_env_hi=None)
    db, dm = eng.upload(head), eng.upload(tail)
    db2 = eng.append_device(db, dm)
    dr = eng.alloc_result(db2)
    try:
        eng.merge(db2, dr)
        logs = eng.download_logs(dr, 1)
    finally:
        eng.free_result(dr)
        for x in (db2, dm, db):
            eng.free_batch(x)
    assert int(logs["status"][0]) == 0 and (logs["digest"][0] == res.logs["digest"][0]).all()


def test_logs_with_more_than_65535_changes(eng):
    """seq / deps are plain numbers in the reference (micromerge.ts:499-511); a replica typed as one change per keystroke passes 65 535
    changes of one actor.  Through the C ABI: the wide envelope column goes up with the batch, the census sends these logs to the HBM-staged kernel, every
    change is admitted; failing logs past 65 535 name the reference's error and the row; an ordinary document in the same batch keeps the LDS kernel; a
    resident log that CROSSES 65 535 changes by ptx_batch_append stays valid.  Expected values: the type-erased reference itself."""
    from test_emu_biglog import wide_envelope_docs, wide_envelope_expected

    docs = wide_envelope_docs()
    names = list(docs)
    small = _load("ptxgen_mini.json")
    all_docs = [docs[k] for k in names] + [d["logs"] for d in small["docs"]]
    exp = wide_envelope_expected(docs) + [d["expected"] for d in small["docs"]]
    batch = wire.encode_docs(all_docs)
    assert batch.chg_env_hi is not None
    res = eng.apply_materialize(batch)
    want = {"single": (0, None), "deps_cross": (0, None), "dep_missing": (abi.ERR_MISSING_DEP, 66001), "seq_gap": (abi.ERR_SEQ_GAP, 66000), "seq_twice": (abi.ERR_SEQ_GAP, 66005)}
    for log, k in enumerate(names):
        st, row = want[k]
        assert int(res.logs["status"][log]) == st, (k, int(res.logs["status"][log]), int(res.logs["reserved"][log, 1]))
        assert ("error" in exp[log][0]) == (st != 0)
        if st == 0:
            H.check_log(batch, res, log, exp[log][0])
        else:
            assert int(res.logs["reserved"][log, 1]) == row
    log = len(names)
    for d in exp[len(names):]:
        for e in d:
            H.check_log(batch, res, log, e)
            assert int(res.logs["reserved"][log, 0]) > 0  # the ordinary logs took the LDS kernel
            log += 1
    # streaming append across the 16-bit line: 65 000 changes resident, 5 001 more arrive (their seqs need the wide column, the base had none)
    one = wire.encode_docs([docs["single"]])
    head, tail = wire.split_batch(one, [65000])  # (one encoding, cut in two: both parts use the same value ids)
    assert not head.chg_env_hi.any() and tail.chg_env_hi.any()
    head = dataclasses.replace(head, chg_env_hi=None)  # what an encoder sends while every value fits 16 bits
    db = eng.upload(head)
    db2 = eng.append(db, tail)
    dr = eng.alloc_result(db2)
    try:
        eng.merge(db2, dr)
        logs = eng.download_logs(dr, 1)
        back = eng.download_batch(db2)
    finally:
        eng.free_result(dr)
        eng.free_batch(db2)
        eng.free_batch(db)
    assert int(logs["status"][0]) == 0 and int(logs["n_visible"][0]) == 70000
    assert (logs["digest"][0] == res.logs["digest"][0]).all()
    assert back.chg_env_hi is not None and (back.chg_seq == np.arange(1, 70002)).all()


@pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")
def test_patch_stream_change_and_cursors_on_long_documents(eng):
    """VERDICT r3 missing #1 / next #5: ptx_replay_patches, ptx_resolve_cursors and ptx_change on documents beyond the LDS merge kernel — a 40 000-op
    insert / delete document (25 000 list elements; merged by the HBM-staged kernel, which now emits the resolved references those entry points read) and a
    40 001-row all-marks log — through the C ABI, against the oracle: every Patch (reference/src/micromerge.ts:661-671, :696-703; peritext.ts:251-281),
    cursors both ways (:465-477), change(InputOperation[]) Change for Change (:308-441, :762-805), and the replica after the made Changes are appended."""
    essay = H.oracle_gen("config2", 1, 77, 40000, 1)["docs"][0]["logs"][0]
    marks = H.synthetic_marks_log(6000, 34000, 9)
    docs = [[essay], [marks]]
    exp = H.oracle_apply(docs, patches=True, timeout=1500)
    batch = wire.encode_docs(docs, extra_comments=[[], []])
    db = eng.upload(batch)
    dr = eng.alloc_result(db)
    made_db = after = dr2 = None
    try:
        eng.merge(db, dr)
        res = eng.download(db, dr)
        assert (res.logs["status"] == 0).all() and (res.logs["reserved"][:, 0] == 0).all()  # both took the HBM-staged kernel
        pat = eng.replay_patches(db, dr)
        assert (pat.logs["status"] == 0).all() and [int(x) for x in pat.logs["n_patches"]] == [len(exp[0][0]["patches"]), len(exp[1][0]["patches"])]
        H.check_patch_streams(batch, pat, exp)
        for log in (0, 1):
            V = int(res.logs["n_visible"][log])
            idx = list(range(0, V, 499)) + [V - 1]
            ids, st = eng.resolve_cursors(db, dr, [log] * len(idx), [abi.CURSOR_GET] * len(idx), idx)
            assert not st.any()
            d = batch.log_doc[log]
            assert [wire.get_cursor(batch, res, log, i) for i in idx[:8]] == ["%d@%s" % (int(x) >> 32, batch.doc_actors[d][int(x) & 0xFFFFFFFF]) for x in ids[:8]]
            back, st = eng.resolve_cursors(db, dr, [log] * len(idx), [abi.CURSOR_RESOLVE] * len(idx), [int(x) for x in ids])
            assert not st.any() and [int(x) for x in back] == idx
        V0, V1 = int(res.logs["n_visible"][0]), int(res.logs["n_visible"][1])
        calls = [[[{"path": ["text"], "action": "insert", "index": V0 // 2, "values": ["x", "y"]}, {"path": ["text"], "action": "delete", "index": 10, "count": 3}],
                  [{"path": ["text"], "action": "addMark", "markType": "strong", "startIndex": 5, "endIndex": V0 - 5}]],
                 [[{"path": ["text"], "action": "addMark", "markType": "link", "attrs": {"url": "https://long.example"}, "startIndex": 100, "endIndex": V1 - 100},
                   {"path": ["text"], "action": "insert", "index": V1, "values": ["!"]}]]]
        actors = [essay[0]["actor"], marks[0]["actor"]]
        want = H.oracle_change(docs, calls, actors)
        made_db, status = eng.change(db, dr, wire.encode_input_ops(batch, calls, actors))
        assert not status.any()
        made = eng.download_batch(made_db, batch.values, batch.urls, batch.log_doc, batch.doc_actors, batch.doc_comments, batch.keys, batch.map_values)
        got = []
        for log, logs in enumerate(docs):
            text_obj = [op["opId"] for c in logs[0] for op in c["ops"] if op["action"] == "makeList"][0]
            got += wire.decode_changes(made, log, text_obj=text_obj)
        assert got == want
        after = eng.append_device(db, made_db)
        dr2 = eng.alloc_result(after)
        eng.merge(after, dr2)
        logs2 = eng.download_logs(dr2, 2)
        assert (logs2["status"] == 0).all() and int(logs2["n_visible"][0]) == V0 + 2 - 3 and int(logs2["n_visible"][1]) == V1 + 1
    finally:
        for h in (dr2, dr):
            if h is not None:
                eng.free_result(h)
        for h in (after, made_db, db):
            if h is not None:
                eng.free_batch(h)


@pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")
def test_patch_stream_and_change_beyond_16_bit_ranks_slots_and_rows(eng):
    """VERDICT r5 missing #2 / next #6, GPU twin of the emulation test of the same name: ptx_replay_patches (the wide build, ptx_replay_kernel_wide) and ptx_change
    (29-bit rows in its list words, the list in global scratch where one CU's LDS cannot hold it) on a 36 000-character document with 1 500 deletes and 2 500
    mark ops of all four types and on a 70 000-op insert / delete essay (more than 65 534 rows and 32 766 elements) — through the C ABI, against the oracle:
    every Patch (reference/src/micromerge.ts:661-671, :696-703; peritext.ts:251-281), change(InputOperation[]) Change for Change (:308-441, :762-805;
    peritext.ts:458-501), and the replicas after the made Changes are appended and merged again."""
    marks = H.synthetic_marks_log(36000, 2500, 19, n_deletes=1500)
    essay = H.oracle_gen("config2", 1, 91, 70000, 1, mix=(80, 20, 0, 0))["docs"][0]["logs"][0]
    docs = [[marks], [essay]]
    exp = H.oracle_apply(docs, patches=True, timeout=2400)
    batch = wire.encode_docs(docs, extra_comments=[[], ["c-wide"]])
    assert int(batch.log_hdr["n_ins"][0]) > 32766 and int(batch.log_off[2] - batch.log_off[1]) > 65534
    db = eng.upload(batch)
    dr = eng.alloc_result(db)
    made_db = after = dr2 = None
    try:
        eng.merge(db, dr)
        res = eng.download(db, dr)
        assert (res.logs["status"] == 0).all()
        pat = eng.replay_patches(db, dr)
        assert (pat.logs["status"] == 0).all() and [int(x) for x in pat.logs["n_patches"]] == [len(exp[0][0]["patches"]), len(exp[1][0]["patches"])]
        H.check_patch_streams(batch, pat, exp)
        V0, V1 = int(res.logs["n_visible"][0]), int(res.logs["n_visible"][1])
        calls = [[[{"path": ["text"], "action": "addMark", "markType": "link", "attrs": {"url": "https://wide.example"}, "startIndex": V0 - 900, "endIndex": V0 - 3},
                   {"path": ["text"], "action": "insert", "index": V0 - 100, "values": ["w", "i", "d", "e"]}, {"path": ["text"], "action": "delete", "index": V0 - 50, "count": 4}],
                  [{"path": ["text"], "action": "addMark", "markType": "strong", "startIndex": 7, "endIndex": V0 - 1}, {"path": ["text"], "action": "insert", "index": V0, "values": ["!"]}]],
                 [[{"path": ["text"], "action": "insert", "index": V1 - 10, "values": ["x", "y"]}, {"path": ["text"], "action": "delete", "index": V1 // 2, "count": 3},
                   {"path": ["text"], "action": "addMark", "markType": "comment", "attrs": {"id": "c-wide"}, "startIndex": V1 - 2000, "endIndex": V1 - 1}]]]
        actors = [marks[0]["actor"], essay[0]["actor"]]
        want = H.oracle_change(docs, calls, actors)
        made_db, status = eng.change(db, dr, wire.encode_input_ops(batch, calls, actors))
        assert not status.any()
        made = eng.download_batch(made_db, batch.values, batch.urls, batch.log_doc, batch.doc_actors, batch.doc_comments, batch.keys, batch.map_values)
        got = []
        for log, logs in enumerate(docs):
            text_obj = [op["opId"] for c in logs[0] for op in c["ops"] if op["action"] == "makeList"][0]
            got += wire.decode_changes(made, log, text_obj=text_obj)
        assert got == want
        after = eng.append_device(db, made_db)
        dr2 = eng.alloc_result(after)
        eng.merge(after, dr2)
        logs2 = eng.download_logs(dr2, 2)
        assert (logs2["status"] == 0).all() and int(logs2["n_visible"][0]) == V0 + 4 - 4 + 1 and int(logs2["n_visible"][1]) == V1 + 2 - 3
        # the appended Changes' own patches (ptx_replay_patches_from): what an editor draws after its change() — against the oracle applying them
        rows0 = [int(batch.log_off[1] - batch.log_off[0]), int(batch.log_off[2] - batch.log_off[1])]
        pat2 = eng.replay_patches(after, dr2, first_row=rows0)
        assert (pat2.logs["status"] == 0).all() and (pat2.logs["n_patches"] > 0).all()
    finally:
        for h in (dr2, dr):
            if h is not None:
                eng.free_result(h)
        for h in (after, made_db, db):
            if h is not None:
                eng.free_batch(h)


@pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")
def test_cursors_on_a_document_beyond_16_bit_row_indices(eng):
    """VERDICT r4 missing #2 (cursors), GPU twin: getCursor / resolveCursor on a 70 000-op document (more than 65 534 rows and 32 766 elements; round 4:
    PTX_ERR_CAPACITY) through ptx_resolve_cursors — the long-document form of cursor_core.h (alive bitmap in LDS, one pass over the rows per query) beside an
    ordinary document of the same batch, against what the oracle's replica answers."""
    essay = H.oracle_gen("config2", 1, 91, 70000, 1, mix=(80, 20, 0, 0))
    small = _load("ptxgen_mini.json")
    docs = [[essay["docs"][0]["logs"][0]], small["docs"][0]["logs"]]
    batch = wire.encode_docs(docs)
    db = eng.upload(batch)
    dr = eng.alloc_result(db)
    try:
        eng.merge(db, dr)
        res = eng.download(db, dr)
        assert (res.logs["status"] == 0).all() and int(res.logs["n_elems"][0]) > 32766 and int(batch.log_off[1]) > 65534
        V = int(res.logs["n_visible"][0])
        exp = H.oracle_apply([docs[0]], cursors=True, no_patches=True, timeout=900)[0][0]
        idx = list(range(0, V, 1777)) + [V - 1]
        ids, st = eng.resolve_cursors(db, dr, [0] * len(idx) + [1], [abi.CURSOR_GET] * (len(idx) + 1), idx + [0])
        assert not st.any()
        assert ["%d@%s" % (int(x) >> 32, batch.doc_actors[0][int(x) & 0xFFFFFFFF]) for x in ids[:-1]] == [exp["cursorAt"][i] for i in idx]
        assert wire.get_cursor(batch, res, 1, 0) == "%d@%s" % (int(ids[-1]) >> 32, batch.doc_actors[1][int(ids[-1]) & 0xFFFFFFFF])  # the ordinary log: the indexed form
        elems = sorted(exp["cursorResolve"])[::997]
        args = [(int(e.split("@")[0]) << 32) | batch.doc_actors[0].index(e.split("@")[1]) for e in elems]
        back, st = eng.resolve_cursors(db, dr, [0] * len(args), [abi.CURSOR_RESOLVE] * len(args), args)
        assert not st.any() and [int(x) for x in back] == [exp["cursorResolve"][e] for e in elems]
        _, st = eng.resolve_cursors(db, dr, [0, 0], [abi.CURSOR_GET, abi.CURSOR_RESOLVE], [V, 999999 << 32])
        assert [int(x) for x in st] == [abi.ERR_INDEX_OOB, abi.ERR_ELEM_NOT_FOUND]
    finally:
        eng.free_result(dr)
        eng.free_batch(db)


@pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")
def test_comment_ids_with_thousands_of_ops_in_the_hbm_staged_kernels(eng):
    """Round 5: a comment id with more than PTX_BIG_COMMENT_OPS_PER_ID (1 024) ops that cover something is swept by the whole team (rounds 3-4: PTX_ERR_CAPACITY):
    a 16 501-row log (team of workgroups) whose 15 000 comment ops fall on five ids, two of them with ~6 600 ops each, against the oracle's intervals."""
    from test_emu_biglog import _one_comment_id_log

    docs = [[_one_comment_id_log(1500, 15000, 11, ("a", "b", "c", "d", "e"), (15, 1, 15, 1, 2))]]
    exp = H.oracle_apply(docs, no_patches=True, timeout=600)
    batch = wire.encode_docs(docs)
    res = eng.apply_materialize(batch)
    assert int(res.logs["status"][0]) == 0 and int(res.logs["reserved"][0, 0]) == 0  # (the HBM-staged kernel reports no LDS figure)
    H.check_log(batch, res, 0, exp[0][0])
