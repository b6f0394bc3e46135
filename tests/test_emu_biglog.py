"""Logs beyond one CU's LDS (VERDICT r2 "missing" #3): peritext_amd/csrc/biglog_core.h — the HBM-staged merge — on the CPU emulation.
The path is taken by size on the GPU; here EVERY log is forced through it, so the committed fixtures (made by the oracle / the type-erased
reference) check its logic in all three loop orders, the error cases check that it names the reference's error and the failing row exactly
like the LDS kernel, and two large documents (one insert/delete-heavy, one all-marks) that the LDS kernel refuses are compared with the
oracle.  Matches the unbounded arrays of reference/src/micromerge.ts:614-672."""
import copy
import dataclasses
import json
import os

import numpy as np
import pytest

import helpers as H
from peritext_amd import abi, wire

GOLDEN_GEN = ["ptxgen_mini.json", "ptxgen_config2.json", "ptxgen_config3_512.json", "ptxgen_config4_600.json", "ptxgen_rich_700.json", "ptxgen_rich_2600.json",
              "ptxgen_mini_10actors.json"]


def _load(name):
    with open(os.path.join(H.GOLDEN, name)) as f:
        return json.load(f)


@pytest.mark.parametrize("reverse", [0, 1, 2])
@pytest.mark.parametrize("name", GOLDEN_GEN)
def test_fixtures_through_the_hbm_staged_path(name, reverse):
    gen = _load(name)
    batch = wire.encode_docs([d["logs"] for d in gen["docs"]])
    for admission in (False, True):
        res = H.emu_merge_big(batch, reverse=reverse, admission=admission)
        log = 0
        for d in gen["docs"]:
            for exp in d["expected"]:
                H.check_log(batch, res, log, exp)
                log += 1
    small = H.emu_merge(batch, admission=True)
    for k in ("status", "n_ops", "n_elems", "n_visible", "n_spans", "n_cintervals", "digest"):
        assert (res.logs[k] == small.logs[k]).all(), k  # the two paths agree row for row, digest for digest
    # ... and on what the patch-stream replay, change() and the cursors read beside the result rows: document positions and resolved references
    assert (res.elem_rank == small.elem_rank).all() and (res.ref_slots == small.ref_slots).all()
    pb, ps = H.emu_replay(batch, res), H.emu_replay(batch, small)
    assert (pb.logs == ps.logs).all() and (pb.patches[: int(pb.patch_off[-1])] == ps.patches[: int(ps.patch_off[-1])]).all()


def test_reference_tests_traces_and_edge_cases_through_the_hbm_staged_path():
    """The reference's 46 test cases, its 9 traces and the SURVEY A.6 quirk documents: the HBM-staged path gives the rows the LDS kernel gives."""
    kat = _load("kat_reference_tests.json")
    docs = [[r["log"] for r in c["replicas"]] for c in kat["cases"]]
    docs += [t["logs"] for t in _load("reference_traces.json")]
    docs += H.edge_case_docs()
    batch = wire.encode_docs(docs)
    for reverse in (0, 2):
        big, small = H.emu_merge_big(batch, reverse=reverse), H.emu_merge(batch, reverse=reverse)
        for k in ("status", "n_visible", "n_spans", "n_cintervals", "digest"):
            assert (big.logs[k] == small.logs[k]).all(), k
        for log in range(batch.n_logs):
            assert wire.decode_spans(batch, big, log) == wire.decode_spans(batch, small, log)
    assert batch.n_logs > 100


@pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")
def test_errors_are_named_like_the_lds_kernel_and_the_reference():
    """Mutated logs (dropped / swapped / duplicated change, skipped seq, inflated dep, unknown element, double fault): status AND failing row equal the LDS
    kernel's, which the other suites pin against live oracle replays."""
    gen = _load("ptxgen_mini.json")
    base = gen["docs"][0]["logs"][1]

    def mutate(kind):
        log = copy.deepcopy(base)
        if kind == "drop":
            del log[3]
        elif kind == "swap":
            idx = [i for i, c in enumerate(log) if c["actor"] == log[-1]["actor"]]
            log[idx[-2]], log[idx[-1]] = log[idx[-1]], log[idx[-2]]
        elif kind == "seq_skip":
            log[5]["seq"] += 1
        elif kind == "dep_future":
            other = [a for a in {c["actor"] for c in log} if a != log[2]["actor"]][0]
            log[2]["deps"][other] = 10 ** 6
        elif kind == "unknown_elem":
            ins = [op for c in log for op in c["ops"] if op.get("insert")]
            ins[len(ins) // 2]["elemId"] = "999@zz"
        elif kind == "unknown_delete":
            dl = [op for c in log for op in c["ops"] if op["action"] == "del"]
            if dl:
                dl[0]["elemId"] = "998@zz"
        elif kind == "double_fault":
            del log[6]
            ins = [op for op in log[2]["ops"] if op.get("insert")]
            if ins:
                ins[0]["elemId"] = "999@zz"
        return log

    kinds = ["drop", "swap", "seq_skip", "dep_future", "unknown_elem", "unknown_delete", "double_fault", "intact"]
    logs = [mutate(k) for k in kinds]
    batch = wire.encode_docs([[l] for l in logs], extra_actors=[["zz"]] * len(logs))
    for admission in (False, True):
        for reverse in (0, 1):
            big, small = H.emu_merge_big(batch, reverse=reverse, admission=admission), H.emu_merge(batch, reverse=reverse, admission=admission)
            assert [int(x) for x in big.logs["status"]] == [int(x) for x in small.logs["status"]], (admission, reverse)
            assert [int(x) for x in big.logs["reserved"][:, 1]] == [int(x) for x in small.logs["reserved"][:, 1]], (admission, reverse)
    assert int(small.logs["status"][-1]) == 0 and int((small.logs["status"] != 0).sum()) >= 5
    exp = H.oracle_apply([[l] for l in logs])
    for k, e, st in zip(kinds, exp, big.logs["status"]):
        assert (int(st) != 0) == ("error" in e[0]), k


def test_capacity_and_lying_headers():
    gen = _load("ptxgen_config4_600.json")
    batch = wire.encode_docs([gen["docs"][0]["logs"]])
    res = H.emu_merge_big(batch, slack=-4096)  # a slice too small for the working set: the log reports it, nothing is written past the slice
    assert (res.logs["status"] == abi.ERR_CAPACITY).all()
    bad = wire.encode_docs([gen["docs"][0]["logs"]])
    bad.log_hdr = bad.log_hdr.copy()
    bad.log_hdr["n_ins"][0] -= 1  # the header understates the inserts: BAD_OP at row 0, never a wrong result
    r = H.emu_merge_big(bad, slack=1 << 16)
    assert int(r.logs["status"][0]) == abi.ERR_BAD_OP and (r.logs["status"][1:] == 0).all()


@pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")
def test_large_documents_against_the_oracle():
    """A 40 000-op insert/delete document (25 000 list elements: the LDS kernel, given a whole CU, reports PTX_ERR_CAPACITY) and a
    mark-heavy one, through the HBM-staged path against the oracle.  (The GPU suite repeats it at 100 000 / 20 000 ops: tests/test_gpu_biglog.py;
    the oracle needs a minute to GENERATE each of those, too long for this suite.)"""
    essay = H.oracle_gen("config2", 1, 77, 40000, 1)
    marks = H.oracle_gen("config3", 1, 78, 5000, 1, mix=(8, 2, 60, 30), marks=("strong", "em", "link", "comment"))
    b1 = wire.encode_docs([d["logs"] for d in essay["docs"]])
    assert int(b1.log_hdr["n_ins"][0]) > 20000  # 12 bytes of LDS per element and more: far beyond the 160 KB of a CU
    assert int(H.emu_merge(b1, lds_bytes=160 * 1024).logs["status"][0]) == abi.ERR_CAPACITY
    r1 = H.emu_merge_big(b1, admission=True)
    H.check_log(b1, r1, 0, essay["docs"][0]["expected"][0])
    b2 = wire.encode_docs([d["logs"] for d in marks["docs"]])
    for reverse in (0, 2):
        r2 = H.emu_merge_big(b2, reverse=reverse, admission=True)
        H.check_log(b2, r2, 0, marks["docs"][0]["expected"][0])
    assert (H.emu_merge(b2, lds_bytes=160 * 1024, admission=True).logs["digest"] == r2.logs["digest"]).all()


@pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")
def test_all_marks_document_of_20000_ops():
    """a 20 000-op all-marks document (4 000 characters, 16 000 add / removeMark ops of the four types, 400 comment ids): built without
    the generator (helpers.synthetic_marks_log), expected output from the oracle's applyChange; """
    log = H.synthetic_marks_log(4000, 16000, 5)
    exp = H.oracle_apply([[log]], no_patches=True)[0][0]
    batch = wire.encode_docs([[log]])
    assert batch.n_ops == 20001
    res = H.emu_merge_big(batch, admission=True)
    H.check_log(batch, res, 0, exp)
    small = H.emu_merge(batch, lds_bytes=160 * 1024, admission=True)  # (a whole CU's LDS just holds this one: 140 KB; the library's launch would give it a CU to itself)
    assert int(small.logs["status"][0]) in (0, abi.ERR_CAPACITY)
    if int(small.logs["status"][0]) == 0:
        assert (small.logs["digest"] == res.logs["digest"]).all()
    assert int(res.logs["n_cintervals"][0]) > 50 and int(res.logs["n_spans"][0]) > 200


# ---- seq / deps beyond 16 bits: the wide envelope column ----
def _typed_log(n_changes, actor="a", first_ctr=1, make_list=True, deps_of=None, seq0=1):
    """One change per keystroke (what bridge.ts:535 produces): change 1 makes the list, every further one inserts one character at the head
    (cheap for the reference: no element search).  deps_of(k) -> deps of the k-th change."""
    log, ctr = [], first_ctr
    for k in range(n_changes):
        if k == 0 and make_list:
            ops = [{"opId": "%d@%s" % (ctr, actor), "action": "makeList", "obj": "_root", "key": "text"}]
        else:
            ops = [{"opId": "%d@%s" % (ctr, actor), "action": "set", "obj": "1@a", "elemId": "_head", "insert": True, "value": chr(97 + k % 26)}]
        log.append({"actor": actor, "seq": seq0 + k, "deps": deps_of(k) if deps_of else {}, "startOp": ctr, "ops": ops})
        ctr += 1
    return log


def wide_envelope_docs(only=None):
    """(i) 70 001 one-op changes of one actor; (ii) two actors, the second one's deps cross 65 535 — valid, and with a dependency one too far;
    (iii) a genuine sequence gap past change 65 535; (iv) the same sequence number twice past 65 535.  `only`: just these documents."""
    want = lambda k: only is None or k in only  # noqa: E731
    out = {}
    single = _typed_log(70001) if any(want(k) for k in ("single", "seq_gap", "seq_twice")) else None
    if want("single"):
        out["single"] = [single]
    if want("deps_cross") or want("dep_missing"):
        a_part = _typed_log(66000)
        b_ok = _typed_log(3, actor="b", first_ctr=66001, make_list=False, deps_of=lambda k: {"a": 66000})
        if want("deps_cross"):
            out["deps_cross"] = [a_part + b_ok]
        if want("dep_missing"):
            b_far = copy.deepcopy(b_ok)
            b_far[1]["deps"] = {"a": 66001}
            out["dep_missing"] = [a_part + b_far]
    if want("seq_gap"):
        gap = [dict(ch) for ch in single[:66010]]
        for ch in gap[66000:]:
            ch["seq"] += 1
        out["seq_gap"] = [gap]
    if want("seq_twice"):
        twice = [dict(ch) for ch in single[:66010]]
        twice[66005]["seq"] = twice[66004]["seq"]
        out["seq_twice"] = [twice]
    return out


def wide_envelope_expected(docs):
    """The type-erased reference's answers for wide_envelope_docs() (whole logs, no patches), per document in `docs` order: the committed fixture,
    refused if it was made for other logs."""
    g = H.wide_envelope_golden()
    assert g["apply_sha16"] == H.inputs_sha16(docs), "tests/golden/wide_envelope_ref.json.gz was made for other logs: rerun tests/make_wide_envelope_golden.py"
    return [g["apply"][k] for k in docs]


def test_logs_with_more_than_65535_changes_against_the_reference():
    """A valid log typed as one change per keystroke passes 65 535 changes of one actor (reference/src/micromerge.ts:499-511 takes plain numbers).
    The encoders then emit the wide envelope column and the HBM-staged kernel admits every change; failing logs past 65 535 still name the
    reference's error and the row it throws at; without the column such a log is PTX_ERR_CAPACITY, never a spurious sequence gap."""
    docs = wide_envelope_docs()
    names = list(docs)
    batch = wire.encode_docs([docs[k] for k in names])
    assert batch.chg_env_hi is not None and int(batch.chg_seq.max()) == 70001
    exp = wide_envelope_expected(docs)
    for reverse in (0, 1):
        res = H.emu_merge_big(batch, reverse=reverse, admission=True)
        for log, k in enumerate(names):
            e = exp[log][0]
            st, row = int(res.logs["status"][log]), int(res.logs["reserved"][log, 1])
            if k in ("single", "deps_cross"):
                assert "error" not in e and st == 0, (k, st, row)
                H.check_log(batch, res, log, e)
            elif k == "dep_missing":
                assert "Missing dependency" in e["error"] and st == abi.ERR_MISSING_DEP and row == 66001, (k, st, row, e["error"])
            else:
                assert "Expected sequence number" in e["error"] and st == abi.ERR_SEQ_GAP and row == (66000 if k == "seq_gap" else 66005), (k, st, row, e["error"])
    assert int(res.logs["n_visible"][0]) == 70000
    # the same batch without the wide column (what an ABI-5 encoder would have sent: values saturated at 65 535): not representable
    es = abi.env_stride(batch.max_actors)
    sat = np.minimum(batch.chg_seq.astype(np.uint64), 65535)
    narrow = dataclasses.replace(batch, chg_env=batch.chg_env.copy(), chg_env_hi=None)
    narrow.chg_env.reshape(-1, es)[:, 0] = sat.astype(np.uint16)
    r = H.emu_merge_big(narrow, admission=True)
    assert (r.logs["status"] == abi.ERR_CAPACITY).all()
    # without admission nothing reads the envelope
    assert (H.emu_merge_big(narrow, admission=False).logs["status"] == 0).all()


@pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")
def test_long_log_of_several_actors_whose_values_stay_narrow():
    """two actors x 33 000 one-op changes = 66 000 changes whose every seq / dep is below 65 535.  The encoders emit NO wide column
    for it (no value needs one) and the census sends it to the HBM-staged kernel (more than 65 533 changes): narrow values that never touch the
    sentinel are exact, so the log is admitted like the reference admits it — round 4 answered PTX_ERR_CAPACITY.  The same log with one dependency too
    far still names the reference's error and row."""
    a = _typed_log(33000)
    b = _typed_log(33000, actor="b", first_ctr=33001, make_list=False, deps_of=lambda k: {"a": 33000})
    far = copy.deepcopy(b)
    far[10]["deps"] = {"a": 33001}
    docs = [[a + b], [a + far]]
    batch = wire.encode_docs(docs)
    assert batch.chg_env_hi is None and int(batch.chg_seq.max()) == 33000 and int(batch.chg_off[1]) == 66000
    exp = H.oracle_apply(docs, no_patches=True, timeout=900)
    for reverse in (0, 2):
        res = H.emu_merge_big(batch, reverse=reverse, admission=True)
        assert "error" not in exp[0][0] and int(res.logs["status"][0]) == 0
        H.check_log(batch, res, 0, exp[0][0])
        assert "Missing dependency" in exp[1][0]["error"] and int(res.logs["status"][1]) == abi.ERR_MISSING_DEP and int(res.logs["reserved"][1, 1]) == 33010
    assert int(res.logs["n_visible"][0]) == 65999


@pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")
def test_patch_stream_change_and_cursors_on_a_40000_op_document():
    """VERDICT r3 missing #1: the editor-facing half on a long document.  The HBM-staged merge now also emits the resolved references the replay / change() /
    cursors read (row of a delete's target, boundary slots of a mark op), so a 40 000-op document (25 000 list elements, a fifth of them visible) gets its
    Patch[] stream (reference/src/micromerge.ts:661-671, :696-703), getCursor / resolveCursor (:465-477) and change(InputOperation[]) (:308-441, :762-805)
    from one CU's LDS — against the oracle.  Beyond the on-chip kernels' 16-bit indices (32 766 elements, 65 534 rows) they still report PTX_ERR_CAPACITY."""
    essay = H.oracle_gen("config2", 1, 77, 40000, 1)
    log = essay["docs"][0]["logs"][0]
    batch = wire.encode_docs([[log]])
    res = H.emu_merge_big(batch, admission=True)
    assert int(res.logs["status"][0]) == 0 and int(res.logs["n_elems"][0]) > 20000
    exp = H.oracle_apply([[log]], patches=True, timeout=900)[0][0]
    pat = H.emu_replay(batch, res, gwin=True)
    assert int(pat.logs["status"][0]) == 0 and int(pat.logs["n_patches"][0]) == len(exp["patches"])
    H.check_patch_streams(batch, pat, [[exp]])
    V = int(res.logs["n_visible"][0])
    idx = list(range(0, V, 499)) + [V - 1]
    ids, st = H.emu_cursors(batch, res, [0] * len(idx), [abi.CURSOR_GET] * len(idx), idx, lds_bytes=160 * 1024)
    assert not st.any() and [wire.get_cursor(batch, res, 0, i) for i in idx[:8]] == ["%d@%s" % (int(x) >> 32, batch.doc_actors[0][int(x) & 0xFFFFFFFF]) for x in ids[:8]]
    back, st = H.emu_cursors(batch, res, [0] * len(idx), [abi.CURSOR_RESOLVE] * len(idx), [int(x) for x in ids], lds_bytes=160 * 1024)
    assert not st.any() and [int(x) for x in back] == idx
    _, st = H.emu_cursors(batch, res, [0], [abi.CURSOR_GET], [V], lds_bytes=160 * 1024)
    assert int(st[0]) == abi.ERR_INDEX_OOB
    calls = [[[{"path": ["text"], "action": "insert", "index": V // 2, "values": ["x", "y"]}, {"path": ["text"], "action": "delete", "index": 10, "count": 3}],
              [{"path": ["text"], "action": "addMark", "markType": "strong", "startIndex": 5, "endIndex": V - 5}]]]
    actor = log[0]["actor"]
    made, status = H.emu_change(batch, res, wire.encode_input_ops(batch, calls, [actor]), lds_bytes=160 * 1024)
    assert int(status[0]) == 0
    text_obj = [op["opId"] for c in log for op in c["ops"] if op["action"] == "makeList"][0]
    assert wire.decode_changes(made, 0, text_obj=text_obj) == H.oracle_change([[log]], calls, [actor])


@pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")
def test_cursors_on_a_document_beyond_16_bit_row_indices():
    """VERDICT r4 missing #2 (cursors): a 70 000-op insert / delete document (more than 65 534 rows, more than 32 766 elements) — getCursor / resolveCursor
    (reference/src/micromerge.ts:465-477 have no bound) through the long-document form of cursor_core.h, against what the oracle's replica answers."""
    essay = H.oracle_gen("config2", 1, 91, 70000, 1, mix=(80, 20, 0, 0))
    log = essay["docs"][0]["logs"][0]
    batch = wire.encode_docs([[log]])
    assert batch.n_ops > 65534
    res = H.emu_merge_big(batch, admission=True)
    assert int(res.logs["status"][0]) == 0 and int(res.logs["n_elems"][0]) > 32766
    V = int(res.logs["n_visible"][0])
    exp = H.oracle_apply([[log]], cursors=True, no_patches=True, timeout=900)[0][0]
    idx = list(range(0, V, 1777)) + [V - 1]
    ids, st = H.emu_cursors(batch, res, [0] * len(idx), [abi.CURSOR_GET] * len(idx), idx, lds_bytes=160 * 1024)
    assert not st.any()
    got = ["%d@%s" % (int(x) >> 32, batch.doc_actors[0][int(x) & 0xFFFFFFFF]) for x in ids]
    assert got == [exp["cursorAt"][i] for i in idx]
    elems = sorted(exp["cursorResolve"])[::997]
    args = [(int(e.split("@")[0]) << 32) | batch.doc_actors[0].index(e.split("@")[1]) for e in elems]
    back, st = H.emu_cursors(batch, res, [0] * len(args), [abi.CURSOR_RESOLVE] * len(args), args, lds_bytes=160 * 1024, reverse=2)
    assert not st.any() and [int(x) for x in back] == [exp["cursorResolve"][e] for e in elems]
    _, st = H.emu_cursors(batch, res, [0, 0], [abi.CURSOR_GET, abi.CURSOR_RESOLVE], [V, (999999 << 32)], lds_bytes=160 * 1024)
    assert [int(x) for x in st] == [abi.ERR_INDEX_OOB, abi.ERR_ELEM_NOT_FOUND]


@pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")
def test_patch_stream_and_change_beyond_16_bit_ranks_slots_and_rows():
    """VERDICT r5 missing #2 / next #6: `applyChange`'s patches (reference/src/micromerge.ts:499-514, :661-671, :696-703; peritext.ts:154-220, :251-281) and
    `change()` (:308-441, :762-805; peritext.ts:458-501) have no size limit; round 5's replay and change kernels stopped at 32 766 list elements / 65 534 rows
    (16-bit ranks and boundary slots).  Round 6: the HBM-staged merge hands the slots' high halves over (out_refs_hi), the replay has a wide build
    (ptx_replay_log<.., kWide>) and change()'s list words hold 29-bit rows, its list in global scratch where the LDS cannot hold it.  Two documents against the
    oracle: a 36 000-character text with 1 500 deletes and 2 500 mark ops of all four types (slots beyond 16 bits on every path), and a 70 000-op insert / delete
    essay (more than 65 534 rows AND 32 766 elements; its 50 000-element list does not fit one CU's LDS in change())."""
    marks = H.synthetic_marks_log(36000, 2500, 19, n_deletes=1500)
    essay = H.oracle_gen("config2", 1, 91, 70000, 1, mix=(80, 20, 0, 0))["docs"][0]["logs"][0]
    docs = [[marks], [essay]]
    batch = wire.encode_docs(docs, extra_comments=[[], ["c-wide"]])  # (the comment id a later change() introduces takes part in the document's id ranks)
    assert int(batch.log_hdr["n_ins"][0]) > 32766 and int(batch.log_off[2] - batch.log_off[1]) > 65534
    res = H.emu_merge_big(batch, admission=True)
    assert (res.logs["status"] == 0).all()
    exp = H.oracle_apply(docs, patches=True, timeout=2400)
    pat = H.emu_replay(batch, res)
    assert (pat.logs["status"] == 0).all() and [int(x) for x in pat.logs["n_patches"]] == [len(exp[0][0]["patches"]), len(exp[1][0]["patches"])]
    H.check_patch_streams(batch, pat, exp)
    pat2 = H.emu_replay(batch, res, reverse=1)  # (the other lane order)
    assert pat2.patches[: int(pat2.patch_off[-1])].tobytes() == pat.patches[: int(pat.patch_off[-1])].tobytes()
    # change(): marks whose boundaries lie beyond slot 65 535, inserts after tombstones, deletes — Change for Change
    V0, V1 = int(res.logs["n_visible"][0]), int(res.logs["n_visible"][1])
    calls = [[[{"path": ["text"], "action": "addMark", "markType": "link", "attrs": {"url": "https://wide.example"}, "startIndex": V0 - 900, "endIndex": V0 - 3},
               {"path": ["text"], "action": "insert", "index": V0 - 100, "values": ["w", "i", "d", "e"]}, {"path": ["text"], "action": "delete", "index": V0 - 50, "count": 4}],
              [{"path": ["text"], "action": "addMark", "markType": "strong", "startIndex": 7, "endIndex": V0 - 1}, {"path": ["text"], "action": "insert", "index": V0, "values": ["!"]}]],
             [[{"path": ["text"], "action": "insert", "index": V1 - 10, "values": ["x", "y"]}, {"path": ["text"], "action": "delete", "index": V1 // 2, "count": 3},
               {"path": ["text"], "action": "addMark", "markType": "comment", "attrs": {"id": "c-wide"}, "startIndex": V1 - 2000, "endIndex": V1 - 1}]]]
    actors = [marks[0]["actor"], essay[0]["actor"]]
    want = H.oracle_change(docs, calls, actors)
    made, status = H.emu_change(batch, res, wire.encode_input_ops(batch, calls, actors), lds_bytes=160 * 1024)
    assert not status.any()
    got = []
    for log, logs in enumerate(docs):
        text_obj = [op["opId"] for c in logs[0] for op in c["ops"] if op["action"] == "makeList"][0]
        got += wire.decode_changes(made, log, text_obj=text_obj)
    assert got == want
    # a result WITHOUT the high halves (allocated for another batch): such a log reports capacity, as before the round — never a wrong stream
    res.ref_slots_hi = None
    pat3 = H.emu_replay(batch, res)
    assert [int(x) for x in pat3.logs["status"]] == [abi.ERR_CAPACITY, abi.ERR_CAPACITY]
    _, status = H.emu_change(batch, res, wire.encode_input_ops(batch, calls, actors), lds_bytes=160 * 1024)
    assert int(status[0]) == abi.ERR_CAPACITY


def _one_comment_id_log(n_chars, n_ops, seed, ids_of_ops=("the-one",), weights=None):
    """A replica log whose n_ops comment ops carry few ids (the HBM-staged path sweeps an id's ops in one lane, quadratic in their number, or — beyond 1 024 — as a team)."""
    import random

    rnd = random.Random(seed)
    ids = ["%d@doc1" % (2 + i) for i in range(n_chars)]
    ops = [{"opId": "1@doc1", "action": "makeList", "obj": "_root", "key": "text"}]
    for i in range(n_chars):
        ops.append({"opId": ids[i], "action": "set", "obj": "1@doc1", "elemId": "_head" if i == 0 else ids[i - 1], "insert": True, "value": "x"})
    changes = [{"actor": "doc1", "seq": 1, "deps": {}, "startOp": 1, "ops": ops}]
    ctr = n_chars + 2
    for k in range(n_ops):
        a = rnd.randrange(n_chars)
        e = a + 1 + rnd.randrange(min(n_chars - a, 1 + n_chars // 6))
        cid = rnd.choices(ids_of_ops, weights)[0]
        op = {"opId": "%d@doc1" % ctr, "action": "addMark" if rnd.random() < 0.6 else "removeMark", "obj": "1@doc1", "markType": "comment", "attrs": {"id": cid},
              "start": {"type": "before", "elemId": ids[a]}, "end": {"type": "after", "elemId": ids[e - 1]}}
        changes.append({"actor": "doc1", "seq": 2 + k, "deps": {}, "startOp": ctr, "ops": [op]})
        ctr += 1
    return changes


@pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")
def test_comment_ops_on_one_id_beyond_one_lanes_sweep_in_the_hbm_staged_path():
    """ADVICE r3 bounded the per-id comment sweep (quadratic, one lane) at PTX_BIG_COMMENT_OPS_PER_ID = 1 024 ops with a visible interval per id; round 5 sweeps an id
    with more as a team (range-chmax tree of the application index over the visible positions, presence bitmap, runs of ones): 900, 1 300 and 3 000 ops on one id
    and a log with two heavy and three light ids all equal the oracle's intervals, in each of the emulation's loop orders."""
    docs = [[_one_comment_id_log(60, 900, 3)], [_one_comment_id_log(60, 1300, 4)], [_one_comment_id_log(200, 3000, 5)],
            [_one_comment_id_log(333, 4200, 6, ("a", "b", "c", "d", "e"), (8, 1, 10, 1, 1))]]
    expected = H.oracle_apply(docs)
    batch = wire.encode_docs(docs)
    for kw in ({}, {"reverse": 1}, {"reverse": 2}):
        res = H.emu_merge_big(batch, **kw)
        assert not res.logs["status"].any(), res.logs["status"]
        for d in range(len(docs)):
            H.check_log(batch, res, d, expected[d][0])
    assert int(H.emu_merge(batch, lds_bytes=160 * 1024).logs["status"][1]) == 0  # (the LDS kernel, whose LDS bounds the ops of a log, sweeps every id in a lane)


def test_team_sweep_of_heavy_comment_ids_equals_the_lds_kernels_lane_sweep_on_random_logs():
    """The HBM-staged kernel's team sweep (ids with more than 1 024 covering ops: range-chmax tree + presence bitmap) against the LDS kernel's per-lane sweep of the
    same log — two implementations of peritext.ts:314-321 over one set of inputs: rows, counts and digests equal on ten random logs of one to four ids, 1 100 to
    2 600 comment ops, short and long ranges (no oracle needed: the LDS kernel's sweep is the one every other comment test pins against it)."""
    import random

    heavy_logs = 0
    for seed in range(10):
        rnd = random.Random(1000 + seed)
        n_chars = rnd.choice([40, 97, 160, 333])
        n_ops = rnd.randrange(1100, 2600)
        ids = tuple("c%d" % i for i in range(rnd.randrange(1, 5)))
        weights = tuple(rnd.choice([1, 2, 9]) for _ in ids)
        log = _one_comment_id_log(n_chars, n_ops, seed, ids, weights)
        per_id = {}
        for ch in log[1:]:
            per_id[ch["ops"][0]["attrs"]["id"]] = per_id.get(ch["ops"][0]["attrs"]["id"], 0) + 1
        heavy_logs += max(per_id.values()) > 1024
        batch = wire.encode_docs([[log]])
        small = H.emu_merge(batch, lds_bytes=160 * 1024)
        big = H.emu_merge_big(batch, reverse=seed % 3)
        assert int(small.logs["status"][0]) == 0 and int(big.logs["status"][0]) == 0
        for f in ("n_visible", "n_spans", "n_cintervals"):
            assert int(small.logs[f][0]) == int(big.logs[f][0]), (seed, f)
        assert (small.logs["digest"][0] == big.logs["digest"][0]).all(), seed
        k = int(big.logs["n_cintervals"][0])
        assert np.array_equal(small.cintervals[:k], big.cintervals[:k]) and np.array_equal(small.spans[:int(big.logs["n_spans"][0])], big.spans[:int(big.logs["n_spans"][0])])
    assert heavy_logs >= 5, heavy_logs
