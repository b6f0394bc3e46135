"""The merge kernel's admission marks (merge_core.h ptx_adm_mark) through the host emulation, no GPU: three-actor logs are merged, grown, and merged again with
the marks of the first merge — the walk then starts at the mark (or is skipped).  Status, error code, error row and result rows of every grown log must be the
oracle's for the WHOLE log, wherever the mark stands (0, 1, C - 1, C) and however long the appended part is (1, 255, 256, 257, 768, 769 changes), whether it is
intact, skips a seq, repeats one or depends on a change the log does not hold."""
import ctypes as C
import os

import numpy as np
import pytest

import adm_mark_cases as M
import helpers as H
from peritext_amd import abi, wire

LIB = os.path.join(H.ROOT, "tests", "emu", "libperitext_emu_marks.so")


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    assert H.have_node(), "these cases need node, the oracle's runtime: a skipped case would hide exactly what this file exists to show"


def merge_marks(b, marks, reverse=0, lean=False):
    """ptx_emu_merge_marks over a wire.Batch; marks: uint32 [n_logs, 4], updated in place (None: no marks, every change walked)."""
    lib = C.CDLL(LIB)
    n = max(b.n_ops, 1)
    res = wire.Results(
        logs=np.zeros(b.n_logs, dtype=abi.LOG_RESULT_DTYPE),
        values=np.full(n, 0xDEADBEEF, dtype=np.uint32),
        spans=np.zeros(n, dtype=abi.SPAN_DTYPE),
        cintervals=np.zeros(n, dtype=abi.CINTERVAL_DTYPE),
        elem_rank=None if lean else np.zeros(n, dtype=np.uint32),
        ref_slots=None if lean else np.full(n, 0xFFFFFFFF, dtype=np.uint32),
    )
    s = H.batch_struct(b)
    f = lib.ptx_emu_merge_marks
    f.restype = C.c_int
    f.argtypes = [C.POINTER(abi.ptx_batch)] + [C.c_void_p] * 7 + [C.c_uint32, C.c_int, C.c_int]
    rc = f(C.byref(s), res.logs.ctypes.data, res.values.ctypes.data, res.spans.ctypes.data, res.cintervals.ctypes.data,
           None if lean else res.elem_rank.ctypes.data, None if lean else res.ref_slots.ctypes.data, None if marks is None else marks.ctypes.data,
           H.LDS_BYTES, reverse, 1 if lean else 0)
    assert rc == 0
    return res


def exact_walks():
    f = C.CDLL(LIB).ptx_emu_marks_exact_walk_count
    f.restype = C.c_ulonglong
    return int(f())


def same_results(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("logs", "values", "spans", "cintervals"))


@pytest.mark.parametrize("reverse,lean", [(0, False), (1, True), (2, False)])
def test_grown_logs_walk_from_their_mark_and_answer_like_the_oracle(reverse, lean):
    cs = M.cases(1400)
    base, grown, cases = cs["base"], cs["grown"], cs["cases"]
    assert {c["s"] for c in cases} >= set(M.SUFFIXES) and {c["m"] for c in cases} >= {0, 1}
    assert any(c["m"] + c["s"] == int(grown.chg_off[l + 1] - grown.chg_off[l]) and c["s"] == 1 for l, c in enumerate(cases))  # mark position C - 1
    marks = np.zeros((base.n_logs, 4), dtype=np.uint32)
    # 1. the bases: what passes leaves its record {changes, rows, clock}, what fails (or is empty) leaves none
    rb = merge_marks(base, marks, reverse, lean)
    for l, c in enumerate(cases):
        ok = c["kind"] != "bad_base"
        assert (int(rb.logs["status"][l]) == 0) == ok, c
        assert marks[l].tolist() == (M.clock_record(base, l) if ok and c["m"] else [0, 0, 0, 0]), (c, marks[l])
    assert same_results(rb, merge_marks(base, marks.copy(), reverse, lean)), "a marked log's result row (its LDS high-water mark included) is the same in every launch"
    for l, c in enumerate(cases):
        if not c["merged"]:
            marks[l] = 0  # (this base is appended to before any merge has seen it)
    # 2. the grown logs, walked from the marks their bases left (what an append hands over)
    before = marks.copy()
    walks = exact_walks()
    rg = merge_marks(grown, marks, reverse, lean)
    n_bad = sum(1 for c in cases if c["code"])
    assert exact_walks() - walks == n_bad, "the exact walk runs for the failing logs and only for them"
    for l, c in enumerate(cases):
        M.check_grown(c, grown, rg, l)
        # a log that passes is marked whole; one that fails writes nothing
        assert marks[l].tolist() == (before[l].tolist() if c["code"] else M.clock_record(grown, l)), (c, marks[l], before[l])
    # 3. mark position C: merged again, no valid log is walked at all; the failing ones fail again, bit for bit
    again = marks.copy()
    r3 = merge_marks(grown, again, reverse, lean)
    assert same_results(rg, r3) and np.array_equal(again, marks)
    assert exact_walks() - walks == 2 * n_bad
    # ... and the same as a merge that knows no marks
    assert same_results(rg, merge_marks(grown, None, reverse, lean))


def test_a_record_that_does_not_fit_the_log_is_ignored():
    """changes_admitted > C, or rows beyond the log's: walked from 0 as if there were no record (and then marked properly)."""
    cs = M.cases(1400)
    grown, cases = cs["grown"], cs["cases"]
    marks = np.zeros((grown.n_logs, 4), dtype=np.uint32)
    for l in range(grown.n_logs):
        C_, N_ = int(grown.chg_off[l + 1] - grown.chg_off[l]), int(grown.log_off[l + 1] - grown.log_off[l])
        marks[l] = [C_ + 1 + l, N_, 7, 7] if l % 2 else [max(C_ - 1, 1), N_ + 5, 7, 7]
    res = merge_marks(grown, marks)
    for l, c in enumerate(cases):
        M.check_grown(c, grown, res, l)
        if not c["code"]:
            assert marks[l].tolist() == M.clock_record(grown, l)


@pytest.mark.parametrize("replicas", [5, 9, 16])
def test_many_actor_marks_say_all_or_nothing(replicas):
    """Documents of more than three actors (the one-pass walks over wider rows up to fifteen actors, the (actor, seq) table beyond): a log that passes is marked
    {C, N, 0, 0} and not walked again — the same result rows, LDS high-water mark included, and the oracle's; a grown log (a record of fewer changes) is walked
    from 0; a log that fails is never marked."""
    import copy

    gen = H.oracle_gen("mini", 1, 40 + replicas, 300, replicas)
    logs = list(gen["docs"][0]["logs"])
    expected = list(gen["docs"][0]["expected"])
    broken = copy.deepcopy(logs[-1])
    broken[5]["seq"] += 1
    assert M._code(H.oracle_apply([[broken]], no_patches=True)[0][0]) == abi.ERR_SEQ_GAP  # (the oracle's own verdict)
    logs[-1] = broken
    batch = wire.encode_docs([logs])
    assert batch.max_actors == replicas
    bad = batch.n_logs - 1
    marks = np.zeros((batch.n_logs, 4), dtype=np.uint32)
    marks[0] = [3, 3, 0, 0]  # (as if an append had handed over a shorter log's record: no suffix form here)
    r1 = merge_marks(batch, marks)
    for l in range(batch.n_logs):
        C_, N_ = int(batch.chg_off[l + 1] - batch.chg_off[l]), int(batch.log_off[l + 1] - batch.log_off[l])
        if l == bad:
            assert int(r1.logs["status"][l]) == abi.ERR_SEQ_GAP and marks[l].tolist() == [0, 0, 0, 0]
        else:
            H.check_log(batch, r1, l, expected[l])
            assert marks[l].tolist() == [C_, N_, 0, 0]
    kept = marks.copy()
    assert same_results(r1, merge_marks(batch, marks)) and np.array_equal(kept, marks)
    assert same_results(r1, merge_marks(batch, None))
