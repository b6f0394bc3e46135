"""Text and span rows of element ranges through the C ABI on a real MI355X (ptx_strings_upload -> ptx_merge -> ptx_result_text_slices): the cases of
tests/test_emu_slices.py with the expected values of tests/slice_cases.py (plain Python slices of the oracle's text, the oracle's spans cut by a plain loop), on a
default context and on a PTX_FLAG_NO_ELEM_RANK one; one batch generated on the device in the `rich4k` mix against Python slices of Engine.text's download of the
same result; find -> windows -> snippets; and the text of every comment against the oracle."""
import ctypes as C
import random

import numpy as np
import pytest

import find_cases as FC
import helpers as H
import slice_cases as SC
import text_cases as TC
from peritext_amd import abi, wire, workloads

pytestmark = pytest.mark.gpu


def _engine(flags):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from peritext_amd.engine import Engine

    return Engine(0, flags=flags)


@pytest.fixture(scope="module")
def eng():
    e = _engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_lean():
    e = _engine(abi.FLAG_NO_ELEM_RANK)
    yield e
    e.close()


class Resident:
    """A batch, its merge and a string table on the device."""

    def __init__(self, eng, batch, table):
        self.eng = eng
        self.db = eng.upload(batch)
        self.dr = eng.alloc_result(self.db)
        self.ds = eng.upload_strings(table)
        eng.merge(self.db, self.dr)

    def slices(self, plan, first, n):
        return self.eng.text_slices(self.db, self.dr, self.ds, plan, first, n)

    def close(self):
        self.eng.free_strings(self.ds)
        self.eng.free_result(self.dr)
        self.eng.free_batch(self.db)


def run_plan(r, suite, make_plan, first=0, n=None, decode=True):
    n = suite.batch.n_logs - first if n is None else n
    rows = r.eng.download_range(r.db, r.dr, first, n)
    plan = make_plan(rows, n)
    got = r.slices(plan, first, n)
    SC.check_range(suite, rows, got, first, n, plan, decode=decode)
    return rows, plan, got


def _suites(e):
    """Every suite of the emulation tests on one engine."""
    suite, _ = SC.edge_suite()
    r = Resident(e, suite.batch, suite.table)
    try:
        _, _, got = run_plan(r, suite, lambda rows, n: SC.edge_plan_list())
        SC.edge_hand_checks(got)
    finally:
        r.close()
    suite = TC.edge_suite()
    r = Resident(e, suite.batch, suite.table)
    try:
        _, plan, got = run_plan(r, suite, SC.plan_bounds)
        SC.text_edge_hand_checks(suite, got, plan)
        run_plan(r, suite, SC.plan_sparse)
        i = TC.edge_docs()[0].index("n63")
        run_plan(r, suite, SC.plan_sparse, first=i, n=4)  # a range that starts behind log 0
        run_plan(r, suite, SC.plan_bounds, first=i + 1, n=5)
        run_plan(r, suite, lambda rows, n: [[] for _ in range(n)])  # zero slices
        run_plan(r, suite, lambda rows, n: [], first=2, n=0)  # the empty range
    finally:
        r.close()
    suite = TC.failed_log_suite()
    r = Resident(e, suite.batch, suite.table)
    try:
        _, _, got = run_plan(r, suite, SC.plan_bounds)
        k0, k1 = int(got.slice_off[1]), int(got.slice_off[2])
        assert k1 > k0 and not got.elem_start[k0:k1].any() and not got.elem_end[k0:k1].any() and int(got.unit_off[k1]) == int(got.unit_off[k0]) and int(got.sspan_off[k1]) == int(got.sspan_off[k0])
        run_plan(r, suite, SC.plan_bounds, first=1, n=2)
    finally:
        r.close()


def test_cases(eng):
    _suites(eng)


def test_cases_without_elem_rank(eng_lean):
    _suites(eng_lean)


@pytest.mark.parametrize("lean", [False, True])
def test_known_answer_documents(eng, eng_lean, lean):
    suite = TC.kat_suite()
    r = Resident(eng_lean if lean else eng, suite.batch, suite.table)
    try:
        rows, plan, got = run_plan(r, suite, SC.plan_kat)
        SC.check_kat_literals(suite, rows, got, plan)
    finally:
        r.close()


def test_arguments_and_the_empty_range(eng):
    from peritext_amd.engine import PtxError

    suite = TC.failed_log_suite()
    r = Resident(eng, suite.batch, suite.table)
    try:
        got = eng.text_slices(r.db, r.dr, r.ds, [], 3, 0)  # an empty range at the end of the batch
        assert len(got.status) == 0 and [int(x) for x in got.unit_off] == [0] and [int(x) for x in got.sspan_off] == [0] and len(got.text) == 0 and len(got.sspans) == 0
        none = eng.text_slices_flat(r.db, r.dr, r.ds, np.zeros(4, np.uint64), None, None)  # zero slices: NULL slice arrays are legal
        assert [int(x) for x in none.unit_off] == [0] and [int(x) for x in none.sspan_off] == [0]
        assert np.array_equal(none.status, eng.text(r.db, r.dr, r.ds).status), "exactly ptx_text.status of the same range"
        whole = eng.text_slices(r.db, r.dr, r.ds, [[(0, SC.ALL)]] * 3)
        assert whole.kernel_ms > 0 and np.array_equal(whole.status, none.status)
        off, start, end = SC.arrays_of([[(0, 1)], [], [(1, 2), (0, 9)]])
        bad = [dict(slice_off=np.array([1, 1, 1, 3], np.uint64), slice_start=start, slice_end=end), dict(slice_off=np.array([0, 2, 1, 3], np.uint64), slice_start=start, slice_end=end),
               dict(slice_off=off, slice_start=None, slice_end=end), dict(slice_off=off, slice_start=start, slice_end=None), dict(slice_off=None, slice_start=start, slice_end=end),
               dict(slice_off=np.array([0, 0, 0, 1 << 32], np.uint64), slice_start=start, slice_end=end),
               dict(slice_off=np.zeros(3, np.uint64), slice_start=None, slice_end=None, first_log=2, n_logs=2), dict(slice_off=np.zeros(1, np.uint64), slice_start=None, slice_end=None, first_log=4, n_logs=0)]
        for kw in bad:
            kw.setdefault("n_logs", 3)
            with pytest.raises(PtxError) as ei:
                eng.text_slices_flat(r.db, r.dr, r.ds, **kw)
            assert ei.value.status == abi.ERR_INVALID_ARG, kw
        empty = eng.upload_strings([])  # every value id is then beyond the table
        t = eng.text_slices(r.db, r.dr, empty, [[(0, 5)]] * 3)
        assert [int(x) for x in t.status] == [abi.ERR_BAD_OP, abi.ERR_SEQ_GAP, abi.ERR_BAD_OP] and not t.elem_end.any() and len(t.text) == 0 and len(t.sspans) == 0
        eng.free_strings(empty)
    finally:
        r.close()


def test_value_id_beyond_the_table(eng):
    """One log with a value id equal to n_strings: PTX_ERR_BAD_OP, empty slices without rows; its neighbours are bit-equal to the run without it."""
    suite = TC.edge_suite()
    log = [k for k, w in enumerate(suite.want) if len(w.units) == TC.T + 1][0]
    bad, _ = TC.bad_id_batch(suite, log)
    n = suite.batch.n_logs
    out, plan = [], None
    for batch in (suite.batch, bad):
        r = Resident(eng, batch, suite.table)
        try:
            rows = eng.download_range(r.db, r.dr, 0, n)
            plan = plan or SC.plan_bounds(rows, n)
            out.append((r.slices(plan, 0, n), rows))
        finally:
            r.close()
    (good, rows), (m, bad_rows) = out
    SC.check_range(suite, rows, good, 0, n, plan, decode=False)
    assert int(m.status[log]) == abi.ERR_BAD_OP and int(bad_rows.logs["status"][log]) == 0
    SC.check_range(suite, rows, m, 0, n, plan, status_of={log: abi.ERR_BAD_OP}, decode=False)
    for k in range(n):
        if k == log:
            continue
        for j in range(len(plan[k])):
            a, b = good.index(k, j), m.index(k, j)
            assert good.of_slice(a) == m.of_slice(b) and good.rows_of_slice(a) == m.rows_of_slice(b) and (good.elem_start[a], good.elem_end[a]) == (m.elem_start[b], m.elem_end[b])


class Generated:
    """100 documents x 3 replicas x 512 ops in the `rich4k` mix, generated and merged on the device, with Engine.text's download of the result."""

    def __init__(self, eng):
        cfg = workloads.gen_config("rich4k", ops=512)
        self.eng, self.n_docs = eng, 100
        self.h, _ = eng.generate(cfg["replicas"], cfg["ops_per_log"], cfg["mix"], cfg["mark_types"], self.n_docs, 23)
        self.dr = eng.alloc_result(self.h)
        eng.merge(self.h, self.dr)
        self.ds = eng.upload_strings([chr(i) for i in range(128)])
        self.text = eng.text(self.h, self.dr, self.ds)
        self.n = len(self.text.status)
        assert self.n == 3 * self.n_docs and not self.text.status.any()

    def units(self, log):
        return self.text.text[int(self.text.text_off[log]) : int(self.text.text_off[log + 1])]

    def close(self):
        self.eng.free_strings(self.ds)
        self.eng.free_result(self.dr)
        self.eng.free_batch(self.h)


@pytest.fixture(scope="module")
def generated(eng):
    g = Generated(eng)
    yield g
    g.close()


def test_generated_batch(eng, generated):
    """300 generated logs with three random slices each: against Python slices of Engine.text's download (one unit per element, so element indexes are unit
    offsets); the rows against the downloaded spans cut by a plain loop."""
    g = generated
    rnd = random.Random(5)
    rows = eng.download_range(g.h, g.dr, 0, g.n)
    plan = []
    for log in range(g.n):
        nv = len(g.units(log))
        plan.append([tuple(rnd.randrange(nv + 3) for _ in range(2)) for _ in range(3)])
    got = eng.text_slices(g.h, g.dr, g.ds, plan)
    assert not got.status.any() and int(got.unit_off[-1]) > 0
    for log in range(g.n):
        units, nv = g.units(log), len(g.units(log))
        sp = rows.spans[int(rows.span_off[log]) : int(rows.span_off[log + 1])]
        starts = [int(x["start"]) for x in sp] + [nv]
        for j, (s, e) in enumerate(plan[log]):
            k = got.index(log, j)
            a, b = min(s, nv), min(e, nv)
            b = max(a, b)
            assert (int(got.elem_start[k]), int(got.elem_end[k])) == (a, b), (log, j)
            assert np.array_equal(got.text[int(got.unit_off[k]) : int(got.unit_off[k + 1])], units[a:b]), (log, j)
            want = [(max(starts[q], a), int(sp[q]["attr"]), max(starts[q], a) - a) for q in range(len(sp)) if a < b and starts[q] < b and starts[q + 1] > a]
            assert got.rows_of_slice(k) == want, (log, j)


def test_find_then_snippets(eng, generated):
    """find_text -> windows of +- 3 elements -> text_slices: every snippet holds the pattern at the unit the hit says and equals the Python slice."""
    g = generated
    pattern = FC.two_letters(g.units(0))
    m = eng.find_text(g.h, g.dr, g.ds, pattern, max_hits_per_log=8)
    assert int(m.hit_off[-1]) > g.n_docs
    plan = [[(max(s - 3, 0), e + 3) for _, s, e in m.of_log(log)] for log in range(g.n)]
    got = eng.text_slices(g.h, g.dr, g.ds, plan)
    for log in range(g.n):
        units, text = g.units(log), wire.Text.of_log(g.text, log)
        for j, (u, s, e) in enumerate(m.of_log(log)):
            k = got.index(log, j)
            a, b = max(s - 3, 0), min(e + 3, len(units))
            assert (int(got.elem_start[k]), int(got.elem_end[k])) == (a, b)
            snippet = got.of_slice(k)
            assert snippet == text[a:b], (log, j)  # one unit per element
            assert snippet[u - a : u - a + len(pattern)] == pattern, (log, j)


def test_text_of_every_comment(eng):
    """slices = the result's cintervals: the text each comment covers, against the oracle's spans that carry the comment's id."""
    suite = TC.kat_suite()
    r = Resident(eng, suite.batch, suite.table)
    try:
        n = suite.batch.n_logs
        rows = eng.download_range(r.db, r.dr, 0, n)
        cints = [[(int(c["id"]), int(c["start"]), int(c["end"])) for c in rows.cintervals[int(rows.cint_off[k]) : int(rows.cint_off[k + 1])]] for k in range(n)]
        plan = [[(s, e) for _, s, e in ci] for ci in cints]
        got = r.slices(plan, 0, n)
        SC.check_range(suite, rows, got, 0, n, plan)
        seen = 0
        for log in range(n):
            comments = suite.batch.doc_comments[suite.batch.log_doc[log]]
            spans = suite.want[log].spans
            for j, (cid, s, e) in enumerate(cints[log]):
                # the oracle's spans that carry this comment and lie in one run with the interval: their joined text holds the interval's text
                marked = "".join(x["text"] for x in spans if any(c["id"] == comments[cid] for c in x["marks"].get("comment", [])))
                assert got.of_slice(got.index(log, j)) in marked and e > s, (log, j)
                seen += 1
        assert seen > 0
    finally:
        r.close()
