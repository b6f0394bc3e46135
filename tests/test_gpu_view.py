"""Resident text views through the C ABI on a real MI355X (ptx_text_view_create -> ptx_view_find_text / ptx_view_text_slices / ptx_view_find_snippets): the cases
of tests/test_emu_view.py with the expected values of tests/view_cases.py, on a default context and on a PTX_FLAG_NO_ELEM_RANK one; every answer also bit-equal
to its ptx_result_* twin.  In every case the string table is freed right after the view is made.  Then 300 logs generated on the device in the `rich4k` mix
against str.find and Python slices of Engine.text's download, and find-snippets -> addMark -> append -> merge against the oracle's spans."""
import ctypes as C

import numpy as np
import pytest

import find_cases as FC
import helpers as H
import slice_cases as SC
import text_cases as TC
import view_cases as VC
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


class GpuView:
    """A view of the logs [first, first + n) of a batch merged on the device, and its twins: the interface tests/view_cases.py names.  The view is made from a
    string table of its own, freed before the first query; the twins get another."""

    def __init__(self, eng, suite, first, n, batch=None):
        self.eng, self.suite, self.first, self.n = eng, suite, first, n
        batch = suite.batch if batch is None else batch
        self.db = eng.upload(batch)
        self.dr = eng.alloc_result(self.db)
        eng.merge(self.db, self.dr)
        gone = eng.upload_strings(suite.table)
        self.view = eng.text_view(self.db, self.dr, gone, first, n)
        eng.free_strings(gone)
        self.ds = eng.upload_strings(suite.table)
        self.rows = eng.download_range(self.db, self.dr, first, n) if n else None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.view.free()
        self.eng.free_strings(self.ds)
        self.eng.free_result(self.dr)
        self.eng.free_batch(self.db)

    def find(self, q):
        return self.view.find_text(q.pattern, ascii_nocase=q.nocase, max_hits_per_log=q.cap)

    def slices(self, plan):
        return self.view.text_slices(plan)

    def snippets(self, q, before, after):
        return self.view.find_snippets(q.pattern, before, after, ascii_nocase=q.nocase, max_hits_per_log=q.cap)

    def twin_find(self, q):
        return self.eng.find_text(self.db, self.dr, self.ds, q.pattern, self.first, self.n, ascii_nocase=q.nocase, max_hits_per_log=q.cap)

    def twin_slices(self, plan):
        return self.eng.text_slices(self.db, self.dr, self.ds, plan, self.first, self.n)


def _run_cases(e):
    """Every shared case; the views of one (suite, range) are made once and queried by all its cases."""
    open_views, total, starts, ends = {}, 0, 0, 0

    class Shared:
        def __init__(self, v):
            self.v = v

        def __enter__(self):
            return self.v

        def __exit__(self, *exc):
            pass

    def opener(suite, first, n):
        key = (suite.name, first, n)
        if key not in open_views:
            open_views[key] = GpuView(e, suite, first, n)
        return Shared(open_views[key])

    try:
        for case in VC.cases():
            ns, a, b = VC.run_case(opener, case)
            total, starts, ends = total + ns, starts + a, ends + b
    finally:
        for v in open_views.values():
            v.__exit__()
    assert total > 1000 and starts > 0 and ends > 0, "snippets were cut, some at element 0 and some at the log's end"


def test_cases(eng):
    _run_cases(eng)


def test_cases_without_elem_rank(eng_lean):
    _run_cases(eng_lean)


@pytest.mark.parametrize("lean", [False, True])
def test_known_answer_documents(eng, eng_lean, lean):
    suite = TC.kat_suite()
    with GpuView(eng_lean if lean else eng, suite, 0, suite.batch.n_logs) as v:  # ONE view, 46 queries
        for case in VC.kat_cases():
            got = v.snippets(case.q, 1, 1)
            ns, _, _ = VC.check_snippets(suite, v.rows, got, 0, v.n, case.q, 1, 1)
            assert ns > 0, "the document holds its own pattern"
            VC.check_same(got.matches(), v.twin_find(case.q), VC.MATCH_FIELDS)


@pytest.mark.parametrize("lean", [False, True])
def test_one_view_many_queries(eng, eng_lean, lean):
    suite, _ = FC.edge_suite()
    with GpuView(eng_lean if lean else eng, suite, 0, suite.batch.n_logs) as v:
        VC.view_session(v, suite, 0, v.n)
        info = v.view.info()
        text = v.eng.text(v.db, v.dr, v.ds)
        nv = sum(int(v.rows.value_off[k + 1]) - int(v.rows.value_off[k]) + 1 for k in range(v.n) if int(text.status[k]) == 0)
        assert (info["n_logs"], info["first_log"], info["n_units"], info["n_prefix_words"]) == (v.n, 0, int(text.text_off[-1]), nv)
        assert info["bytes"] >= 2 * info["n_units"] + 4 * nv and info["kernel_ms"] > 0


def test_the_empty_view_and_invalid_arguments(eng):
    from peritext_amd.engine import PtxError

    suite = TC.failed_log_suite()
    with GpuView(eng, suite, 3, 0) as v:  # an empty range at the end of the batch
        m = v.find(FC.Query("a"))
        assert len(m.status) == 0 and [int(x) for x in m.hit_off] == [0] and len(m.hit_unit) == 0 and len(m.n_matches) == 0
        s = v.snippets(FC.Query("a"), 1, 1)
        assert [int(x) for x in s.slice_off] == [0] and [int(x) for x in s.unit_off] == [0] and [int(x) for x in s.sspan_off] == [0] and len(s.text) == 0 and len(s.match_unit) == 0
        c = v.slices([])
        assert [int(x) for x in c.unit_off] == [0] and [int(x) for x in c.sspan_off] == [0] and len(c.text) == 0 and len(c.sspans) == 0
        assert v.view.info()["bytes"] == 0 and v.view.info()["n_units"] == 0
        for first, n in ((2, 2), (4, 0)):  # a range outside the batch
            with pytest.raises(PtxError) as ei:
                eng.text_view(v.db, v.dr, v.ds, first, n)
            assert ei.value.status == abi.ERR_INVALID_ARG
    with GpuView(eng, suite, 0, 3) as v:
        whole = v.snippets(FC.Query("a"), 1, 1)
        assert whole.kernel_ms > 0 and np.array_equal(whole.status, eng.text(v.db, v.dr, v.ds).status), "exactly ptx_text.status of the same range"
        for q in (FC.Query(""), FC.Query("a" * (abi.FIND_PATTERN_MAX + 1))):
            for call in (lambda: v.find(q), lambda: v.snippets(q, 1, 1)):
                with pytest.raises(PtxError) as ei:
                    call()
                assert ei.value.status == abi.ERR_INVALID_ARG, q
        pat = TC.u16("a").astype(np.uint16)
        out, snip, cut = abi.ptx_matches(), abi.ptx_snippets(), abi.ptx_slices()
        for flags in (2, 0x80000000, 3):  # an unknown flag bit, alone or beside the known one
            assert eng.lib.ptx_view_find_text(eng.ctx, v.view.handle, pat.ctypes.data_as(abi.u16p), 1, flags, 1, C.byref(out)) == abi.ERR_INVALID_ARG
            assert eng.lib.ptx_view_find_snippets(eng.ctx, v.view.handle, pat.ctypes.data_as(abi.u16p), 1, flags, 1, 0, 0, C.byref(snip)) == abi.ERR_INVALID_ARG
        # the NULL view
        assert eng.lib.ptx_view_find_text(eng.ctx, None, pat.ctypes.data_as(abi.u16p), 1, 0, 1, C.byref(out)) == abi.ERR_INVALID_ARG
        assert eng.lib.ptx_view_find_snippets(eng.ctx, None, pat.ctypes.data_as(abi.u16p), 1, 0, 1, 0, 0, C.byref(snip)) == abi.ERR_INVALID_ARG
        assert eng.lib.ptx_view_text_slices(eng.ctx, None, None, None, None, C.byref(cut)) == abi.ERR_INVALID_ARG
        assert eng.lib.ptx_view_info(eng.ctx, None, C.byref(abi.ptx_view_desc())) == abi.ERR_INVALID_ARG
        count_only = v.snippets(FC.Query("a", cap=0), 1, 1)
        assert np.array_equal(count_only.n_matches, whole.n_matches) and len(count_only.hit_unit) == 0 and not count_only.slice_off.any() and len(count_only.text) == 0
        off, start, end = SC.arrays_of([[(0, 1)], [], [(1, 2), (0, 9)]])
        bad = [(np.array([1, 1, 1, 3], np.uint64), start, end), (np.array([0, 2, 1, 3], np.uint64), start, end), (off, None, end), (off, start, None), (None, start, end),
               (np.array([0, 0, 0, 1 << 32], np.uint64), start, end)]
        for arrays in bad:
            with pytest.raises(PtxError) as ei:
                v.view.text_slices_flat(*arrays)
            assert ei.value.status == abi.ERR_INVALID_ARG
        none = v.view.text_slices_flat(np.zeros(4, np.uint64), None, None)  # zero slices: NULL slice arrays are legal
        assert [int(x) for x in none.unit_off] == [0] and [int(x) for x in none.sspan_off] == [0] and np.array_equal(none.status, whole.status)
        empty = eng.upload_strings([])  # every value id is then beyond the table
        ev = eng.text_view(v.db, v.dr, empty)
        eng.free_strings(empty)
        t = ev.find_snippets("a", 1, 1)
        assert [int(x) for x in t.status] == [abi.ERR_BAD_OP, abi.ERR_SEQ_GAP, abi.ERR_BAD_OP] and not t.n_matches.any() and ev.info()["n_prefix_words"] == 0
        ev.free()


def test_value_id_beyond_the_table(eng):
    """One log with a value id equal to n_strings: PTX_ERR_BAD_OP as the twins say, no hits and no snippets; its neighbours are bit-equal to the run without it."""
    suite = TC.edge_suite()
    log = [k for k, w in enumerate(suite.want) if len(w.units) == TC.T + 1][0]
    bad, _ = TC.bad_id_batch(suite, log)
    n, q = suite.batch.n_logs, FC.Query("e")
    with GpuView(eng, suite, 0, n) as g, GpuView(eng, suite, 0, n, batch=bad) as v:
        good, m = g.snippets(q, 2, 2), v.snippets(q, 2, 2)
        assert int(good.n_matches[log]) > 0
        assert int(m.status[log]) == abi.ERR_BAD_OP and int(v.rows.logs["status"][log]) == 0 and int(m.n_matches[log]) == 0 and int(m.slice_off[log + 1]) == int(m.slice_off[log])
        assert np.array_equal(m.status, v.twin_find(q).status)
        VC.check_snippets(suite, g.rows, m, 0, n, q, 2, 2, status_of={log: abi.ERR_BAD_OP}, decode=False)
        for k in range(n):
            if k != log:
                assert good.of_log(k) == m.of_log(k) and int(m.n_matches[k]) == int(good.n_matches[k])
                assert [good.rows_of_slice(good.index(k, j)) for j in range(len(good.of_log(k)))] == [m.rows_of_slice(m.index(k, j)) for j in range(len(m.of_log(k)))]


def test_generated_batch(eng):
    """100 documents x 3 replicas x 512 ops in the `rich4k` mix, generated on the device: snippets of +- 16 elements around a two-letter pattern of the first
    log's own text, against str.find repeated and Python slices of Engine.text's download of the same result (one unit per element, so element indexes are unit
    offsets); some snippet saturates at each end."""
    cfg = workloads.gen_config("rich4k", ops=512)
    h, _ = eng.generate(cfg["replicas"], cfg["ops_per_log"], cfg["mix"], cfg["mark_types"], 100, 23)
    dr = ds = view = None
    try:
        dr = eng.alloc_result(h)
        eng.merge(h, dr)
        ds = eng.upload_strings([chr(i) for i in range(128)])
        text = eng.text(h, dr, ds)
        n = len(text.status)
        assert n == 300 and not text.status.any()
        view = eng.text_view(h, dr, ds)
        eng.free_strings(ds)
        ds = None
        pattern = FC.two_letters(text.text[int(text.text_off[0]) : int(text.text_off[1])])
        got = view.find_snippets(pattern, 16, 16, max_hits_per_log=8)
        assert not got.status.any() and int(got.n_matches[0]) >= 1, "the first log holds its own pattern"
        at_start = at_end = 0
        for log in range(n):
            t = wire.Text.of_log(text, log)
            hits, p = [], t.find(pattern)
            while p >= 0:
                hits.append(p)
                p = t.find(pattern, p + 1)
            assert int(got.n_matches[log]) == len(hits), log
            want = [(p, p, p + 2, t[max(p - 16, 0) : p + 18], p - max(p - 16, 0)) for p in hits[:8]]
            assert got.of_log(log) == want, log
            at_start += sum(p < 16 for p in hits[:8])
            at_end += sum(p + 18 > len(t) for p in hits[:8])
        assert at_start > 0 and at_end > 0, "a snippet saturates at each end"
        assert view.info()["n_units"] == len(text.text) and view.info()["n_prefix_words"] == len(text.text) + n
    finally:
        if view is not None:
            view.free()
        if ds is not None:
            eng.free_strings(ds)
        if dr is not None:
            eng.free_result(dr)
        eng.free_batch(h)


def test_find_snippets_then_mark_every_mention(eng):
    """Snippets of a word from a view, every hit fed to Engine.change as addMark strong {startIndex: hit_start, endIndex: hit_end}, append, merge: the spans equal
    the oracle's for the same InputOperations, and every mention — and nothing else — is bold."""
    sentence = "the cat and the hat; breathe, then the end"
    values = list(sentence)
    values[4:7] = ["cat"]  # a pasted word as ONE element: element indexes are not unit offsets behind it
    base = H.mini_doc([], first_text=values)
    batch = wire.encode_docs([[base]])
    suite = TC.Suite("mentions", batch, list(batch.values), [], [])
    made_h = grown_h = dr2 = None
    with GpuView(eng, suite, 0, 1) as r:
        try:
            got = r.snippets(FC.Query("the"), 1, 1)
            hits = got.of_log(0)
            assert [(u, s, e) for u, s, e, _, _ in hits] == [(0, 0, 3), (12, 10, 13), (25, 23, 26), (30, 28, 31), (35, 33, 36)]
            assert [(t, mu) for _, _, _, t, mu in hits] == [("the ", 0), (" the ", 1), ("athe,", 1), (" then", 1), (" the ", 1)]
            marks = [{"path": ["text"], "action": "addMark", "markType": "strong", "startIndex": s, "endIndex": e} for _, s, e, _, _ in hits]
            calls = [[marks]]
            made_h, status = eng.change(r.db, r.dr, wire.encode_input_ops(batch, calls, ["a"]))
            assert [int(s) for s in status] == [0]
            grown_h = eng.append_device(r.db, made_h)
            dr2 = eng.alloc_result(grown_h)
            eng.merge(grown_h, dr2)
            grown = eng.download_batch(grown_h, batch.values, batch.urls, batch.log_doc, batch.doc_actors, batch.doc_comments)
            res = eng.download(grown_h, dr2)
        finally:
            if dr2 is not None:
                eng.free_result(dr2)
            for h in (made_h, grown_h):
                if h is not None:
                    eng.free_batch(h)
    assert int(res.logs["status"][0]) == 0
    spans = wire.decode_spans(grown, res, 0)
    made = H.oracle_change([[base]], calls, ["a"])
    want = H.oracle_apply([[base + made]], no_patches=True)[0][0]["spans"]
    assert H.norm_spans(spans) == H.norm_spans(want)
    assert [s["text"] for s in spans if s["marks"]] == ["the"] * 5 and "".join(s["text"] for s in spans) == sentence
