"""Find and replace on resident text views through the C ABI on a real MI355X (ptx_view_replace_plan): the cases of tests/test_emu_replace.py with the expected
values of tests/replace_cases.py, on a default context and on a PTX_FLAG_NO_ELEM_RANK one; every plan's matches are also those of ptx_view_find_text of the same
view.  Then replace all end to end: Engine.replace_text -> ptx_change -> append -> merge against the oracle's Changes and spans, and str.replace."""
import ctypes as C

import numpy as np
import pytest

import find_cases as FC
import helpers as H
import replace_cases as RC
import text_cases as TC
from peritext_amd import abi, wire

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
    """A view of the logs [first, first + n) of a batch merged on the device: the interface tests/replace_cases.py names.  The string table is freed right after the
    view is made."""

    def __init__(self, eng, suite, first, n):
        self.eng, self.suite, self.first, self.n = eng, suite, first, n
        self.db = eng.upload(suite.batch)
        self.dr = eng.alloc_result(self.db)
        eng.merge(self.db, self.dr)
        gone = eng.upload_strings(suite.table)
        self.view = eng.text_view(self.db, self.dr, gone, first, n)
        eng.free_strings(gone)
        self.rows = eng.download_range(self.db, self.dr, first, n) if n else None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.view.free()
        self.eng.free_result(self.dr)
        self.eng.free_batch(self.db)

    def find(self, q):
        return self.view.find_text(q.pattern, ascii_nocase=q.nocase, max_hits_per_log=q.cap)

    def replace_plan(self, ask, n_batch):
        _, ids = RC.ids_of(self.suite, ask)
        plan = self.view.replace_plan(ask.pattern, ids, n_batch, ascii_nocase=ask.nocase)
        assert plan.first_log == self.first and plan.ops.actor is None and plan.ops.max_actors == 0
        return plan


def _run_asks(e):
    """Every shared case; the views of one (suite, range) are made once and queried by all its cases."""
    open_views, changes, replaced, skipped = {}, 0, 0, 0

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
        for ask in RC.asks():
            c, r, s = RC.run_ask(opener, ask)
            changes, replaced, skipped = changes + c, replaced + r, skipped + s
    finally:
        for v in open_views.values():
            v.__exit__()
    assert changes > 40 and replaced > 1000 and skipped >= 5, "Changes were planned, matches replaced, and some skipped inside an element"


def test_cases(eng):
    _run_asks(eng)


def test_cases_without_elem_rank(eng_lean):
    _run_asks(eng_lean)


@pytest.mark.parametrize("lean", [False, True])
def test_known_answer_documents(eng, eng_lean, lean):
    suite = TC.kat_suite()
    n = suite.batch.n_logs
    with GpuView(eng_lean if lean else eng, suite, 0, n) as v:  # ONE view, two plans
        for ask in RC.kat_asks():
            table, _ = RC.ids_of(suite, ask)
            plan = v.replace_plan(ask, n)
            c, r, _ = RC.check_plan(suite, v.rows, plan, 0, n, n, ask, table)
            assert c > 0 and r >= c and plan.kernel_ms > 0, "some documents hold the pattern"
            assert np.array_equal(plan.n_matches, v.find(ask.query).n_matches)


def test_the_empty_view_and_invalid_arguments(eng):
    from peritext_amd.engine import PtxError

    suite = TC.failed_log_suite()
    with GpuView(eng, suite, 3, 0) as v:  # an empty range at the end of the batch: the all-zero plan
        p = v.view.replace_plan("a", [1, 2], 5)
        assert len(p.status) == 0 and [int(x) for x in p.ops.chg_off] == [0] * 6 and [int(x) for x in p.ops.op_off] == [0] and len(p.ops.action) == 0
        assert [int(x) for x in p.ops.values] == [1, 2] and p.n_replacement == 2
        with pytest.raises(PtxError) as ei:
            v.view.replace_plan("a", [1], 2)
        assert ei.value.status == abi.ERR_INVALID_ARG, "n_batch_logs ends before the view's range, empty as it is"
    with GpuView(eng, suite, 1, 2) as v:
        bad = [lambda: v.view.replace_plan("", [1], 3), lambda: v.view.replace_plan("a" * (abi.FIND_PATTERN_MAX + 1), [1], 3),
               lambda: v.view.replace_plan("a", np.zeros(abi.CHANGE_ROWS_MAX + 1, np.uint32), 3), lambda: v.view.replace_plan("a", [1], 2), lambda: v.view.replace_plan("a", [1], 0)]
        for call in bad:
            with pytest.raises(PtxError) as ei:
                call()
            assert ei.value.status == abi.ERR_INVALID_ARG
        pat, ids, out = TC.u16("a").astype(np.uint16), np.array([1], np.uint32), abi.ptx_replace_plan()
        pp, ip = pat.ctypes.data_as(abi.u16p), ids.ctypes.data_as(abi.u32p)
        for flags in (2, 0x80000000, 3):  # an unknown flag bit, alone or beside the known one
            assert eng.lib.ptx_view_replace_plan(eng.ctx, v.view.handle, pp, 1, flags, ip, 1, 3, C.byref(out)) == abi.ERR_INVALID_ARG
        assert eng.lib.ptx_view_replace_plan(eng.ctx, v.view.handle, pp, 1, 0, None, 1, 3, C.byref(out)) == abi.ERR_INVALID_ARG, "a replacement without ids"
        assert eng.lib.ptx_view_replace_plan(eng.ctx, v.view.handle, None, 1, 0, ip, 1, 3, C.byref(out)) == abi.ERR_INVALID_ARG, "the NULL pattern"
        assert eng.lib.ptx_view_replace_plan(eng.ctx, None, pp, 1, 0, ip, 1, 3, C.byref(out)) == abi.ERR_INVALID_ARG, "the NULL view"
        assert eng.lib.ptx_view_replace_plan(eng.ctx, v.view.handle, pp, 1, 0, ip, 1, 3, None) == abi.ERR_INVALID_ARG
        eng.lib.ptx_replace_plan_free(None)
        eng.lib.ptx_replace_plan_free(C.byref(out))  # a zeroed plan: nothing to free
        ok = v.view.replace_plan("a", [], 3)  # no replacement: NULL ids are legal, delete only
        assert not (ok.ops.action == abi.IN_INSERT).any() and np.array_equal(ok.status, v.find(FC.Query("a")).status)
        assert v.view.replace_plan("a", np.zeros(abi.CHANGE_ROWS_MAX, np.uint32), 3).n_replacement == abi.CHANGE_ROWS_MAX


@pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")
def test_replace_all_end_to_end(eng):
    """Engine.replace_text on two replicas' logs: the Changes equal the oracle's change() of the Python-built ops, and after append and merge the spans and the
    text equal the oracle's document after that change, and str.replace; a new view of the grown batch finds the pattern no more."""
    sentence = "the cat and the hat; breathe, then the end"
    values = list(sentence)
    values[4:7] = ["cat"]  # a pasted word as ONE element: element indexes are not unit offsets behind it
    other = list("no match here") + ["the"] + list(" the")  # "the" as ONE element: a whole element, replaceable, count 1
    docs = [[H.mini_doc([{"action": "addMark", "markType": "strong", "start": TC.bf(1), "end": TC.bf(14)}], first_text=values)], [H.mini_doc([], first_text=other)]]
    batch = wire.encode_docs(docs)
    suite = TC.Suite("replace_end_to_end", batch, list(batch.values), [TC.want_of_oracle(e[0]) for e in H.oracle_apply(docs, no_patches=True)], [])
    ask = RC.Ask("replace_end_to_end", "the", ("A", "n"))
    made_h = grown_h = dr2 = ds2 = view2 = None
    with GpuView(eng, suite, 0, 2) as r:
        try:
            made_h, status, plan = eng.replace_text(r.db, r.dr, r.view, batch, ask.pattern, list(ask.replacement), ["a", "a"])
            assert [int(s) for s in status] == [0, 0] and [int(x) for x in plan.n_replaced] == [5, 2]
            RC.check_plan(suite, r.rows, plan, 0, 2, 2, ask, batch.values)
            calls = [[RC.expect(suite, r.rows, 0, k, ask)["ops"]] for k in range(2)]
            assert plan.per_log(batch.values) == calls
            made = eng.download_batch(made_h, batch.values, batch.urls, batch.log_doc, batch.doc_actors, batch.doc_comments, batch.keys, batch.map_values)
            want = H.oracle_change(docs, calls, ["a", "a"])
            assert wire.decode_changes(made, 0, text_obj="1@a") + wire.decode_changes(made, 1, text_obj="1@a") == want
            grown_h = eng.append_device(r.db, made_h)
            dr2 = eng.alloc_result(grown_h)
            eng.merge(grown_h, dr2)
            grown = eng.download_batch(grown_h, batch.values, batch.urls, batch.log_doc, batch.doc_actors, batch.doc_comments)
            res = eng.download(grown_h, dr2)
            ds2 = eng.upload_strings(batch.values)
            view2 = eng.text_view(grown_h, dr2, ds2)
            again = view2.find_text(ask.pattern)
            text2 = eng.text(grown_h, dr2, ds2)
        finally:
            if view2 is not None:
                view2.free()
            if ds2 is not None:
                eng.free_strings(ds2)
            if dr2 is not None:
                eng.free_result(dr2)
            for h in (made_h, grown_h):
                if h is not None:
                    eng.free_batch(h)
    assert not res.logs["status"].any() and not again.status.any() and not again.n_matches.any(), "the replacement does not recreate the pattern"
    after = H.oracle_apply([[docs[0][0] + want[:1]], [docs[1][0] + want[1:]]], no_patches=True)
    for log, src in enumerate((sentence, "".join(other))):
        spans = wire.decode_spans(grown, res, log)
        assert H.norm_spans(spans) == H.norm_spans(after[log][0]["spans"])
        assert "".join(s["text"] for s in spans) == src.replace("the", "An") == wire.Text.of_log(text2, log)
