"""Find and replace with the InputOperations left on the device, through the C ABI on a real MI355X (ptx_view_replace_plan_device): the shared cases of
tests/replace_cases.py with its independent expected values, the downloaded device plan equal to ptx_view_replace_plan's byte for byte, on a default context and on
a PTX_FLAG_NO_ELEM_RANK one (the plan only: ptx_change_device refuses such a context as ptx_change does).  Then replace all end to end without the ops leaving
the device: Engine.replace_text_resident -> ptx_change_device -> append -> merge against the oracle's Changes and spans, and str.replace."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import find_cases as FC
import helpers as H
import replace_cases as RC
import test_gpu_replace as TGR
import text_cases as TC
from peritext_amd import abi, wire

pytestmark = pytest.mark.gpu

MAX_ACTORS = 3


@pytest.fixture(scope="module")
def eng():
    e = TGR._engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_lean():
    e = TGR._engine(abi.FLAG_NO_ELEM_RANK)
    yield e
    e.close()


def _same_ops(a, b, what):
    for f in ("chg_off", "op_off", "action", "mark_type", "index", "count", "payload", "values"):
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), "%s: %s" % (what, f)


class DeviceView(TGR.GpuView):
    """tests/test_gpu_replace.py's view, its plan made by ptx_view_replace_plan_device and brought down: equal to ptx_view_replace_plan's byte for byte, `actor`
    and `max_actors` those passed."""

    def replace_plan(self, ask, n_batch):
        _, ids = RC.ids_of(self.suite, ask)
        host = self.view.replace_plan(ask.pattern, ids, n_batch, ascii_nocase=ask.nocase)
        actor = (np.arange(n_batch, dtype=np.uint32) * 7 + 1) % MAX_ACTORS
        plan, h = self.view.replace_plan_device(ask.pattern, ids, n_batch, actor, MAX_ACTORS, ascii_nocase=ask.nocase)
        try:
            assert plan.ops is None and plan.first_log == self.first and plan.kernel_ms >= 0
            ops = self.eng.download_input_ops(h)
        finally:
            self.eng.free_input_ops(h)
        tag = "%s %r" % (self.suite.name, ask.pattern)
        for f in ("status", "n_matches", "n_chosen", "n_replaced"):
            assert getattr(plan, f).tobytes() == getattr(host, f).tobytes(), "%s: %s" % (tag, f)
        assert (plan.n_pattern, plan.n_replacement) == (host.n_pattern, host.n_replacement)
        _same_ops(ops, host.ops, tag)
        assert ops.max_actors == MAX_ACTORS and np.array_equal(ops.actor, actor), "actor and max_actors are those passed"
        return dataclasses.replace(plan, ops=ops)


def _run_asks(e):
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
            open_views[key] = DeviceView(e, suite, first, n)
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
    with DeviceView(eng_lean if lean else eng, suite, 0, n) as v:  # ONE view, two plans
        for ask in RC.kat_asks():
            table, _ = RC.ids_of(suite, ask)
            plan = v.replace_plan(ask, n)
            c, r, _ = RC.check_plan(suite, v.rows, plan, 0, n, n, ask, table)
            assert c > 0 and r >= c, "some documents hold the pattern"


def test_change_device_refuses_a_context_without_elem_rank(eng_lean):
    from peritext_amd.engine import PtxError

    suite = TC.kat_suite()
    n = suite.batch.n_logs
    with DeviceView(eng_lean, suite, 0, n) as v:
        _, h = v.view.replace_plan_device("e", [0], n, np.zeros(n, np.uint32), max(suite.batch.max_actors, 1))
        try:
            with pytest.raises(PtxError) as ei:
                eng_lean.change_device(v.db, v.dr, h)
            assert ei.value.status == abi.ERR_INVALID_ARG
        finally:
            eng_lean.free_input_ops(h)


def test_the_empty_view_and_invalid_arguments(eng):
    from peritext_amd.engine import PtxError

    suite = TC.failed_log_suite()
    act5, act3 = np.array([2, 0, 1, 0, 2], np.uint32), np.array([1, 0, 2], np.uint32)
    with DeviceView(eng, suite, 3, 0) as v:  # an empty range at the end of the batch: the all-zero plan
        p, h = v.view.replace_plan_device("a", [1, 2], 5, act5, 3)
        try:
            o = eng.download_input_ops(h)
        finally:
            eng.free_input_ops(h)
        assert len(p.status) == 0 and p.ops is None and p.n_replacement == 2
        assert [int(x) for x in o.chg_off] == [0] * 6 and [int(x) for x in o.op_off] == [0] and len(o.action) == 0
        assert [int(x) for x in o.values] == [1, 2] and np.array_equal(o.actor, act5) and o.max_actors == 3
        with pytest.raises(PtxError) as ei:
            v.view.replace_plan_device("a", [1], 2, act3[:2], 3)
        assert ei.value.status == abi.ERR_INVALID_ARG, "n_batch_logs ends before the view's range, empty as it is"
    with DeviceView(eng, suite, 1, 2) as v:
        d = lambda pat, ids, nb: v.view.replace_plan_device(pat, ids, nb, act3[:nb], 3)  # noqa: E731
        bad = [lambda: d("", [1], 3), lambda: d("a" * (abi.FIND_PATTERN_MAX + 1), [1], 3), lambda: d("a", np.zeros(abi.CHANGE_ROWS_MAX + 1, np.uint32), 3), lambda: d("a", [1], 2),
               lambda: d("a", [1], 0)]
        for call in bad:
            with pytest.raises(PtxError) as ei:
                call()
            assert ei.value.status == abi.ERR_INVALID_ARG
        pat, ids, out, h = TC.u16("a").astype(np.uint16), np.array([1], np.uint32), abi.ptx_replace_plan(), C.c_void_p()
        pp, ip, ap = pat.ctypes.data_as(abi.u16p), ids.ctypes.data_as(abi.u32p), act3.ctypes.data_as(abi.u32p)
        f = eng.lib.ptx_view_replace_plan_device
        for flags in (2, 0x80000000, 3):  # an unknown flag bit, alone or beside the known one
            assert f(eng.ctx, v.view.handle, pp, 1, flags, ip, 1, 3, ap, 3, C.byref(out), C.byref(h)) == abi.ERR_INVALID_ARG
        assert f(eng.ctx, v.view.handle, pp, 1, 0, None, 1, 3, ap, 3, C.byref(out), C.byref(h)) == abi.ERR_INVALID_ARG, "a replacement without ids"
        assert f(eng.ctx, v.view.handle, None, 1, 0, ip, 1, 3, ap, 3, C.byref(out), C.byref(h)) == abi.ERR_INVALID_ARG, "the NULL pattern"
        assert f(eng.ctx, None, pp, 1, 0, ip, 1, 3, ap, 3, C.byref(out), C.byref(h)) == abi.ERR_INVALID_ARG, "the NULL view"
        assert f(eng.ctx, v.view.handle, pp, 1, 0, ip, 1, 3, None, 3, C.byref(out), C.byref(h)) == abi.ERR_INVALID_ARG, "the NULL actor with logs in the batch"
        assert f(eng.ctx, v.view.handle, pp, 1, 0, ip, 1, 3, ap, 3, None, C.byref(h)) == abi.ERR_INVALID_ARG
        assert f(eng.ctx, v.view.handle, pp, 1, 0, ip, 1, 3, ap, 3, C.byref(out), None) == abi.ERR_INVALID_ARG
        assert not h.value
        eng.lib.ptx_input_ops_free(eng.ctx, None)
        eng.lib.ptx_host_input_ops_free(None)
        ok, h2 = d("a", [], 3)  # no replacement: NULL ids are legal, delete only
        try:
            o = eng.download_input_ops(h2)
        finally:
            eng.free_input_ops(h2)
        assert not (o.action == abi.IN_INSERT).any() and np.array_equal(ok.status, v.find(FC.Query("a")).status) and len(o.values) == 0


@pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")
def test_replace_all_resident_end_to_end(eng):
    """Engine.replace_text_resident on the two replicas of tests/test_gpu_replace.py's sentence case: the Changes equal the oracle's change() of the Python-built
    ops, and after append and merge the spans and the text equal the oracle's document after that change, and str.replace; a new view of the grown batch finds the
    pattern no more."""
    sentence = "the cat and the hat; breathe, then the end"
    values = list(sentence)
    values[4:7] = ["cat"]  # a pasted word as ONE element: element indexes are not unit offsets behind it
    other = list("no match here") + ["the"] + list(" the")  # "the" as ONE element: a whole element, replaceable, count 1
    docs = [[H.mini_doc([{"action": "addMark", "markType": "strong", "start": TC.bf(1), "end": TC.bf(14)}], first_text=values)], [H.mini_doc([], first_text=other)]]
    batch = wire.encode_docs(docs)
    suite = TC.Suite("replace_end_to_end", batch, list(batch.values), [TC.want_of_oracle(e[0]) for e in H.oracle_apply(docs, no_patches=True)], [])
    ask = RC.Ask("replace_end_to_end", "the", ("A", "n"))
    made_h = grown_h = dr2 = ds2 = view2 = None
    with TGR.GpuView(eng, suite, 0, 2) as r:
        try:
            made_h, status, plan = eng.replace_text_resident(r.db, r.dr, r.view, batch, ask.pattern, list(ask.replacement), ["a", "a"])
            assert [int(s) for s in status] == [0, 0] and [int(x) for x in plan.n_replaced] == [5, 2] and plan.ops is None
            calls = [[RC.expect(suite, r.rows, 0, k, ask)["ops"]] for k in range(2)]
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


def test_capacity_edge_logs_make_no_ops_on_the_device(eng):
    """replace_cases' capacity pair: a log whose Change would make more than 65 534 rows is PTX_ERR_CAPACITY and has no ops in the resident object either, while its
    neighbour makes its Change (the ops of a delete and of an insert of 65 533 values lie there).  Where every log with a match is beyond the capacity, the
    resident plan goes through ptx_change_device as ptx_change takes the host plan: no Change, every status PTX_OK.  (The Change of 65 534 rows itself is not made
    here: one wave inserting 65 533 elements one by one takes longer than a test may.)"""
    suite, N = RC.edge_suite()
    batch = suite.batch
    first, n, nb = N["cap_two"], 3, batch.n_logs
    actor, na = np.zeros(nb, np.uint32), max(batch.max_actors, 1)
    with TGR.GpuView(eng, suite, first, n) as v:
        for nrep, want_status, want_makes in ((abi.CHANGE_ROWS_MAX - 1, [abi.ERR_CAPACITY, 0, 0], [0, 1, 0]), (abi.CHANGE_ROWS_MAX, [abi.ERR_CAPACITY, abi.ERR_CAPACITY, 0], [0, 0, 0])):
            ask = next(a for a in RC.asks() if a.tag == "capacity %d" % nrep)
            _, ids = RC.ids_of(suite, ask)
            plan, h = v.view.replace_plan_device(ask.pattern, ids, nb, actor, na)
            made_h = made_host = None
            try:
                ops = eng.download_input_ops(h)
                assert [int(x) for x in plan.status] == want_status and [int(x) for x in plan.n_replaced] == [2, 1, 0]
                makes = np.diff(ops.chg_off.astype(np.int64))
                assert makes[first : first + 3].tolist() == want_makes and makes.sum() == sum(want_makes), "a log beyond the capacity has no ops; its neighbour makes its Change"
                if sum(want_makes):
                    assert ops.action.tolist() == [abi.IN_DELETE, abi.IN_INSERT] and ops.count.tolist() == [1, nrep] and ops.index.tolist() == [0, 0] and len(ops.values) == nrep
                    continue
                made_h, status = eng.change_device(v.db, v.dr, h)
                host = v.view.replace_plan(ask.pattern, ids, nb)
                host.ops.actor, host.ops.max_actors = actor, na
                made_host, status_host = eng.change(v.db, v.dr, host.ops)
                assert np.array_equal(status, status_host) and not status.any()
                a, b = eng.download_batch(made_h), eng.download_batch(made_host)
                assert a.n_ops == 0 and a.n_logs == nb
                for f in ("log_off", "chg_off", "log_hdr"):
                    assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
            finally:
                eng.free_input_ops(h)
                for m in (made_h, made_host):
                    if m is not None:
                        eng.free_batch(m)
