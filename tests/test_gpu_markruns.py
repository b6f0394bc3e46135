"""Queries by format on a resident text view through the C ABI on a real MI355X (ptx_view_mark_runs, ptx_view_mark_snippets, ptx_view_find_in_marks): the cases of
tests/test_emu_markruns.py with the expected values of tests/markrun_cases.py, on a default context and on a PTX_FLAG_NO_ELEM_RANK one.  Then 300 logs generated on
the device in the `rich4k` mix against the host path a caller had before (the downloaded spans and cintervals coalesced with numpy), and every comment's run from
mark_snippets -> removeMark over it through ptx_change -> append -> merge: the oracle's spans of the grown replicas hold no comment id."""
import ctypes as C

import numpy as np
import pytest

import find_cases as FC
import helpers as H
import markrun_cases as MC
import text_cases as TC
from peritext_amd import abi, wire, workloads
from test_gpu_view import GpuView, _engine

pytestmark = pytest.mark.gpu


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


class GpuMarkView(GpuView):
    """tests/test_gpu_view.py's view and, over it, the interface tests/markrun_cases.py names."""

    def mark_runs(self, mark_type, ident, cap):
        return self.view.mark_runs(mark_type, ident, max_runs_per_log=cap)

    def mark_snippets(self, mark_type, ident, cap, before, after):
        return self.view.mark_snippets(mark_type, ident, before, after, max_runs_per_log=cap)

    def find_in_marks(self, q, mark_type, ident):
        return self.view.find_in_marks(q.pattern, mark_type, ident, ascii_nocase=q.nocase, max_hits_per_log=q.cap)


class _Views:
    """The views of one (suite, range) are made once and queried by all its cases."""

    def __init__(self, e):
        self.e, self.open = e, {}

    def __call__(self, suite, first, n):
        key = (suite.name, first, n)
        if key not in self.open:
            self.open[key] = GpuMarkView(self.e, suite, first, n)
        views = self

        class Shared:
            def __enter__(self):
                return views.open[key]

            def __exit__(self, *exc):
                pass

        return Shared()

    def close(self):
        for v in self.open.values():
            v.__exit__()


@pytest.fixture(scope="module", params=[False, True], ids=["default", "no_elem_rank"])
def views(request, eng, eng_lean):
    v = _Views(eng_lean if request.param else eng)
    yield v
    v.close()


def test_run_cases(views):
    runs = snips = 0
    for case in MC.run_cases():
        r, s = MC.run_run_case(views, case)
        runs, snips = runs + r, snips + s
    assert runs > 1000 and snips == runs, "runs were listed, one snippet each"


def test_find_in_marks(views):
    kept = dropped = 0
    for case in MC.find_cases():
        k, d = MC.run_find_case(views, case)
        kept, dropped = kept + k, dropped + d
    assert kept > 300 and dropped > 300, "hits were kept and hits were dropped"


def test_known_answer_documents(views):
    runs = sum(MC.run_run_case(views, case)[0] for case in MC.kat_run_cases())
    assert runs > 50, "the documents hold marks of every kind"
    assert sum(MC.run_find_case(views, case)[0] for case in MC.kat_find_cases()) > 0


def test_any_comment_order_is_the_results(views):
    """PTX_MARK_ANY_ID on comments: the runs ARE the log's cinterval rows, in the result's own order (id, start), which is not ascending start across ids."""
    suite, N = MC.edge_suite()
    with views(suite, N["comments"], 1) as v:
        got = v.mark_runs(MC.COMMENT, MC.ANY, MC.ALL)
        c = v.rows.cintervals[int(v.rows.cint_off[0]) : int(v.rows.cint_off[1])]
        assert [(s, e, i) for s, e, i, _, _ in got.of_log(0)] == [(int(x["start"]), int(x["end"]), int(x["id"])) for x in c] and len(c) == 3
        starts = [s for s, *_ in got.of_log(0)]
        assert starts != sorted(starts) and got.kernel_ms > 0


def test_the_empty_view_and_invalid_arguments(eng):
    from peritext_amd.engine import PtxError

    suite = TC.failed_log_suite()
    with GpuMarkView(eng, suite, 3, 0) as v:  # an empty range at the end of the batch
        r = v.mark_runs(MC.STRONG, MC.ANY, MC.ALL)
        assert len(r.status) == 0 and [int(x) for x in r.run_off] == [0] and len(r.run_start) == 0 and len(r.n_runs) == 0
        s = v.mark_snippets(MC.COMMENT, MC.ANY, MC.ALL, 1, 1)
        assert [int(x) for x in s.slice_off] == [0] and [int(x) for x in s.unit_off] == [0] and [int(x) for x in s.sspan_off] == [0] and len(s.text) == 0 and len(s.match_unit) == 0
        m = v.find_in_marks(FC.Query("a"), MC.LINK, MC.ANY)
        assert len(m.status) == 0 and [int(x) for x in m.hit_off] == [0] and len(m.hit_unit) == 0
    with GpuMarkView(eng, suite, 0, 3) as v:
        whole = v.find(FC.Query("a"))
        for mark_type, ident, find_only in MC.invalid_selectors():
            calls = [lambda: v.find_in_marks(FC.Query("a"), mark_type, ident)]
            if not find_only:
                calls += [lambda: v.mark_runs(mark_type, ident, MC.ALL), lambda: v.mark_snippets(mark_type, ident, MC.ALL, 1, 1)]
            for call in calls:
                with pytest.raises(PtxError) as ei:
                    call()
                assert ei.value.status == abi.ERR_INVALID_ARG, (mark_type, ident)
        for q in (FC.Query(""), FC.Query("a" * (abi.FIND_PATTERN_MAX + 1))):  # the argument errors of ptx_view_find_text
            with pytest.raises(PtxError) as ei:
                v.find_in_marks(q, MC.STRONG, MC.ANY)
            assert ei.value.status == abi.ERR_INVALID_ARG, q
        pat = TC.u16("a").astype(np.uint16)
        out, runs, snip = abi.ptx_matches(), abi.ptx_mark_runs(), abi.ptx_mark_snippets()
        assert eng.lib.ptx_view_find_in_marks(eng.ctx, v.view.handle, pat.ctypes.data_as(abi.u16p), 1, 2, MC.STRONG, MC.ANY, 1, C.byref(out)) == abi.ERR_INVALID_ARG, "an unknown flag"
        # the NULL view
        assert eng.lib.ptx_view_mark_runs(eng.ctx, None, MC.STRONG, MC.ANY, 1, C.byref(runs)) == abi.ERR_INVALID_ARG
        assert eng.lib.ptx_view_mark_snippets(eng.ctx, None, MC.STRONG, MC.ANY, 1, 0, 0, C.byref(snip)) == abi.ERR_INVALID_ARG
        assert eng.lib.ptx_view_find_in_marks(eng.ctx, None, pat.ctypes.data_as(abi.u16p), 1, 0, MC.STRONG, MC.ANY, 1, C.byref(out)) == abi.ERR_INVALID_ARG
        r = v.mark_runs(MC.LINK, abi.ATTR_ID_MASK, MC.ALL)  # the largest url id is a legal selector; nothing has it
        assert not r.n_runs.any() and np.array_equal(r.status, whole.status), "exactly ptx_matches.status of the view"
        count_only = v.mark_snippets(MC.STRONG, MC.ANY, 0, 1, 1)
        assert np.array_equal(count_only.n_runs, v.mark_runs(MC.STRONG, MC.ANY, MC.ALL).n_runs) and not count_only.slice_off.any() and len(count_only.text) == 0


def _numpy_filter(m, runs, n):
    """The hits of a wire.Matches (uncapped) that lie inside one run of a wire.MarkRuns (uncapped): the host path's filter."""
    out = []
    for k in range(n):
        h0, h1, r0, r1 = int(m.hit_off[k]), int(m.hit_off[k + 1]), int(runs.run_off[k]), int(runs.run_off[k + 1])
        rs, re_ = runs.run_start[r0:r1], runs.run_end[r0:r1]
        hs, he = m.hit_start[h0:h1], m.hit_end[h0:h1]
        at = np.searchsorted(rs, hs, side="right").astype(np.int64) - 1
        ok = (at >= 0) & (he <= (re_[np.maximum(at, 0)] if len(rs) else np.zeros(len(hs), np.uint32)))
        out.append([(int(m.hit_unit[h0 + i]), int(hs[i]), int(he[i])) for i in np.flatnonzero(ok)])
    return out


def test_generated_batch_end_to_end(eng):
    """100 documents x 3 replicas x 512 ops in the `rich4k` mix, generated on the device.  Every selector's runs against the numpy host path over the downloaded
    rows (one unit per element, so run_unit == run_start); the text of every comment's run; find inside strong against find_text and a numpy filter.  Then
    removeMark over every comment run, through ptx_change, append and merge: no comment id is left, in the library's result and in the oracle's spans."""
    cfg = workloads.gen_config("rich4k", ops=512)
    h, info = eng.generate(cfg["replicas"], cfg["ops_per_log"], cfg["mix"], cfg["mark_types"], 100, 29)
    actors_t, comments_t, log_doc_t = wire.generated_tables(100, cfg["replicas"], info["n_comments"])
    dr = dr2 = ds = view = view2 = made_h = grown_h = None
    try:
        batch = eng.download_batch(h, wire.GEN_VALUES, wire.GEN_URLS, log_doc_t, actors_t, comments_t)
        dr = eng.alloc_result(h)
        eng.merge(h, dr)
        ds = eng.upload_strings([chr(i) for i in range(128)])
        text = eng.text(h, dr, ds)
        view = eng.text_view(h, dr, ds)
        rows = eng.download_range(h, dr, 0, batch.n_logs)
        n = batch.n_logs
        assert n == 300 and not text.status.any()
        total = {}
        for mt, ident in ((MC.STRONG, MC.ANY), (MC.EM, MC.ANY), (MC.LINK, MC.ANY), (MC.LINK, 1), (MC.COMMENT, MC.ANY), (MC.COMMENT, 0)):
            got = view.mark_runs(mt, ident)
            for k in range(n):
                want = MC.host_runs(rows, k, mt, ident)
                assert [r[:3] for r in got.of_log(k)] == want and int(got.n_runs[k]) == len(want), (mt, ident, k)
                assert [(u, ln) for _, _, _, u, ln in got.of_log(k)] == [(s, e - s) for s, e, _ in want], "one unit per element"
            total[(mt, ident)] = int(got.run_off[n])
        assert all(v > 0 for (_, ident), v in total.items() if ident == MC.ANY), total
        snip = view.mark_snippets(MC.COMMENT, MC.ANY)
        for k in range(n):
            t = text.of_log(k)
            assert [x[5] for x in snip.of_log(k)] == [t[s:e] for s, e, _ in MC.host_runs(rows, k, MC.COMMENT, MC.ANY)], k
        pattern = FC.two_letters(text.text[int(text.text_off[0]) : int(text.text_off[1])])[:1]
        inside, every, strong = view.find_in_marks(pattern, MC.STRONG), view.find_text(pattern), view.mark_runs(MC.STRONG)
        want = _numpy_filter(every, strong, n)
        assert [inside.of_log(k) for k in range(n)] == want and [int(x) for x in inside.n_matches] == [len(w) for w in want]
        assert 0 < int(inside.hit_off[n]) < int(every.hit_off[n]), "hits were kept and hits were dropped"
        # removeMark over every run of every comment
        calls, who = [], []
        for log in range(n):
            ids = batch.doc_comments[batch.log_doc[log]]
            ops = [{"path": ["text"], "action": "removeMark", "markType": "comment", "attrs": {"id": ids[i]}, "startIndex": s, "endIndex": e} for s, e, i, *_ in snip.of_log(log)]
            calls.append([ops] if ops else [])
            who.append("doc%d" % (log % cfg["replicas"] + 1))
        made_h, status = eng.change(h, dr, wire.encode_input_ops(batch, calls, who))
        assert not status.any()
        grown_h = eng.append_device(h, made_h)
        dr2 = eng.alloc_result(grown_h)
        eng.merge(grown_h, dr2)
        view2 = eng.text_view(grown_h, dr2, ds)
        after = view2.mark_runs(MC.COMMENT, MC.ANY)
        assert not after.status.any() and not after.n_runs.any(), "no comment run is left"
        assert np.array_equal(view2.mark_runs(MC.STRONG).run_start, strong.run_start), "the other marks are where they were"
        grown = eng.download_batch(grown_h, batch.values, batch.urls, batch.log_doc, batch.doc_actors, batch.doc_comments)
    finally:
        for v in (view, view2):
            if v is not None:
                v.free()
        if ds is not None:
            eng.free_strings(ds)
        for r in (dr, dr2):
            if r is not None:
                eng.free_result(r)
        for x in (h, made_h, grown_h):
            if x is not None:
                eng.free_batch(x)
    docs = [[wire.decode_changes(grown, d * cfg["replicas"] + r) for r in range(cfg["replicas"])] for d in range(100)]
    held = 0
    for doc in H.oracle_apply(docs, no_patches=True):
        for rep in doc:
            assert "error" not in rep
            assert not any(s["marks"].get("comment") for s in rep["spans"]), "the oracle's spans hold no comment id"
            held += sum("comment" in s["marks"] for s in rep["spans"])
    assert held > 0, "the key stays: comment: [] is what removeMark leaves"
