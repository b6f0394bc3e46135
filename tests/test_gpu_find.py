"""Find in the documents' text through the C ABI on a real MI355X (ptx_strings_upload -> ptx_merge -> ptx_result_find_text): the cases of
tests/test_emu_find.py with the expected values of tests/find_cases.py (a plain loop over the oracle's text), on a default context and on a
PTX_FLAG_NO_ELEM_RANK one; one batch generated on the device in the `rich4k` mix against a Python search of Engine.text's download of the same result; and find ->
change -> append -> merge against the oracle's spans for the same InputOperations."""
import numpy as np
import pytest

import find_cases as FC
import helpers as H
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

    def find(self, q, first, n):
        return self.eng.find_text(self.db, self.dr, self.ds, q.pattern, first, n, ascii_nocase=q.nocase, max_hits_per_log=q.cap)

    def close(self):
        self.eng.free_strings(self.ds)
        self.eng.free_result(self.dr)
        self.eng.free_batch(self.db)


def run_queries(e, suite, queries):
    r = Resident(e, suite.batch, suite.table)
    got, rows = {}, {}
    try:
        for q in queries:
            first, n = q.rng or (0, suite.batch.n_logs)
            if (first, n) not in rows:
                rows[(first, n)] = e.download_range(r.db, r.dr, first, n)
            m = r.find(q, first, n)
            assert m.n_pattern == len(TC.u16(q.pattern))
            FC.check_range(suite, rows[(first, n)], m, first, n, q)
            if q.rng is None and q.cap == FC.ALL:
                got[(q.pattern, q.nocase)] = m
    finally:
        r.close()
    return got


def _cases(name):
    if name == "find_edges":
        return FC.edge_suite()[0], FC.edge_queries()
    return {"text_edges": (TC.edge_suite(), FC.text_edge_queries()), "failed_log": (TC.failed_log_suite(), FC.failed_log_queries()), "kat": (TC.kat_suite(), FC.kat_queries())}[name]


@pytest.mark.parametrize("name", ["find_edges", "text_edges", "failed_log", "kat"])
def test_cases(eng, name):
    suite, queries = _cases(name)
    got = run_queries(eng, suite, queries)
    if name == "find_edges":
        FC.edge_hand_checks(suite, FC.edge_suite()[1], got)


@pytest.mark.parametrize("name", ["find_edges", "text_edges", "failed_log", "kat"])
def test_cases_without_elem_rank(eng_lean, name):
    suite, queries = _cases(name)
    got = run_queries(eng_lean, suite, queries)
    if name == "find_edges":
        FC.edge_hand_checks(suite, FC.edge_suite()[1], got)


def test_arguments_and_the_empty_range(eng):
    from peritext_amd.engine import PtxError

    suite = TC.failed_log_suite()
    r = Resident(eng, suite.batch, suite.table)
    try:
        m = eng.find_text(r.db, r.dr, r.ds, "a", 3, 0)  # an empty range at the end of the batch
        assert len(m.status) == 0 and len(m.n_matches) == 0 and [int(x) for x in m.hit_off] == [0] and len(m.hit_unit) == 0
        whole = eng.find_text(r.db, r.dr, r.ds, "a")
        assert len(whole.status) == 3 and whole.kernel_ms > 0
        assert np.array_equal(whole.status, eng.text(r.db, r.dr, r.ds).status), "exactly ptx_text.status of the same range"
        for kw in (dict(pattern=""), dict(pattern="a" * (abi.FIND_PATTERN_MAX + 1)), dict(pattern="a", first_log=2, n_logs=2), dict(pattern="a", first_log=4, n_logs=0)):
            with pytest.raises(PtxError) as ei:
                eng.find_text(r.db, r.dr, r.ds, **kw)
            assert ei.value.status == abi.ERR_INVALID_ARG, kw
        import ctypes as C

        pat = TC.u16("a").astype(np.uint16)
        out = abi.ptx_matches()
        for flags in (2, 0x80000000, 3):  # an unknown flag bit, alone or beside the known one
            assert eng.lib.ptx_result_find_text(eng.ctx, r.db, r.dr, r.ds, 0, 3, pat.ctypes.data_as(abi.u16p), 1, flags, 1, C.byref(out)) == abi.ERR_INVALID_ARG
        count_only = eng.find_text(r.db, r.dr, r.ds, "a", max_hits_per_log=0)
        assert np.array_equal(count_only.n_matches, whole.n_matches) and len(count_only.hit_unit) == 0 and not count_only.hit_off.any()
        empty = eng.upload_strings([])  # every value id is then beyond the table
        t = eng.find_text(r.db, r.dr, empty, "a")
        assert [int(x) for x in t.status] == [abi.ERR_BAD_OP, abi.ERR_SEQ_GAP, abi.ERR_BAD_OP] and not t.n_matches.any()
        eng.free_strings(empty)
    finally:
        r.close()


def test_value_id_beyond_the_table(eng):
    """One log with a value id equal to n_strings: PTX_ERR_BAD_OP, zero matches; its neighbours are bit-equal to the run without it."""
    suite = TC.edge_suite()
    log = [k for k, w in enumerate(suite.want) if len(w.units) == TC.T + 1][0]
    bad, _ = TC.bad_id_batch(suite, log)
    n = suite.batch.n_logs
    q = FC.Query("e")
    out = []
    for batch in (suite.batch, bad):
        r = Resident(eng, batch, suite.table)
        try:
            out.append((r.find(q, 0, n), eng.download_range(r.db, r.dr, 0, n)))
        finally:
            r.close()
    (good, rows), (m, bad_rows) = out
    FC.check_range(suite, rows, good, 0, n, q)
    assert int(good.n_matches[log]) > 0
    assert int(m.status[log]) == abi.ERR_BAD_OP and int(bad_rows.logs["status"][log]) == 0 and int(m.n_matches[log]) == 0 and int(m.hit_off[log + 1]) == int(m.hit_off[log])
    for k in range(n):
        if k != log:
            assert int(m.status[k]) == int(good.status[k]) and int(m.n_matches[k]) == int(good.n_matches[k])
            a, b, c, d = int(m.hit_off[k]), int(m.hit_off[k + 1]), int(good.hit_off[k]), int(good.hit_off[k + 1])
            for col in ("hit_unit", "hit_start", "hit_end"):
                assert getattr(m, col)[a:b].tobytes() == getattr(good, col)[c:d].tobytes(), (k, col)


def test_generated_batch(eng):
    """100 documents x 3 replicas x 512 ops in the `rich4k` mix, generated on the device, searched for a two-letter pattern of the first log's own text: against
    a Python search of Engine.text's download of the same result; one unit per element, so hit_start == hit_unit."""
    cfg = workloads.gen_config("rich4k", ops=512)
    n_docs, seed = 100, 23
    h, info = eng.generate(cfg["replicas"], cfg["ops_per_log"], cfg["mix"], cfg["mark_types"], n_docs, seed)
    dr = ds = None
    try:
        dr = eng.alloc_result(h)
        eng.merge(h, dr)
        ds = eng.upload_strings([chr(i) for i in range(128)])
        text = eng.text(h, dr, ds)
        n = len(text.status)
        assert n == 3 * n_docs and not text.status.any()
        pattern = FC.two_letters(text.text[int(text.text_off[0]) : int(text.text_off[1])])
        pat = TC.u16(pattern)
        m = eng.find_text(h, dr, ds, pattern)
        capped = eng.find_text(h, dr, ds, pattern, max_hits_per_log=2)
        assert not m.status.any() and int(m.n_matches[0]) >= 1, "the first log holds its own pattern"
        for log in range(n):
            units = text.text[int(text.text_off[log]) : int(text.text_off[log + 1])]
            hits = FC.search(units, pat)
            assert int(m.n_matches[log]) == len(hits) == int(capped.n_matches[log]), log
            assert m.of_log(log) == [(p, p, p + 2) for p in hits], log
            assert capped.of_log(log) == [(p, p, p + 2) for p in hits[:2]], log
        assert int(m.n_matches.max()) > 2, "some log has more hits than the second call lists"
    finally:
        if ds is not None:
            eng.free_strings(ds)
        if dr is not None:
            eng.free_result(dr)
        eng.free_batch(h)


def test_find_then_mark_every_mention(eng):
    """Find a word, feed every hit to Engine.change as addMark strong {startIndex: hit_start, endIndex: hit_end}, append, merge: the spans equal the oracle's
    for the same InputOperations, and every mention — and nothing else — is bold."""
    sentence = "the cat and the hat; breathe, then the end"
    values = list(sentence)
    values[4:7] = ["cat"]  # a pasted word as ONE element: element indexes are not unit offsets behind it
    base = H.mini_doc([], first_text=values)
    batch = wire.encode_docs([[base]])
    r = Resident(eng, batch, list(batch.values))
    made_h = grown_h = dr2 = None
    try:
        m = r.find(FC.Query("the"), 0, 1)
        hits = m.of_log(0)
        assert [u for u, _, _ in hits] == [0, 12, 25, 30, 35] and hits[1] == (12, 10, 13)
        marks = [{"path": ["text"], "action": "addMark", "markType": "strong", "startIndex": s, "endIndex": e} for _, s, e in hits]
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
        r.close()
    assert int(res.logs["status"][0]) == 0
    got = wire.decode_spans(grown, res, 0)
    made = H.oracle_change([[base]], calls, ["a"])
    want = H.oracle_apply([[base + made]], no_patches=True)[0][0]["spans"]
    assert H.norm_spans(got) == H.norm_spans(want)
    assert [s["text"] for s in got if s["marks"]] == ["the"] * 5 and "".join(s["text"] for s in got) == sentence
