"""Document text assembled on the device through the C ABI on a real MI355X (ptx_strings_upload -> ptx_merge -> ptx_result_text_range): the cases of
tests/test_emu_text.py with the expected values of tests/text_cases.py (the oracle's spans, the reference's known answers, one hand-written literal), on a
default context and on a PTX_FLAG_NO_ELEM_RANK one, and one batch generated on the device in the `rich4k` mix."""
import numpy as np
import pytest

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

    def text(self, first, n):
        return self.eng.download_range(self.db, self.dr, first, n), self.eng.text(self.db, self.dr, self.ds, first, n)

    def close(self):
        self.eng.free_strings(self.ds)
        self.eng.free_result(self.dr)
        self.eng.free_batch(self.db)


def run_suite(e, suite):
    r = Resident(e, suite.batch, suite.table)
    try:
        for first, n in [(0, suite.batch.n_logs)] + suite.ranges:
            res, text = r.text(first, n)
            TC.check_range(suite, res, text, first, n)
    finally:
        r.close()


@pytest.mark.parametrize("name", ["edges", "big_table", "failed_log", "kat"])
def test_cases(eng, name):
    run_suite(eng, {s.name: s for s in TC.suites()}[name])


@pytest.mark.parametrize("name", ["edges", "big_table", "failed_log", "kat"])
def test_cases_without_elem_rank(eng_lean, name):
    run_suite(eng_lean, {s.name: s for s in TC.suites()}[name])


def test_ranges_and_arguments(eng):
    suite = TC.failed_log_suite()
    r = Resident(eng, suite.batch, suite.table)
    try:
        text = eng.text(r.db, r.dr, r.ds, 3, 0)  # an empty range at the end of the batch
        assert len(text.status) == 0 and len(text.text) == 0 and [int(x) for x in text.text_off] == [0] and [int(x) for x in text.span_off] == [0]
        whole = eng.text(r.db, r.dr, r.ds)
        assert len(whole.status) == 3 and whole.kernel_ms > 0
        from peritext_amd.engine import PtxError

        for first, n in ((2, 2), (4, 0)):
            with pytest.raises(PtxError) as ei:
                eng.text(r.db, r.dr, r.ds, first, n)
            assert ei.value.status == abi.ERR_INVALID_ARG
        empty = eng.upload_strings([])  # n_strings == 0 is legal: every value id is then beyond the table
        t = eng.text(r.db, r.dr, empty)
        assert [int(x) for x in t.status] == [abi.ERR_BAD_OP, abi.ERR_SEQ_GAP, abi.ERR_BAD_OP] and len(t.text) == 0
        eng.free_strings(empty)
    finally:
        r.close()


def test_value_id_beyond_the_table(eng):
    """One log with a value id equal to n_strings reports PTX_ERR_BAD_OP (a reported status: the id is checked before the table is read) and has no text;
    its neighbours are bit-equal to the run without it.  The emulation and its sanitizer program pass the same case (tests/test_emu_text.py)."""
    suite = TC.edge_suite()
    log = [k for k, w in enumerate(suite.want) if len(w.units) == TC.T + 1][0]
    bad, _ = TC.bad_id_batch(suite, log)
    n = suite.batch.n_logs
    good = Resident(eng, suite.batch, suite.table)
    try:
        _, good_text = good.text(0, n)
    finally:
        good.close()
    r = Resident(eng, bad, suite.table)
    try:
        res, text = r.text(0, n)
    finally:
        r.close()
    assert int(text.status[log]) == abi.ERR_BAD_OP and int(res.logs["status"][log]) == 0
    assert int(text.text_off[log + 1]) == int(text.text_off[log]), "no text"
    assert np.array_equal(text.span_off, good_text.span_off) and not text.span_unit[int(text.span_off[log]) : int(text.span_off[log + 1])].any()
    for k in range(n):
        if k != log:
            assert int(text.status[k]) == int(good_text.status[k])
            a = text.text[int(text.text_off[k]) : int(text.text_off[k + 1])]
            assert a.tobytes() == good_text.text[int(good_text.text_off[k]) : int(good_text.text_off[k + 1])].tobytes(), k
            sa = text.span_unit[int(text.span_off[k]) : int(text.span_off[k + 1])]
            assert sa.tobytes() == good_text.span_unit[int(good_text.span_off[k]) : int(good_text.span_off[k + 1])].tobytes(), k


@pytest.mark.parametrize("n_codes", [128, 65536])
def test_generated_batch(eng, n_codes):
    """8 documents x 3 replicas x 512 ops in the `rich4k` mix, generated on the device: its insert payloads are character codes, so a table of 128 one-unit
    strings (or 65 536 of them) serves it.  Against a Python join of the downloaded value ids, and against the oracle for 2 documents."""
    cfg = workloads.gen_config("rich4k", ops=512)
    n_docs, seed = 8, 11
    h, info = eng.generate(cfg["replicas"], cfg["ops_per_log"], cfg["mix"], cfg["mark_types"], n_docs, seed)
    dr = ds = None
    try:
        actors, comments, log_doc = wire.generated_tables(n_docs, cfg["replicas"], info["n_comments"])
        batch = eng.download_batch(h, wire.GEN_VALUES, wire.GEN_URLS, log_doc, actors, comments)
        dr = eng.alloc_result(h)
        eng.merge(h, dr)
        ds = eng.upload_strings([chr(i) for i in range(n_codes)])
        res, text = eng.download(h, dr), eng.text(h, dr, ds)
        assert (res.logs["status"] == 0).all() and not text.status.any() and np.array_equal(text.span_off, res.span_off)
        assert np.array_equal(text.text_off, res.value_off), "one unit per element"
        for log in range(batch.n_logs):
            v, s, _ = wire.canonical_of_log(batch, res, log)
            assert text.of_log(log) == "".join(chr(int(x)) for x in v), log
            assert [int(x) for x in text.span_unit[int(text.span_off[log]) : int(text.span_off[log + 1])]] == [int(x["start"]) for x in s], log
        gen = H.oracle_gen("rich4k", docs=2, seed=seed, ops=512)
        log = 0
        for d in gen["docs"]:
            for exp in d["expected"]:
                assert int(res.logs["n_visible"][log]) > 64
                assert H.norm_spans(wire.decode_spans_text(batch, res, text, log)) == H.norm_spans(exp["spans"]), log
                log += 1
    finally:
        if ds is not None:
            eng.free_strings(ds)
        if dr is not None:
            eng.free_result(dr)
        eng.free_batch(h)
