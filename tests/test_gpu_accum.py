"""Patch streams accumulated back into canonical rows on a real MI355X, through the C ABI: ptx_accumulate_patches (records of any origin -> rows) and
ptx_check_patches (replay + accumulate on the device + compare with the merge: the third assertion of the reference's fuzzer, test/fuzz.ts:245-278, with no
record downloaded).  The cases of tests/test_emu_accum.py; expected values are the reference's spans and text from committed fixtures (tests/accum_cases.py)
through helpers.check_log — no node and no reference needed on the GPU box."""
import copy

import numpy as np
import pytest

import accum_cases as AC
import helpers as H
from peritext_amd import abi, wire

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from peritext_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_hbm():
    """every log accumulated with its state in global scratch (PTX_FLAG_ACCUM_HBM_STATE)"""
    from peritext_amd.engine import Engine

    e = Engine(0, flags=abi.FLAG_ACCUM_HBM_STATE)
    yield e
    e.close()


def merged(eng, batch):
    db = eng.upload(batch)
    dr = eng.alloc_result(db)
    eng.merge(db, dr)
    eng.sync()
    return db, dr


def stream_fn(eng):
    def f(batch):
        db, dr = merged(eng, batch)
        try:
            f.merged = eng.download(db, dr)
            return eng.replay_patches(db, dr)
        finally:
            eng.free_result(dr)
            eng.free_batch(db)
    return f


def acc_fn(eng):
    def f(batch, pat):
        db = eng.upload(batch)
        try:
            return eng.accumulate_patches(db, pat)
        finally:
            eng.free_batch(db)
    return f


def check(eng, batch, against=None):
    """check_patches of `batch` against its own merge (or the merge of `against`)"""
    db, dr = merged(eng, batch)
    other = merged(eng, against) if against is not None else None
    try:
        return eng.check_patches(db, other[1] if other else dr)
    finally:
        for h in (other, (db, dr)):
            if h:
                eng.free_result(h[1])
                eng.free_batch(h[0])


def assert_all_agree(eng, batch, res):
    rows, bad = check(eng, batch)
    assert bad == 0 and (rows["status"] == 0).all() and (rows["agrees"] == 1).all() and (rows["first_bad_record"] == 0xFFFFFFFF).all()
    assert np.array_equal(rows["digest"], res.logs["digest"])
    return rows


CASES = ["quirks"] + AC.FIXTURES
_lds_runs = {}


def run_case(name, eng):
    sf = stream_fn(eng)
    if name == "quirks":
        batch, pat, res, _ = AC.run_quirks(sf, acc_fn(eng))
    else:
        batch, pat, res = AC.run_fixture(name, sf, acc_fn(eng))
    assert np.array_equal(res.logs["digest"], sf.merged.logs["digest"]) and np.array_equal(res.logs["n_elems"], sf.merged.logs["n_elems"])
    return batch, pat, res


@pytest.mark.parametrize("name", CASES)
def test_streams_rebuild_the_reference_documents(eng, name):
    """Cases 1 to 3 of the issue (the chunk-edge document with the quirk, boundary, KAT and trace streams in one batch; the fixtures): rows, counts and digests
    of the accumulated streams are the reference's; and ptx_check_patches agrees on every log of the same batches (case 7)."""
    batch, pat, res = run_case(name, eng)
    _lds_runs[name] = res
    rows = assert_all_agree(eng, batch, res)
    assert np.array_equal(rows["n_patches"], pat.logs["n_patches"])


@pytest.mark.parametrize("name", CASES)
def test_state_in_global_scratch_gives_identical_rows(eng, eng_hbm, name):
    """Case 4: the same under PTX_FLAG_ACCUM_HBM_STATE — the reference's documents again, and row for row what the LDS store wrote."""
    batch, pat, res = run_case(name, eng_hbm)
    lds = _lds_runs.get(name) or run_case(name, eng)[2]
    for f in ("status", "n_elems", "n_visible", "n_spans", "n_cintervals", "digest"):
        assert np.array_equal(res.logs[f], lds.logs[f]), f
    assert np.array_equal(res.values, lds.values) and np.array_equal(res.spans, lds.spans) and np.array_equal(res.cintervals, lds.cintervals)
    assert_all_agree(eng_hbm, batch, res)


def test_failed_log_beside_good_ones(eng, eng_hbm):
    for e in (eng, eng_hbm):
        AC.run_failed_log(stream_fn(e), acc_fn(e))
    # ... and through ptx_check_patches: the merge status, no stream, not counted as a disagreement
    gen = AC._fixture("ptxgen_mini.json")
    logs = [copy.deepcopy(l) for l in gen["docs"][0]["logs"]]
    logs[1][5]["seq"] += 1
    rows, bad = check(eng, wire.encode_docs([logs]))
    assert [int(x) for x in rows["status"]] == [0, abi.ERR_SEQ_GAP, 0] and [int(x) for x in rows["agrees"]] == [1, 0, 1] and bad == 0
    assert [int(x) for x in rows["digest"][1]] == [0, 0]


def test_foreign_streams(eng):
    """Case 6: folded deletes (b > 1) give the same rows; one tampered record fails that log alone, at that record; a dropped DELETE is another document."""
    AC.run_foreign_streams(stream_fn(eng), acc_fn(eng))


def test_foreign_streams_state_in_global_scratch(eng_hbm):
    AC.run_foreign_streams(stream_fn(eng_hbm), acc_fn(eng_hbm))


def _twin(batch):
    """The same batch with another value in the insert row of first-text character 5 of document 1 (it survives): same structure, one value differs."""
    twin = copy.copy(batch)
    twin.payload = batch.payload.copy()
    row = int(batch.log_off[0]) + 1 + 5
    assert int(batch.action[row]) == abi.ACT_INSERT
    twin.payload[row] = batch.payload[row + 1]
    assert twin.payload[row] != batch.payload[row]
    return twin


def test_check_patches_finds_the_log_whose_merge_differs(eng, eng_hbm):
    docs, _ = AC.quirk_case()
    batch = wire.encode_docs(docs)
    for e in (eng, eng_hbm):
        rows, bad = check(e, batch, against=_twin(batch))
        assert bad == 1 and [int(x) for x in np.flatnonzero(rows["agrees"] == 0)] == [0] and (rows["status"] == 0).all()


def test_check_patches_needs_elem_rank():
    from peritext_amd.engine import Engine, PtxError

    docs, _ = AC.fixture_case("patches_mini.json")
    with Engine(0, flags=abi.FLAG_NO_ELEM_RANK) as e:
        db, dr = merged(e, wire.encode_docs(docs))
        try:
            with pytest.raises(PtxError) as err:
                e.check_patches(db, dr)
            assert err.value.status == abi.ERR_INVALID_ARG
        finally:
            e.free_result(dr)
            e.free_batch(db)


def test_check_patches_on_the_chunked_pack_path(eng, monkeypatch):
    """PTX_REPLAY_PACK_RECORDS=64: the packed copy holds a few logs at a time and is accumulated range by range — the same answers."""
    docs, _ = AC.quirk_case()
    batch = wire.encode_docs(docs)
    whole, bad0 = check(eng, batch)
    twin_rows, _ = check(eng, batch, against=_twin(batch))
    monkeypatch.setenv("PTX_REPLAY_PACK_RECORDS", "64")
    rows, bad = check(eng, batch)
    assert bad == bad0 == 0 and np.array_equal(rows, whole)
    rows, bad = check(eng, batch, against=_twin(batch))
    assert bad == 1 and np.array_equal(rows, twin_rows)
