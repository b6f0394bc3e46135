"""change() through the C ABI on a real MI355X at the edges of its wave-wide list walks (tests/change_probe.py: the probe harness and the case tables shared
with tests/test_emu_change_edges.py): ptx_gen_select across 64-lane ballots (A), ptx_gen_after_tombstones across chunks anchored at pos + 1 (B), the 16-byte-block
gap opener ptx_list_shift_up (C: the device build has no CPU twin, this file is its check), this call's own elements and tombstones (D), several replicas and
logs of very different sizes in one launch (E), and all of A - D again with the element list in global scratch (F: PTX_CHANGE_LIST_IN_HBM).  Every made Change
is compared with the oracle's, Change for Change; what was made is appended on the device (ptx_batch_append_device), merged, and the spans of every grown
replica are compared with the oracle applying log + wanted Changes."""
import os

import pytest

import change_probe as CP
import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    assert H.have_node(), "these cases need node, the oracle's runtime: a skipped case would hide exactly what this file exists to show"
    from peritext_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(params=[False, True], ids=["lds", "hbm"])
def list_in_hbm(request):
    """F: the library reads PTX_CHANGE_LIST_IN_HBM per call"""
    old = os.environ.pop("PTX_CHANGE_LIST_IN_HBM", None)
    if request.param:
        os.environ["PTX_CHANGE_LIST_IN_HBM"] = "1"
    yield request.param
    os.environ.pop("PTX_CHANGE_LIST_IN_HBM", None)
    if old is not None:
        os.environ["PTX_CHANGE_LIST_IN_HBM"] = old


class GpuBackend:
    def __init__(self, eng):
        self.eng = eng

    def change_and_grow(self, batch, ops):
        e = self.eng
        tables = (batch.values, batch.urls, batch.log_doc, batch.doc_actors, batch.doc_comments, batch.keys, batch.map_values)
        db = e.upload(batch)
        dr = e.alloc_result(db)
        made_h = grown_h = dr2 = None
        try:
            e.merge(db, dr)
            e.sync()
            made_h, status = e.change(db, dr, ops)
            made = e.download_batch(made_h, *tables)
            grown_h = e.append_device(db, made_h)
            dr2 = e.alloc_result(grown_h)
            e.merge(grown_h, dr2)
            e.sync()
            grown = e.download_batch(grown_h, *tables)
            res = e.download(grown_h, dr2)
        finally:
            for h in (dr, dr2):
                if h is not None:
                    e.free_result(h)
            for h in (db, made_h, grown_h):
                if h is not None:
                    e.free_batch(h)
        return made, status, grown, res


@pytest.mark.parametrize("family", sorted(CP.FAMILIES))
def test_single_replica_families(eng, family, list_in_hbm):
    """A: select across chunks (+ out-of-bounds logs beside good ones), B: lookAfterTombstones across chunks, C: the gap opener, D: this call's own elements"""
    CP.run_cases(GpuBackend(eng), CP.FAMILIES[family]())


def test_generated_replicas_every_replica_edits(eng, list_in_hbm):
    docs, calls, actors = CP.family_E_generated()
    want = CP.run(GpuBackend(eng), docs, calls, actors, expect_status=[0] * len(actors))
    assert all(w["error"] is None and len(w["changes"]) == 10 for w in want)  # no case dropped
    assert any(len(c["deps"]) == 3 for w in want for c in w["changes"])        # the deps name the other actors


def test_mixed_sizes_in_one_batch(eng, list_in_hbm):
    docs, calls, actors = CP.family_E_mixed()
    CP.run(GpuBackend(eng), docs, calls, actors, expect_status=[0, 0, 0, 0])
