"""change() from resident InputOperations through the C ABI on a real MI355X (ptx_input_ops_upload / _wrap_device / _download, ptx_change_device).
(a) oracle parity on the change() edge families of tests/change_probe.py, Change for Change and span for span, with the element lists in LDS and in HBM;
(b) on the same cases the made batch and the status equal Engine.change's of the same ops, column for column, through an upload and through torch tensors that
are wrapped; (c) every invalid input of tests/change_prep_cases.py is PTX_ERR_INVALID_ARG from ptx_change AND from ptx_change_device, nothing is made, and the
context goes on working; (d) the offsets of the made batch at the scan's chunk edges; (e) upload and download round trip."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

import change_prep_cases as PC
import change_probe as CP
import helpers as H
from peritext_amd import abi, wire

pytestmark = pytest.mark.gpu

BATCH_COLUMNS = ("log_off", "op_id", "ref_a", "ref_b", "payload", "action", "mark_type", "side_a", "side_b", "chg_off", "chg_hdr", "chg_env", "chg_env_hi", "log_hdr")
OPS_ARRAYS = ("chg_off", "op_off", "action", "mark_type", "index", "count", "payload", "values", "actor")


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from peritext_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(params=[False, True], ids=["lds", "hbm"])
def list_in_hbm(request):
    """the library reads PTX_CHANGE_LIST_IN_HBM per call"""
    old = os.environ.pop("PTX_CHANGE_LIST_IN_HBM", None)
    if request.param:
        os.environ["PTX_CHANGE_LIST_IN_HBM"] = "1"
    yield request.param
    os.environ.pop("PTX_CHANGE_LIST_IN_HBM", None)
    if old is not None:
        os.environ["PTX_CHANGE_LIST_IN_HBM"] = old


def same_batch(a, b, what):
    assert (a.n_logs, a.n_ops, a.max_actors) == (b.n_logs, b.n_ops, b.max_actors), what
    for f in BATCH_COLUMNS:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), "%s: %s" % (what, f)
        if x is not None:
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), "%s: %s" % (what, f)


def wrap_tensors(eng, ops):
    """`ops` as torch tensors on the device, wrapped: (handle, the tensors — to be kept alive while the handle is)."""
    import torch

    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint8): np.uint8}
    keep, ptrs = [], {}
    for f in OPS_ARRAYS:
        a = getattr(ops, f)
        if a is None:
            continue
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a.view(signed[a.dtype]).copy()).to("cuda:0") if len(a) else torch.zeros(4, dtype=torch.uint8, device="cuda:0")
        keep.append(t)
        ptrs[f] = t.data_ptr()
    torch.cuda.synchronize()
    n_logs = len(ops.chg_off) - 1
    nc = int(ops.chg_off[n_logs]) if n_logs else 0
    h = eng.wrap_input_ops(n_logs, nc, int(ops.op_off[nc]) if nc else 0, 0 if ops.values is None else len(ops.values), ops.max_actors, ptrs)
    return h, keep


class DeviceBackend:
    """change_probe's backend over upload_input_ops / wrap_input_ops -> change_device; beside it Engine.change of the same ops, for (b)."""

    def __init__(self, eng, wrap):
        self.eng, self.wrap, self.compared = eng, wrap, 0

    def change_and_grow(self, batch, ops):
        e = self.eng
        tables = (batch.values, batch.urls, batch.log_doc, batch.doc_actors, batch.doc_comments, batch.keys, batch.map_values)
        db = e.upload(batch)
        dr = e.alloc_result(db)
        made_h = host_h = grown_h = dr2 = h = keep = None
        try:
            e.merge(db, dr)
            e.sync()
            h, keep = wrap_tensors(e, ops) if self.wrap else (e.upload_input_ops(ops), None)
            made_h, status = e.change_device(db, dr, h)
            made = e.download_batch(made_h, *tables)
            host_h, host_status = e.change(db, dr, ops)
            assert np.array_equal(status, host_status), "status_out is ptx_change's"
            same_batch(made, e.download_batch(host_h, *tables), "the made batch is ptx_change's")
            self.compared += 1
            grown_h = e.append_device(db, made_h)
            dr2 = e.alloc_result(grown_h)
            e.merge(grown_h, dr2)
            e.sync()
            grown = e.download_batch(grown_h, *tables)
            res = e.download(grown_h, dr2)
        finally:
            if h is not None:
                e.free_input_ops(h)
            del keep
            for r in (dr, dr2):
                if r is not None:
                    e.free_result(r)
            for b in (db, made_h, host_h, grown_h):
                if b is not None:
                    e.free_batch(b)
        return made, status, grown, res


def _node():
    assert H.have_node(), "these cases need node, the oracle's runtime: a skipped case would hide exactly what this file exists to show"


@pytest.mark.parametrize("wrap", [False, True], ids=["upload", "wrap"])
@pytest.mark.parametrize("family", sorted(CP.FAMILIES))
def test_single_replica_families(eng, family, list_in_hbm, wrap):
    """(a), (b): select across chunks (+ out-of-bounds logs beside good ones), lookAfterTombstones across chunks, the gap opener, this call's own elements"""
    _node()
    b = DeviceBackend(eng, wrap)
    CP.run_cases(b, CP.FAMILIES[family]())
    assert b.compared == 1


@pytest.mark.parametrize("wrap", [False, True], ids=["upload", "wrap"])
def test_generated_replicas_every_replica_edits(eng, list_in_hbm, wrap):
    _node()
    docs, calls, actors = CP.family_E_generated()
    b = DeviceBackend(eng, wrap)
    want = CP.run(b, docs, calls, actors, expect_status=[0] * len(actors))
    assert all(w["error"] is None and len(w["changes"]) == 10 for w in want) and b.compared == 1  # no case dropped


@pytest.mark.parametrize("wrap", [False, True], ids=["upload", "wrap"])
def test_mixed_sizes_in_one_batch(eng, list_in_hbm, wrap):
    _node()
    docs, calls, actors = CP.family_E_mixed()
    b = DeviceBackend(eng, wrap)
    CP.run(b, docs, calls, actors, expect_status=[0, 0, 0, 0])
    assert b.compared == 1


# ---- (c), (d): a base batch of L copies of one replica of six visible elements ----
class Tiled:
    def __init__(self, eng, L):
        self.eng = eng
        self.one = wire.encode_docs([[H.mini_doc([], first_text=list("abcdef"))]])
        assert len(self.one.values) >= 6
        self.db = eng.upload(self.one, copies=L)
        self.dr = eng.alloc_result(self.db)
        eng.merge(self.db, self.dr)
        eng.sync()

    def ops_of(self, c):
        return dataclasses.replace(c.ops, max_actors=max(self.one.max_actors, 1), actor=np.zeros(c.n_logs, np.uint32))

    def free(self):
        self.eng.free_result(self.dr)
        self.eng.free_batch(self.db)


@pytest.fixture(scope="module")
def tiled(eng):
    made = {}

    def get(L):
        if L not in made:
            made[L] = Tiled(eng, L)
        return made[L]

    yield get
    for t in made.values():
        t.free()


def _struct(eng, c, ops):
    s = eng._input_ops_struct(ops)
    s.n_values = c.values_count()
    if not c.has_values:
        s.values = C.cast(None, abi.u32p)
    return s


def _error(eng):
    return (eng.lib.ptx_last_error(eng.ctx) or b"").decode()


def test_invalid_inputs_fail_both_calls(eng, tiled):
    """(c): every invalid input of the emulation's table.  ptx_change finds it walking the arrays on the host, ptx_change_device on the device at its first wait:
    both PTX_ERR_INVALID_ARG, `made` NULL, status_out untouched, the message naming the LOWEST offending entry or log; a valid call on the same context succeeds
    afterwards."""
    cases = PC.invalid_cases()
    assert len(cases) == 7 + 2 + 2 * 5 + 2
    for c in cases:
        t = tiled(c.n_logs)
        ops = t.ops_of(c)
        s = _struct(eng, c, ops)
        status = np.full(c.n_logs, 0xA5A5A5A5, np.uint32)
        made = C.c_void_p(0x1234)
        assert eng.lib.ptx_change(eng.ctx, t.db, t.dr, C.byref(s), C.byref(made), status.ctypes.data_as(abi.u32p)) == abi.ERR_INVALID_ARG, c.name
        assert not made.value, c.name
        h = C.c_void_p()
        assert eng.lib.ptx_input_ops_upload(eng.ctx, C.byref(s), C.byref(h)) == 0, c.name + ": the upload validates nothing"
        try:
            made = C.c_void_p(0x1234)
            assert eng.lib.ptx_change_device(eng.ctx, t.db, t.dr, h, C.byref(made), status.ctypes.data_as(abi.u32p)) == abi.ERR_INVALID_ARG, c.name
            assert not made.value and (status == 0xA5A5A5A5).all(), c.name
            code, at = c.want_error
            msg = _error(eng)
            if code in (PC.CHG_ORDER, PC.OP_ORDER):
                assert msg.endswith("decreases at entry %d" % at) and ("chg_off" if code == PC.CHG_ORDER else "op_off") in msg, (c.name, msg)
            elif code in (PC.VALUES, PC.ROWS):
                assert msg.endswith("(log %d)" % at), (c.name, msg)
            else:
                assert "must start at 0" in msg, (c.name, msg)
        finally:
            eng.lib.ptx_input_ops_free(eng.ctx, h)
    # sizes that are the caller's word and do not agree with the arrays: the device call alone can be asked
    for c in PC.wrapped_size_cases():
        t = tiled(c.n_logs)
        h, keep = wrap_tensors(eng, t.ops_of(c))
        eng.free_input_ops(h)
        ptrs = {f: k.data_ptr() for f, k in zip(OPS_ARRAYS, keep)}
        h = eng.wrap_input_ops(c.n_logs, c.sizes[0], c.sizes[1], c.values_count(), max(t.one.max_actors, 1), ptrs)
        try:
            made, status = C.c_void_p(0x1234), np.full(c.n_logs, 0xA5A5A5A5, np.uint32)
            assert eng.lib.ptx_change_device(eng.ctx, t.db, t.dr, h, C.byref(made), status.ctypes.data_as(abi.u32p)) == abi.ERR_INVALID_ARG, c.name
            assert not made.value and (status == 0xA5A5A5A5).all() and "does not end at the size" in _error(eng), c.name
        finally:
            eng.free_input_ops(h)
            del keep
    # the context goes on working
    c = PC.many_logs_case(1)
    t = tiled(1)
    h = eng.upload_input_ops(t.ops_of(c))
    try:
        made_h, status = eng.change_device(t.db, t.dr, h)
        assert not status.any() and eng.download_batch(made_h).n_ops == int(PC.per_log(c)[0][0]) > 0
        eng.free_batch(made_h)
    finally:
        eng.free_input_ops(h)


@pytest.mark.parametrize("n_logs", PC.MANY)
def test_offsets_of_the_made_batch_at_the_scan_chunk_edges(eng, tiled, n_logs, list_in_hbm):
    """(d): batches of 1, 1 023, 1 024, 1 025 and 2 049 logs, most of them idle; every busy log makes one op its replica accepts.  log_off and chg_off of the
    made batch against np.cumsum of the cases' row counts — the numpy ones the emulation is held to on the CPU — and of the Changes asked for; the batch equal to
    ptx_change's."""
    c = PC.many_logs_case(n_logs)
    t = tiled(n_logs)
    ops = t.ops_of(c)
    rows = PC.per_log(c)[0].astype(np.uint32)  # numpy: no GPU test process may load an emulation library (tests/test_gpu_parity.py); test_emu_change_prep.py holds the emulation to these counts
    h = eng.upload_input_ops(ops)
    made_h = host_h = None
    try:
        made_h, status = eng.change_device(t.db, t.dr, h)
        host_h, host_status = eng.change(t.db, t.dr, ops)
        assert not status.any() and not host_status.any(), "every op is one the replica accepts"
        made = eng.download_batch(made_h)
        assert np.array_equal(made.log_off, np.concatenate([[0], np.cumsum(rows.astype(np.uint64))]).astype(np.uint64))
        assert np.array_equal(made.chg_off, ops.chg_off) and made.n_ops == int(rows.sum()) > 0
        same_batch(made, eng.download_batch(host_h), "%d logs" % n_logs)
    finally:
        eng.free_input_ops(h)
        for b in (made_h, host_h):
            if b is not None:
                eng.free_batch(b)


def test_upload_and_download_round_trip(eng):
    """(e): download_input_ops(upload_input_ops(x)) == x, array for array; the same through wrapped tensors; a NULL `values` stays NULL."""
    cases = PC.lane_edge_cases() + [PC.many_logs_case(1025)]
    assert any(c.n_logs == 0 for c in cases)
    for c in cases:
        x = dataclasses.replace(c.ops, max_actors=3, actor=(np.arange(c.n_logs, dtype=np.uint32) * 5) % 3)
        for wrap in (False, True):
            h, keep = wrap_tensors(eng, x) if wrap else (eng.upload_input_ops(x), None)
            try:
                y = eng.download_input_ops(h)
            finally:
                eng.free_input_ops(h)
                del keep
            assert y.max_actors == x.max_actors, c.name
            for f in OPS_ARRAYS:
                a, b = getattr(x, f), getattr(y, f)
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), "%s: %s (%s)" % (c.name, f, "wrap" if wrap else "upload")
    x = dataclasses.replace(PC.limit_cases()[5].ops, values=None)
    h = eng.upload_input_ops(x)
    try:
        y = eng.download_input_ops(h)
    finally:
        eng.free_input_ops(h)
    assert len(y.values) == 0 and y.action.tolist() == [abi.IN_INSERT] and y.count.tolist() == [0]
