"""The row index of a resident batch (merge_core.h ptx_row_index_off) on the GPU: the first merge of a batch classifies and checks its rows and leaves
the lists behind, the later ones read them back — and every answer is still the oracle's.  The logs are those of tests/test_emu_row_index.py
(tests/row_index_cases.py: 1 to 1 025 rows at the edges of the indexed pass) and of tests/adm_mark_cases.py (96 to 1 100 ops, some inadmissible).  Nothing
expected here comes from this library: a second and a third merge are compared with the oracle like the first.

What this file shows is that the ANSWERS do not depend on the index, and — through ptx_debug_row_index, a test hook of the library outside its C ABI — that the
host really hands the index out: who wrote it, that every log that passes is indexed after the first eligible merge, and that the batches which must have none
have none.  That a reading merge then takes no full row pass inside the kernel is shown by the emulation twin, which counts the passes."""
import ctypes as C

import numpy as np
import pytest

import adm_mark_cases as M
import helpers as H
import row_index_cases as R
from peritext_amd import abi, wire

pytestmark = pytest.mark.gpu
NO_RANK = abi.FLAG_NO_ELEM_RANK


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch  # (first, as in the other GPU modules: the wrapped batch below lives in torch tensors)

    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    assert H.have_node(), "these cases need node, the oracle's runtime"


def _engine(flags=0, threads=0):
    from peritext_amd.engine import Engine

    e = Engine(0, flags=flags)
    if threads:
        e.set_launch_shape(threads, 0)
    return e


def _index(e, db):
    """-> (state, logs indexed): -1 = the batch has no index; 0 nobody has written it; 2 / 3 written (the writing merge has / has not been seen to end)."""
    f = e.lib.ptx_debug_row_index
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    n = C.c_uint32(0)
    return int(f(e.ctx, db, C.byref(n))), int(n.value)


def _merge(e, db):
    dr = e.alloc_result(db)
    try:
        e.merge(db, dr)
        return e.download(db, dr)
    finally:
        e.free_result(dr)


def _same(a, b):
    for k in ("logs", "values", "spans", "cintervals", "elem_rank"):
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()), k


def _check_shapes(batch, exp, res):
    for l, x in enumerate(exp):
        H.check_log(batch, res, l, x)


@pytest.mark.parametrize("flags,force,threads,kernel", [(0, 0, 128, ("ptx_merge_kernel_w7", "ptx_merge_kernel")), (NO_RANK, 0, 64, ("ptx_merge_kernel_lean64",)),
                                                        (NO_RANK, 0, 128, ("ptx_merge_kernel_lean128",)), (NO_RANK, 192, 192, ("ptx_merge_kernel_lean192",))],
                         ids=["general", "lean64", "lean128", "lean192"])
def test_three_merges_of_one_batch_answer_like_the_oracle_every_time(flags, force, threads, kernel):
    """The writer, then two readers, per build: the shapes at the edges of the indexed pass (the one-wave build: those of up to 512 rows) and the logs of the
    admission marks' cases, whose inadmissible ones fail identically all three times.  The build a batch takes is what it was without an index."""
    batch, exp, _ = R.shapes(R.SHORT if threads == 64 else None)
    cs = M.cases(1100, 350 if threads == 64 else None)
    with _engine(flags, force) as e:
        db, dg = e.upload(batch), e.upload(cs["grown"])
        try:
            names = (e.batch_kernel_name(db), e.batch_kernel_name(dg))
            assert names[0] in kernel and names[1] in kernel and e.launch_shape(db)[0] == threads
            assert _index(e, db) == (0, 0)
            runs = [_merge(e, db)]
            assert _index(e, db) == (2, batch.n_logs), "the first merge wrote the index of every log (all of them pass)"
            runs += [_merge(e, db) for _ in range(2)]
            grown = [_merge(e, dg) for _ in range(3)]
            st, n_ix = _index(e, dg)  # (every log whose changes are admissible passes the row pass and is indexed)
            assert st == 2 and sum(1 for c in cs["cases"] if not c["code"]) <= n_ix <= cs["grown"].n_logs
            assert (e.batch_kernel_name(db), e.batch_kernel_name(dg)) == names
        finally:
            e.free_batch(db)
            e.free_batch(dg)
    for r in runs:
        _check_shapes(batch, exp, r)
    _same(runs[0], runs[1])
    _same(runs[0], runs[2])
    for r in grown:
        for l, c in enumerate(cs["cases"]):
            M.check_grown(c, cs["grown"], r, l)
    _same(grown[0], grown[1])
    _same(grown[0], grown[2])


def test_a_readmit_context_first_then_a_plain_one():
    """A PTX_FLAG_READMIT context neither writes nor reads the index: the batch's first merge through it, then a plain context (the writer, then a reader), then
    the READMIT context again — the same answers, the oracle's."""
    batch, exp, _ = R.shapes()
    with _engine(NO_RANK | abi.FLAG_READMIT) as f, _engine(NO_RANK) as e:
        db = e.upload(batch)
        try:
            runs = [_merge(f, db)]
            assert _index(f, db) == (0, 0), "a READMIT context writes nothing"
            runs += [_merge(e, db)]
            assert _index(e, db) == (2, batch.n_logs)
            runs += [_merge(e, db), _merge(f, db)]
            assert _index(f, db) == (2, batch.n_logs), "... and asks nothing about it"
        finally:
            e.free_batch(db)
    _check_shapes(batch, exp, runs[0])
    _check_shapes(batch, exp, runs[2])
    for r in runs[1:]:
        _same(runs[0], r)


def test_a_second_context_on_another_stream_right_behind_the_writer():
    """Two contexts, each on its own stream, no host synchronisation between their launches: the second neither reads nor writes the index while the writer may
    still run (it parks in its own result), and reads it once the writer has ended.  The oracle's answers from both, every time."""
    batch, exp, _ = R.shapes()
    with _engine(NO_RANK) as e1, _engine(NO_RANK) as e2:
        db = e1.upload(batch)
        r1, r2 = e1.alloc_result(db), e2.alloc_result(db)
        try:
            outs = []
            for _ in range(3):
                e1.merge(db, r1)
                e2.merge(db, r2)
                outs.append((e1.download(db, r1), e2.download(db, r2)))
            assert _index(e2, db) == (3, batch.n_logs), "the second context has learnt from the writer's event that the index stands"
        finally:
            e1.free_result(r1)
            e2.free_result(r2)
            e1.free_batch(db)
    for a, b in outs:
        _check_shapes(batch, exp, a)
        _check_shapes(batch, exp, b)
        _same(outs[0][0], a)
        _same(outs[0][0], b)


def test_an_append_starts_with_an_empty_index():
    """The grown batch of an append has an index of its own, empty: merged twice (writer, reader), the oracle's answers each time; the base, merged before and
    after, is as it was."""
    cs = M.cases(1100)
    grown, cases = cs["grown"], cs["cases"]
    head, tail = wire.split_batch(grown, [c["m"] for c in cases])
    with _engine(NO_RANK) as e:
        dh = e.upload(head)
        dg = None
        try:
            rh = [_merge(e, dh), _merge(e, dh)]
            dg = e.append(dh, tail)
            r1, r2 = _merge(e, dg), _merge(e, dg)
            rh.append(_merge(e, dh))
        finally:
            if dg is not None:
                e.free_batch(dg)
            e.free_batch(dh)
    for r in (r1, r2):
        for l, c in enumerate(cases):
            M.check_grown(c, grown, r, l)
    _same(r1, r2)
    _same(rh[0], rh[1])
    _same(rh[0], rh[2])


def test_wrapped_batches_and_wide_keys_have_no_index():
    """A batch wrapped around caller-owned device columns, and a batch that holds a log whose id keys pass 16 bits: merged twice each, the oracle's answers."""
    import torch

    batch, exp, _ = R.shapes()
    gen = H.oracle_gen("mini", 2, 5, 300, 3)
    docs = [d["logs"] for d in gen["docs"]]
    narrow, wide = wire.encode_docs(docs), wire.encode_docs(H.shift_counters(docs, 70000))  # (the same histories, every op counter 70 000 higher)
    narrow_exp = [x for d in gen["docs"] for x in d["expected"]]
    with _engine(0) as e:
        cols = {}
        for k in ("log_off", "op_id", "ref_a", "ref_b", "payload", "action", "mark_type", "side_a", "side_b"):
            x = getattr(batch, k)
            as_signed = {np.dtype("uint64"): np.int64, np.dtype("uint32"): np.int32, np.dtype("uint8"): np.uint8}[x.dtype]
            pad = np.zeros(8, dtype=x.dtype)  # (the byte columns are read a dword at a time)
            cols[k] = torch.from_numpy(np.concatenate([x, pad]).view(as_signed).copy()).cuda()
        torch.cuda.synchronize()
        dw = e.wrap_device(batch.n_logs, batch.n_ops, {k: v.data_ptr() for k, v in cols.items()})
        dk, dn = e.upload(wide), e.upload(narrow)
        try:
            w1, w2 = _merge(e, dw), _merge(e, dw)
            k1, k2 = _merge(e, dk), _merge(e, dk)
            assert _index(e, dw)[0] == -1 and _index(e, dk)[0] == -1
            n1 = _merge(e, dn)
        finally:
            e.free_batch(dw)
            e.free_batch(dk)
            e.free_batch(dn)
        del cols
    _check_shapes(batch, exp, w1)
    _same(w1, w2)
    assert (int(wide.log_hdr["max_counter"].max()) + 1) * (int(wide.log_hdr["max_actor"].max()) + 1) > 65536
    for l, x in enumerate(narrow_exp):
        H.check_log(narrow, n1, l, x)
        assert wire.decode_spans(wide, k1, l) == wire.decode_spans(narrow, n1, l)
    assert (k1.logs["status"] == 0).all() and (k1.logs["digest"] == n1.logs["digest"]).all()
    _same(k1, k2)
