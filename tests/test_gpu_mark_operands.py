"""The operand words of a resident batch's mark ops (merge_core.h ptx_mark_operand_pack) on the GPU: the first merge of a batch writes them from P5a's
registers, the later ones run P5a on them — and every answer is still the oracle's.  The logs are those of tests/test_emu_mark_operands.py
(tests/mark_operand_cases.py: 0 to 385 mark ops at the edges of P5a's blocks and steps, every kind of operand, logs that fail behind the row pass).  Nothing
expected here comes from this library: a second and a third merge are compared with the oracle like the first.

What this file shows is that the ANSWERS do not depend on the words, and — through ptx_debug_mark_operands, a test hook of the library outside its C ABI — that
the host really hands them out: every log that gets through P5a has its word after the first eligible merge, and the batches which must have none have none.
That a reading merge then gathers no operand inside the kernel is shown by the emulation twin, which counts the gathers."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import mark_operand_cases as M
from peritext_amd import abi

pytestmark = pytest.mark.gpu
NO_RANK = abi.FLAG_NO_ELEM_RANK


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch  # (first, as in the other GPU modules)

    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    assert H.have_node(), "these cases need node, the oracle's runtime"


def _engine(flags=0, threads=0):
    from peritext_amd.engine import Engine

    e = Engine(0, flags=flags)
    if threads:
        e.set_launch_shape(threads, 0)
    return e


def _stand(e, db):
    """-> logs whose operand words stand, or -1: the batch has no operand words."""
    f = e.lib.ptx_debug_mark_operands
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    n = C.c_uint32(0)
    return -1 if int(f(e.ctx, db, C.byref(n))) < 0 else int(n.value)


def _merge(e, db):
    dr = e.alloc_result(db)
    try:
        e.merge(db, dr)
        return e.download(db, dr)
    finally:
        e.free_result(dr)


def _same(a, b):
    for k in ("logs", "values", "spans", "cintervals", "elem_rank", "ref_slots"):
        x, y = getattr(a, k, None), getattr(b, k, None)
        assert (x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()), k


def _check_shapes(batch, exp, res):
    for l, x in enumerate(exp):
        H.check_log(batch, res, l, x)


@pytest.mark.parametrize("flags,force,threads,kernel", [(0, 128, 128, ("ptx_merge_kernel_w7", "ptx_merge_kernel")), (NO_RANK, 0, 64, ("ptx_merge_kernel_lean64",)),
                                                        (NO_RANK, 128, 128, ("ptx_merge_kernel_lean128",)), (NO_RANK, 192, 192, ("ptx_merge_kernel_lean192",))],
                         ids=["general", "lean64", "lean128", "lean192"])
def test_three_merges_of_one_batch_answer_like_the_oracle_every_time(flags, force, threads, kernel):
    """The writer, then two readers, per build: the shapes at the edges of P5a's blocks and steps (the one-wave build: those it takes), the logs that fail
    behind the row pass, and the log whose header declares a comment id too few — each failing with the same status and row all three times."""
    batch, exp, _ = M.shapes(M.SHORT if threads == 64 else None)
    fb, fexp, codes = M.failing()
    cb, bad, bad_row, cexp = M.bad_comment()
    with _engine(flags, force) as e:
        db, df, dc = e.upload(batch), e.upload(fb), e.upload(cb)
        try:
            assert e.batch_kernel_name(db) in kernel and e.launch_shape(db)[0] == threads
            assert (_stand(e, db), _stand(e, df), _stand(e, dc)) == (0, 0, 0), "made with the index, empty"
            runs = [_merge(e, db)]
            assert _stand(e, db) == batch.n_logs, "the first merge wrote the operand words of every log (all of them pass)"
            runs += [_merge(e, db) for _ in range(2)]
            fruns = [_merge(e, df) for _ in range(3)]
            assert _stand(e, df) == sum(1 for c in codes if not c), "a log that leaves before P5a has no word"
            cruns = [_merge(e, dc) for _ in range(3)]
            assert _stand(e, dc) == cb.n_logs, "P5a ran to its end in all three: the offending op is named from its word by the readers"
        finally:
            e.free_batch(db)
            e.free_batch(df)
            e.free_batch(dc)
    for r in runs:
        _check_shapes(batch, exp, r)
    _same(runs[0], runs[1])
    _same(runs[0], runs[2])
    for r in fruns:
        assert [int(x) for x in r.logs["status"]] == codes
        for l, c in enumerate(codes):
            if not c:
                H.check_log(fb, r, l, fexp[l])
        assert np.array_equal(r.logs, fruns[0].logs), "the same status and row from the writer and from both readers"
    for r in cruns:
        assert int(r.logs["status"][bad]) == abi.ERR_BAD_OP and int(r.logs["reserved"][bad, 1]) == bad_row
        for l in range(cb.n_logs):
            if l != bad:
                H.check_log(cb, r, l, cexp[l])
        assert np.array_equal(r.logs, cruns[0].logs)


def test_a_readmit_context_neither_writes_nor_reads_the_words():
    """A PTX_FLAG_READMIT context first (nothing stands afterwards), then a plain one (the writer, then a reader), then the READMIT context again: the same
    answers, the oracle's."""
    batch, exp, _ = M.shapes()
    with _engine(NO_RANK | abi.FLAG_READMIT) as f, _engine(NO_RANK) as e:
        db = e.upload(batch)
        try:
            runs = [_merge(f, db)]
            assert _stand(f, db) == 0, "a READMIT context writes nothing"
            runs += [_merge(e, db)]
            assert _stand(e, db) == batch.n_logs
            runs += [_merge(e, db), _merge(f, db)]
        finally:
            e.free_batch(db)
    _check_shapes(batch, exp, runs[0])
    _check_shapes(batch, exp, runs[2])
    for r in runs[1:]:
        _same(runs[0], r)


def test_a_second_context_on_another_stream_right_behind_the_writer():
    """Two contexts, each on its own stream, no host synchronisation between their launches: the second gathers while the writer may still run and reads the
    words once the writer has ended.  The oracle's answers from both, every time."""
    batch, exp, _ = M.shapes()
    with _engine(NO_RANK) as e1, _engine(NO_RANK) as e2:
        db = e1.upload(batch)
        r1, r2 = e1.alloc_result(db), e2.alloc_result(db)
        try:
            outs = []
            for _ in range(3):
                e1.merge(db, r1)
                e2.merge(db, r2)
                outs.append((e1.download(db, r1), e2.download(db, r2)))
            assert _stand(e2, db) == batch.n_logs
        finally:
            e1.free_result(r1)
            e2.free_result(r2)
            e1.free_batch(db)
    for a, b in outs:
        _check_shapes(batch, exp, a)
        _check_shapes(batch, exp, b)
        _same(outs[0][0], a)
        _same(outs[0][0], b)


def test_an_append_starts_with_empty_operand_words_and_a_wrapped_batch_has_none():
    """The grown batch of an append has operand words of its own, none standing: merged twice (writer, reader), the same answers, and the base's words are as
    they were.  A batch wrapped around caller-owned device columns has none at all."""
    import torch

    from peritext_amd import wire

    batch, exp, _ = M.shapes()
    n_chg = (batch.chg_off[1:] - batch.chg_off[:-1]).astype(np.int64)
    head, tail = wire.split_batch(batch, [int(c) - int(c) // 3 for c in n_chg])  # (the last third of every log's changes — mark ops, one per change — arrives later)
    with _engine(NO_RANK) as e:
        dh = e.upload(head)
        dg = dw = None
        try:
            r0 = _merge(e, dh)
            assert _stand(e, dh) == batch.n_logs
            dg = e.append(dh, tail)
            assert _stand(e, dg) == 0, "the grown batch starts empty"
            g1 = _merge(e, dg)
            assert _stand(e, dg) == batch.n_logs and _stand(e, dh) == batch.n_logs
            g2, r1 = _merge(e, dg), _merge(e, dh)
            cols = {}
            for k in ("log_off", "op_id", "ref_a", "ref_b", "payload", "action", "mark_type", "side_a", "side_b"):
                x = getattr(batch, k)
                as_signed = {np.dtype("uint64"): np.int64, np.dtype("uint32"): np.int32, np.dtype("uint8"): np.uint8}[x.dtype]
                cols[k] = torch.from_numpy(np.concatenate([x, np.zeros(8, dtype=x.dtype)]).view(as_signed).copy()).cuda()
            torch.cuda.synchronize()
            dw = e.wrap_device(batch.n_logs, batch.n_ops, {k: v.data_ptr() for k, v in cols.items()})
            w1, w2 = _merge(e, dw), _merge(e, dw)
            assert _stand(e, dw) == -1
        finally:
            for d in (dg, dw, dh):
                if d is not None:
                    e.free_batch(d)
        del cols
    for r in (g1, w1):
        _check_shapes(batch, exp, r)
    assert (r0.logs["status"] == 0).all()
    _same(g1, g2)
    _same(r0, r1)
    _same(w1, w2)
