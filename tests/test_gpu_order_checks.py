"""A standing log's row-order checks are not run again (merge_core.h PtxMergeArgs::order_checks_once) on the GPU: the first merge of a batch runs the
checks of P3a / P3b and lets the log's word stand, the later ones of the three-wave lean build take them as passed — and every answer is still the oracle's.  The
logs are those of tests/test_emu_order_checks.py at the step sizes of the launch shapes here (tests/order_check_cases.py: n and D at the edges of P3a's steps
and of its rest loop, every kind of parent and target, logs that fail in P3a or P3b).  Nothing expected here comes from this library: a second and a third merge
are compared with the oracle like the first.

What this file shows is that the ANSWERS do not depend on the skip, that a log which fails — whose checks are the ones that matter — fails with the same status and
row in every merge, and, through ptx_debug_mark_operands, a test hook of the library outside its C ABI, which logs stand.  That a reading merge then makes no
check inside the kernel is shown by the emulation twin, which counts them."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import order_check_cases as M
from peritext_amd import abi

pytestmark = pytest.mark.gpu
NO_RANK = abi.FLAG_NO_ELEM_RANK
# threads per log -> items of one P3a step of the body that takes the logs here (threads x PTX_U, merge_core.h).  The 64-thread logs: logs of 3 S + 1 inserts
# and as many deletes need a larger LDS window than the one-wave lean build is launched with, so they run the general build (PTX_U = 2), at a launch shape the
# test sets; the 128-thread logs run the two-wave lean build or the general one (PTX_U = 2 in both), the 192-thread logs the three-wave lean build (PTX_U = 2)
STEP = {64: 128, 128: 256, 192: 384}
GENERAL = ("ptx_merge_kernel_w7", "ptx_merge_kernel")
SHAPES = [(64, 64, GENERAL), (128, 0, ("ptx_merge_kernel_lean128",) + GENERAL), (192, 0, ("ptx_merge_kernel_lean192",))]


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


@pytest.mark.parametrize("threads,force,kernel", SHAPES, ids=["threads64", "threads128", "threads192"])
def test_three_merges_of_one_batch_answer_like_the_oracle_every_time(threads, force, kernel):
    """The writer, then two readers, per launch shape: 64-thread logs (a shape the test sets), and by the library's own choice 128-thread logs (up to 2 048 rows)
    and 192-thread logs (the largest shape has more) — the shapes at the edges of that build's steps and rest loop, and the logs that fail in P3a or P3b, each failing
    with the same status and row all three times."""
    S = STEP[threads]
    batch, exp, shapes = M.shapes(S, threads)
    fb, fexp, codes, fails = M.failing(S, threads)
    rows = int((batch.log_off[1:] - batch.log_off[:-1]).max())
    assert {64: rows <= 2048, 128: 512 < rows <= 2048, 192: 2048 < rows <= 4608}[threads], rows
    with _engine(NO_RANK, force) as e:
        db, df = e.upload(batch), e.upload(fb)
        try:
            assert e.batch_kernel_name(db) in kernel and e.launch_shape(db)[0] == threads, (e.batch_kernel_name(db), e.launch_shape(db))
            assert (_stand(e, db), _stand(e, df)) == (0, 0), "made with the index, empty"
            runs = [_merge(e, db)]
            assert _stand(e, db) == batch.n_logs, "every log passes: all of them stand behind the first merge"
            runs += [_merge(e, db) for _ in range(2)]
            fruns = [_merge(e, df) for _ in range(3)]
            assert _stand(e, df) == sum(1 for c in codes if not c), "a log that leaves in P3a or P3b never stands"
        finally:
            e.free_batch(db)
            e.free_batch(df)
    for r in runs:
        _check_shapes(batch, exp, r)
    _same(runs[0], runs[1])
    _same(runs[0], runs[2])
    for r in fruns:
        assert [int(x) for x in r.logs["status"]] == codes, fails
        for l, c in enumerate(codes):
            if not c:
                H.check_log(fb, r, l, fexp[l])
        assert np.array_equal(r.logs, fruns[0].logs), "the same status and row from the writer and from both readers"


def test_the_general_build_checks_and_the_lean_build_trusts_it():
    """A context that asks for elem_rank merges first (the general build: the batch's writer, which runs every check), then a lean context reads the words it left standing, then the first again:
    the oracle's answers from all three."""
    batch, exp, _ = M.shapes(STEP[192], 192)
    with _engine(0) as g, _engine(NO_RANK) as e:
        db = g.upload(batch)
        try:
            assert g.batch_kernel_name(db) in GENERAL
            a = _merge(g, db)
            g.sync()
            assert _stand(g, db) == batch.n_logs
            b, c, d = _merge(e, db), _merge(e, db), _merge(g, db)
        finally:
            g.free_batch(db)
    for r in (a, b, c, d):
        _check_shapes(batch, exp, r)
    _same(a, d)
    _same(b, c)


def test_a_readmit_context_checks_every_time():
    """A PTX_FLAG_READMIT context first (nothing stands afterwards), then a plain one (the writer, then a reader), then the READMIT context again: the same
    answers, the oracle's."""
    batch, exp, _ = M.shapes(STEP[192], 192)
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


def test_an_appended_batch_is_checked_again_and_a_wrapped_batch_every_time():
    """The grown batch of an append has words of its own, none standing: its first merge checks every log again (writer), the next two trust it; the same
    answers.  A batch wrapped around caller-owned device columns has no words: every merge checks."""
    import torch

    from peritext_amd import wire

    batch, exp, _ = M.shapes(STEP[192], 192)
    n_chg = (batch.chg_off[1:] - batch.chg_off[:-1]).astype(np.int64)
    head, tail = wire.split_batch(batch, [int(c) - int(c) // 3 for c in n_chg])  # (the last third of every log's changes — deletes and mark ops — arrives later)
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
            g2, g3, r1 = _merge(e, dg), _merge(e, dg), _merge(e, dh)
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
    _same(g1, g3)
    _same(r0, r1)
    _same(w1, w2)
