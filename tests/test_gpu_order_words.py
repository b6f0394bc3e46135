"""A standing log's element order is read, not rebuilt (merge_core.h ptx_order_word) on the GPU: the first merge of a batch runs P3 and, in the
three-wave lean build, leaves the log's order words standing; the later merges of that build fill their LDS arrays from the words and run nothing of P3 — and
every answer is still the oracle's.  The logs are those of tests/test_emu_order_words.py at the sizes of the launch shapes here (tests/order_word_cases.py:
order_check_cases' logs, n at the edges of the 16-byte groups, of the tombstone words and of the reader's load step, the deletions, the tree shapes, the logs
that fail).  Nothing expected here comes from this library: a second and a third merge are compared with the oracle like the first.

What this file shows is that the ANSWERS do not depend on the words, that a log which fails fails with the same status and row in every merge, and, through
ptx_debug_order_words, a test hook of the library outside its C ABI, which logs stand.  That a reading merge then runs no tree inside the kernel is shown by the
emulation twin, which counts the passes."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import order_word_cases as W
from peritext_amd import abi

pytestmark = pytest.mark.gpu
NO_RANK = abi.FLAG_NO_ELEM_RANK
# threads per log -> items of one P3a step of the body that takes the logs here (tests/test_gpu_order_checks.py: the same three shapes, for the same reasons)
STEP = {64: 128, 128: 256, 192: 384}
GENERAL = ("ptx_merge_kernel_w7", "ptx_merge_kernel")
WORDS = "ptx_merge_kernel_lean192"  # the one build that holds the order words (merge_core.h PTX_ORDER_WORDS_FORM)
SHAPES = [(64, 64, GENERAL), (128, 0, ("ptx_merge_kernel_lean128",) + GENERAL), (192, 0, (WORDS,))]


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
    """-> logs whose order words stand, or -1: the batch has no order words."""
    f = e.lib.ptx_debug_order_words
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


def _check(batch, exp, res):
    for l, x in enumerate(exp):
        H.check_log(batch, res, l, x)


@pytest.mark.parametrize("threads,force,kernel", SHAPES, ids=["threads64", "threads128", "threads192"])
def test_three_merges_of_one_batch_answer_like_the_oracle_every_time(threads, force, kernel):
    """The writer, then two readers, per launch shape.  In the build that holds the words exactly the passing logs stand behind the first merge; the other builds
    leave none standing and run P3 every time.  The logs that fail report the same status and row all three times."""
    batch, exp, names = W.shapes(STEP[threads], threads)
    fb, fexp, codes, fails = W.failing(STEP[threads], threads)
    rows = int((batch.log_off[1:] - batch.log_off[:-1]).max())
    assert {64: rows <= 2048, 128: 512 < rows <= 2048, 192: 2048 < rows <= 4608}[threads], rows
    # (the failing logs are short: left to the library they would run two waves per log, so their three-wave shape is one the test sets)
    with _engine(NO_RANK, force) as e, _engine(NO_RANK, threads) as ef:
        db, df = e.upload(batch), ef.upload(fb)
        try:
            name, fname = e.batch_kernel_name(db), ef.batch_kernel_name(df)
            assert name in kernel and e.launch_shape(db)[0] == threads, (name, e.launch_shape(db))
            assert fname in kernel + ("ptx_merge_kernel_lean%d" % threads,) and ef.launch_shape(df)[0] == threads, (fname, ef.launch_shape(df))
            assert (_stand(e, db), _stand(ef, df)) == (0, 0), "made with the index, empty"
            runs = [_merge(e, db)]
            assert _stand(e, db) == (batch.n_logs if name == WORDS else 0), "every log passes: all of them stand behind the first merge of the build that holds the words"
            runs += [_merge(e, db) for _ in range(2)]
            fruns = [_merge(ef, df) for _ in range(3)]
            assert _stand(ef, df) == (sum(1 for c in codes if not c) if fname == WORDS else 0), "a log that leaves in P1 .. P3 never stands"
        finally:
            e.free_batch(db)
            ef.free_batch(df)
    for r in runs:
        _check(batch, exp, r)
    _same(runs[0], runs[1])
    _same(runs[0], runs[2])
    keep = [l for l in range(fb.n_logs) if fails[l] != "p1_duplicate_id"]  # (which of two rows with one id is "the repeat" is a race: its status alone)
    for r in fruns:
        assert [int(x) for x in r.logs["status"]] == codes, fails
        for l, c in enumerate(codes):
            if not c:
                H.check_log(fb, r, l, fexp[l])
        assert np.array_equal(r.logs[keep], fruns[0].logs[keep]), "the same status and row from the writer and from both readers"


@pytest.mark.parametrize("threads,force,kernel", SHAPES, ids=["threads64", "threads128", "threads192"])
def test_logs_at_the_edge_of_a_load_step_answer_like_the_oracle_every_time(threads, force, kernel):
    """One short of, at and one past a full step of the reader's load loop for this many threads, three merges.  (With 192 threads that is 1 535 .. 1 537
    elements, a window that no longer lets nine logs share a CU: the general build takes them — order_word_cases.step_edge — and nothing stands.)"""
    batch, exp, names = W.step_edge(threads)
    with _engine(NO_RANK, force) as e:
        db = e.upload(batch)
        try:
            name = e.batch_kernel_name(db)
            assert name in kernel + GENERAL and e.launch_shape(db)[0] == threads, (name, e.launch_shape(db))
            runs = [_merge(e, db)]
            assert _stand(e, db) == (batch.n_logs if name == WORDS else 0)
            runs += [_merge(e, db) for _ in range(2)]
        finally:
            e.free_batch(db)
    for r in runs:
        _check(batch, exp, r)
    _same(runs[0], runs[1])
    _same(runs[0], runs[2])


def test_a_log_that_fails_behind_the_tree_stands_and_repeats_its_error():
    """A comment id beyond the header's n_comment_ids, in the build that holds the words (a launch shape the test sets: the logs are short): the log passes P3,
    so it stands, and reports PTX_ERR_BAD_OP at the same row in all three merges; its neighbours answer like the oracle."""
    batch, bad, row, exp = W.bad_comment()
    with _engine(NO_RANK, 192) as e:
        db = e.upload(batch)
        try:
            assert e.batch_kernel_name(db) == WORDS
            runs = [_merge(e, db)]
            assert _stand(e, db) == batch.n_logs
            runs += [_merge(e, db) for _ in range(2)]
        finally:
            e.free_batch(db)
    for r in runs:
        assert int(r.logs["status"][bad]) == abi.ERR_BAD_OP
        assert np.array_equal(r.logs, runs[0].logs)
        for l in range(batch.n_logs):
            if l != bad:
                H.check_log(batch, r, l, exp[l])


def test_a_readmit_context_runs_the_tree_every_time_and_answers_the_same():
    """A PTX_FLAG_READMIT context first (nothing stands afterwards), then a plain one (the writer, then a reader of the words), then the READMIT context again:
    the same answers, the oracle's."""
    batch, exp, _ = W.shapes(STEP[192], 192)
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
    _check(batch, exp, runs[0])
    _check(batch, exp, runs[2])
    for r in runs[1:]:
        _same(runs[0], r)


def test_an_appended_batch_starts_with_no_word_standing():
    """The grown batch of an append has blocks of its own, none standing: its first merge runs P3 for every log again (writer), the next two read the words; the
    same answers, the oracle's.  The batch it grew from keeps its own."""
    from peritext_amd import wire

    batch, exp, _ = W.shapes(STEP[192], 192)
    n_chg = (batch.chg_off[1:] - batch.chg_off[:-1]).astype(np.int64)
    head, tail = wire.split_batch(batch, [int(c) - int(c) // 3 for c in n_chg])  # (the last third of every log's changes — deletes and mark ops — arrives later)
    with _engine(NO_RANK) as e:
        dh = e.upload(head)
        dg = None
        try:
            r0 = _merge(e, dh)
            stood = _stand(e, dh)
            assert stood == int((r0.logs["status"] == 0).sum())
            dg = e.append(dh, tail)
            assert _stand(e, dg) == 0, "the grown batch starts empty"
            g1 = _merge(e, dg)
            assert _stand(e, dg) == batch.n_logs and _stand(e, dh) == stood
            g2, g3, r1 = _merge(e, dg), _merge(e, dg), _merge(e, dh)
        finally:
            for d in (dg, dh):
                if d is not None:
                    e.free_batch(d)
    _check(batch, exp, g1)
    _same(g1, g2)
    _same(g1, g3)
    _same(r0, r1)
