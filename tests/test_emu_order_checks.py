"""A standing log's row-order checks are not run again (merge_core.h PtxMergeArgs::order_checks_once), through the host emulation, no GPU: every batch is
merged with one caller-held index and one set of operand words — the writer, then readers in other lane orders with the host's leave.  Status, counts, digests and
rows are the oracle's in every run and identical between them; a lean reader with the leave makes no row-order check of a log whose word stands; a writer, a
reader without the leave, a reader that resolves references and a reader of a log that does not stand make exactly the checks they made before; and a log that
fails never stands, so it fails with the same code and row in every run.

The driver compiles the skip into every body (PTX_ORDER_CHECKS_ONCE_FORM 1).  The product keeps it to the three-wave lean build, which never has out_refs: the
"resolves references" half of the condition, shown here on the general body, guards what the emulation alone can reach."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import order_check_cases as M
from peritext_amd import abi, wire

LIB = os.path.join(H.ROOT, "tests", "emu", "libperitext_emu_orderchecks.so")
EMU_T = 1  # the emulation's one thread ...


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    assert H.have_node(), "these cases need node, the oracle's runtime: a skipped case would hide exactly what this file exists to show"


def _lib():
    lib = C.CDLL(LIB)
    for name in ("ptx_emu_orderchecks_words", "ptx_emu_orderchecks_bits_words"):
        getattr(lib, name).restype = C.c_ulonglong
        getattr(lib, name).argtypes = [C.c_ulonglong, C.c_ulonglong]
    lib.ptx_emu_orderchecks_step_items.restype = C.c_uint32
    return lib


def EMU_S():
    return int(_lib().ptx_emu_orderchecks_step_items())  # ... and its PTX_U items per step


class Words:
    """The caller-held index and operand words of one batch: what the host library keeps beside a resident batch."""

    def __init__(self, b):
        lib = _lib()
        words = int(lib.ptx_emu_orderchecks_words(b.n_ops, b.n_logs))
        self.index = np.full(words, 0xEEEEEEEE, dtype=np.uint32)  # (never zeroed by the library either)
        self.bits = np.full(int(lib.ptx_emu_orderchecks_bits_words(b.n_ops, b.n_logs)), 0xEEEEEEEE, dtype=np.uint32)
        self.rows_indexed = np.zeros(max(b.n_logs, 1), dtype=np.uint32)
        self.ops = np.full(words, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
        self.stand = np.zeros(max(b.n_logs, 1), dtype=np.uint32)


def merge(b, w, write, once, reverse=0, lean=False):
    """-> (Results, row-order checks per log) of ptx_emu_merge_orderchecks over a wire.Batch; w: Words or None."""
    n = max(b.n_ops, 1)
    res = wire.Results(
        logs=np.zeros(b.n_logs, dtype=abi.LOG_RESULT_DTYPE),
        values=np.full(n, 0xDEADBEEF, dtype=np.uint32),
        spans=np.zeros(n, dtype=abi.SPAN_DTYPE),
        cintervals=np.zeros(n, dtype=abi.CINTERVAL_DTYPE),
        elem_rank=None if lean else np.zeros(n, dtype=np.uint32),
        ref_slots=None if lean else np.full(n, 0xFFFFFFFF, dtype=np.uint32),
    )
    checks = np.zeros(max(b.n_logs, 1), dtype=np.uint64)
    s = H.batch_struct(b)
    f = C.CDLL(LIB).ptx_emu_merge_orderchecks
    f.restype = C.c_int
    f.argtypes = [C.POINTER(abi.ptx_batch)] + [C.c_void_p] * 11 + [C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_int]
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    rc = f(C.byref(s), res.logs.ctypes.data, res.values.ctypes.data, res.spans.ctypes.data, res.cintervals.ctypes.data,
           None if lean else res.elem_rank.ctypes.data, None if lean else res.ref_slots.ctypes.data,
           None if w is None else ptr(w.index), None if w is None else ptr(w.bits), None if w is None else ptr(w.rows_indexed),
           None if w is None else ptr(w.ops), None if w is None else ptr(w.stand),
           1 if write else 0, 1 if once else 0, checks.ctypes.data, H.LDS_BYTES, reverse, 1 if lean else 0)
    assert rc == 0
    return res, checks[: b.n_logs]


def same_results(a, b, batch):
    """The result rows (LDS high-water mark included), and of every log that passes its values / span rows / comment intervals (rows beyond a log's counts are
    scratch) — and, where the run has them, the resolved references of its delete and mark rows."""
    if not np.array_equal(a.logs, b.logs):
        return False
    for l in range(batch.n_logs):
        if int(a.logs["status"][l]):
            continue
        r0, r1 = int(batch.log_off[l]), int(batch.log_off[l + 1])
        for k, cnt in (("values", "n_visible"), ("spans", "n_spans"), ("cintervals", "n_cintervals")):
            c = int(a.logs[cnt][l]) if cnt in a.logs.dtype.names else 0
            if not np.array_equal(getattr(a, k)[r0: r0 + c], getattr(b, k)[r0: r0 + c]):
                return False
        if a.ref_slots is not None and not (np.array_equal(a.ref_slots[r0:r1], b.ref_slots[r0:r1]) and np.array_equal(a.elem_rank[r0:r1], b.elem_rank[r0:r1])):
            return False
    return True


def _checks(n, D):
    """Row-order checks of one passing log, as the hook counts them: one per delete (the pass behind P3a over the fused ones, the rest loop over the others) and
    one per insert (P3b)."""
    return n + D


@pytest.mark.parametrize("orders,lean", [((0, 1, 2), True), ((2, 0, 1), False), ((1, 2, 0), True), ((0, 2, 1), False)])
def test_writer_and_readers_answer_like_the_oracle_and_a_lean_reader_checks_nothing(orders, lean):
    S = EMU_S()
    batch, exp, shapes = M.shapes(S, EMU_T)
    assert {n for n, D in shapes} == set(M.step_values(S)) <= {D for n, D in shapes}
    N = (batch.log_off[1:] - batch.log_off[:-1]).astype(np.uint32)
    want = np.array([_checks(n, D) for n, D in shapes], dtype=np.uint64)
    plain, c_plain = merge(batch, None, False, True, orders[0], lean)
    assert np.array_equal(c_plain, want), ("a launch without an index checks what it always checked, leave or no leave", c_plain.tolist(), want.tolist())
    no_leave = Words(batch)
    for k in range(3):  # (the writer and two readers of the operand words WITHOUT the host's leave: every check, as before)
        res, c = merge(batch, no_leave, k == 0, False, orders[1], lean)
        assert np.array_equal(c, want) and same_results(res, plain, batch)
    w = Words(batch)
    runs = []
    for k, order in enumerate(orders):
        res, c = merge(batch, w, k == 0, True, order, lean)  # (the leave is given to the writer too: a writing launch never reads a word, so it checks)
        for l in range(batch.n_logs):
            H.check_log(batch, res, l, exp[l])
        assert np.array_equal(w.rows_indexed, N) and np.array_equal(w.stand, N)
        if k == 0 or not lean:  # the general body resolves references here (out_refs): nothing is skipped
            assert np.array_equal(c, want), (k, c.tolist())
        else:
            assert not c.any(), (k, c.tolist())
        runs.append(res)
    for r in runs[1:]:
        assert same_results(runs[0], r, batch), "writer and readers agree byte for byte, whatever the lane order"
    assert same_results(runs[0], plain, batch), "... and a merge without an index answers the same, LDS high-water mark included"


def test_a_log_that_does_not_stand_is_checked_again():
    """A reader with the leave that finds a log's word at 0 — or at anything but its row count — runs every check, and answers the same."""
    S = EMU_S()
    batch, exp, shapes = M.shapes(S, EMU_T)
    w = Words(batch)
    first, _ = merge(batch, w, True, True, 0, True)
    N = (batch.log_off[1:] - batch.log_off[:-1]).astype(np.uint32)
    want = np.array([_checks(n, D) for n, D in shapes], dtype=np.uint64)
    w.stand[0::2] = 0
    w.stand[1::2] = N[1::2] + 1
    res, c = merge(batch, w, False, True, 2, True)
    assert np.array_equal(c, want) and same_results(first, res, batch)


@pytest.mark.parametrize("lean", [False, True])
def test_a_failing_log_never_stands_and_fails_alike_in_every_run(lean):
    """Parents and targets that are out of the header's bounds, never inserted or inserted later, in the fused loop and on the rest path: each log passes P1
    (rows_indexed = N) and leaves in P3a or P3b — its word never stands, so every run checks it again.  Status from the oracle; status and row equal in all
    three runs and equal to those of a merge without an index."""
    S = EMU_S()
    batch, exp, codes, fails = M.failing(S, EMU_T)
    assert sum(c != 0 for c in codes) == len(M.FAILS)
    N = (batch.log_off[1:] - batch.log_off[:-1]).astype(np.uint32)
    plain, c_plain = merge(batch, None, False, True, 1, lean)
    w = Words(batch)
    runs = []
    for k, order in enumerate((0, 1, 2)):
        res, c = merge(batch, w, k == 0, True, order, lean)
        for l in range(batch.n_logs):
            assert int(res.logs["status"][l]) == codes[l], (k, l, fails[l])
            assert int(w.rows_indexed[l]) == int(N[l]) and int(w.stand[l]) == (0 if codes[l] else int(N[l])), (k, l)
            if not codes[l]:
                H.check_log(batch, res, l, exp[l])
                assert int(c[l]) == (int(c_plain[l]) if k == 0 or not lean else 0)
            elif fails[l] in ("parent_inserted_later", "delete_inserted_later", "rest_delete_inserted_later"):
                assert int(c[l]) > 0, "the order checks are what finds these: a run that skipped them would pass the log"
        runs.append(res)
    assert np.array_equal(runs[0].logs, runs[1].logs) and np.array_equal(runs[0].logs, runs[2].logs) and np.array_equal(runs[0].logs, plain.logs)


def test_sanitizer_program_writer_and_readers(tmp_path):
    """tests/emu/emu_orderchecks_main.cc: the same entry over the shapes' batch, every block exactly as large as the host library makes it, compiled with
    -fsanitize=address,undefined and run as a child process (nothing sanitized is loaded into this interpreter).  Write, read, read."""
    batch, _, _ = M.shapes(EMU_S(), EMU_T)
    path = str(tmp_path / "batch.bin")
    with open(path, "wb") as f:
        n_changes = int(batch.chg_off[-1])
        f.write(np.array([batch.n_logs, batch.n_ops, n_changes, batch.max_actors, abi.env_stride(batch.max_actors)], dtype=np.uint64).tobytes())
        for name, dt in (("log_off", np.uint64), ("op_id", np.uint64), ("ref_a", np.uint64), ("ref_b", np.uint64), ("payload", np.uint32), ("action", np.uint8),
                         ("mark_type", np.uint8), ("side_a", np.uint8), ("side_b", np.uint8), ("chg_off", np.uint64), ("chg_hdr", np.uint32), ("chg_env", np.uint16)):
            col = np.ascontiguousarray(getattr(batch, name), dtype=dt)
            f.write(col[: {"log_off": batch.n_logs + 1, "chg_off": batch.n_logs + 1, "chg_hdr": n_changes, "chg_env": n_changes * abi.env_stride(batch.max_actors)}.get(name, batch.n_ops)].tobytes())
    exe = str(tmp_path / "emu_orderchecks_main")
    src = os.path.join(H.ROOT, "tests", "emu", "emu_orderchecks_main.cc")
    # (-g1: line tables are all a report needs; full debug info doubles the compile)
    b = subprocess.run(["g++", "-O1", "-g1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    for lean in ("0", "1"):
        p = subprocess.run([exe, path, lean], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
        assert "0 disagreements" in p.stdout and "0 checks by the readers" in p.stdout and " %d words stand" % batch.n_logs in p.stdout, p.stdout
