"""The operand words of a resident batch's mark ops (merge_core.h ptx_mark_operand_pack) through the host emulation, no GPU: every batch is merged with one
caller-held index and one caller-held set of operand words — the writer, then readers in other lane orders.  Status, counts, digests and rows are the oracle's in
every run and identical between them; a log's word stands exactly when its writer got through P5a; a reader gathers no operand of a log whose word stands, a
writer and a launch without an index gather what they gathered before; and the words hold, field by field, what the columns say."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import mark_operand_cases as M
from peritext_amd import abi, wire

LIB = os.path.join(H.ROOT, "tests", "emu", "libperitext_emu_markops.so")
ROWIX_LIB = os.path.join(H.ROOT, "tests", "emu", "libperitext_emu_rowindex.so")
EMU_JB_CAP = 8  # (ptx_platform_emu.h PTX_JB_CAP: a block of the emulation holds eight mark ops, so every K here ends a block somewhere else than on the GPU)


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    assert H.have_node(), "these cases need node, the oracle's runtime: a skipped case would hide exactly what this file exists to show"


class Words:
    """The caller-held index and operand words of one batch: what the host library keeps beside a resident batch."""

    def __init__(self, b, ops=True):
        lib = C.CDLL(LIB)
        for name in ("ptx_emu_markops_words", "ptx_emu_markops_bits_words", "ptx_emu_markops_off", "ptx_emu_markops_gathers"):
            getattr(lib, name).restype = C.c_ulonglong
            getattr(lib, name).argtypes = [] if name.endswith("gathers") else [C.c_ulonglong, C.c_ulonglong]
        self.lib = lib
        words = int(lib.ptx_emu_markops_words(b.n_ops, b.n_logs))
        self.index = np.full(words, 0xEEEEEEEE, dtype=np.uint32)  # (never zeroed by the library either)
        self.bits = np.full(int(lib.ptx_emu_markops_bits_words(b.n_ops, b.n_logs)), 0xEEEEEEEE, dtype=np.uint32)
        self.rows_indexed = np.zeros(max(b.n_logs, 1), dtype=np.uint32)
        self.ops = np.full(words, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64) if ops else None
        self.stand = np.zeros(max(b.n_logs, 1), dtype=np.uint32) if ops else None

    def off(self, b, log):
        return int(self.lib.ptx_emu_markops_off(int(b.log_off[log]), log))


def merge(b, w, write, reverse=0, lean=False):
    """-> (Results, operand gathers per log) of ptx_emu_merge_markops over a wire.Batch; w: Words or None."""
    n = max(b.n_ops, 1)
    res = wire.Results(
        logs=np.zeros(b.n_logs, dtype=abi.LOG_RESULT_DTYPE),
        values=np.full(n, 0xDEADBEEF, dtype=np.uint32),
        spans=np.zeros(n, dtype=abi.SPAN_DTYPE),
        cintervals=np.zeros(n, dtype=abi.CINTERVAL_DTYPE),
        elem_rank=None if lean else np.zeros(n, dtype=np.uint32),
        ref_slots=None if lean else np.full(n, 0xFFFFFFFF, dtype=np.uint32),
    )
    gathers = np.zeros(max(b.n_logs, 1), dtype=np.uint64)
    s = H.batch_struct(b)
    f = C.CDLL(LIB).ptx_emu_merge_markops
    f.restype = C.c_int
    f.argtypes = [C.POINTER(abi.ptx_batch)] + [C.c_void_p] * 11 + [C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_int]
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    rc = f(C.byref(s), res.logs.ctypes.data, res.values.ctypes.data, res.spans.ctypes.data, res.cintervals.ctypes.data,
           None if lean else res.elem_rank.ctypes.data, None if lean else res.ref_slots.ctypes.data,
           None if w is None else ptr(w.index), None if w is None else ptr(w.bits), None if w is None else ptr(w.rows_indexed),
           None if w is None else ptr(w.ops), None if w is None else ptr(w.stand),
           1 if write else 0, gathers.ctypes.data, H.LDS_BYTES, reverse, 1 if lean else 0)
    assert rc == 0
    return res, gathers[: b.n_logs]


def same_results(a, b, batch):
    """The result rows, and of every log that passes its values / span rows / comment intervals (rows beyond a log's counts are scratch) — and, where the run
    has them, the resolved references of its delete and mark rows."""
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


def _steps(K):
    """Operand gathers of one log's P5a in its first form, as the emulation walks it: one per lane slot of every block (ceil(K / (EMU_JB_CAP - 4)) blocks, so that
    the four slices of a block fit it) and one more, the look-ahead behind the last step."""
    return (((K + EMU_JB_CAP - 5) // (EMU_JB_CAP - 4)) if K else 0) * EMU_JB_CAP + 1


def _census(batch, l):
    act = batch.action[int(batch.log_off[l]): int(batch.log_off[l + 1])]
    return int((act == abi.ACT_INSERT).sum()), int((act == abi.ACT_DELETE).sum()), int(np.isin(act, (abi.ACT_ADDMARK, abi.ACT_REMOVEMARK)).sum())


def _expected_words(batch, l, park_rows):
    """The operand word of every mark op of log l, in park order, from the columns and the census header alone."""
    lo, hi = int(batch.log_off[l]), int(batch.log_off[l + 1])
    ids = batch.op_id[lo:hi]
    max_ctr, max_actor = int((ids >> np.uint64(32)).max()), int((ids & np.uint64(0xFFFFFFFF)).max())
    is_c = (batch.mark_type[lo:hi] == abi.MARK_COMMENT) & np.isin(batch.action[lo:hi], (abi.ACT_ADDMARK, abi.ACT_REMOVEMARK))
    kid = int(batch.payload[lo:hi][is_c].max()) + 1 if is_c.any() else 0

    def key(ref):
        ctr, actor = int(ref) >> 32, int(ref) & 0xFFFFFFFF
        return ctr * (max_actor + 1) + actor if 1 <= ctr <= max_ctr and actor <= max_actor else 0

    out = []
    for r in park_rows:
        g = lo + int(r)
        cm = int(batch.payload[g]) if is_c[r] else 0
        out.append({"key_a": key(batch.ref_a[g]), "key_b": key(batch.ref_b[g]), "side_a": min(int(batch.side_a[g]), 2), "side_b": min(int(batch.side_b[g]), 2),
                    "comment": cm if cm < kid else 0, "bad": int(bool(is_c[r]) and cm >= kid)})
    return out


def _fields(w):
    w = int(w)
    return {"key_a": w & 0xFFFF, "key_b": (w >> 16) & 0xFFFF, "comment": (w >> 32) & 0xFFFF, "side_a": (w >> 48) & 3, "side_b": (w >> 50) & 3, "bad": (w >> 52) & 1}


def test_the_one_wave_cases_fit_the_one_wave_build():
    """The LDS windows of mark_operand_cases.SHORT, by the host's own rule: more than 24 of them share a CU, and no log has more than 512 rows."""
    batch, _, _ = M.shapes()
    f = C.CDLL(ROWIX_LIB).ptx_emu_rowindex_lds_need
    f.restype = None
    f.argtypes = [C.POINTER(abi.ptx_batch), C.c_void_p]
    need = np.zeros(batch.n_logs, dtype=np.uint64)
    s = H.batch_struct(batch)
    f(C.byref(s), need.ctypes.data)
    N = batch.log_off[1:] - batch.log_off[:-1]
    assert len(M.SHORT) >= 12 and all(int(need[i]) <= 160 * 1024 // 25 and int(N[i]) <= 512 for i in M.SHORT), need.tolist()


@pytest.mark.parametrize("orders,lean", [((0, 0, 1, 2), True), ((2, 0, 1, 2), False), ((1, 2, 0, 1), True), ((0, 1, 2, 0), False)])
def test_writer_and_readers_answer_like_the_oracle_and_a_reader_gathers_nothing(orders, lean):
    batch, exp, shapes = M.shapes()
    assert {K for n, D, K, e in shapes} >= {0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 385}
    N = (batch.log_off[1:] - batch.log_off[:-1]).astype(np.uint32)
    want_g = np.array([_steps(K) for n, D, K, e in shapes], dtype=np.uint64)
    plain, g_plain = merge(batch, None, False, orders[0], lean)
    assert np.array_equal(g_plain, want_g), "a launch without an index gathers what it always gathered"
    index_only = Words(batch, ops=False)
    for k in range(2):  # (an index without operand words, the batch of a failed allocation: the writer and a reader on the gathers)
        res, g = merge(batch, index_only, k == 0, orders[1], lean)
        assert np.array_equal(g, want_g) and same_results(res, plain, batch)
    w = Words(batch)
    runs = []
    for k, order in enumerate(orders):
        res, g = merge(batch, w, k == 0, order, lean)
        for l in range(batch.n_logs):
            H.check_log(batch, res, l, exp[l])
        assert np.array_equal(w.rows_indexed, N) and np.array_equal(w.stand, N), "every log that gets through P5a has its word, with its row count"
        assert np.array_equal(g, want_g) if k == 0 else not g.any(), (k, g.tolist())
        runs.append(res)
    for r in runs[1:]:
        assert same_results(runs[0], r, batch), "writer and readers agree byte for byte, whatever the lane order"
    assert same_results(runs[0], plain, batch), "... and a merge without an index answers the same, LDS high-water mark included"
    # the words the writer left, field by field, against the columns; nothing outside the K words of a log was touched
    touched = np.zeros(len(w.ops), dtype=bool)
    for l in range(batch.n_logs):
        n, D, K = _census(batch, l)
        o, n4 = w.off(batch, l), (n + 3) & ~3
        park_rows = w.index[o + n4 + D: o + n4 + D + K] & 0xFFFF
        assert [_fields(x) for x in w.ops[o: o + K]] == _expected_words(batch, l, park_rows), (l, K)
        touched[o: o + K] = True
    assert (w.ops[~touched] == np.uint64(0xEEEEEEEEEEEEEEEE)).all()
    ops_case = [l for l, s in enumerate(shapes) if s[3] == "operands"][0]
    o, K = w.off(batch, ops_case), shapes[ops_case][2]
    f = [_fields(x) for x in w.ops[o: o + K]]
    assert any(x["key_a"] == 0 for x in f) and any(x["key_b"] == 0 for x in f) and {x["side_a"] for x in f} == {0, 1, 2} and {x["side_b"] for x in f} == {0, 1, 2}
    assert len({x["comment"] for x in f}) >= 3 and not any(x["bad"] for x in f)


def test_a_word_that_does_not_stand_is_never_consumed():
    """A reader that finds a log's word at 0 — or at anything but its row count — gathers, and answers the same: the words of such a log are never read (they
    are poisoned here with keys, rows' worth of sides and comment ids that would change every interval)."""
    batch, exp, shapes = M.shapes()
    w = Words(batch)
    first, _ = merge(batch, w, True, 0, True)
    N = (batch.log_off[1:] - batch.log_off[:-1]).astype(np.uint32)
    want_g = np.array([_steps(K) for n, D, K, e in shapes], dtype=np.uint64)
    w.ops[:] = np.uint64(0x001FFFFF00010001)
    w.stand[0::2] = 0
    w.stand[1::2] = N[1::2] + 1
    res, g = merge(batch, w, False, 2, True)
    assert np.array_equal(g, want_g) and same_results(first, res, batch)
    assert (w.ops == np.uint64(0x001FFFFF00010001)).all(), "a reader writes nothing"


@pytest.mark.parametrize("lean", [False, True])
def test_logs_that_fail_behind_the_row_pass_fail_alike_in_writer_and_readers(lean):
    """A delete of an element nobody inserted: the log passes P1 (rows_indexed = N) and leaves in P3a, before P5a — its word never stands, in the writer or
    later, and the readers gather nothing for it because they leave at the same place.  Status from the oracle; status and row equal in all three runs."""
    batch, exp, codes = M.failing()
    N = (batch.log_off[1:] - batch.log_off[:-1]).astype(np.uint32)
    w = Words(batch)
    runs = []
    for k, order in enumerate((0, 1, 2)):
        res, g = merge(batch, w, k == 0, order, lean)
        for l in range(batch.n_logs):
            assert int(res.logs["status"][l]) == codes[l], (k, l)
            assert int(w.rows_indexed[l]) == int(N[l]) and int(w.stand[l]) == (0 if codes[l] else int(N[l])), (k, l)
            if codes[l]:
                assert int(g[l]) == 0
            else:
                H.check_log(batch, res, l, exp[l])
                assert int(g[l]) == (_steps(_census(batch, l)[2]) if k == 0 else 0)
        runs.append(res)
    assert np.array_equal(runs[0].logs, runs[1].logs) and np.array_equal(runs[0].logs, runs[2].logs)


@pytest.mark.parametrize("lean", [False, True])
def test_a_comment_id_beyond_the_header_is_the_same_bad_op_from_the_words(lean):
    """The caller's header declares one comment id less than one op of the log uses: PTX_ERR_BAD_OP at that op's row (the header's contract, peritext_hip.h) from
    the writer, which reads the payload, and from two readers, which read the word's bit; the word stands (P5a ran to its end); the other logs are the oracle's."""
    batch, bad, row, exp = M.bad_comment()
    w = Words(batch)
    runs = []
    for k, order in enumerate((0, 2, 1)):
        res, g = merge(batch, w, k == 0, order, lean)
        assert int(res.logs["status"][bad]) == abi.ERR_BAD_OP and int(res.logs["reserved"][bad, 1]) == row, (k, res.logs[bad])
        for l in range(batch.n_logs):
            if l != bad:
                H.check_log(batch, res, l, exp[l])
        assert w.stand.tolist() == (batch.log_off[1:] - batch.log_off[:-1]).tolist() and (k == 0 or not g.any())
        runs.append(res)
    assert np.array_equal(runs[0].logs, runs[1].logs) and np.array_equal(runs[0].logs, runs[2].logs)
    o = w.off(batch, bad)
    K = _census(batch, bad)[2]
    assert sum(_fields(x)["bad"] for x in w.ops[o: o + K]) == 1


def test_sanitizer_program_writer_and_readers(tmp_path):
    """tests/emu/emu_markops_main.cc: the same entry over the shapes' batch, every block exactly as large as the host library makes it, compiled with
    -fsanitize=address,undefined and run as a child process (nothing sanitized is loaded into this interpreter)."""
    batch, _, _ = M.shapes()
    path = str(tmp_path / "batch.bin")
    with open(path, "wb") as f:
        n_changes = int(batch.chg_off[-1])
        f.write(np.array([batch.n_logs, batch.n_ops, n_changes, batch.max_actors, abi.env_stride(batch.max_actors)], dtype=np.uint64).tobytes())
        for name, dt in (("log_off", np.uint64), ("op_id", np.uint64), ("ref_a", np.uint64), ("ref_b", np.uint64), ("payload", np.uint32), ("action", np.uint8),
                         ("mark_type", np.uint8), ("side_a", np.uint8), ("side_b", np.uint8), ("chg_off", np.uint64), ("chg_hdr", np.uint32), ("chg_env", np.uint16)):
            col = np.ascontiguousarray(getattr(batch, name), dtype=dt)
            f.write(col[: {"log_off": batch.n_logs + 1, "chg_off": batch.n_logs + 1, "chg_hdr": n_changes, "chg_env": n_changes * abi.env_stride(batch.max_actors)}.get(name, batch.n_ops)].tobytes())
    exe = str(tmp_path / "emu_markops_main")
    src = os.path.join(H.ROOT, "tests", "emu", "emu_markops_main.cc")
    # (-g1: line tables are all a report needs; full debug info doubles the compile)
    b = subprocess.run(["g++", "-O1", "-g1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    for lean in ("0", "1"):
        p = subprocess.run([exe, path, lean], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
        assert "0 disagreements" in p.stdout and "0 gathers by the readers" in p.stdout and " %d words stand" % batch.n_logs in p.stdout, p.stdout
