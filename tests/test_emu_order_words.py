"""A standing log's element order is read, not rebuilt (merge_core.h ptx_order_word), through the host emulation, no GPU: every batch is merged with one
caller-held set of blocks — the writer, then readers in three lane orders.  Status, counts, digests and rows are the oracle's in every run and identical between
them, the LDS high-water mark included; a reader of a standing log never enters P3, gathers no mark operand and makes no row-order check; a writer, a reader
without the blocks, a reader that resolves references and a reader of a log that does not stand count what they always counted; the words themselves are the
general body's elem_rank, field by field; and a log that fails in P1 .. P3 never stands, so it fails with the same code and row in every run.

The driver (tests/emu/emu_orderwords.cc) compiles the words into every body (PTX_ORDER_WORDS_FORM 1).  The product keeps them to the three-wave lean build, which
never has out_refs: the "resolves references" half of the condition, shown here on the general body, guards what the emulation alone can reach."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import order_word_cases as W
from peritext_amd import abi, wire

LIB = os.path.join(H.ROOT, "tests", "emu", "libperitext_emu_orderwords.so")
EMU_T = 1  # the emulation's one thread
EMU_S = 2  # ... and its PTX_U items per P3a step (kThreads = 0)


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    assert H.have_node(), "these cases need node, the oracle's runtime: a skipped case would hide exactly what this file exists to show"


def _lib():
    lib = C.CDLL(LIB)
    for name in ("ptx_emu_orderwords_words", "ptx_emu_orderwords_bits_words", "ptx_emu_orderwords_off", "ptx_emu_orderwords_bits_off"):
        getattr(lib, name).restype = C.c_ulonglong
        getattr(lib, name).argtypes = [C.c_ulonglong, C.c_ulonglong]
    lib.ptx_emu_orderwords_load_step.restype = C.c_uint32
    return lib


def test_the_cases_stand_at_the_edges_of_the_emulations_load_step():
    assert int(_lib().ptx_emu_orderwords_load_step()) == W.load_step(EMU_T)
    assert W.step_edge_sizes(EMU_T) == (7, 8, 9)


class Words:
    """The caller-held blocks of one batch: what the host library keeps beside a resident batch.  Every block at the library's exact size, pre-filled with
    0xEE (the library never zeroes them); only the words per log are zeroed.  order=False: a batch whose order words could not be allocated."""

    def __init__(self, b, order=True):
        lib = _lib()
        words = int(lib.ptx_emu_orderwords_words(b.n_ops, b.n_logs))
        bits = int(lib.ptx_emu_orderwords_bits_words(b.n_ops, b.n_logs))
        self.index = np.full(words, 0xEEEEEEEE, dtype=np.uint32)
        self.bits = np.full(bits, 0xEEEEEEEE, dtype=np.uint32)
        self.rows_indexed = np.zeros(max(b.n_logs, 1), dtype=np.uint32)
        self.ops = np.full(words, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
        self.stand = np.zeros(max(b.n_logs, 1), dtype=np.uint32)
        self.ow = np.full(words, 0xEEEEEEEE, dtype=np.uint32) if order else None
        self.ob = np.full(bits, 0xEEEEEEEE, dtype=np.uint32) if order else None
        self.ostand = np.zeros(max(b.n_logs, 1), dtype=np.uint32) if order else None


def merge(b, w, write, reverse=0, lean=False, once=True):
    """-> (Results, [tree passes, mark gathers, row-order checks] per log) of ptx_emu_merge_orderwords over a wire.Batch; w: Words or None."""
    n = max(b.n_ops, 1)
    res = wire.Results(
        logs=np.zeros(b.n_logs, dtype=abi.LOG_RESULT_DTYPE),
        values=np.full(n, 0xDEADBEEF, dtype=np.uint32),
        spans=np.zeros(n, dtype=abi.SPAN_DTYPE),
        cintervals=np.zeros(n, dtype=abi.CINTERVAL_DTYPE),
        elem_rank=None if lean else np.zeros(n, dtype=np.uint32),
        ref_slots=None if lean else np.full(n, 0xFFFFFFFF, dtype=np.uint32),
    )
    counts = np.zeros((max(b.n_logs, 1), 3), dtype=np.uint64)
    s = H.batch_struct(b)
    f = C.CDLL(LIB).ptx_emu_merge_orderwords
    f.restype = C.c_int
    f.argtypes = [C.POINTER(abi.ptx_batch)] + [C.c_void_p] * 14 + [C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_int]
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    blocks = [None] * 8 if w is None else [ptr(x) for x in (w.index, w.bits, w.rows_indexed, w.ops, w.stand, w.ow, w.ob, w.ostand)]
    rc = f(C.byref(s), res.logs.ctypes.data, res.values.ctypes.data, res.spans.ctypes.data, res.cintervals.ctypes.data,
           None if lean else res.elem_rank.ctypes.data, None if lean else res.ref_slots.ctypes.data, *blocks,
           1 if write else 0, 1 if once else 0, counts.ctypes.data, H.LDS_BYTES, reverse, 1 if lean else 0)
    assert rc == 0
    return res, counts[: b.n_logs]


def same_results(a, b, batch):
    """The result rows (LDS high-water mark included), and of every log that passes its values / span rows / comment intervals (rows beyond a log's counts are
    scratch) — and, where the run has them, elem_rank and the resolved references of its rows."""
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


def _census(batch):
    """-> per log (n, D, K) from the rows."""
    out = []
    for l in range(batch.n_logs):
        a = batch.action[int(batch.log_off[l]): int(batch.log_off[l + 1])]
        out.append((int((a == abi.ACT_INSERT).sum()), int((a == abi.ACT_DELETE).sum()), int(((a == abi.ACT_ADDMARK) | (a == abi.ACT_REMOVEMARK)).sum())))
    return out


def _full(c_plain, gathers=True, checks=True):
    """What the logs count on the full path, from a merge without any block (c_plain): one tree pass each, the gathers of P5a's first form (none where the operand
    words are read) and one row-order check per insert and per delete (none where a lean reader has the host's leave)."""
    c = c_plain.copy()
    if not gathers:
        c[:, 1] = 0
    if not checks:
        c[:, 2] = 0
    return c


def _plain(batch, order, lean):
    res, c = merge(batch, None, False, order, lean)
    ok = res.logs["status"] == 0
    assert (c[ok, 0] == 1).all() and np.array_equal(c[ok, 2], np.array([n + D for n, D, K in _census(batch)], dtype=np.uint64)[ok])
    assert (c[:, 1] >= np.array([K for n, D, K in _census(batch)], dtype=np.uint64))[ok].all()  # (a lane slot without an op gathers too)
    return res, c


def _rows(batch):
    return (batch.log_off[1:] - batch.log_off[:-1]).astype(np.uint32)


@pytest.mark.parametrize("cases", ["shapes", "step_edge"])
@pytest.mark.parametrize("orders,lean", [((0, 0, 1, 2), True), ((2, 1, 0, 2), False), ((1, 2, 0, 1), True)])
def test_writer_and_readers_answer_like_the_oracle_and_a_standing_reader_runs_no_tree(orders, lean, cases):
    batch, exp, names = W.shapes(EMU_S, EMU_T) if cases == "shapes" else W.step_edge(EMU_T)
    N = _rows(batch)
    plain, c_plain = _plain(batch, orders[0], lean)
    # a batch without order words (their allocation failed): the writer and the readers on the full path, as before the words
    nw = Words(batch, order=False)
    for k in range(3):
        res, c = merge(batch, nw, k == 0, orders[1], lean)
        assert np.array_equal(c, _full(c_plain, gathers=k == 0, checks=k == 0 or not lean)), (k, "a reader without the blocks counts what it counted before")
        assert same_results(res, plain, batch)
    w = Words(batch)
    runs = []
    for k, order in enumerate(orders):
        res, c = merge(batch, w, k == 0, order, lean)
        for l in range(batch.n_logs):
            H.check_log(batch, res, l, exp[l])
        assert np.array_equal(w.rows_indexed, N) and np.array_equal(w.stand, N) and np.array_equal(w.ostand, N), "every log passes: all of them stand"
        if k == 0:
            assert np.array_equal(c, c_plain), "the writer counts what it counted before"
        elif lean:
            assert not c.any(), (k, [(names[l], c[l].tolist()) for l in np.flatnonzero(c.any(axis=1))])
        else:  # the general body resolves references here (out_refs): P3 runs, every check with it
            assert np.array_equal(c, _full(c_plain, gathers=False)), (k, "a reader that resolves references counts what it counted before")
        runs.append(res)
    for r in runs[1:]:
        assert same_results(runs[0], r, batch), "writer and readers agree byte for byte, whatever the lane order"
    assert same_results(runs[0], plain, batch), "... and a merge without an index answers the same, LDS high-water mark included"


def test_the_words_are_the_general_bodys_elem_rank_field_by_field():
    """Word e of a log = row_of[e] | rnk[e] << 16, bit e of its tombstone words = deleted: against elem_rank (position | tombstone, by the row that inserted the
    element) of a general-body merge of the same log.  Elements come in the order of their id keys: counter, then actor."""
    batch, exp, names = W.shapes(EMU_S, EMU_T)
    lib = _lib()
    w = Words(batch)
    merge(batch, w, True, 1, True)
    general, _ = merge(batch, None, False, 0, False)
    for l, (n, D, K) in enumerate(_census(batch)):
        r0, r1 = int(batch.log_off[l]), int(batch.log_off[l + 1])
        at, bat = int(lib.ptx_emu_orderwords_off(r0, l)), int(lib.ptx_emu_orderwords_bits_off(r0, l))
        ins = np.flatnonzero(batch.action[r0:r1] == abi.ACT_INSERT)
        ids = batch.op_id[r0:r1][ins]
        by_key = ins[np.lexsort((ids & 0xFFFFFFFF, ids >> 32))]  # the rows of the elements, ascending id
        words = w.ow[at: at + n]
        assert np.array_equal(words & 0xFFFF, by_key.astype(np.uint32)), (names[l], "rows")
        rank = general.elem_rank[r0:r1][by_key]
        assert np.array_equal(words >> 16, rank & ~np.uint32(abi.RANK_TOMBSTONE)), (names[l], "positions")
        tomb = np.array([(int(w.ob[bat + (e >> 5)]) >> (e & 31)) & 1 for e in range(n)], dtype=bool)
        assert np.array_equal(tomb, (rank & abi.RANK_TOMBSTONE) != 0), (names[l], "tombstones")
        assert sorted((words >> 16).tolist()) == list(range(n)), (names[l], "the positions are a permutation")
        if n:
            assert np.all(w.ow[at + ((n + 3) & ~3): at + (r1 - r0) + 5] == 0xEEEEEEEE), (names[l], "nothing behind the last group of four")


def test_a_log_that_does_not_stand_runs_the_tree_again():
    """A reader that finds a log's order word at 0 — or at anything but its row count — runs all of P3, and answers the same; its neighbours do not."""
    batch, exp, names = W.shapes(EMU_S, EMU_T)
    w = Words(batch)
    _, c_plain = _plain(batch, 0, True)
    first, _ = merge(batch, w, True, 0, True)
    N = _rows(batch)
    w.ostand[0::3] = 0
    w.ostand[1::3] = N[1::3] + 1
    res, c = merge(batch, w, False, 2, True)
    want = _full(c_plain, gathers=False, checks=False)
    want[2::3] = 0
    assert np.array_equal(c, want) and same_results(first, res, batch)
    # ... nor a log whose operand words do not stand: the order words are read only beside them
    w.ostand[:] = N
    w.stand[0::2] = 0
    res, c = merge(batch, w, False, 1, True)
    want = _full(c_plain)
    want[1::2] = 0
    assert np.array_equal(c, want) and same_results(first, res, batch)


@pytest.mark.parametrize("lean", [False, True])
def test_a_failing_log_never_stands_and_fails_alike_in_every_run(lean):
    """An unknown parent, a delete of an unknown element, a parent's row after the child's, a delete's row before its target's — each leaves in P3a or P3b — and
    an op id on two rows, which leaves in P1: none of them ever stands, every run takes the full path and reports the same status and row."""
    batch, exp, codes, fails = W.failing(EMU_S, EMU_T)
    N = _rows(batch)
    plain, c_plain = _plain(batch, 1, lean)
    w = Words(batch)
    runs = []
    for k, order in enumerate((0, 1, 2, 0)):
        res, c = merge(batch, w, k == 0, order, lean)
        for l in range(batch.n_logs):
            assert int(res.logs["status"][l]) == codes[l], (k, l, fails[l])
            assert int(w.ostand[l]) == (0 if codes[l] else int(N[l])), (k, l, fails[l])
            if not codes[l]:
                H.check_log(batch, res, l, exp[l])
                assert c[l].tolist() == (c_plain[l].tolist() if k == 0 else [0, 0, 0] if lean else [1, 0, int(c_plain[l][2])]), (k, l)
            elif fails[l] != "p1_duplicate_id":
                assert int(c[l][0]) == 1, "a log that does not stand enters P3 in every run"
        runs.append(res)
    # (which of two rows with one id is "the repeat" depends on the lane order, merge_core.h: of that log the status alone is compared — asserted above)
    keep = [l for l in range(batch.n_logs) if fails[l] != "p1_duplicate_id"]
    for r in runs[1:] + [plain]:
        assert np.array_equal(runs[0].logs[keep], r.logs[keep]), "the same status and row from the writer, from every reader and without an index"


def test_a_log_that_fails_behind_the_tree_stands_and_repeats_its_error():
    """A comment id beyond the header's n_comment_ids: the log passes P3 — its order words stand — and raises PTX_ERR_BAD_OP in P5a, at the same row, in the
    writer and in every reader; the other logs answer like the oracle."""
    batch, bad, row, exp = W.bad_comment()
    N = _rows(batch)
    plain, _ = merge(batch, None, False, 0, True)
    assert int(plain.logs["status"][bad]) == abi.ERR_BAD_OP
    w = Words(batch)
    for k, order in enumerate((0, 1, 2)):
        res, c = merge(batch, w, k == 0, order, True)
        assert np.array_equal(w.ostand, N) and np.array_equal(w.stand, N)
        assert np.array_equal(res.logs, plain.logs), (k, "status, row and LDS high-water mark of every log")
        assert k == 0 or not c.any()
        for l in range(batch.n_logs):
            if l != bad:
                H.check_log(batch, res, l, exp[l])


def _write_batch(path, batch):
    with open(path, "wb") as f:
        n_changes = int(batch.chg_off[-1])
        f.write(np.array([batch.n_logs, batch.n_ops, n_changes, batch.max_actors, abi.env_stride(batch.max_actors)], dtype=np.uint64).tobytes())
        for name, dt in (("log_off", np.uint64), ("op_id", np.uint64), ("ref_a", np.uint64), ("ref_b", np.uint64), ("payload", np.uint32), ("action", np.uint8),
                         ("mark_type", np.uint8), ("side_a", np.uint8), ("side_b", np.uint8), ("chg_off", np.uint64), ("chg_hdr", np.uint32), ("chg_env", np.uint16)):
            col = np.ascontiguousarray(getattr(batch, name), dtype=dt)
            f.write(col[: {"log_off": batch.n_logs + 1, "chg_off": batch.n_logs + 1, "chg_hdr": n_changes, "chg_env": n_changes * abi.env_stride(batch.max_actors)}.get(name, batch.n_ops)].tobytes())


def test_sanitizer_program_writer_and_readers(tmp_path):
    """tests/emu/emu_orderwords_main.cc: the same entry over the cases' batch and over the failing logs, every block exactly as large as the host library makes
    it, compiled with -fsanitize=address,undefined and run as a child process (nothing sanitized is loaded into this interpreter).  Write, then three reads."""
    batch, _, _ = W.shapes(EMU_S, EMU_T)
    fb, _, codes, _ = W.M.failing(EMU_S, EMU_T)  # (without the repeated id: the row that log names depends on the lane order, the program compares whole result rows)
    good, bad = str(tmp_path / "batch.bin"), str(tmp_path / "failing.bin")
    _write_batch(good, batch)
    _write_batch(bad, fb)
    exe = str(tmp_path / "emu_orderwords_main")
    src = os.path.join(H.ROOT, "tests", "emu", "emu_orderwords_main.cc")
    # (-g1: line tables are all a report needs; full debug info doubles the compile)
    b = subprocess.run(["g++", "-O1", "-g1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    for lean in ("0", "1"):
        p = subprocess.run([exe, good, lean], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
        assert "0 disagreements" in p.stdout and " %d order words stand" % batch.n_logs in p.stdout, p.stdout
        if lean == "1":
            assert "0 tree passes by the readers of standing logs" in p.stdout, p.stdout
        p = subprocess.run([exe, bad, lean], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
        assert "0 disagreements" in p.stdout and " %d order words stand" % sum(1 for c in codes if not c) in p.stdout, p.stdout
