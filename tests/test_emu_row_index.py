"""The merge kernel's row index (merge_core.h ptx_row_index_off) through the host emulation, no GPU: every batch is merged three times with one caller-held
index — the writer, then two readers in other lane orders.  Status, counts, digests and rows are the oracle's in all three runs and identical between them;
rows_indexed == N exactly for the logs that pass P1's checks; the readers take no full row pass for those logs and the full pass, with the same code and row,
for every log that fails one of P1's checks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import row_index_cases as R
from peritext_amd import abi, wire

LIB = os.path.join(H.ROOT, "tests", "emu", "libperitext_emu_rowindex.so")


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    assert H.have_node(), "these cases need node, the oracle's runtime: a skipped case would hide exactly what this file exists to show"


class Index:
    """The caller-held index of one batch: what the host library keeps beside a resident batch."""

    def __init__(self, b):
        lib = C.CDLL(LIB)
        for name in ("ptx_emu_rowindex_words", "ptx_emu_rowindex_bits_words", "ptx_emu_rowindex_off", "ptx_emu_rowindex_full_passes"):
            getattr(lib, name).restype = C.c_ulonglong
            getattr(lib, name).argtypes = [] if name.endswith("passes") else [C.c_ulonglong, C.c_ulonglong]
        self.lib = lib
        self.words = np.full(int(lib.ptx_emu_rowindex_words(b.n_ops, b.n_logs)), 0xEEEEEEEE, dtype=np.uint32)  # (never zeroed by the library either)
        self.bits = np.full(int(lib.ptx_emu_rowindex_bits_words(b.n_ops, b.n_logs)), 0xEEEEEEEE, dtype=np.uint32)
        self.rows_indexed = np.zeros(max(b.n_logs, 1), dtype=np.uint32)

    def region(self, b, log):
        o = int(self.lib.ptx_emu_rowindex_off(int(b.log_off[log]), log))
        return self.words[o: o + int(b.log_off[log + 1] - b.log_off[log]) + 5]  # (a region holds N + 5 words at least)


def merge(b, ix, write, reverse=0, lean=False):
    """-> (Results, full_pass[n_logs]) of ptx_emu_merge_rowindex over a wire.Batch; ix: Index or None."""
    n = max(b.n_ops, 1)
    res = wire.Results(
        logs=np.zeros(b.n_logs, dtype=abi.LOG_RESULT_DTYPE),
        values=np.full(n, 0xDEADBEEF, dtype=np.uint32),
        spans=np.zeros(n, dtype=abi.SPAN_DTYPE),
        cintervals=np.zeros(n, dtype=abi.CINTERVAL_DTYPE),
        elem_rank=None if lean else np.zeros(n, dtype=np.uint32),
        ref_slots=None if lean else np.full(n, 0xFFFFFFFF, dtype=np.uint32),
    )
    full = np.zeros(max(b.n_logs, 1), dtype=np.uint8)
    s = H.batch_struct(b)
    f = C.CDLL(LIB).ptx_emu_merge_rowindex
    f.restype = C.c_int
    f.argtypes = [C.POINTER(abi.ptx_batch)] + [C.c_void_p] * 9 + [C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_int]
    rc = f(C.byref(s), res.logs.ctypes.data, res.values.ctypes.data, res.spans.ctypes.data, res.cintervals.ctypes.data,
           None if lean else res.elem_rank.ctypes.data, None if lean else res.ref_slots.ctypes.data,
           None if ix is None else ix.words.ctypes.data, None if ix is None else ix.bits.ctypes.data, None if ix is None else ix.rows_indexed.ctypes.data,
           1 if write else 0, full.ctypes.data, H.LDS_BYTES, reverse, 1 if lean else 0)
    assert rc == 0
    return res, full[: b.n_logs]


def same_results(a, b, batch):
    """The result rows, and of every log that passes its values / span rows / comment intervals (rows beyond a log's counts are scratch)."""
    if not np.array_equal(a.logs, b.logs):
        return False
    for l in range(batch.n_logs):
        if int(a.logs["status"][l]):
            continue
        r0 = int(batch.log_off[l])
        for k, cnt in (("values", "n_visible"), ("spans", "n_spans"), ("cintervals", "n_cintervals")):
            c = int(a.logs[cnt][l]) if cnt in a.logs.dtype.names else 0
            if not np.array_equal(getattr(a, k)[r0: r0 + c], getattr(b, k)[r0: r0 + c]):
                return False
    return True


@pytest.mark.parametrize("orders,lean", [((0, 1, 2), True), ((2, 0, 1), False), ((1, 2, 0), True), ((0, 2, 1), False)])
def test_write_read_read_answers_like_the_oracle_at_the_edges_of_the_indexed_pass(orders, lean):
    batch, exp, shapes = R.shapes()
    assert {n for n, D, K in shapes} >= {0, 1, 3, 4, 5, 255, 256, 257, 511, 512, 513, 767, 768, 769} and {K for n, D, K in shapes} >= {0, 31, 32, 33}
    assert any(D == 0 for n, D, K in shapes) and {1 + n + D + K for n, D, K in shapes} >= {257, 1025}
    ix = Index(batch)
    plain, full0 = merge(batch, None, False, orders[0], lean)
    assert full0.all(), "without an index every log takes the full row pass"
    runs = []
    for k, order in enumerate(orders):
        res, full = merge(batch, ix, k == 0, order, lean)
        for l in range(batch.n_logs):
            H.check_log(batch, res, l, exp[l])
        N = (batch.log_off[1:] - batch.log_off[:-1]).astype(np.uint32)
        assert np.array_equal(ix.rows_indexed, N), "every log that passes P1's checks is indexed, with its row count"
        assert full.all() if k == 0 else not full.any(), (k, full.tolist())
        runs.append(res)
    assert same_results(runs[0], runs[1], batch) and same_results(runs[0], runs[2], batch), "the order of a log's lists decides nothing"
    assert same_results(runs[0], plain, batch), "... and a merge without an index answers the same, LDS high-water mark included"
    # what the writer left: the inserts' words first, then — from the next multiple of four words — the deletes', then the mark ops': every listed row exactly once
    for l, (n, D, K) in enumerate(shapes):
        n4 = (n + 3) & ~3
        reg = ix.region(batch, l)
        rows = np.concatenate([reg[:n], reg[n4: n4 + D + K]]) & 0xFFFF
        lo = int(batch.log_off[l])
        act = batch.action[lo + rows.astype(np.int64)]
        assert len(set(rows.tolist())) == n + D + K
        assert (act[:n] == abi.ACT_INSERT).all() and (act[n: n + D] == abi.ACT_DELETE).all() and np.isin(act[n + D:], (abi.ACT_ADDMARK, abi.ACT_REMOVEMARK)).all()


def test_a_reader_that_finds_no_index_parks_in_its_own_rows_and_writes_nothing():
    """A launch that may only read (another launch is the batch's writer) and finds rows_indexed 0: today's pass, and the index stays as it was."""
    batch, exp, _ = R.shapes()
    ix = Index(batch)
    res, full = merge(batch, ix, False, 1, True)
    assert full.all() and not ix.rows_indexed.any() and (ix.words == 0xEEEEEEEE).all() and (ix.bits == 0xEEEEEEEE).all()
    for l in range(batch.n_logs):
        H.check_log(batch, res, l, exp[l])
    ix.rows_indexed[:] = 7  # neither 0 nor N: no index
    res2, full2 = merge(batch, ix, False, 0, True)
    N = batch.log_off[1:] - batch.log_off[:-1]
    assert full2[N != 7].all() and same_results(res, res2, batch)


def _failing_batches():
    """[(batch, {log: (code, row or None)})]: a malformed action, a mark type above 3, an op id beyond the header's bounds, a header that lies about a class
    count (helpers.malformed_row_batches), a repeated op id (helpers.duplicate_op_docs)."""
    base, cases = H.malformed_row_batches()
    out = [(b, {l: (abi.ERR_BAD_OP, None) for l in want}) for b, want, _ in cases]
    dup = wire.encode_docs(H.duplicate_op_docs())
    out.append((dup, {0: (abi.ERR_DUPLICATE_OP, None)}))
    return out


@pytest.mark.parametrize("lean", [False, True])
def test_logs_that_fail_a_check_of_the_row_pass_are_never_indexed(lean):
    """Each failing log leaves rows_indexed 0, takes the full pass in every run and fails with the same code in every run.  The error ROW is compared across the
    runs for the malformed / out-of-bounds / lying-header logs only: of a repeated op id the kernel names one of the id's two rows, whichever its lanes meet
    second (merge_core.h: "the status is what is reported"), and the three runs differ in lane order on purpose — for those logs this asserts less than
    "the same code and row in every run": the code alone."""
    for batch, want in _failing_batches():
        ix = Index(batch)
        first = None
        for k, order in enumerate((0, 1, 2)):
            res, full = merge(batch, ix, k == 0, order, lean)
            N = (batch.log_off[1:] - batch.log_off[:-1]).astype(np.uint32)
            for l in range(batch.n_logs):
                st = int(res.logs["status"][l])
                if l in want:
                    assert st == want[l][0] and int(ix.rows_indexed[l]) == 0 and full[l], (l, st, int(ix.rows_indexed[l]), int(full[l]))
                else:
                    assert st == 0 and int(ix.rows_indexed[l]) == int(N[l]) and bool(full[l]) == (k == 0), (l, st, k)
            if first is None:
                first = res
            else:  # the same code and the same row in every run (a repeated id names one of its two rows: the status is what is reported)
                assert np.array_equal(first.logs["status"], res.logs["status"])
                bad_op = [l for l in want if want[l][0] == abi.ERR_BAD_OP]
                assert np.array_equal(first.logs["reserved"][bad_op, 1], res.logs["reserved"][bad_op, 1])
                keep = [l for l in range(batch.n_logs) if want.get(l, (0,))[0] != abi.ERR_DUPLICATE_OP]
                assert np.array_equal(first.logs[keep], res.logs[keep])
        # ... and the rows the helpers pin (tests/test_emu_merge.py's own check, through this driver's reading runs)
    H.check_malformed_rows(lambda b: merge(b, _kept_index(b), False, 0, lean)[0])


_KEPT = {}


def _kept_index(b):
    """An index per batch object that a writing merge has filled before: check_malformed_rows then goes through reading merges."""
    if id(b) not in _KEPT:
        ix = Index(b)
        merge(b, ix, True, 2, False)
        _KEPT[id(b)] = (b, ix)
    return _KEPT[id(b)][1]


def test_sanitizer_program_write_read_read(tmp_path):
    """tests/emu/emu_rowindex_main.cc: the same entry over the shapes' batch, every block exactly as large as the host library makes it, compiled with
    -fsanitize=address,undefined and run as a child process (nothing sanitized is loaded into this interpreter)."""
    batch, _, _ = R.shapes()
    path = str(tmp_path / "batch.bin")
    with open(path, "wb") as f:
        n_changes = int(batch.chg_off[-1])
        f.write(np.array([batch.n_logs, batch.n_ops, n_changes, batch.max_actors, abi.env_stride(batch.max_actors)], dtype=np.uint64).tobytes())
        for name, dt in (("log_off", np.uint64), ("op_id", np.uint64), ("ref_a", np.uint64), ("ref_b", np.uint64), ("payload", np.uint32), ("action", np.uint8),
                         ("mark_type", np.uint8), ("side_a", np.uint8), ("side_b", np.uint8), ("chg_off", np.uint64), ("chg_hdr", np.uint32), ("chg_env", np.uint16)):
            col = np.ascontiguousarray(getattr(batch, name), dtype=dt)
            f.write(col[: {"log_off": batch.n_logs + 1, "chg_off": batch.n_logs + 1, "chg_hdr": n_changes, "chg_env": n_changes * abi.env_stride(batch.max_actors)}.get(name, batch.n_ops)].tobytes())
    exe = str(tmp_path / "emu_rowindex_main")
    src = os.path.join(H.ROOT, "tests", "emu", "emu_rowindex_main.cc")
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    for lean in ("0", "1"):
        p = subprocess.run([exe, path, lean], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
        assert "0 disagreements" in p.stdout and " %d full row passes" % batch.n_logs in p.stdout, p.stdout  # (the writer's, one per log)
