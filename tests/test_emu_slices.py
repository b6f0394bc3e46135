"""Text and span rows of element ranges (peritext_amd/csrc/slice_core.h: plan, prefix, bounds, scan, copy, span emit over the text text_core.h assembles) on the CPU
emulation, in every lane order.  The cases and their expected values are tests/slice_cases.py's (plain Python slices of the oracle's text, the oracle's spans cut
by a plain loop, element boundaries from the merge's value ids); tests/test_gpu_slices.py repeats them through the C ABI.  The text the slices are cut from is the
text emulation's own output for the same range (tests/test_emu_text.py checks that one), the merge results are the emulation's merge of the same batch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
import slice_cases as SC
import test_emu_text as TE
import text_cases as TC
from peritext_amd import abi, wire

EMU_SLICE_LIB = os.path.join(H.ROOT, "tests", "emu", "libperitext_emu_slice.so")
needs_emu = [pytest.mark.skipif(not os.path.exists(EMU_SLICE_LIB) or not os.path.exists(TE.EMU_TEXT_LIB), reason="tests/emu/libperitext_emu_slice.so not built (run __graft_entry__.build())"),
             pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")]
GUARD = 64  # words of 0xA5 before and behind every output array


def emu(fn):
    for m in needs_emu:
        fn = m(fn)
    return fn


def test_the_entry_points_are_declared():
    """The symbols and the struct stand in the C header and in the ctypes prototypes, the block size is mirrored, the ABI version is still 7 and the build's
    no-spill guard names the kernels (no skip: this one needs no library)."""
    with open(os.path.join(H.ROOT, "include", "peritext_hip.h")) as f:
        header = f.read()
    for name, nargs in (("ptx_result_text_slices", 10), ("ptx_slices_free", 1)):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in abi.FUNCTIONS and len(abi.FUNCTIONS[name][1]) == nargs, name
    assert re.search(r"typedef\s+struct\s+ptx_slices\s*\{", header)
    assert re.search(r"#define\s+PTX_ABI_VERSION\s+7u", header), "the addition is purely additive"
    assert C.sizeof(abi.ptx_slices) == 16 + 9 * 8
    head = lambda s: [f[0] for f in s._fields_[:4]]  # noqa: E731
    assert head(abi.ptx_slices) == ["n_logs", "n_slices", "kernel_ms", "reserved"] and [f[1] for f in abi.ptx_slices._fields_[:4]] == [f[1] for f in abi.ptx_matches._fields_[:4]]
    with open(os.path.join(H.ROOT, "peritext_amd", "csrc", "slice_core.h")) as f:
        core = f.read()
    assert int(re.search(r"#define\s+PTX_SLICE_BLOCK\s+(\d+)u", core).group(1)) == abi.SLICE_BLOCK
    with open(os.path.join(H.ROOT, "__graft_entry__.py")) as f:
        entry = f.read()
    guard = re.search(r"NO_SPILL_KERNELS = \((.*?)\)", entry, re.S).group(1)
    for k in ("ptx_slice_prefix_kernel", "ptx_slice_bounds_kernel", "ptx_slice_copy_kernel", "ptx_slice_span_kernel"):
        assert '"%s"' % k in guard, "the build's no-spill guard names " + k
    assert "libperitext_emu_slice.so" in entry
    assert hasattr(wire, "Slices") and hasattr(wire, "decode_slice_spans")


def _guarded(count, dtype):
    fill = {1: 0xA5, 2: 0xA5A5, 4: 0xA5A5A5A5, 8: 0xA5A5A5A5A5A5A5A5}[np.dtype(dtype).itemsize]
    return np.full(2 * GUARD + count, fill, dtype), fill


def _inner(buf, count):
    return C.c_void_p(buf.ctypes.data + GUARD * buf.itemsize)


def _untouched(buf, fill, count):
    return (buf[:GUARD] == fill).all() and (buf[GUARD + count :] == fill).all()


def emu_slices(batch, res, table, text, first, n, arrays, reverse=0):
    """ptx_result_text_slices' passes behind the text passes over host arrays: (return code, wire.Slices).  arrays: (slice_off, slice_start, slice_end) or None
    in their places.  Every output is pre-filled with 0xA5 and guarded by 64 words on both sides."""
    lib = C.CDLL(EMU_SLICE_LIB)
    lib.ptx_emu_slices_bounds.restype = lib.ptx_emu_slices_emit.restype = C.c_int
    assert lib.ptx_emu_slice_block() == abi.SLICE_BLOCK
    vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(None)  # noqa: E731
    u32 = C.c_uint32
    off, start, end = arrays
    ns = int(off[n]) if off is not None and n and int(off[n]) <= 0xFFFFFFFF else 0
    keep = [np.ascontiguousarray(x) if x is not None else None for x in (off, start, end)]
    if keep[1] is not None and len(keep[1]) == 0:
        keep[1] = keep[2] = np.zeros(1, np.uint32)
    status = np.ascontiguousarray(np.concatenate([text.status, np.zeros(1, np.uint32)])[: max(n, 1)].astype(np.uint32))
    toff = np.ascontiguousarray(np.concatenate([text.text_off, text.span_off]).astype(np.uint64))
    units = text.text[: len(text.text)].astype(np.uint16).copy() if len(text.text) else np.zeros(1, np.uint16)  # exactly the text
    soff = TC.table_arrays(table)[1]
    (ea, f32), (eb, _), (oo, f64) = _guarded(ns, np.uint32), _guarded(ns, np.uint32), _guarded(2 * (ns + 1), np.uint64)
    handle = C.c_void_p()
    rc = lib.ptx_emu_slices_bounds(vp(batch.log_off), u32(batch.n_logs), vp(res.logs), vp(res.values), vp(res.spans), vp(soff), u32(len(table)), u32(first), u32(n), vp(status), vp(toff),
                                   vp(units), vp(keep[0]), vp(keep[1]), vp(keep[2]), C.c_int(reverse), _inner(ea, ns), _inner(eb, ns), _inner(oo, 2 * (ns + 1)), C.byref(handle))
    if rc != 0:
        return rc, None
    try:
        assert _untouched(ea, f32, ns) and _untouched(eb, f32, ns) and _untouched(oo, f64, 2 * (ns + 1)), "a word outside the per-slice arrays was written"
        out_off = oo[GUARD : GUARD + 2 * (ns + 1)].copy()
        unit_off, sspan_off = out_off[: ns + 1], out_off[ns + 1 :]
        nu, nr = int(unit_off[ns]), int(sspan_off[ns])
        (ot, f16), (os_, _), (ou, _) = _guarded(nu, np.uint16), _guarded(2 * nr, np.uint32), _guarded(nr, np.uint32)
        rc = lib.ptx_emu_slices_emit(handle, C.c_int(reverse), _inner(ot, nu), _inner(os_, 2 * nr), _inner(ou, nr))
        assert rc == 0
        assert _untouched(ot, f16, nu) and _untouched(os_, f32, 2 * nr) and _untouched(ou, f32, nr), "a word outside the output was written"
    finally:
        lib.ptx_emu_slices_close(handle)
    return 0, wire.Slices(status=text.status.copy(), slice_off=np.array(off, np.uint64) if n else np.zeros(1, np.uint64), elem_start=ea[GUARD : GUARD + ns].copy(),
                          elem_end=eb[GUARD : GUARD + ns].copy(), unit_off=unit_off, text=ot[GUARD : GUARD + nu].copy(), sspan_off=sspan_off,
                          sspans=os_[GUARD : GUARD + 2 * nr].copy().view(abi.SPAN_DTYPE), sspan_unit=ou[GUARD : GUARD + nr].copy())


_TEXT = {}


def assembled(suite, res, first, n, reverse):
    k = (suite.name, first, n, reverse)
    if k not in _TEXT:
        rc, text = TE.emu_text(suite.batch, res, suite.table, first, n, reverse)
        assert rc == 0
        _TEXT[k] = text
    return _TEXT[k]


def run_plan(suite, make_plan, reverse, first=0, n=None, decode=True):
    n = suite.batch.n_logs - first if n is None else n
    res = TE.merged(suite, reverse)
    rows = TE.compact(suite.batch, res, first, n)
    plan = make_plan(rows, n)
    rc, got = emu_slices(suite.batch, res, suite.table, assembled(suite, res, first, n, reverse), first, n, SC.arrays_of(plan), reverse)
    assert rc == 0
    SC.check_range(suite, rows, got, first, n, plan, decode=decode)
    return rows, plan, got


@emu
@pytest.mark.parametrize("reverse", [0, 1, 2])
def test_edges_in_every_lane_order(reverse):
    suite, _ = SC.edge_suite()
    _, _, got = run_plan(suite, lambda rows, n: SC.edge_plan_list(), reverse)
    SC.edge_hand_checks(got)


@emu
@pytest.mark.parametrize("reverse", [0, 1, 2])
def test_element_bounds_of_the_text_cases(reverse):
    suite = TC.edge_suite()
    _, plan, got = run_plan(suite, SC.plan_bounds, reverse)
    SC.text_edge_hand_checks(suite, got, plan)


@emu
@pytest.mark.parametrize("reverse", [0, 1, 2])
def test_orders_and_logs_without_slices(reverse):
    suite = TC.edge_suite()
    run_plan(suite, SC.plan_sparse, reverse)
    i = TC.edge_docs()[0].index("n63")
    run_plan(suite, SC.plan_sparse, reverse, first=i, n=4)  # a range that starts behind log 0
    run_plan(suite, SC.plan_bounds, reverse, first=i + 1, n=5)
    run_plan(suite, lambda rows, n: [[] for _ in range(n)], reverse)  # zero slices
    run_plan(suite, lambda rows, n: [], reverse, first=2, n=0)  # the empty range


@emu
@pytest.mark.parametrize("reverse", [0, 1, 2])
def test_failed_log_between_good_ones(reverse):
    suite = TC.failed_log_suite()
    _, _, got = run_plan(suite, SC.plan_bounds, reverse)
    k0, k1 = int(got.slice_off[1]), int(got.slice_off[2])
    assert k1 > k0 and not got.elem_start[k0:k1].any() and not got.elem_end[k0:k1].any() and int(got.unit_off[k1]) == int(got.unit_off[k0]) and int(got.sspan_off[k1]) == int(got.sspan_off[k0])
    run_plan(suite, SC.plan_bounds, reverse, first=1, n=2)


@emu
@pytest.mark.parametrize("reverse", [0, 1, 2])
def test_known_answer_documents(reverse):
    suite = TC.kat_suite()
    rows, plan, got = run_plan(suite, SC.plan_kat, reverse)
    SC.check_kat_literals(suite, rows, got, plan)


@emu
def test_invalid_arguments():
    suite = TC.failed_log_suite()
    res = TE.merged(suite, 0)
    text = assembled(suite, res, 0, 3, 0)
    off, start, end = SC.arrays_of([[(0, 1)], [], [(1, 2), (0, 9)]])
    bad = [(np.array([1, 1, 1, 3], np.uint64), start, end), (np.array([0, 2, 1, 3], np.uint64), start, end), (off, None, end), (off, start, None), (None, start, end),
           (np.array([0, 0, 0, 1 << 32], np.uint64), start, end)]
    for arrays in bad:
        assert emu_slices(suite.batch, res, suite.table, text, 0, 3, arrays)[0] == abi.ERR_INVALID_ARG
    assert emu_slices(suite.batch, res, suite.table, assembled(suite, res, 2, 1, 0), 2, 2, (np.zeros(3, np.uint64), None, None))[0] == abi.ERR_INVALID_ARG, "a range outside the batch"
    rc, got = emu_slices(suite.batch, res, suite.table, text, 0, 3, (np.zeros(4, np.uint64), None, None))
    assert rc == 0 and [int(x) for x in got.unit_off] == [0] and [int(x) for x in got.sspan_off] == [0] and len(got.text) == 0, "zero slices: NULL slice arrays are legal"


@emu
@pytest.mark.parametrize("reverse", [0, 1, 2])
def test_value_id_beyond_the_table(reverse):
    """One log with a value id equal to n_strings: PTX_ERR_BAD_OP, empty slices without rows; its neighbours are bit-equal to the run without it."""
    suite = TC.edge_suite()
    log = [k for k, w in enumerate(suite.want) if len(w.units) == TC.T + 1][0]
    bad, _ = TC.bad_id_batch(suite, log)
    n = suite.batch.n_logs
    good_rows, plan, good = run_plan(suite, SC.plan_bounds, reverse)
    res = TE.merged(suite, reverse, batch=bad)
    rc, text = TE.emu_text(bad, res, suite.table, 0, n, reverse)
    assert rc == 0
    rc, m = emu_slices(bad, res, suite.table, text, 0, n, SC.arrays_of(plan), reverse)
    assert rc == 0 and int(m.status[log]) == abi.ERR_BAD_OP
    SC.check_range(suite, good_rows, m, 0, n, plan, status_of={log: abi.ERR_BAD_OP}, decode=False)
    for k in range(n):
        if k == log:
            continue
        for j in range(len(plan[k])):
            a, b = good.index(k, j), m.index(k, j)
            assert good.of_slice(a) == m.of_slice(b) and good.rows_of_slice(a) == m.rows_of_slice(b) and (good.elem_start[a], good.elem_end[a]) == (m.elem_start[b], m.elem_end[b])


@emu
def test_sanitizer_program(tmp_path):
    """tests/emu/emu_slice_main.cc: all passes over tables, logs and slice lists built in the file, against a sequential cut inside the file, compiled with
    -fsanitize=address,undefined and run as a child process (every buffer exactly as large as the host library makes it)."""
    exe = str(tmp_path / "emu_slice_main")
    src = os.path.join(H.ROOT, "tests", "emu", "emu_slice_main.cc")
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "slice emulation ok" in r.stdout
