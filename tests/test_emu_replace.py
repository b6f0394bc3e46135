"""Find and replace on resident text views (peritext_amd/csrc/replace_core.h: the greedy choice by pointer doubling, the whole-element test, the ops in descending
order) on the CPU emulation, in every lane order.  The cases and their expected values are tests/replace_cases.py's; tests/test_gpu_replace.py repeats them through
the C ABI.  The view and its hits are made by tests/test_emu_view.py's emulation (count, positions, locate: unchanged passes); every output of the new passes is
pre-filled with 0xA5 and guarded on both sides."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import find_cases as FC
import helpers as H
import replace_cases as RC
import test_emu_slices as TS
import test_emu_view as TV
import text_cases as TC
from peritext_amd import abi, wire

EMU_REPLACE_LIB = os.path.join(H.ROOT, "tests", "emu", "libperitext_emu_replace.so")
needs_emu = [pytest.mark.skipif(not os.path.exists(EMU_REPLACE_LIB), reason="tests/emu/libperitext_emu_replace.so not built (run __graft_entry__.build())")] + TV.needs_emu
ORDERS = [0, 1, 2]


def emu(fn):
    for m in needs_emu:
        fn = m(fn)
    return fn


def test_the_entry_points_are_declared():
    """The symbols and the struct stand in the C header and in the ctypes prototypes, the ABI version is still 7, the row limit has one name shared with
    ptx_change, the build's no-spill guard names the new kernels and the build makes the emulation library (no skip: this one needs no library)."""
    with open(os.path.join(H.ROOT, "include", "peritext_hip.h")) as f:
        header = f.read()
    for name, nargs in (("ptx_view_replace_plan", 9), ("ptx_replace_plan_free", 1)):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in abi.FUNCTIONS and len(abi.FUNCTIONS[name][1]) == nargs, name
    assert re.search(r"typedef\s+struct\s+ptx_replace_plan\s*\{", header) and "bridge.ts:425-446" in header
    assert re.search(r"#define\s+PTX_ABI_VERSION\s+7u", header), "the addition is purely additive"
    assert re.search(r"#define\s+PTX_CHANGE_ROWS_MAX\s+65534u", header) and abi.CHANGE_ROWS_MAX == 65534
    assert C.sizeof(abi.ptx_input_ops) == 8 + 10 * 8 and C.sizeof(abi.ptx_replace_plan) == 16 + 4 * 8 + C.sizeof(abi.ptx_input_ops) + 8
    with open(os.path.join(H.ROOT, "peritext_amd", "csrc", "peritext_hip.hip")) as f:
        assert "rows > PTX_CHANGE_ROWS_MAX" in f.read(), "ptx_change checks the same limit by the same name"
    with open(os.path.join(H.ROOT, "__graft_entry__.py")) as f:
        entry = f.read()
    guard = re.search(r"NO_SPILL_KERNELS = \((.*?)\)", entry, re.S).group(1)
    for k in ("ptx_replace_select_kernel", "ptx_replace_emit_kernel"):
        assert '"%s"' % k in guard, "the build's no-spill guard names " + k
    assert "libperitext_emu_replace.so" in entry
    assert hasattr(wire, "ReplacePlan") and hasattr(wire, "decode_input_ops")


class EmuReplaceIn(C.Structure):
    _fields_ = [("status", C.c_void_p), ("pre_off", C.c_void_p), ("pre", C.c_void_p), ("hit_off", C.c_void_p), ("hit_unit", C.c_void_p), ("hit_start", C.c_void_p),
                ("hit_end", C.c_void_p), ("n_logs", C.c_uint32), ("n_pattern", C.c_uint32), ("n_replacement", C.c_uint32), ("first_log", C.c_uint32), ("n_batch_logs", C.c_uint32)]


def _lib():
    lib = C.CDLL(EMU_REPLACE_LIB)
    for f in ("ptx_emu_replace_check", "ptx_emu_replace_select", "ptx_emu_replace_emit"):
        getattr(lib, f).restype = C.c_int
    assert lib.ptx_emu_replace_tile() == abi.REPLACE_TILE and lib.ptx_emu_replace_rows_max() == abi.CHANGE_ROWS_MAX
    return lib


vp, u32 = TV.vp, TV.u32


def emu_plan(v, pattern, nocase, ids, n_batch, reverse, has_replacement=True):
    """ptx_view_replace_plan over the emulated view `v` (test_emu_view.EmuView): (return code, wire.ReplacePlan)."""
    lib, n, G = _lib(), v.n, TS.GUARD
    pat = TC.u16(pattern)
    flags = abi.FIND_ASCII_NOCASE if nocase is True else int(nocase)
    rc = lib.ptx_emu_replace_check(1, 1 if pattern is not None else 0, u32(len(pat)), u32(flags), int(has_replacement), u32(len(ids)), u32(v.first), u32(n), u32(n_batch))
    if rc != 0:
        return rc, None
    q = FC.Query(pattern, nocase=nocase)
    rc, counted = v._count(q)
    assert rc == 0
    n_matches, hit_off = counted[3], np.ascontiguousarray(counted[4])
    nh = int(hit_off[n])
    hu, hs, he = (np.ascontiguousarray(np.concatenate([a, np.zeros(0, np.uint32)])) for a in v._hits(q, counted))  # exactly nh words each
    one = np.zeros(1, np.uint32)
    keep = [np.ascontiguousarray(v.status) if n else one, np.ascontiguousarray(v.pre_off) if n else np.zeros(1, np.uint64), np.ascontiguousarray(v.pre[: max(v.n_pre, 0)]) if n and v.n_pre else one]
    a = EmuReplaceIn(keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, hit_off.ctypes.data, hu.ctypes.data if nh else None, hs.ctypes.data if nh else None,
                     he.ctypes.data if nh else None, n, len(pat), len(ids), v.first, n_batch)
    g32 = lambda c: TS._guarded(c, np.uint32)[0]  # noqa: E731
    g64 = lambda c: TS._guarded(c, np.uint64)[0]  # noqa: E731
    sel, st, nc, nr, nops, makes, chg, olo = g32(nh), g32(n), g32(n), g32(n), g32(n), g32(n_batch), g64(n_batch + 1), g64(n + 1)
    rc = lib.ptx_emu_replace_select(C.byref(a), C.c_int(reverse), TS._inner(sel, nh), TS._inner(st, n), TS._inner(nc, n), TS._inner(nr, n), TS._inner(nops, n), TS._inner(makes, n_batch),
                                    TS._inner(chg, n_batch + 1), TS._inner(olo, n + 1))
    assert rc == 0
    for buf, cnt in ((sel, nh), (st, n), (nc, n), (nr, n), (nops, n), (makes, n_batch)):
        assert TS._untouched(buf, 0xA5A5A5A5, cnt), "a word outside a per-hit or per-log array was written"
    assert TS._untouched(chg, 0xA5A5A5A5A5A5A5A5, n_batch + 1) and TS._untouched(olo, 0xA5A5A5A5A5A5A5A5, n + 1)
    if nh:
        assert (sel[G : G + nh] != 0xA5A5A5A5).all(), "every hit has its flag"
    n_chg, ni = int(chg[G + n_batch]), int(olo[G + n])
    oo, ix, ct, pl = g64(n_chg + 1), g32(ni), g32(ni), g32(ni)
    (ac, f8), (mt, _) = TS._guarded(ni, np.uint8), TS._guarded(ni, np.uint8)
    rc = lib.ptx_emu_replace_emit(C.byref(a), C.c_int(reverse), TS._inner(sel, nh), TS._inner(nr, n), TS._inner(nops, n), TS._inner(chg, n_batch + 1), TS._inner(olo, n + 1),
                                  TS._inner(oo, n_chg + 1), TS._inner(ac, ni), TS._inner(mt, ni), TS._inner(ix, ni), TS._inner(ct, ni), TS._inner(pl, ni))
    assert rc == 0
    assert TS._untouched(oo, 0xA5A5A5A5A5A5A5A5, n_chg + 1) and TS._untouched(ac, f8, ni) and TS._untouched(mt, f8, ni), "a word outside op_off or a byte outside a column was written"
    for buf in (ix, ct, pl):
        assert TS._untouched(buf, 0xA5A5A5A5, ni)
    assert (oo[G : G + n_chg + 1] != 0xA5A5A5A5A5A5A5A5).all() and (ix[G : G + ni] != 0xA5A5A5A5).all() and (ac[G : G + ni] != 0xA5).all(), "every op and every op_off entry is written"
    cut = lambda b, c: b[G : G + c].copy()  # noqa: E731
    ops = wire.InputOps(cut(chg, n_batch + 1), cut(oo, n_chg + 1), cut(ac, ni), cut(mt, ni), cut(ix, ni), cut(ct, ni), cut(pl, ni), np.asarray(ids, np.uint32).copy(), None, 0)
    return 0, wire.ReplacePlan(status=cut(st, n), n_matches=n_matches, n_chosen=cut(nc, n), n_replaced=cut(nr, n), ops=ops, first_log=v.first, n_pattern=len(pat), n_replacement=len(ids))


class EmuReplaceView(TV.EmuView):
    def replace_plan(self, ask, n_batch):
        _, ids = RC.ids_of(self.suite, ask)
        rc, plan = emu_plan(self, ask.pattern, ask.nocase, ids, n_batch, self.reverse)
        assert rc == 0
        return plan


def opener(reverse):
    return lambda suite, first, n: EmuReplaceView(suite, first, n, reverse)


@emu
@pytest.mark.parametrize("reverse", ORDERS)
def test_cases_in_every_lane_order(reverse):
    changes = replaced = skipped = 0
    for ask in RC.asks():
        c, r, s = RC.run_ask(opener(reverse), ask)
        changes, replaced, skipped = changes + c, replaced + r, skipped + s
    assert changes > 40 and replaced > 1000 and skipped >= 5, "Changes were planned, matches replaced, and some skipped inside an element"


@emu
@pytest.mark.parametrize("reverse", ORDERS)
def test_known_answer_documents(reverse):
    suite = TC.kat_suite()
    n = suite.batch.n_logs
    with EmuReplaceView(suite, 0, n, reverse) as v:  # ONE view, two plans
        for ask in RC.kat_asks():
            table, _ = RC.ids_of(suite, ask)
            c, r, _ = RC.check_plan(suite, v.rows, v.replace_plan(ask, n), 0, n, n, ask, table)
            assert c > 0 and r >= c, "some documents hold the pattern"


@emu
def test_the_empty_view_and_invalid_arguments():
    suite = TC.failed_log_suite()
    ids = np.array([1, 2], np.uint32)
    with EmuReplaceView(suite, 3, 0, 0) as v:  # an empty range at the end of the batch: the all-zero plan
        rc, p = emu_plan(v, "a", False, ids, 5, 0)
        assert rc == 0 and len(p.status) == 0 and [int(x) for x in p.ops.chg_off] == [0] * 6 and [int(x) for x in p.ops.op_off] == [0] and len(p.ops.action) == 0
    with EmuReplaceView(suite, 1, 2, 0) as v:
        bad = [dict(pattern=""), dict(pattern="a" * (abi.FIND_PATTERN_MAX + 1)), dict(nocase=2), dict(nocase=0x80000000), dict(ids=np.zeros(abi.CHANGE_ROWS_MAX + 1, np.uint32)),
               dict(has_replacement=False), dict(n_batch=2), dict(n_batch=0)]
        for kw in bad:
            args = dict(pattern="a", nocase=False, ids=ids, n_batch=3, has_replacement=True)
            args.update(kw)
            assert emu_plan(v, args["pattern"], args["nocase"], args["ids"], args["n_batch"], 0, args["has_replacement"])[0] == abi.ERR_INVALID_ARG, kw
        assert emu_plan(v, "a", False, np.zeros(0, np.uint32), 3, 0, has_replacement=False)[0] == 0, "no replacement: a NULL pointer is legal"
        assert emu_plan(v, "a", False, np.zeros(abi.CHANGE_ROWS_MAX, np.uint32), 3, 0)[0] == 0
        assert _lib().ptx_emu_replace_check(0, 1, u32(1), u32(0), 1, u32(1), u32(0), u32(0), u32(0)) == abi.ERR_INVALID_ARG, "the NULL view"


@emu
def test_sanitizer_program(tmp_path):
    """tests/emu/emu_replace_main.cc: select, the scans and emit over hit lists built in the file, against a sequential greedy loop inside the file, compiled with
    -fsanitize=address,undefined and run as a child process (the hit and flag arrays end exactly at their last element)."""
    exe = str(tmp_path / "emu_replace_main")
    src = os.path.join(H.ROOT, "tests", "emu", "emu_replace_main.cc")
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "replace emulation ok" in r.stdout
