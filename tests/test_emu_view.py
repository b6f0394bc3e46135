"""Resident text views (peritext_amd/csrc/view_core.h: plan and prefix of every good log once; then count, positions, locate by binary search over the resident
prefix, windows with match_unit, and slice_core.h's passes over device-resident bounds) on the CPU emulation, in every lane order.  The cases and their expected
values are tests/view_cases.py's; tests/test_gpu_view.py repeats them through the C ABI.  Every output is pre-filled with 0xA5 and guarded on both sides; after a
view is made, the arrays it was made from (the batch's log_off, the result's value ids and per-log rows, the string table) are overwritten with 0xA5: a query that still read
them would show.  The twins a view's answers are compared with are the find and slice emulations of tests/test_emu_find.py and tests/test_emu_slices.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import find_cases as FC
import helpers as H
import slice_cases as SC
import test_emu_find as TF
import test_emu_slices as TS
import test_emu_text as TE
import text_cases as TC
import view_cases as VC
from peritext_amd import abi, wire

EMU_VIEW_LIB = os.path.join(H.ROOT, "tests", "emu", "libperitext_emu_view.so")
needs_emu = [pytest.mark.skipif(not all(os.path.exists(p) for p in (EMU_VIEW_LIB, TF.EMU_FIND_LIB, TS.EMU_SLICE_LIB, TE.EMU_TEXT_LIB)),
                                reason="tests/emu/libperitext_emu_view.so not built (run __graft_entry__.build())"),
             pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")]
ORDERS = [0, 1, 2]


def emu(fn):
    for m in needs_emu:
        fn = m(fn)
    return fn


def test_the_entry_points_are_declared():
    """The symbols and structs stand in the C header and in the ctypes prototypes, the ABI version is still 7, the build's no-spill guard names the new kernels and
    the build makes the emulation library (no skip: this one needs no library)."""
    with open(os.path.join(H.ROOT, "include", "peritext_hip.h")) as f:
        header = f.read()
    for name, nargs in (("ptx_text_view_create", 7), ("ptx_text_view_free", 2), ("ptx_view_info", 3), ("ptx_view_find_text", 7), ("ptx_view_text_slices", 6),
                        ("ptx_view_find_snippets", 9), ("ptx_snippets_free", 1)):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in abi.FUNCTIONS and len(abi.FUNCTIONS[name][1]) == nargs, name
    assert re.search(r"typedef\s+struct\s+ptx_dview\s+ptx_dview\s*;", header) and re.search(r"typedef\s+struct\s+ptx_snippets\s*\{", header)
    assert re.search(r"#define\s+PTX_ABI_VERSION\s+7u", header), "the addition is purely additive"
    assert C.sizeof(abi.ptx_snippets) == 16 + 15 * 8 and C.sizeof(abi.ptx_view_desc) == 8 + 3 * 8 + 8
    with open(os.path.join(H.ROOT, "__graft_entry__.py")) as f:
        entry = f.read()
    guard = re.search(r"NO_SPILL_KERNELS = \((.*?)\)", entry, re.S).group(1)
    for k in ("ptx_view_plan_kernel", "ptx_view_positions_kernel", "ptx_view_locate_kernel", "ptx_view_windows_kernel"):
        assert '"%s"' % k in guard, "the build's no-spill guard names " + k
    assert "libperitext_emu_view.so" in entry
    assert hasattr(wire, "Snippets")


def _lib():
    lib = C.CDLL(EMU_VIEW_LIB)
    for f in ("ptx_emu_view_create", "ptx_emu_view_count", "ptx_emu_view_hits", "ptx_emu_view_bounds", "ptx_emu_view_emit"):
        getattr(lib, f).restype = C.c_int
    assert lib.ptx_emu_view_find_step() == abi.FIND_STEP and lib.ptx_emu_view_slice_block() == abi.SLICE_BLOCK
    return lib


vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(None)  # noqa: E731
u32 = C.c_uint32


class EmuView:
    """A view of the logs [first, first + n) of the emulation's merge of a batch, and its twins: the interface tests/view_cases.py names."""

    def __init__(self, suite, first, n, reverse, batch=None):
        self.suite, self.first, self.n, self.reverse = suite, first, n, reverse
        self.batch = suite.batch if batch is None else batch
        self.res = TE.merged(suite, reverse, batch=batch)
        self.rows = TE.compact(self.batch, self.res, first, n) if first + n <= self.batch.n_logs else None
        self.lib, self.handle = _lib(), C.c_void_p()
        units, soff = TC.table_arrays(suite.table)
        units = np.concatenate([units, np.zeros(1, np.uint16)])[: max(len(units), 1)].copy()
        gone = [np.ascontiguousarray(self.batch.log_off).copy(), np.ascontiguousarray(self.res.values).copy(), units, soff.copy(), np.ascontiguousarray(self.res.logs).copy()]
        self.rc = self.lib.ptx_emu_view_create(vp(gone[0]), u32(self.batch.n_logs), vp(gone[4]), vp(gone[1]), vp(self.res.spans), vp(gone[2]), vp(gone[3]), u32(len(suite.table)),
                                               u32(first), u32(n), C.c_int(reverse), C.byref(self.handle))
        for a in gone:  # the batch and the strings "are freed": what a query reads of them now is 0xA5
            a.view(np.uint8)[:] = 0xA5
        self._gone = gone
        self._text = None
        if self.rc == 0:
            sizes = np.zeros(3, np.uint64)
            self.lib.ptx_emu_view_sizes(self.handle, vp(sizes))
            self.n_units, self.n_spans, self.n_pre = (int(x) for x in sizes)
            self.status, self.off = np.zeros(max(n, 1), np.uint32), np.zeros(2 * (n + 1), np.uint64)
            self.text, self.span_unit = np.zeros(max(self.n_units, 1), np.uint16), np.zeros(max(self.n_spans, 1), np.uint32)
            self.pre_off, self.pre = np.zeros(n + 1, np.uint64), np.zeros(max(self.n_pre, 1), np.uint32)
            self.lib.ptx_emu_view_read(self.handle, vp(self.status), vp(self.off), vp(self.text), vp(self.span_unit), vp(self.pre_off), vp(self.pre))
            self.status = self.status[:n]

    def close(self):
        self.lib.ptx_emu_view_close(self.handle)
        self.handle = C.c_void_p()

    def __enter__(self):
        assert self.rc == 0
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- the view's queries ----
    def _count(self, q):
        pat = np.ascontiguousarray(TC.u16(q.pattern).astype(np.uint16))
        patbuf = np.concatenate([pat, np.zeros(1, np.uint16)])
        flags = abi.FIND_ASCII_NOCASE if q.nocase is True else int(q.nocase)
        n = self.n
        (cb, f32), (ob, f64) = TS._guarded(n, np.uint32), TS._guarded(n + 1, np.uint64)
        rc = self.lib.ptx_emu_view_count(self.handle, vp(patbuf), u32(len(pat)), u32(flags), u32(q.cap), C.c_int(self.reverse), TS._inner(cb, n), TS._inner(ob, n + 1))
        if rc != 0:
            return rc, None
        assert TS._untouched(cb, f32, n) and TS._untouched(ob, f64, n + 1), "a word outside n_matches / hit_off was written"
        G = TS.GUARD
        return 0, (patbuf, len(pat), flags, cb[G : G + n].copy(), ob[G : G + n + 1].copy())

    def _hits(self, q, counted, windows=None):
        patbuf, m, flags, n_matches, hit_off = counted
        nh, G = int(hit_off[self.n]), TS.GUARD
        cols = [TS._guarded(nh, np.uint32)[0] for _ in range(6 if windows else 3)]
        ptrs = [TS._inner(c, nh) for c in cols] + [C.c_void_p(None)] * (6 - len(cols))
        before, after = windows or (0, 0)
        rc = self.lib.ptx_emu_view_hits(self.handle, vp(patbuf), u32(m), u32(flags), u32(q.cap), C.c_int(self.reverse), vp(hit_off), ptrs[0], ptrs[1], ptrs[2], u32(before), u32(after),
                                        ptrs[3], ptrs[4], ptrs[5])
        assert rc == 0
        for c in cols:
            assert TS._untouched(c, 0xA5A5A5A5, nh), "a word outside the per-hit arrays was written"
        return [c[G : G + nh].copy() for c in cols]

    def find(self, q):
        rc, counted = self._count(q)
        assert rc == 0
        hu, hs, he = self._hits(q, counted)
        return wire.Matches(status=self.status.copy(), n_matches=counted[3], hit_off=counted[4], hit_unit=hu, hit_start=hs, hit_end=he, n_pattern=counted[1])

    def _cut(self, arrays, check):
        """bounds, scan, copy and span emit: (rc, the per-slice and output arrays)."""
        off, start, end = arrays
        n, G = self.n, TS.GUARD
        ns = int(off[n]) if off is not None and n and int(off[n]) <= 0xFFFFFFFF else 0
        keep = [np.ascontiguousarray(x) if x is not None else None for x in (off, start, end)]
        if keep[1] is not None and len(keep[1]) == 0:
            keep[1] = keep[2] = np.zeros(1, np.uint32)
        (ea, f32), (eb, _), (oo, f64) = TS._guarded(ns, np.uint32), TS._guarded(ns, np.uint32), TS._guarded(2 * (ns + 1), np.uint64)
        handle = C.c_void_p()
        rc = self.lib.ptx_emu_view_bounds(self.handle, vp(keep[0]), vp(keep[1]), vp(keep[2]), C.c_int(check), C.c_int(self.reverse), TS._inner(ea, ns), TS._inner(eb, ns),
                                          TS._inner(oo, 2 * (ns + 1)), C.byref(handle))
        if rc != 0:
            return rc, None
        try:
            assert TS._untouched(ea, f32, ns) and TS._untouched(eb, f32, ns) and TS._untouched(oo, f64, 2 * (ns + 1)), "a word outside the per-slice arrays was written"
            out_off = oo[G : G + 2 * (ns + 1)].copy()
            unit_off, sspan_off = out_off[: ns + 1], out_off[ns + 1 :]
            nu, nr = int(unit_off[ns]), int(sspan_off[ns])
            (ot, f16), (os_, _), (ou, _) = TS._guarded(nu, np.uint16), TS._guarded(2 * nr, np.uint32), TS._guarded(nr, np.uint32)
            assert self.lib.ptx_emu_view_emit(handle, C.c_int(self.reverse), TS._inner(ot, nu), TS._inner(os_, 2 * nr), TS._inner(ou, nr)) == 0
            assert TS._untouched(ot, f16, nu) and TS._untouched(os_, f32, 2 * nr) and TS._untouched(ou, f32, nr), "a word outside the output was written"
        finally:
            self.lib.ptx_emu_view_cut_close(handle)
        return 0, dict(status=self.status.copy(), slice_off=np.array(off, np.uint64) if n else np.zeros(1, np.uint64), elem_start=ea[G : G + ns].copy(), elem_end=eb[G : G + ns].copy(),
                       unit_off=unit_off, text=ot[G : G + nu].copy(), sspan_off=sspan_off, sspans=os_[G : G + 2 * nr].copy().view(abi.SPAN_DTYPE), sspan_unit=ou[G : G + nr].copy())

    def slices_flat(self, arrays):
        rc, f = self._cut(arrays, 1)
        return rc, (wire.Slices(**f) if rc == 0 else None)

    def slices(self, plan):
        rc, got = self.slices_flat(SC.arrays_of(plan))
        assert rc == 0
        return got

    def snippets(self, q, before, after):
        rc, counted = self._count(q)
        assert rc == 0
        hu, hs, he, ws, we, mu = self._hits(q, counted, (before, after))
        rc, f = self._cut((counted[4], ws, we), 0)
        assert rc == 0
        return wire.Snippets(n_matches=counted[3], hit_unit=hu, hit_start=hs, hit_end=he, match_unit=mu, n_pattern=counted[1], **f)

    # ---- the twins ----
    def twin_text(self):
        if self._text is None:
            rc, self._text = TE.emu_text(self.batch, self.res, self.suite.table, self.first, self.n, self.reverse)
            assert rc == 0
        return self._text

    def twin_find(self, q):
        rc, m = TF.emu_find(self.batch, self.res, self.suite.table, self.twin_text(), self.first, self.n, q, self.reverse)
        assert rc == 0
        return m

    def twin_slices(self, plan):
        rc, m = TS.emu_slices(self.batch, self.res, self.suite.table, self.twin_text(), self.first, self.n, SC.arrays_of(plan), self.reverse)
        assert rc == 0
        return m


def opener(reverse):
    return lambda suite, first, n: EmuView(suite, first, n, reverse)


@emu
@pytest.mark.parametrize("reverse", ORDERS)
def test_cases_in_every_lane_order(reverse):
    total = starts = ends = 0
    for case in VC.cases():
        ns, a, b = VC.run_case(opener(reverse), case)
        total, starts, ends = total + ns, starts + a, ends + b
    assert total > 1000 and starts > 0 and ends > 0, "snippets were cut, some at element 0 and some at the log's end"


@emu
@pytest.mark.parametrize("reverse", ORDERS)
def test_known_answer_documents(reverse):
    suite = TC.kat_suite()
    with EmuView(suite, 0, suite.batch.n_logs, reverse) as v:  # ONE view, 46 queries
        for case in VC.kat_cases():
            got = v.snippets(case.q, 1, 1)
            ns, _, _ = VC.check_snippets(suite, v.rows, got, 0, v.n, case.q, 1, 1)
            assert ns > 0, "the document holds its own pattern"
            VC.check_same(got.matches(), v.twin_find(case.q), VC.MATCH_FIELDS)


@emu
@pytest.mark.parametrize("reverse", ORDERS)
def test_what_the_view_holds(reverse):
    """status, text_off, span_off, text and span_unit are the text passes' answer for the range; pre is the exclusive scan of the elements' lengths of every good
    log, n_visible + 1 words each, and nothing for a failed one."""
    for suite, first, n in ((TC.edge_suite(), 0, None), (TC.edge_suite(), TC.edge_docs()[0].index("n63"), 4), (TC.failed_log_suite(), 0, None), (FC.edge_suite()[0], 0, None)):
        n = suite.batch.n_logs - first if n is None else n
        with EmuView(suite, first, n, reverse) as v:
            t = v.twin_text()
            TC.check_range(suite, v.rows, t, first, n)
            assert np.array_equal(v.status, t.status) and np.array_equal(v.off[: n + 1], t.text_off) and np.array_equal(v.off[n + 1 :], t.span_off)
            assert np.array_equal(v.text[: v.n_units], t.text) and np.array_equal(v.span_unit[: v.n_spans], t.span_unit) and v.n_units == len(t.text)
            at = 0
            for k in range(n):
                assert int(v.pre_off[k]) == at
                if int(t.status[k]) == 0:
                    pre = SC.LogView(suite, v.rows, first, k).pre
                    assert [int(x) for x in v.pre[at : at + len(pre)]] == pre, (suite.name, first + k)
                    at += len(pre)
            assert int(v.pre_off[n]) == at == v.n_pre


@emu
@pytest.mark.parametrize("reverse", ORDERS)
def test_one_view_many_queries(reverse):
    suite, _ = FC.edge_suite()
    with EmuView(suite, 0, suite.batch.n_logs, reverse) as v:
        VC.view_session(v, suite, 0, v.n)


@emu
def test_the_empty_view_and_invalid_arguments():
    suite = TC.failed_log_suite()
    with EmuView(suite, 3, 0, 0) as v:  # an empty range at the end of the batch
        m = v.find(FC.Query("a"))
        assert [int(x) for x in m.hit_off] == [0] and len(m.hit_unit) == 0 and len(m.n_matches) == 0
        s = v.snippets(FC.Query("a"), 1, 1)
        assert [int(x) for x in s.slice_off] == [0] and [int(x) for x in s.unit_off] == [0] and [int(x) for x in s.sspan_off] == [0] and len(s.text) == 0 and len(s.match_unit) == 0
        c = v.slices([])
        assert [int(x) for x in c.unit_off] == [0] and [int(x) for x in c.sspan_off] == [0] and len(c.text) == 0
        assert v.n_units == v.n_pre == 0
    for first, n in ((2, 2), (4, 0)):
        assert EmuView(suite, first, n, 0).rc == abi.ERR_INVALID_ARG, "a range outside the batch"
    with EmuView(suite, 0, 3, 0) as v:
        for q in (FC.Query(""), FC.Query("a" * (abi.FIND_PATTERN_MAX + 1)), FC.Query("a", nocase=2), FC.Query("a", nocase=0x80000000)):
            assert v._count(q)[0] == abi.ERR_INVALID_ARG, q
        off, start, end = SC.arrays_of([[(0, 1)], [], [(1, 2), (0, 9)]])
        bad = [(np.array([1, 1, 1, 3], np.uint64), start, end), (np.array([0, 2, 1, 3], np.uint64), start, end), (off, None, end), (off, start, None), (None, start, end),
               (np.array([0, 0, 0, 1 << 32], np.uint64), start, end)]
        for arrays in bad:
            assert v.slices_flat(arrays)[0] == abi.ERR_INVALID_ARG
        rc, none = v.slices_flat((np.zeros(4, np.uint64), None, None))
        assert rc == 0 and [int(x) for x in none.unit_off] == [0] and len(none.text) == 0, "zero slices: NULL slice arrays are legal"
        lib, pat, out = v.lib, np.array([0x61, 0], np.uint16), np.zeros(8, np.uint64)
        assert lib.ptx_emu_view_count(None, vp(pat), u32(1), u32(0), u32(1), C.c_int(0), vp(out), vp(out)) == abi.ERR_INVALID_ARG, "the NULL view"
        h = C.c_void_p()
        assert lib.ptx_emu_view_bounds(None, vp(out), None, None, C.c_int(1), C.c_int(0), vp(out), vp(out), vp(out), C.byref(h)) == abi.ERR_INVALID_ARG


@emu
@pytest.mark.parametrize("reverse", ORDERS)
def test_value_id_beyond_the_table(reverse):
    """One log with a value id equal to n_strings: PTX_ERR_BAD_OP as the twins say, no words of the prefix, no hits; its neighbours are bit-equal to the run
    without it."""
    suite = TC.edge_suite()
    log = [k for k, w in enumerate(suite.want) if len(w.units) == TC.T + 1][0]
    bad, _ = TC.bad_id_batch(suite, log)
    n, q = suite.batch.n_logs, FC.Query("e")
    with EmuView(suite, 0, n, reverse) as g, EmuView(suite, 0, n, reverse, batch=bad) as v:
        good, m = g.snippets(q, 2, 2), v.snippets(q, 2, 2)
        assert int(good.n_matches[log]) > 0
        assert int(m.status[log]) == abi.ERR_BAD_OP and int(m.n_matches[log]) == 0 and int(m.slice_off[log + 1]) == int(m.slice_off[log])
        assert int(v.pre_off[log + 1]) == int(v.pre_off[log]) and np.array_equal(m.status, v.twin_find(q).status)
        VC.check_snippets(suite, g.rows, m, 0, n, q, 2, 2, status_of={log: abi.ERR_BAD_OP}, decode=False)
        for k in range(n):
            if k != log:
                assert good.of_log(k) == m.of_log(k) and int(m.n_matches[k]) == int(good.n_matches[k])
                assert [good.rows_of_slice(good.index(k, j)) for j in range(len(good.of_log(k)))] == [m.rows_of_slice(m.index(k, j)) for j in range(len(m.of_log(k)))]


@emu
def test_sanitizer_program(tmp_path):
    """tests/emu/emu_view_main.cc: every pass over tables and logs built in the file, against a sequential search and cut inside the file, compiled with
    -fsanitize=address,undefined and run as a child process (every buffer exactly as large as the library makes it: `pre` ends at pre[n_visible] of the last
    good log)."""
    exe = str(tmp_path / "emu_view_main")
    src = os.path.join(H.ROOT, "tests", "emu", "emu_view_main.cc")
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "view emulation ok" in r.stdout
