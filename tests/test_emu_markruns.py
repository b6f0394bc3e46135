"""Queries by format on a resident text view (peritext_amd/csrc/markrun_core.h: count, scan, emit and finish of the runs of a mark; the slice passes over the runs'
windows; the filter of a find's hits by the runs) on the CPU emulation, in every lane order.  The cases and their expected values are tests/markrun_cases.py's;
tests/test_gpu_markruns.py repeats them through the C ABI.  Every output is pre-filled with 0xA5 and guarded on both sides, as tests/test_emu_view.py does; the
view is that file's, made by the same emulation library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import find_cases as FC
import helpers as H
import markrun_cases as MC
import test_emu_slices as TS
import test_emu_view as TV
import text_cases as TC
from peritext_amd import abi, wire

EMU_LIB = os.path.join(H.ROOT, "tests", "emu", "libperitext_emu_markruns.so")
needs_emu = [pytest.mark.skipif(not all(os.path.exists(p) for p in (EMU_LIB, TV.EMU_VIEW_LIB)), reason="tests/emu/libperitext_emu_markruns.so not built (run __graft_entry__.build())"),
             pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")]
ORDERS = [0, 1, 2]
vp, u32 = TV.vp, TV.u32


def emu(fn):
    for m in needs_emu:
        fn = m(fn)
    return fn


def test_the_entry_points_are_declared():
    """The symbols and structs stand in the C header and in the ctypes prototypes, the ABI version is still 7, the build's no-spill guard names the new kernels and
    the build makes the emulation library (no skip: this one needs no library)."""
    with open(os.path.join(H.ROOT, "include", "peritext_hip.h")) as f:
        header = f.read()
    for name, nargs in (("ptx_view_mark_runs", 6), ("ptx_mark_runs_free", 1), ("ptx_view_mark_snippets", 8), ("ptx_mark_snippets_free", 1), ("ptx_view_find_in_marks", 9)):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in abi.FUNCTIONS and len(abi.FUNCTIONS[name][1]) == nargs, name
    assert re.search(r"typedef\s+struct\s+ptx_mark_runs\s*\{", header) and re.search(r"typedef\s+struct\s+ptx_mark_snippets\s*\{", header)
    assert re.search(r"#define\s+PTX_MARK_ANY_ID\s+0xFFFFFFFFu", header) and abi.MARK_ANY_ID == 0xFFFFFFFF
    assert re.search(r"#define\s+PTX_ABI_VERSION\s+7u", header), "the addition is purely additive"
    assert C.sizeof(abi.ptx_mark_runs) == 16 + 9 * 8 and C.sizeof(abi.ptx_mark_snippets) == 16 + 17 * 8
    with open(os.path.join(H.ROOT, "__graft_entry__.py")) as f:
        entry = f.read()
    guard = re.search(r"NO_SPILL_KERNELS = \((.*?)\)", entry, re.S).group(1)
    for k in ("ptx_markrun_count_kernel", "ptx_markrun_emit_kernel", "ptx_markrun_finish_kernel", "ptx_markrun_filter_count_kernel", "ptx_markrun_filter_emit_kernel"):
        assert '"%s"' % k in guard, "the build's no-spill guard names " + k
    assert "libperitext_emu_markruns.so" in entry
    assert hasattr(wire, "MarkRuns") and hasattr(wire, "MarkSnippets")


def _lib():
    lib = C.CDLL(EMU_LIB)
    for f in ("ptx_emu_markrun_count", "ptx_emu_markrun_emit", "ptx_emu_markrun_filter_count", "ptx_emu_markrun_filter_emit"):
        getattr(lib, f).restype = C.c_int
    assert lib.ptx_emu_markrun_step() == abi.MARKRUN_STEP
    return lib


class EmuMarkView(TV.EmuView):
    """tests/test_emu_view.py's view and, over it, the interface tests/markrun_cases.py names.  The comment intervals and the per-log rows are the merge's own
    (capacity layout), as the library reads them through the view's result."""

    def __init__(self, suite, first, n, reverse):
        super().__init__(suite, first, n, reverse)
        self.mlib = _lib()

    def _run_count(self, mark_type, ident, cap, find=0):
        n, G = self.n, TS.GUARD
        (cb, f32), (ob, f64) = TS._guarded(n, np.uint32), TS._guarded(n + 1, np.uint64)
        rc = self.mlib.ptx_emu_markrun_count(self.handle, vp(self.res.cintervals), vp(self.res.logs), u32(mark_type), u32(ident), u32(cap), C.c_int(find), C.c_int(self.reverse),
                                             TS._inner(cb, n), TS._inner(ob, n + 1))
        if rc != 0:
            return rc, None, None
        assert TS._untouched(cb, f32, n) and TS._untouched(ob, f64, n + 1), "a word outside n_runs / run_off was written"
        return 0, cb[G : G + n].copy(), ob[G : G + n + 1].copy()

    def _run_emit(self, mark_type, ident, cap, run_off, finish=True, windows=None):
        nr, G = int(run_off[self.n]), TS.GUARD
        cols = [TS._guarded(nr, np.uint32)[0] for _ in range(3 + (2 if finish else 0) + (3 if windows else 0))]
        ptrs = [TS._inner(c, nr) for c in cols]
        null = C.c_void_p(None)
        ptrs = ptrs[:3] + (ptrs[3:5] if finish else [null, null]) + (ptrs[-3:] if windows else [null, null, null])
        before, after = windows or (0, 0)
        rc = self.mlib.ptx_emu_markrun_emit(self.handle, vp(self.res.cintervals), vp(self.res.logs), u32(mark_type), u32(ident), u32(cap), C.c_int(self.reverse), vp(run_off),
                                            ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], u32(before), u32(after), ptrs[5], ptrs[6], ptrs[7])
        assert rc == 0
        for c in cols:
            assert TS._untouched(c, 0xA5A5A5A5, nr), "a word outside the per-run arrays was written"
        return [c[G : G + nr].copy() for c in cols]

    def mark_runs(self, mark_type, ident, cap):
        rc, n_runs, run_off = self._run_count(mark_type, ident, cap)
        assert rc == 0
        rs, re_, ri, ru, rl = self._run_emit(mark_type, ident, cap, run_off)
        return wire.MarkRuns(status=self.status.copy(), n_runs=n_runs, run_off=run_off, run_start=rs, run_end=re_, run_id=ri, run_unit=ru, run_len=rl, mark_type=mark_type)

    def mark_snippets(self, mark_type, ident, cap, before, after):
        rc, n_runs, run_off = self._run_count(mark_type, ident, cap)
        assert rc == 0
        rs, re_, ri, ru, rl, ws, we, mu = self._run_emit(mark_type, ident, cap, run_off, windows=(before, after))
        rc, f = self._cut((run_off, ws, we), 0)
        assert rc == 0
        return wire.MarkSnippets(n_runs=n_runs, run_start=rs, run_end=re_, run_id=ri, run_unit=ru, run_len=rl, match_unit=mu, mark_type=mark_type, **f)

    def find_in_marks(self, q, mark_type, ident):
        rc, _, run_off = self._run_count(mark_type, ident, MC.ALL, find=1)
        assert rc == 0
        rs, re_, _ = self._run_emit(mark_type, ident, MC.ALL, run_off, finish=False)  # as the library: the uncapped runs stay in scratch, nobody measures them
        every = self.find(FC.Query(q.pattern, nocase=q.nocase, cap=MC.ALL))
        n, G = self.n, TS.GUARD
        (kb, f32), (ob, f64) = TS._guarded(n, np.uint32), TS._guarded(n + 1, np.uint64)
        pad = lambda a: a if len(a) else np.zeros(1, a.dtype)  # noqa: E731
        hu, hs, he, rs, re_ = (pad(a) for a in (every.hit_unit, every.hit_start, every.hit_end, rs, re_))
        assert self.mlib.ptx_emu_markrun_filter_count(u32(n), u32(q.cap), vp(every.hit_off), vp(hs), vp(he), vp(run_off), vp(rs), vp(re_), C.c_int(self.reverse), TS._inner(kb, n),
                                                      TS._inner(ob, n + 1)) == 0
        assert TS._untouched(kb, f32, n) and TS._untouched(ob, f64, n + 1), "a word outside n_matches / hit_off was written"
        out_off = ob[G : G + n + 1].copy()
        nk = int(out_off[n])
        cols = [TS._guarded(nk, np.uint32)[0] for _ in range(3)]
        assert self.mlib.ptx_emu_markrun_filter_emit(u32(n), u32(q.cap), vp(every.hit_off), vp(hu), vp(hs), vp(he), vp(run_off), vp(rs), vp(re_), C.c_int(self.reverse), vp(out_off),
                                                     *[TS._inner(c, nk) for c in cols]) == 0
        for c in cols:
            assert TS._untouched(c, 0xA5A5A5A5, nk), "a word outside the kept hits was written"
        return wire.Matches(status=self.status.copy(), n_matches=kb[G : G + n].copy(), hit_off=out_off, hit_unit=cols[0][G : G + nk].copy(), hit_start=cols[1][G : G + nk].copy(),
                            hit_end=cols[2][G : G + nk].copy(), n_pattern=every.n_pattern)


class _Views:
    """The views of one (suite, range) are made once per lane order and queried by all its cases."""

    def __init__(self, reverse):
        self.reverse, self.open = reverse, {}

    def __call__(self, suite, first, n):
        key = (suite.name, first, n)
        if key not in self.open:
            v = EmuMarkView(suite, first, n, self.reverse)
            assert v.rc == 0
            self.open[key] = v
        views = self

        class Shared:
            def __enter__(self):
                return views.open[key]

            def __exit__(self, *exc):
                pass

        return Shared()

    def close(self):
        for v in self.open.values():
            v.close()


@pytest.fixture(scope="module", params=ORDERS)
def views(request):
    v = _Views(request.param)
    yield v
    v.close()


@emu
def test_run_cases_in_every_lane_order(views):
    runs = snips = 0
    for case in MC.run_cases():
        r, s = MC.run_run_case(views, case)
        runs, snips = runs + r, snips + s
    assert runs > 1000 and snips == runs, "runs were listed, one snippet each"


@emu
def test_find_in_marks_in_every_lane_order(views):
    kept = dropped = 0
    for case in MC.find_cases():
        k, d = MC.run_find_case(views, case)
        kept, dropped = kept + k, dropped + d
    assert kept > 300 and dropped > 300, "hits were kept and hits were dropped"


@emu
def test_known_answer_documents(views):
    runs = 0
    for case in MC.kat_run_cases():
        runs += MC.run_run_case(views, case)[0]
    assert runs > 50, "the documents hold marks of every kind"
    kept = sum(MC.run_find_case(views, case)[0] for case in MC.kat_find_cases())
    assert kept > 0


@emu
def test_any_comment_order_is_the_results(views):
    """PTX_MARK_ANY_ID on comments: the runs ARE the log's cinterval rows, in the result's own order (id, start), which is not ascending start across ids."""
    suite, N = MC.edge_suite()
    k = N["comments"]
    with views(suite, k, 1) as v:
        got = v.mark_runs(MC.COMMENT, MC.ANY, MC.ALL)
        c = v.rows.cintervals[int(v.rows.cint_off[0]) : int(v.rows.cint_off[1])]
        assert [(s, e, i) for s, e, i, _, _ in got.of_log(0)] == [(int(x["start"]), int(x["end"]), int(x["id"])) for x in c] and len(c) == 3
        starts = [s for s, *_ in got.of_log(0)]
        assert starts != sorted(starts) and [i for _, _, i, _, _ in got.of_log(0)] == sorted(i for _, _, i, _, _ in got.of_log(0))


@emu
def test_the_empty_view_and_invalid_arguments():
    suite = TC.failed_log_suite()
    with EmuMarkView(suite, 3, 0, 0) as v:  # an empty range at the end of the batch
        r = v.mark_runs(MC.STRONG, MC.ANY, MC.ALL)
        assert [int(x) for x in r.run_off] == [0] and len(r.run_start) == 0 and len(r.n_runs) == 0
        s = v.mark_snippets(MC.COMMENT, MC.ANY, MC.ALL, 1, 1)
        assert [int(x) for x in s.slice_off] == [0] and [int(x) for x in s.unit_off] == [0] and [int(x) for x in s.sspan_off] == [0] and len(s.text) == 0 and len(s.match_unit) == 0
        m = v.find_in_marks(FC.Query("a"), MC.LINK, MC.ANY)
        assert [int(x) for x in m.hit_off] == [0] and len(m.hit_unit) == 0 and len(m.n_matches) == 0
    with EmuMarkView(suite, 0, 3, 0) as v:
        for mark_type, ident, find_only in MC.invalid_selectors():
            assert v._run_count(mark_type, ident, MC.ALL, find=1)[0] == abi.ERR_INVALID_ARG, (mark_type, ident)
            assert (v._run_count(mark_type, ident, MC.ALL, find=0)[0] == abi.ERR_INVALID_ARG) == (not find_only), (mark_type, ident)
        out = np.zeros(8, np.uint64)
        assert v.mlib.ptx_emu_markrun_count(None, None, None, u32(0), u32(MC.ANY), u32(1), C.c_int(0), C.c_int(0), vp(out), vp(out)) == abi.ERR_INVALID_ARG, "the NULL view"
        assert v._run_count(MC.LINK, abi.ATTR_ID_MASK, MC.ALL)[0] == 0, "the largest url id is a legal selector"


@emu
def test_sanitizer_program(tmp_path):
    """tests/emu/emu_markruns_main.cc: every pass over span rows, comment intervals and prefixes built in the file, against a sequential walk inside the file,
    compiled with -fsanitize=address,undefined and run as a child process (the run and cinterval arrays end exactly at their last row)."""
    exe = str(tmp_path / "emu_markruns_main")
    src = os.path.join(H.ROOT, "tests", "emu", "emu_markruns_main.cc")
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "markrun emulation ok" in r.stdout
