"""Find in the documents' text (peritext_amd/csrc/find_core.h: count, scan, emit over the text text_core.h assembles) on the CPU emulation, in every lane
order.  The cases and their expected values are tests/find_cases.py's (a plain loop over the oracle's text, element boundaries from the merge's value ids);
tests/test_gpu_find.py repeats them through the C ABI.  The text the search reads is the text emulation's own output for the same range (tests/test_emu_text.py
checks that one), the merge results are the emulation's merge of the same batch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import find_cases as FC
import helpers as H
import test_emu_text as TE
import text_cases as TC
from peritext_amd import abi, wire

EMU_FIND_LIB = os.path.join(H.ROOT, "tests", "emu", "libperitext_emu_find.so")
needs_emu = [pytest.mark.skipif(not os.path.exists(EMU_FIND_LIB) or not os.path.exists(TE.EMU_TEXT_LIB), reason="tests/emu/libperitext_emu_find.so not built (run __graft_entry__.build())"),
             pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")]
GUARD = 64  # words of 0xA5A5A5A5 before and behind every output array


def emu(fn):
    for m in needs_emu:
        fn = m(fn)
    return fn


def test_the_entry_points_are_declared():
    """The symbols and the struct stand in the C header and in the ctypes prototypes, the two constants are mirrored, and the ABI version is still 7 (no skip:
    this one needs no library)."""
    with open(os.path.join(H.ROOT, "include", "peritext_hip.h")) as f:
        header = f.read()
    for name, nargs in (("ptx_result_find_text", 11), ("ptx_matches_free", 1)):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in abi.FUNCTIONS and len(abi.FUNCTIONS[name][1]) == nargs, name
    assert re.search(r"typedef\s+struct\s+ptx_matches\s*\{", header)
    assert re.search(r"#define\s+PTX_ABI_VERSION\s+7u", header), "the addition is purely additive"
    assert C.sizeof(abi.ptx_matches) == 16 + 7 * 8
    assert int(re.search(r"#define\s+PTX_FIND_PATTERN_MAX\s+(\d+)u", header).group(1)) == abi.FIND_PATTERN_MAX
    assert int(re.search(r"#define\s+PTX_FIND_ASCII_NOCASE\s+(\d+)u", header).group(1)) == abi.FIND_ASCII_NOCASE
    with open(os.path.join(H.ROOT, "peritext_amd", "csrc", "find_core.h")) as f:
        core = f.read()
    per_lane = int(re.search(r"#define\s+PTX_FIND_PER_LANE\s+(\d+)u", core).group(1))
    assert re.search(r"#define\s+PTX_FIND_STEP\s+\(64u \* PTX_FIND_PER_LANE\)", core) and abi.FIND_STEP == 64 * per_lane
    with open(os.path.join(H.ROOT, "__graft_entry__.py")) as f:
        guard = re.search(r"NO_SPILL_KERNELS = \((.*?)\)", f.read(), re.S).group(1)
    assert '"ptx_find_count_kernel"' in guard and '"ptx_find_emit_kernel"' in guard, "the build's no-spill guard names the new kernels"


_TEXT = {}


def assembled(suite, res, first, n, reverse):
    """The text passes' output for a range (status, off rows, text) — once per (suite, range, lane order)."""
    k = (suite.name, first, n, reverse)
    if k not in _TEXT:
        rc, text = TE.emu_text(suite.batch, res, suite.table, first, n, reverse)
        assert rc == 0
        _TEXT[k] = text
    return _TEXT[k]


def emu_find(batch, res, table, text, first, n, q, reverse=0):
    """ptx_result_find_text's count, scan and emit passes over host arrays: (return code, wire.Matches).  Every output is pre-filled with 0xA5 and guarded."""
    lib = C.CDLL(EMU_FIND_LIB)
    lib.ptx_emu_find_count.restype = lib.ptx_emu_find_emit.restype = C.c_int
    assert lib.ptx_emu_find_step() == abi.FIND_STEP and lib.ptx_emu_find_pattern_max() == abi.FIND_PATTERN_MAX
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    u32 = C.c_uint32
    pat = np.ascontiguousarray(TC.u16(q.pattern).astype(np.uint16))
    patbuf = np.concatenate([pat, np.zeros(1, np.uint16)])  # (never an empty array: its pointer must exist for n_pattern == 0 too)
    status = np.ascontiguousarray(np.concatenate([text.status, np.zeros(1, np.uint32)])[: max(n, 1)].astype(np.uint32))
    off = np.ascontiguousarray(np.concatenate([text.text_off, text.span_off]).astype(np.uint64))
    units = np.ascontiguousarray(text.text.astype(np.uint16)) if len(text.text) else np.zeros(1, np.uint16)
    if len(text.text):
        units = units[: len(text.text)].copy()  # exactly the text: the last log's halo must end with it
    cbuf = np.full(2 * GUARD + n, 0xA5A5A5A5, np.uint32)
    obuf = np.full(2 * GUARD + n + 1, 0xA5A5A5A5A5A5A5A5, np.uint64)
    flags = abi.FIND_ASCII_NOCASE if q.nocase is True else int(q.nocase)
    rc = lib.ptx_emu_find_count(vp(status), vp(off), vp(units), u32(n), vp(patbuf), u32(len(pat)), u32(flags), u32(q.cap), C.c_int(reverse),
                                C.c_void_p(cbuf.ctypes.data + 4 * GUARD), C.c_void_p(obuf.ctypes.data + 8 * GUARD))
    if rc != 0:
        return rc, None
    assert (cbuf[:GUARD] == 0xA5A5A5A5).all() and (cbuf[GUARD + n :] == 0xA5A5A5A5).all() and (obuf[:GUARD] == obuf[0]).all() and (obuf[GUARD + n + 1 :] == obuf[0]).all()
    n_matches, hit_off = cbuf[GUARD : GUARD + n].copy(), obuf[GUARD : GUARD + n + 1].copy()
    nh = int(hit_off[n])
    hb = [np.full(2 * GUARD + nh, 0xA5A5A5A5, np.uint32) for _ in range(3)]
    soff = TC.table_arrays(table)[1]
    rc = lib.ptx_emu_find_emit(vp(batch.log_off), vp(res.logs), vp(res.values), vp(soff), u32(len(table)), u32(first), u32(n), vp(status), vp(off), vp(units), vp(patbuf), u32(len(pat)),
                               u32(flags), u32(q.cap), C.c_int(reverse), vp(hit_off), *[C.c_void_p(b.ctypes.data + 4 * GUARD) for b in hb])
    assert rc == 0
    for b in hb:
        assert (b[:GUARD] == 0xA5A5A5A5).all() and (b[GUARD + nh :] == 0xA5A5A5A5).all(), "a word outside the hit arrays was written"
    cols = [b[GUARD : GUARD + nh].copy() for b in hb]
    return 0, wire.Matches(status=text.status.copy(), n_matches=n_matches, hit_off=hit_off, hit_unit=cols[0], hit_start=cols[1], hit_end=cols[2], n_pattern=len(pat))


def run_queries(suite, queries, reverse):
    res = TE.merged(suite, reverse)
    got = {}
    for q in queries:
        first, n = q.rng or (0, suite.batch.n_logs)
        text = assembled(suite, res, first, n, reverse)
        rc, m = emu_find(suite.batch, res, suite.table, text, first, n, q, reverse)
        assert rc == 0
        FC.check_range(suite, TE.compact(suite.batch, res, first, n), m, first, n, q)
        if q.rng is None and q.cap == FC.ALL:
            got[(q.pattern, q.nocase)] = m
    return got


@emu
@pytest.mark.parametrize("reverse", [0, 1, 2])
def test_edges_in_every_lane_order(reverse):
    suite, names = FC.edge_suite()
    got = run_queries(suite, FC.edge_queries(), reverse)
    FC.edge_hand_checks(suite, names, got)


@emu
@pytest.mark.parametrize("reverse", [0, 1, 2])
@pytest.mark.parametrize("name", ["text_edges", "failed_log", "kat"])
def test_suites_of_the_text_cases(name, reverse):
    suite, queries = {"text_edges": (TC.edge_suite(), FC.text_edge_queries()), "failed_log": (TC.failed_log_suite(), FC.failed_log_queries()), "kat": (TC.kat_suite(), FC.kat_queries())}[name]
    run_queries(suite, queries, reverse)


@emu
def test_invalid_arguments_and_the_empty_range():
    suite = TC.failed_log_suite()
    res = TE.merged(suite, 0)
    text = assembled(suite, res, 0, 3, 0)
    for q in (FC.Query(""), FC.Query("a" * (abi.FIND_PATTERN_MAX + 1)), FC.Query("a", nocase=2), FC.Query("a", nocase=0x80000000)):
        assert emu_find(suite.batch, res, suite.table, text, 0, 3, q)[0] == abi.ERR_INVALID_ARG, q
    assert TE.emu_text(suite.batch, res, suite.table, 2, 2)[0] == abi.ERR_INVALID_ARG, "a range outside the batch ends in the text passes"
    empty = assembled(suite, res, 3, 0, 0)
    rc, m = emu_find(suite.batch, res, suite.table, empty, 3, 0, FC.Query("a"))
    assert rc == 0 and [int(x) for x in m.hit_off] == [0] and len(m.hit_unit) == 0 and len(m.n_matches) == 0


@emu
@pytest.mark.parametrize("reverse", [0, 1, 2])
def test_value_id_beyond_the_table(reverse):
    """One log with a value id equal to n_strings: PTX_ERR_BAD_OP, zero matches; its neighbours are bit-equal to the run without it."""
    suite = TC.edge_suite()
    log = [k for k, w in enumerate(suite.want) if len(w.units) == TC.T + 1][0]
    bad, _ = TC.bad_id_batch(suite, log)
    n = suite.batch.n_logs
    q = FC.Query("e")
    good_res = TE.merged(suite, reverse)
    _, good = emu_find(suite.batch, good_res, suite.table, assembled(suite, good_res, 0, n, reverse), 0, n, q, reverse)
    assert int(good.n_matches[log]) > 0
    res = TE.merged(suite, reverse, batch=bad)
    rc, text = TE.emu_text(bad, res, suite.table, 0, n, reverse)
    assert rc == 0
    rc, m = emu_find(bad, res, suite.table, text, 0, n, q, reverse)
    assert rc == 0 and int(m.status[log]) == abi.ERR_BAD_OP and int(m.n_matches[log]) == 0 and int(m.hit_off[log + 1]) == int(m.hit_off[log])
    for k in range(n):
        if k != log:
            assert int(m.status[k]) == int(good.status[k]) and int(m.n_matches[k]) == int(good.n_matches[k])
            a, b, c, d = int(m.hit_off[k]), int(m.hit_off[k + 1]), int(good.hit_off[k]), int(good.hit_off[k + 1])
            for col in ("hit_unit", "hit_start", "hit_end"):
                assert getattr(m, col)[a:b].tobytes() == getattr(good, col)[c:d].tobytes(), (k, col)


@emu
def test_sanitizer_program(tmp_path):
    """tests/emu/emu_find_main.cc: all passes over tables and logs built in the file, against a sequential search inside the file, compiled with
    -fsanitize=address,undefined and run as a child process (every buffer exactly as large as the host library makes it)."""
    exe = str(tmp_path / "emu_find_main")
    src = os.path.join(H.ROOT, "tests", "emu", "emu_find_main.cc")
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "find emulation ok" in r.stdout
