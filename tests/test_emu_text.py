"""Document text assembled on the device (peritext_amd/csrc/text_core.h: lengths, then one UTF-16 buffer per range with per-span code-unit offsets) on the CPU
emulation, in every lane order.  The cases and their expected values are tests/text_cases.py's (the oracle's spans, the reference's known answers, one
hand-written literal); tests/test_gpu_text.py repeats them through the C ABI.  The merge results the text passes read are the emulation's own merge of the same
batch, in the capacity layout the kernels write on the device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
import text_cases as TC
from peritext_amd import abi, wire

EMU_TEXT_LIB = os.path.join(H.ROOT, "tests", "emu", "libperitext_emu_text.so")
needs_emu = [pytest.mark.skipif(not os.path.exists(EMU_TEXT_LIB), reason="tests/emu/libperitext_emu_text.so not built (run __graft_entry__.build())"),
             pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")]
GUARD = 64  # units of 0xA5A5 before and behind the text buffer (an even count: the first unit of the text stays dword-aligned)


def emu(fn):
    for m in needs_emu:
        fn = m(fn)
    return fn


def test_the_entry_points_are_declared():
    """The symbols stand in the C header and in the ctypes prototypes, the tile and the threshold are mirrored, and the ABI version is still 7 (no skip: this
    one needs no library)."""
    with open(os.path.join(H.ROOT, "include", "peritext_hip.h")) as f:
        header = f.read()
    for name, nargs in (("ptx_strings_upload", 5), ("ptx_strings_free", 2), ("ptx_result_text_range", 7), ("ptx_text_free", 1)):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in abi.FUNCTIONS and len(abi.FUNCTIONS[name][1]) == nargs, name
    assert re.search(r"typedef\s+struct\s+ptx_text\s*\{", header) and re.search(r"typedef\s+struct\s+ptx_dstrings\s+ptx_dstrings\s*;", header)
    assert re.search(r"#define\s+PTX_ABI_VERSION\s+7u", header), "the addition is purely additive"
    assert C.sizeof(abi.ptx_text) == 16 + 6 * 8
    with open(os.path.join(H.ROOT, "peritext_amd", "csrc", "text_core.h")) as f:
        core = f.read()
    per_lane = int(re.search(r"#define\s+PTX_TEXT_PER_LANE\s+(\d+)u", core).group(1))
    assert re.search(r"#define\s+PTX_TEXT_TILE\s+\(64u \* PTX_TEXT_PER_LANE\)", core) and abi.TEXT_TILE == 64 * per_lane
    assert int(re.search(r"#define\s+PTX_TEXT_LANE_MAX\s+(\d+)u", core).group(1)) == abi.TEXT_LANE_MAX


def compact(batch, res, first, n):
    """The rows of the logs [first, first + n) of a capacity-layout result as ptx_result_download_range returns them (status, counts, compact spans and
    comment intervals; a failed log has none)."""
    logs = res.logs[first : first + n].copy()
    ok = logs["status"] == 0
    counts = [np.where(ok, logs[k], 0).astype(np.uint64) for k in ("n_visible", "n_spans", "n_cintervals")]
    offs = [np.concatenate([[0], np.cumsum(c)]).astype(np.uint64) for c in counts]
    rows = lambda a, c: np.concatenate([a[int(batch.log_off[first + k]) : int(batch.log_off[first + k]) + int(c[k])] for k in range(n)] + [a[:0]])  # noqa: E731
    return wire.Results(logs=logs, values=rows(res.values, counts[0]), spans=rows(res.spans, counts[1]), cintervals=rows(res.cintervals, counts[2]),
                        elem_rank=np.zeros(0, np.uint32), value_off=offs[0], span_off=offs[1], cint_off=offs[2])


def emu_text(batch, res, table, first, n, reverse=0):
    """ptx_result_text_range over a wire.Batch and a capacity-layout wire.Results through the host emulation: (return code, wire.Text)."""
    lib = C.CDLL(EMU_TEXT_LIB)
    lib.ptx_emu_text_lengths.restype = lib.ptx_emu_text_assemble.restype = C.c_int
    assert lib.ptx_emu_text_tile() == abi.TEXT_TILE and lib.ptx_emu_text_lane_max() == abi.TEXT_LANE_MAX
    units, soff = TC.table_arrays(table)
    units = np.concatenate([units, np.zeros(1, np.uint16)])[: max(len(units), 1)]  # (at least one unit, as the library allocates)
    status = np.full(max(n, 1), 0xA5A5A5A5, np.uint32)
    off = np.full(2 * (n + 1), 0xA5A5A5A5A5A5A5A5, np.uint64)
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    u32 = C.c_uint32
    rc = lib.ptx_emu_text_lengths(vp(batch.log_off), u32(batch.n_logs), vp(res.logs), vp(res.values), vp(res.spans), vp(units), vp(soff), u32(len(table)), u32(first), u32(n),
                                  C.c_int(reverse), vp(status), vp(off))
    if rc != 0:
        return rc, None
    text_off, span_off = off[: n + 1].copy(), off[n + 1 :].copy()
    buf = np.full(2 * GUARD + int(text_off[n]), 0xA5A5, np.uint16)
    assert (buf.ctypes.data + 2 * GUARD) % 4 == 0
    text = buf[GUARD : GUARD + int(text_off[n])]
    sbuf = np.full(2 * GUARD + int(span_off[n]), 0xA5A5A5A5, np.uint32)
    span_unit = sbuf[GUARD : GUARD + int(span_off[n])]
    rc = lib.ptx_emu_text_assemble(vp(batch.log_off), vp(res.logs), vp(res.values), vp(res.spans), vp(units), vp(soff), u32(len(table)), u32(first), u32(n), C.c_int(reverse),
                                   vp(status), vp(off), C.c_void_p(buf.ctypes.data + 2 * GUARD), C.c_void_p(sbuf.ctypes.data + 4 * GUARD))
    assert rc == 0
    # nothing outside [text_off[0], text_off[n]) is written (inside, every unit belongs to exactly one log and is compared by the caller)
    assert (buf[:GUARD] == 0xA5A5).all() and (buf[GUARD + int(text_off[n]) :] == 0xA5A5).all(), "a unit outside the text was written"
    assert (sbuf[:GUARD] == 0xA5A5A5A5).all() and (sbuf[GUARD + int(span_off[n]) :] == 0xA5A5A5A5).all()
    return 0, wire.Text(status=status[:n], text_off=text_off, text=text.copy(), span_off=span_off, span_unit=span_unit.copy())


_MERGED = {}


def merged(suite, reverse, batch=None):
    """The emulation's merge of the suite's batch (WITH admission: the failed log is a sequence gap), once per lane order."""
    key = (suite.name, reverse)
    if batch is not None:
        return H.emu_merge(batch, reverse=reverse, admission=True)
    if key not in _MERGED:
        _MERGED[key] = H.emu_merge(suite.batch, reverse=reverse, admission=True)
    return _MERGED[key]


@emu
@pytest.mark.parametrize("reverse", [0, 1, 2])
@pytest.mark.parametrize("name", ["edges", "big_table", "failed_log", "kat"])
def test_cases_in_every_lane_order(name, reverse):
    suite = {s.name: s for s in TC.suites()}[name]
    res = merged(suite, reverse)
    for first, n in [(0, suite.batch.n_logs)] + suite.ranges:
        rc, text = emu_text(suite.batch, res, suite.table, first, n, reverse)
        assert rc == 0
        TC.check_range(suite, compact(suite.batch, res, first, n), text, first, n)


@emu
def test_range_outside_the_batch():
    suite = TC.failed_log_suite()
    res = merged(suite, 0)
    assert emu_text(suite.batch, res, suite.table, 2, 2)[0] == abi.ERR_INVALID_ARG
    assert emu_text(suite.batch, res, suite.table, 4, 0)[0] == abi.ERR_INVALID_ARG
    rc, text = emu_text(suite.batch, res, suite.table, 3, 0)
    assert rc == 0 and len(text.text) == 0 and [int(x) for x in text.text_off] == [0] and [int(x) for x in text.span_off] == [0]


@emu
@pytest.mark.parametrize("reverse", [0, 1, 2])
def test_value_id_beyond_the_table(reverse):
    """One log with a value id equal to n_strings reports PTX_ERR_BAD_OP and has no text; its neighbours are bit-equal to the run without it."""
    suite = TC.edge_suite()
    log = [k for k, w in enumerate(suite.want) if len(w.units) == TC.T + 1][0]
    bad, _ = TC.bad_id_batch(suite, log)
    n = suite.batch.n_logs
    _, good_text = emu_text(suite.batch, merged(suite, reverse), suite.table, 0, n, reverse)
    res = merged(suite, reverse, batch=bad)
    rc, text = emu_text(bad, res, suite.table, 0, n, reverse)
    assert rc == 0 and int(text.status[log]) == abi.ERR_BAD_OP and int(res.logs["status"][log]) == 0
    assert int(text.text_off[log + 1]) == int(text.text_off[log]), "no text"
    assert np.array_equal(text.span_off, good_text.span_off) and not text.span_unit[int(text.span_off[log]) : int(text.span_off[log + 1])].any()
    for k in range(n):
        if k != log:
            assert int(text.status[k]) == int(good_text.status[k])
            a = text.text[int(text.text_off[k]) : int(text.text_off[k + 1])]
            b = good_text.text[int(good_text.text_off[k]) : int(good_text.text_off[k + 1])]
            assert a.tobytes() == b.tobytes(), k
            sa = text.span_unit[int(text.span_off[k]) : int(text.span_off[k + 1])]
            assert sa.tobytes() == good_text.span_unit[int(good_text.span_off[k]) : int(good_text.span_off[k + 1])].tobytes(), k
    with pytest.raises(ValueError):
        wire.decode_spans_text(suite.batch, compact(bad, res, 0, n), text, log)


@emu
def test_sanitizer_program(tmp_path):
    """tests/emu/emu_text_main.cc: both passes over tables and logs built in the file, against a sequential join inside the file, compiled with
    -fsanitize=address,undefined and run as a child process (every buffer exactly as large as the host library makes it)."""
    exe = str(tmp_path / "emu_text_main")
    src = os.path.join(H.ROOT, "tests", "emu", "emu_text_main.cc")
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "text emulation ok" in r.stdout
