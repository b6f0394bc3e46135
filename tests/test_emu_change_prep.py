"""The preparation of change() from resident InputOperations (peritext_amd/csrc/change_prep_core.h: rows and inserted values per log in 64 bits, the inserts
against `values`, the two offset arrays, the launch's LDS need and list words) on the CPU emulation, in every lane order.  The cases and their expected values
are tests/change_prep_cases.py's; tests/test_gpu_change_device.py runs the C ABI on the GPU.  Every output is pre-filled with 0xA5 and guarded on both sides."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import change_prep_cases as PC
import helpers as H
from peritext_amd import abi

needs_emu = pytest.mark.skipif(not os.path.exists(PC.EMU_PREP_LIB), reason="tests/emu/libperitext_emu_change_prep.so not built (run __graft_entry__.build())")
ORDERS = [0, 1, 2]


def test_the_entry_points_are_declared():
    """The symbols and the struct stand in the C header and in the ctypes prototypes, the ABI version is still 7, the build's no-spill and no-scratch guards name
    the two new kernels and the build makes the emulation library (no skip: this one needs no library)."""
    with open(os.path.join(H.ROOT, "include", "peritext_hip.h")) as f:
        header = f.read()
    for name, nargs in (("ptx_input_ops_upload", 3), ("ptx_input_ops_wrap_device", 5), ("ptx_input_ops_download", 3), ("ptx_host_input_ops_free", 1), ("ptx_input_ops_free", 2),
                        ("ptx_change_device", 6), ("ptx_view_replace_plan_device", 12)):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in abi.FUNCTIONS and len(abi.FUNCTIONS[name][1]) == nargs, name
    assert re.search(r"typedef\s+struct\s+ptx_dinput_ops\s+ptx_dinput_ops\s*;", header) and re.search(r"typedef\s+struct\s+ptx_host_input_ops\s*\{", header)
    assert re.search(r"#define\s+PTX_ABI_VERSION\s+7u", header) and abi.PTX_ABI_VERSION == 7, "the additions are purely additive"
    assert C.sizeof(abi.ptx_host_input_ops) == C.sizeof(abi.ptx_input_ops) + 3 * 8
    with open(os.path.join(H.ROOT, "__graft_entry__.py")) as f:
        entry = f.read()
    for guard in (re.search(r"NO_SPILL_KERNELS = \((.*?)\)", entry, re.S).group(1), re.search(r"NO_SCRATCH_KERNELS = .*", entry).group(0)):
        for k in ("ptx_change_prep_kernel", "ptx_change_offsets_check_kernel"):
            assert '"%s"' % k in guard, "the build's guard names " + k
    assert "libperitext_emu_change_prep.so" in entry
    from peritext_amd.engine import Engine, TextView

    for m in ("upload_input_ops", "wrap_input_ops", "download_input_ops", "free_input_ops", "change_device", "replace_text_resident"):
        assert callable(getattr(Engine, m)), m
    assert callable(TextView.replace_plan_device)


@needs_emu
def test_the_emulation_is_built_from_this_header():
    lib = PC._Shim.get()
    assert lib.ptx_emu_prep_abi_version() == 7 and lib.ptx_emu_prep_rows_max() == PC.ROWS_MAX == 65534
    assert lib.ptx_emu_prep_log_hdr_bytes() == abi.LOG_HDR_DTYPE.itemsize


def _check(c, reverse, all_in_hbm=False, max_lds=PC.MAX_LDS):
    want = PC.expected(c, all_in_hbm=all_in_hbm, max_lds=max_lds)
    got = PC.emu_prep(c, reverse, all_in_hbm=all_in_hbm, max_lds=max_lds)
    assert got["error"] == want["error"], c.name
    if want["error"] is not None:
        return want
    if c.n_logs == 0:
        assert got["out_off"].tolist() == [0] and got["list_off"].tolist() == [0] and got["need"] == 0, c.name
        return want
    for k in ("rows", "list_words", "out_off", "list_off"):
        assert np.array_equal(got[k], want[k]), (c.name, k)
    assert got["need"] == want["need"], c.name
    return want


@needs_emu
@pytest.mark.parametrize("reverse", ORDERS)
@pytest.mark.parametrize("all_in_hbm", [False, True], ids=["lds", "hbm"])
def test_lane_edges_and_change_counts(reverse, all_in_hbm):
    busy = 0
    for c in PC.lane_edge_cases():
        want = _check(c, reverse, all_in_hbm=all_in_hbm)
        if c.n_logs and want["error"] is None:
            busy += int((want["rows"] > 0).sum())
            assert bool(want["list_words"].any()) == (all_in_hbm and bool((np.diff(c.ops.chg_off.astype(np.int64)) > 0).any())), c.name
    assert busy >= 21  # no case dropped


@needs_emu
@pytest.mark.parametrize("reverse", ORDERS)
@pytest.mark.parametrize("n_logs", PC.MANY)
def test_many_logs_most_of_them_idle(reverse, n_logs):
    """The scan's chunk edges (1 024 logs a step); PTX_CHANGE_LIST_IN_HBM on and off, and an LDS so small that some lists fit and some do not."""
    c = PC.many_logs_case(n_logs)
    want = _check(c, reverse)
    assert not want["list_words"].any() and int(want["out_off"][-1]) > 0
    want = _check(c, reverse, all_in_hbm=True)
    assert int((want["list_words"] > 0).sum()) == int((np.diff(c.ops.chg_off.astype(np.int64)) > 0).sum())
    small = PC.lds_need(6, 2, 1, 2)  # a log of six elements that inserts two values fits, one that inserts three does not (the list is rounded to 16 bytes)
    assert PC.lds_need(6, 3, 1, 2) > small
    want = _check(c, reverse, max_lds=small)
    if n_logs > 1:
        assert 0 < int((want["list_words"] > 0).sum()) < int((np.diff(c.ops.chg_off.astype(np.int64)) > 0).sum())


@needs_emu
@pytest.mark.parametrize("reverse", ORDERS)
def test_limits_of_rows_and_values(reverse):
    valid = 0
    for c in PC.limit_cases():
        want = _check(c, reverse)
        assert (want["error"] is None) == (c.want_error is None), c.name
        valid += want["error"] is None
    assert valid == 4
    c = PC.limit_cases()[0]
    assert PC.expected(c)["rows"].tolist() == [65534]


@needs_emu
@pytest.mark.parametrize("reverse", ORDERS)
def test_bad_offsets(reverse):
    cases = PC.offset_cases() + PC.wrapped_size_cases()
    assert len(cases) == 2 + 2 * 5 + 2 + 2
    for c in cases:
        assert c.want_error is not None
        _check(c, reverse)


@needs_emu
def test_sanitizer_program(tmp_path):
    """tests/emu/emu_change_prep_main.cc: the offsets check, the prepare pass and the scans over arrays that end exactly at their last element, against a
    sequential loop inside the file, compiled with -fsanitize=address,undefined and run as a child process."""
    exe = str(tmp_path / "emu_change_prep_main")
    src = os.path.join(H.ROOT, "tests", "emu", "emu_change_prep_main.cc")
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "change prep emulation ok" in r.stdout
