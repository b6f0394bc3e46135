"""Patch streams accumulated back into canonical rows (peritext_amd/csrc/accum_core.h: reference/test/accumulatePatches.ts on the device, the third
assertion of the reference's fuzzer, test/fuzz.ts:245-278) on the CPU emulation: every lane order, both state stores (the LDS window and the slice of global
scratch, each filled with 0xA5 first).  The cases and their expected values are tests/accum_cases.py's: the reference's spans through helpers.check_log, never
the code under test.  tests/test_gpu_accum.py repeats them through the C ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import accum_cases as AC
import helpers as H
from peritext_amd import abi, wire

EMU_ACCUM_LIB = os.path.join(H.ROOT, "tests", "emu", "libperitext_emu_accum.so")
# (no skip when the library is missing: __graft_entry__.build() makes it with the other emulation libraries, and a missing one is an error)

REVERSE = [0, 1, 2]
STORES = ["lds", "hbm"]


def emu_accum(batch, pat, hbm=False, reverse=0, lds_bytes=H.LDS_BYTES, want=None, rows=True):
    """ptx_accumulate_patches over a wire.Batch through the host emulation: wire.Results in the capacity layout (+ the check rows when `want` is given)."""
    lib = C.CDLL(EMU_ACCUM_LIB)
    lib.ptx_emu_accum.restype = C.c_int
    lib.ptx_emu_accum.argtypes = [C.c_void_p] * 10 + [C.c_int, C.c_int, C.c_uint32, C.c_void_p]
    n = max(batch.n_ops, 1)
    res = wire.Results(logs=np.zeros(batch.n_logs, dtype=abi.LOG_RESULT_DTYPE), values=np.full(n, 0xDEADBEEF, dtype=np.uint32), spans=np.zeros(n, dtype=abi.SPAN_DTYPE),
                       cintervals=np.zeros(n, dtype=abi.CINTERVAL_DTYPE), elem_rank=np.zeros(0, dtype=np.uint32))
    check = np.zeros(max(batch.n_logs, 1), dtype=abi.PATCH_CHECK_DTYPE) if want is not None else None
    used = np.zeros(max(batch.n_logs, 1), dtype=np.uint8)
    off = np.ascontiguousarray(pat.patch_off, dtype=np.uint64)
    logs = np.ascontiguousarray(pat.logs, dtype=abi.PATCH_LOG_DTYPE)
    recs = np.ascontiguousarray(pat.patches, dtype=abi.PATCH_DTYPE)
    s = H.batch_struct(batch)
    vp = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    rc = lib.ptx_emu_accum(C.cast(C.byref(s), C.c_void_p), vp(off), vp(logs), vp(recs), vp(res.logs), vp(res.values) if rows else None, vp(res.spans) if rows else None,
                           vp(res.cintervals) if rows else None, vp(want), vp(check), 1 if hbm else 0, reverse, lds_bytes, vp(used))
    assert rc == 0
    res.used_hbm = used[:batch.n_logs]
    return (res, check[:batch.n_logs]) if want is not None else res


def stream_fn(reverse):
    def f(batch):
        res = H.emu_merge(batch, reverse=reverse, admission=True)
        f.merged = res
        return H.emu_replay(batch, res, reverse=reverse)
    return f


def acc_fn(store, reverse):
    def f(batch, pat):
        res = emu_accum(batch, pat, hbm=(store == "hbm"), reverse=reverse)
        assert res.used_hbm.all() if store == "hbm" else not res.used_hbm.any()
        return res
    return f


@pytest.mark.parametrize("reverse", REVERSE)
@pytest.mark.parametrize("store", STORES)
def test_chunk_edge_quirk_and_boundary_streams(store, reverse):
    """Cases 1 and 2 of the issue in one batch: the chunk-edge document, helpers.edge_case_docs(), helpers.boundary_docs(), the 46 KATs, the 9 traces."""
    sf = stream_fn(reverse)
    batch, pat, res, _ = AC.run_quirks(sf, acc_fn(store, reverse))
    # what the merge computed and what the stream rebuilds are the same rows (the check of ptx_check_patches, here on the host)
    assert np.array_equal(res.logs["digest"], sf.merged.logs["digest"]) and np.array_equal(res.logs["n_elems"], sf.merged.logs["n_elems"])


@pytest.mark.parametrize("reverse", REVERSE)
@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("name", AC.FIXTURES)
def test_fixtures(name, store, reverse):
    AC.run_fixture(name, stream_fn(reverse), acc_fn(store, reverse))


@pytest.mark.parametrize("name", AC.FIXTURES[:1] + AC.FIXTURES[2:3])
def test_both_stores_write_the_same_rows(name):
    docs, _ = AC.fixture_case(name)
    batch = wire.encode_docs(docs)
    pat = stream_fn(0)(batch)
    a, b = emu_accum(batch, pat, hbm=False), emu_accum(batch, pat, hbm=True, reverse=2)
    skip = ("reserved",)
    for f in a.logs.dtype.names:
        assert f in skip or np.array_equal(a.logs[f], b.logs[f]), f
    assert np.array_equal(a.values, b.values) and np.array_equal(a.spans, b.spans) and np.array_equal(a.cintervals, b.cintervals)


@pytest.mark.parametrize("reverse", REVERSE)
@pytest.mark.parametrize("store", STORES)
def test_failed_log_beside_good_ones(store, reverse):
    AC.run_failed_log(stream_fn(reverse), acc_fn(store, reverse))


@pytest.mark.parametrize("reverse", REVERSE)
@pytest.mark.parametrize("store", STORES)
def test_foreign_streams(store, reverse):
    AC.run_foreign_streams(stream_fn(reverse), acc_fn(store, reverse))


def test_a_log_beyond_the_lds_window_takes_the_hbm_store_and_counts_only_mode():
    """The host library's routing: a log whose state exceeds the window goes to the slice of global scratch (here a window of 4 KB); and the form without
    output rows (ptx_check_patches: counts and digest only) with the comparison in the kernel's tail."""
    docs, expected = AC.fixture_case("ptxgen_rich_700.json")
    batch = wire.encode_docs(docs)
    sf = stream_fn(0)
    pat = sf(batch)
    res = emu_accum(batch, pat, lds_bytes=4096)
    assert res.used_hbm.any()
    AC.check_all(batch, res, expected)
    want = sf.merged.logs.copy()
    want["digest"][1][0] ^= 1  # a merge result that is not this stream's
    res2, check = emu_accum(batch, pat, want=want, rows=False)
    assert np.array_equal(res2.logs["digest"], res.logs["digest"]) and (res2.values == 0xDEADBEEF).all()
    assert [int(x) for x in check["agrees"]] == [0 if l == 1 else 1 for l in range(batch.n_logs)]
    assert np.array_equal(check["digest"], res.logs["digest"]) and np.array_equal(check["n_patches"], pat.logs["n_patches"]) and (check["first_bad_record"] == 0xFFFFFFFF).all()


def test_capacity_statuses():
    """More INSERT records than the log has insert rows: refused at that record, never overrun."""
    docs, _ = AC.fixture_case("patches_mini.json")
    batch = wire.encode_docs(docs[:2])
    pat = stream_fn(0)(batch)
    recs = pat.of_log(0)
    k = int(np.flatnonzero(recs["kind"] == abi.PATCH_INSERT)[-1])
    n_ins = int((recs["kind"] == abi.PATCH_INSERT).sum())
    more = np.concatenate([recs, np.repeat(recs[k:k + 1], 1)])
    more["a"][-1] = 0
    for store in STORES:
        res = emu_accum(batch, AC.with_stream(pat, 0, more), hbm=(store == "hbm"))
        assert (int(res.logs["status"][0]), int(res.logs["reserved"][0][1])) == (abi.ERR_CAPACITY, len(recs)) and (res.logs["status"][1:] == 0).all()
    assert n_ins == int(batch.log_hdr["n_ins"][0])


def test_sanitizer_program(tmp_path):
    """tests/emu/emu_accum_main.cc: streams it builds itself (inserts, folded deletes and marks of all four types around the 64-character chunk edges, malformed
    records) through both stores in the three lane orders against a sequential model inside the file, compiled with -fsanitize=address,undefined and run as a
    child process (the LDS block and the state slice are exactly as large as the host library makes them)."""
    exe = str(tmp_path / "emu_accum_main")
    src = os.path.join(H.ROOT, "tests", "emu", "emu_accum_main.cc")
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "accum emulation ok" in r.stdout
