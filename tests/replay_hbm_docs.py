"""Shared inputs of the HBM-state replay tests (test_emu_replay_hbm.py, test_gpu_replay_hbm.py): two documents whose replay working set exceeds the 160 KB of
LDS of one CU, their expected patch streams from the oracle (ONE call for both, cached per process), and the ctypes binding of the emulation driver
tests/emu/emu_replay_hbm.cc."""
import ctypes as C
import functools
import os
import random

import numpy as np

import helpers as H
from peritext_amd import abi, wire

EMU_HBM_LIB = os.path.join(H.ROOT, "tests", "emu", "libperitext_emu_replay_hbm.so")
NONE64 = 0xFFFFFFFFFFFFFFFF


def doc_a():
    """100 000 characters typed in order, 3 000 deletes, then 3 000 random mark ops of the four types (one op per change)."""
    return H.synthetic_marks_log(100000, 3000, 23, n_deletes=3000)


def scattered_typing_log(n_ops, seed, per_change=50):
    """A single-actor log of n_ops ops after the makeList, in changes of per_change ops: with probability 15/110 a delete of a random live element, otherwise an
    insert after the last element typed — one insert in eight after a uniformly random earlier element instead."""
    rnd = random.Random(seed)
    ops = [{"opId": "1@doc1", "action": "makeList", "obj": "_root", "key": "text"}]
    changes, start, seq = [], 1, 1
    live, everyone, last, ctr = [], [], "_head", 2

    def flush():
        nonlocal ops, start, seq
        if ops:
            changes.append({"actor": "doc1", "seq": seq, "deps": {}, "startOp": start, "ops": ops})
            seq += 1
            start = ctr
            ops = []

    for _ in range(n_ops):
        oid = "%d@doc1" % ctr
        if live and rnd.random() < 15.0 / 110.0:
            k = rnd.randrange(len(live))
            live[k], live[-1] = live[-1], live[k]
            ops.append({"opId": oid, "action": "del", "obj": "1@doc1", "elemId": live.pop()})
        else:
            after = everyone[rnd.randrange(len(everyone))] if everyone and rnd.randrange(8) == 0 else last
            ops.append({"opId": oid, "action": "set", "obj": "1@doc1", "elemId": after, "insert": True, "value": "abcdefghij"[rnd.randrange(10)]})
            live.append(oid)
            everyone.append(oid)
            last = oid
        ctr += 1
        if len(ops) >= per_change:
            flush()
    flush()
    return changes


def doc_b():
    return scattered_typing_log(110000, 7)


def typed_log(n_chars):
    """n_chars typed in order in ONE change (the stream is known without an oracle: makeList, then insert k at index k)."""
    ids = ["%d@doc1" % (2 + i) for i in range(n_chars)]
    ops = [{"opId": "1@doc1", "action": "makeList", "obj": "_root", "key": "text"}]
    for i in range(n_chars):
        ops.append({"opId": ids[i], "action": "set", "obj": "1@doc1", "elemId": "_head" if i == 0 else ids[i - 1], "insert": True, "value": "abcdefghij"[i % 10]})
    return [{"actor": "doc1", "seq": 1, "deps": {}, "startOp": 1, "ops": ops}]


@functools.lru_cache(maxsize=None)
def docs():
    """[[A], [B]]: one replica log per document."""
    return [[doc_a()], [doc_b()]]


@functools.lru_cache(maxsize=None)
def expected():
    """What the oracle's applyChange returns for docs(), patches included (about two minutes: once per process)."""
    return H.oracle_apply(docs(), patches=True, timeout=1800)


@functools.lru_cache(maxsize=None)
def batch():
    return wire.encode_docs(docs())


def lds_working_set(b, log):
    """Bytes of LDS the replay of replay_core.h needs for the log (its form with the tables in global memory, 32-bit ranks and slots)."""
    lib = C.CDLL(H.EMU_LIB)
    lib.ptx_emu_replay_lds_need_wide.restype = C.c_uint64
    lib.ptx_emu_replay_lds_need_wide.argtypes = [C.c_uint64] * 4
    h = b.log_hdr[log]
    K, Kc = int(h["n_mark"].sum()), int(h["n_mark"][3])
    return int(lib.ptx_emu_replay_lds_need_wide(int(h["n_ins"]), K, Kc, int(h["n_comment_ids"]) if Kc else 0))


@functools.lru_cache(maxsize=None)
def _lib(path=EMU_HBM_LIB):
    lib = C.CDLL(path)
    lib.ptx_emu_replay_hbm.restype = C.c_int
    lib.ptx_emu_replay_hbm.argtypes = [C.c_void_p] * 8 + [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.ptx_emu_replay_hbm_units.restype = C.c_uint64
    lib.ptx_emu_replay_hbm_units.argtypes = [C.c_uint64] * 4
    lib.ptx_emu_replay_hbm_lds_bytes.restype = C.c_uint32
    return lib


def _call(lib, b, res, off, rows, logs, reverse, first, arena, ext):
    s = H.batch_struct(b)
    hi = getattr(res, "ref_slots_hi", None)
    rc = lib.ptx_emu_replay_hbm(C.cast(C.byref(s), C.c_void_p), res.logs.ctypes.data, res.elem_rank.ctypes.data, res.ref_slots.ctypes.data, None if hi is None else hi.ctypes.data,
                                off.ctypes.data, rows.ctypes.data, logs.ctypes.data, reverse, None if first is None else first.ctypes.data, arena, None if ext is None else ext.ctypes.data)
    assert rc == 0


def emu_replay_hbm(b, res, reverse=0, cap=None, first_row=None, lib_path=EMU_HBM_LIB):
    """Patch streams from the host emulation of replay_hbm_core.h, every log of the batch with its state in a scratch slice: wire.Patches (as helpers.emu_replay:
    capacities of two records per row, once more with exact ones where a log outgrows them; cap: that many records per log, no second run)."""
    n_logs = b.n_logs
    sizes = np.diff(b.log_off.astype(np.int64))
    first = None if first_row is None else np.ascontiguousarray(first_row, dtype=np.uint32)
    if first is not None:
        sizes = sizes - np.minimum(first.astype(np.int64), sizes)
    caps = (2 * sizes + 16) if cap is None else np.full(n_logs, cap, dtype=np.int64)
    off = np.zeros(n_logs + 1, dtype=np.uint64)
    off[1:] = np.cumsum(caps)
    logs = np.zeros(n_logs, dtype=abi.PATCH_LOG_DTYPE)
    rows = np.zeros(max(int(off[-1]), 1), dtype=abi.PATCH_DTYPE)
    lib = _lib(lib_path)
    launches = 0
    while True:
        _call(lib, b, res, off, rows, logs, reverse, first, 0, None)
        launches += 1
        produced = logs["n_patches"].astype(np.int64)
        if launches == 2 or cap is not None or not np.any(produced > caps):
            break
        caps = np.maximum(produced, 1)
        off[1:] = np.cumsum(caps)
        rows = np.zeros(max(int(off[-1]), 1), dtype=abi.PATCH_DTYPE)
    return wire.Patches(patch_off=off, logs=logs, patches=rows, launches=launches, hbm_logs=n_logs)


def emu_replay_hbm_with_arena(b, res, cap, arena, reverse=0, lib_path=EMU_HBM_LIB):
    """`cap` records of capacity per log and an overflow arena of `arena` records behind the capacities, packed to exact offsets as the library's pack kernel
    does (helpers.emu_replay_with_arena for this driver): (wire.Patches, the extents)."""
    n_logs = b.n_logs
    off = (np.arange(n_logs + 1, dtype=np.uint64) * np.uint64(cap)).astype(np.uint64)
    logs = np.zeros(n_logs, dtype=abi.PATCH_LOG_DTYPE)
    rows = np.zeros(int(off[-1]) + arena + 1, dtype=abi.PATCH_DTYPE)
    ext = np.zeros(3 * max(n_logs, 1), dtype=np.uint64)
    _call(_lib(lib_path), b, res, off, rows, logs, reverse, None, arena, ext)
    xoff = np.zeros(n_logs + 1, dtype=np.uint64)
    xoff[1:] = np.cumsum(np.where(logs["status"] == 0, logs["n_patches"], 0).astype(np.uint64))
    packed = np.zeros(max(int(xoff[-1]), 1), dtype=abi.PATCH_DTYPE)
    for l in range(n_logs):
        n = int(xoff[l + 1] - xoff[l])
        a = min(n, cap)
        packed[int(xoff[l]):int(xoff[l]) + a] = rows[int(off[l]):int(off[l]) + a]
        if n > a:
            x0, x1, xcap = int(ext[3 * l]), int(ext[3 * l + 1]), int(ext[3 * l + 2])
            assert x0 != NONE64
            k = min(n - a, xcap)
            packed[int(xoff[l]) + a:int(xoff[l]) + a + k] = rows[x0:x0 + k]
            if n - a > k:
                assert x1 != NONE64
                packed[int(xoff[l]) + a + k:int(xoff[l]) + n] = rows[x1:x1 + n - a - k]
    return wire.Patches(patch_off=xoff, logs=logs, patches=packed, launches=1, hbm_logs=n_logs), ext.reshape(-1, 3)


def stream(pat, log):
    """The records of one log."""
    b0 = int(pat.patch_off[log])
    return pat.patches[b0:b0 + int(pat.logs["n_patches"][log])]
