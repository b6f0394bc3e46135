"""Shared test plumbing: oracle invocation (node), the host emulation of the kernel logic, comparison."""
import ctypes as C
import functools
import gzip
import hashlib
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np

from peritext_amd import abi, canon, wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NODE = shutil.which("node")
EMU_LIB = os.environ.get("PTX_EMU_LIB") or os.path.join(ROOT, "tests", "emu", "libperitext_emu.so")
LDS_BYTES = 160 * 1024


def have_node():
    return NODE is not None


def run_node(args, timeout=600):
    p = subprocess.run([NODE] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError("node %s failed:\n%s\n%s" % (" ".join(args), p.stdout[-2000:], p.stderr[-2000:]))
    return p.stdout


@functools.lru_cache(maxsize=None)
def oracle_gen(config="mini", docs=4, seed=1, ops=None, replicas=None, first=0, impl="oracle", mix=None, marks=None, initial_text=None):
    """PTXGEN traces + expected output from the oracle (or the erased reference with impl='ref')."""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "gen.json")
        args = ["oracle/cli.js", "gen", "--config", config, "--docs", str(docs), "--seed", str(seed), "--first", str(first), "--impl", impl, "--out", out]
        if ops is not None:
            args += ["--ops", str(ops)]
        if replicas is not None:
            args += ["--replicas", str(replicas)]
        if mix is not None:
            args += ["--mix", ",".join(str(x) for x in mix)]
        if marks is not None:
            args += ["--marks", ",".join(marks)]
        if initial_text is not None:
            args += ["--initial-text", initial_text]
        run_node(args)
        with open(out) as f:
            return json.load(f)


def oracle_apply(docs_logs, impl="oracle", cursors=False, patches=False, roots=False, no_patches=False, timeout=600):
    """Apply every log of every doc to a fresh oracle replica; returns [[{spans,text,error?}]]."""
    with tempfile.TemporaryDirectory() as td:
        inp, out = os.path.join(td, "in.json"), os.path.join(td, "out.json")
        with open(inp, "w") as f:
            json.dump({"docs": [{"logs": logs} for logs in docs_logs]}, f)
        run_node(["oracle/cli.js", "apply", "--in", inp, "--impl", impl, "--out", out] + (["--cursors"] if cursors else []) + (["--patches"] if patches else []) + (["--roots"] if roots else []) + (["--no-patches"] if no_patches else []), timeout=timeout)
        with open(out) as f:
            return [d["expected"] for d in json.load(f)["docs"]]


def oracle_change(docs_logs, calls, actors, impl="oracle"):
    """doc.change(ops) on replicas rebuilt from their logs (oracle/cli.js change): calls[l] = list of change() calls of the
    replica behind log l (document-major order), actors[l] its actor id.  Returns the Changes made, flat in log order (one list
    entry per call); an error of the oracle is raised."""
    reps, l = [], 0
    for logs in docs_logs:
        for log in logs:
            reps.append({"actor": actors[l], "log": log, "calls": calls[l]})
            l += 1
    with tempfile.TemporaryDirectory() as td:
        inp, out = os.path.join(td, "in.json"), os.path.join(td, "out.json")
        with open(inp, "w") as f:
            json.dump({"replicas": reps}, f)
        run_node(["oracle/cli.js", "change", "--in", inp, "--impl", impl, "--out", out])
        with open(out) as f:
            res = json.load(f)["replicas"]
    flat = []
    for r in res:
        if "error" in r:
            raise RuntimeError(r["error"])
        flat += r["changes"]
    return flat


def _load_golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def inputs_sha16(obj):
    """Identity of the inputs a fixture of the reference's answers was made for (inputs built here in Python, not stored with it)."""
    return hashlib.sha256(json.dumps(obj, sort_keys=True).encode("utf-8")).hexdigest()[:16]


def wide_envelope_golden():
    """tests/golden/wide_envelope_ref.json.gz (tests/make_wide_envelope_golden.py): what the type-erased reference answers for the logs of
    more than 65 535 changes that test_emu_biglog.wide_envelope_docs() and test_emu_change.past_65535_replica() build."""
    with gzip.open(os.path.join(GOLDEN, "wide_envelope_ref.json.gz"), "rt", encoding="utf-8") as f:
        g = json.load(f)
    assert g["impl"] == "ref"
    return g


def batch_struct(b):
    """ctypes ptx_batch pointing into the numpy columns of a wire.Batch (keep `b` alive)."""
    s = abi.ptx_batch()
    s.n_logs = b.n_logs
    s.n_ops = b.n_ops
    ptr = lambda a, t: a.ctypes.data_as(t)  # noqa: E731
    s.log_off = ptr(b.log_off, abi.u64p)
    s.op_id = ptr(b.op_id, abi.u64p)
    s.ref_a = ptr(b.ref_a, abi.u64p)
    s.ref_b = ptr(b.ref_b, abi.u64p)
    s.payload = ptr(b.payload, abi.u32p)
    s.action = ptr(b.action, abi.u8p)
    s.mark_type = ptr(b.mark_type, abi.u8p)
    s.side_a = ptr(b.side_a, abi.u8p)
    s.side_b = ptr(b.side_b, abi.u8p)
    if b.chg_off is not None:  # a batch without the Change envelope: NULL = no admission
        s.chg_off = ptr(b.chg_off, abi.u64p)
        s.chg_hdr = ptr(b.chg_hdr, abi.u32p)
        s.chg_env = ptr(b.chg_env, abi.u16p)
        if b.chg_env_hi is not None:
            s.chg_env_hi = ptr(b.chg_env_hi, abi.u16p)
        s.max_actors = b.max_actors
    if b.log_hdr is not None and len(b.log_hdr):
        s.log_hdr = b.log_hdr.ctypes.data_as(C.POINTER(abi.ptx_log_hdr))
    return s


@functools.lru_cache(maxsize=None)
def _emu(path):
    lib = C.CDLL(path)
    for fn in (lib.ptx_emu_merge, lib.ptx_emu_merge_admit):
        fn.restype = C.c_int
        fn.argtypes = [C.POINTER(abi.ptx_batch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int]
    lib.ptx_emu_replay.restype = C.c_int
    lib.ptx_emu_replay.argtypes = [C.POINTER(abi.ptx_batch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int]
    lib.ptx_emu_replay_from.restype = C.c_int
    lib.ptx_emu_replay_from.argtypes = lib.ptx_emu_replay.argtypes + [C.c_void_p]
    lib.ptx_emu_merge_refs.restype = C.c_int
    lib.ptx_emu_merge_refs.argtypes = [C.POINTER(abi.ptx_batch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int]
    return lib


def emu_merge(b, lds_bytes=LDS_BYTES, reverse=0, lib_path=EMU_LIB, admission=False, lean=False):
    """Run the host emulation of the kernel logic (tests only) over a wire.Batch.  lean: the body the ptx_merge_kernel_lean* builds are made of (no elem_rank,
    no resolved references, 16-bit id keys) for every log that qualifies."""
    n = max(b.n_ops, 1)
    if lean:
        res = wire.Results(
            logs=np.zeros(b.n_logs, dtype=abi.LOG_RESULT_DTYPE),
            values=np.full(n, 0xDEADBEEF, dtype=np.uint32),
            spans=np.zeros(n, dtype=abi.SPAN_DTYPE),
            cintervals=np.zeros(n, dtype=abi.CINTERVAL_DTYPE),
            elem_rank=None,
        )
        s = batch_struct(b)
        f = _emu(lib_path).ptx_emu_merge_lean
        f.restype = C.c_int
        f.argtypes = [C.POINTER(abi.ptx_batch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int]
        rc = f(C.byref(s), res.logs.ctypes.data, res.values.ctypes.data, res.spans.ctypes.data, res.cintervals.ctypes.data, lds_bytes, reverse, 1 if admission else 0)
        assert rc == 0
        return res
    res = wire.Results(
        logs=np.zeros(b.n_logs, dtype=abi.LOG_RESULT_DTYPE),
        values=np.full(n, 0xDEADBEEF, dtype=np.uint32),
        spans=np.zeros(n, dtype=abi.SPAN_DTYPE),
        cintervals=np.zeros(n, dtype=abi.CINTERVAL_DTYPE),
        elem_rank=np.zeros(n, dtype=np.uint32),
        ref_slots=np.full(n, 0xFFFFFFFF, dtype=np.uint32),
    )
    s = batch_struct(b)
    rc = _emu(lib_path).ptx_emu_merge_refs(
        C.byref(s), res.logs.ctypes.data, res.values.ctypes.data, res.spans.ctypes.data, res.cintervals.ctypes.data,
        res.elem_rank.ctypes.data, res.ref_slots.ctypes.data, lds_bytes, reverse, 1 if admission else 0,
    )
    assert rc == 0
    return res


def synthetic_marks_log(n_chars, n_marks, seed, n_deletes=0, max_span=40):
    """ONE replica log (Change[]) built without the generator: a text of n_chars, n_deletes deletes, then n_marks random add / removeMark ops of the four mark
    types over it (the boundary rule of peritext.ts:483-497: inclusive marks end `before` the next element or at endOfText, the others `after` the last).
    For documents far beyond what the oracle's change() generates in reasonable time; the expected output comes from the oracle's applyChange."""
    import random

    rnd = random.Random(seed)
    ids = ["%d@doc1" % (2 + i) for i in range(n_chars)]
    ops = [{"opId": "1@doc1", "action": "makeList", "obj": "_root", "key": "text"}]
    for i in range(n_chars):
        ops.append({"opId": ids[i], "action": "set", "obj": "1@doc1", "elemId": "_head" if i == 0 else ids[i - 1], "insert": True, "value": "abcdefghij"[rnd.randrange(10)]})
    changes = [{"actor": "doc1", "seq": 1, "deps": {}, "startOp": 1, "ops": ops}]
    ctr = n_chars + 2
    seq = 2
    for _ in range(n_deletes):
        changes.append({"actor": "doc1", "seq": seq, "deps": {}, "startOp": ctr, "ops": [{"opId": "%d@doc1" % ctr, "action": "del", "obj": "1@doc1", "elemId": ids[rnd.randrange(n_chars)]}]})
        ctr += 1
        seq += 1
    for _ in range(n_marks):
        mt = ("strong", "em", "link", "comment")[rnd.randrange(4)]
        a = rnd.randrange(n_chars)
        e = a + 1 + rnd.randrange(min(n_chars - a, max_span))  # (the reference copies the op set of every slot it passes: short spans keep it tractable)
        op = {"opId": "%d@doc1" % ctr, "action": "addMark" if rnd.random() < 0.65 else "removeMark", "obj": "1@doc1", "start": {"type": "before", "elemId": ids[a]}, "markType": mt}
        if mt in ("strong", "em"):
            op["end"] = {"type": "endOfText"} if e >= n_chars else {"type": "before", "elemId": ids[e]}
        else:
            op["end"] = {"type": "after", "elemId": ids[e - 1]}
        if mt == "link" and op["action"] == "addMark":
            op["attrs"] = {"url": "%s.com" % "ABCDEFGHIJKLMNOPQRSTUVWXYZ"[rnd.randrange(26)]}
        if mt == "comment":
            op["attrs"] = {"id": "comment-%d" % rnd.randrange(max(1, n_marks // 40))}
        changes.append({"actor": "doc1", "seq": seq, "deps": {}, "startOp": ctr, "ops": [op]})
        ctr += 1
        seq += 1
    return changes


def _emu_set_refs_hi(lib, arr):
    """(round 6) the emulation's stand-in for ptx_dresult.refs_hi: the buffer the next merge writes / the next replay or change() reads (None: a result without it)"""
    lib.ptx_emu_set_refs_hi.argtypes = [C.c_void_p]
    lib.ptx_emu_set_refs_hi.restype = None
    lib.ptx_emu_set_refs_hi(None if arr is None else arr.ctypes.data)


def emu_merge_big(b, reverse=0, lib_path=EMU_LIB, admission=False, slack=0, refs_hi=True):
    """The HBM-staged path for logs beyond one CU's LDS (biglog_core.h) through the host emulation: every log of the batch, whatever its size.
    refs_hi: the result carries the high halves of the boundary slots (what ptx_result_alloc provides when the census finds a log of more than 32 766 elements)."""
    n = max(b.n_ops, 1)
    res = wire.Results(
        logs=np.zeros(b.n_logs, dtype=abi.LOG_RESULT_DTYPE),
        values=np.full(n, 0xDEADBEEF, dtype=np.uint32),
        spans=np.zeros(n, dtype=abi.SPAN_DTYPE),
        cintervals=np.zeros(n, dtype=abi.CINTERVAL_DTYPE),
        elem_rank=np.zeros(n, dtype=np.uint32),
        ref_slots=np.full(n, 0xFFFFFFFF, dtype=np.uint32),
        ref_slots_hi=np.full(n, 0xFFFFFFFF, dtype=np.uint32) if refs_hi else None,
    )
    s = batch_struct(b)
    _emu_set_refs_hi(_emu(lib_path), res.ref_slots_hi)
    f = _emu(lib_path).ptx_emu_merge_big
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_void_p]
    rc = f(C.byref(s), res.logs.ctypes.data, res.values.ctypes.data, res.spans.ctypes.data, res.cintervals.ctypes.data, res.elem_rank.ctypes.data, reverse,
           1 if admission else 0, slack, res.ref_slots.ctypes.data)
    _emu_set_refs_hi(_emu(lib_path), None)
    assert rc == 0
    return res


def emu_exact_walks(lib_path=EMU_LIB):
    """Logs (so far, in this process) whose one-pass admission check failed and were walked again by the exact code."""
    f = _emu(lib_path).ptx_emu_exact_walk_count
    f.restype = C.c_ulonglong
    return int(f())


def emu_replay(b, res, lds_bytes=160 * 1024, reverse=0, lib_path=EMU_LIB, cap=None, gwin=False, first_row=None):
    """Patch streams from the host emulation of replay_core.h (tests only): wire.Patches.  gwin: the form with the per-slot link urls, the op tables and the comment ops' id tables in global memory;
    first_row[l]: only the records of the rows from there on (ptx_replay_patches_from)."""
    reverse |= 256 if gwin else 0
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
    s = batch_struct(b)
    lib = _emu(lib_path)
    _emu_set_refs_hi(lib, getattr(res, "ref_slots_hi", None))
    launches = 0
    while True:
        rc = lib.ptx_emu_replay_from(C.byref(s), res.logs.ctypes.data, res.elem_rank.ctypes.data, res.ref_slots.ctypes.data, off.ctypes.data, rows.ctypes.data, logs.ctypes.data, lds_bytes, reverse,
                                     None if first is None else first.ctypes.data)
        assert rc == 0
        launches += 1
        produced = logs["n_patches"].astype(np.int64)
        if launches == 2 or cap is not None or not np.any(produced > caps):
            break
        caps = np.maximum(produced, 1)  # what ptx_replay_patches does: once more with exact sizes
        off[1:] = np.cumsum(caps)
        rows = np.zeros(max(int(off[-1]), 1), dtype=abi.PATCH_DTYPE)
    _emu_set_refs_hi(lib, None)
    return wire.Patches(patch_off=off, logs=logs, patches=rows, launches=launches)


def emu_replay_with_arena(b, res, cap, arena, lds_bytes=160 * 1024, reverse=0, lib_path=EMU_LIB, gwin=False):
    """The replay with `cap` records of capacity per log and an overflow arena of `arena` records behind the capacities (what ptx_replay_patches does in its one
    launch), packed to exact offsets here as the library's pack kernel does: wire.Patches."""
    reverse |= 256 if gwin else 0
    n_logs = b.n_logs
    off = (np.arange(n_logs + 1, dtype=np.uint64) * np.uint64(cap)).astype(np.uint64)
    logs = np.zeros(n_logs, dtype=abi.PATCH_LOG_DTYPE)
    rows = np.zeros(int(off[-1]) + arena + 1, dtype=abi.PATCH_DTYPE)
    ext = np.zeros(3 * max(n_logs, 1), dtype=np.uint64)
    s = batch_struct(b)
    lib = _emu(lib_path)
    lib.ptx_emu_replay_arena.restype = C.c_int
    lib.ptx_emu_replay_arena.argtypes = [C.c_void_p] * 7 + [C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
    rc = lib.ptx_emu_replay_arena(C.cast(C.byref(s), C.c_void_p), res.logs.ctypes.data, res.elem_rank.ctypes.data, res.ref_slots.ctypes.data, off.ctypes.data, rows.ctypes.data, logs.ctypes.data,
                                  lds_bytes, reverse, None, arena, ext.ctypes.data)
    assert rc == 0
    xoff = np.zeros(n_logs + 1, dtype=np.uint64)
    xoff[1:] = np.cumsum(np.where(logs["status"] == 0, logs["n_patches"], 0).astype(np.uint64))
    packed = np.zeros(max(int(xoff[-1]), 1), dtype=abi.PATCH_DTYPE)
    for l in range(n_logs):
        n = int(xoff[l + 1] - xoff[l])
        a = min(n, cap)
        packed[int(xoff[l]):int(xoff[l]) + a] = rows[int(off[l]):int(off[l]) + a]
        if n > a:
            x0, x1, xcap = int(ext[3 * l]), int(ext[3 * l + 1]), int(ext[3 * l + 2])
            assert x0 != 0xFFFFFFFFFFFFFFFF
            k = min(n - a, xcap)
            packed[int(xoff[l]) + a:int(xoff[l]) + a + k] = rows[x0:x0 + k]
            if n - a > k:
                assert x1 != 0xFFFFFFFFFFFFFFFF
                packed[int(xoff[l]) + a + k:int(xoff[l]) + n] = rows[x1:x1 + n - a - k]
    return wire.Patches(patch_off=xoff, logs=logs, patches=packed, launches=1), ext.reshape(-1, 3)


def input_ops_struct(ops):
    s = abi.ptx_input_ops()
    s.n_logs, s.max_actors = len(ops.chg_off) - 1, ops.max_actors
    p = lambda a, t: a.ctypes.data_as(t)  # noqa: E731
    s.chg_off, s.op_off = p(ops.chg_off, abi.u64p), p(ops.op_off, abi.u64p)
    s.action, s.mark_type = p(ops.action, abi.u8p), p(ops.mark_type, abi.u8p)
    s.index, s.count, s.payload = p(ops.index, abi.u32p), p(ops.count, abi.u32p), p(ops.payload, abi.u32p)
    s.values, s.n_values, s.actor = p(ops.values, abi.u32p), len(ops.values), p(ops.actor, abi.u32p)
    return s


def rows_of_input_ops(ops):
    """Rows every log will make: one per inserted value, per deleted element, per mark, per makeList."""
    per_op = np.where(ops.action == abi.IN_INSERT, ops.count, np.where(ops.action == abi.IN_DELETE, ops.count, 1)).astype(np.uint64)
    cum = np.concatenate([[0], np.cumsum(per_op)]).astype(np.uint64)
    op_of_log = ops.op_off[ops.chg_off.astype(np.int64)].astype(np.int64)
    return cum[op_of_log]


def made_batch(batch, ops, cols, env, rows_made, chgs_made, out_off):
    """Compact the capacity-layout output of a change() kernel into a wire.Batch of the new Changes (tables of `batch`)."""
    n_logs = batch.n_logs
    na = ops.max_actors
    keep = np.concatenate([np.arange(int(out_off[l]), int(out_off[l]) + int(rows_made[l])) for l in range(n_logs)] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    ckeep = np.concatenate([np.arange(int(ops.chg_off[l]), int(ops.chg_off[l]) + int(chgs_made[l])) for l in range(n_logs)] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    log_off = np.zeros(n_logs + 1, dtype=np.uint64)
    log_off[1:] = np.cumsum(rows_made[:n_logs].astype(np.uint64))
    chg_off = np.zeros(n_logs + 1, dtype=np.uint64)
    chg_off[1:] = np.cumsum(chgs_made[:n_logs].astype(np.uint64))
    return wire.Batch(log_off, cols["op_id"][keep], cols["ref_a"][keep], cols["ref_b"][keep], cols["payload"][keep], cols["action"][keep], cols["mark_type"][keep],
                      cols["side_a"][keep], cols["side_b"][keep], chg_off, env["chg_hdr"][ckeep], env["chg_env"].reshape(-1, abi.env_stride(na))[ckeep].reshape(-1),
                      na, None, batch.values, batch.urls, batch.log_doc, batch.doc_actors, batch.doc_comments, batch.keys, batch.map_values,
                      chg_env_hi=env["chg_env_hi"].reshape(-1, abi.env_stride(na))[ckeep].reshape(-1) if env.get("any_wide") is not None and int(env["any_wide"][0]) else None)


def emu_change(batch, res, ops, lds_bytes=LDS_BYTES, reverse=0, lib_path=EMU_LIB):
    """change() for caller-supplied InputOperations through the host emulation of change_core.h (tests only):
    (wire.Batch of the new Changes, status per log)."""
    n_logs = batch.n_logs
    out_off = rows_of_input_ops(ops)
    T, NC, na = max(int(out_off[-1]), 1), max(int(ops.chg_off[-1]), 1), ops.max_actors
    cols = {"op_id": np.zeros(T, np.uint64), "ref_a": np.zeros(T, np.uint64), "ref_b": np.zeros(T, np.uint64), "payload": np.zeros(T, np.uint32),
            "action": np.zeros(T, np.uint8), "mark_type": np.zeros(T, np.uint8), "side_a": np.zeros(T, np.uint8), "side_b": np.zeros(T, np.uint8)}
    env = {"chg_hdr": np.zeros(NC, np.uint32), "chg_env": np.zeros(NC * abi.env_stride(na), np.uint16), "chg_env_hi": np.zeros(NC * abi.env_stride(na), np.uint16),
           "any_wide": np.zeros(1, np.uint32)}
    status, rows_made, chgs_made = (np.zeros(max(n_logs, 1), np.uint32) for _ in range(3))
    lib = C.CDLL(lib_path)
    lib.ptx_emu_change.restype = C.c_int
    _emu_set_refs_hi(lib, getattr(res, "ref_slots_hi", None))
    s, si = batch_struct(batch), input_ops_struct(ops)
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    rc = lib.ptx_emu_change(C.byref(s), vp(res.logs), vp(res.elem_rank), vp(res.ref_slots), C.byref(si), vp(out_off), vp(cols["op_id"]), vp(cols["ref_a"]), vp(cols["ref_b"]), vp(cols["payload"]),
                            vp(cols["action"]), vp(cols["mark_type"]), vp(cols["side_a"]), vp(cols["side_b"]), vp(env["chg_hdr"]), vp(env["chg_env"]), vp(env["chg_env_hi"]), vp(env["any_wide"]), vp(status), vp(rows_made), vp(chgs_made), C.c_uint32(lds_bytes), C.c_int(reverse))
    _emu_set_refs_hi(lib, None)
    assert rc == 0
    return made_batch(batch, ops, cols, env, rows_made, chgs_made, out_off), status[:n_logs]


def emu_cursors(batch, res, q_log, q_kind, q_arg, lds_bytes=LDS_BYTES, reverse=0, lib_path=EMU_LIB):
    """Cursor queries through the host emulation of cursor_core.h (tests only): (out u64[n], status u32[n])."""
    ql, qk, qa = np.asarray(q_log, np.uint32), np.asarray(q_kind, np.uint8), np.asarray(q_arg, np.uint64)
    n = len(ql)
    perm = np.argsort(ql, kind="stable").astype(np.uint32)
    sl = ql[perm]
    starts = np.flatnonzero(np.concatenate([[True], sl[1:] != sl[:-1]])) if n else np.zeros(0, np.int64)
    g_log = sl[starts].astype(np.uint32)
    g_off = np.concatenate([starts, [n]]).astype(np.uint64)
    out, status = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint32)
    lib = C.CDLL(lib_path)
    lib.ptx_emu_cursors.restype = C.c_int
    s = batch_struct(batch)
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    rc = lib.ptx_emu_cursors(C.byref(s), vp(res.logs), vp(res.elem_rank), C.c_uint32(len(g_log)), vp(g_log), vp(g_off), vp(perm), vp(qk), vp(qa), vp(out), vp(status),
                             C.c_uint32(lds_bytes), C.c_int(reverse))
    assert rc == 0
    return out[:n], status[:n]


def cursor_queries(batch, expected_per_doc):
    """Every getCursor(index) and resolveCursor(elemId) of an oracle `apply --cursors` output as device queries + the wanted answers."""
    q_log, q_kind, q_arg, want = [], [], [], []
    log = 0
    for d in expected_per_doc:
        for e in d:
            actors = batch.doc_actors[batch.log_doc[log]]
            enc = lambda s: (int(s.split("@")[0]) << 32) | actors.index(s.split("@", 1)[1])  # noqa: E731
            for i, elem in enumerate(e["cursorAt"]):
                q_log.append(log), q_kind.append(abi.CURSOR_GET), q_arg.append(i), want.append(enc(elem))
            q_log.append(log), q_kind.append(abi.CURSOR_GET), q_arg.append(len(e["text"])), want.append(None)  # past the end
            for elem, idx in e["cursorResolve"].items():
                q_log.append(log), q_kind.append(abi.CURSOR_RESOLVE), q_arg.append(enc(elem)), want.append(idx)
            q_log.append(log), q_kind.append(abi.CURSOR_RESOLVE), q_arg.append((999999 << 32) | 0), want.append(None)  # no such element
            log += 1
    return q_log, q_kind, q_arg, want


def check_cursor_answers(q_kind, want, out, status):
    for k, w, o, st in zip(q_kind, want, out, status):
        if w is None:
            assert int(st) == (abi.ERR_INDEX_OOB if k == abi.CURSOR_GET else abi.ERR_ELEM_NOT_FOUND)
        else:
            assert int(st) == 0 and int(o) == w


def concat_batches(base, more):
    """Host-side twin of ptx_batch_append: log l of the result = log l of `base` followed by log l of `more` (same tables)."""
    rows, chgs = [], []
    for l in range(base.n_logs):
        rows += [("b", int(base.log_off[l]), int(base.log_off[l + 1])), ("m", int(more.log_off[l]), int(more.log_off[l + 1]))]
        chgs += [("b", int(base.chg_off[l]), int(base.chg_off[l + 1])), ("m", int(more.chg_off[l]), int(more.chg_off[l + 1]))]
    na = max(base.max_actors, more.max_actors)

    def cat(name, parts):
        out = [getattr(base if src == "b" else more, name)[a:b] for src, a, b in parts]
        return np.concatenate(out) if out else np.zeros(0)

    def cat_env(parts):
        out = []
        for src, a, b in parts:
            x = base if src == "b" else more
            out.append((x.chg_actor[a:b], x.chg_seq[a:b], x.chg_nops[a:b], np.pad(x.chg_deps[a:b], ((0, 0), (0, na - x.max_actors))) if b > a else np.zeros((0, na), np.uint32)))
        return wire.pack_envelope_wide(*(np.concatenate([o[k] for o in out]) for k in range(4)), na)

    hdr, env, env_hi = cat_env(chgs)
    return wire.Batch((base.log_off + more.log_off).astype(np.uint64), cat("op_id", rows), cat("ref_a", rows), cat("ref_b", rows), cat("payload", rows), cat("action", rows),
                      cat("mark_type", rows), cat("side_a", rows), cat("side_b", rows), (base.chg_off + more.chg_off).astype(np.uint64), hdr, env, na, None,
                      base.values, base.urls, base.log_doc, base.doc_actors, base.doc_comments, base.keys, base.map_values, chg_env_hi=env_hi)


def mini_doc(ops_second_change, first_text="ABCDE"):
    """A hand-written log: change 1 = makeList + text, change 2 = the given ops (opIds assigned here)."""
    ops1 = [{"opId": "1@a", "action": "makeList", "obj": "_root", "key": "text"}]
    prev = "_head"
    for i, ch in enumerate(first_text):
        ops1.append({"opId": "%d@a" % (i + 2), "action": "set", "obj": "1@a", "elemId": prev, "insert": True, "value": ch})
        prev = "%d@a" % (i + 2)
    c1 = {"actor": "a", "seq": 1, "deps": {}, "startOp": 1, "ops": ops1}
    start = len(ops1) + 1
    ops2 = []
    for k, op in enumerate(ops_second_change):
        o = dict(op)
        o["opId"] = "%d@a" % (start + k)
        o["obj"] = "1@a"
        ops2.append(o)
    c2 = {"actor": "a", "seq": 2, "deps": {"a": 1}, "startOp": start, "ops": ops2}
    return [c1, c2]



# ---- hand-written logs shared by the emulation suite and its GPU twin (tests/test_gpu_edges.py) ----
def edge_case_docs():
    """Quirks of SURVEY.md Appendix A.6 that no reference test covers (one single-replica document each)."""
    _mini_doc = mini_doc
    el = lambda i: "%d@a" % (i + 2)  # noqa: E731  element id of initial char i
    return [
        [_mini_doc([{"action": "removeMark", "markType": "comment", "attrs": {"id": "c1"}, "start": {"type": "before", "elemId": el(1)}, "end": {"type": "after", "elemId": el(3)}}])],
        [_mini_doc([{"action": "addMark", "markType": "strong", "start": {"type": "before", "elemId": el(2)}, "end": {"type": "before", "elemId": el(2)}}])],
        [_mini_doc([{"action": "addMark", "markType": "link", "attrs": {"url": "u"}, "start": {"type": "before", "elemId": el(2)}, "end": {"type": "after", "elemId": el(1)}}])],
        [_mini_doc([{"action": "addMark", "markType": "em", "start": {"type": "before", "elemId": "99@zz"}, "end": {"type": "endOfText"}}])],
        [_mini_doc([{"action": "addMark", "markType": "em", "start": {"type": "before", "elemId": el(3)}, "end": {"type": "endOfText"}},
                    {"action": "set", "insert": True, "elemId": el(4), "value": "!"}])],
        [_mini_doc([], first_text="")],
        [_mini_doc([{"action": "del", "elemId": el(i)} for i in range(5)] + [{"action": "del", "elemId": el(0)}])],
        [_mini_doc([{"action": "addMark", "markType": "comment", "attrs": {"id": "c2"}, "start": {"type": "before", "elemId": el(0)}, "end": {"type": "after", "elemId": el(2)}},
                    {"action": "addMark", "markType": "comment", "attrs": {"id": "c1"}, "start": {"type": "before", "elemId": el(1)}, "end": {"type": "after", "elemId": el(4)}},
                    {"action": "removeMark", "markType": "comment", "attrs": {"id": "c2"}, "start": {"type": "before", "elemId": el(1)}, "end": {"type": "after", "elemId": el(1)}},
                    {"action": "addMark", "markType": "comment", "attrs": {"id": "c2"}, "start": {"type": "before", "elemId": el(4)}, "end": {"type": "after", "elemId": el(4)}}])],
    ]


def boundary_docs():
    """Boundaries `changeMark` (peritext.ts:458-501) never generates but the Operation type allows (peritext.ts:17-21): startOfText as a start and as an end,
    endOfText as a start, an `after` start on an inclusive mark, a `before` end on a link — each with a later insert / delete / second mark around it so that the
    patch stream (getActiveMarksAtIndex, :251-281) meets the slot too.  VERDICT r5 'weak' #1: PTX_SIDE_START_OF_TEXT was exercised by no committed test."""
    el = lambda i: "%d@a" % (i + 2)  # noqa: E731
    bf = lambda i: {"type": "before", "elemId": el(i)}  # noqa: E731
    af = lambda i: {"type": "after", "elemId": el(i)}  # noqa: E731
    sot, eot = {"type": "startOfText"}, {"type": "endOfText"}
    return [
        [mini_doc([{"action": "addMark", "markType": "strong", "start": sot, "end": af(2)},
                   {"action": "set", "insert": True, "elemId": "_head", "value": "x"},
                   {"action": "removeMark", "markType": "strong", "start": sot, "end": bf(1)}])],
        [mini_doc([{"action": "addMark", "markType": "em", "start": bf(1), "end": sot},
                   {"action": "set", "insert": True, "elemId": el(0), "value": "y"},
                   {"action": "addMark", "markType": "link", "attrs": {"url": "u"}, "start": bf(0), "end": sot}])],
        [mini_doc([{"action": "addMark", "markType": "strong", "start": eot, "end": eot},
                   {"action": "addMark", "markType": "comment", "attrs": {"id": "c1"}, "start": eot, "end": af(4)},
                   {"action": "set", "insert": True, "elemId": el(4), "value": "!"}])],
        [mini_doc([{"action": "addMark", "markType": "strong", "start": af(1), "end": af(3)},
                   {"action": "set", "insert": True, "elemId": el(1), "value": "i"},
                   {"action": "del", "elemId": el(2)},
                   {"action": "addMark", "markType": "em", "start": af(0), "end": eot}])],
        [mini_doc([{"action": "addMark", "markType": "link", "attrs": {"url": "u"}, "start": bf(1), "end": bf(3)},
                   {"action": "set", "insert": True, "elemId": el(2), "value": "k"},
                   {"action": "addMark", "markType": "link", "attrs": {"url": "v"}, "start": af(0), "end": bf(2)},
                   {"action": "removeMark", "markType": "link", "start": sot, "end": bf(1)}])],
    ]


def huge_bucket_log(n_head=70):
    """n_head inserts at index 0 (all children of HEAD: 70 take the lane-per-member ranking of a large bucket, more than 256 the bitmap-ranked path)
    interleaved with children of other elements, deletes and a mark."""
    ops = []
    for k in range(n_head):
        ops.append({"action": "set", "insert": True, "elemId": "_head", "value": "abcdefghij"[k % 10]})
        if k % 7 == 0:
            ops.append({"action": "set", "insert": True, "elemId": "3@a", "value": "X"})  # siblings under 'B': a medium bucket
        if k % 9 == 0:
            ops.append({"action": "set", "insert": True, "elemId": "5@a", "value": "y"})
    for k in range(11):
        ops.append({"action": "set", "insert": True, "elemId": "4@a", "value": "m"})  # 11 siblings: the PTX_G-lane path
    ops.append({"action": "del", "elemId": "4@a"})
    ops.append({"action": "addMark", "markType": "strong", "start": {"type": "before", "elemId": "2@a"}, "end": {"type": "endOfText"}})
    return mini_doc(ops)


def unsynced_docs():
    """Replicas that have NOT seen the same changes: every prefix of a replica log is itself a valid log.  The comment ids of
    a document are ranked over all its replicas, so such a log uses ranks beyond its own number of comment ops."""
    with open(os.path.join(GOLDEN, "ptxgen_mini.json")) as f:
        gen = json.load(f)
    docs = []
    for d in gen["docs"][:6]:
        logs = []
        for k, log in enumerate(d["logs"]):
            for frac in (3, 2):
                logs.append(log[: max(1, len(log) * (k + 1) // (frac * len(d["logs"])))])
        logs.append(d["logs"][0])
        docs.append(logs)
    # two replicas that each know ONE comment the other has not seen
    el = lambda i: "%d@a" % (i + 2)  # noqa: E731
    base = mini_doc([])
    ca = {"actor": "b", "seq": 1, "deps": {"a": 2}, "startOp": 8, "ops": [{"opId": "8@b", "obj": "1@a", "action": "addMark", "markType": "comment", "attrs": {"id": "A"},
                                                                             "start": {"type": "before", "elemId": el(0)}, "end": {"type": "after", "elemId": el(2)}}]}
    cb = {"actor": "c", "seq": 1, "deps": {"a": 2}, "startOp": 8, "ops": [{"opId": "8@c", "obj": "1@a", "action": "addMark", "markType": "comment", "attrs": {"id": "B"},
                                                                             "start": {"type": "before", "elemId": el(1)}, "end": {"type": "after", "elemId": el(4)}}]}
    docs.append([base + [ca], base + [cb], base + [ca, cb], base + [cb, ca]])
    return docs




def redeal_logs(logs, rng, n_logs):
    """n_logs random causally closed sub-logs (random linear extensions of the causal order) of the document whose replicas' logs are `logs`;
    logs that do not hold the makeList change (no text list yet) are left out."""
    by_key = {}
    for log in logs:
        for ch in log:
            by_key[(ch["actor"], ch["seq"])] = ch
    changes = list(by_key.values())
    out = []
    for _ in range(n_logs):
        want = rng.randint(1, len(changes))
        clock, log, pool = {}, [], list(changes)
        while len(log) < want:
            ready = [c for c in pool if c["seq"] == clock.get(c["actor"], 0) + 1 and all(clock.get(a, 0) >= s for a, s in c["deps"].items())]
            if not ready:
                break
            c = rng.choice(ready)
            pool.remove(c)
            clock[c["actor"]] = c["seq"]
            log.append(c)
        if any(op["action"] == "makeList" for ch in log for op in ch["ops"]):
            out.append(log)
    return out


def concurrent_marks_doc(n_chars, per_actor, seed):
    """One document: actor `a` types n_chars, then actors a, b, c — each knowing only that text — make per_actor random mark ops of all four types.  Returned:
    the three replicas' logs [a's order: own ops first, then b's, then c's], [c's ops, then b's, then a's: every later op has a SMALLER opId than many applied
    before it], and random causally closed interleavings."""
    import random

    rnd = random.Random(seed)
    ids = ["%d@a" % (2 + i) for i in range(n_chars)]
    ops = [{"opId": "1@a", "action": "makeList", "obj": "_root", "key": "text"}]
    for i in range(n_chars):
        ops.append({"opId": ids[i], "action": "set", "obj": "1@a", "elemId": "_head" if i == 0 else ids[i - 1], "insert": True, "value": "abcdefghij"[rnd.randrange(10)]})
    base = {"actor": "a", "seq": 1, "deps": {}, "startOp": 1, "ops": ops}
    chains = {}
    for actor in "abc":
        ctr, seq, chain = n_chars + 2, (2 if actor == "a" else 1), []
        for _ in range(per_actor):
            mt = ("strong", "em", "link", "comment")[rnd.randrange(4)]
            a = rnd.randrange(n_chars)
            e = a + 1 + rnd.randrange(n_chars - a)
            op = {"opId": "%d@%s" % (ctr, actor), "action": "addMark" if rnd.random() < 0.6 else "removeMark", "obj": "1@a", "start": {"type": "before", "elemId": ids[a]}, "markType": mt}
            if mt in ("strong", "em"):
                op["end"] = {"type": "endOfText"} if e >= n_chars else {"type": "before", "elemId": ids[e]}
            else:
                op["end"] = {"type": "after", "elemId": ids[e - 1]}
            if mt == "link" and op["action"] == "addMark":
                op["attrs"] = {"url": "%s.com" % "ABC"[rnd.randrange(3)]}
            if mt == "comment":
                op["attrs"] = {"id": "comment-%d" % rnd.randrange(6)}
            chain.append({"actor": actor, "seq": seq, "deps": {} if actor == "a" else {"a": 1}, "startOp": ctr, "ops": [op]})
            ctr += 1
            seq += 1
        chains[actor] = chain
    fwd = [base] + chains["a"] + chains["b"] + chains["c"]
    back = [base] + chains["c"] + chains["b"] + chains["a"]
    return [fwd, back] + redeal_logs([fwd], rnd, 4)


def concurrent_marks_docs():
    return [concurrent_marks_doc(40, 60, 1), concurrent_marks_doc(25, 120, 2)]


def more_deletes_than_inserts_docs():
    """Logs with more deletes than inserts + 1 (the same chars deleted again and again, which the reference allows,
    micromerge.ts:693): [all fine -> "!", a late delete whose target is only inserted by the NEXT op, a late delete of an unknown
    element].  The kernel resolves the first n + 1 deletes beside the inserts and the rest in a loop of their own."""
    el = lambda i: "%d@a" % (i + 2)  # noqa: E731
    dels = [{"action": "del", "elemId": el(i)} for i in range(5)] + [{"action": "del", "elemId": el(i)} for i in range(4)]
    ok = mini_doc(dels + [{"action": "set", "insert": True, "elemId": el(4), "value": "!"}])
    # ops of change 2 get ids 7, 8, ...: nine deletes (7..15), a delete of 17@a (16), the insert 17@a
    later = mini_doc(dels + [{"action": "del", "elemId": "17@a"}, {"action": "set", "insert": True, "elemId": el(4), "value": "!"}])
    unknown = mini_doc(dels + [{"action": "del", "elemId": "99@zz"}, {"action": "set", "insert": True, "elemId": el(4), "value": "!"}])
    return [[ok], [later], [unknown]]


def shift_counters(docs, delta):
    """The same documents with every op counter moved up by `delta` (opIds, element references, startOp): the histories stay
    valid, the id key space of the kernel's element index grows past 16 bits (its 32-bit key paths)."""
    def sid(x):
        if isinstance(x, str) and "@" in x:
            c, a = x.split("@", 1)
            return "%d@%s" % (int(c) + delta, a)
        return x

    def sop(op):
        o = dict(op)
        for k in ("opId", "obj", "elemId"):
            if k in o:
                o[k] = sid(o[k])
        for k in ("start", "end"):
            if k in o and "elemId" in o[k]:
                o[k] = dict(o[k], elemId=sid(o[k]["elemId"]))
        return o

    return [[[dict(c, startOp=c["startOp"] + delta, ops=[sop(o) for o in c["ops"]]) for c in log] for log in d] for d in docs]


def duplicate_op_docs():
    """[a log with one opId on two rows, a well-formed neighbour]."""
    dup = mini_doc([{"action": "set", "insert": True, "elemId": "6@a", "value": "x"}, {"action": "del", "elemId": "3@a"}])
    dup[1]["ops"][1]["opId"] = dup[1]["ops"][0]["opId"]
    ok = mini_doc([{"action": "set", "insert": True, "elemId": "6@a", "value": "x"}])
    return [[dup], [ok]]


def norm_patches(patches):
    return [json.loads(json.dumps(p, sort_keys=True)) for p in patches]


def check_patch_streams(batch, pat, expected_per_doc):
    log = 0
    for exp in expected_per_doc:
        for e in exp:
            got = norm_patches(wire.decode_patches(batch, pat, log))
            want = norm_patches(e["patches"])
            assert len(got) == len(want), "log %d: %d patches, expected %d" % (log, len(got), len(want))
            for i, (x, y) in enumerate(zip(got, want)):
                assert x == y, "log %d patch %d: %r != %r" % (log, i, x, y)
            log += 1
    return log


def accumulate_patches(patches):
    """reference/test/accumulatePatches.ts restated: replay a patch stream per character -> FormatSpanWithText[].
    One deliberate difference: the reference's checker handles `removeMark comment` by deleting the whole `comment`
    key (every id; its own fuzzer never removes comments, and the patch does not even carry the id).  Here the id comes
    from the op row behind the patch ("_commentId", wire.decode_patches(with_rows=True)) and only that id is removed,
    keeping the (possibly empty) list — what the replica itself holds (peritext.ts:318-320)."""
    chars = []
    for p in patches:
        a = p["action"]
        if a == "insert":
            for k, ch in enumerate(p["values"]):
                chars.insert(p["index"] + k, [ch, json.loads(json.dumps(p["marks"]))])
        elif a == "delete":
            del chars[p["index"]:p["index"] + p["count"]]
        elif a == "addMark":
            for i in range(p["startIndex"], p["endIndex"]):
                m = chars[i][1]
                if p["markType"] != "comment":
                    m[p["markType"]] = dict(p.get("attrs") or {"active": True})
                else:
                    cur = m.get("comment")
                    if cur is None:
                        m["comment"] = [dict(p["attrs"])]
                    elif not any(c["id"] == p["attrs"]["id"] for c in cur):
                        m["comment"] = sorted(cur + [dict(p["attrs"])], key=lambda c: c["id"])
        elif a == "removeMark":
            for i in range(p["startIndex"], p["endIndex"]):
                if p["markType"] == "comment":
                    chars[i][1]["comment"] = [c for c in chars[i][1].get("comment", []) if c["id"] != p["_commentId"]]
                else:
                    chars[i][1].pop(p["markType"], None)
    spans = []
    for ch, m in chars:
        if spans and spans[-1]["marks"] == m:
            spans[-1]["text"] += ch
        else:
            spans.append({"text": ch, "marks": json.loads(json.dumps(m))})
    return spans


def norm_spans(spans):
    """Order-insensitive form of FormatSpanWithText[] (deepStrictEqual ignores key order)."""
    return [{"text": s["text"], "marks": json.loads(json.dumps(s["marks"], sort_keys=True))} for s in spans]


def check_log(batch, res, log, expected):
    """One log of a result against the oracle's {spans, text}: decoded JSON, raw canonical arrays, digest."""
    r = res.logs[log]
    assert int(r["status"]) == 0, "log %d status %d" % (log, int(r["status"]))
    got = wire.decode_spans(batch, res, log)
    assert norm_spans(got) == norm_spans(expected["spans"]), "log %d spans differ" % log
    d = batch.log_doc[log]
    value_ix = {v: i for i, v in enumerate(batch.values)}
    url_ix = {u: i for i, u in enumerate(batch.urls)}
    crank = {c: i for i, c in enumerate(batch.doc_comments[d])}
    ev, es, ec = canon.canonical_from_spans(expected["spans"], expected["text"], value_ix, url_ix, crank)
    v, s, c = wire.canonical_of_log(batch, res, log)
    assert list(map(int, v)) == ev, "log %d values differ" % log
    assert [(int(x["start"]), int(x["attr"])) for x in s] == es, "log %d span rows differ" % log
    assert [(int(x["id"]), int(x["start"]), int(x["end"])) for x in c] == ec, "log %d comment intervals differ" % log
    h = canon.digest(ev, es, ec, int(r["n_elems"]))
    assert (int(r["digest"][0]), int(r["digest"][1])) == h, "log %d digest differs" % log


def check_generated(gen, res_fn):
    """Encode an oracle_gen() result, run `res_fn(batch)`, compare every replica log."""
    docs = [d["logs"] for d in gen["docs"]]
    batch = wire.encode_docs(docs)
    res = res_fn(batch)
    log = 0
    for d in gen["docs"]:
        for r, exp in enumerate(d["expected"]):
            check_log(batch, res, log, exp)
            log += 1
    return batch, res


def load_kat():
    with open(os.path.join(GOLDEN, "kat_reference_tests.json")) as f:
        return json.load(f)["cases"]


# ---- on-device change() / PTXGEN (peritext_amd/csrc/gen_core.h) through the host emulation ----
class _GenArgs(C.Structure):
    _fields_ = [("n_docs", C.c_uint32), ("first_doc", C.c_uint32), ("seed", C.c_uint32), ("R", C.c_uint32), ("ops_per_log", C.c_uint32),
                ("mix0", C.c_uint32), ("mix01", C.c_uint32), ("mix012", C.c_uint32), ("n_mark_types", C.c_uint32), ("mark_types", C.c_uint8 * 4),
                ("init_len", C.c_uint32), ("init_text", C.c_uint8 * 16), ("rows_per_log", C.c_uint32), ("list_cap", C.c_uint32), ("lds_bytes", C.c_uint32),
                ("op_id", C.c_void_p), ("ref_a", C.c_void_p), ("ref_b", C.c_void_p), ("payload", C.c_void_p), ("action", C.c_void_p),
                ("mark_type", C.c_void_p), ("side_a", C.c_void_p), ("side_b", C.c_void_p), ("chg_hdr", C.c_void_p), ("chg_env", C.c_void_p),
                ("n_changes", C.c_void_p), ("n_comments", C.c_void_p), ("status", C.c_void_p),
                ("ctab", C.c_void_p), ("known", C.c_void_p)]


def gen_config(name, ops=None, replicas=None):
    """The PTXGEN workload definitions as the generator's parameters (peritext_amd/workloads.py; oracle side: oracle/ptxgen.js CONFIGS)."""
    from peritext_amd import workloads

    return workloads.gen_config(name, ops=ops, replicas=replicas)


def batch_from_generated(cfg, n_docs, cols, env, n_changes, n_comments):
    """Assemble a wire.Batch from the generator's capacity-layout output (the envelope is compacted here)."""
    R, N = cfg["replicas"], cfg["ops_per_log"] + 1
    n_logs = n_docs * R
    log_off = (np.arange(n_logs + 1, dtype=np.uint64) * np.uint64(N)).astype(np.uint64)
    keep = np.concatenate([np.arange(l * N, l * N + int(n_changes[l])) for l in range(n_logs)]) if n_logs else np.zeros(0, dtype=np.int64)
    chg_off = np.zeros(n_logs + 1, dtype=np.uint64)
    chg_off[1:] = np.cumsum(n_changes.astype(np.uint64))
    actors, comments, log_doc = wire.generated_tables(n_docs, R, n_comments)
    return wire.Batch(log_off, cols["op_id"], cols["ref_a"], cols["ref_b"], cols["payload"], cols["action"], cols["mark_type"], cols["side_a"], cols["side_b"],
                      chg_off, env["chg_hdr"][keep], env["chg_env"].reshape(-1, abi.env_stride(R))[keep].reshape(-1), R,
                      None, wire.GEN_VALUES, wire.GEN_URLS, log_doc, actors, comments)


def emu_generate(cfg, n_docs, seed, first_doc=0, list_cap=None, reverse=0, lib_path=EMU_LIB):
    """PTXGEN documents made by the host emulation of gen_core.h (tests only): (wire.Batch, status per doc)."""
    R, N = cfg["replicas"], cfg["ops_per_log"] + 1
    rows = max(n_docs * R * N, 1)
    cols = {"op_id": np.zeros(rows, np.uint64), "ref_a": np.zeros(rows, np.uint64), "ref_b": np.zeros(rows, np.uint64), "payload": np.zeros(rows, np.uint32),
            "action": np.zeros(rows, np.uint8), "mark_type": np.zeros(rows, np.uint8), "side_a": np.zeros(rows, np.uint8), "side_b": np.zeros(rows, np.uint8)}
    env = {"chg_hdr": np.zeros(rows, np.uint32), "chg_env": np.zeros(rows * abi.env_stride(R), np.uint16)}
    n_changes = np.zeros(max(n_docs * R, 1), np.uint32)
    n_comments = np.zeros(max(n_docs, 1), np.uint32)
    status = np.zeros(max(n_docs, 1), np.uint32)
    a = _GenArgs()
    a.n_docs, a.first_doc, a.seed, a.R, a.ops_per_log = n_docs, first_doc, seed, R, cfg["ops_per_log"]
    m = cfg["mix"]
    a.mix0, a.mix01, a.mix012 = m[0], m[0] + m[1], m[0] + m[1] + m[2]
    a.n_mark_types = len(cfg["mark_types"])
    for i, t in enumerate(cfg["mark_types"]):
        a.mark_types[i] = t
    text = cfg.get("initial_text", "ABCDE")
    a.init_len = len(text)
    for i, ch in enumerate(text):
        a.init_text[i] = ord(ch)
    a.rows_per_log = N
    a.list_cap = list_cap or N + 8
    for k, v in list(cols.items()) + list(env.items()):
        setattr(a, k, v.ctypes.data)
    a.n_changes, a.n_comments, a.status = n_changes.ctypes.data, n_comments.ctypes.data, status.ctypes.data
    lib = C.CDLL(lib_path)
    lib.ptx_emu_generate.restype = C.c_int
    lib.ptx_emu_generate.argtypes = [C.POINTER(_GenArgs), C.c_int]
    assert lib.ptx_emu_generate(C.byref(a), reverse) == 0
    return batch_from_generated(cfg, n_docs, cols, env, n_changes[:n_docs * R], n_comments[:n_docs]), status[:n_docs]


def malformed_row_batches():
    """Logs of ptxgen_mini with ONE kind of malformed row each (VERDICT-style 'named error' cases for the row pass, which only flags
    such rows while it streams and names the first one in a second, rare pass): [(batch, {log: first bad row}, intact logs)].
    Batch A has no header (the library's census ignores rows of unknown action, so the malformed row is the only error);
    batch B keeps the encoder's header (op ids outside its bounds; a header that promises far fewer rows than the log has)."""
    import copy
    import json

    with open(os.path.join(GOLDEN, "ptxgen_mini.json")) as f:
        gen = json.load(f)
    base = wire.encode_docs([d["logs"] for d in gen["docs"]])
    out = []
    # A: action / mark type bytes
    a = copy.deepcopy(base)
    a.action = a.action.copy()
    a.mark_type = a.mark_type.copy()
    a.log_hdr = None
    want = {}

    def row_of(log, k, pred=None):
        lo, hi = int(a.log_off[log]), int(a.log_off[log + 1])
        rows = [r for r in range(lo + 1, hi) if pred is None or pred(r)]
        return rows[min(k, len(rows) - 1)] - lo, rows[min(k, len(rows) - 1)]

    is_mark = lambda r: int(base.action[r]) in (abi.ACT_ADDMARK, abi.ACT_REMOVEMARK)  # noqa: E731
    r, g = row_of(0, 17)
    a.action[g] = 8  # the first code beyond the table (6 / 7 are the map ops)
    want[0] = r
    r, g = row_of(1, 40)
    a.action[g] = 200
    want[1] = r
    r, g = row_of(2, 5, is_mark)
    a.mark_type[g] = 9
    want[2] = r
    r1, g1 = row_of(3, 60)
    r0, g0 = row_of(3, 11)
    a.action[g1] = 9
    a.action[g0] = 33
    want[3] = r0  # the FIRST of two
    out.append((a, want, [l for l in range(a.n_logs) if l not in want]))
    # B: op ids beyond the header's bounds, a header that understates the rows
    b = copy.deepcopy(base)
    b.op_id = b.op_id.copy()
    b.log_hdr = b.log_hdr.copy()
    want = {}
    lo = int(b.log_off[0])
    b.op_id[lo + 9] = np.uint64(int(b.op_id[lo + 9]) & 0xFFFFFFFF)  # counter 0
    want[0] = 9
    lo = int(b.log_off[1])
    b.op_id[lo + 30] = np.uint64((int(b.op_id[lo + 30]) & ~0xFFFFFFFF) | (int(b.log_hdr["max_actor"][1]) + 1))  # an actor the header does not know
    want[1] = 30
    lo = int(b.log_off[2])
    b.op_id[lo + 3] = np.uint64(((int(b.log_hdr["max_counter"][2]) + 5) << 32) | (int(b.op_id[lo + 3]) & 0xFFFFFFFF))  # a counter beyond the header's
    want[2] = 3
    b.log_hdr["n_ins"][3] = 0  # every insert of the log overflows its (empty) list: stores stay inside the log's window, the census rejects it
    b.log_hdr["n_del"][3] = 1
    want[3] = 0
    b.log_hdr["n_mark"][4] = [1, 0, 0, 0]
    want[4] = 0
    out.append((b, want, [l for l in range(b.n_logs) if l not in want]))
    return base, out


def check_malformed_rows(merge_fn):
    base, cases = malformed_row_batches()
    good = merge_fn(base)
    assert (good.logs["status"] == 0).all()
    for batch, want, intact in cases:
        res = merge_fn(batch)
        for log, row in want.items():
            assert int(res.logs["status"][log]) == abi.ERR_BAD_OP, (log, int(res.logs["status"][log]))
            # (a malformed row of a counted class also leaves the header's census one short: that is reported at row 0)
            assert int(res.logs["reserved"][log, 1]) in ((row,) if batch.log_hdr is None else (row, 0)), (log, int(res.logs["reserved"][log, 1]), row)
            assert int(res.logs["n_visible"][log]) == 0 and int(res.logs["n_spans"][log]) == 0
        for log in intact:
            assert int(res.logs["status"][log]) == 0
            assert (res.logs["digest"][log] == good.logs["digest"][log]).all()


# ---- map objects (getRoot): hand-written logs shared by the emulation suite and its GPU twin ----
def root_map_docs():
    """Documents whose changes write the root map and nested maps concurrently (micromerge.ts:572-602: last writer wins per key),
    every replica in another delivery order; plus logs the reference throws on (an op on a map that does not exist yet)."""
    def text_change(actor="a", text="ABC"):
        ops = [{"opId": "1@%s" % actor, "action": "makeList", "obj": "_root", "key": "text"}]
        prev = "_head"
        for i, ch in enumerate(text):
            ops.append({"opId": "%d@%s" % (i + 2, actor), "action": "set", "obj": "1@%s" % actor, "elemId": prev, "insert": True, "value": ch})
            prev = "%d@%s" % (i + 2, actor)
        return {"actor": actor, "seq": 1, "deps": {}, "startOp": 1, "ops": ops}

    a1 = text_change()
    a2 = {"actor": "a", "seq": 2, "deps": {"a": 1}, "startOp": 5, "ops": [
        {"opId": "5@a", "action": "set", "obj": "_root", "key": "title", "value": "A title"},
        {"opId": "6@a", "action": "makeMap", "obj": "_root", "key": "meta"},
        {"opId": "7@a", "action": "set", "obj": "6@a", "key": "lang", "value": "en"},
        {"opId": "8@a", "action": "set", "obj": "_root", "key": "count", "value": 1},
    ]}
    b1 = {"actor": "b", "seq": 1, "deps": {"a": 1}, "startOp": 5, "ops": [
        {"opId": "5@b", "action": "set", "obj": "_root", "key": "title", "value": "B title"},
        {"opId": "6@b", "action": "del", "obj": "_root", "key": "count"},
        {"opId": "7@b", "action": "makeMap", "obj": "_root", "key": "meta"},
        {"opId": "8@b", "action": "set", "obj": "7@b", "key": "lang", "value": "fr"},
        {"opId": "9@b", "action": "set", "obj": "_root", "key": "flag", "value": True},
    ]}
    c1 = {"actor": "c", "seq": 1, "deps": {"a": 2}, "startOp": 9, "ops": [
        {"opId": "9@c", "action": "set", "obj": "_root", "key": "title", "value": "C title \u00e9"},
        {"opId": "10@c", "action": "del", "obj": "_root", "key": "flag"},
        {"opId": "11@c", "action": "set", "obj": "6@a", "key": "extra", "value": None},
        {"opId": "12@c", "action": "makeList", "obj": "_root", "key": "notes"},
        {"opId": "13@c", "action": "set", "obj": "1@a", "elemId": "4@a", "insert": True, "value": "!"},
    ]}
    doc1 = [[a1, a2, b1, c1], [a1, b1, a2, c1], [a1, a2, c1, b1]]
    # nested maps three deep, a parent key deleted afterwards (its subtree is not reachable any more), keys re-set after a del
    d2 = {"actor": "a", "seq": 2, "deps": {"a": 1}, "startOp": 5, "ops": [
        {"opId": "5@a", "action": "makeMap", "obj": "_root", "key": "cfg"},
        {"opId": "6@a", "action": "makeMap", "obj": "5@a", "key": "ui"},
        {"opId": "7@a", "action": "makeMap", "obj": "6@a", "key": "theme"},
        {"opId": "8@a", "action": "set", "obj": "7@a", "key": "dark", "value": False},
        {"opId": "9@a", "action": "set", "obj": "5@a", "key": "version", "value": 3.5},
        {"opId": "10@a", "action": "del", "obj": "_root", "key": "gone"},
        {"opId": "11@a", "action": "set", "obj": "_root", "key": "gone", "value": "back"},
        {"opId": "12@a", "action": "set", "obj": "_root", "key": "nil", "value": None},
    ]}
    e1 = {"actor": "e", "seq": 1, "deps": {"a": 2}, "startOp": 13, "ops": [
        {"opId": "13@e", "action": "del", "obj": "5@a", "key": "ui"},
        {"opId": "14@e", "action": "set", "obj": "7@a", "key": "dark", "value": True},
        {"opId": "15@e", "action": "del", "obj": "_root", "key": "gone"},
    ]}
    doc2 = [[a1, d2, e1], [a1, d2]]
    # the reference throws: an op on a map that is only created later in this replica's order (its deps do not name the creator)
    early = {"actor": "z", "seq": 1, "deps": {"a": 1}, "startOp": 5, "ops": [
        {"opId": "5@z", "action": "set", "obj": "_root", "key": "ok", "value": 1},
        {"opId": "6@z", "action": "set", "obj": "6@a", "key": "lang", "value": "xx"},
    ]}
    ghost = {"actor": "g", "seq": 1, "deps": {"a": 1}, "startOp": 5, "ops": [{"opId": "5@g", "action": "del", "obj": "77@q", "key": "k"}]}
    doc3 = [[a1, early, a2], [a1, ghost], [a1, a2, early]]
    return [doc1, doc2, doc3]


def check_root_maps(root_fn, merge_fn, expected):
    """root_fn(batch) -> wire.RootMaps, merge_fn(batch) -> wire.Results; expected = oracle_apply(..., roots=True) of root_map_docs()."""
    docs = root_map_docs()
    batch = wire.encode_docs(docs)
    rm = root_fn(batch)
    res = merge_fn(batch)
    log = 0
    for d, exp in enumerate(expected):
        for e in exp:
            if e.get("error"):
                assert "Object does not exist" in e["error"], e["error"]
                assert int(rm.logs["status"][log]) == abi.ERR_ELEM_NOT_FOUND, (log, rm.logs[log])
                bad = int(rm.logs["first_bad_row"][log])
                b0 = int(batch.log_off[log])
                assert int(batch.action[b0 + bad]) in (abi.ACT_MAPSET, abi.ACT_MAPDEL)
            else:
                assert int(rm.logs["status"][log]) == 0, (log, rm.logs[log])
                assert wire.decode_root(batch, rm, log) == e["root"], (log, wire.decode_root(batch, rm, log), e["root"])
                check_log(batch, res, log, e)  # the text path does not see the map ops
            log += 1
    assert log == batch.n_logs
    return batch, rm


def emu_root_map(b, lds_bytes=64 * 1024, reverse=0, lib_path=EMU_LIB):
    """ptx_root_map on the host emulation (tests only)."""
    is_map = (b.action == abi.ACT_MAPSET) | (b.action == abi.ACT_MAPDEL) | (b.action == abi.ACT_MAKELIST)
    cum = np.concatenate([[0], np.cumsum(is_map.astype(np.int64))])
    counts = cum[b.log_off[1:].astype(np.int64)] - cum[b.log_off[:-1].astype(np.int64)]
    off = np.zeros(b.n_logs + 1, dtype=np.uint64)
    off[1:] = np.cumsum(counts)
    ent = np.zeros(max(int(off[-1]), 1), dtype=abi.ROOT_ENTRY_DTYPE)
    logs = np.zeros(max(b.n_logs, 1), dtype=abi.ROOT_LOG_DTYPE)
    s = batch_struct(b)
    lib = _emu(lib_path)
    lib.ptx_emu_root_map.restype = C.c_int
    lib.ptx_emu_root_map.argtypes = [C.POINTER(abi.ptx_batch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int]
    rc = lib.ptx_emu_root_map(C.byref(s), off.ctypes.data, ent.ctypes.data, logs.ctypes.data, lds_bytes, reverse)
    assert rc == 0
    return wire.RootMaps(entry_off=off, logs=logs[: b.n_logs], entries=ent[: int(off[-1])])


def root_map_change_calls():
    """change() calls with InputOperations on map objects (micromerge.ts:400-425) for the replicas of root_map_docs()[0:2] and of a
    document that shows the reference's order-dependent CHILDREN table (a makeMap registers its child only if it wins its key when it
    is applied; a later scalar winner leaves the entry alone): (docs, calls per log, actor per log)."""
    docs = root_map_docs()[:2]
    a1 = docs[0][0][0]
    mk = {"actor": "m", "seq": 1, "deps": {"a": 1}, "startOp": 5, "ops": [{"opId": "5@m", "action": "makeMap", "obj": "_root", "key": "cfgx"}]}
    st = {"actor": "s", "seq": 1, "deps": {"a": 1}, "startOp": 6, "ops": [{"opId": "6@s", "action": "set", "obj": "_root", "key": "cfgx", "value": 1}]}
    docs = docs + [[[a1, mk, st], [a1, st, mk]]]
    T = ["text"]
    mixed = [
        {"path": [], "action": "set", "key": "title", "value": "new title"},
        {"path": [], "action": "makeMap", "key": "fresh"},
        {"path": ["fresh"], "action": "set", "key": "n", "value": 7},
        {"path": ["meta"], "action": "set", "key": "lang", "value": "de"},
        {"path": T, "action": "insert", "index": 1, "values": ["x", "y"]},
        {"path": ["fresh"], "action": "makeMap", "key": "deep"},
        {"path": ["fresh", "deep"], "action": "del", "key": "nothing"},
        {"path": [], "action": "del", "key": "count"},
        {"path": [], "action": "makeList", "key": "todo"},
        {"path": T, "action": "addMark", "markType": "strong", "startIndex": 0, "endIndex": 2},
    ]
    nested = [
        {"path": ["cfg"], "action": "set", "key": "version", "value": 4},
        {"path": ["cfg", "ui"], "action": "set", "key": "zz", "value": True},  # doc 2, replica 0: `ui` was deleted, CHILDREN still knows it
        {"path": ["cfg", "ui", "theme"], "action": "del", "key": "dark"},
    ]
    through = [{"path": ["cfgx"], "action": "set", "key": "k", "value": None}]
    calls = [[mixed, [{"path": [], "action": "set", "key": "title", "value": "second call"}]], [mixed], [mixed], [nested], [nested], [through], [through]]
    actors = ["a", "b", "c", "a", "e", "m", "s"]
    return docs, calls, actors


def check_map_change_calls(change_fn, golden_change):
    """change_fn(batch, ops) -> (made wire.Batch, status per log); golden_change = rootmap_ref.json["change"] (made by the reference)."""
    import change_script as CS

    docs, calls, actors = root_map_change_calls()
    assert golden_change["docs"] == docs and golden_change["calls"] == calls and golden_change["actors"] == actors
    want = golden_change["made"]
    batch = wire.encode_docs(docs)
    ok = [("error" not in w) for w in want]
    # the reference's getObjectIdForPath throws where a path does not resolve: so does the host-side resolution
    for l, w in enumerate(want):
        if "error" in w:
            assert "Child not found" in w["error"]
            try:
                wire.encode_input_ops(batch, [calls[k] if k == l else [] for k in range(len(calls))], actors)
                raise AssertionError("log %d: the path should not resolve" % l)
            except ValueError as e:
                assert "Child not found" in str(e)
    ops = wire.encode_input_ops(batch, [calls[l] if ok[l] else [] for l in range(len(calls))], actors)
    made, status = change_fn(batch, ops)
    assert (status == 0).all(), status
    log = 0
    for logs in docs:
        for changes in logs:
            if ok[log]:
                got = wire.decode_changes(made, log, text_obj=CS.text_obj_of(changes))
                assert [CS.norm_change(c) for c in got] == [CS.norm_change(c) for c in want[log]["changes"]], (log, got, want[log]["changes"])
            log += 1
    return batch, made
