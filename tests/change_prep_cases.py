"""The preparation of change() from resident InputOperations (ptx_change_device; peritext_amd/csrc/change_prep_core.h): the cases tests/test_emu_change_prep.py
(CPU emulation) and tests/test_gpu_change_device.py (the C ABI on the GPU) share.

Expected values never come from the code under test.  The rows every log makes are helpers.rows_of_input_ops; the inserted values (grow) are a numpy sum; the
LDS need and the list words are the library's own ptx_change_lds_need / ptx_change_list_words of change_core.h — the two helpers ptx_change calls on the host —
called here through a shim the emulation library exports; the offsets are np.cumsum.  The verdict on bad arrays is ptx_change's list of checks restated in numpy:
the lowest (code, entry or log) in the order of change_prep_core.h's codes.

A case is a PrepCase: InputOperations (possibly invalid), the base batch's log_off and headers, and the sizes the resident object is made with.  The sizes are
what ptx_input_ops_upload reads off the arrays (chg_off[n_logs], op_off[n_changes]) unless the case gives its own, as a ptx_input_ops_wrap_device caller may.
Every array of an invalid case is at least as long as those sizes say, so that the host's ptx_change and the upload read nothing behind them."""
import ctypes as C
import dataclasses
import os

import numpy as np

import helpers as H
from peritext_amd import abi, wire

EMU_PREP_LIB = os.path.join(H.ROOT, "tests", "emu", "libperitext_emu_change_prep.so")
ROWS_MAX = abi.CHANGE_ROWS_MAX
MAX_LDS = 160 * 1024
# the codes of change_prep_core.h
CHG_START, CHG_ORDER, OP_START, OP_ORDER, SIZES, VALUES, ROWS = range(1, 8)
NO_ERROR = 0xFFFFFFFFFFFFFFFF


@dataclasses.dataclass
class PrepCase:
    name: str
    ops: wire.InputOps
    log_off: np.ndarray  # [n_logs + 1] of the base batch
    log_hdr: np.ndarray  # abi.LOG_HDR_DTYPE [n_logs]
    n_values: int = None  # None: len(ops.values)
    has_values: bool = True
    sizes: tuple = None  # (n_changes, n_input_ops) the object is made with; None: read off the arrays
    want_error: tuple = None  # hand-written (code, at) of an invalid case: what the case is there for

    @property
    def n_logs(self):
        return len(self.log_hdr)

    def values_count(self):
        return len(self.ops.values) if self.n_values is None else self.n_values

    def object_sizes(self):
        if self.sizes is not None:
            return self.sizes
        nc = int(self.ops.chg_off[self.n_logs]) if self.n_logs else 0
        return nc, (int(self.ops.op_off[nc]) if nc else 0)


class _Shim:
    lib = None

    @classmethod
    def get(cls):
        if cls.lib is None:
            lib = C.CDLL(EMU_PREP_LIB)
            lib.ptx_emu_change_lds_need.restype = C.c_uint64
            lib.ptx_emu_change_lds_need.argtypes = [C.c_uint64] * 4 + [C.c_int]
            lib.ptx_emu_change_list_words.restype = C.c_uint64
            lib.ptx_emu_change_list_words.argtypes = [C.c_uint64] * 2
            lib.ptx_emu_change_prep.restype = C.c_int
            lib.ptx_emu_change_prep.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6
            for f in ("ptx_emu_prep_abi_version", "ptx_emu_prep_rows_max", "ptx_emu_prep_log_hdr_bytes"):
                getattr(lib, f).restype = C.c_uint32
            cls.lib = lib
        return cls.lib


def lds_need(n, grow, ks, na, in_hbm=False):
    return int(_Shim.get().ptx_emu_change_lds_need(int(n), int(grow), int(ks), int(na), 1 if in_hbm else 0))


def list_words(n, grow):
    return int(_Shim.get().ptx_emu_change_list_words(int(n), int(grow)))


def expected_error(c):
    """ptx_change's checks of the arrays, all of them, as (code, at); the lowest, or None."""
    L, o = c.n_logs, c.ops
    if L == 0:
        return None
    nc, ni = c.object_sizes()
    errs = []

    def offsets(off, n, start, order, which):
        off = np.asarray(off[: n + 1], dtype=np.uint64)
        if int(off[0]) != 0:
            errs.append((start, 0))
        down = np.nonzero(off[1:] < off[:-1])[0]
        if len(down):
            errs.append((order, int(down[0]) + 1))
        if int(off[n]) != (nc if which == 0 else ni):
            errs.append((SIZES, which))

    offsets(o.chg_off, L, CHG_START, CHG_ORDER, 0)
    if nc:
        offsets(o.op_off, nc, OP_START, OP_ORDER, 1)
    if errs:
        return min(errs)
    rows, grow, bad = per_log(c)
    for l in range(L):
        if bad[l]:
            errs.append((VALUES, l))
        if int(rows[l]) > ROWS_MAX:
            errs.append((ROWS, l))
    return min(errs) if errs else None


def per_log(c):
    """(rows, grow, bad insert) per log of a case whose offsets are in order."""
    o, L = c.ops, c.n_logs
    ni = int(o.op_off[int(o.chg_off[L])]) if L and int(o.chg_off[L]) else 0
    cut = dataclasses.replace(o, action=o.action[:ni], count=o.count[:ni])
    cum_rows = H.rows_of_input_ops(cut) if L else np.zeros(1, np.uint64)
    rows = np.diff(cum_rows.astype(np.int64)) if L else np.zeros(0, np.int64)
    is_ins = o.action[:ni] == abi.IN_INSERT
    first = o.op_off[o.chg_off.astype(np.int64)].astype(np.int64) if L else np.zeros(1, np.int64)
    cum_grow = np.concatenate([[0], np.cumsum(np.where(is_ins, o.count[:ni], 0).astype(np.int64))])
    grow = cum_grow[first[1:]] - cum_grow[first[:-1]] if L else np.zeros(0, np.int64)
    wrong = is_ins & ((o.payload[:ni].astype(np.uint64) + o.count[:ni].astype(np.uint64) > np.uint64(c.values_count())) | ((o.count[:ni] > 0) & (not c.has_values)))
    cum_bad = np.concatenate([[0], np.cumsum(wrong.astype(np.int64))])
    bad = (cum_bad[first[1:]] - cum_bad[first[:-1]]) > 0 if L else np.zeros(0, bool)
    return rows, grow, bad


def expected(c, all_in_hbm=False, max_lds=MAX_LDS):
    """{"error": (code, at) or None, and for a valid case "rows", "list_words", "out_off", "list_off" and "need"}."""
    err = expected_error(c)
    if c.want_error is not None:
        assert err == c.want_error, (c.name, err)
    if err is not None or c.n_logs == 0:
        return {"error": err}
    L, o = c.n_logs, c.ops
    rows, grow, _ = per_log(c)
    words, need = np.zeros(L, np.int64), 0
    for l in range(L):
        if int(o.chg_off[l + 1]) == int(o.chg_off[l]):
            continue
        has_rows = int(c.log_off[l + 1]) > int(c.log_off[l])
        n = int(c.log_hdr["n_ins"][l]) if has_rows else 0
        ks = (int(c.log_hdr["max_counter"][l]) + 1) * (min(int(c.log_hdr["max_actor"][l]), 4095) + 1) if has_rows else 1
        in_hbm = all_in_hbm or lds_need(n, grow[l], ks, o.max_actors) > max_lds
        if in_hbm:
            words[l] = list_words(n, grow[l])
        need = max(need, lds_need(n, grow[l], ks, o.max_actors, in_hbm))
    cs = lambda v: np.concatenate([[0], np.cumsum(v)]).astype(np.uint64)  # noqa: E731
    return {"error": None, "rows": rows.astype(np.uint32), "list_words": words.astype(np.uint32), "out_off": cs(rows), "list_off": cs(words), "need": need}


class _In(C.Structure):
    _fields_ = [("chg_off", C.c_void_p), ("op_off", C.c_void_p), ("action", C.c_void_p), ("count", C.c_void_p), ("payload", C.c_void_p), ("n_changes", C.c_uint64),
                ("n_input_ops", C.c_uint64), ("n_values", C.c_uint64), ("has_values", C.c_uint32), ("n_logs", C.c_uint32), ("log_off", C.c_void_p), ("log_hdr", C.c_void_p),
                ("max_actors", C.c_uint32), ("all_in_hbm", C.c_uint32), ("max_lds", C.c_uint64)]


GUARD = 16  # words of 0xA5 on either side of every output


def emu_prep(c, reverse=0, all_in_hbm=False, max_lds=MAX_LDS):
    """The passes through the emulation: {"error", "rows", "list_words", "out_off", "list_off", "need"}.  The outputs are pre-filled with 0xA5 and guarded."""
    lib, L, o = _Shim.get(), c.n_logs, c.ops
    assert lib.ptx_emu_prep_log_hdr_bytes() == abi.LOG_HDR_DTYPE.itemsize
    nc, ni = c.object_sizes()
    keep = [np.ascontiguousarray(a) for a in (o.chg_off.astype(np.uint64), o.op_off.astype(np.uint64), o.action.astype(np.uint8), o.count.astype(np.uint32),
                                              o.payload.astype(np.uint32), np.asarray(c.log_off, np.uint64), np.asarray(c.log_hdr, abi.LOG_HDR_DTYPE))]
    assert len(keep[0]) >= L + 1 and len(keep[1]) >= nc + 1 and min(len(keep[2]), len(keep[3]), len(keep[4])) >= ni and len(keep[5]) >= L + 1
    s = _In()
    s.chg_off, s.op_off, s.action, s.count, s.payload, s.log_off, s.log_hdr = [a.ctypes.data for a in keep]
    s.n_changes, s.n_input_ops, s.n_values, s.has_values, s.n_logs = nc, ni, c.values_count(), 1 if c.has_values else 0, L
    s.max_actors, s.all_in_hbm, s.max_lds = o.max_actors, 1 if all_in_hbm else 0, max_lds

    def guarded(n, dtype):
        a = np.full(n + 2 * GUARD, 0xA5A5A5A5A5A5A5A5 if dtype == np.uint64 else 0xA5A5A5A5, dtype=dtype)
        return a, a[GUARD : GUARD + n]

    (g_rows, rows), (g_lw, lw), (g_oo, oo), (g_lo, lo) = guarded(L, np.uint32), guarded(L, np.uint32), guarded(L + 1, np.uint64), guarded(L + 1, np.uint64)
    err, need = C.c_uint64(0), C.c_uint64(0)
    assert lib.ptx_emu_change_prep(C.byref(s), reverse, rows.ctypes.data, lw.ctypes.data, oo.ctypes.data, lo.ctypes.data, C.byref(err), C.byref(need)) == 0
    for g, n in ((g_rows, L), (g_lw, L), (g_oo, L + 1), (g_lo, L + 1)):
        fill = g[0]
        assert (g[:GUARD] == fill).all() and (g[GUARD + n :] == fill).all(), "%s: a store outside an output" % c.name
    e = int(err.value)
    return {"error": None if e == NO_ERROR else (e >> 56, e & ((1 << 56) - 1)), "rows": rows.copy(), "list_words": lw.copy(), "out_off": oo.copy(), "list_off": lo.copy(),
            "need": int(need.value)}


# ---- builders ----
def _hdr(n_rows, n_ins):
    """Headers of a base batch whose log l has n_rows[l] rows, n_ins[l] of them inserts."""
    n_rows, n_ins = np.asarray(n_rows, np.int64), np.asarray(n_ins, np.int64)
    h = np.zeros(len(n_rows), dtype=abi.LOG_HDR_DTYPE)
    h["n_ins"], h["max_counter"], h["max_actor"] = n_ins, n_rows + 1, 1
    return np.concatenate([[0], np.cumsum(n_rows)]).astype(np.uint64), h


def make_ops(per_log, n_values, max_actors=2):
    """per_log[l] = the Changes of log l, each a list of (action, count, payload[, index, mark_type]); `values` is range(n_values)."""
    chg_off, op_off, rows = [0], [0], []
    for calls in per_log:
        for ops in calls:
            rows.extend(ops)
            op_off.append(len(rows))
        chg_off.append(len(op_off) - 1)
    col = lambda k, dt, default=0: np.array([r[k] if len(r) > k else default for r in rows], dtype=dt)  # noqa: E731
    return wire.InputOps(np.array(chg_off, np.uint64), np.array(op_off, np.uint64), col(0, np.uint8), col(4, np.uint8), col(3, np.uint32), col(1, np.uint32),
                         col(2, np.uint32), np.arange(n_values, dtype=np.uint32), np.zeros(len(per_log), np.uint32), max_actors)


def _rng_ops(rng, n, n_values):
    """n InputOperations of every action kind; the inserts stay inside `values`."""
    out = []
    for _ in range(n):
        a = int(rng.integers(0, 7))
        cnt = int(rng.integers(0, 5))
        out.append((a, cnt, int(rng.integers(0, n_values - cnt + 1)) if a == abi.IN_INSERT else int(rng.integers(0, 1000)), int(rng.integers(0, 50)), int(rng.integers(0, 4))))
    return out


def lane_edge_cases():
    """Logs of 0, 1, 63, 64, 65, 128 and 129 InputOperations beside idle logs; logs of 0 to 3 Changes, one of them without ops; every action kind."""
    rng = np.random.default_rng(811)
    out = []
    for n in (0, 1, 63, 64, 65, 128, 129):
        for n_chg in (1, 2, 3):
            ops = _rng_ops(rng, n, 40)
            cuts = sorted(int(x) for x in rng.integers(0, n + 1, size=n_chg - 1))
            calls = [ops[a:b] for a, b in zip([0] + cuts, cuts + [n])]
            if n_chg == 3:
                calls[1:1] = [[]]  # a Change without ops between the others
            per = [[], calls, [], [[(abi.IN_MAKELIST, 0, 0)]]]
            log_off, hdr = _hdr([7, 300, 0, 0], [3, 120, 0, 0])
            out.append(PrepCase("%d ops in %d Changes" % (n, len(calls)), make_ops(per, 40), log_off, hdr))
    kinds = [[(a, 3, 1, 2, 1) for a in range(7)]]  # every action once: 3 + 3 + 1 + 1 + 1 + 1 + 1 rows, the map rows counted as 1
    log_off, hdr = _hdr([9], [4])
    c = PrepCase("every action kind", make_ops([kinds], 10), log_off, hdr)
    assert per_log(c)[0].tolist() == [11] and per_log(c)[1].tolist() == [3]
    out.append(c)
    log_off, hdr = _hdr([], [])
    out.append(PrepCase("no logs", make_ops([], 0), log_off, hdr))
    log_off, hdr = _hdr([5, 0, 2], [2, 0, 1])
    out.append(PrepCase("no Changes", make_ops([[], [], []], 0), log_off, hdr))
    return out


def many_logs_case(L, seed=5, n_ins=6, n_rows=8):
    """L logs, most of them idle, for the scan's chunk edges.  Every busy log makes ONE op that a replica of n_ins visible elements accepts, so that the GPU
    test can run it: an insert of 1 to 3 values at 0 .. n_ins, a delete of 1 to n_ins elements at 0, or a mark over [0, 1]."""
    rng = np.random.default_rng(seed + L)
    per = []
    for l in range(L):
        if l not in (0, L - 1) and rng.integers(0, 40) != 0:
            per.append([])
            continue
        k = int(rng.integers(0, 3))
        if k == 0:
            cnt = int(rng.integers(1, 4))
            per.append([[(abi.IN_INSERT, cnt, int(rng.integers(0, 6 - cnt + 1)), int(rng.integers(0, n_ins + 1)), 0)]])
        elif k == 1:
            per.append([[(abi.IN_DELETE, int(rng.integers(1, n_ins + 1)), 0, 0, 0)]])
        else:
            per.append([[(abi.IN_ADDMARK, 1, 0, 0, abi.MARK_STRONG)]])
    log_off, hdr = _hdr([n_rows] * L, [n_ins] * L)
    return PrepCase("%d logs" % L, make_ops(per, 6), log_off, hdr)


MANY = (1, 1023, 1024, 1025, 2049)


def limit_cases():
    """(case, valid?) at the limits of rows and of `values`."""
    one = lambda name, op, nv, **kw: PrepCase(name, make_ops([[[op]]], nv), *_hdr([4], [2]), **kw)  # noqa: E731
    out = [one("65534 rows", (abi.IN_DELETE, 65534, 0), 0),
           one("65535 rows by one op", (abi.IN_DELETE, 65535, 0), 0, want_error=(ROWS, 0)),
           one("insert ends at n_values", (abi.IN_INSERT, 7, 3), 10),
           one("insert ends one behind n_values", (abi.IN_INSERT, 8, 3), 10, want_error=(VALUES, 0)),
           one("payload 0xFFFFFFFF, count 2", (abi.IN_INSERT, 2, 0xFFFFFFFF), 10, want_error=(VALUES, 0)),
           one("zero-count insert, values NULL", (abi.IN_INSERT, 0, 0), 0, has_values=False),
           one("insert, values NULL", (abi.IN_INSERT, 1, 0), 0, n_values=5, has_values=False, want_error=(VALUES, 0))]
    ops65 = [(abi.IN_DELETE, 1008, 0)] * 64
    log_off, hdr = _hdr([3, 3, 3], [1, 1, 1])
    out.append(PrepCase("65534 rows of 65 ops", make_ops([[], [ops65 + [(abi.IN_DELETE, 1022, 0)]], [ops65 + [(abi.IN_DELETE, 1008, 0)]]], 0), log_off, hdr))
    out.append(PrepCase("65535 rows, the last of 65 ops tips it", make_ops([[], [ops65 + [(abi.IN_DELETE, 1022, 0)]], [ops65 + [(abi.IN_DELETE, 1023, 0)]]], 0), log_off, hdr,
                        want_error=(ROWS, 2)))
    out.append(PrepCase("two logs over the limit", make_ops([[], [ops65 + [(abi.IN_DELETE, 1023, 0)]], [ops65 + [(abi.IN_DELETE, 1023, 0)]]], 0), log_off, hdr,
                        want_error=(ROWS, 1)))
    out.append(PrepCase("a bad insert below a log over the limit", make_ops([[[(abi.IN_INSERT, 1, 9)]], [ops65 + [(abi.IN_DELETE, 1023, 0)]], []], 9), log_off, hdr,
                        want_error=(VALUES, 0)))
    return out


OFFSET_LOGS = 600  # logs of the offsets cases: entries 255, 256, 257 and a last one far behind them


def _offsets_base():
    L = OFFSET_LOGS
    per = [[[(abi.IN_DELETE, 1, 0, 0, 0), (abi.IN_ADDMARK, 1, 0, 0, abi.MARK_STRONG)]] for _ in range(L)]  # one Change of two ops per log
    return make_ops(per, 4), _hdr([8] * L, [5] * L)


def offset_cases():
    """Invalid offsets.  An entry only ever becomes SMALLER than it was, so the arrays stay as long as the (smaller) sizes read off them say."""
    out, L = [], OFFSET_LOGS

    def case(name, which, edit, want):
        ops, (log_off, hdr) = _offsets_base()
        off = (ops.chg_off if which == 0 else ops.op_off).copy()
        edit(off)
        ops = dataclasses.replace(ops, chg_off=off) if which == 0 else dataclasses.replace(ops, op_off=off)
        out.append(PrepCase(name, ops, log_off, hdr, want_error=want))

    def bump0(off):
        off[0] = 1

    case("chg_off[0] != 0", 0, bump0, (CHG_START, 0))
    case("op_off[0] != 0", 1, bump0, (OP_START, 0))
    for which, nm, start, order in ((0, "chg_off", CHG_START, CHG_ORDER), (1, "op_off", OP_START, OP_ORDER)):

        def first(off):  # entry 1 below entry 0: entry 0 cannot be 0 then, and the start is what is reported
            off[0], off[1] = 2, 1

        case("%s decreases at entry 1" % nm, which, first, (start, 0))
        for at in (255, 256, 257, L):

            def down(off, at=at):
                off[at] = off[at - 1] - 1

            case("%s decreases at entry %d" % (nm, at), which, down, (order, at))

    def two(off):
        off[300] = off[299] - 1
        off[17] = off[16] - 1

    case("chg_off decreases twice: the lower entry is reported", 0, two, (CHG_ORDER, 17))
    case("op_off decreases twice: the lower entry is reported", 1, two, (OP_ORDER, 17))
    return out


def wrapped_size_cases():
    """Sizes that are a caller's word (ptx_input_ops_wrap_device) and do not agree with the arrays: refused, and nothing is read behind the columns."""
    ops, (log_off, hdr) = _offsets_base()
    nc, ni = OFFSET_LOGS, 2 * OFFSET_LOGS
    cut = dataclasses.replace(ops, action=ops.action[: ni - 1], count=ops.count[: ni - 1], payload=ops.payload[: ni - 1], index=ops.index[: ni - 1], mark_type=ops.mark_type[: ni - 1])
    return [PrepCase("n_input_ops one short of op_off's end", cut, log_off, hdr, sizes=(nc, ni - 1), want_error=(SIZES, 1)),
            PrepCase("n_changes one short of chg_off's end", ops, log_off, hdr, sizes=(nc - 1, int(ops.op_off[nc - 1])), want_error=(SIZES, 0))]


def invalid_cases():
    """The table of invalid inputs: every one is PTX_ERR_INVALID_ARG from ptx_change and from ptx_change_device."""
    return [c for c in limit_cases() if c.want_error] + offset_cases()
