"""Thin ctypes driver over the C ABI (include/peritext_hip.h).  Plumbing only: every merge goes
through libperitext_hip.so on a gfx950 device; nothing here computes a result on the CPU."""
import ctypes as C
import os

import numpy as np

from . import abi, wire


class PtxError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("peritext_hip status %d: %s" % (status, message))
        self.status = status


def _batch_struct(b):
    s = abi.ptx_batch()
    s.n_logs = b.n_logs
    s.n_ops = b.n_ops
    p = lambda a, t: a.ctypes.data_as(t)  # noqa: E731
    s.log_off = p(b.log_off, abi.u64p)
    s.op_id = p(b.op_id, abi.u64p)
    s.ref_a = p(b.ref_a, abi.u64p)
    s.ref_b = p(b.ref_b, abi.u64p)
    s.payload = p(b.payload, abi.u32p)
    s.action = p(b.action, abi.u8p)
    s.mark_type = p(b.mark_type, abi.u8p)
    s.side_a = p(b.side_a, abi.u8p)
    s.side_b = p(b.side_b, abi.u8p)
    if b.chg_off is not None:  # a batch without the Change envelope (e.g. downloaded from wrapped device columns): NULL = no admission
        s.chg_off = p(b.chg_off, abi.u64p)
        s.chg_hdr = p(b.chg_hdr, abi.u32p)
        s.chg_env = p(b.chg_env, abi.u16p)
        if b.chg_env_hi is not None:
            s.chg_env_hi = p(b.chg_env_hi, abi.u16p)
        s.max_actors = b.max_actors
    if b.log_hdr is not None and len(b.log_hdr):
        s.log_hdr = b.log_hdr.ctypes.data_as(C.POINTER(abi.ptx_log_hdr))
    return s


def _copy_result(res):
    """ptx_result (library-owned host memory, COMPACT rows since ABI 7) -> wire.Results (numpy copies)."""
    nl, nr = int(res.n_logs), int(res.n_rows)

    def arr(ptr, dtype, n):
        if n == 0:
            return np.zeros(0, dtype=dtype)
        buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(C.addressof(ptr.contents))
        return np.frombuffer(buf, dtype=dtype, count=n).copy()

    voff, soff, coff = (arr(p, np.uint64, nl + 1) if nl else np.zeros(1, dtype=np.uint64) for p in (res.value_off, res.span_off, res.cint_off))
    return wire.Results(
        logs=arr(res.logs, abi.LOG_RESULT_DTYPE, nl),
        values=arr(res.values, np.uint32, int(voff[nl])),
        spans=arr(res.spans, abi.SPAN_DTYPE, int(soff[nl])),
        cintervals=arr(res.cintervals, abi.CINTERVAL_DTYPE, int(coff[nl])),
        elem_rank=arr(res.elem_rank, np.uint32, nr) if res.elem_rank else np.zeros(0, dtype=np.uint32),
        value_off=voff,
        span_off=soff,
        cint_off=coff,
    )


def _copied(ptr, dtype, count):
    """A numpy copy of `count` items of a library-owned array (the library frees its own right after)."""
    if count == 0:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(count * np.dtype(dtype).itemsize,)).view(dtype).copy()


def _matches_of(m):
    n, arr = int(m.n_logs), _copied
    hit_off = arr(m.hit_off, np.uint64, n + 1)
    nh = int(hit_off[n])
    return wire.Matches(status=arr(m.status, np.uint32, n), n_matches=arr(m.n_matches, np.uint32, n), hit_off=hit_off, hit_unit=arr(m.hit_unit, np.uint32, nh),
                        hit_start=arr(m.hit_start, np.uint32, nh), hit_end=arr(m.hit_end, np.uint32, nh), n_pattern=int(m.n_pattern), kernel_ms=float(m.kernel_ms))


class TextView:
    """Engine.text_view's handle: the queries of a resident text view (include/peritext_hip.h "a resident text view")."""

    def __init__(self, engine, handle):
        self.engine, self.handle = engine, handle

    def _pattern(self, pattern):
        return np.frombuffer(pattern.encode("utf-16-le", "surrogatepass"), dtype="<u2").astype(np.uint16)

    def info(self):
        """{n_logs, first_log, n_units, n_prefix_words, bytes, kernel_ms} (ptx_view_info)."""
        d = abi.ptx_view_desc()
        self.engine._check(self.engine.lib.ptx_view_info(self.engine.ctx, self.handle, C.byref(d)))
        return {"n_logs": int(d.n_logs), "first_log": int(d.first_log), "n_units": int(d.n_units), "n_prefix_words": int(d.n_prefix_words), "bytes": int(d.bytes),
                "kernel_ms": float(d.kernel_ms)}

    def find_text(self, pattern, ascii_nocase=False, max_hits_per_log=0xFFFFFFFF):
        """Engine.find_text over the view's range (ptx_view_find_text): the same wire.Matches."""
        eng, pat = self.engine, self._pattern(pattern)
        m = abi.ptx_matches()
        eng._check(eng.lib.ptx_view_find_text(eng.ctx, self.handle, pat.ctypes.data_as(abi.u16p), len(pat), abi.FIND_ASCII_NOCASE if ascii_nocase else 0, max_hits_per_log, C.byref(m)))
        try:
            return _matches_of(m)
        finally:
            eng.lib.ptx_matches_free(C.byref(m))

    def text_slices(self, slices):
        """Engine.text_slices over the view's range (ptx_view_text_slices): the same wire.Slices."""
        n_logs = self.info()["n_logs"]
        if len(slices) != n_logs:
            raise ValueError("slices holds %d lists for %d logs" % (len(slices), n_logs))
        off = np.zeros(n_logs + 1, dtype=np.uint64)
        if n_logs:
            off[1:] = np.cumsum([len(s) for s in slices], dtype=np.uint64)
        flat = np.array([p for s in slices for p in s], dtype=np.uint32).reshape(-1, 2)
        return self.text_slices_flat(off, np.ascontiguousarray(flat[:, 0]), np.ascontiguousarray(flat[:, 1]))

    def text_slices_flat(self, slice_off, slice_start, slice_end):
        """text_slices with the C ABI's own arrays (numpy; None passes NULL)."""
        eng = self.engine
        ptr = lambda a, t: a.ctypes.data_as(t) if a is not None and len(a) else C.cast(None, t)  # noqa: E731
        m = abi.ptx_slices()
        eng._check(eng.lib.ptx_view_text_slices(eng.ctx, self.handle, ptr(slice_off, abi.u64p), ptr(slice_start, abi.u32p), ptr(slice_end, abi.u32p), C.byref(m)))
        try:
            n, k, arr = int(m.n_logs), int(m.n_slices), _copied
            unit_off, sspan_off = arr(m.unit_off, np.uint64, k + 1), arr(m.sspan_off, np.uint64, k + 1)
            nr = int(sspan_off[k])
            return wire.Slices(status=arr(m.status, np.uint32, n), slice_off=np.array(slice_off, dtype=np.uint64) if n else np.zeros(1, np.uint64),
                               elem_start=arr(m.elem_start, np.uint32, k), elem_end=arr(m.elem_end, np.uint32, k), unit_off=unit_off,
                               text=arr(m.text, np.uint16, int(unit_off[k])), sspan_off=sspan_off, sspans=arr(m.sspans, abi.SPAN_DTYPE, nr),
                               sspan_unit=arr(m.sspan_unit, np.uint32, nr), kernel_ms=float(m.kernel_ms))
        finally:
            eng.lib.ptx_slices_free(C.byref(m))

    def find_snippets(self, pattern, before=0, after=0, ascii_nocase=False, max_hits_per_log=0xFFFFFFFF):
        """find_text, and for every listed hit the text and the span rows of the elements [hit_start - before, hit_end + after) with the match's offset inside
        that text, in one call that keeps the hits on the device (ptx_view_find_snippets): wire.Snippets."""
        eng, pat = self.engine, self._pattern(pattern)
        m = abi.ptx_snippets()
        eng._check(eng.lib.ptx_view_find_snippets(eng.ctx, self.handle, pat.ctypes.data_as(abi.u16p), len(pat), abi.FIND_ASCII_NOCASE if ascii_nocase else 0, max_hits_per_log,
                                                  before, after, C.byref(m)))
        try:
            n, k, arr = int(m.n_logs), int(m.n_slices), _copied
            unit_off, sspan_off = arr(m.unit_off, np.uint64, k + 1), arr(m.sspan_off, np.uint64, k + 1)
            nr = int(sspan_off[k])
            return wire.Snippets(status=arr(m.status, np.uint32, n), slice_off=arr(m.hit_off, np.uint64, n + 1), elem_start=arr(m.elem_start, np.uint32, k),
                                 elem_end=arr(m.elem_end, np.uint32, k), unit_off=unit_off, text=arr(m.text, np.uint16, int(unit_off[k])), sspan_off=sspan_off,
                                 sspans=arr(m.sspans, abi.SPAN_DTYPE, nr), sspan_unit=arr(m.sspan_unit, np.uint32, nr), kernel_ms=float(m.kernel_ms),
                                 n_matches=arr(m.n_matches, np.uint32, n), hit_unit=arr(m.hit_unit, np.uint32, k), hit_start=arr(m.hit_start, np.uint32, k),
                                 hit_end=arr(m.hit_end, np.uint32, k), match_unit=arr(m.match_unit, np.uint32, k), n_pattern=int(m.n_pattern))
        finally:
            eng.lib.ptx_snippets_free(C.byref(m))

    def mark_runs(self, mark_type, id=abi.MARK_ANY_ID, max_runs_per_log=0xFFFFFFFF):
        """The runs of a mark, chosen on the device (ptx_view_mark_runs): maximal sequences of span rows with the strong / em flag or the same link url, or the
        comment intervals of one id (abi.MARK_ANY_ID: any url, every comment): wire.MarkRuns."""
        eng = self.engine
        m = abi.ptx_mark_runs()
        eng._check(eng.lib.ptx_view_mark_runs(eng.ctx, self.handle, mark_type, id, max_runs_per_log, C.byref(m)))
        try:
            n, arr = int(m.n_logs), _copied
            run_off = arr(m.run_off, np.uint64, n + 1)
            k = int(run_off[n])
            return wire.MarkRuns(status=arr(m.status, np.uint32, n), n_runs=arr(m.n_runs, np.uint32, n), run_off=run_off, run_start=arr(m.run_start, np.uint32, k),
                                 run_end=arr(m.run_end, np.uint32, k), run_id=arr(m.run_id, np.uint32, k), run_unit=arr(m.run_unit, np.uint32, k),
                                 run_len=arr(m.run_len, np.uint32, k), mark_type=int(m.mark_type), kernel_ms=float(m.kernel_ms))
        finally:
            eng.lib.ptx_mark_runs_free(C.byref(m))

    def mark_snippets(self, mark_type, id=abi.MARK_ANY_ID, before=0, after=0, max_runs_per_log=0xFFFFFFFF):
        """mark_runs, and for every listed run the text and the span rows of the elements [run_start - before, run_end + after) in one call that keeps the runs
        on the device (ptx_view_mark_snippets): wire.MarkSnippets.  before == after == 0: the text each run covers."""
        eng = self.engine
        m = abi.ptx_mark_snippets()
        eng._check(eng.lib.ptx_view_mark_snippets(eng.ctx, self.handle, mark_type, id, max_runs_per_log, before, after, C.byref(m)))
        try:
            n, k, arr = int(m.n_logs), int(m.n_slices), _copied
            unit_off, sspan_off = arr(m.unit_off, np.uint64, k + 1), arr(m.sspan_off, np.uint64, k + 1)
            nr = int(sspan_off[k])
            return wire.MarkSnippets(status=arr(m.status, np.uint32, n), slice_off=arr(m.run_off, np.uint64, n + 1), elem_start=arr(m.elem_start, np.uint32, k),
                                     elem_end=arr(m.elem_end, np.uint32, k), unit_off=unit_off, text=arr(m.text, np.uint16, int(unit_off[k])), sspan_off=sspan_off,
                                     sspans=arr(m.sspans, abi.SPAN_DTYPE, nr), sspan_unit=arr(m.sspan_unit, np.uint32, nr), kernel_ms=float(m.kernel_ms),
                                     n_runs=arr(m.n_runs, np.uint32, n), run_start=arr(m.run_start, np.uint32, k), run_end=arr(m.run_end, np.uint32, k),
                                     run_id=arr(m.run_id, np.uint32, k), run_unit=arr(m.run_unit, np.uint32, k), run_len=arr(m.run_len, np.uint32, k),
                                     match_unit=arr(m.match_unit, np.uint32, k), mark_type=int(m.mark_type))
        finally:
            eng.lib.ptx_mark_snippets_free(C.byref(m))

    def find_in_marks(self, pattern, mark_type, id=abi.MARK_ANY_ID, ascii_nocase=False, max_hits_per_log=0xFFFFFFFF):
        """find_text restricted to the hits whose elements lie inside ONE run of the selector, filtered on the device (ptx_view_find_in_marks): wire.Matches whose
        n_matches counts the contained hits.  A comment selector needs one id."""
        eng, pat = self.engine, self._pattern(pattern)
        m = abi.ptx_matches()
        eng._check(eng.lib.ptx_view_find_in_marks(eng.ctx, self.handle, pat.ctypes.data_as(abi.u16p), len(pat), abi.FIND_ASCII_NOCASE if ascii_nocase else 0, mark_type, id,
                                                  max_hits_per_log, C.byref(m)))
        try:
            return _matches_of(m)
        finally:
            eng.lib.ptx_matches_free(C.byref(m))

    def replace_plan(self, pattern, replacement_ids, n_batch_logs, ascii_nocase=False):
        """replaceAll as change() input (ptx_view_replace_plan): per log the matches str.replace would replace — greedy, leftmost, non-overlapping — and, for those
        that cover whole elements, a delete and an insert of the value ids `replacement_ids` (one element each) per match, in descending order, as ONE Change
        per log: wire.ReplacePlan, its `ops` shaped for a batch of n_batch_logs logs."""
        eng, pat = self.engine, self._pattern(pattern)
        ids = np.ascontiguousarray(replacement_ids, dtype=np.uint32)
        m = abi.ptx_replace_plan()
        eng._check(eng.lib.ptx_view_replace_plan(eng.ctx, self.handle, pat.ctypes.data_as(abi.u16p), len(pat), abi.FIND_ASCII_NOCASE if ascii_nocase else 0,
                                                 ids.ctypes.data_as(abi.u32p) if len(ids) else C.cast(None, abi.u32p), len(ids), n_batch_logs, C.byref(m)))
        try:
            n, nb, arr, o = int(m.n_logs), int(m.ops.n_logs), _copied, m.ops
            chg_off = arr(o.chg_off, np.uint64, nb + 1)
            op_off = arr(o.op_off, np.uint64, int(chg_off[nb]) + 1)
            ni = int(op_off[-1])
            ops = wire.InputOps(chg_off, op_off, arr(o.action, np.uint8, ni), arr(o.mark_type, np.uint8, ni), arr(o.index, np.uint32, ni), arr(o.count, np.uint32, ni),
                                arr(o.payload, np.uint32, ni), arr(o.values, np.uint32, int(o.n_values)), None, int(o.max_actors))
            return wire.ReplacePlan(status=arr(m.status, np.uint32, n), n_matches=arr(m.n_matches, np.uint32, n), n_chosen=arr(m.n_chosen, np.uint32, n),
                                    n_replaced=arr(m.n_replaced, np.uint32, n), ops=ops, first_log=self.info()["first_log"], n_pattern=int(m.n_pattern),
                                    n_replacement=int(m.n_replacement), kernel_ms=float(m.kernel_ms))
        finally:
            eng.lib.ptx_replace_plan_free(C.byref(m))

    def replace_plan_device(self, pattern, replacement_ids, n_batch_logs, actor, max_actors, ascii_nocase=False):
        """replace_plan with the InputOperations left on the device (ptx_view_replace_plan_device): (wire.ReplacePlan with the per-log counts and ops=None, handle
        of the resident ops — made for Engine.change_device, freed with Engine.free_input_ops).  actor[l] = actorRank of the replica behind log l of the batch."""
        eng, pat = self.engine, self._pattern(pattern)
        ids = np.ascontiguousarray(replacement_ids, dtype=np.uint32)
        act = None if actor is None else np.ascontiguousarray(actor, dtype=np.uint32)
        if act is not None and len(act) != n_batch_logs:
            raise ValueError("actor must name every log of the batch")
        m, h = abi.ptx_replace_plan(), C.c_void_p()
        eng._check(eng.lib.ptx_view_replace_plan_device(eng.ctx, self.handle, pat.ctypes.data_as(abi.u16p), len(pat), abi.FIND_ASCII_NOCASE if ascii_nocase else 0,
                                                        ids.ctypes.data_as(abi.u32p) if len(ids) else C.cast(None, abi.u32p), len(ids), n_batch_logs,
                                                        act.ctypes.data_as(abi.u32p) if act is not None and len(act) else C.cast(None, abi.u32p), max_actors, C.byref(m), C.byref(h)))
        try:
            n, arr = int(m.n_logs), _copied
            return wire.ReplacePlan(status=arr(m.status, np.uint32, n), n_matches=arr(m.n_matches, np.uint32, n), n_chosen=arr(m.n_chosen, np.uint32, n),
                                    n_replaced=arr(m.n_replaced, np.uint32, n), ops=None, first_log=self.info()["first_log"], n_pattern=int(m.n_pattern),
                                    n_replacement=int(m.n_replacement), kernel_ms=float(m.kernel_ms)), h
        finally:
            eng.lib.ptx_replace_plan_free(C.byref(m))

    def free(self):
        if self.handle is not None:
            self.engine.lib.ptx_text_view_free(self.engine.ctx, self.handle)
            self.handle = None


class Engine:
    """One device context (one HIP stream).  One Engine per process/GPU in multi-GPU runs."""

    def __init__(self, device=0, lib_path=None, flags=0):
        self.lib = abi.load_library(lib_path)
        ctx = C.c_void_p()
        st = self.lib.ptx_create(device, flags, C.byref(ctx))
        if st != 0:
            raise PtxError(st, (self.lib.ptx_last_error(None) or b"").decode())
        self.ctx = ctx
        self.device = device

    def _check(self, st):
        if st != 0:
            raise PtxError(st, (self.lib.ptx_last_error(self.ctx) or b"").decode())

    def set_launch_shape(self, threads_per_log=0, lds_bytes_per_log=0):
        """Threads per log / LDS window per log of the batches made resident after this call (0 = the library's choice)."""
        self._check(self.lib.ptx_set_launch_shape(self.ctx, threads_per_log, lds_bytes_per_log))

    def close(self):
        if self.ctx:
            self.lib.ptx_destroy(self.ctx)
            self.ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- the drop-in call ----
    def apply_materialize(self, batch):
        """Upload, merge, download: wire.Batch -> wire.Results (ptx_apply_materialize)."""
        s = _batch_struct(batch)
        res = abi.ptx_result()
        self._check(self.lib.ptx_apply_materialize(self.ctx, C.byref(s), C.byref(res)))
        try:
            return _copy_result(res)
        finally:
            self.lib.ptx_result_free(C.byref(res))

    # ---- staged form ----
    def upload(self, batch, copies=1):
        s = _batch_struct(batch)
        h = C.c_void_p()
        self._check(self.lib.ptx_batch_upload_tiled(self.ctx, C.byref(s), copies, C.byref(h)))
        return h

    def wrap_device(self, n_logs, n_ops, ptrs, log_hdr_ptr=0):
        """Adopt caller-owned DEVICE columns (ptx_batch_wrap_device): `ptrs` maps the nine column names of
        ptx_batch (log_off, op_id, ref_a, ref_b, payload, action, mark_type, side_a, side_b) to device addresses,
        e.g. torch tensors' data_ptr().  Nothing is copied; the log headers are computed on the device unless
        `log_hdr_ptr` (device address of n_logs ptx_log_hdr rows) is given."""
        s = abi.ptx_batch()
        s.n_logs = n_logs
        s.n_ops = n_ops
        for name, typ in (("log_off", abi.u64p), ("op_id", abi.u64p), ("ref_a", abi.u64p), ("ref_b", abi.u64p), ("payload", abi.u32p),
                          ("action", abi.u8p), ("mark_type", abi.u8p), ("side_a", abi.u8p), ("side_b", abi.u8p)):
            setattr(s, name, C.cast(C.c_void_p(int(ptrs[name])), typ))
        if log_hdr_ptr:
            s.log_hdr = C.cast(C.c_void_p(int(log_hdr_ptr)), C.POINTER(abi.ptx_log_hdr))
        h = C.c_void_p()
        self._check(self.lib.ptx_batch_wrap_device(self.ctx, C.byref(s), C.byref(h)))
        return h

    def append(self, dbatch, more):
        """Streaming append: a new resident batch whose log l = log l of `dbatch` + log l of the wire.Batch `more`."""
        s = _batch_struct(more)
        h = C.c_void_p()
        self._check(self.lib.ptx_batch_append(self.ctx, dbatch, C.byref(s), C.byref(h)))
        return h

    def resolve_cursors(self, dbatch, dresult, q_log, q_kind, q_arg):
        """Micromerge.resolveCursor / getCursor (micromerge.ts:465-477) for many replicas on the device (ptx_resolve_cursors):
        query q = (log, abi.CURSOR_RESOLVE, elemId as counter << 32 | actorRank) -> visible index, or (log, abi.CURSOR_GET, visible
        index) -> elemId.  Returns (out u64[n], status u32[n])."""
        ql = np.ascontiguousarray(q_log, dtype=np.uint32)
        qk = np.ascontiguousarray(q_kind, dtype=np.uint8)
        qa = np.ascontiguousarray(q_arg, dtype=np.uint64)
        n = len(ql)
        out = np.zeros(max(n, 1), dtype=np.uint64)
        status = np.zeros(max(n, 1), dtype=np.uint32)
        self._check(self.lib.ptx_resolve_cursors(self.ctx, dbatch, dresult, n, ql.ctypes.data_as(abi.u32p), qk.ctypes.data_as(abi.u8p), qa.ctypes.data_as(abi.u64p),
                                                 out.ctypes.data_as(abi.u64p), status.ctypes.data_as(abi.u32p)))
        return out[:n], status[:n]

    def append_device(self, dbatch, more_dbatch):
        """The same with `more` already resident (e.g. the batch Engine.change made)."""
        h = C.c_void_p()
        self._check(self.lib.ptx_batch_append_device(self.ctx, dbatch, more_dbatch, C.byref(h)))
        return h

    def change(self, dbatch, dresult, ops):
        """Micromerge.change for many replicas at once (ptx_change): `ops` = wire.InputOps (index-based InputOperations per
        log, grouped into the Changes to make) resolved against the replica states `dresult` = merge of `dbatch` holds.
        Returns (resident batch of the new Changes only, status per log as a numpy array)."""
        s = abi.ptx_input_ops()
        s.n_logs, s.max_actors = len(ops.chg_off) - 1, ops.max_actors
        p = lambda a, t: a.ctypes.data_as(t)  # noqa: E731
        s.chg_off, s.op_off = p(ops.chg_off, abi.u64p), p(ops.op_off, abi.u64p)
        s.action, s.mark_type = p(ops.action, abi.u8p), p(ops.mark_type, abi.u8p)
        s.index, s.count, s.payload = p(ops.index, abi.u32p), p(ops.count, abi.u32p), p(ops.payload, abi.u32p)
        s.values, s.n_values, s.actor = p(ops.values, abi.u32p), len(ops.values), p(ops.actor, abi.u32p)
        status = np.zeros(max(s.n_logs, 1), dtype=np.uint32)
        h = C.c_void_p()
        self._check(self.lib.ptx_change(self.ctx, dbatch, dresult, C.byref(s), C.byref(h), status.ctypes.data_as(abi.u32p)))
        return h, status[: s.n_logs]

    @staticmethod
    def _input_ops_struct(ops):
        s = abi.ptx_input_ops()
        s.n_logs, s.max_actors = len(ops.chg_off) - 1, ops.max_actors
        p = lambda a, t: a.ctypes.data_as(t) if a is not None else C.cast(None, t)  # noqa: E731
        s.chg_off, s.op_off = p(ops.chg_off, abi.u64p), p(ops.op_off, abi.u64p)
        s.action, s.mark_type = p(ops.action, abi.u8p), p(ops.mark_type, abi.u8p)
        s.index, s.count, s.payload = p(ops.index, abi.u32p), p(ops.count, abi.u32p), p(ops.payload, abi.u32p)
        s.values, s.n_values, s.actor = p(ops.values, abi.u32p), 0 if ops.values is None else len(ops.values), p(ops.actor, abi.u32p)
        return s

    def upload_input_ops(self, ops):
        """wire.InputOps made resident (ptx_input_ops_upload): a handle for change_device, freed with free_input_ops.  Only the sizes are read here; what
        Engine.change checks of the arrays on the host, change_device checks on the device."""
        s, h = self._input_ops_struct(ops), C.c_void_p()
        self._check(self.lib.ptx_input_ops_upload(self.ctx, C.byref(s), C.byref(h)))
        return h

    def wrap_input_ops(self, n_logs, n_changes, n_input_ops, n_values, max_actors, ptrs):
        """Adopt caller-owned DEVICE columns as InputOperations (ptx_input_ops_wrap_device): `ptrs` maps the nine array names of ptx_input_ops (chg_off, op_off,
        action, mark_type, index, count, payload, values, actor) to device addresses, e.g. torch tensors' data_ptr(); a missing name is NULL.  Nothing is
        copied: the memory must outlive the handle and every call that takes it."""
        s = abi.ptx_input_ops()
        s.n_logs, s.max_actors, s.n_values = n_logs, max_actors, n_values
        for name, typ in (("chg_off", abi.u64p), ("op_off", abi.u64p), ("action", abi.u8p), ("mark_type", abi.u8p), ("index", abi.u32p), ("count", abi.u32p),
                          ("payload", abi.u32p), ("values", abi.u32p), ("actor", abi.u32p)):
            setattr(s, name, C.cast(C.c_void_p(int(ptrs.get(name) or 0) or None), typ))
        h = C.c_void_p()
        self._check(self.lib.ptx_input_ops_wrap_device(self.ctx, C.byref(s), n_changes, n_input_ops, C.byref(h)))
        return h

    def download_input_ops(self, h):
        """Resident InputOperations back on the host (ptx_input_ops_download): wire.InputOps."""
        m = abi.ptx_host_input_ops()
        self._check(self.lib.ptx_input_ops_download(self.ctx, h, C.byref(m)))
        try:
            o, arr, nl, nc, ni = m.ops, _copied, int(m.ops.n_logs), int(m.n_changes), int(m.n_input_ops)
            return wire.InputOps(arr(o.chg_off, np.uint64, nl + 1 if o.chg_off else 0), arr(o.op_off, np.uint64, nc + 1 if o.op_off else 0), arr(o.action, np.uint8, ni),
                                 arr(o.mark_type, np.uint8, ni), arr(o.index, np.uint32, ni), arr(o.count, np.uint32, ni), arr(o.payload, np.uint32, ni),
                                 arr(o.values, np.uint32, int(o.n_values) if o.values else 0), arr(o.actor, np.uint32, nl), int(o.max_actors))
        finally:
            self.lib.ptx_host_input_ops_free(C.byref(m))

    def free_input_ops(self, h):
        self.lib.ptx_input_ops_free(self.ctx, h)

    def change_device(self, dbatch, dresult, h):
        """Engine.change for InputOperations that are resident (ptx_change_device): the same Changes and the same status; the rows every log makes, the checks
        of the arrays and the launch's size are worked out on the device.  Returns (resident batch of the new Changes only, status per log)."""
        n = int(self.lib.ptx_batch_n_logs(dbatch))
        status = np.zeros(max(n, 1), dtype=np.uint32)
        made = C.c_void_p()
        self._check(self.lib.ptx_change_device(self.ctx, dbatch, dresult, h, C.byref(made), status.ctypes.data_as(abi.u32p)))
        return made, status[:n]

    def replace_text_resident(self, dbatch, dresult, view, batch, pattern, replacement_values, actors, ascii_nocase=False):
        """replace_text without the InputOperations leaving the device: TextView.replace_plan_device and change_device.  The same arguments and the same return,
        the wire.ReplacePlan carrying the per-log counts and no ops."""
        value_ix = {v: i for i, v in enumerate(batch.values)}
        ids = []
        for v in replacement_values:
            if not isinstance(v, str):
                raise ValueError("Expected value inserted into text to be a string")
            if v not in value_ix:
                value_ix[v] = len(batch.values)
                batch.values.append(v)
            ids.append(value_ix[v])
        actor = np.asarray([batch.doc_actors[batch.log_doc[l]].index(actors[l]) for l in range(batch.n_logs)], dtype=np.uint32)
        max_actors = max(batch.max_actors, max((len(a) for a in batch.doc_actors), default=1))
        plan, h = view.replace_plan_device(pattern, ids, batch.n_logs, actor, max_actors, ascii_nocase=ascii_nocase)
        try:
            made, status = self.change_device(dbatch, dresult, h)
        finally:
            self.free_input_ops(h)
        return made, status, plan

    def replace_text(self, dbatch, dresult, view, batch, pattern, replacement_values, actors, ascii_nocase=False):
        """Replace all on many replicas at once: TextView.replace_plan of `view` (a view of `dresult` = merge of `dbatch`, WITH elem_rank) made into Changes by
        ptx_change.  replacement_values: the replacement's element strings (an editor passes list(text): bridge.ts:445), interned into batch.values as
        wire.encode_input_ops does — upload the strings again before the next text query; actors[l] = the actor id of the replica behind log l of `batch`.
        Returns (resident batch of the new Changes only, status per log of the batch from ptx_change, the wire.ReplacePlan)."""
        value_ix = {v: i for i, v in enumerate(batch.values)}
        ids = []
        for v in replacement_values:
            if not isinstance(v, str):
                raise ValueError("Expected value inserted into text to be a string")
            if v not in value_ix:
                value_ix[v] = len(batch.values)
                batch.values.append(v)
            ids.append(value_ix[v])
        plan = view.replace_plan(pattern, ids, batch.n_logs, ascii_nocase=ascii_nocase)
        plan.ops.actor = np.asarray([batch.doc_actors[batch.log_doc[l]].index(actors[l]) for l in range(batch.n_logs)], dtype=np.uint32)
        plan.ops.max_actors = max(batch.max_actors, max((len(a) for a in batch.doc_actors), default=1))
        made, status = self.change(dbatch, dresult, plan.ops)
        return made, status, plan

    def sync_replicas(self, dbatch, pairs, max_attempts=10001):
        """getMissingChanges + applyChanges (reference/test/merge.ts:4-38) for many replica pairs with the logs resident (ptx_sync_replicas):
        `pairs` = [(source log, target log)], two replicas of one document each; a bidirectional sync is (l, r) and (r, l) in one call.
        max_attempts: the reference's guard (10 001; 0 = unbounded).  Returns (resident batch `more` whose log `target` holds the changes the
        target lacks in the order it admits them — made for append_device(dbatch, more) —, status per pair as a numpy array)."""
        pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        src, dst = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        n = len(pr)
        status = np.zeros(max(n, 1), dtype=np.uint32)
        h = C.c_void_p()
        self._check(self.lib.ptx_sync_replicas(self.ctx, dbatch, n, src.ctypes.data_as(abi.u32p), dst.ctypes.data_as(abi.u32p), max_attempts, C.byref(h),
                                               status.ctypes.data_as(abi.u32p)))
        return h, status[:n]

    def at_versions(self, dbatch, cuts, clocks=None, prefix=None, then_rest=False):
        """Resident logs at a past version (ptx_batch_at_versions): `cuts` = the source log of every cut; either `clocks` ([n_cuts, max_actors] u32: a change of
        actor a is kept iff seq <= clocks[c][a], abi.VERSION_ALL = all) or `prefix` ([n_cuts]: the first k changes of the log).  then_rest: the dropped
        changes follow the kept ones, and first_row[c] is what replay_patches takes as first_row for the Patch[] from that version to the present.
        Returns (resident batch whose log c is cut c, status, n_kept, first_row, clocks_out [n_cuts, max_actors]) — the last four numpy arrays; a failed
        cut (abi.ERR_MISSING_DEP for a clock no replica could have had, ERR_CAPACITY, ERR_BAD_OP) is an empty log."""
        src = np.ascontiguousarray(cuts, dtype=np.uint32).reshape(-1)
        n, na = len(src), int(self.lib.ptx_batch_max_actors(dbatch))
        ck = pf = None
        if clocks is not None:
            ck = np.ascontiguousarray(clocks, dtype=np.uint32).reshape(-1)
            if len(ck) != n * na:
                raise ValueError("at_versions: clocks must hold max_actors (%d) entries per cut" % na)
        if prefix is not None:
            pf = np.ascontiguousarray(prefix, dtype=np.uint32).reshape(-1)
            if len(pf) != n:
                raise ValueError("at_versions: prefix must hold one entry per cut")
        ptr = lambda a: a.ctypes.data_as(abi.u32p) if a is not None and len(a) else (C.cast(C.c_void_p(a.ctypes.data), abi.u32p) if a is not None else None)  # noqa: E731
        status, n_kept, first_row = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(3))
        clocks_out = np.zeros(max(n * na, 1), dtype=np.uint32)
        h = C.c_void_p()
        self._check(self.lib.ptx_batch_at_versions(self.ctx, dbatch, n, ptr(src), ptr(ck), ptr(pf), abi.VERSIONS_THEN_REST if then_rest else 0, C.byref(h), ptr(status),
                                                   ptr(n_kept), ptr(first_row), ptr(clocks_out)))
        return h, status[:n], n_kept[:n], first_row[:n], clocks_out[: n * na].reshape(n, na)

    def free_batch(self, h):
        self.lib.ptx_batch_free(self.ctx, h)

    def alloc_result(self, dbatch):
        h = C.c_void_p()
        self._check(self.lib.ptx_result_alloc(self.ctx, dbatch, C.byref(h)))
        return h

    def free_result(self, h):
        self.lib.ptx_dresult_free(self.ctx, h)

    def merge(self, dbatch, dresult):
        self._check(self.lib.ptx_merge(self.ctx, dbatch, dresult))

    def merge_timed(self, dbatch, dresult, iters):
        """Milliseconds (HIP events on the engine's stream) of `iters` back-to-back merges."""
        ms = C.c_float()
        self._check(self.lib.ptx_merge_timed(self.ctx, dbatch, dresult, iters, C.byref(ms)))
        return float(ms.value)

    def root_map(self, dbatch):
        """The map objects of every replica of a resident batch (ptx_root_map: getRoot(), micromerge.ts:443-449): wire.RootMaps."""
        m = abi.ptx_root_maps()
        self._check(self.lib.ptx_root_map(self.ctx, dbatch, C.byref(m)))
        try:
            n = int(m.n_logs)
            off = np.ctypeslib.as_array(m.entry_off, shape=(n + 1,)).astype(np.uint64).copy()
            logs = np.frombuffer(C.string_at(m.logs, max(n, 1) * C.sizeof(abi.ptx_root_log)), dtype=abi.ROOT_LOG_DTYPE)[:n].copy()
            total = int(off[-1])
            ent = np.frombuffer(C.string_at(m.entries, total * C.sizeof(abi.ptx_root_entry)), dtype=abi.ROOT_ENTRY_DTYPE).copy() if total else np.zeros(0, dtype=abi.ROOT_ENTRY_DTYPE)
            return wire.RootMaps(entry_off=off, logs=logs, entries=ent)
        finally:
            self.lib.ptx_root_maps_free(C.byref(m))

    def phase_cycles(self, dbatch, dresult, n=32):
        """Diagnostic: shader-clock cycles per phase of merge_core.h, summed over all workgroups."""
        out = (C.c_uint64 * n)()
        self._check(self.lib.ptx_merge_phase_cycles(self.ctx, dbatch, dresult, out, n))
        return [int(x) for x in out]

    def set_stream(self, hip_stream):
        """Run this engine on the caller's HIP stream (an int: e.g. torch.cuda.current_stream().cuda_stream); 0 = its own again."""
        self._check(self.lib.ptx_set_stream(self.ctx, C.c_void_p(hip_stream or None)))

    def count_converged(self, dresult, replicas, count_device_ptr):
        """Documents whose `replicas` logs all carry the same digest, into a u64 in device memory (stream-ordered, no host sync)."""
        self._check(self.lib.ptx_count_converged(self.ctx, dresult, replicas, C.c_void_p(count_device_ptr)))

    def calib_stream(self, dbatch):
        """Diagnostic: stream the batch's columns once (kernel ptx_calib_stream_kernel); returns the bytes that stream is."""
        n = C.c_uint64()
        self._check(self.lib.ptx_calib_stream(self.ctx, dbatch, C.byref(n)))
        return int(n.value)

    # ---- multi-GPU: the digest all-gather over RCCL, inside the library ----
    def comm_use_library(self, path):
        """Bind the collective library from `path` (before the first comm_* call of the process) instead of the process's librccl.so.1."""
        self._check(self.lib.ptx_comm_use_library(self.ctx, os.fsencode(path)))

    def comm_unique_id(self):
        """128 bytes (ncclUniqueId) rank 0 makes and hands to the other ranks."""
        buf = (C.c_uint8 * abi.COMM_ID_BYTES)()
        self._check(self.lib.ptx_comm_unique_id(self.ctx, buf))
        return bytes(buf)

    def comm_init(self, unique_id, rank, n_ranks):
        buf = (C.c_uint8 * abi.COMM_ID_BYTES).from_buffer_copy(unique_id)
        h = C.c_void_p()
        self._check(self.lib.ptx_comm_init(self.ctx, buf, rank, n_ranks, C.byref(h)))
        return h

    def comm_destroy(self, comm):
        self.lib.ptx_comm_destroy(self.ctx, comm)

    def allgather_digests(self, comm, dresult, counts, out_device_ptr):
        """Digests of every rank's result -> [sum(counts), 2] u64 at `out_device_ptr` (rank-major), on the engine's stream."""
        c = np.ascontiguousarray(counts, dtype=np.uint32)
        if len(c) != self.lib.ptx_comm_n_ranks(comm):
            raise ValueError("allgather_digests: counts must hold one entry per rank of the communicator (%d)" % self.lib.ptx_comm_n_ranks(comm))
        self._check(self.lib.ptx_allgather_digests(self.ctx, comm, dresult, c.ctypes.data_as(abi.u32p), C.c_void_p(out_device_ptr)))

    def count_converged_digests(self, digests_device_ptr, n_logs, replicas, count_device_ptr):
        self._check(self.lib.ptx_count_converged_digests(self.ctx, C.c_void_p(digests_device_ptr), n_logs, replicas, C.c_void_p(count_device_ptr)))

    def sync(self):
        self._check(self.lib.ptx_sync(self.ctx))

    def download(self, dbatch, dresult):
        res = abi.ptx_result()
        self._check(self.lib.ptx_result_download(self.ctx, dbatch, dresult, C.byref(res)))
        try:
            return _copy_result(res)
        finally:
            self.lib.ptx_result_free(C.byref(res))

    def download_range(self, dbatch, dresult, first_log, n_logs):
        """Result rows of logs [first_log, first_log + n_logs) only, rebased to row 0 (a sample of a large resident batch)."""
        res = abi.ptx_result()
        self._check(self.lib.ptx_result_download_range(self.ctx, dbatch, dresult, first_log, n_logs, C.byref(res)))
        try:
            return _copy_result(res)
        finally:
            self.lib.ptx_result_free(C.byref(res))

    # ---- document text ----
    def upload_strings(self, values):
        """A string table made resident (ptx_strings_upload): `values` = the batch's string table (wire.Batch.values), JS strings — UTF-16 code
        units, lone surrogates allowed.  Returns the handle Engine.text takes; free it with free_strings."""
        enc = [v.encode("utf-16-le", "surrogatepass") for v in values]
        off = np.zeros(len(enc) + 1, dtype=np.uint64)
        if enc:
            off[1:] = np.cumsum([len(e) // 2 for e in enc], dtype=np.uint64)
        units = np.frombuffer(b"".join(enc), dtype="<u2") if int(off[-1]) else np.zeros(1, dtype=np.uint16)
        h = C.c_void_p()
        self._check(self.lib.ptx_strings_upload(self.ctx, units.ctypes.data_as(abi.u16p), off.ctypes.data_as(abi.u64p), len(enc), C.byref(h)))
        return h

    def free_strings(self, h):
        self.lib.ptx_strings_free(self.ctx, h)

    def text(self, dbatch, dresult, dstrings, first_log=0, n_logs=None):
        """The text of the logs [first_log, first_log + n_logs) assembled on the device (ptx_result_text_range): wire.Text — one UTF-16 buffer, per-log
        offsets into it and per span the code-unit offset of its first character, so that a span's text is one slice (wire.decode_spans_text)."""
        if n_logs is None:
            n_logs = self.n_logs(dbatch) - first_log
        t = abi.ptx_text()
        self._check(self.lib.ptx_result_text_range(self.ctx, dbatch, dresult, dstrings, first_log, n_logs, C.byref(t)))
        try:
            n, arr = int(t.n_logs), _copied
            text_off, span_off = arr(t.text_off, np.uint64, n + 1), arr(t.span_off, np.uint64, n + 1)
            return wire.Text(status=arr(t.status, np.uint32, n), text_off=text_off, text=arr(t.text, np.uint16, int(text_off[n])), span_off=span_off,
                             span_unit=arr(t.span_unit, np.uint32, int(span_off[n])), kernel_ms=float(t.kernel_ms))
        finally:
            self.lib.ptx_text_free(C.byref(t))

    def find_text(self, dbatch, dresult, dstrings, pattern, first_log=0, n_logs=None, ascii_nocase=False, max_hits_per_log=0xFFFFFFFF):
        """Every position of `pattern` (a str: UTF-16 code units, lone surrogates allowed) in the text of the logs [first_log, first_log + n_logs), found on the
        device without downloading the text (ptx_result_find_text): wire.Matches — per log the count of ALL matches and, for the first max_hits_per_log of
        them in ascending order, the code-unit offset and the range [hit_start, hit_end) of visible element indexes, which Engine.change takes as
        delete {index, count} or addMark {startIndex, endIndex}.  max_hits_per_log=0 only counts."""
        if n_logs is None:
            n_logs = self.n_logs(dbatch) - first_log
        pat = np.frombuffer(pattern.encode("utf-16-le", "surrogatepass"), dtype="<u2").astype(np.uint16)
        m = abi.ptx_matches()
        self._check(self.lib.ptx_result_find_text(self.ctx, dbatch, dresult, dstrings, first_log, n_logs, pat.ctypes.data_as(abi.u16p), len(pat),
                                                  abi.FIND_ASCII_NOCASE if ascii_nocase else 0, max_hits_per_log, C.byref(m)))
        try:
            n, arr = int(m.n_logs), _copied
            hit_off = arr(m.hit_off, np.uint64, n + 1)
            nh = int(hit_off[n])
            return wire.Matches(status=arr(m.status, np.uint32, n), n_matches=arr(m.n_matches, np.uint32, n), hit_off=hit_off, hit_unit=arr(m.hit_unit, np.uint32, nh),
                                hit_start=arr(m.hit_start, np.uint32, nh), hit_end=arr(m.hit_end, np.uint32, nh), n_pattern=int(m.n_pattern), kernel_ms=float(m.kernel_ms))
        finally:
            self.lib.ptx_matches_free(C.byref(m))

    def text_slices(self, dbatch, dresult, dstrings, slices, first_log=0, n_logs=None):
        """The text and the span rows of element ranges of the logs [first_log, first_log + n_logs), cut on the device without downloading the documents
        (ptx_result_text_slices): wire.Slices.  `slices` holds, per log of the range, a list of (start, end) visible element indexes with
        Array.prototype.slice's clamping for non-negative arguments (0xFFFFFFFF is a legal bound); a log's slices may come in any order, overlap and repeat,
        and every output follows that order: hits of find_text widened by some context, a result's cintervals, a viewport."""
        if n_logs is None:
            n_logs = self.n_logs(dbatch) - first_log
        if len(slices) != n_logs:
            raise ValueError("slices holds %d lists for %d logs" % (len(slices), n_logs))
        off = np.zeros(n_logs + 1, dtype=np.uint64)
        if n_logs:
            off[1:] = np.cumsum([len(s) for s in slices], dtype=np.uint64)
        flat = np.array([p for s in slices for p in s], dtype=np.uint32).reshape(-1, 2)
        start, end = np.ascontiguousarray(flat[:, 0]), np.ascontiguousarray(flat[:, 1])
        return self.text_slices_flat(dbatch, dresult, dstrings, off, start, end, first_log, n_logs)

    def text_slices_flat(self, dbatch, dresult, dstrings, slice_off, slice_start, slice_end, first_log=0, n_logs=None):
        """text_slices with the C ABI's own arrays: slice_off u64 [n_logs + 1], slice_start / slice_end u32 [slice_off[n_logs]] (numpy; None passes NULL)."""
        if n_logs is None:
            n_logs = self.n_logs(dbatch) - first_log
        ptr = lambda a, t: a.ctypes.data_as(t) if a is not None and len(a) else C.cast(None, t)  # noqa: E731
        m = abi.ptx_slices()
        self._check(self.lib.ptx_result_text_slices(self.ctx, dbatch, dresult, dstrings, first_log, n_logs, ptr(slice_off, abi.u64p), ptr(slice_start, abi.u32p),
                                                    ptr(slice_end, abi.u32p), C.byref(m)))
        try:
            n, k, arr = int(m.n_logs), int(m.n_slices), _copied
            unit_off, sspan_off = arr(m.unit_off, np.uint64, k + 1), arr(m.sspan_off, np.uint64, k + 1)
            nr = int(sspan_off[k])
            return wire.Slices(status=arr(m.status, np.uint32, n), slice_off=np.array(slice_off, dtype=np.uint64) if n else np.zeros(1, np.uint64),
                               elem_start=arr(m.elem_start, np.uint32, k), elem_end=arr(m.elem_end, np.uint32, k), unit_off=unit_off,
                               text=arr(m.text, np.uint16, int(unit_off[k])), sspan_off=sspan_off, sspans=arr(m.sspans, abi.SPAN_DTYPE, nr),
                               sspan_unit=arr(m.sspan_unit, np.uint32, nr), kernel_ms=float(m.kernel_ms))
        finally:
            self.lib.ptx_slices_free(C.byref(m))

    def text_view(self, dbatch, dresult, dstrings, first_log=0, n_logs=None):
        """A resident text view of the logs [first_log, first_log + n_logs) of one merge (ptx_text_view_create): the assembled text and the element prefix stay on
        the device, and TextView.find_text / text_slices / find_snippets query them any number of times without a text or prefix pass.  `dstrings` (and the
        batch) may be freed once this returns; `dresult` must outlive the view and stay the merge it was made from.  Free it with TextView.free()."""
        if n_logs is None:
            n_logs = self.n_logs(dbatch) - first_log
        h = C.c_void_p()
        self._check(self.lib.ptx_text_view_create(self.ctx, dbatch, dresult, dstrings, first_log, n_logs, C.byref(h)))
        return TextView(self, h)

    def replay_patches(self, dbatch, dresult, first_row=None):
        """The Patch[] stream every applyChange of every log would have returned (reference/src/micromerge.ts:499),
        as wire.Patches; `dresult` = the merge of the same batch (engine created without FLAG_NO_ELEM_RANK).
        first_row[l]: only the records of log l's rows from there on (ptx_replay_patches_from: the Changes appended to a resident replica)."""
        p = abi.ptx_patches()
        if first_row is None:
            self._check(self.lib.ptx_replay_patches(self.ctx, dbatch, dresult, C.byref(p)))
        else:
            first = np.ascontiguousarray(first_row, dtype=np.uint32)
            if len(first) != self.n_logs(dbatch):
                raise ValueError("first_row needs one entry per replica log")
            self._check(self.lib.ptx_replay_patches_from(self.ctx, dbatch, dresult, first.ctypes.data_as(C.c_void_p), C.byref(p)))
        try:
            n = int(p.n_logs)
            off = np.ctypeslib.as_array(p.patch_off, shape=(n + 1,)).copy() if n else np.zeros(1, dtype=np.uint64)
            logs = np.frombuffer(C.string_at(p.logs, n * C.sizeof(abi.ptx_patch_log)), dtype=abi.PATCH_LOG_DTYPE).copy() if n else np.zeros(0, dtype=abi.PATCH_LOG_DTYPE)
            total = int(off[n]) if n else 0
            if total:  # (not C.string_at: its size is a C int, and the streams of a large batch exceed 2 GiB)
                rows = np.ctypeslib.as_array(C.cast(p.patches, C.POINTER(C.c_uint8)), shape=(total * C.sizeof(abi.ptx_patch),)).view(abi.PATCH_DTYPE).copy()
            else:
                rows = np.zeros(0, dtype=abi.PATCH_DTYPE)
            return wire.Patches(patch_off=off, logs=logs, patches=rows, kernel_ms=float(p.kernel_ms), launches=int(p.launches), hbm_logs=int(p.reserved))
        finally:
            self.lib.ptx_patches_free(C.byref(p))

    def accumulate_patches(self, dbatch, pat):
        """Patch streams of any origin (wire.Patches: this library's replay, or records a peer sent) turned back into the canonical rows of the documents
        they describe — reference/test/accumulatePatches.ts on the device (ptx_accumulate_patches).  Returns what `download` returns (no elem_rank); a
        log whose stream is malformed reports PTX_ERR_INDEX_OOB / BAD_OP / CAPACITY and the index of its first bad record in reserved[1]."""
        n = self.n_logs(dbatch)
        off = np.ascontiguousarray(pat.patch_off, dtype=np.uint64)
        logs = np.ascontiguousarray(pat.logs, dtype=abi.PATCH_LOG_DTYPE)
        rows = np.ascontiguousarray(pat.patches, dtype=abi.PATCH_DTYPE)
        if len(logs) != n or len(off) != n + 1 or len(rows) < int(off[n]):
            raise ValueError("the patch streams do not match the batch")
        p = abi.ptx_patches()
        p.n_logs = n
        p.patch_off = off.ctypes.data_as(abi.u64p)
        p.logs = logs.ctypes.data_as(C.POINTER(abi.ptx_patch_log))
        p.patches = rows.ctypes.data_as(C.POINTER(abi.ptx_patch))
        res = abi.ptx_result()
        self._check(self.lib.ptx_accumulate_patches(self.ctx, dbatch, C.byref(p), C.byref(res)))
        try:
            return _copy_result(res)
        finally:
            self.lib.ptx_result_free(C.byref(res))

    def check_patches(self, dbatch, dresult):
        """The fuzzer's patch assertion (reference/test/fuzz.ts:245-278) for every log of a resident batch, on the device: replay, accumulate the records
        where they were written, compare with the merge `dresult` (ptx_check_patches; no record is downloaded).  Returns (rows, n_disagree): rows =
        PATCH_CHECK_DTYPE [n_logs] {status, agrees, n_patches, first_bad_record, digest}, n_disagree = the logs with status 0 and agrees == 0."""
        n = self.n_logs(dbatch)
        rows = np.zeros(max(n, 1), dtype=abi.PATCH_CHECK_DTYPE)
        bad = C.c_uint64(0)
        self._check(self.lib.ptx_check_patches(self.ctx, dbatch, dresult, rows.ctypes.data_as(C.POINTER(abi.ptx_patch_check_log)), C.byref(bad)))
        return rows[:n], int(bad.value)

    def check_patches_ms(self):
        """(replay_ms, accum_ms): HIP-event durations of the kernels of the last check_patches: the replay launches of its last replay attempt only, and the accumulate launches summed over the packed ranges."""
        a, b = C.c_float(0), C.c_float(0)
        self._check(self.lib.ptx_check_patches_ms(self.ctx, C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    def generate(self, replicas, ops_per_log, mix, mark_types, n_docs, seed, first_doc=0, list_cap=0, initial_text=""):
        """On-device change(): n_docs PTXGEN documents (oracle/ptxgen.js, i.e. the workload of reference/test/fuzz.ts)
        generated straight into HBM.  Returns (resident batch handle, {"kernel_ms", "n_comments"})."""
        cfg = abi.ptx_gen_config()
        cfg.replicas, cfg.ops_per_log, cfg.n_mark_types = replicas, ops_per_log, len(mark_types)
        for i in range(4):
            cfg.mix[i] = mix[i]
        for i, t in enumerate(mark_types):
            cfg.mark_types[i] = t
        cfg.seed, cfg.first_doc, cfg.n_docs, cfg.list_cap = seed, first_doc, n_docs, list_cap
        cfg.initial_text = initial_text.encode("ascii")
        h = C.c_void_p()
        info = abi.ptx_gen_info()
        self._check(self.lib.ptx_generate(self.ctx, C.byref(cfg), C.byref(h), C.byref(info)))
        try:
            nc = np.ctypeslib.as_array(info.n_comments, shape=(n_docs,)).copy() if n_docs else np.zeros(0, dtype=np.uint32)
            return h, {"kernel_ms": float(info.kernel_ms), "n_comments": nc}
        finally:
            self.lib.ptx_gen_info_free(C.byref(info))

    def download_batch(self, dbatch, values=None, urls=None, log_doc=None, doc_actors=None, doc_comments=None, keys=None, map_values=None):
        """Copy a resident batch back as a wire.Batch (the decode tables are the caller's: a generated batch uses
        wire.GEN_VALUES / GEN_URLS / generated_tables)."""
        hb = abi.ptx_host_batch()
        self._check(self.lib.ptx_batch_download(self.ctx, dbatch, C.byref(hb)))
        try:
            b = hb.b
            L, T = int(b.n_logs), int(b.n_ops)

            def arr(ptr, dtype, n):
                return np.frombuffer(C.string_at(ptr, n * np.dtype(dtype).itemsize), dtype=dtype).copy() if n else np.zeros(0, dtype=dtype)

            log_off = arr(b.log_off, np.uint64, L + 1)
            has_env = bool(b.chg_off)
            chg_off = arr(b.chg_off, np.uint64, L + 1) if has_env else None
            NC = int(chg_off[-1]) if has_env else 0
            return wire.Batch(
                log_off, arr(b.op_id, np.uint64, T), arr(b.ref_a, np.uint64, T), arr(b.ref_b, np.uint64, T), arr(b.payload, np.uint32, T),
                arr(b.action, np.uint8, T), arr(b.mark_type, np.uint8, T), arr(b.side_a, np.uint8, T), arr(b.side_b, np.uint8, T),
                chg_off, arr(b.chg_hdr, np.uint32, NC) if has_env else None,
                arr(b.chg_env, np.uint16, NC * abi.env_stride(b.max_actors)) if has_env else None, int(b.max_actors), arr(b.log_hdr, abi.LOG_HDR_DTYPE, L), values or [], urls or [], log_doc or [], doc_actors or [], doc_comments or [], keys or [], map_values or [],
                chg_env_hi=arr(b.chg_env_hi, np.uint16, NC * abi.env_stride(b.max_actors)) if has_env and bool(b.chg_env_hi) else None)
        finally:
            self.lib.ptx_host_batch_free(C.byref(hb))

    def download_logs(self, dresult, n_logs):
        out = np.zeros(n_logs, dtype=abi.LOG_RESULT_DTYPE)
        self._check(self.lib.ptx_result_download_logs(self.ctx, dresult, out.ctypes.data_as(C.POINTER(abi.ptx_log_result)), n_logs))
        return out

    def pack_digests(self, dresult, first, count, dst_device_ptr):
        self._check(self.lib.ptx_pack_digests(self.ctx, dresult, first, count, C.c_void_p(dst_device_ptr)))

    def n_logs(self, dbatch):
        return int(self.lib.ptx_batch_n_logs(dbatch))

    def n_ops(self, dbatch):
        return int(self.lib.ptx_batch_n_ops(dbatch))

    def n_changes(self, dbatch):
        return int(self.lib.ptx_batch_n_changes(dbatch))

    def launch_shape(self, dbatch):
        """(threads per workgroup, dynamic LDS bytes per workgroup) the library chose for this batch."""
        t, l = C.c_uint32(), C.c_uint32()
        self.lib.ptx_batch_launch_shape(dbatch, C.byref(t), C.byref(l))
        return int(t.value), int(l.value)

    def max_ops_per_log(self):
        return int(self.lib.ptx_max_ops_per_log(self.ctx))

    def kernel_name(self):
        return self.lib.ptx_kernel_name().decode()

    def batch_kernel_name(self, dbatch):
        """The build of the merge kernel ptx_merge launches for this resident batch (its name in a rocprofv3 trace)."""
        return self.lib.ptx_batch_kernel_name(self.ctx, dbatch).decode()
