"""Shared by tests/test_layout_cases.py (CPU: the references below against the encoder, the emulation and committed fixtures) and
tests/test_gpu_layout_kernels.py (the C ABI on a real MI355X): case builders and numpy references for the kernels written directly in
peritext_amd/csrc/peritext_hip.hip, which have no CPU build — result offsets and compaction, the device census, the tiled upload's offsets, the
streaming append, the convergence counts and digest packing, the patch pack.

Every comparison made with these is exact.  A reference is never what the library returned: offsets are prefix sums of the EMULATION's per-log counts,
log headers come from wire.census (itself held to a count over the Change JSON in the CPU module), appended batches from helpers.concat_batches (held
there to one encode of the whole logs), tilings from Batch.tile (held to an encode of the documents repeated).

The logs of the census and append cases hold ONE op per change, so that a log can be cut after any number of rows (wire.split_batch cuts at changes) and
every row may carry any actor and counter; they are valid documents all the same (seq contiguous per actor, deps = everything made before)."""
import functools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

import helpers as H
from peritext_amd import abi, wire

OP_COLUMNS = ("op_id", "ref_a", "ref_b", "payload", "action", "mark_type", "side_a", "side_b")
SMALL_DOWNLOAD_ROWS = 65536  # PTX_SMALL_DOWNLOAD_ROWS of peritext_hip.hip: ranges of up to this many op rows take the context's staging blocks
CHUNK = 1024  # logs per step of ptx_result_offsets_kernel


def _golden(name):
    with open(os.path.join(H.GOLDEN, name)) as f:
        return json.load(f)


# ---- 1. result offsets and compaction ----
RANGE_SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049)
RANGE_FIRSTS = ("0", "1", "end")  # "end": the range that ends at the batch's last log
RESULT_COPIES = 257  # 8 logs x 257 = 2 056 > 2 * 1 024 + 1, well below 65 536 op rows: every range takes the staging-block path
RESULT_COPIES_LARGE = 1300  # more than 65 536 op rows and more than 2 048 logs: the whole download takes the exact-totals path


def result_base_docs():
    """[(what the log is, document)] of the heterogeneous base of the download tests: eight single-replica documents.  The empty log and the failing
    log are the first two and, mirrored, the last two: every tiled batch (and every range from log 0 or log 1, or up to the last log) starts and ends on them."""
    dup = H.duplicate_op_docs()[0]
    edge = H.edge_case_docs()
    return [("empty", [[]]), ("fails", dup), ("all_deleted", edge[6]), ("several_spans", H.boundary_docs()[3]), ("comments", edge[7]),
            ("ordinary", [H.mini_doc([])]), ("fails", dup), ("empty", [[]])]


def result_base_expected():
    """What the reference itself answered for the logs of the base that have an answer (tests/golden/edge_cases_ref.json; the plain text by hand): {log: {spans, text}}."""
    g = _golden("edge_cases_ref.json")
    assert g["impl"] == "ref"
    return {2: g["edge"][6][0], 3: g["boundary"][3][0], 4: g["edge"][7][0], 5: {"spans": [{"text": "ABCDE", "marks": {}}], "text": list("ABCDE")}}


@functools.lru_cache(maxsize=None)
def result_base():
    return wire.encode_docs([d for _, d in result_base_docs()])


def emu_results(batch):
    """The emulation's rows for a batch as the device merges it (admission on): wire.Results in the capacity layout."""
    return H.emu_merge(batch, admission=True)


_RESULT_FIELDS = ("logs", "values", "spans", "cintervals")


def emu_results_in_child(builder="result_base"):
    """emu_results(<builder>()) computed by a child process.  The GPU modules run in one process with tests/test_gpu_parity.py, which asserts that the CPU
    emulation is never loaded beside the HIP library; the child has no GPU open and is started once per module."""
    code = ("import sys; sys.path[:0] = [%r, %r]; import numpy as np; import layout_cases as LC; r = LC.emu_results(getattr(LC, sys.argv[2])()); "
            "np.savez(sys.argv[1], **{k: getattr(r, k) for k in LC._RESULT_FIELDS})" % (os.path.join(H.ROOT, "tests"), H.ROOT))
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "emu.npz")
        p = subprocess.run([sys.executable, "-c", code, out, builder], cwd=H.ROOT, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        with np.load(out) as z:
            return wire.Results(logs=z["logs"], values=z["values"], spans=z["spans"], cintervals=z["cintervals"], elem_rank=None)


COUNT_FIELDS = ("n_visible", "n_spans", "n_cintervals")
# every field of ptx_log_result but reserved[0]: the LDS bytes the log needed in the BUILD of the merge kernel that ran (a diagnostic, not a property of the log)
LOG_FIELDS = ("status", "n_ops", "n_elems", "n_visible", "n_spans", "n_cintervals", "digest")


def assert_logs_equal(got, want):
    assert len(got) == len(want)
    for f in LOG_FIELDS:
        assert np.array_equal(got[f], want[f]), f
    assert np.array_equal(got["reserved"][:, 1], want["reserved"][:, 1]), "first bad row"


class TiledExpectation:
    """The emulation's result of a base batch, tiled in numpy: what a download of logs [first, first + n) of upload(base, copies) must return."""

    def __init__(self, base, exp, copies):
        self.base, self.exp, self.copies = base, exp, copies
        self.nb = base.n_logs
        self.n_logs = self.nb * copies
        self.logs = np.tile(exp.logs, copies)
        self.log_off = base.tile(copies).log_off
        lo = base.log_off.astype(np.int64)
        self.pieces = []  # per base log: its rows in the emulation's capacity layout
        for l in range(self.nb):
            r = exp.logs[l]
            self.pieces.append((exp.values[lo[l]:lo[l] + int(r["n_visible"])], exp.spans[lo[l]:lo[l] + int(r["n_spans"])], exp.cintervals[lo[l]:lo[l] + int(r["n_cintervals"])]))

    def first_of(self, name, n):
        return {"0": 0, "1": 1, "end": self.n_logs - n}[name]

    def op_rows(self, first, n):
        return int(self.log_off[first + n] - self.log_off[first])

    def offsets(self, first, n):
        """(value_off, span_off, cint_off): exclusive prefix sums of the emulation's counts over the range, n + 1 entries each."""
        return tuple(np.concatenate([np.zeros(1, np.uint64), np.cumsum(self.logs[k][first:first + n].astype(np.uint64), dtype=np.uint64)]) for k in COUNT_FIELDS)

    def dense(self, first, n):
        """(values, spans, cintervals) of the range, back to back."""
        idx = np.arange(first, first + n) % self.nb
        empty = (np.zeros(0, np.uint32), np.zeros(0, abi.SPAN_DTYPE), np.zeros(0, abi.CINTERVAL_DTYPE))
        return tuple(np.concatenate([self.pieces[i][k] for i in idx] + [empty[k]]) for k in range(3))

    def sample(self, first, n):
        """Positions within the range whose canonical rows are compared log by log: first, last, around the 1 024-log chunk edge, one copy of every base log."""
        pos = {0, n - 1, CHUNK - 1, CHUNK, CHUNK + 1} | set(range(n // 2, n // 2 + self.nb))
        return sorted(p for p in pos if 0 <= p < n)

    def check(self, got, first, n):
        """A wire.Results the library downloaded for the range against the tiled emulation: offsets, exact dense lengths, log rows, dense rows byte for byte."""
        want_off = self.offsets(first, n)
        for name, w in zip(("value_off", "span_off", "cint_off"), want_off):
            g = getattr(got, name)
            assert g.dtype == np.uint64 and np.array_equal(g, w), (name, first, n)
        assert (len(got.values), len(got.spans), len(got.cintervals)) == tuple(int(w[-1]) for w in want_off), (first, n)
        assert_logs_equal(got.logs, self.logs[first:first + n])
        for k, (g, w) in enumerate(zip((got.values, got.spans, got.cintervals), self.dense(first, n))):
            assert g.tobytes() == w.tobytes(), (COUNT_FIELDS[k], first, n)
        for p in self.sample(first, n):
            for a, b in zip(wire.canonical_of_log(None, got, p), wire.canonical_of_log(self.base, self.exp, (first + p) % self.nb)):
                assert a.tobytes() == b.tobytes(), (first, n, p)


# ---- 2. the device census ----
CENSUS_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025)
STRIDE_EDGES = (0, 63, 64, 255, 256)  # lane 0 / last lane of a wave / first lane of the next / last thread of the workgroup / its first row of the second stride
BIG_COUNTER = 5000  # the counter of the row that carries max_counter (every other counter is 1 + its row)
LAST_COMMENT = "zz-last"  # sorts behind every other comment id: the row that uses it carries the largest comment payload


def stride_edges(n_rows):
    """The rows of a log of n_rows at which a maximum is placed: the census kernel's stride edges that the log has, and its last row."""
    return sorted({e for e in STRIDE_EDGES + (n_rows - 1,) if 0 <= e < n_rows})


def census_log(n_rows, pc=None, pa=None, pm=None, comments=True, maps=False, headless=False):
    """ONE replica log of exactly n_rows rows, one op per change.  Row 0 makes the text list, the rest is a typing run interleaved with deletes and add / removeMark
    ops of all four mark types (comments unless comments=False; maps: root-map writes and a second list object among them, rows that count in no census
    counter).  pc / pa / pm: the row that carries the log's largest op counter / the largest actor rank (actor `z`, used by that row alone) / the largest
    comment payload (a mark row: not row 0 unless headless — a log without its makeList, encoded with text_objs like newly arrived changes)."""
    if n_rows == 0:
        return []
    text = "1@a"
    changes, clock, chars = [], {}, []
    for row in range(n_rows):
        actor = "z" if row == pa else ("a" if row == 0 else "m")
        ctr = BIG_COUNTER if row == pc else row + 1
        oid = "%d@%s" % (ctr, actor)
        if row == 0 and not headless:
            op = {"opId": oid, "action": "makeList", "obj": "_root", "key": "text"}
            text = oid
        else:
            kind = "comment_last" if row == pm else "insert" if not chars else ("insert", "insert", "del", "strong", "insert", "em", "link", "comment", "insert", "map")[row % 10]
            if headless and not chars and kind != "comment_last":
                kind = "insert"
            if kind == "comment" and not comments:
                kind = "strong"
            if kind == "map" and not maps:
                kind = "insert"
            pick = lambda k: chars[(row * 7 + k) % len(chars)] if chars else "4000@a"  # noqa: E731  (a headless log's row 0 names an element it does not hold)
            if kind == "insert":
                op = {"opId": oid, "action": "set", "obj": text, "elemId": chars[-1] if chars else "_head", "insert": True, "value": "abcdefghij"[row % 10]}
                chars.append(oid)
            elif kind == "del":
                op = {"opId": oid, "action": "del", "obj": text, "elemId": pick(0)}
            elif kind == "map":
                op = ({"opId": oid, "action": "set", "obj": "_root", "key": "title", "value": "t%d" % row} if row % 20 == 9 else
                      {"opId": oid, "action": "makeList", "obj": "_root", "key": "notes%d" % row})
            else:
                a = (row * 7) % len(chars) if chars else 0
                e = min(len(chars) - 1, a + row % 5) if chars else 0
                mt = "comment" if kind == "comment_last" else kind
                op = {"opId": oid, "action": "removeMark" if row % 3 == 0 and kind != "comment_last" else "addMark", "obj": text, "markType": mt,
                      "start": {"type": "before", "elemId": chars[a] if chars else "4000@a"}}
                op["end"] = ({"type": "endOfText"} if row % 4 == 0 else {"type": "before", "elemId": chars[e] if chars else "4000@a"}) if mt in ("strong", "em") else \
                    {"type": "after", "elemId": chars[e] if chars else "4000@a"}
                if mt == "link" and op["action"] == "addMark":
                    op["attrs"] = {"url": "%s.com" % "ABC"[row % 3]}
                if mt == "comment":
                    op["attrs"] = {"id": LAST_COMMENT if kind == "comment_last" else "c%02d" % (row % 7)}
        deps = {a: s for a, s in clock.items() if a != actor}
        clock[actor] = clock.get(actor, 0) + 1
        changes.append({"actor": actor, "seq": clock[actor], "deps": deps, "startOp": ctr, "ops": [op]})
    return changes


@functools.lru_cache(maxsize=None)
def census_cases():
    """[(n_rows, pc, pa, pm, flags)]: every size of CENSUS_SIZES, each maximum at each stride edge of some log (the rotations), a log with map rows, a log
    without any comment mark, a headless log whose row 0 carries the largest comment payload."""
    cases = []
    for k, n in enumerate(CENSUS_SIZES):
        edges = stride_edges(n)
        for rot in range(len(edges) if n in (257, 1025) else 1):
            if not edges:
                cases.append((n, None, None, None, ""))
                continue
            pc, pa, pm = (edges[(k + rot + j) % len(edges)] for j in range(3))
            if pm < 2:  # (row 0 makes the list, row 1 types the first character: a mark needs one)
                pm = n - 1 if n - 1 >= 2 else None
            cases.append((n, pc, pa, pm, ""))
    cases.append((513, 256, 63, None, "no_comments"))
    cases.append((257, 255, 256, 64, "maps"))
    cases.append((65, 64, 63, 0, "headless"))
    return tuple(cases)


def census_docs():
    """(docs, text_objs) for wire.encode_docs: one single-replica document per case of census_cases()."""
    docs, text_objs = [], []
    for n, pc, pa, pm, flags in census_cases():
        docs.append([census_log(n, pc, pa, pm, comments=flags != "no_comments", maps=flags == "maps", headless=flags == "headless")])
        text_objs.append("1@a" if flags == "headless" else None)
    return docs, text_objs


@functools.lru_cache(maxsize=None)
def census_batch():
    docs, text_objs = census_docs()
    return wire.encode_docs(docs, text_objs=text_objs)


def census_of_changes(log, actors, comments):
    """The ptx_log_hdr fields of one log counted over the Change JSON (not over the encoded columns): what wire.census is held to."""
    h = {"n_ins": 0, "n_del": 0, "n_mark": [0, 0, 0, 0], "max_counter": 0, "max_actor": 0, "n_comment_ids": 0}
    for ch in log:
        for op in ch["ops"]:
            ctr, actor = wire.split_op_id(op["opId"])
            h["max_counter"], h["max_actor"] = max(h["max_counter"], ctr), max(h["max_actor"], actors.index(actor))
            on_list = "elemId" in op or op["action"] in ("addMark", "removeMark")
            if op["action"] == "set" and on_list:
                h["n_ins"] += 1
            elif op["action"] == "del" and on_list:
                h["n_del"] += 1
            elif op["action"] in ("addMark", "removeMark"):
                h["n_mark"][abi.MARK_NAMES.index(op["markType"])] += 1
                if op["markType"] == "comment":
                    h["n_comment_ids"] = max(h["n_comment_ids"], comments.index(op["attrs"]["id"]) + 1)
    return h


def maxima_rows(batch, log):
    """(row of the largest counter, row of the largest actor rank, row of the largest comment payload or None) of one encoded log, each required to be unique."""
    b0, b1 = int(batch.log_off[log]), int(batch.log_off[log + 1])
    ctr, act = (batch.op_id[b0:b1] >> np.uint64(32)).astype(np.int64), (batch.op_id[b0:b1] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    is_c = ((batch.action[b0:b1] == abi.ACT_ADDMARK) | (batch.action[b0:b1] == abi.ACT_REMOVEMARK)) & (batch.mark_type[b0:b1] == abi.MARK_COMMENT)
    pl = np.where(is_c, batch.payload[b0:b1].astype(np.int64), -1)
    out = []
    for v in (ctr, act, pl):
        top = np.flatnonzero(v == v.max()) if len(v) and v.max() >= 0 else []
        out.append(int(top[0]) if len(top) == 1 else None)
    return tuple(out)


def batch_without(batch, *names):
    """A shallow copy of a wire.Batch with the named optional columns set to None (log_hdr: the library computes it; chg_env_hi)."""
    import copy

    b = copy.copy(batch)
    for n in names:
        setattr(b, n, None)
    return b


def device_columns(batch):
    """The nine columns ptx_batch_wrap_device adopts, as torch tensors on the device (keep them alive while the wrapped batch is)."""
    import torch

    cols = {}
    for name in ("log_off",) + OP_COLUMNS:
        a = getattr(batch, name)
        as_signed = {np.dtype("uint64"): np.int64, np.dtype("uint32"): np.int32, np.dtype("uint8"): np.uint8}[a.dtype]
        cols[name] = torch.from_numpy(a.view(as_signed).copy()).cuda()
    torch.cuda.synchronize()
    return cols


# ---- comparing whole batches ----
def assert_batches_equal(got, want, hdr=True, what=""):
    """Column for column: log_off, the eight op columns, the envelope (present on both sides or on neither, the wide column too), the log headers."""
    for k in ("log_off",) + OP_COLUMNS:
        g, w = getattr(got, k), getattr(want, k)
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, k)
    assert (got.chg_off is None) == (want.chg_off is None), (what, "envelope")
    if want.chg_off is not None:
        assert got.max_actors == want.max_actors, (what, "max_actors")
        for k in ("chg_off", "chg_hdr", "chg_env"):
            assert np.array_equal(getattr(got, k), getattr(want, k)), (what, k)
        assert (got.chg_env_hi is None) == (want.chg_env_hi is None), (what, "chg_env_hi present")
        if want.chg_env_hi is not None:
            assert np.array_equal(got.chg_env_hi, want.chg_env_hi), (what, "chg_env_hi")
    if hdr:
        g, w = (b.log_hdr if b.log_hdr is not None else wire.census(b.log_off, b.op_id, b.action, b.mark_type, b.payload) for b in (got, want))
        assert np.array_equal(g, w), (what, "log_hdr")


# ---- 3. the tiled upload ----
TILE_SHAPES = ((127, 2), (51, 5), (16, 16), (7, 73), (8, 64), (32, 32))  # n_logs * copies + 1 = 255, 256, 257, 512, 513, 1 025 offsets
TILE_OFFSET_COUNTS = (255, 256, 257, 512, 513, 1025)


def small_docs(n_docs, empty_ends=True):
    """n_docs tiny single-replica documents from a pool (plain text, marks, comments, a failing log, a log without changes); with empty_ends the first and
    the last log are empty.  Change-free logs repeat their chg_off entry."""
    el = lambda i: "%d@a" % (i + 2)  # noqa: E731
    pool = [
        [H.mini_doc([])],
        [H.mini_doc([{"action": "addMark", "markType": "strong", "start": {"type": "before", "elemId": el(1)}, "end": {"type": "before", "elemId": el(3)}}])],
        [[]],
        [H.mini_doc([{"action": "addMark", "markType": "comment", "attrs": {"id": "c1"}, "start": {"type": "before", "elemId": el(0)}, "end": {"type": "after", "elemId": el(2)}},
                     {"action": "del", "elemId": el(4)}], first_text="ABCDEFG")],
        H.duplicate_op_docs()[0],
        [H.mini_doc([{"action": "set", "insert": True, "elemId": el(4), "value": "!"}])],
    ]
    docs = [pool[i % len(pool)] for i in range(n_docs)]
    if empty_ends and n_docs:
        docs[0] = docs[-1] = [[]]
    return docs


# ---- 4. append ----
APPEND_ROW_PAIRS = ((0, 0), (0, 5), (5, 0), (1, 1), (1, 255), (255, 1), (256, 1), (1, 256), (256, 256), (257, 600), (600, 257), (0, 600), (600, 0), (255, 257), (1, 0), (0, 1))
APPEND_LOG_COUNTS = (255, 256, 257)


def append_rows_case(extra_actors=0):
    """(whole, base, more): logs of one op per change cut so that log l has APPEND_ROW_PAIRS[l] rows on the two sides.  extra_actors: that many actor names
    more per document (max_actors 3 + extra: 9 actors make envelope rows of 12 entries, not a power of two)."""
    docs = []
    for k, (nb, nm) in enumerate(APPEND_ROW_PAIRS):
        n = nb + nm
        edges = stride_edges(n)
        docs.append([census_log(n, *(edges[(k + j) % len(edges)] if edges else None for j in range(2)), pm=n - 1 if n > 2 else None)])
    whole = wire.encode_docs(docs, extra_actors=[["x%d" % i for i in range(extra_actors)]] * len(docs))
    base, more = wire.split_batch(whole, [nb for nb, _ in APPEND_ROW_PAIRS])
    rows = lambda b: np.diff(b.log_off.astype(np.int64)).tolist()  # noqa: E731
    assert list(zip(rows(base), rows(more))) == list(APPEND_ROW_PAIRS)
    return whole, base, more


def append_logs_case(n_logs):
    """(whole, base, more) of n_logs tiny logs, cut after 0, 1 or all of their changes in turn (the offsets kernel's `i <= n` thread writes entry n_logs)."""
    whole = wire.encode_docs(small_docs(n_logs, empty_ends=False))
    base, more = wire.split_batch(whole, [(0, 1, 2)[l % 3] for l in range(n_logs)])
    return whole, base, more


def with_wide_column(batch, bump):
    """The batch with its envelope packed again as wire.pack_envelope_wide packs it: bump=True moves the seq of every third change beyond 16 bits (the wide column
    is needed; the logs are no valid documents any more), bump=False keeps the values and carries a wide column of zeros."""
    import copy

    b = copy.copy(batch)
    seq = batch.chg_seq.astype(np.uint64).copy()
    if bump:
        seq[::3] += np.uint64(70000)
    b.chg_hdr, b.chg_env, b.chg_env_hi = wire.pack_envelope_wide(batch.chg_actor, seq, batch.chg_nops, batch.chg_deps, batch.max_actors)
    if b.chg_env_hi is None:
        b.chg_env_hi = np.zeros_like(b.chg_env)
    return b


def appended(base, more):
    """What append(base, more) must hold: helpers.concat_batches, carrying the wide column exactly when either side carries it (a side without it contributes
    zeros); an envelope-less base without a row takes the envelope of `more`."""
    if base.chg_off is None:
        assert base.n_ops == 0
        return more
    out = H.concat_batches(base, more)
    either = base.chg_env_hi is not None or more.chg_env_hi is not None
    if either and out.chg_env_hi is None:
        out.chg_env_hi = np.zeros_like(out.chg_env)
    assert (out.chg_env_hi is not None) == either
    return out


def empty_base(n_logs):
    """n_logs logs without a row and without the Change envelope."""
    z = lambda t: np.zeros(0, dtype=t)  # noqa: E731
    return wire.Batch(np.zeros(n_logs + 1, np.uint64), z(np.uint64), z(np.uint64), z(np.uint64), z(np.uint32), z(np.uint8), z(np.uint8), z(np.uint8), z(np.uint8),
                      None, None, None, 0, None)


def split_in_four(whole):
    """Four batches whose logs, appended in order, are the logs of `whole`: cut after a quarter, a half and three quarters of every log's changes."""
    nch = np.diff(whole.chg_off.astype(np.int64))
    parts, rest, taken = [], whole, np.zeros_like(nch)
    for q in (1, 2, 3):
        cut = nch * q // 4
        head, rest = wire.split_batch(rest, cut - taken)
        parts.append(head)
        taken = cut
    return parts + [rest]


# ---- 5. convergence counts ----
CONVERGED_DOCS = (1, 63, 64, 65, 255, 256, 257, 513)
CONVERGED_REPLICAS = (1, 2, 3, 5)
DIVERGENCE_KINDS = ("first_word", "second_word", "last_replica")


def synthetic_digests(n_docs, replicas, variant):
    """(digests u64 [n_docs + 1, replicas, 2], {doc: kind}): converged documents with non-zero digests, except — where the index exists — divergent ones at 0, 63,
    64, 255, 256 and the last (in one word of one replica; which word / replica rotates with `variant`), failed ones (all {0, 0}) at 3, 61, 67, 253 and 259, and
    documents whose first word is zero and second is not (they count) at 2, 66 and 258.  The extra document behind the last is converged: a kernel that looked at
    one document too many would count it."""
    rng = np.random.default_rng(1000 * n_docs + 10 * replicas + variant)
    one = rng.integers(1, 2 ** 63, size=(n_docs + 1, 1, 2), dtype=np.uint64)
    dg = np.repeat(one, replicas, axis=1)
    kinds = {}
    for d in (2, 66, 258):
        if d < n_docs:
            dg[d, :, 0] = 0
            kinds[d] = "zero_first_word"
    for d in (3, 61, 67, 253, 259):
        if d < n_docs:
            dg[d] = 0
            kinds[d] = "failed"
    if replicas > 1:
        for k, d in enumerate(sorted({e for e in STRIDE_EDGES + (n_docs - 1,) if e < n_docs})):
            kind = DIVERGENCE_KINDS[(k + variant) % 3]
            r = replicas - 1 if kind == "last_replica" else 1 + (k % (replicas - 1))
            w = 1 if kind == "second_word" else 0 if kind == "first_word" else k % 2
            dg[d, r, w] ^= np.uint64(1 << (k + 1))
            kinds[d] = kind
    return dg, kinds


def converged_count(dg, n_docs):
    """The numpy expression of tests/test_gpu_edges.py, with the rule for failed logs: every replica's digest equals the first's, and that is not {0, 0}."""
    dg = dg[:n_docs]
    return int(((dg == dg[:, :1, :]).all(axis=(1, 2)) & (dg[:, 0, :] != 0).any(axis=1)).sum())


def converged_logs_count(logs, replicas):
    """The same over downloaded ptx_log_result rows (ptx_count_converged: every replica's status is PTX_OK too)."""
    dg = logs["digest"].reshape(-1, replicas, 2)
    return int(((dg == dg[:, :1, :]).all(axis=(1, 2)) & (logs["status"].reshape(-1, replicas) == 0).all(axis=1)).sum())


CONVERGENCE_COPIES = (7, 8, 9, 31, 32, 33)  # x 8 documents: 56 / 64 / 72 and 248 / 256 / 264 documents of three replicas


def convergence_docs():
    """Eight documents of three replicas: the first and the last have a replica that lags (tiled, they stand at 8k and 8k + 7: on both sides of 64 and of 256), one
    document fails in every replica, the rest converged."""
    el = lambda i: "%d@a" % (i + 2)  # noqa: E731
    ins = lambda v: H.mini_doc([{"action": "set", "insert": True, "elemId": el(4), "value": v}])  # noqa: E731
    dup = H.duplicate_op_docs()[0][0]
    lag = lambda v: [ins(v), ins(v), ins(v)[:1]]  # noqa: E731
    conv = lambda v: [ins(v)] * 3  # noqa: E731
    return [lag("p"), conv("q"), conv("r"), [dup] * 3, conv("s"), conv("q"), conv("t"), lag("u")]


PACK_COUNTS = (0, 1, 255, 256, 257)


# ---- 6. the patch pack ----
def patch_pack_case():
    """(batch, {log: expected patches}) of tests/golden/patches_rich_300.json (made by the reference) with an empty log and a failing log before and behind it."""
    g = _golden("patches_rich_300.json")
    assert g["impl"] == "ref"
    dup = H.duplicate_op_docs()[0]
    docs = [[[]], dup] + [d["logs"] for d in g["docs"]] + [dup, [[]]]
    want, log = {}, 2
    for d in g["docs"]:
        for e in d["expected"]:
            want[log] = e["patches"]
            log += 1
    return wire.encode_docs(docs), want
