"""Probe harness for change() on the device at the edges of its wave-wide list walks (peritext_amd/csrc/change_core.h: ptx_gen_select,
ptx_gen_after_tombstones, ptx_list_shift_up), independent of the backend in the manner of tests/change_script.py: the CPU emulation
(tests/test_emu_change_edges.py) and the C ABI on the GPU (tests/test_gpu_change_edges.py) run the same case tables.

The key device is the PROBE: `addMark strong {startIndex: i, endIndex: j}` with j < visible length emits before(elem[i]) and
before(elem[j]) (changeMark, peritext.ts:458-501) and changes nothing in the list the kernel holds (inclusive types set no
PTX_GK_AFTER flag).  A run of probes after an edit, in the same change() call, is therefore a read-out of that list: a shift that
corrupts it away from the edit shows up in the Change although the edit's own ops look right.

Expected values always come from the in-repo oracle at run time (helpers.oracle_change / oracle_apply), never from another backend
or another build.  A backend offers
    change_and_grow(batch, ops) -> (made batch, status per log, grown batch, merge results of the grown batch)
where the grown batch is log l of `batch` followed by what log l made (ptx_batch_append_device on the GPU, helpers.concat_batches
under emulation)."""
import json
import random

import change_script as CS
import helpers as H
from peritext_amd import abi, wire

T = ["text"]
OOB = "RangeError: List index out of bounds"


# ---- base replica logs with chosen places ----
class Base:
    """ONE replica log built without the generator, like helpers.synthetic_marks_log but with CHOSEN places: n_chars characters typed left to
    right (element i = list position i for good: nothing is ever inserted between them), then marks and deletes in the order of the calls.
    Element i has the id "<i + 2>@<actor>"."""

    def __init__(self, n_chars, actor="doc1"):
        self.actor, self.n = actor, n_chars
        self.ids = ["%d@%s" % (2 + i, actor) for i in range(n_chars)]
        self.chars = ["abcdefghij"[i % 10] for i in range(n_chars)]
        self.dead = [False] * n_chars
        ops = [{"opId": "1@%s" % actor, "action": "makeList", "obj": "_root", "key": "text"}]
        for i in range(n_chars):
            ops.append({"opId": self.ids[i], "action": "set", "obj": "1@%s" % actor, "elemId": "_head" if i == 0 else self.ids[i - 1], "insert": True, "value": self.chars[i]})
        self.log = [{"actor": actor, "seq": 1, "deps": {}, "startOp": 1, "ops": ops}]
        self.ctr = n_chars + 2

    def _change(self, ops):
        seq = len(self.log) + 1
        for k, op in enumerate(ops):
            op["opId"] = "%d@%s" % (self.ctr + k, self.actor)
            op["obj"] = "1@%s" % self.actor
        self.log.append({"actor": self.actor, "seq": seq, "deps": {self.actor: seq - 1}, "startOp": self.ctr, "ops": ops})
        self.ctr += len(ops)
        return self

    def mark(self, mark_type, start, end, action="addMark", attrs=None):
        """start / end = ("before" | "after", element) or "endOfText" — any boundary the Operation type allows (peritext.ts:17-21), also those
        changeMark never generates (an `after` start, an end that precedes its start)."""
        bd = lambda b: {"type": b} if isinstance(b, str) else {"type": b[0], "elemId": self.ids[b[1]]}  # noqa: E731
        op = {"action": action, "markType": mark_type, "start": bd(start), "end": bd(end)}
        if attrs is None and mark_type == "link" and action == "addMark":
            attrs = {"url": "base.example"}
        if attrs is None and mark_type == "comment":
            attrs = {"id": "comment-base"}
        if attrs is not None:
            op["attrs"] = attrs
        return self._change([op])

    def link(self, first, last):
        """addMark link over elements first..last: it ends `after` element `last` (made before that element dies)"""
        assert not self.dead[first] and not self.dead[last]
        return self.mark("link", ("before", first), ("after", last))

    def comment(self, first, last):
        assert not self.dead[first] and not self.dead[last]
        return self.mark("comment", ("before", first), ("after", last))

    def delete(self, lo, hi):
        """elements [lo, hi) die (one Change)"""
        assert all(not self.dead[i] for i in range(lo, hi))
        for i in range(lo, hi):
            self.dead[i] = True
        return self._change([{"action": "del", "elemId": self.ids[i]} for i in range(lo, hi)])

    def delete_each(self, places):
        for i in places:
            self.delete(i, i + 1)
        return self

    @property
    def vis_pos(self):
        """list positions of the visible elements, in order: visible index k lives at list position vis_pos[k]"""
        return [i for i in range(self.n) if not self.dead[i]]

    @property
    def vis(self):
        return self.n - sum(self.dead)

    def index_of(self, pos):
        """visible index of the element at list position `pos`, which must be alive"""
        assert not self.dead[pos], "position %d is a tombstone" % pos
        return pos - sum(self.dead[:pos])

    def text(self):
        return [self.chars[p] for p in self.vis_pos]


# ---- InputOperations ----
def ins(index, values):
    return {"path": T, "action": "insert", "index": index, "values": list(values)}


def dele(index, count=1):
    return {"path": T, "action": "delete", "index": index, "count": count}


def mark(mark_type, start, end, action="addMark"):
    op = {"path": T, "action": action, "markType": mark_type, "startIndex": start, "endIndex": end}
    if mark_type == "link" and action == "addMark":
        op["attrs"] = {"url": "probe.example"}
    if mark_type == "comment":
        op["attrs"] = {"id": "comment-new"}
    return op


def probes(indices, vis):
    """Probe ops that read the elements at the given visible indices (those >= vis are dropped), two per op: (i0, i1), (i2, i3) ...;
    an odd one out is read together with its predecessor."""
    ix = sorted(set(i for i in indices if 0 <= i < vis))
    out = [mark("strong", ix[k], ix[k + 1]) for k in range(0, len(ix) - 1, 2)]
    if len(ix) % 2:
        out.append(mark("strong", ix[-2] if len(ix) > 1 else ix[-1], ix[-1]))
    return out


def read_out(vis, step=1):
    """The full read-out: (0, 1), (2, 3) ... so that every position is read once; step > 1 reads every step-th."""
    return probes(range(0, vis, step), vis)


def around(index, vis, width=12):
    """a dozen probes' worth of indices around an edit"""
    return probes(range(max(0, index - width), min(vis, index + width)), vis)


def vis_after(vis, ops):
    for op in ops:
        if op["action"] == "insert":
            vis += len(op["values"])
        elif op["action"] == "delete":
            vis -= op["count"]
    return vis


def with_read_out(vis, ops, step=1):
    return list(ops) + read_out(vis_after(vis, ops), step)


class Case:
    """One replica log and the change() calls made on it; check(changes the oracle made) pins the literals of the case so that a later change of
    the builder cannot empty it."""

    def __init__(self, name, log, calls, actor="doc1", check=None):
        self.name, self.log, self.calls, self.actor, self.check = name, log, calls, actor, check


# ---- the oracle, asked once per table ----
_oracle_cache = {}


def _cached(kind, key_obj, fn):
    key = (kind, H.inputs_sha16(key_obj))
    if key not in _oracle_cache:
        _oracle_cache[key] = fn()
    return json.loads(json.dumps(_oracle_cache[key]))  # the shared answer stays unchanged


def oracle_change_per_replica(docs, calls, actors, impl="oracle"):
    """helpers.oracle_change without its raise on the first error (its callers see what they always saw): one {"changes": the Changes of the calls
    before the one that threw, "error": the message or None} per log, from the same `oracle/cli.js change`."""
    import os
    import tempfile

    reps, l = [], 0
    for logs in docs:
        for log in logs:
            reps.append({"actor": actors[l], "log": log, "calls": calls[l]})
            l += 1
    with tempfile.TemporaryDirectory() as td:
        inp, out = os.path.join(td, "in.json"), os.path.join(td, "out.json")
        with open(inp, "w") as f:
            json.dump({"replicas": reps}, f)
        H.run_node(["oracle/cli.js", "change", "--in", inp, "--impl", impl, "--out", out])
        with open(out) as f:
            return [{"changes": r["changes"], "error": r.get("error")} for r in json.load(f)["replicas"]]


def oracle_changes(docs, calls, actors, impl="oracle"):
    return _cached("change-" + impl, [docs, calls, actors], lambda: oracle_change_per_replica(docs, calls, actors, impl=impl))


def lds_bytes_without_lists(batch, ops):
    """The LDS window that holds everything of every log of the call BUT its element list (ptx_change_lds_need of change_core.h, restated): with it, the
    emulation driver keeps every list in its slice of "global" scratch, as the library does for lists beyond one CU's LDS and for every list under
    PTX_CHANGE_LIST_IN_HBM.  Asserts that no log that makes a change would fit WITH its list."""
    import numpy as np

    a16 = lambda x: (x + 15) & ~15  # noqa: E731
    hdr = a16(4 * (6 + 36))  # PtxChangeHdr
    per_op = np.where(ops.action == abi.IN_INSERT, ops.count, 0).astype(np.int64)
    cum = np.concatenate([[0], np.cumsum(per_op)])
    first_op = ops.op_off[ops.chg_off.astype(np.int64)].astype(np.int64)
    grow = cum[first_op[1:]] - cum[first_op[:-1]]
    rest = [hdr + a16(4 * (int(g) + 1)) + a16(4 * (ops.max_actors + 1)) for g in grow]
    busy = [l for l in range(batch.n_logs) if ops.chg_off[l + 1] > ops.chg_off[l]]
    lds = max(rest[l] for l in busy)
    for l in busy:
        n = int((batch.action[int(batch.log_off[l]):int(batch.log_off[l + 1])] == abi.ACT_INSERT).sum())
        assert rest[l] + a16(4 * (n + int(grow[l]) + 64)) > lds, "log %d would keep its list in LDS" % l
    return lds


def oracle_spans(docs):
    return _cached("apply", docs, lambda: H.oracle_apply(docs))


def comment_ids_of(calls):
    return sorted({op["attrs"]["id"] for ops in calls for op in ops if op.get("markType") == "comment"})


def run(backend, docs, calls, actors, expect_status=None, names=None):
    """docs[d] = the replica logs of document d; calls[l] = the change() calls of the replica behind log l (document-major), actors[l] its actor.
    Every made Change against the oracle's; where the oracle raises, the per-log status instead (such a log makes nothing and holds ONE call);
    then what was made is appended and merged, and the spans of every grown replica are compared with the oracle applying log + wanted Changes.
    Returns the oracle's per-log answers."""
    names = names or ["log %d" % l for l in range(len(calls))]
    want = oracle_changes(docs, calls, actors)
    per_doc_calls, l = [], 0
    for logs in docs:
        per_doc_calls.append([c for k in range(len(logs)) for c in calls[l + k]])
        l += len(logs)
    l = 0
    doc_actors = []
    for logs in docs:
        doc_actors.append(actors[l:l + len(logs)])
        l += len(logs)
    batch = wire.encode_docs(docs, extra_actors=doc_actors, extra_comments=[comment_ids_of(c) for c in per_doc_calls])
    ops = wire.encode_input_ops(batch, calls, actors)
    made, status, grown, res = backend.change_and_grow(batch, ops)
    flat_logs = [log for logs in docs for log in logs]
    assert len(want) == len(flat_logs) == len(status)
    wanted_logs = []
    for l, (log, w) in enumerate(zip(flat_logs, want)):
        got = wire.decode_changes(made, l, text_obj=CS.text_obj_of(log))
        if w["error"] is not None:
            assert len(calls[l]) == 1, names[l]
            assert int(status[l]) != 0, "%s: the oracle raised %r, the device made a Change" % (names[l], w["error"])
            if w["error"].startswith(OOB):
                assert int(status[l]) == abi.ERR_INDEX_OOB, names[l]
            assert got == [], names[l]
            wanted_logs.append(log)
            continue
        assert int(status[l]) == 0, "%s: status %d" % (names[l], int(status[l]))
        assert len(got) == len(w["changes"]) == len(calls[l]), names[l]
        for k, (g, x) in enumerate(zip(got, w["changes"])):
            g, x = CS.norm_change(g), CS.norm_change(x)
            if g != x:
                assert g["ops"] == x["ops"], "%s: call %d: first differing op %r" % (
                    names[l], k, next(((i, a, b) for i, (a, b) in enumerate(zip(g["ops"], x["ops"])) if a != b), (len(g["ops"]), len(x["ops"]))))
            assert g == x, "%s: call %d" % (names[l], k)
        wanted_logs.append(log + w["changes"])
    if expect_status is not None:
        assert [int(s) for s in status] == list(expect_status)
    # the replicas after their changes
    assert grown.n_logs == len(flat_logs)
    exp = oracle_spans([[wl] for wl in wanted_logs])
    for l, wl in enumerate(wanted_logs):
        assert int(res.logs["status"][l]) == 0, names[l]
        e = exp[l][0]
        if not any(op["action"] == "makeList" for c in wl for op in c["ops"]):
            assert int(res.logs["n_visible"][l]) == 0, names[l]  # no text list: nothing to show on either side
            continue
        assert e.get("error") is None, (names[l], e.get("error"))
        assert H.norm_spans(wire.decode_spans(grown, res, l)) == H.norm_spans(e["spans"]), "%s: spans after the call" % names[l]
    return want


def run_cases(backend, cases):
    """A table of single-replica cases as ONE batch (one document per case), then every case's own check."""
    want = run(backend, [[c.log] for c in cases], [c.calls for c in cases], [c.actor for c in cases], names=[c.name for c in cases])
    for c, w in zip(cases, want):
        if c.check:
            c.check(w)
    return want


def first_ref(w, call=0, op=0):
    return w["changes"][call]["ops"][op].get("elemId")


# ---- A. select across chunks ----
A_TARGETS = (63, 64, 65, 127, 128)


def bases_A():
    """300 characters, every third of the first 200 deleted — in two phases, since of three neighbouring positions one is always a multiple of three:
    phase 2 keeps 63, 64, 127 alive, phase 0 keeps 64, 65, 127, 128."""
    out = []
    for phase in (2, 0):
        b = Base(300).delete_each([i for i in range(200) if i % 3 == phase])
        out.append((phase, b, [p for p in A_TARGETS if not b.dead[p]] + [b.vis_pos[-1]]))
    return out


def cases_A():
    cases = []
    for phase, b, targets in bases_A():
        assert b.vis == (234 if phase == 2 else 233) and targets[-1] == 299
        for p in targets:
            i, v = b.index_of(p), b.vis
            assert b.vis_pos[i] == p and i != p  # tombstones before it: position != index
            j = b.index_of(64) if p != 64 else b.index_of(127)
            lo, hi = min(i, j), max(i, j)
            edits = {
                "insert": [ins(i + 1, ["X"])],                       # getListElementId(index - 1): resolves AT p
                "delete": [dele(i)],
                "inclusive": [mark("em", lo, hi)],                   # before(elem[i]) as a start or an end
                "link": [mark("link", min(i, 3), i + 1)],            # after(elem[endIndex - 1]) = after p
                "comment": [mark("comment", min(i, 5), i + 1)],
            }
            for kind, ops in edits.items():
                cases.append(Case("A phase %d pos %d %s" % (phase, p, kind), b.log, [with_read_out(v, ops)], check=_check_A(b, p, kind)))
    b = bases_A()[0][1]
    v = b.vis
    for name, ops in (("insert at vis + 1", [ins(v + 1, ["X"])]), ("delete at vis", [dele(v)]), ("delete count past the end", [dele(v - 2, 5)]),
                      ("mark startIndex = vis", [mark("strong", v, v + 2)]), ("link endIndex = 0", [mark("link", 0, 0)]),
                      ("inclusive endIndex > vis", [mark("strong", 5, v + 3)])):
        cases.append(Case("A oob " + name, b.log, [ops], check=_check_oob(name != "inclusive endIndex > vis")))
    return cases


def _check_oob(raises):
    def check(w):  # error or endOfText is the oracle's decision; pinned here so that the six stay what their names say
        if raises:
            assert w["error"] is not None and w["error"].startswith(OOB) and w["changes"] == [], w
        else:
            assert w["error"] is None and w["changes"][0]["ops"][0]["end"] == {"type": "endOfText"}, w
    return check


def _check_A(b, p, kind):
    def check(w):
        assert w["error"] is None
        op = w["changes"][0]["ops"][0]
        pid = b.ids[p]
        if kind == "insert":
            assert op["elemId"] == pid  # (no `after` slot of the base is a defined one: the tombstones behind it are not looked past)
        elif kind == "delete":
            assert op["elemId"] == pid
        elif kind == "inclusive":
            assert pid in (op["start"]["elemId"], op["end"]["elemId"])
        else:
            assert op["end"] == {"type": "after", "elemId": pid}
    return check


# ---- B. lookAfterTombstones across chunks ----
def cases_B():
    cases = []
    # B1: the marked tombstone in the second 64-chunk of the run wins over the one in the first
    b = Base(400).link(50, 180).comment(60, 120).delete(100, 230)
    cases.append(Case("B1", b.log, [with_read_out(b.vis, [ins(100, ["x", "y", "z"])])], check=lambda w: _eq(first_ref(w), "182@doc1")))
    # B2: the run reaches the end of the list
    b = Base(300).link(10, 290).delete(200, 300)
    cases.append(Case("B2", b.log, [with_read_out(b.vis, [ins(200, ["x"])])], check=lambda w: _eq(first_ref(w), "292@doc1")))
    # runs of exactly 63, 64 and 65 tombstones, the winning marked one at run offset 62, 63, 64 (an earlier marked one at offset 3)
    for run_len in (63, 64, 65):
        for off in (62, 63, 64):
            if off >= run_len:
                continue
            b = Base(200).delete_each(range(0, 20, 2)).link(5, 21 + off).comment(7, 21 + 3).delete(21, 21 + run_len)
            i = b.index_of(20) + 1
            cases.append(Case("B run %d marked at %d" % (run_len, off), b.log, [with_read_out(b.vis, [ins(i, ["x", "y"])])],
                              check=lambda w, want=b.ids[21 + off]: _eq(first_ref(w), want)))
    # a marked tombstone BEHIND the next visible element must not be taken: nothing marked in the run itself
    for run_len in (5, 62, 63, 64, 65):
        b = Base(200).delete_each(range(0, 20, 2)).link(5, 24 + run_len).delete(21, 21 + run_len).delete(22 + run_len, 30 + run_len)
        i = b.index_of(20) + 1
        cases.append(Case("B marked behind the next visible, run %d" % run_len, b.log, [with_read_out(b.vis, [ins(i, ["x"])])],
                          check=lambda w, want=b.ids[20]: _eq(first_ref(w), want)))
        # ... and one marked in the run as well: that one, not the later one
        b = Base(200).delete_each(range(0, 20, 2)).link(5, 24 + run_len).comment(7, 22).delete(21, 21 + run_len).delete(22 + run_len, 30 + run_len)
        cases.append(Case("B marked in the run and behind it, run %d" % run_len, b.log, [with_read_out(b.vis, [ins(i, ["x"])])],
                          check=lambda w, want=b.ids[22]: _eq(first_ref(w), want)))
    # the closed form of the defined `after` slots (change_core.h: end_first / start_written / end_written)
    b = Base(120)
    b.mark("link", ("after", 30), ("after", 35))      # both slots written, the start an `after` slot
    b.mark("link", ("after", 40), ("after", 40))      # the end slot is the slot it starts on
    b.mark("comment", ("before", 70), ("after", 50))  # the end element precedes the start: the end is met first
    b.mark("link", ("after", 90), ("after", 80))      # the same with an `after` start, which is then never written
    runs = (30, 35, 40, 50, 70, 80, 90)
    for p in runs:
        b.delete(p - 1, p + 2)
    ops = [ins(b.index_of(p - 2) + 1, ["x"]) for p in reversed(runs)]  # right to left: the indices to the left stay valid
    cases.append(Case("B closed form of the after slots", b.log, [with_read_out(b.vis, ops)], check=_check_closed_form(b, runs)))
    # an `after` flag set by a link made in this very call, on an element deleted later in the call, before an insert there
    b = Base(150).delete_each(range(1, 60, 4))
    i = b.index_of(60)
    ops = [mark("link", i, i + 11), dele(i + 6, 8), ins(i + 6, ["x"])]
    cases.append(Case("B after flag made in this call", b.log, [with_read_out(b.vis, ops)], check=lambda w, want=b.ids[70]: _eq(w["changes"][0]["ops"][9].get("elemId"), want)))
    return cases


def _eq(a, b):
    assert a == b, (a, b)


def _check_closed_form(b, runs):
    def check(w):
        refs = [op["elemId"] for op in w["changes"][0]["ops"][:len(runs)]]
        got = dict(zip(reversed(runs), refs))
        # which runs hold a defined `after` slot is the ORACLE's answer; what is pinned here is that the case still tells the branches apart
        taken = {p for p in runs if got[p] == b.ids[p]}
        assert all(got[p] in (b.ids[p], b.ids[p - 2]) for p in runs)
        assert {30, 35, 50, 80} <= taken and 70 not in taken, got
    return check


# ---- C. the gap opener ----
def cases_C_small():
    """every combination of n % 4 and at % 4 on a 40-element list, at = 0 and at = n included (no tombstones: index = position)"""
    return [Case("C n %d at %d" % (n, at), Base(n).log, [with_read_out(n, [ins(at, ["X"])])]) for n in (40, 41, 42, 43) for at in range(n + 1)]


C1_INDICES = (0, 1, 2, 3, 4, 255, 256, 257, 258, 259, 1023, 1024)


def case_C1():
    def check(w):
        assert len(w["changes"][0]["ops"]) == 533  # twelve inserts, 521 probes
    b = Base(1030)
    return Case("C1", b.log, [with_read_out(b.vis, [ins(i, ["X"]) for i in C1_INDICES])], check=check)


def cases_C_large():
    cases = [case_C1()]
    # the same with tombstones
    b = Base(1030).delete_each([i for i in range(1030) if i % 7 == 3]).delete(501, 504).delete(768, 773)
    v = b.vis
    idx = [0, 1, 2, 3, 4] + [b.index_of(p) for p in (254, 256, 257, 258, 259)] + [v - 1, v]
    ops, k = [], 0
    for i in idx:  # (earlier inserts move the later indices up by one each)
        ops.append(ins(i + k, ["X"]))
        k += 1
    cases.append(Case("C1 with tombstones", b.log, [with_read_out(v, ops)]))
    # a multi-value insert of 70 values: every value shifts
    b = Base(300).delete_each(range(2, 300, 5))
    cases.append(Case("C 70 values", b.log, [with_read_out(b.vis, [ins(10, ["v%d" % k for k in range(70)])])]))
    # at and n exactly 63, 64 and 65 16-byte blocks apart (one step of 64 blocks, and the first block of a second step), aligned and not
    for diff in (63, 64, 65):
        for at, n in ((8, 4 * (2 + diff)), (11, 4 * (2 + diff) + 3), (8, 4 * (2 + diff) + 3), (11, 4 * (2 + diff))):
            assert n // 4 - at // 4 == diff
            cases.append(Case("C blocks apart %d at %d n %d" % (diff, at, n), Base(n).log, [with_read_out(n, [ins(at, ["X"])])]))
    return cases


# ---- D. this call's own elements and tombstones ----
def cases_D():
    cases = []
    b = Base(100).delete_each(range(1, 80, 4))
    v = b.vis
    ops = [ins(30, list("ABCDE"))] + probes(range(27, 38), v + 5)
    ops += [dele(31, 2)]                       # two of the new elements die
    ops += [mark("link", 30, 32)]              # ends after a new element
    ops += [mark("comment", 29, 31)]           # ends after the first new element
    ops += [dele(31, 1)]                       # the link's end element dies ...
    ops += [ins(31, ["F", "G"])]               # ... and an insert there looks past the new tombstones
    ops += [mark("em", 30, 33), mark("link", 31, 33, action="removeMark")]
    cases.append(Case("D own elements", b.log, [with_read_out(v, ops)], check=_check_D_own))
    # delete count across a chunk boundary, then an insert at the same index
    b = Base(200).delete_each(range(0, 100, 3))
    i = b.index_of(59)
    assert b.vis_pos[i + 11] > 64
    cases.append(Case("D delete across a chunk", b.log, [with_read_out(b.vis, [dele(i, 12), ins(i, ["p", "q"])])]))
    b = Base(150).delete_each(range(3, 150, 9))
    cases.append(Case("D delete then insert", b.log, [with_read_out(b.vis, [dele(70, 3), ins(70, ["p", "q"]), dele(70, 1), ins(71, ["r"])])]))
    # several Changes in one call
    b = Base(100).delete_each(range(2, 100, 6))
    v = b.vis
    c1 = [ins(40, list("abc"))] + around(40, v + 3)
    c2 = [dele(41, 2), mark("link", 39, 41)] + around(40, v + 1)
    c3 = [ins(41, ["z"])]
    c3 = with_read_out(v + 1, c3)
    cases.append(Case("D several Changes", b.log, [c1, c2, c3], check=lambda w, n0=len(b.log), ctr=b.ctr, n=(len(c1) + 2, len(c2) + 1, len(c3)): _check_chain(w, n0, ctr, n)))
    return cases


def _check_D_own(w):
    ops = w["changes"][0]["ops"]
    own = [op["opId"] for op in ops[:5]]
    dels = [op for op in ops if op["action"] == "del"]
    assert len(dels) == 3 and all(d["elemId"] in own for d in dels)      # deletes that land on this call's own elements
    link = [op for op in ops if op["action"] == "addMark" and op["markType"] == "link"][0]
    assert link["end"]["elemId"] in own                                      # a link end on one of them
    late = [op for op in ops if op["action"] == "set" and op["value"] == "F"][0]
    assert late["elemId"] in own                                             # lookAfterTombstones over this call's own tombstones


def _check_chain(w, n_base, ctr, n_ops):
    ch = w["changes"]
    assert [c["seq"] for c in ch] == [n_base + 1, n_base + 2, n_base + 3]
    assert [c["deps"] for c in ch] == [{"doc1": n_base}, {"doc1": n_base + 1}, {"doc1": n_base + 2}]
    assert [len(c["ops"]) for c in ch] == list(n_ops)
    assert [c["startOp"] for c in ch] == [ctr, ctr + n_ops[0], ctr + n_ops[0] + n_ops[1]]


# ---- E. several replicas and several logs ----
def random_calls(vis, seed, comment_id="comment-new"):
    """Fixed-seed calls of one replica, one Change each: insert, delete, add / removeMark of all four types in a random order, each followed by a
    dozen probes around the edit.  Indices are drawn from the visible length, so every call is valid."""
    rnd = random.Random(seed)
    kinds = ["insert", "delete"] + [(a, m) for a in ("addMark", "removeMark") for m in ("strong", "em", "link", "comment")]
    rnd.shuffle(kinds)
    calls = []
    for kind in kinds:
        if kind == "insert":
            i = rnd.randrange(vis + 1)
            edit = ins(i, ["Q", "R", "S"][:1 + rnd.randrange(3)])
        elif kind == "delete":
            i = rnd.randrange(vis - 4)
            edit = dele(i, 1 + rnd.randrange(4))
        else:
            i = rnd.randrange(vis - 1)
            e = i + 1 + rnd.randrange(min(vis - i, 40))
            edit = mark(kind[1], i, e, action=kind[0])
            if kind[1] == "comment":
                edit["attrs"] = {"id": comment_id}
        v2 = vis_after(vis, [edit])
        calls.append([edit] + around(min(i, v2 - 1), v2, 12))
        vis = v2
    return calls


def family_E_generated():
    """ptxgen_rich_700: two documents of three replicas; EVERY replica edits, so me != 0 and the deps name the other actors"""
    gen = H._load_golden("ptxgen_rich_700.json")
    docs, calls, actors = [], [], []
    for d, doc in enumerate(gen["docs"]):
        assert len(doc["logs"]) == 3
        docs.append(doc["logs"])
        for r, log in enumerate(doc["logs"]):
            calls.append(random_calls(len(doc["expected"][r]["text"]), 100 * d + r))
            actors.append(doc["actors"][r])
    return docs, calls, actors


def family_E_mixed():
    """one batch of a 1 030-element log, a 40-element log, a log without calls and an empty log: the LDS window is sized by the largest"""
    c1 = case_C1()
    small = Base(40).delete_each((3, 17, 18))
    docs = [[c1.log], [small.log], [Base(50).delete(10, 20).log], [[]]]
    calls = [c1.calls, [with_read_out(small.vis, [ins(17, ["X", "Y"]), dele(3, 2)])], [],
             [[{"path": [], "action": "makeList", "key": "text"}, ins(0, list("hey"))] + read_out(3)]]
    return docs, calls, ["doc1", "doc1", "doc1", "zed"]


FAMILIES = {"A": cases_A, "B": cases_B, "C_small": cases_C_small, "C_large": cases_C_large, "D": cases_D}
