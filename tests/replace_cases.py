"""Find and replace on resident text views (ptx_view_replace_plan; peritext_amd/csrc/replace_core.h): the cases tests/test_emu_replace.py (CPU emulation),
tests/test_gpu_replace.py (the C ABI on the GPU) and the Node pair share.  Built on the suites and builders of tests/find_cases.py and tests/text_cases.py
(imported, not edited) and one suite of its own.

Expected values never come from the code under test.  The matches are find_cases.expect's: a plain loop over the oracle's u16 text, element ranges from
table[values[i]] of the merge's result.  The chosen matches are a sequential greedy loop over them (the first, then the first at or behind the end of the last
chosen one: String.prototype.replaceAll, str.replace); a chosen match is replaceable iff Python prefix sums of the elements' lengths say that it starts and ends
on element boundaries; the ops are written out in descending order, a delete and — with a replacement — an insert each; the element list after the edit is
Python list surgery with those ops.  Where every element of a log is one code unit, the joined list must ALSO equal text.replace(pattern, replacement) (a folded
plain loop under NOCASE): the pinned identity.  The cases that exist for one edge carry their answer hand-written as well.

S = abi.REPLACE_TILE, the hits of one step of the select walk.

Both test files hand `run_ask` an object with this small interface (a view on one range of one resident batch):
  .rows                           compact wire.Results of the range
  .replace_plan(ask, n_batch)     wire.ReplacePlan of the view (ask.ids: the replacement's value ids)
  .find(q)                        the view's ptx_view_find_text twin: wire.Matches"""
import dataclasses
import functools

import numpy as np

import find_cases as FC
import helpers as H
import text_cases as TC
from peritext_amd import abi, wire

S = abi.REPLACE_TILE
ROWS_MAX = abi.CHANGE_ROWS_MAX
ALL = 0xFFFFFFFF
CHAIN = (0, 1, 2, 3, S - 1, S, S + 1, 2 * S, 2 * S + 1, 4 * S + 3)


@dataclasses.dataclass
class Ask:
    suite: str  # a key of suites()
    pattern: str
    replacement: tuple  # the replacement's element strings
    nocase: bool = False
    rng: tuple = None  # (first_log, n_logs); None: the whole batch
    want: dict = None  # {log: (n_matches, n_chosen, n_replaced)} hand-written: what the case is there for
    want_ops: dict = None  # {log: [(action, index, count)]} hand-written
    want_status: dict = None  # {log: status} hand-written
    tag: str = ""

    @property
    def query(self):
        return FC.Query(self.pattern, nocase=self.nocase)


def _fill(n):
    return ["x"] * n


@functools.lru_cache(maxsize=None)
def edge_suite():
    """Single-replica documents at the edges of the select walk; the second value gives a log's index by name."""
    docs = []

    def add(name, values):
        docs.append((name, H.mini_doc([], first_text=values)))

    # overlap chains across tile edges: n x "a" (n = 0: everything deleted)
    for n in CHAIN:
        if n == 0:
            docs.append(("chain0", H.mini_doc([{"action": "del", "elemId": TC.el(i)} for i in range(2)], first_text=list("aa"))))
        else:
            add("chain%d" % n, ["a"] * n)
    add("abab", list("ab" * (S + 3)) + ["a"])  # "aba" at every even unit: the chosen ones are every other match, S + 3 matches in all
    # 63, 64, 65 and 129 non-overlapping hits of "ay" in one log
    for k in (S - 1, S, S + 1, 2 * S + 1):
        add("hits%d" % k, ["a", "y"] * k)
    # twenty separate "aa", then a run of 100 x "a" that begins in the first tile of hits and ends in the second, then one more "aa"
    add("run_over_edge", ["a", "a", "x"] * 20 + ["a"] * 100 + ["x", "a", "a"])
    # "xyaaaz": "aa" at unit 2 starts inside "ya" — chosen, skipped — and blocks the match at unit 3, which covers the whole elements "a", "a"
    add("blocked", ["x", "ya", "a", "a", "z"])
    # multi-unit elements under "ab" / "abcd"
    add("multi_inside", ["x", "cabd", "y"])
    add("multi_end_inside", ["x", "a", "bc"])
    add("multi_start_inside", ["ca", "b", "x"])
    add("multi_one", ["x", "ab", "y"])
    add("multi_two", ["x", "ab", "cd", "y"])
    # empty-string elements before, inside and after the match "ab"
    add("empties", ["", "a", "", "b", "", "c"])
    # a match at unit 0 and at the last unit
    add("positions", ["a", "b", "x", "x", "a", "b"])
    # folding: "AB", "aB" under "ab" with NOCASE
    add("case", ["A", "B", "x", "a", "B", "b"])
    # capacity: one match of "Q" each in a three-element log and its neighbours: two matches before it, none behind it
    add("cap_two", ["Q", "x", "Q"])
    add("cap_log", ["Q", "x", "x"])
    add("cap_none", ["x", "y", "z"])
    names = [n for n, _ in docs]
    logs = [[log] for _, log in docs]
    want = [TC.want_of_oracle(e[0]) for e in H.oracle_apply(logs, no_patches=True)]
    batch = wire.encode_docs(logs)
    N = {n: k for k, n in enumerate(names)}
    assert len(want[N["chain0"]].units) == 0 and len(want[N["chain%d" % (4 * S + 3)]].units) == 4 * S + 3 and len(want[N["blocked"]].units) == 6
    return TC.Suite("replace_edges", batch, list(batch.values), want, []), N


def suites():
    return {"replace_edges": edge_suite()[0], "failed_log": TC.failed_log_suite(), "kat": TC.kat_suite()}


DEL, INS = abi.IN_DELETE, abi.IN_INSERT


def asks():
    _, N = edge_suite()
    out = []
    # chains: n x "a" under "aa" and "aaa" — floor(n / m) chosen, all of them whole elements; the neighbours' hits ("run_over_edge", "blocked") ride along
    for m in (2, 3):
        want = {N["chain%d" % n]: (max(n - m + 1, 0), n // m, n // m) for n in CHAIN}
        if m == 2:
            want[N["run_over_edge"]] = (20 + 99 + 1, 20 + 50 + 1, 20 + 50 + 1)
            want[N["blocked"]] = (2, 1, 0)
        out.append(Ask("replace_edges", "a" * m, ("b",), want=want, tag="chains %d" % m))
    out.append(Ask("replace_edges", "aba", ("c", "d"), want={N["abab"]: (S + 3, (S + 4) // 2, (S + 4) // 2)}, tag="abab"))
    # hit counts at the tile's edges
    out.append(Ask("replace_edges", "ay", ("z",), want={N["hits%d" % k]: (k, k, k) for k in (S - 1, S, S + 1, 2 * S + 1)}, tag="hit counts"))
    # multi-unit elements
    out.append(Ask("replace_edges", "ab", ("Z",), tag="multi ab",
                   want={N["multi_inside"]: (1, 1, 0), N["multi_end_inside"]: (1, 1, 0), N["multi_start_inside"]: (1, 1, 0), N["multi_one"]: (1, 1, 1), N["multi_two"]: (1, 1, 1),
                         N["empties"]: (1, 1, 1), N["positions"]: (2, 2, 2), N["case"]: (0, 0, 0)},
                   want_ops={N["multi_one"]: [(DEL, 1, 1), (INS, 1, 1)], N["empties"]: [(DEL, 1, 3), (INS, 1, 1)],
                             N["positions"]: [(DEL, 4, 2), (INS, 4, 1), (DEL, 0, 2), (INS, 0, 1)], N["multi_inside"]: []}))
    out.append(Ask("replace_edges", "abcd", ("Z", "Y"), want={N["multi_two"]: (1, 1, 1), N["multi_inside"]: (0, 0, 0)},
                   want_ops={N["multi_two"]: [(DEL, 1, 2), (INS, 1, 2)]}, tag="multi abcd"))
    out.append(Ask("replace_edges", "ab", ("Z",), nocase=True, want={N["case"]: (2, 2, 2), N["positions"]: (2, 2, 2)},
                   want_ops={N["case"]: [(DEL, 3, 2), (INS, 3, 1), (DEL, 0, 2), (INS, 0, 1)]}, tag="nocase"))
    # replacements: empty (delete only), one element, longer than the pattern, containing the pattern, a multi-unit element
    for rep in ((), ("b",), ("x", "y", "z"), ("a", "a", "a"), ("aa",)):
        out.append(Ask("replace_edges", "aa", rep, rng=(N["chain3"], 5), want={N["chain%d" % (S + 1)]: (S, (S + 1) // 2, (S + 1) // 2)},
                       want_ops={N["chain3"]: [(DEL, 0, 2)] + ([(INS, 0, len(rep))] if rep else [])}, tag="replacement %r" % (rep,)))
    # capacity: 1 + 65 533 = 65 534 rows is the most a log may make
    for nrep, st in ((ROWS_MAX - 1, 0), (ROWS_MAX, abi.ERR_CAPACITY)):
        out.append(Ask("replace_edges", "Q", ("z",) * nrep, rng=(N["cap_two"], 3), want={N["cap_two"]: (2, 2, 2), N["cap_log"]: (1, 1, 1), N["cap_none"]: (0, 0, 0)},
                       want_status={N["cap_two"]: abi.ERR_CAPACITY, N["cap_log"]: st, N["cap_none"]: 0}, tag="capacity %d" % nrep))
    # a failed log, and logs without hits, between logs with hits; a view behind log 0 of a batch that goes on behind it
    for q in FC.failed_log_queries():
        out.append(Ask("failed_log", q.pattern, ("R",), rng=q.rng, tag="failed log"))
    out.append(Ask("replace_edges", "aa", ("b",), rng=(N["chain2"], 4), tag="a range inside the batch"))
    return out


def kat_asks():
    """The 46 known-answer documents under two patterns: the most frequent letter of English, and a two-letter pattern of the first document's own text."""
    two = FC.kat_queries()[0].pattern
    return [Ask("kat", "e", ("E",), tag="kat e"), Ask("kat", two, ("<", ">"), nocase=True, tag="kat two letters")]


def ids_of(suite, ask):
    """(the suite's string table extended by the replacement's strings, the replacement's value ids): what Engine.replace_text does with batch.values."""
    table = list(suite.table)
    ix = {v: i for i, v in enumerate(table)}
    ids = []
    for v in ask.replacement:
        if v not in ix:
            ix[v] = len(table)
            table.append(v)
        ids.append(ix[v])
    return table, np.asarray(ids, dtype=np.uint32)


def greedy(listed, m):
    """The leftmost non-overlapping ones of [(unit, start, end)], sequentially."""
    chosen, limit = [], 0
    for u, s, e in listed:
        if u >= limit:
            chosen.append((u, s, e))
            limit = u + m
    return chosen


def fold_str(s):
    return "".join(chr(ord(c) + 0x20) if "A" <= c <= "Z" else c for c in s)


def replace_all(text, pattern, replacement, nocase):
    """str.replace by a plain loop, ASCII-folded where asked."""
    if not nocase:
        return text.replace(pattern, replacement)
    ft, fp, out, i = fold_str(text), fold_str(pattern), [], 0
    while i < len(text):
        if ft.startswith(fp, i):
            out.append(replacement)
            i += len(pattern)
        else:
            out.append(text[i])
            i += 1
    return "".join(out)


def expect(suite, rows, first, k, ask):
    """dict(status, n_matches, n_chosen, n_replaced, ops: [InputOperation dicts], after: the element strings after the edit) of log first + k."""
    st, count, listed = FC.expect(suite, rows, first, k, ask.query)
    m, nrep = len(TC.u16(ask.pattern)), len(ask.replacement)
    if st != 0:
        return dict(status=st, n_matches=0, n_chosen=0, n_replaced=0, ops=[], after=None)
    elems = [suite.table[int(i)] for i in rows.values[int(rows.value_off[k]) : int(rows.value_off[k + 1])]]
    pre = [0]
    for s in elems:
        pre.append(pre[-1] + len(TC.u16(s)))
    chosen = greedy(listed, m)
    whole = [(u, s, e) for u, s, e in chosen if pre[s] == u and pre[e] == u + m]
    made = sum(e - s for _, s, e in whole) + len(whole) * nrep
    if made > ROWS_MAX:
        return dict(status=abi.ERR_CAPACITY, n_matches=count, n_chosen=len(chosen), n_replaced=len(whole), ops=[], after=elems)
    ops, after = [], list(elems)
    for u, s, e in reversed(whole):
        ops.append({"path": ["text"], "action": "delete", "index": s, "count": e - s})
        del after[s:e]
        if nrep:
            ops.append({"path": ["text"], "action": "insert", "index": s, "values": list(ask.replacement)})
            after[s:s] = list(ask.replacement)
    if all(len(TC.u16(s)) == 1 for s in elems):  # the pinned identity: every chosen match covers whole elements, so the edit IS replaceAll
        assert len(whole) == len(chosen)
        assert "".join(after) == replace_all("".join(elems), ask.pattern, "".join(ask.replacement), ask.nocase), "%s log %d" % (suite.name, first + k)
    return dict(status=0, n_matches=count, n_chosen=len(chosen), n_replaced=len(whole), ops=ops, after=after)


def check_plan(suite, rows, plan, first, n, n_batch, ask, table):
    """`plan` (wire.ReplacePlan) of the logs [first, first + n) of a batch of n_batch logs against the expectations; returns (Changes, replaced matches, skipped
    matches)."""
    for f in ("status", "n_matches", "n_chosen", "n_replaced"):
        assert len(getattr(plan, f)) == n and getattr(plan, f).dtype == np.uint32, f
    o = plan.ops
    assert len(o.chg_off) == n_batch + 1 and int(o.chg_off[0]) == 0 and int(o.op_off[0]) == 0 and len(o.op_off) == int(o.chg_off[n_batch]) + 1
    assert plan.n_pattern == len(TC.u16(ask.pattern)) and plan.n_replacement == len(ask.replacement)
    _, ids = ids_of(suite, ask)
    assert np.array_equal(o.values, ids), "`values` is the caller's ids once"
    ni = int(o.op_off[-1])
    for col in (o.action, o.mark_type, o.index, o.count, o.payload):
        assert len(col) == ni
    assert not o.mark_type.any() and not o.payload.any(), "every insert points at the shared values"
    per_log = plan.per_log(table)
    assert len(per_log) == n_batch
    changes = replaced = skipped = 0
    for b in range(n_batch):
        if not first <= b < first + n:
            assert per_log[b] == [], "a log outside the view's range makes no Change"
            continue
        k, tag = b - first, "%s log %d %r -> %r" % (suite.name, b, ask.pattern, ask.replacement[:4])
        w = expect(suite, rows, first, k, ask)
        got = (int(plan.status[k]), int(plan.n_matches[k]), int(plan.n_chosen[k]), int(plan.n_replaced[k]))
        assert got == (w["status"], w["n_matches"], w["n_chosen"], w["n_replaced"]), tag
        if ask.want and b in ask.want:
            assert got[1:] == ask.want[b], tag + ": the case's own counts"
        if ask.want_status and b in ask.want_status:
            assert got[0] == ask.want_status[b], tag + ": the case's own status"
        assert per_log[b] == ([w["ops"]] if w["ops"] else []), tag
        assert plan.ops_of_log(k, table) == w["ops"], tag
        if ask.want_ops and b in ask.want_ops:
            flat = [(DEL if op["action"] == "delete" else INS, op["index"], op.get("count", len(op.get("values", ())))) for op in w["ops"]]
            assert flat == ask.want_ops[b], tag + ": the case's own ops"
        changes += bool(w["ops"])
        replaced += w["n_replaced"]
        skipped += w["n_chosen"] - w["n_replaced"]
    return changes, replaced, skipped


def range_of(suite, ask):
    return ask.rng or (0, suite.batch.n_logs)


def run_ask(open_view, ask):
    """open_view(suite, first, n) -> the interface of the module docstring (a context manager).  Returns check_plan's counts."""
    suite = suites()[ask.suite]
    first, n = range_of(suite, ask)
    nb = suite.batch.n_logs
    table, _ = ids_of(suite, ask)
    with open_view(suite, first, n) as v:
        plan = v.replace_plan(ask, nb)
        counts = check_plan(suite, v.rows, plan, first, n, nb, ask, table)
        m = v.find(ask.query)  # the second check, not the only one: the plan's matches are the view's find
        assert np.array_equal(plan.status == abi.ERR_CAPACITY, (plan.status != m.status)) and np.array_equal(plan.n_matches, m.n_matches)
        for k in range(n):
            assert int(plan.n_chosen[k]) == len(greedy(m.of_log(k), plan.n_pattern)), "the greedy choice over the view's own hits"
    return counts
