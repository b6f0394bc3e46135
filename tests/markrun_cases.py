"""Queries by format on a resident text view (ptx_view_mark_runs, ptx_view_mark_snippets, ptx_view_find_in_marks; peritext_amd/csrc/markrun_core.h): the cases
tests/test_emu_markruns.py (CPU emulation) and tests/test_gpu_markruns.py (the C ABI on the GPU) share.  Built on the suites and builders of tests/text_cases.py,
tests/find_cases.py and tests/slice_cases.py (imported, not edited) and one suite of its own.

Expected values never come from the code under test.  The runs are a plain loop over the ORACLE's getTextWithFormatting spans (text_cases.Want.spans): adjacent
spans whose `marks` carry the selected mark — for a link with the same url — are joined; for comments, per id, the maximal ranges of spans whose `comment` array
holds it, ordered by (rank of the id in the document, start).  A span's element range comes from slice_cases.LogView, which has asserted that the merge's rows
start where the oracle's spans do.  run_unit and run_len are sums of the Python lengths of the oracle's span texts.  A snippet's text, rows and decoded spans are
slice_cases.check_range's; the contained hits are find_cases.expect's hits filtered by a Python loop over those runs.  The cases that exist for one edge carry
their answer hand-written as well.  A second check per case is the host path a caller had before: the spans and cintervals of the downloaded range (`rows`)
coalesced with numpy must give the same runs.

Both test files hand the checks an object with the same small interface (a view on one range of one resident batch):
  .rows                                            compact wire.Results of the range
  .mark_runs(mark_type, id, cap)                   wire.MarkRuns
  .mark_snippets(mark_type, id, cap, before, after)  wire.MarkSnippets
  .find_in_marks(q, mark_type, id)                 wire.Matches (q: find_cases.Query, its cap the cap of the kept hits)
  .find(q)                                         ptx_view_find_text: wire.Matches"""
import dataclasses
import functools

import numpy as np

import find_cases as FC
import helpers as H
import slice_cases as SC
import text_cases as TC
from peritext_amd import abi, wire

ALL = 0xFFFFFFFF
ANY = abi.MARK_ANY_ID
STRONG, EM, COMMENT, LINK = abi.MARK_STRONG, abi.MARK_EM, abi.MARK_COMMENT, abi.MARK_LINK
STEP = abi.MARKRUN_STEP
Query = FC.Query
bf, af = TC.bf, TC.af
EOT = {"type": "endOfText"}


def _flag(mark_type, i, j, n):
    """strong / em on the elements [i, j) of a document of n (an inclusive mark ends `before` the next element or at endOfText)"""
    return {"action": "addMark", "markType": mark_type, "start": bf(i), "end": bf(j) if j < n else EOT}


def _link(url, i, j):
    return {"action": "addMark", "markType": "link", "attrs": {"url": url}, "start": bf(i), "end": af(j - 1)}


def _comment(cid, i, j, action="addMark"):
    return {"action": action, "markType": "comment", "attrs": {"id": cid}, "start": bf(i), "end": af(j - 1)}


def _rows(n, strong=()):
    """n characters, em on every even one — every character is its own span row —, strong on the given element ranges"""
    ops = [_flag("em", i, i + 1, n) for i in range(0, n, 2)] + [_flag("strong", i, j, n) for i, j in strong]
    return H.mini_doc(ops, first_text=TC._chars(n, n))


ROW_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129)
EMPTIES = ["a", "", "b", "", "", "c", "d", "Hello", "e"]
FIM = list("abcabcabc") + ["", "abcabc", "a", "", "b", "c"]


@functools.lru_cache(maxsize=None)
def edge_suite():
    """Single-replica documents at the edges of the 64-row step, of the url and comment id tests and of the element; NAMES gives a log's index."""
    docs = []

    def add(name, log):
        docs.append((name, log))

    add("all_deleted", H.mini_doc([{"action": "del", "elemId": TC.el(i)} for i in range(3)], first_text=TC._chars(3)))  # no span row at all, or one without elements
    for n in ROW_COUNTS:
        add("all_%d" % n, _rows(n, [(0, n)]))  # strong over ALL rows: one run, over two step edges at 129
    add("r62_65", _rows(129, [(62, 66)]))  # one run that starts in step 0 and ends in step 1
    add("two_mid", _rows(129, [(60, 63), (64, 67)]))  # an unmarked row 63 between: a run ends before the step's last row, the next starts on the step's first
    add("two_end63", _rows(129, [(60, 64), (65, 68)]))  # a run ends exactly on row 63, the step's last
    add("adjacent", _rows(129, [(60, 64), (64, 68)]))  # ... and the next starts exactly on row 64: no row between them, ONE run
    add("tail", _rows(129, [(126, 129)]))  # a run to the last row: its end is n_visible
    add("plain", _rows(70))  # no matching row
    add("alt", H.mini_doc([_flag("strong", i, i + 1, 131) for i in range(0, 131, 2)], first_text=TC._chars(131, 5)))  # 66 runs of one row
    add("far_end", _rows(140, [(0, 1), (60, 70), (130, 132)]))  # run 1 starts in step 0 and ends in step 1, run 2 in step 2: the caps 1, 2
    add("links", H.mini_doc([_link("a.com", 0, 3), _link("b.com", 3, 6), _link("a.com", 7, 11), _flag("em", 9, 10, 12)], first_text=TC._chars(12, 1)))
    add("comments", H.mini_doc([_comment("c-A", 2, 10), _comment("c-B", 6, 14), _comment("c-A", 20, 24), _comment("c-C", 26, 28), _comment("c-C", 26, 28, "removeMark")],
                               first_text=TC._chars(30, 2)))
    for n in (63, 64, 65):  # n intervals of one id, one of another
        add("cm%d" % n, H.mini_doc([_comment("z", 1, 2)] + [_comment("c-1", 2 * i, 2 * i + 1) for i in range(n)], first_text=TC._chars(2 * n + 1, 4)))
    add("empties", H.mini_doc([_flag("strong", 3, 5, len(EMPTIES)), _flag("strong", 7, 8, len(EMPTIES))], first_text=EMPTIES))
    add("fim", H.mini_doc([_flag("strong", 0, 3, len(FIM)), _flag("strong", 6, 8, len(FIM)), _flag("strong", 10, 12, len(FIM)), _flag("strong", 13, 15, len(FIM))], first_text=FIM))
    for n in (63, 64, 65):  # n kept hits and five dropped ones
        add("dense%d" % n, H.mini_doc([_flag("strong", 0, n, n + 5)], first_text=["a"] * (n + 5)))
    names = [n for n, _ in docs]
    logs = [[log] for _, log in docs]
    expected = H.oracle_apply(logs, no_patches=True)
    want = [TC.want_of_oracle(e[0]) for e in expected]
    batch = wire.encode_docs(logs)
    w = dict(zip(names, want))
    for n in ROW_COUNTS:
        assert len(w["all_%d" % n].spans) == n, "every character is its own span row"
    assert len(w["r62_65"].spans) == 129 and len(w["alt"].spans) == 131 and len(w["far_end"].spans) == 140
    assert any(s["marks"].get("comment") == [] for s in w["comments"].spans), "comment: [] is a real state"
    return TC.Suite("markrun_edges", batch, list(batch.values), want, []), {n: k for k, n in enumerate(names)}


def suites():
    return {"markrun_edges": edge_suite()[0], "failed_log": TC.failed_log_suite(), "kat": TC.kat_suite(), "text_edges": TC.edge_suite()}


# ---- the expectations ----
def _key_of(marks, mark_type):
    """What joins adjacent spans: True (strong / em), the url (link), None where the span does not carry the mark."""
    if mark_type == LINK:
        m = marks.get("link")
        return m.get("url") if m and m.get("active", True) else None
    m = marks.get("strong" if mark_type == STRONG else "em")
    return True if m and m.get("active", True) else None


def selector_id(batch, log, mark_type, sel):
    """The C ABI's id of a selector: sel None -> PTX_MARK_ANY_ID; a url -> its id in the batch's table; a comment id string -> its rank in the log's document; a
    number is taken as it is.  A url or id the batch does not have gets an id nothing has."""
    if sel is None:
        return ANY
    if isinstance(sel, int):
        return sel
    table = batch.urls if mark_type == LINK else batch.doc_comments[batch.log_doc[log]]
    return list(table).index(sel) if sel in table else len(table) + 1000


def expect_runs(suite, lv, log, mark_type, ident):
    """[(start, end, id, unit, len)] of ALL runs of the selector (mark_type, ident: the C ABI's id) in the good log `log`; lv: its slice_cases.LogView."""
    batch, w = suite.batch, lv.w
    nsp = len(w.spans)
    e_of = lambda q: lv.starts[q] if q < nsp else lv.nv  # noqa: E731  first element of span q; behind the last span: n_visible
    u_of = lambda q: w.span_unit[q] if q < nsp else len(w.units)  # noqa: E731  sum of the Python lengths of the span texts before span q
    assert [u_of(q + 1) - u_of(q) for q in range(nsp)] == [len(TC.u16(s["text"])) for s in w.spans]
    out = []
    if mark_type != COMMENT:
        q = 0
        while q < nsp:
            key = _key_of(w.spans[q]["marks"], mark_type)
            rid = 0 if key in (None, True) else list(batch.urls).index(key)
            if key is None or (mark_type == LINK and ident != ANY and rid != ident):
                q += 1
                continue
            p = q + 1
            while p < nsp and _key_of(w.spans[p]["marks"], mark_type) == key:
                p += 1
            out.append((e_of(q), e_of(p), rid, u_of(q), u_of(p) - u_of(q)))
            q = p
        return out
    ranks = batch.doc_comments[batch.log_doc[log]]
    held = [[c["id"] for c in s["marks"].get("comment", [])] for s in w.spans]
    for rank, cid in enumerate(ranks):
        if ident != ANY and rank != ident:
            continue
        q = 0
        while q < nsp:
            if cid not in held[q]:
                q += 1
                continue
            p = q + 1
            while p < nsp and cid in held[p]:
                p += 1
            out.append((e_of(q), e_of(p), rank, u_of(q), u_of(p) - u_of(q)))
            q = p
    return out


def host_runs(rows, k, mark_type, ident):
    """The host path a caller had: (start, end, id) of the runs of log k from the DOWNLOADED spans and cintervals, coalesced with numpy."""
    if mark_type == COMMENT:
        c = rows.cintervals[int(rows.cint_off[k]) : int(rows.cint_off[k + 1])]
        keep = np.ones(len(c), bool) if ident == ANY else c["id"] == ident
        return [(int(x["start"]), int(x["end"]), int(x["id"])) for x in c[keep]]
    sp = rows.spans[int(rows.span_off[k]) : int(rows.span_off[k + 1])]
    nv = int(rows.value_off[k + 1]) - int(rows.value_off[k])
    if len(sp) == 0:
        return []
    attr, start = sp["attr"].astype(np.uint32), sp["start"].astype(np.uint32)
    flag = {STRONG: abi.ATTR_STRONG, EM: abi.ATTR_EM, LINK: abi.ATTR_LINK}[mark_type]
    key = attr & np.uint32(abi.ATTR_ID_MASK) if mark_type == LINK else np.zeros(len(sp), np.uint32)
    m = (attr & np.uint32(flag)) != 0
    if mark_type == LINK and ident != ANY:
        m &= key == np.uint32(ident)
    joined = m[1:] & m[:-1] & (key[1:] == key[:-1])
    first = m & ~np.concatenate([[False], joined])
    last = m & ~np.concatenate([joined, [False]])
    ends = np.concatenate([start[1:], [nv]])
    return [(int(a), int(b), int(c)) for a, b, c in zip(start[first], ends[last], key[first])]


def check_runs(suite, rows, got, first, n, mark_type, ident, cap, status_of=None):
    """`got` (wire.MarkRuns) of the logs [first, first + n) against both expectations; ident: the id given to the call.  Returns every log's listed runs."""
    assert len(got.status) == n and len(got.n_runs) == n and len(got.run_off) == n + 1 and int(got.run_off[0]) == 0 and got.mark_type == mark_type
    listed = []
    for k in range(n):
        tag = "%s log %d type %d id %#x cap %d" % (suite.name, first + k, mark_type, ident, cap)
        st = (status_of or {}).get(first + k, suite.want[first + k].status)
        assert int(got.status[k]) == st, tag
        runs = expect_runs(suite, SC.LogView(suite, rows, first, k), first + k, mark_type, ident) if st == 0 else []
        assert int(got.n_runs[k]) == len(runs), tag
        assert got.of_log(k) == runs[:cap], tag
        if st == 0:
            assert [r[:3] for r in runs] == host_runs(rows, k, mark_type, ident), tag + ": the host path"
        if mark_type != COMMENT:
            assert all(a[1] <= b[0] and a[0] < a[1] for a, b in zip(runs, runs[1:])), "runs ascend by start and are disjoint"
        listed.append(runs[:cap])
    for f in ("run_start", "run_end", "run_id", "run_unit", "run_len"):
        assert len(getattr(got, f)) == int(got.run_off[n]), f
    return listed


def window(s, e, before, after):
    return max(s - before, 0), min(e + after, ALL)


def check_mark_snippets(suite, rows, got, first, n, mark_type, ident, cap, before, after, status_of=None):
    """`got` (wire.MarkSnippets): the runs, ONE slice per listed run in run order, match_unit.  Returns the number of snippets."""
    listed = check_runs(suite, rows, got.runs(), first, n, mark_type, ident, cap, status_of)
    plan = [[window(s, e, before, after) for s, e, _, _, _ in runs] for runs in listed]
    ns = sum(len(p) for p in plan)
    assert ns == int(got.slice_off[n]) == len(got.match_unit)
    SC.check_range(suite, rows, got, first, n, plan, status_of=status_of)
    for l in range(n):
        if not listed[l]:
            continue
        lv = SC.LogView(suite, rows, first, l)
        for j, (s, e, _, unit, length) in enumerate(listed[l]):
            k = got.index(l, j)
            a, b = lv.clamp(*plan[l][j])
            assert a <= s <= e <= b, "the snippet holds the run"
            assert int(got.match_unit[k]) == unit - lv.pre[a], "%s log %d run %d: match_unit" % (suite.name, first + l, j)
            if before == 0 and after == 0:
                assert (a, b) == (s, e) and int(got.unit_off[k + 1]) - int(got.unit_off[k]) == length, "the snippet IS the run's text"
                assert list(TC.u16(got.of_slice(k))) == [int(x) for x in lv.w.units[unit : unit + length]]
    return ns


def expect_contained(suite, rows, first, k, q, runs):
    """find_cases.expect's hits of log first + k (ALL of them) whose [hit_start, hit_end) lies inside ONE of `runs`: a plain loop."""
    _, _, hits = FC.expect(suite, rows, first, k, dataclasses.replace(q, cap=ALL))
    return [(u, s, e) for u, s, e in hits if any(rs <= s and e <= re for rs, re, _, _, _ in runs)]


def check_find_in_marks(suite, rows, got, plain, first, n, q, mark_type, ident, status_of=None):
    """`got` (wire.Matches of ptx_view_find_in_marks under q.cap) against the filtered expectation; plain: ptx_view_find_text of the same pattern, uncapped.
    Returns (kept, dropped) summed over the logs."""
    assert len(got.status) == n and len(got.n_matches) == n and len(got.hit_off) == n + 1 and int(got.hit_off[0]) == 0
    kept_all = dropped = 0
    for k in range(n):
        tag = "%s log %d pattern %r type %d id %#x cap %d" % (suite.name, first + k, q.pattern, mark_type, ident, q.cap)
        st = (status_of or {}).get(first + k, suite.want[first + k].status)
        assert int(got.status[k]) == st, tag
        runs = expect_runs(suite, SC.LogView(suite, rows, first, k), first + k, mark_type, ident) if st == 0 else []
        kept = expect_contained(suite, rows, first, k, q, runs) if st == 0 else []
        assert int(got.n_matches[k]) == len(kept), tag
        assert got.of_log(k) == kept[: q.cap], tag
        every = plain.of_log(k)
        assert set(kept) <= set(every) and int(plain.n_matches[k]) == len(every), tag + ": find_in_marks is a subset of find_text"
        if len(runs) == 1 and st == 0 and runs[0][0] == 0 and runs[0][1] == SC.LogView(suite, rows, first, k).nv:
            assert kept == every, tag + ": one run covers the log"
        kept_all, dropped = kept_all + len(kept), dropped + len(every) - len(kept)
    assert len(got.hit_unit) == len(got.hit_start) == len(got.hit_end) == int(got.hit_off[n])
    return kept_all, dropped


# ---- the cases ----
@dataclasses.dataclass
class RunCase:
    suite: str
    mark_type: int
    sel: object = None  # None: PTX_MARK_ANY_ID; a url or comment id string; a number: the id itself
    cap: int = ALL
    rng: tuple = None  # (first_log, n_logs); a name of edge_suite: that log alone; None: the whole batch
    before: int = 0
    after: int = 0
    hand: list = None  # [(start, end, id, unit, len)] of the range's first log, hand-written
    hand_snip: list = None  # [(snippet text, match_unit)] likewise


def run_cases():
    _, N = edge_suite()
    one = lambda name: (N[name], 1)  # noqa: E731
    out = []
    # span row counts 0, 1, 2, 63, 64, 65, 127, 128, 129 under strong (one run over all of them), em (a run per even row) and a mark no row has
    for mt in (STRONG, EM, LINK, COMMENT):
        for b, a in ((0, 0), (1, 1)):
            out.append(RunCase("markrun_edges", mt, before=b, after=a))
    for n in ROW_COUNTS:
        unit = n  # one unit per element
        out.append(RunCase("markrun_edges", STRONG, rng=one("all_%d" % n), hand=[(0, n, 0, 0, unit)]))
    out.append(RunCase("markrun_edges", STRONG, rng=one("r62_65"), hand=[(62, 66, 0, 62, 4)]))
    out.append(RunCase("markrun_edges", STRONG, rng=one("two_mid"), hand=[(60, 63, 0, 60, 3), (64, 67, 0, 64, 3)]))
    out.append(RunCase("markrun_edges", STRONG, rng=one("two_end63"), hand=[(60, 64, 0, 60, 4), (65, 68, 0, 65, 3)]))
    out.append(RunCase("markrun_edges", STRONG, rng=one("adjacent"), hand=[(60, 68, 0, 60, 8)]))
    out.append(RunCase("markrun_edges", STRONG, rng=one("tail"), hand=[(126, 129, 0, 126, 3)]))
    out.append(RunCase("markrun_edges", STRONG, rng=one("plain"), hand=[]))
    out.append(RunCase("markrun_edges", STRONG, rng=one("all_deleted"), hand=[]))
    out.append(RunCase("markrun_edges", EM, rng=one("all_129"), cap=3, hand=[(0, 1, 0, 0, 1), (2, 3, 0, 2, 1), (4, 5, 0, 4, 1)]))
    # links: adjacent urls are two runs, one url split by em is one; a specific url; a url the batch lacks; the largest url id (nothing has it)
    out.append(RunCase("markrun_edges", LINK, rng=one("links")))
    for sel in ("a.com", "b.com", "nowhere.org", abi.ATTR_ID_MASK):
        out.append(RunCase("markrun_edges", LINK, sel=sel, rng=one("links"), before=1, after=1))
    # comments: two ids overlapping, one id with two intervals, an id the log lacks, comment: [] in no run; 63, 64, 65 intervals of one id; (id, start) order
    for sel in (None, "c-A", "c-B", "c-C", 7):
        out.append(RunCase("markrun_edges", COMMENT, sel=sel, rng=one("comments"), after=2))
    for n in (63, 64, 65):
        for sel in (None, "c-1", "z"):
            out.append(RunCase("markrun_edges", COMMENT, sel=sel, rng=one("cm%d" % n)))
        out.append(RunCase("markrun_edges", COMMENT, sel="c-1", rng=one("cm%d" % n), cap=64))
    # caps: 66 runs of one row under 0, 1, 64, 65 and all; a cap that falls between a listed run's start step and its end step, and one before it
    for cap in (0, 1, 64, 65, ALL):
        out.append(RunCase("markrun_edges", STRONG, rng=one("alt"), cap=cap, before=1))
    out.append(RunCase("markrun_edges", STRONG, rng=one("far_end"), cap=2, hand=[(0, 1, 0, 0, 1), (60, 70, 0, 60, 10)]))
    out.append(RunCase("markrun_edges", STRONG, rng=one("far_end"), cap=1, hand=[(0, 1, 0, 0, 1)]))
    out.append(RunCase("markrun_edges", STRONG, rng=one("far_end"), hand=[(0, 1, 0, 0, 1), (60, 70, 0, 60, 10), (130, 132, 0, 130, 2)]))
    out.append(RunCase("markrun_edges", STRONG, rng=one("r62_65"), cap=1, hand=[(62, 66, 0, 62, 4)]))
    out.append(RunCase("markrun_edges", COMMENT, rng=one("comments"), cap=2))
    # mixed ranges: a failed log and run-less logs between logs with runs; a range behind log 0
    for mt in (STRONG, EM, LINK, COMMENT):
        out.append(RunCase("failed_log", mt, before=2, after=2))
        out.append(RunCase("failed_log", mt, rng=(1, 2)))
        out.append(RunCase("markrun_edges", mt, rng=(N["plain"], 6), cap=3, before=1))
        out.append(RunCase("text_edges", mt, after=1))
    # empty strings: a run made only of empty-string elements (zero units, still a run), a run of one multi-unit element
    #   a "" b "" "" c d Hello e : pre = 0 1 1 2 2 2 3 4 9 10
    out.append(RunCase("markrun_edges", STRONG, rng=one("empties"), hand=[(3, 5, 0, 2, 0), (7, 8, 0, 4, 5)], hand_snip=[("", 0), ("Hello", 0)]))
    out.append(RunCase("markrun_edges", STRONG, rng=one("empties"), before=1, after=1, hand=[(3, 5, 0, 2, 0), (7, 8, 0, 4, 5)], hand_snip=[("bc", 1), ("dHelloe", 1)]))
    out.append(RunCase("markrun_edges", STRONG, rng=one("empties"), before=2, after=0, hand_snip=[("b", 1), ("cdHello", 2)]))
    return out


def kat_run_cases():
    """The 46 known-answer documents under every selector: each flag, every link, every comment, each url of the batch, the comment ranks 0 .. 2."""
    suite = TC.kat_suite()
    out = [RunCase("kat", STRONG), RunCase("kat", EM, before=1, after=1), RunCase("kat", LINK), RunCase("kat", COMMENT)]
    out += [RunCase("kat", LINK, sel=u) for u in list(suite.batch.urls)[:4]]
    out += [RunCase("kat", COMMENT, sel=r, after=1) for r in range(3)]
    return out


def _range(case):
    suite = suites()[case.suite]
    if case.rng is None:
        return suite, 0, suite.batch.n_logs
    return (suite,) + tuple(case.rng)


def run_run_case(open_view, case):
    """open_view(suite, first, n) -> the interface of the module docstring (a context manager).  Returns (listed runs, snippets)."""
    suite, first, n = _range(case)
    ident = selector_id(suite.batch, first, case.mark_type, case.sel)
    with open_view(suite, first, n) as v:
        runs = v.mark_runs(case.mark_type, ident, case.cap)
        listed = check_runs(suite, v.rows, runs, first, n, case.mark_type, ident, case.cap)
        snip = v.mark_snippets(case.mark_type, ident, case.cap, case.before, case.after)
        ns = check_mark_snippets(suite, v.rows, snip, first, n, case.mark_type, ident, case.cap, case.before, case.after)
        for f in ("status", "n_runs", "run_off", "run_start", "run_end", "run_id", "run_unit", "run_len"):
            assert getattr(runs, f).tobytes() == getattr(snip.runs(), f).tobytes(), "both entry points list the same runs: " + f
        if case.hand is not None:
            assert runs.of_log(0) == case.hand, "the hand-written runs"
        if case.hand_snip is not None:
            assert [(t, mu) for *_, t, mu in snip.of_log(0)] == case.hand_snip, "the hand-written snippets"
        if case.cap == 0:
            assert int(runs.run_off[n]) == 0 and len(snip.text) == 0, "the count-only answer"
    return sum(len(r) for r in listed), ns


@dataclasses.dataclass
class FindCase:
    suite: str
    q: Query
    mark_type: int
    sel: object = None
    rng: tuple = None
    hand: list = None  # [(unit, start, end)] of the range's first log


def find_cases():
    _, N = edge_suite()
    one = lambda name: (N[name], 1)  # noqa: E731
    out = []
    # a hit inside a run (unit 0); one that straddles a run's edge by one element (unit 6: elements [6, 9), the run is [6, 8)); two inside ONE multi-unit marked
    # element (units 9, 12); one whose range holds an unmarked empty-string element (unit 15: elements [11, 15), element 12 is unmarked) — and unit 3, unmarked
    out.append(FindCase("markrun_edges", Query("abc"), STRONG, rng=one("fim"), hand=[(0, 0, 3), (9, 10, 11), (12, 10, 11)]))
    out.append(FindCase("markrun_edges", Query("bc"), STRONG, rng=one("fim"), hand=[(1, 1, 3), (10, 10, 11), (13, 10, 11), (16, 13, 15)]))
    out.append(FindCase("markrun_edges", Query("ABC", nocase=True, cap=2), STRONG, rng=one("fim"), hand=[(0, 0, 3), (9, 10, 11)]))
    # 63, 64 and 65 kept hits in one log (and five dropped) under the caps 0, 1, 64 and all
    for n in (63, 64, 65):
        for cap in (0, 1, 64, ALL):
            out.append(FindCase("markrun_edges", Query("a", cap=cap), STRONG, rng=one("dense%d" % n), hand=[(i, i, i + 1) for i in range(min(n, cap))]))
    # a log whose every hit is dropped; the whole batch (logs of every kind between each other); one run covers the log: equality with find_text
    out.append(FindCase("markrun_edges", Query(FC.two_letters(edge_suite()[0].want[N["plain"]].units)), STRONG, rng=one("plain"), hand=[]))
    for mt in (STRONG, EM, LINK):
        out.append(FindCase("markrun_edges", Query("a", cap=5), mt))
        out.append(FindCase("markrun_edges", Query("e"), mt, rng=(N["all_63"], 8)))
    out.append(FindCase("markrun_edges", Query("e"), LINK, sel="a.com", rng=one("links")))
    for sel in ("c-A", "c-B", "c-C", 7):
        for pat in ("e", FC.two_letters(edge_suite()[0].want[N["comments"]].units[4:10])):
            out.append(FindCase("markrun_edges", Query(pat), COMMENT, sel=sel, rng=one("comments")))
    for n in (63, 64, 65):
        out.append(FindCase("markrun_edges", Query(SC.text_of(edge_suite()[0].want[N["cm%d" % n]].units[2 * n - 2 : 2 * n - 1])), COMMENT, sel="c-1", rng=one("cm%d" % n)))
    for mt, sel in ((STRONG, None), (LINK, None), (COMMENT, 0)):
        out.append(FindCase("failed_log", FC.failed_log_queries()[0], mt, sel=sel))
        out.append(FindCase("text_edges", Query("e"), mt, sel=sel))
    return out


def kat_find_cases():
    out = []
    for i, q in enumerate(FC.kat_queries()):
        mt, sel = ((STRONG, None), (EM, None), (LINK, None), (COMMENT, 0), (COMMENT, 1))[i % 5]
        out.append(FindCase("kat", q, mt, sel=sel))
    return out


def run_find_case(open_view, case):
    """Returns check_find_in_marks' (kept, dropped)."""
    suite = suites()[case.suite]
    first, n = case.rng or (0, suite.batch.n_logs)
    ident = selector_id(suite.batch, first, case.mark_type, case.sel)
    with open_view(suite, first, n) as v:
        got = v.find_in_marks(case.q, case.mark_type, ident)
        plain = v.find(dataclasses.replace(case.q, cap=ALL))
        counts = check_find_in_marks(suite, v.rows, got, plain, first, n, case.q, case.mark_type, ident)
        if case.hand is not None:
            assert got.of_log(0) == case.hand, "the hand-written hits"
    return counts


def invalid_selectors():
    """(mark_type, id, find only) of every invalid selector the header names."""
    return [(4, ANY, False), (0xFFFFFFFF, ANY, False), (STRONG, 0, False), (EM, 5, False), (LINK, abi.ATTR_ID_MASK + 1, False), (LINK, 0xFFFFFFFE, False), (COMMENT, ANY, True)]
