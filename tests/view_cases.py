"""Resident text views (ptx_text_view_create and the ptx_view_* queries; peritext_amd/csrc/view_core.h): the cases tests/test_emu_view.py (CPU emulation) and
tests/test_gpu_view.py (the C ABI on the GPU) share.  Built on the suites and builders of tests/find_cases.py, tests/slice_cases.py and tests/text_cases.py
(imported, not edited).

Expected values never come from the code under test.  The hits are find_cases.expect's: a plain loop over the oracle's u16 text, element boundaries from
table[values[i]] of the merge's result.  A snippet's window is [hit_start - before, hit_end + after) computed here with Python integers and cut to 32 bits; its
text, rows and decoded spans are slice_cases.check_range's: Python slices of the oracle's text between element boundaries, the oracle's spans cut by a plain
loop.  match_unit is hit_unit minus the boundary of the snippet's first element, and the pinned identity — the snippet holds the pattern there — is asserted on
every snippet of every case.  The cases that exist for one edge carry their answer hand-written as well.

Both test files hand `run_case` and `view_session` an object with the same small interface (a view and its twins on one range of one resident batch):
  .rows                       compact wire.Results of the range (ptx_result_download_range / its emulation twin)
  .find(q)  .slices(plan)  .snippets(q, before, after)            the view's queries: wire.Matches, wire.Slices, wire.Snippets
  .twin_find(q)  .twin_slices(plan)                               ptx_result_find_text / ptx_result_text_slices over the same range"""
import dataclasses

import numpy as np

import find_cases as FC
import slice_cases as SC
import text_cases as TC

S, T = FC.S, FC.T
ALL = 0xFFFFFFFF
Query = FC.Query
WINDOWS = (0, 1, 3, ALL)


@dataclasses.dataclass
class Case:
    suite: str  # a key of suites()
    q: Query
    before: int
    after: int
    tag: str = ""


def suites():
    return {"find_edges": FC.edge_suite()[0], "slice_edges": SC.edge_suite()[0], "text_edges": TC.edge_suite(), "failed_log": TC.failed_log_suite(), "kat": TC.kat_suite()}


def window(s, e, before, after):
    """[s - before, e + after) saturated at 0 and at 0xFFFFFFFF."""
    return max(s - before, 0), min(e + after, ALL)


def check_same(a, b, fields):
    """Two results field by field, bit for bit (kernel_ms excepted)."""
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f


MATCH_FIELDS = ("status", "n_matches", "hit_off", "hit_unit", "hit_start", "hit_end")
SLICE_FIELDS = ("status", "slice_off", "elem_start", "elem_end", "unit_off", "text", "sspan_off", "sspans", "sspan_unit")


def check_snippets(suite, rows, got, first, n, q, before, after, status_of=None, decode=True):
    """`got` (wire.Snippets) of the logs [first, first + n) against the expectations; returns (number of snippets, of those cut at element 0, of those cut at the
    log's end)."""
    FC.check_range(suite, rows, got.matches(), first, n, q, status_of)
    listed = [FC.expect(suite, rows, first, k, q, (status_of or {}).get(first + k))[2] for k in range(n)]
    plan = [[window(s, e, before, after) for _, s, e in hits] for hits in listed]
    ns = sum(len(p) for p in plan)
    assert ns == int(got.slice_off[n]) and len(got.match_unit) == ns and got.n_pattern == len(TC.u16(q.pattern))
    SC.check_range(suite, rows, got, first, n, plan, status_of=status_of, decode=decode)
    pat = TC.u16(q.pattern).astype(np.uint16)
    at_start = at_end = 0
    for l in range(n):
        if not listed[l]:
            continue
        view = SC.LogView(suite, rows, first, l)
        prev = -1
        for j, (u, s, e) in enumerate(listed[l]):
            k = got.index(l, j)
            a, b = view.clamp(*plan[l][j])
            assert a <= s < e <= b, "the snippet holds the hit's elements"
            at_start += s - before < 0
            at_end += e + after > view.nv
            mu = int(got.match_unit[k])
            assert mu == u - view.pre[a], "%s log %d hit %d: match_unit" % (suite.name, first + l, j)
            seg = got.text[int(got.unit_off[k]) + mu : int(got.unit_off[k]) + mu + len(pat)]
            assert int(got.unit_off[k]) + mu + len(pat) <= int(got.unit_off[k + 1]), "the match lies inside its snippet"
            if q.nocase:
                assert np.array_equal(FC.fold(seg), FC.fold(pat)), "the pinned identity, folded"
            else:
                assert np.array_equal(seg, pat), "the pinned identity"
            assert a >= prev, "snippets stay in hit order"
            prev = a
    return ns, at_start, at_end


def _range_of(suite, q):
    return q.rng or (0, suite.batch.n_logs)


def cases():
    """Every shared snippet case."""
    _, N = FC.edge_suite()
    _, SN = SC.edge_suite()
    dense = 2 * S + 1
    out = []
    # locate: every query of the find tests (unit 0, the last unit, inside and across a multi-unit element, behind and across empty strings, the last element, the
    # astral character whole and split under the pair and either surrogate, tile edges, caps, a range behind log 0, folding), each under a pair of WINDOWS in turn
    pairs = [(b, a) for b in WINDOWS for a in WINDOWS]
    for i, q in enumerate(FC.edge_queries()):
        b, a = pairs[i % len(pairs)]
        out.append(Case("find_edges", q, b, a, "edge query %d" % i))
    # windows: every pair on the queries whose hits sit at unit 0, at the last unit and behind empty strings: saturation at 0, at n_visible, and past 32 bits
    for b, a in pairs:
        out.append(Case("find_edges", Query("q", rng=(N["positions"], 2)), b, a, "positions"))
        out.append(Case("find_edges", Query("b", rng=(N["empties"], 1)), b, a, "empties"))
    # 2S + 1 x "a" under "aa": overlapping snippets, in order, at the caps
    for cap in (0, 1, 64, 65, ALL):
        out.append(Case("find_edges", Query("aa", cap=cap, rng=(N["dense"], 1), want_counts={N["dense"]: dense - 1}), 1, 1, "dense aa cap %d" % cap))
    # 63, 64, 65 and 257 listed hits in total: the edges of a lane per hit
    for cap in (63, 64, 65, 257):
        out.append(Case("find_edges", Query("a", cap=cap, rng=(N["dense"], 1), want_counts={N["dense"]: dense}), 3, 0, "%d hits in total" % cap))
    # match_unit where elem_start is a multi-unit element; the hand-written answers are in hand_checks
    out.append(Case("find_edges", Query("y", rng=(N["multi"], 1), want_counts={N["multi"]: 1}), 1, 0, "multi y"))
    out.append(Case("find_edges", Query("world", rng=(N["multi"], 1), want_counts={N["multi"]: 1}), 0, 1, "multi world"))
    out.append(Case("find_edges", Query("hELLO", nocase=True, rng=(N["multi"], 1), want_counts={N["multi"]: 1}), 3, 3, "multi hELLO"))
    # spans: a snippet cut exactly on a span start, inside one span, and over all three rows
    out.append(Case("slice_edges", Query("f", rng=(SN["spans"], 1)), 0, 2, "spans f"))
    out.append(Case("slice_edges", Query("h", rng=(SN["spans"], 1)), 1, 1, "spans h"))
    out.append(Case("slice_edges", Query("gh", rng=(SN["spans"], 1)), ALL, ALL, "spans gh"))
    # logs of 0, 1, T - 1, T, T + 1 and 2T + 1 elements, long values, a comment and a link under the snippets (decoded through decode_slice_spans)
    for i, q in enumerate(FC.text_edge_queries()):
        b, a = ((3, 3), (ALL, 0), (0, ALL), (1, 1))[i % 4]
        out.append(Case("text_edges", q, b, a, "text edge query %d" % i))
    names = TC.edge_docs()[0]
    bold = TC.edge_suite().want[names.index("alternating_bold")].units
    for at in (64, 110):  # inside the comment (elements 60 .. 70), inside the link (100 .. 127)
        pat = SC.text_of(bold[at : at + 2])
        out.append(Case("text_edges", Query(pat, rng=(names.index("alternating_bold"), 1)), 3, 3, "alternating_bold %d" % at))
    out.append(Case("text_edges", Query("e", rng=(names.index("n63"), 4)), 3, 1, "a range behind log 0"))
    # a failed log, and logs without hits, between logs with hits
    for q in FC.failed_log_queries():
        out.append(Case("failed_log", q, 1, 3, "failed log"))
    return out


def kat_cases():
    """The 46 known-answer documents: snippets of two letters of their own text with one element of context."""
    return [Case("kat", q, 1, 1, "kat %d" % i) for i, q in enumerate(FC.kat_queries())]


def run_case(open_view, case):
    """open_view(suite, first, n) -> the interface of the module docstring (a context manager).  Returns check_snippets' counts."""
    suite = suites()[case.suite]
    first, n = _range_of(suite, case.q)
    with open_view(suite, first, n) as v:
        got = v.snippets(case.q, case.before, case.after)
        counts = check_snippets(suite, v.rows, got, first, n, case.q, case.before, case.after)
        check_same(got.matches(), v.twin_find(case.q), MATCH_FIELDS)  # the second check, not the only one
        plan = [[window(s, e, case.before, case.after) for _, s, e in got.matches().of_log(k)] for k in range(n)]
        check_same(got, v.twin_slices(plan), SLICE_FIELDS)
        hand_checks(case, got)
    return counts


def hand_checks(case, got):
    """The hand-written answers of the cases that exist for one edge: got.of_log = [(unit, start, end, snippet, match_unit)]."""
    g = got.of_log(0)
    if case.tag == "multi y":  # ["x", "Hello, world", "y", "z"]: the snippet starts with the twelve-unit element, so the match is at unit 12, not at 1
        assert g == [(13, 2, 3, "Hello, worldy", 12)]
    elif case.tag == "multi world":  # inside one multi-unit element: hit_end == hit_start + 1, and the offset inside it survives
        assert g == [(8, 1, 2, "Hello, worldy", 7)]
    elif case.tag == "multi hELLO":
        assert g == [(1, 1, 2, "xHello, worldyz", 1)]
    elif case.tag == "spans f":  # exactly on the start of the bold span [5, 10)
        assert g == [(5, 5, 6, "fgh", 0)] and got.rows_of_slice(0) == [(5, SC.STRONG, 0)]
    elif case.tag == "spans h":  # inside it
        assert g == [(7, 7, 8, "ghi", 1)] and got.rows_of_slice(0) == [(6, SC.STRONG, 0)]
    elif case.tag == "spans gh":  # both ends saturate: the whole log and its three rows
        assert g == [(6, 6, 8, "abcdefghijklmnopqrst", 6)] and got.rows_of_slice(0) == [(0, 0, 0), (5, SC.STRONG, 5), (10, 0, 10)]
    elif case.tag == "empties" and (case.before, case.after) == (1, 0):  # ["a", "", "b", ...]: "b" is element 2; one element before it is the EMPTY string
        assert g == [(1, 2, 3, "b", 0)] and (int(got.elem_start[0]), int(got.elem_end[0])) == (1, 3)
    elif case.tag == "empties" and (case.before, case.after) == (3, ALL):
        assert g == [(1, 2, 3, "abcd", 1)] and (int(got.elem_start[0]), int(got.elem_end[0])) == (0, 7)
    elif case.tag == "positions" and (case.before, case.after) == (3, 3):  # hits at units 0 and S + 40 (the last): cut at 0 and at n_visible
        assert g[0] == (0, 0, 1, "qxxx", 0) and g[-1] == (S + 40, S + 40, S + 41, "xxxq", 3)
    elif case.tag.startswith("dense aa cap") and case.q.cap >= 64:  # overlapping hits give overlapping snippets; nothing is merged
        assert g[0] == (0, 0, 2, "aaa", 0) and g[1] == (1, 1, 3, "aaaa", 1) and g[63] == (63, 63, 65, "aaaa", 1)
        assert len(g) == min(case.q.cap, 2 * S)
    elif case.tag.endswith("hits in total"):
        assert len(g) == case.q.cap == int(got.slice_off[-1]) and g[-1] == (case.q.cap - 1, case.q.cap - 1, case.q.cap, "aaaa", 3)


def view_session(v, suite, first, n):
    """Two patterns, then slices, then the first pattern again on ONE view: the first and the last answer are bit-equal, and every answer is right."""
    qa, qb = Query("a"), Query("aa", cap=5)
    first_a = v.snippets(qa, 2, 2)
    check_snippets(suite, v.rows, first_a, first, n, qa, 2, 2)
    check_snippets(suite, v.rows, v.snippets(qb, 0, ALL), first, n, qb, 0, ALL)
    m = v.find(qb)
    FC.check_range(suite, v.rows, m, first, n, qb)
    check_same(m, v.twin_find(qb), MATCH_FIELDS)
    plan = SC.plan_sparse(v.rows, n)
    cut = v.slices(plan)
    SC.check_range(suite, v.rows, cut, first, n, plan)
    check_same(cut, v.twin_slices(plan), SLICE_FIELDS)
    again = v.snippets(qa, 2, 2)
    check_same(first_a, again, SLICE_FIELDS + ("n_matches", "hit_unit", "hit_start", "hit_end", "match_unit"))
