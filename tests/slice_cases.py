"""Text and span rows of element ranges on the device (ptx_result_text_slices; peritext_amd/csrc/slice_core.h): the cases tests/test_emu_slices.py (CPU emulation)
and tests/test_gpu_slices.py (the C ABI on the GPU) share.  Built on the suites of tests/text_cases.py (imported, not edited) and one suite of its own.

Expected values never come from the code under test.  A log's text is the oracle's "".join(span.text) (text_cases.Want.units; the reference-held literal for the
46 known-answer documents).  Element boundaries come from the lengths of table[values[i]] of the MERGE's result — the merge is not changed here — after `LogView`
has asserted that their join equals the oracle's text and that the merge's span rows start where the oracle's spans do.  A slice's expected text is a plain Python
slice of the oracle's text between two of those boundaries; its expected rows are a plain loop that cuts the oracle's spans ({text, marks}) to the slice.  The
cases that exist for one particular edge carry their answer hand-written as well.  Edge sizes come from abi.TEXT_TILE (T) and abi.SLICE_BLOCK (B)."""
import dataclasses
import functools

import numpy as np

import helpers as H
import text_cases as TC
from peritext_amd import abi, wire

T, B = abi.TEXT_TILE, abi.SLICE_BLOCK
ALL = 0xFFFFFFFF
STRONG = abi.ATTR_STRONG


def text_of(units):
    return np.asarray(units).astype("<u2").tobytes().decode("utf-16-le", "surrogatepass")


class LogView:
    """What the expectations of one good log are cut from: the oracle's text and spans, element boundaries from the merge's value ids."""

    def __init__(self, suite, res, first, k):
        self.w = w = suite.want[first + k]
        ids = res.values[int(res.value_off[k]) : int(res.value_off[k + 1])]
        parts = [TC.u16(suite.table[int(i)]) for i in ids]
        joined = np.concatenate(parts + [np.zeros(0, "<u2")])
        assert len(joined) == len(w.units) and np.array_equal(joined, w.units), "the elements' strings join to the oracle's text"
        self.nv = len(parts)
        self.pre = [0] * (self.nv + 1)  # exclusive scan: pre[e] = first unit of element e
        for e, p in enumerate(parts):
            self.pre[e + 1] = self.pre[e] + len(p)
        rows = res.spans[int(res.span_off[k]) : int(res.span_off[k + 1])]
        self.starts = [int(r["start"]) for r in rows]
        self.attrs = [int(r["attr"]) for r in rows]
        assert len(rows) == len(w.spans) and [self.pre[s] for s in self.starts] == w.span_unit, "the merge's span rows start where the oracle's spans do"
        self.cints = [(int(c["start"]), int(c["end"])) for c in res.cintervals[int(res.cint_off[k]) : int(res.cint_off[k + 1])]]

    def clamp(self, s, e):
        a, b = min(s, self.nv), min(e, self.nv)
        return (a, a) if a >= b else (a, b)

    def cut(self, s, e):
        """(a, b, units, [(start, attr, unit)], FormatSpanWithText[]) of the slice (s, e)."""
        a, b = self.clamp(s, e)
        units = self.w.units[self.pre[a] : self.pre[b]]
        rows, spans = [], []
        for q, s0 in enumerate(self.starts):
            s1 = self.starts[q + 1] if q + 1 < len(self.starts) else self.nv
            if a < b and s0 < b and s1 > a:
                lo, hi = max(s0, a), min(s1, b)
                rows.append((lo, self.attrs[q], self.pre[lo] - self.pre[a]))
                whole = TC.u16(self.w.spans[q]["text"])  # the oracle's span, cut to the slice
                spans.append({"text": text_of(whole[self.pre[lo] - self.pre[s0] : self.pre[hi] - self.pre[s0]]), "marks": self.w.spans[q]["marks"]})
        return a, b, units, rows, spans


def check_range(suite, res, got, first, n, plan, status_of=None, decode=True):
    """`got` (wire.Slices) of the logs [first, first + n) against the expectations; plan[k] = [(start, end)] of log first + k; res: the compact wire.Results of
    the range; status_of: {log: status} overrides (a text-only failure)."""
    ns = sum(len(p) for p in plan)
    assert len(got.status) == n and len(got.elem_start) == len(got.elem_end) == ns and len(got.unit_off) == len(got.sspan_off) == ns + 1
    assert int(got.unit_off[0]) == 0 and int(got.sspan_off[0]) == 0
    assert len(got.text) == int(got.unit_off[ns]) and len(got.sspans) == len(got.sspan_unit) == int(got.sspan_off[ns])
    sub = dataclasses.replace(suite.batch, log_doc=suite.batch.log_doc[first:])
    k = 0
    for l in range(n):
        st = (status_of or {}).get(first + l, suite.want[first + l].status)
        assert int(got.status[l]) == st, "%s log %d" % (suite.name, first + l)
        view = LogView(suite, res, first, l) if st == 0 else None
        for j, (s, e) in enumerate(plan[l]):
            tag = "%s log %d slice %d (%d, %d)" % (suite.name, first + l, j, s, e)
            a, b, units, rows, spans = view.cut(s, e) if view else (0, 0, np.zeros(0, "<u2"), [], [])
            assert (int(got.elem_start[k]), int(got.elem_end[k])) == (a, b), tag
            g = got.text[int(got.unit_off[k]) : int(got.unit_off[k + 1])]
            assert len(g) == len(units) and np.array_equal(g, units), tag
            assert got.rows_of_slice(k) == rows, tag
            if view and decode:
                dec = wire.decode_slice_spans(sub, res, got, l, j)
                assert H.norm_spans(dec) == H.norm_spans(spans) and [list(TC.u16(x["text"])) for x in dec] == [list(TC.u16(x["text"])) for x in spans], tag
            k += 1
    assert k == ns


def bounds_of(nv):
    """Every pair of the bounds the element walk can go wrong at: empty and reversed slices, slices behind the end and 0xFFFFFFFF included."""
    pts = sorted({0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T, max(nv - 1, 0), nv, nv + 1, ALL})
    return [(a, b) for a in pts for b in pts] + [(66, 67)]  # (and element 66 alone: text_cases' 5 000-unit value as a slice of its own)


def n_visible(res, n):
    return [int(res.value_off[k + 1]) - int(res.value_off[k]) for k in range(n)]


def plan_bounds(res, n):
    """Every log gets every pair of bounds_of(its n_visible)."""
    return [bounds_of(nv) for nv in n_visible(res, n)]


def plan_sparse(res, n):
    """Logs without slices between logs with them; descending, overlapping, nested and repeated slices; the whole log; exactly one tile."""
    order = [(10, 20), (5, 8), (0, 3), (0, 30), (10, 40), (0, 50), (10, 20), (7, 9), (7, 9), (7, 9), (0, ALL), (0, T), (T, 2 * T), (3, 3), (9, 2)]
    return [order if k % 3 == 1 else [] for k in range(n)]


def plan_kat(res, n):
    """One slice per span of the merge's result, one per comment interval, one for the whole document."""
    plan = []
    for k in range(n):
        st = [int(r["start"]) for r in res.spans[int(res.span_off[k]) : int(res.span_off[k + 1])]]
        nv = int(res.value_off[k + 1]) - int(res.value_off[k])
        p = [(st[q], st[q + 1] if q + 1 < len(st) else nv) for q in range(len(st))]
        p += [(int(c["start"]), int(c["end"])) for c in res.cintervals[int(res.cint_off[k]) : int(res.cint_off[k + 1])]]
        plan.append(p + [(0, ALL)])
    return plan


def check_kat_literals(suite, res, got, plan):
    """The slice of span q reproduces the reference-held text of that span and its single row."""
    assert sum("comment" in s["marks"] for w in suite.want for s in w.spans) > 0 and len(res.cintervals) > 0, "the documents hold comments"
    for l, w in enumerate(suite.want):
        for q, span in enumerate(w.spans):
            if int(got.elem_end[got.index(l, q)]) == int(got.elem_start[got.index(l, q)]):
                continue  # (a span without elements does not exist in a merge's result; an empty slice has no rows by contract)
            dec = wire.decode_slice_spans(suite.batch, res, got, l, q)
            assert H.norm_spans(dec) == H.norm_spans([span]), (l, q)
            assert got.of_slice(got.index(l, q)) == span["text"], (l, q)
        whole = len(plan[l]) - 1
        assert H.norm_spans(wire.decode_slice_spans(suite.batch, res, got, l, whole)) == H.norm_spans(w.spans), l


@functools.lru_cache(maxsize=None)
def edge_suite():
    """Single-replica documents at the edges of the output block, the span rows and the element; NAMES gives a log's index."""
    docs = []

    def add(name, values, ops=()):
        docs.append((name, H.mini_doc(list(ops), first_text=values)))

    strong = lambda i, j: {"action": "addMark", "markType": "strong", "start": TC.bf(i), "end": TC.bf(j)}  # noqa: E731  bold on the elements [i, j)
    add("blocks", [chr(0x61 + i % 26) for i in range(B + 40)])
    add("parity", list("abcdefg"))
    add("spans", [chr(0x61 + i) for i in range(20)], [strong(5, 10)])
    add("skipped", list("no slices here"))
    add("multi", ["x", "Hello, world", "y", "z"])
    add("empties", ["a", "", "b", "", "", "c", "d"], [strong(3, 5)])
    add("astral_split", list(TC.SPLIT_PAIR_VALUES))
    names = [n for n, _ in docs]
    logs = [[log] for _, log in docs]
    expected = H.oracle_apply(logs, no_patches=True)
    want = [TC.want_of_oracle(e[0]) for e in expected]
    i = names.index("astral_split")  # the oracle's JSON holds the joined pair; as text_cases: a hand-checked literal
    assert list(TC.u16(expected[i][0]["spans"][0]["text"])) == [0x61, 0xD83D, 0xDE00, 0x62]
    want[i] = TC.want_of_spans([{"text": TC.SPLIT_PAIR_TEXT, "marks": {}}])
    batch = wire.encode_docs(logs)
    w = dict(zip(names, want))
    assert len(w["blocks"].units) == B + 40 and len(w["spans"].spans) == 3 and len(w["empties"].spans) == 3 and len(w["multi"].units) == 15
    return TC.Suite("slice_edges", batch, list(batch.values), want, []), {n: k for k, n in enumerate(names)}


def edge_plan():
    """{name: [(start, end)]} of edge_suite, and per name the hand-written answers [(text, [(start, attr, unit)])] (None: the generic expectation only)."""
    plan, hand = {}, {}
    # cumulative output ends exactly at B - 1, B and B + 1 units; then B + 1 one-unit slices in a row; 65 empty slices between two non-empty ones
    plan["blocks"] = [(0, B - 1), (5, 6), (6, 7)] + [(i, i + 1) for i in range(B + 1)] + [(7, 7)] * 65 + [(3, 5), (0, B + 40)]
    # odd lengths: heads at (source, destination) parities (e, e), (e, o), (o, e), (o, o), and the tails likewise
    plan["parity"] = [(0, 3), (0, 3), (1, 4), (1, 4), (2, 3)]
    hand["parity"] = [("abc", [(0, 0, 0)]), ("abc", [(0, 0, 0)]), ("bcd", [(1, 0, 0)]), ("bcd", [(1, 0, 0)]), ("c", [(2, 0, 0)])]
    heads, tails, dst = set(), set(), 0
    for a, b in plan["parity"][:4]:
        heads.add((a & 1, dst & 1)), tails.add(((b - 1) & 1, (dst + b - a - 1) & 1))
        dst += b - a
    assert len(heads) == 4 and len(tails) == 4
    # exactly on a span start, one element before it, one after it (inside one span), the last row clipped by `end`, a slice over all three rows
    plan["spans"] = [(5, 8), (4, 8), (6, 8), (2, 12), (0, ALL), (10, 10)]
    hand["spans"] = [("fgh", [(5, STRONG, 0)]), ("efgh", [(4, 0, 0), (5, STRONG, 1)]), ("gh", [(6, STRONG, 0)]), ("cdefghijkl", [(2, 0, 0), (5, STRONG, 3), (10, 0, 8)]),
                     ("abcdefghijklmnopqrst", [(0, 0, 0), (5, STRONG, 5), (10, 0, 10)]), ("", [])]
    plan["skipped"] = []
    # a multi-unit value as a slice of its own, last, first and enclosed
    plan["multi"] = [(1, 2), (0, 2), (1, 3), (0, 3)]
    hand["multi"] = [("Hello, world", [(1, 0, 0)]), ("xHello, world", [(0, 0, 0)]), ("Hello, worldy", [(1, 0, 0)]), ("xHello, worldy", [(0, 0, 0)])]
    # only an empty-string element: zero units, a row; only the empty-string elements of the bold span; from an empty-string element to one
    plan["empties"] = [(1, 2), (3, 5), (1, 5), (0, ALL)]
    hand["empties"] = [("", [(1, 0, 0)]), ("", [(3, STRONG, 0)]), ("b", [(1, 0, 0), (3, STRONG, 1)]), ("abcd", [(0, 0, 0), (3, STRONG, 2), (5, 0, 2)])]
    # the pair split over two elements, cut between them: lone surrogates
    plan["astral_split"] = [(0, 2), (2, 4), (1, 3), (1, 2)]
    hand["astral_split"] = [("a\ud83d", [(0, 0, 0)]), ("\ude00b", [(2, 0, 0)]), ("😀", [(1, 0, 0)]), ("\ud83d", [(1, 0, 0)])]
    return plan, hand


def edge_plan_list():
    suite, names = edge_suite()
    plan, _ = edge_plan()
    return [plan[n] for n in sorted(names, key=names.get)]


def edge_hand_checks(got):
    """The hand-written answers of edge_plan against `got` (wire.Slices of the whole edge batch run with edge_plan_list())."""
    suite, names = edge_suite()
    plan, hand = edge_plan()
    for name, answers in hand.items():
        for j, (text, rows) in enumerate(answers):
            k = got.index(names[name], j)
            assert list(TC.u16(got.of_slice(k))) == list(TC.u16(text)), (name, j)
            assert got.rows_of_slice(k) == rows, (name, j)
    blocks = names["blocks"]
    ends = [int(got.unit_off[got.index(blocks, j) + 1]) for j in range(3)]
    assert ends == [B - 1, B, B + 1], "the first three slices end at B - 1, B and B + 1 units of the output"


def text_edge_hand_checks(suite, got, plan):
    """text_cases' edge suite run with plan_bounds: the cases that exist for one edge."""
    names, _ = TC.edge_docs()
    names = names + ["astral_split_pair"]
    at = lambda name, s, e: got.index(names.index(name), plan[names.index(name)].index((s, e)))  # noqa: E731
    k = at("five_thousand", 66, 67)
    assert got.of_slice(k) == suite.table[int(np.argmax([len(v) for v in suite.table]))], "the 5 000-unit value as a slice of its own"
    assert int(got.unit_off[k + 1]) - int(got.unit_off[k]) == 5000 > 4 * B, "its output crosses many blocks"
    assert got.of_slice(at("multi_first_edge_last", 0, 1)) == "Hello, " and got.of_slice(at("multi_first_edge_last", T - 1, T)) == " is great!"
    assert got.of_slice(at("multi_first_edge_last", T + 8, ALL)) == "the end."
    whole = at("n%d" % (2 * T + 1), 0, ALL)
    assert int(got.elem_end[whole]) == 2 * T + 1 and int(got.unit_off[whole + 1]) - int(got.unit_off[whole]) == 2 * T + 1
    tile = at("n%d" % (2 * T + 1), T, 2 * T)
    assert (int(got.elem_start[tile]), int(got.elem_end[tile])) == (T, 2 * T)
    assert list(TC.u16(got.of_slice(at("astral_split_pair", 1, ALL)))) == [0xD83D, 0xDE00, 0x62]
    past = at("n63", 64, ALL)
    assert (int(got.elem_start[past]), int(got.elem_end[past])) == (63, 63), "start >= n_visible: the empty slice at n_visible"
    rev = at("n65", 64, 1)
    assert (int(got.elem_start[rev]), int(got.elem_end[rev])) == (64, 64), "start > end: the empty slice at min(start, n_visible)"
    bold = at("alternating_bold", 0, ALL)
    assert int(got.sspan_off[bold + 1]) - int(got.sspan_off[bold]) > max(64, T), "more than 64 and more than T span rows in one slice"


def arrays_of(plan):
    """(slice_off u64, slice_start u32, slice_end u32) of a plan, as the C ABI takes them."""
    off = np.zeros(len(plan) + 1, np.uint64)
    if plan:
        off[1:] = np.cumsum([len(p) for p in plan], dtype=np.uint64)
    flat = np.array([x for p in plan for x in p], dtype=np.uint32).reshape(-1, 2)
    return off, np.ascontiguousarray(flat[:, 0]), np.ascontiguousarray(flat[:, 1])
