"""Find in the documents' text on the device (ptx_result_find_text; peritext_amd/csrc/find_core.h): the cases tests/test_emu_find.py (CPU emulation) and
tests/test_gpu_find.py (the C ABI on the GPU) share.  Built on the suites of tests/text_cases.py (imported, not edited) and one suite of its own.

Expected values never come from the code under test: a log's text is the oracle's "".join(span.text) (text_cases.Want.units; the reference-held literal for
the 46 known-answer documents), the hits are a plain loop over that u16 array (String.prototype.indexOf repeated from p + 1, over code units), the element
boundaries come from the lengths of table[values[i]] of the MERGE's result — the merge is not changed here — after `expect` has asserted that their join
equals the oracle's text.  Edge sizes come from abi.FIND_STEP (S), abi.TEXT_TILE (T) and abi.FIND_PATTERN_MAX (P)."""
import dataclasses
import functools

import numpy as np

import helpers as H
import text_cases as TC
from peritext_amd import abi, wire

S, T, P = abi.FIND_STEP, abi.TEXT_TILE, abi.FIND_PATTERN_MAX
ALL = 0xFFFFFFFF
LONGEST = "".join(chr(0x61 + (i * 5) % 26) for i in range(P))  # a pattern of P units that starts with "a": behind one "y" it matches at offset 1 only


@dataclasses.dataclass
class Query:
    pattern: str
    nocase: bool = False
    cap: int = ALL
    rng: tuple = None  # (first_log, n_logs); None: the whole batch
    want_counts: dict = None  # {log: n_matches} hand-written, checked against the loop's count: what the case is there for


def fold(a):
    a = a.astype(np.uint16).copy()
    a[(a >= 0x41) & (a <= 0x5A)] += 0x20
    return a


def search(units, pat, nocase=False):
    """Every p with units[p : p + m] == pat, ascending: indexOf repeated from p + 1."""
    if nocase:
        units, pat = fold(units), fold(pat)
    m, out = len(pat), []
    for p in range(len(units) - m + 1):
        if units[p] == pat[0] and np.array_equal(units[p : p + m], pat):
            out.append(p)
    return out


def expect(suite, res, first, k, q, status=None):
    """(status, n_matches, [(unit, start, end)] listed) of log first + k; res: the compact wire.Results of the range (its value ids give the element lengths)."""
    w = suite.want[first + k]
    st = w.status if status is None else status
    if st != 0:
        return st, 0, []
    ids = res.values[int(res.value_off[k]) : int(res.value_off[k + 1])]
    parts = [TC.u16(suite.table[int(i)]) for i in ids]
    joined = np.concatenate(parts + [np.zeros(0, "<u2")])
    assert len(joined) == len(w.units) and np.array_equal(joined, w.units), "the elements' strings join to the oracle's text"
    pre = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)[:-1]  # exclusive scan: pre[e] = first unit of element e
    pat = TC.u16(q.pattern)
    hits = search(w.units, pat, q.nocase)
    holder = lambda u: int(np.searchsorted(pre, u, side="right")) - 1  # noqa: E731  the last e with pre[e] <= u
    listed = [(p, holder(p), holder(p + len(pat) - 1) + 1) for p in hits[: q.cap]]
    return 0, len(hits), listed


def check_range(suite, res, got, first, n, q, status_of=None):
    """`got` (wire.Matches) of the logs [first, first + n) against the expectations; status_of: {log: status} overrides (a text-only failure)."""
    assert len(got.status) == n and len(got.n_matches) == n and len(got.hit_off) == n + 1 and int(got.hit_off[0]) == 0
    for k in range(n):
        tag = "%s log %d pattern %r" % (suite.name, first + k, q.pattern)
        st, count, listed = expect(suite, res, first, k, q, (status_of or {}).get(first + k))
        assert int(got.status[k]) == st, tag
        assert int(got.n_matches[k]) == count, tag
        if q.want_counts and (first + k) in q.want_counts:
            assert count == q.want_counts[first + k], tag + ": the case's own count"
        assert got.of_log(k) == listed, tag
    assert len(got.hit_unit) == len(got.hit_start) == len(got.hit_end) == int(got.hit_off[n])


def _fill(n):
    return ["x"] * n


@functools.lru_cache(maxsize=None)
def edge_suite():
    """Single-replica documents at the edges of the step, the tile, the log and the element; NAMES gives a log's index."""
    docs = []

    def add(name, values):
        docs.append((name, H.mini_doc([], first_text=values)))

    # positions: 'q' at units 0, 63, 64, 65, S - 1, S, S + 1 and as the very last unit (a match that ends exactly at L)
    v = _fill(S + 41)
    for p in (0, 63, 64, 65, S - 1, S, S + 1, len(v) - 1):
        v[p] = "q"
    add("positions", v)
    # m = 3 across the step edge: "aaaa" at S - 2 .. S + 1 holds "aaa" at S - 2 and at S - 1
    v = _fill(S + 4)
    v[S - 2 : S + 2] = ["a"] * 4
    add("straddle", v)
    # log boundaries: "xab" | "cab" | "c": "abc" lies across both borders and in no log; odd lengths, so the later logs start on odd units
    add("ends_ab", list("xab"))
    add("c_then_ab", list("cab"))
    add("only_c", list("c"))
    add("abc", list("abc"))  # L == m
    add("ab", list("ab"))  # L == m - 1
    docs.append(("all_deleted", H.mini_doc([{"action": "del", "elemId": TC.el(i)} for i in range(3)], first_text=list("abc"))))  # L == 0
    # m = P in a text of P + 1 units that holds it at offset 1
    add("longest_pattern", ["y"] + list(LONGEST))
    # dense: 2S + 1 times "a"
    add("dense", ["a"] * (2 * S + 1))
    # elements: a hit inside one multi-unit element; one that spans it and its one-unit neighbours
    add("multi", ["x", "Hello, world", "y", "z"])
    # a hit across empty-string elements ("abc" over a,"",b,"","",c); an empty string directly before the hit's first unit ("b": element 1 is empty)
    add("empties", ["a", "", "b", "", "", "c", "d"])
    # first unit in element T - 1, last in element T ("QZ"); a hit entirely in the second tile ("WV")
    v = _fill(T + 9)
    v[T - 1], v[T], v[T + 3], v[T + 4] = "Q", "Z", "W", "V"
    add("tile_edge", v)
    # a tile made only of empty strings, then text
    add("empty_tile", [""] * (T + 1) + ["p", "q"])
    # the astral character as one value, and as a pair split over two elements
    add("astral_one_value", ["a", "\U0001F600", "b"])
    add("astral_split", list(TC.SPLIT_PAIR_VALUES))
    # ASCII case folding only: U+0130 and U+212A fold to i / k in Unicode, not here
    add("case", list("Hello ") + ["\u0130", "\u212a"])
    names = [n for n, _ in docs]
    logs = [[log] for _, log in docs]
    expected = H.oracle_apply(logs, no_patches=True)
    want = [TC.want_of_oracle(e[0]) for e in expected]
    i = names.index("astral_split")  # the oracle's JSON holds the joined pair; as text_cases: a hand-checked literal
    assert list(TC.u16(expected[i][0]["spans"][0]["text"])) == [0x61, 0xD83D, 0xDE00, 0x62]
    want[i] = TC.want_of_spans([{"text": TC.SPLIT_PAIR_TEXT, "marks": {}}])
    batch = wire.encode_docs(logs)
    w = dict(zip(names, want))
    assert len(w["all_deleted"].units) == 0 and len(w["dense"].units) == 2 * S + 1 and len(w["longest_pattern"].units) == P + 1 and len(w["multi"].units) == 15
    suite = TC.Suite("find_edges", batch, list(batch.values), want, [])
    return suite, {n: k for k, n in enumerate(names)}


def edge_queries():
    suite, N = edge_suite()
    dense = 2 * S + 1
    qs = [
        Query("q", want_counts={N["positions"]: 8, N["empty_tile"]: 1}),  # m = 1
        Query("aaa", want_counts={N["straddle"]: 2, N["dense"]: dense - 2}),
        Query("abc", want_counts={N["ends_ab"]: 0, N["c_then_ab"]: 0, N["only_c"]: 0, N["abc"]: 1, N["ab"]: 0, N["all_deleted"]: 0, N["empties"]: 1}),
        Query("abc", rng=(N["c_then_ab"], 4)),  # a range that starts behind log 0, on an odd unit of the buffer
        Query(LONGEST, want_counts={N["longest_pattern"]: 1}),
        Query("a", want_counts={N["dense"]: dense}),  # every position hits: more than 64 per step
        Query("aa", want_counts={N["dense"]: dense - 1}),
        Query("world", want_counts={N["multi"]: 1}),
        Query("xHello, worldy", want_counts={N["multi"]: 1}),
        Query("b", want_counts={N["empties"]: 1}),
        Query("QZ", want_counts={N["tile_edge"]: 1}),
        Query("WV", want_counts={N["tile_edge"]: 1}),
        Query("pq", want_counts={N["empty_tile"]: 1}),
        Query("😀", want_counts={N["astral_one_value"]: 1, N["astral_split"]: 1}),
        Query("\ud83d", want_counts={N["astral_one_value"]: 1, N["astral_split"]: 1}),
        Query("\ude00", want_counts={N["astral_one_value"]: 1, N["astral_split"]: 1}),
        Query("hELLO", nocase=True, want_counts={N["case"]: 1, N["multi"]: 1}),
        Query("hELLO", want_counts={N["case"]: 0, N["multi"]: 0}),
        Query("i", nocase=True, want_counts={N["case"]: 0}),
        Query("k", nocase=True, want_counts={N["case"]: 0}),
    ]
    for cap in (0, 1, 64, 65, dense):
        qs.append(Query("a", cap=cap, want_counts={N["dense"]: dense}))
    return qs


def edge_hand_checks(suite, N, got_by_pattern):
    """Hand-written element ranges of the cases that exist for them: got_by_pattern[(pattern, nocase)] = wire.Matches of the whole batch, cap ALL."""
    g = lambda pat, name, nocase=False: got_by_pattern[(pat, nocase)].of_log(N[name])  # noqa: E731
    assert g("world", "multi") == [(8, 1, 2)], "inside one multi-unit element: hit_end == hit_start + 1"
    assert g("xHello, worldy", "multi") == [(0, 0, 3)]
    assert g("abc", "empties") == [(0, 0, 6)], "across empty-string elements"
    assert g("b", "empties") == [(1, 2, 3)], "the empty string before the hit's first unit is skipped"
    assert g("QZ", "tile_edge") == [(T - 1, T - 1, T + 1)] and g("WV", "tile_edge") == [(T + 3, T + 3, T + 5)]
    assert g("pq", "empty_tile") == [(0, T + 1, T + 3)]
    assert g("😀", "astral_one_value") == [(1, 1, 2)] and g("😀", "astral_split") == [(1, 1, 3)]
    assert g("\ude00", "astral_one_value") == [(2, 1, 2)] and g("\ude00", "astral_split") == [(2, 2, 3)]
    assert [h[0] for h in g("q", "positions")] == [0, 63, 64, 65, S - 1, S, S + 1, S + 40]
    assert [h[0] for h in g("aaa", "straddle")] == [S - 2, S - 1]
    assert g(LONGEST, "longest_pattern") == [(1, 1, P + 1)]


def two_letters(units):
    """A two-unit pattern taken from a text: its middle."""
    at = max(0, len(units) // 2 - 1)
    return units[at : at + 2].astype("<u2").tobytes().decode("utf-16-le", "surrogatepass")


@functools.lru_cache(maxsize=None)
def kat_queries():
    """One query per known-answer document: a two-letter pattern from the text of its first replica, searched in the whole batch."""
    suite = TC.kat_suite()
    out, log = [], 0
    for c in H.load_kat():
        u = suite.want[log].units
        assert len(u) >= 2
        out.append(Query(two_letters(u), want_counts=None))
        assert search(u, TC.u16(out[-1].pattern)), "the document holds its own pattern"
        log += len(c["replicas"])
    assert len(out) == 46
    return out


def failed_log_queries():
    suite = TC.failed_log_suite()
    return [Query(two_letters(suite.want[0].units)), Query(two_letters(suite.want[2].units), cap=1), Query(two_letters(suite.want[2].units), rng=(1, 2))]


def text_edge_queries():
    """text_cases' own edge suite (tile-sized logs of odd lengths in a row, long values, the 5 000-unit value) searched for letters of its texts."""
    return [Query("ho"), Query("great"), Query("e"), Query("\u4e00\u4e01"), Query("ZZ"), Query("E", nocase=True, cap=3)]
