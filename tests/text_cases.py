"""Document text assembled on the device (ptx_result_text_range; peritext_amd/csrc/text_core.h): the cases tests/test_emu_text.py (CPU emulation) and
tests/test_gpu_text.py (the C ABI on the GPU) share.

A SUITE is a wire.Batch, the string table to upload, and per log what must come out: status, the text as UTF-16 code units, span_unit per span and — where
the log is good — the FormatSpanWithText[] itself.  Expected values never come from the code under test: the text is "".join(span["text"]) of the oracle's
spans (oracle/cli.js, or the reference-held expectedResult literal for the 46 known-answer documents), span_unit[k] the running UTF-16 length of the span
texts before span k; the one exception, stated by the case, is the surrogate pair split over two elements, whose text is a hand-written literal.
Edge sizes come from abi.TEXT_TILE (T below) and abi.TEXT_LANE_MAX (M)."""
import copy
import dataclasses
import functools
import json
import os

import numpy as np

import helpers as H
from peritext_amd import abi, wire

T, M = abi.TEXT_TILE, abi.TEXT_LANE_MAX


def u16(s):
    """A JS string as UTF-16 code units (lone surrogates stay)."""
    return np.frombuffer(s.encode("utf-16-le", "surrogatepass"), dtype="<u2")


def table_arrays(values):
    """(units u16[], off u64[n + 1]) of a string table, as ptx_strings_upload takes them."""
    enc = [u16(v) for v in values]
    off = np.zeros(len(enc) + 1, dtype=np.uint64)
    if enc:
        off[1:] = np.cumsum([len(e) for e in enc], dtype=np.uint64)
    units = np.concatenate(enc).astype(np.uint16) if int(off[-1]) else np.zeros(0, dtype=np.uint16)
    return np.ascontiguousarray(units), off


@dataclasses.dataclass
class Want:
    status: int  # 0 or the per-log status
    units: np.ndarray  # u16: the log's text
    span_unit: list  # per span of the MERGE's result
    spans: list = None  # FormatSpanWithText[] (good logs), compared through wire.decode_spans_text


@dataclasses.dataclass
class Suite:
    name: str
    batch: wire.Batch
    table: list  # the strings to upload (batch.values unless the case says otherwise)
    want: list  # Want per log
    ranges: list  # (first_log, n_logs) to run besides the whole batch


def _code(exp):
    err = exp.get("error")
    if not err:
        return 0
    for needle, code in (("Expected sequence number", abi.ERR_SEQ_GAP), ("Missing dependency", abi.ERR_MISSING_DEP), ("List element not found", abi.ERR_ELEM_NOT_FOUND)):
        if needle in err:
            return code
    raise AssertionError("unexpected oracle error: " + err)


def want_of_spans(spans):
    """Expected text and span_unit of a good log from a FormatSpanWithText[] literal."""
    at, run = [], 0
    for s in spans:
        at.append(run)
        run += len(u16(s["text"]))
    return Want(0, u16("".join(s["text"] for s in spans)), at, spans)


def want_of_oracle(exp):
    if "error" in exp:
        return Want(_code(exp), np.zeros(0, dtype=np.uint16), [], None)
    return want_of_spans(exp["spans"])


el = lambda i: "%d@a" % (i + 2)  # noqa: E731  element id of the i-th value of H.mini_doc
bf = lambda i: {"type": "before", "elemId": el(i)}  # noqa: E731
af = lambda i: {"type": "after", "elemId": el(i)}  # noqa: E731


def _chars(n, shift=0):
    return [chr(0x61 + (i * 7 + shift) % 26) for i in range(n)]


def _strong(i, n):
    """bold on element i alone (an inclusive mark ends `before` the next element or at endOfText, peritext.ts:483-497)"""
    return {"action": "addMark", "markType": "strong", "start": bf(i), "end": bf(i + 1) if i + 1 < n else {"type": "endOfText"}}


def edge_docs():
    """(names, docs): single-replica documents; H.mini_doc takes the values of the first change as a list, one insert each."""
    out = []
    # visible counts 1, 0 (everything deleted: an empty log between two non-empty ones), 63, 64, 65, T - 1, T, T + 1, 2T + 1: most of them odd, so later logs start on odd units
    out.append(("n1", H.mini_doc([], first_text=_chars(1))))
    out.append(("all_deleted", H.mini_doc([{"action": "del", "elemId": el(i)} for i in range(3)], first_text=_chars(3))))
    for n in (63, 64, 65, T - 1, T, T + 1, 2 * T + 1):
        ops = [_strong(n // 2, n)] if n > 2 else []
        out.append(("n%d" % n, H.mini_doc(ops, first_text=_chars(n, n))))
    # a multi-unit value as the first element, one that straddles the tile edge (element T - 1: a pasted run is ONE element), one as the last
    v = _chars(T + 9)
    v[0], v[T - 1], v[-1] = "Hello, ", " is great!", "the end."
    out.append(("multi_first_edge_last", H.mini_doc([_strong(T - 1, len(v)), _strong(len(v) - 1, len(v))], first_text=v)))
    # values of exactly threshold - 1, threshold, threshold + 1 units between one-unit ones, and one value of 5 000 units
    v = _chars(11)
    v[2], v[5], v[8] = "x" * (M - 1), "y" * M, "z" * (M + 1)
    out.append(("threshold", H.mini_doc([_strong(5, len(v))], first_text=v)))
    v = _chars(70)
    v[66] = "".join(chr(0x4E00 + k % 500) for k in range(5000))
    out.append(("five_thousand", H.mini_doc([_strong(67, len(v))], first_text=v)))
    # an empty-string value between others, and one span made only of empty-string elements (elements 3 and 4)
    v = ["a", "", "b", "", "", "c", "d"]
    out.append(("empty_strings", H.mini_doc([{"action": "addMark", "markType": "strong", "start": bf(3), "end": bf(5)}], first_text=v)))
    # a tile of empty strings only, then text
    out.append(("empty_tile", H.mini_doc([_strong(T, T + 3)], first_text=[""] * (T + 1) + ["p", "q"])))
    # alternating bold on every character: one span per element, span starts on both sides of the wave edge (63 | 64) and of the tile edge (T - 1 | T); a
    # comment-marked range and a link on top, so that wire.decode_spans_text is compared with the oracle's full {text, marks}
    n = max(130, T + 2)
    ops = [_strong(i, n) for i in range(0, n, 2)]
    ops.append({"action": "addMark", "markType": "comment", "attrs": {"id": "c-1"}, "start": bf(60), "end": af(70)})
    ops.append({"action": "addMark", "markType": "link", "attrs": {"url": "https://inkandswitch.com"}, "start": bf(100), "end": af(127)})
    out.append(("alternating_bold", H.mini_doc(ops, first_text=_chars(n, 3))))
    # an astral character as ONE value (two units)
    out.append(("astral_one_value", H.mini_doc([_strong(1, 3)], first_text=["a", "\U0001F600", "b"])))
    return [n for n, _ in out], [[log] for _, log in out]


SPLIT_PAIR_VALUES = ["a", "\ud83d", "\ude00", "b"]  # the same pair split over two adjacent elements: high surrogate, then low
SPLIT_PAIR_TEXT = "a\U0001F600b"  # hand-written: JS joins the two lone surrogates into the pair ("a" + "\ud83d" + "\ude00" + "b" === "a😀b")


@functools.lru_cache(maxsize=None)
def edge_suite():
    names, docs = edge_docs()
    split = [H.mini_doc([], first_text=SPLIT_PAIR_VALUES)]
    expected = H.oracle_apply(docs + [split], no_patches=True)
    want = [want_of_oracle(e[0]) for e in expected[:-1]]
    # the split pair as the reference would see it: a legal insert of two values (no error, ONE unmarked span, four elements' worth of text)
    e = expected[-1][0]
    assert "error" not in e and len(e["spans"]) == 1 and e["spans"][0]["marks"] == {}
    assert list(u16(e["spans"][0]["text"])) == [0x61, 0xD83D, 0xDE00, 0x62] == list(u16(SPLIT_PAIR_TEXT))
    want.append(want_of_spans([{"text": SPLIT_PAIR_TEXT, "marks": {}}]))
    names = names + ["astral_split_pair"]
    batch = wire.encode_docs(docs + [split])
    w = dict(zip(names, want))
    assert len(w["all_deleted"].units) == 0 and len(w["n1"].units) == 1 and len(w["n%d" % (2 * T + 1)].units) == 2 * T + 1
    assert any(s["text"] == "" for s in w["empty_strings"].spans), "one span is made only of empty-string elements"
    assert len(w["alternating_bold"].spans) >= max(130, T + 2) - 30 and any("comment" in s["marks"] for s in w["alternating_bold"].spans)
    assert len(w["astral_one_value"].units) == 4
    i = names.index("n63")
    return Suite("edges", batch, list(batch.values), want, [(i, 4), (1, 1), (2, 0), (batch.n_logs - 1, 1)])


@functools.lru_cache(maxsize=None)
def big_table_suite():
    """A string table of 70 000 strings (two units each: string offsets beyond 2^16) with value ids above 65 535 in use, ids repeated, ids not in table order."""
    table = [chr(0x3400 + i % 20000) + chr(0x61 + i // 20000) for i in range(70000)]
    ids = [69999, 3, 65536, 69999, 66000, 5, 65536, 0, 32768, 65535, 69998, 3] * 6
    docs = [[H.mini_doc([_strong(7, len(ids))], first_text=[table[i] for i in ids])], [H.mini_doc([], first_text=[table[69000], table[1]])]]
    batch = wire.encode_docs(docs)
    index = {s: i for i, s in enumerate(table)}
    remap = np.array([index[v] for v in batch.values], dtype=np.uint32)
    ins = batch.action == abi.ACT_INSERT
    payload = batch.payload.copy()
    payload[ins] = remap[batch.payload[ins]]
    batch = dataclasses.replace(batch, payload=payload, values=table)
    assert int(payload[ins].max()) == 69999
    want = [want_of_oracle(e[0]) for e in H.oracle_apply(docs, no_patches=True)]
    return Suite("big_table", batch, table, want, [(1, 1)])


@functools.lru_cache(maxsize=None)
def failed_log_suite():
    """A failed log (a sequence gap) between two good logs: its status is copied, it has no text and no spans."""
    with open(os.path.join(H.GOLDEN, "ptxgen_mini.json")) as f:
        gen = json.load(f)
    logs = [copy.deepcopy(l) for l in gen["docs"][0]["logs"]]
    logs[1][5]["seq"] += 1
    expected = H.oracle_apply([logs], no_patches=True)[0]
    want = [want_of_oracle(e) for e in expected]
    assert [w.status for w in want] == [0, abi.ERR_SEQ_GAP, 0] and len(want[0].units) and len(want[2].units)
    batch = wire.encode_docs([logs])
    return Suite("failed_log", batch, list(batch.values), want, [(1, 2)])


@functools.lru_cache(maxsize=None)
def kat_suite():
    """The 46 reference known-answer documents: text and spans equal the reference-held expectedResult (the oracle's spans where a case holds no literal)."""
    cases = H.load_kat()
    batch = wire.encode_docs([[r["log"] for r in c["replicas"]] for c in cases])
    want = []
    for c in cases:
        for r in c["replicas"]:
            want.append(want_of_spans(c.get("expected", r["spans"])))
    assert len(cases) == 46 and len(want) == batch.n_logs
    return Suite("kat", batch, list(batch.values), want, [])


def suites():
    return [edge_suite(), big_table_suite(), failed_log_suite(), kat_suite()]


def bad_id_batch(suite, log):
    """The suite's batch with ONE value id of `log` set to n_strings (the first id beyond the table): (batch, the row changed)."""
    b = suite.batch
    rows = np.arange(int(b.log_off[log]), int(b.log_off[log + 1]))
    ins = rows[b.action[rows] == abi.ACT_INSERT]
    row = int(ins[len(ins) // 2])
    payload = b.payload.copy()
    payload[row] = len(suite.table)
    return dataclasses.replace(b, payload=payload), row


def check_range(suite, res, text, first, n, decode=True):
    """`text` (wire.Text) and `res` (wire.Results, compact rows) of the logs [first, first + n) against the suite's expectations."""
    assert len(text.status) == n and len(text.text_off) == n + 1 and len(text.span_off) == n + 1
    assert int(text.text_off[0]) == 0 and int(text.span_off[0]) == 0
    assert np.array_equal(text.span_off, res.span_off), "span_off is the result's"
    for k in range(n):
        w, tag = suite.want[first + k], "%s log %d" % (suite.name, first + k)
        assert int(text.status[k]) == w.status == int(res.logs["status"][k]), tag
        got = text.text[int(text.text_off[k]) : int(text.text_off[k + 1])]
        assert len(got) == len(w.units) and np.array_equal(got, w.units), tag
        su = text.span_unit[int(text.span_off[k]) : int(text.span_off[k + 1])]
        assert [int(x) for x in su] == w.span_unit, tag
        if w.status == 0 and decode:
            sub = dataclasses.replace(suite.batch, log_doc=suite.batch.log_doc[first:])
            got_spans = wire.decode_spans_text(sub, res, text, k)
            assert H.norm_spans(got_spans) == H.norm_spans(w.spans), tag
            assert [list(u16(s["text"])) for s in got_spans] == [list(u16(s["text"])) for s in w.spans], tag
    assert len(text.text) == int(text.text_off[n]) and len(text.span_unit) == int(text.span_off[n])
