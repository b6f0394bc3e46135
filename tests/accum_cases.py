"""Cases of the accumulation of patch streams (peritext_amd/csrc/accum_core.h), shared by tests/test_emu_accum.py (the CPU emulation, every lane order, both
state stores) and tests/test_gpu_accum.py (the C ABI on a real MI355X).  Expected values never come from the code under test: they are the reference's spans
and text — tests/golden/accum_edges.json (tests/make_accum_golden.py: the type-erased reference on the chunk-edge document, the 46 KATs and the 9 traces),
tests/golden/edge_cases_ref.json, and the `expected` the generated fixtures hold — through helpers.check_log (decoded spans, raw rows, digest with n_elems).

A test body takes two callables:  stream_fn(batch) -> wire.Patches (the replay of the merged batch)  and  acc_fn(batch, pat) -> wire.Results."""
import copy
import json
import os

import numpy as np

import helpers as H
from peritext_amd import abi, wire

EDGE_TEXT = "".join("abcdefghijklmnopqrstuvwxyz"[i % 26] for i in range(130))
FIXTURES = ["patches_mini.json", "patches_rich_300.json", "ptxgen_rich_700.json", "ptxgen_config4_600.json"]


def edges_log():
    """The chunk-edge document: a 130-character text, then one change whose inserts, deletes and marks sit on the 64- and 128-character boundaries of the
    accumulate kernel's list walks."""
    el = lambda i: "%d@a" % (i + 2)  # noqa: E731
    bf = lambda i: {"type": "before", "elemId": el(i)}  # noqa: E731
    af = lambda i: {"type": "after", "elemId": el(i)}  # noqa: E731
    mark = lambda act, mt, s, e, **attrs: dict({"action": act, "markType": mt, "start": s, "end": e}, **({"attrs": attrs} if attrs else {}))  # noqa: E731
    ins = lambda after, v: {"action": "set", "insert": True, "elemId": after, "value": v}  # noqa: E731
    ops = [
        mark("addMark", "strong", bf(0), af(63)),
        mark("addMark", "em", bf(63), af(64)),
        mark("addMark", "link", bf(64), af(127), url="u"),
        mark("addMark", "comment", bf(1), af(129), id="c1"),
        mark("addMark", "comment", bf(31), af(33), id="c2"),
    ]
    ops += [ins(a, v) for a, v in zip(["_head", el(62), el(63), el(64), el(126), el(127), el(129)], "ABCDEFG")]
    ops += [
        mark("removeMark", "comment", bf(60), af(70), id="c1"),
        mark("removeMark", "strong", bf(10), af(20)),
        mark("addMark", "link", bf(100), af(129), url="v"),
    ]
    ops += [{"action": "del", "elemId": el(i)} for i in (0, 63, 64, 127, 129, 128)]
    ops += [ins(el(32), "H"), ins(el(65), "I")]
    ops += [mark("removeMark", "link", bf(120), af(126)), mark("addMark", "comment", bf(0), af(129), id="c3")]
    return H.mini_doc(ops, first_text=EDGE_TEXT)


def kat_and_trace_docs():
    with open(os.path.join(H.GOLDEN, "reference_traces.json")) as f:
        traces = json.load(f)
    return [[r["log"] for r in c["replicas"]] for c in H.load_kat()] + [t["logs"] for t in traces]


def load_golden():
    with open(os.path.join(H.GOLDEN, "accum_edges.json")) as f:
        g = json.load(f)
    assert g["impl"] == "ref"
    assert g["edges"]["logs"] == [edges_log()], "tests/golden/accum_edges.json was made for another chunk-edge document (tests/make_accum_golden.py)"
    assert g["kat_inputs"] == H.inputs_sha16(kat_and_trace_docs())
    return g


def _fixture(name):
    with open(os.path.join(H.GOLDEN, name)) as f:
        return json.load(f)


def quirk_case():
    """(docs, expected per log): document 0 = the chunk-edge document, then helpers.edge_case_docs(), helpers.boundary_docs(), the 46 KATs and the 9 traces."""
    g = load_golden()
    edge = _fixture("edge_cases_ref.json")
    assert edge["impl"] == "ref"
    docs = [[edges_log()]] + H.edge_case_docs() + H.boundary_docs() + kat_and_trace_docs()
    exp = [[g["edges"]["expected"]]] + edge["edge"] + edge["boundary"] + g["kat"]
    flat = [e for d in exp for e in d]
    assert len(flat) == sum(len(d) for d in docs)
    return docs, flat


def fixture_case(name):
    g = _fixture(name)
    if "from" in g:  # the patch fixtures name the generated fixture whose logs they replay
        src = _fixture(g["from"])
        return [d["logs"] for d in src["docs"]], [{"spans": e["spans"], "text": e["text"]} for d in src["docs"] for e in d["expected"]]
    return [d["logs"] for d in g["docs"]], [e for d in g["docs"] for e in d["expected"]]


# ---- streams as numpy records ----
def with_stream(pat, log, recs, status=0):
    """A copy of `pat` in which log `log` has the records `recs`."""
    n = len(pat.logs)
    parts = [np.asarray(recs, dtype=abi.PATCH_DTYPE) if l == log else pat.of_log(l) for l in range(n)]
    logs = pat.logs.copy()
    logs["n_patches"][log] = len(parts[log])
    logs["status"][log] = status
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    rows = np.concatenate(parts) if parts else np.zeros(0, dtype=abi.PATCH_DTYPE)
    return wire.Patches(patch_off=off, logs=logs, patches=rows)


def lengths_before(recs):
    """Length of the document before each record."""
    out, n = [], 0
    for r in recs:
        out.append(n)
        if int(r["kind"]) == abi.PATCH_INSERT:
            n += 1
        elif int(r["kind"]) == abi.PATCH_DELETE:
            n -= int(r["b"])
    return out


def fold_deletes(recs):
    """Every run of consecutive DELETE records at one index as ONE record with b = the run's length (what a peer that folds deletes sends)."""
    out = []
    for r in recs:
        if out and int(r["kind"]) == abi.PATCH_DELETE and int(out[-1]["kind"]) == abi.PATCH_DELETE and int(out[-1]["a"]) == int(r["a"]):
            out[-1]["b"] += r["b"]
        else:
            out.append(r.copy())
    return np.array(out, dtype=abi.PATCH_DTYPE)


def tamper_cases(recs, n_rows, n_comment_ids):
    """[(name, records with ONE record changed, status, index of that record)] — the malformed streams of the issue."""
    lb = lengths_before(recs)
    kinds = [int(r["kind"]) for r in recs]
    marks = (abi.PATCH_ADDMARK, abi.PATCH_REMOVEMARK)
    last = lambda pred: max(k for k in range(len(recs)) if pred(k))  # noqa: E731
    k_ins, k_del, k_mark = last(lambda k: kinds[k] == abi.PATCH_INSERT), last(lambda k: kinds[k] == abi.PATCH_DELETE), last(lambda k: kinds[k] in marks)
    k_ic = last(lambda k: kinds[k] == abi.PATCH_INSERT_COMMENT)
    k_orphan = last(lambda k: kinds[k] in marks and kinds[k - 1] not in (abi.PATCH_INSERT, abi.PATCH_INSERT_COMMENT))
    out = []

    def case(name, k, status, **fields):
        r = recs.copy()
        for f, v in fields.items():
            r[f][k] = v
        out.append((name, r, status, k))

    case("insert at length + 1", k_ins, abi.ERR_INDEX_OOB, a=lb[k_ins] + 1)
    case("delete past the end", k_del, abi.ERR_INDEX_OOB, a=lb[k_del])
    case("mark with b = length + 1", k_mark, abi.ERR_INDEX_OOB, b=lb[k_mark] + 1)
    case("mark with a > b", k_mark, abi.ERR_INDEX_OOB, a=int(recs["b"][k_mark]) + 1)
    case("kind 9", k_mark, abi.ERR_BAD_OP, kind=9)
    case("orphan INSERT_COMMENT", k_orphan, abi.ERR_BAD_OP, kind=abi.PATCH_INSERT_COMMENT, a=0)
    case("row = the log's rows", k_del, abi.ERR_BAD_OP, row=n_rows)
    case("comment id = n_comment_ids", k_ic, abi.ERR_BAD_OP, a=n_comment_ids)
    return out


# ---- test bodies ----
def check_all(batch, res, expected, logs=None):
    for log in (range(batch.n_logs) if logs is None else logs):
        H.check_log(batch, res, log, expected[log])
        assert int(res.logs["reserved"][log][1]) == 0xFFFFFFFF


def assert_edge_stream_facts(batch, pat, res):
    """What makes document 0 a chunk-edge document, asserted on its stream so that a changed fixture cannot hollow the test out."""
    recs = pat.of_log(0)
    kind, a, b = recs["kind"].astype(int), recs["a"].astype(int), recs["b"].astype(int)
    assert int(batch.log_off[1] - batch.log_off[0]) == 156 and len(recs) == 186
    r = res.logs[0]
    assert (int(r["n_visible"]), int(r["n_spans"]), int(r["n_cintervals"])) == (133, 14, 4) and int((kind == abi.PATCH_INSERT_COMMENT).sum()) == 7
    second = np.flatnonzero(recs["row"] > 130)  # the records of the second change
    ins = {int(a[k]) for k in second if kind[k] == abi.PATCH_INSERT}
    assert 0 in ins and {64, 65} & ins and any(x >= 128 for x in ins) and any(x in (63, 64) for x in ins)
    dels = [int(a[k]) for k in second if kind[k] == abi.PATCH_DELETE]
    assert {1, 64, 65} <= set(dels) and {129, 130, 131} & set(dels) and all(int(b[k]) == 1 for k in second if kind[k] == abi.PATCH_DELETE)
    ranges = {(int(a[k]), int(b[k])) for k in second if kind[k] in (abi.PATCH_ADDMARK, abi.PATCH_REMOVEMARK)}
    assert {(0, 64), (63, 64), (64, 65), (65, 128), (128, 130)} <= ranges, sorted(ranges)


def run_quirks(stream_fn, acc_fn):
    docs, expected = quirk_case()
    batch = wire.encode_docs(docs)
    pat = stream_fn(batch)
    res = acc_fn(batch, pat)
    check_all(batch, res, expected)
    assert_edge_stream_facts(batch, pat, res)
    # the quirks, by name: the empty document; the remove of an absent comment (a span with the key and no interval); everything deleted
    assert int(res.logs["n_visible"][1 + 5]) == 0 and int(res.logs["n_spans"][1 + 5]) == 0
    v, s, c = wire.canonical_of_log(batch, res, 1)
    assert any(int(x["attr"]) & abi.ATTR_COMMENT for x in s) and len(c) == 0
    assert int(res.logs["n_visible"][1 + 6]) == 0 and int(res.logs["n_elems"][1 + 6]) == 5
    return batch, pat, res, expected


def run_fixture(name, stream_fn, acc_fn):
    docs, expected = fixture_case(name)
    batch = wire.encode_docs(docs)
    pat = stream_fn(batch)
    res = acc_fn(batch, pat)
    check_all(batch, res, expected)
    return batch, pat, res


def run_failed_log(stream_fn, acc_fn):
    """A log the merge refuses (a skipped seq: the reference's RangeError "Expected sequence number") beside good ones."""
    gen = _fixture("ptxgen_mini.json")
    logs = [copy.deepcopy(l) for l in gen["docs"][0]["logs"]]
    logs[1][5]["seq"] += 1
    batch = wire.encode_docs([logs])
    pat = stream_fn(batch)
    res = acc_fn(batch, pat)
    r = res.logs[1]
    assert int(pat.logs["status"][1]) == abi.ERR_SEQ_GAP and int(r["status"]) == abi.ERR_SEQ_GAP
    assert (int(r["n_visible"]), int(r["n_spans"]), int(r["n_cintervals"]), int(r["n_elems"])) == (0, 0, 0, 0) and [int(x) for x in r["digest"]] == [0, 0]
    check_all(batch, res, gen["docs"][0]["expected"], logs=[0, 2])


def run_foreign_streams(stream_fn, acc_fn):
    docs, expected = quirk_case()
    docs, expected = docs[:9], expected[:9]  # the chunk-edge document and the eight quirk documents beside it
    batch = wire.encode_docs(docs)
    pat = stream_fn(batch)
    base = acc_fn(batch, pat)
    check_all(batch, base, expected)
    recs = pat.of_log(0)
    n_rows, n_ids = int(batch.log_off[1] - batch.log_off[0]), int(batch.log_hdr["n_comment_ids"][0])
    others = range(1, batch.n_logs)

    def same_rows(x, y, log):
        assert np.array_equal(x.logs[log], y.logs[log])
        for p, q in zip(wire.canonical_of_log(batch, x, log), wire.canonical_of_log(batch, y, log)):
            assert np.array_equal(p, q)

    # (a) folded deletes, in every log of the batch that has a run of them (the chunk-edge document deletes at distinct indexes; the all-deleted quirk
    # document deletes five times at index 0): the same documents, row for row
    fpat, widest = pat, 0
    for log in range(batch.n_logs):
        f = fold_deletes(pat.of_log(log))
        if len(f) < len(pat.of_log(log)):
            widest = max(widest, int(f["b"][f["kind"] == abi.PATCH_DELETE].max()))
            fpat = with_stream(fpat, log, f)
    assert widest >= 5
    res = acc_fn(batch, fpat)
    check_all(batch, res, expected)
    for log in range(batch.n_logs):
        for p, q in zip(wire.canonical_of_log(batch, res, log), wire.canonical_of_log(batch, base, log)):
            assert np.array_equal(p, q)
        assert np.array_equal(res.logs["digest"][log], base.logs["digest"][log])
    # (b) one record tampered with: that log alone fails, at that record
    cases = tamper_cases(recs, n_rows, n_ids)
    assert len(cases) == 8
    for name, bad, status, k in cases:
        res = acc_fn(batch, with_stream(pat, 0, bad))
        r = res.logs[0]
        assert (int(r["status"]), int(r["reserved"][1])) == (status, k), name
        assert (int(r["n_visible"]), int(r["n_spans"]), int(r["n_cintervals"])) == (0, 0, 0) and [int(x) for x in r["digest"]] == [0, 0], name
        for log in others:
            same_rows(res, base, log)
    # (c) one in-bounds DELETE record dropped: a well-formed stream of ANOTHER document
    kd = [k for k in range(len(recs)) if int(recs["kind"][k]) == abi.PATCH_DELETE][2]
    res = acc_fn(batch, with_stream(pat, 0, np.delete(recs, kd)))
    assert int(res.logs["status"][0]) == 0 and int(res.logs["n_visible"][0]) == int(base.logs["n_visible"][0]) + 1
    assert not np.array_equal(res.logs["digest"][0], base.logs["digest"][0])
    for log in others:
        same_rows(res, base, log)
