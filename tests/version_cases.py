"""Shared by tests/test_emu_versions.py and tests/test_gpu_versions.py: the version-cut cases (documents, cuts), what the reference answers for them
(tests/version_oracle.js over oracle/peritext_oracle.js, computed once per case and mode) and the comparisons per cut.

A case is {"docs": [[log, ...], ...], "cuts": [{"log": l, "clock": {actorId: seq | "all"}} | {"log": l, "changes": k}, ...]} with the logs numbered across the
documents in order, as wire.encode_docs lays them out; the cuts of one case are all clock cuts or all prefix cuts (one call takes one kind).  The hand-made
logs are built from sync_cases' one-op changes (change 1 of `a` makes the text list, every other change inserts one character at the head) and from changes
WITHOUT ops, which are valid anywhere: they put the list's maker — the one change a clock {a: 1} keeps — at any lane of the 64-change steps."""
import functools
import json
import os
import tempfile

import numpy as np

import helpers as H
import sync_cases as SC
from peritext_amd import abi, wire

SIZES = (0, 1, 63, 64, 65, 129, 136)  # source logs: empty, one change, around one and two 64-change steps, and sync_cases' 136
ALL = "all"


# ---- the oracle ----
def oracle_versions(logs, cuts, then_rest):
    with tempfile.TemporaryDirectory() as td:
        inp, out = os.path.join(td, "in.json"), os.path.join(td, "out.json")
        with open(inp, "w") as f:
            json.dump({"logs": logs, "cuts": cuts, "thenRest": bool(then_rest)}, f)
        H.run_node(["tests/version_oracle.js", inp, out])
        with open(out) as f:
            return json.load(f)["cuts"]


def oracle_of(case, then_rest):
    """The oracle's answer for a case in one mode, computed once."""
    key = "oracle_rest" if then_rest else "oracle"
    if key not in case:
        case[key] = oracle_versions(SC.flat_logs(case), case["cuts"], then_rest)
    return case[key]


# ---- hand-made logs ----
def empty_change(actor, seq, deps=None):
    return {"actor": actor, "seq": seq, "deps": dict(deps or {}), "startOp": 0, "ops": []}


def multi_change(actor, seq, deps, ctr, nops):
    """A change of `nops` head inserts (op ids ctr ..)."""
    if nops == 0:
        return empty_change(actor, seq, deps)
    ops = [{"opId": "%d@%s" % (ctr + j, actor), "action": "set", "obj": SC.TEXT, "elemId": "_head", "insert": True, "value": chr(97 + (ctr + j) % 26)} for j in range(nops)]
    return {"actor": actor, "seq": seq, "deps": dict(deps), "startOp": ctr, "ops": ops}


def maker_at(n, lane):
    """n changes whose `lane`-th is the list's maker (a's only change): changes of b without ops before it, b's head inserts behind it."""
    before = [empty_change("b", k + 1) for k in range(lane)]
    after = SC.run_of("b", n - lane - 1, lambda k: {"a": 1}, seq0=lane + 1)
    return before + [SC.first_change()] + after


def alternating(n):
    """a's changes at the even places (the first makes the list), b's at the odd ones."""
    log, na, nb = [], 0, 0
    for i in range(n):
        if i % 2 == 0:
            na += 1
            log.append(SC.change("a", na, {}, 2 * i + 1, make_list=(i == 0)))
        else:
            nb += 1
            log.append(SC.change("b", nb, {"a": 1}, 2 * i + 1))
    return log


@functools.lru_cache(maxsize=None)
def keep_pattern_case():
    """Every size of SIZES with every keep pattern it admits: none, all, every second change, only lane 0, only lane 63, only the first lane of the second
    step — the ballot slots at both ends of a step and across it.  One document per (size, pattern)."""
    docs, cuts, names = [], [], []

    def add(log, clock, name):
        docs.append([log])
        cuts.append({"log": len(docs) - 1, "clock": clock})
        names.append(name)

    for n in SIZES:
        add(alternating(n), {}, "none/%d" % n)
        add(alternating(n), {"a": ALL, "b": ALL}, "all/%d" % n)
        if n:
            add(alternating(n), {"a": ALL}, "second/%d" % n)
            add(maker_at(n, 0), {"a": 1}, "lane0/%d" % n)
        if n >= 64:
            add(maker_at(n, 63), {"a": 1}, "lane63/%d" % n)
        if n >= 65:
            add(maker_at(n, 64), {"a": 1}, "lane64/%d" % n)
    return {"docs": docs, "cuts": cuts, "names": names}


NOPS = (1, 0, 3, 2, 0, 0, 4)  # places 62 .. 65 hold 4, 1, 0, 3 ops; shifted by one place in the second log: 1, 0, 3, 2


def multi_op_log(n, shift):
    log, seq, ctr = [SC.first_change()], {"a": 1, "b": 0}, 10
    for i in range(1, n):
        actor = "ab"[i % 2]
        seq[actor] += 1
        k = NOPS[(i + shift) % len(NOPS)]
        log.append(multi_change(actor, seq[actor], {"a": 1} if actor == "b" else {}, ctr, k))
        ctr += k
    return log


@functools.lru_cache(maxsize=None)
def multi_op_case(prefix):
    """Changes of 0, 1 and several ops on both sides of the step edge (the row scans; a change without ops shares its successor's first row)."""
    docs = [[multi_op_log(70, 0)], [multi_op_log(70, 1)], [multi_op_log(131, 2)]]
    if prefix:
        cuts = [{"log": l, "changes": k} for l in range(3) for k in (62, 63, 64, 65, 66)] + [{"log": 2, "changes": k} for k in (127, 128, 129, 200)]
    else:
        cuts = [{"log": l, "clock": c} for l in range(3) for c in ({"a": ALL}, {"a": 1, "b": ALL}, {"a": 32, "b": 32}, {"a": 33, "b": 31}, {"a": ALL, "b": ALL})]
    return {"docs": docs, "cuts": cuts}


STRIDE_ACTORS = (1, 3, 4, 5, 9, 13, 17)  # envelope rows of 4, 4, 8, 8, 12, 16 and 20 u16


@functools.lru_cache(maxsize=None)
def stride_case():
    """Documents of 1 .. 17 actors; the cut clock's non-zero entries stand at the lowest and the highest rank."""
    docs, cuts = [], []
    for n in STRIDE_ACTORS:
        names = SC.actor_names(n)
        log = [SC.first_change()] + [SC.change(x, 1, {"a": 1}, 100 + 10 * i) for i, x in enumerate(names[1:])] + SC.run_of("a", 3, lambda k: {}, seq0=2, ctr0=500)
        docs.append([log])
        cuts.append({"log": len(docs) - 1, "clock": {"a": 2, names[-1]: 1} if n > 1 else {"a": 2}})
    return {"docs": docs, "cuts": cuts}


def open_clock_log(f, n=136):
    """n changes of b without ops; the one at place f of the log waits for c's first change, which stands at the head of the log (f = 0: behind b's changes,
    a log nobody could have applied); the list's maker comes last.  The clock {b: all} keeps b's changes only: applyChange throws "Missing dependency" at
    the one that waits."""
    k_dep = f - 1 if f else 0
    bs = [empty_change("b", k + 1, {"c": 1} if k == k_dep else {}) for k in range(n)]
    return ([empty_change("c", 1)] + bs if f else bs + [empty_change("c", 1)]) + [SC.first_change()]


@functools.lru_cache(maxsize=None)
def open_clock_case():
    """Non-closed clocks: the kept change with the missing dep at lane 0, at lane 63 and in the second step; one closed cut of the same logs beside them."""
    docs = [[open_clock_log(f)] for f in (0, 63, 70)]
    cuts = [{"log": l, "clock": {"b": ALL}} for l in range(3)] + [{"log": 1, "clock": {"b": 62}}, {"log": 2, "clock": {"b": 69}}]
    return {"docs": docs, "cuts": cuts}


@functools.lru_cache(maxsize=None)
def history_strip_case():
    """One 130-change source (65 rounds of two actors answering each other) cut at every prefix 0 .. 130 in ONE call."""
    src = SC.ping_pong(65, 0)[0]
    assert len(src) == 130
    return {"docs": [[src]], "cuts": [{"log": 0, "changes": k} for k in range(131)]}


def clock_of(log):
    c = {}
    for ch in log:
        c[ch["actor"]] = max(c.get(ch["actor"], 0), ch["seq"])
    return c


@functools.lru_cache(maxsize=None)
def redealt_case(config, replicas=None):
    """The re-dealt logs of sync_cases.redeal_case: every replica cut at the clock of every other replica of its document (closed by construction: a clock
    some replica really had); a clock that is ahead of the source keeps what the source has."""
    base = SC.redeal_case(config, replicas)
    docs, cuts, at = [], [], 0
    for doc in base["docs"]:
        n = int(round(len(doc) ** 0.5))  # (redeal_case carries one more copy of the target per ordered pair behind the n re-dealt logs)
        assert n * n == len(doc)
        logs = doc[:n]
        docs.append(logs)
        cuts += [{"log": at + s, "clock": clock_of(logs[t])} for s in range(n) for t in range(n) if s != t]
        at += n
    return {"docs": docs, "cuts": cuts}


# ---- running a case ----
def cut_tables(case, batch):
    """(src_log u32[n], clocks u32[n, max_actors] | None, prefix u32[n] | None) of a case's cuts."""
    src = np.array([c["log"] for c in case["cuts"]], dtype=np.uint32)
    if case["cuts"] and "changes" in case["cuts"][0]:
        return src, None, np.array([c["changes"] for c in case["cuts"]], dtype=np.uint32)
    clocks = np.zeros((len(src), batch.max_actors), dtype=np.uint32)
    for i, c in enumerate(case["cuts"]):
        actors = batch.doc_actors[batch.log_doc[c["log"]]]
        for a, q in c["clock"].items():
            if a in actors:  # (an actor the document never saw keeps nothing of anybody)
                clocks[i, actors.index(a)] = abi.VERSION_ALL if q == ALL else q
    return src, clocks, None


def cut_batch(batch, src, cols, log_off, chg_off):
    """wire.Batch of the cut logs given as raw columns, with the tables of `batch`: log c belongs to the document of its source."""
    T, NC, es = int(log_off[-1]), int(chg_off[-1]), abi.env_stride(batch.max_actors)
    return wire.Batch(log_off, cols["op_id"][:T], cols["ref_a"][:T], cols["ref_b"][:T], cols["payload"][:T], cols["action"][:T], cols["mark_type"][:T], cols["side_a"][:T],
                      cols["side_b"][:T], chg_off, cols["chg_hdr"][:NC], cols["chg_env"][:NC * es], batch.max_actors, None, batch.values, batch.urls,
                      [batch.log_doc[int(s)] for s in src], batch.doc_actors, batch.doc_comments, batch.keys, batch.map_values,
                      chg_env_hi=cols["chg_env_hi"][:NC * es] if batch.chg_env_hi is not None else None)


def expected_status(o):
    """The cut's status from the oracle's first error: only the causal RangeError can come from a cut of an applied log."""
    if o["error"] is None:
        return 0
    assert o["error"]["kind"] == "Missing dependency", o["error"]
    return abi.ERR_MISSING_DEP


def check_cuts(case, batch, out, status, n_kept, first_row, clocks_out, then_rest):
    """Comparisons 1 and 2: status, n_kept, first_row and clocks_out are the oracle's; the Changes decoded from the cut log deep-equal the oracle's kept list
    (followed by its rest with then_rest), in order.  A failed cut is an empty log with zero outputs."""
    oracle, logs, text_obj = oracle_of(case, then_rest), SC.flat_logs(case), SC.text_obj_of(case)
    assert out.n_logs == len(case["cuts"]) and out.max_actors == batch.max_actors and (out.chg_env_hi is None) == (batch.chg_env_hi is None)
    for c, (cut, o) in enumerate(zip(case["cuts"], oracle)):
        want = expected_status(o)
        assert int(status[c]) == want, "cut %d: status %d, expected %d" % (c, int(status[c]), want)
        got = wire.decode_changes(out, c, text_obj=text_obj)
        if want:
            assert got == [] and int(out.log_off[c + 1]) == int(out.log_off[c]), "cut %d: a failed cut contributes an empty log" % c
            assert int(n_kept[c]) == 0 and int(first_row[c]) == 0 and not clocks_out[c].any()
            continue
        actors = batch.doc_actors[batch.log_doc[cut["log"]]]
        assert int(n_kept[c]) == len(o["kept"]), "cut %d: %d kept, expected %d" % (c, int(n_kept[c]), len(o["kept"]))
        assert int(first_row[c]) == o["keptRows"], "cut %d: first_row %d, expected %d" % (c, int(first_row[c]), o["keptRows"])
        assert {actors[a]: int(q) for a, q in enumerate(clocks_out[c]) if q} == o["clock"], "cut %d: effective clock" % c
        keyed = SC.by_key(logs[cut["log"]])
        order = o["kept"] + (o["rest"] if then_rest else [])
        assert [[x["actor"], x["seq"]] for x in got] == order, "cut %d: the cut log's order differs" % c
        assert got == [keyed[(a, q)] for a, q in order], "cut %d: the Changes of the cut log differ from the source's" % c


def check_merged(case, out, res, status, rm=None, pat=None, then_rest=False):
    """Comparisons 3 to 5: the merge WITH admission is OK and shows the oracle's spans at the version (then_rest: the source's present spans); ptx_root_map of
    the cut batch is the oracle's root at the version; with then_rest the patch stream from first_row on is the oracle's patch list of the rest."""
    oracle = oracle_of(case, then_rest)
    for c, o in enumerate(oracle):
        assert int(res.logs[c]["status"]) == 0, "cut %d: merge status %d" % (c, int(res.logs[c]["status"]))
        if int(status[c]):
            continue
        shown = o["atEnd"] if then_rest else o["atVersion"]
        if shown is not None:  # (a replica that holds no text list yet has nothing to show)
            H.check_log(out, res, c, shown)
        else:
            assert int(res.logs[c]["n_visible"]) == 0
        if rm is not None and not then_rest:
            assert int(rm.logs["status"][c]) == 0
            assert wire.decode_root(out, rm, c) == o["root"], "cut %d: root %r, expected %r" % (c, wire.decode_root(out, rm, c), o["root"])
        if pat is not None and then_rest:
            got, want = H.norm_patches(wire.decode_patches(out, pat, c)), H.norm_patches(o["restPatches"])
            assert got == want, "cut %d: the patch stream from the version differs (%d records, expected %d)" % (c, len(got), len(want))


def same_log(out, c, batch, l):
    """Log c of `out` holds the columns and the envelope of log l of `batch`, byte for byte."""
    a0, a1, b0, b1 = int(out.log_off[c]), int(out.log_off[c + 1]), int(batch.log_off[l]), int(batch.log_off[l + 1])
    for name in ("op_id", "ref_a", "ref_b", "payload", "action", "mark_type", "side_a", "side_b"):
        if not np.array_equal(getattr(out, name)[a0:a1], getattr(batch, name)[b0:b1]):
            return False
    es = abi.env_stride(batch.max_actors)
    a0, a1, b0, b1 = int(out.chg_off[c]), int(out.chg_off[c + 1]), int(batch.chg_off[l]), int(batch.chg_off[l + 1])
    same = np.array_equal(out.chg_hdr[a0:a1], batch.chg_hdr[b0:b1]) and np.array_equal(out.chg_env[a0 * es:a1 * es], batch.chg_env[b0 * es:b1 * es])
    if batch.chg_env_hi is not None:
        same = same and np.array_equal(out.chg_env_hi[a0 * es:a1 * es], batch.chg_env_hi[b0 * es:b1 * es])
    return same
