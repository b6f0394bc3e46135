"""Shared by tests/test_emu_sync.py and tests/test_gpu_sync.py: the sync cases (documents, pairs), what the reference answers for them
(tests/sync_oracle.js over oracle/harness.js and oracle/peritext_oracle.js, computed once per case) and the three comparisons per pair.

A case is {"docs": [[log, ...], ...], "pairs": [(source log, target log), ...]} with the logs numbered across the documents in order, as
wire.encode_docs lays them out.  The hand-made logs hold one-op changes: change 1 of the list's author makes the text list, every other change
inserts one character at the head (valid in any order once the list exists), so only the envelopes decide what happens."""
import functools
import json
import os
import random
import tempfile

import helpers as H
from peritext_amd import abi, wire

REFERENCE_GUARD = 10001  # reference/test/merge.ts:18: the 10 002nd attempt throws


# ---- the oracle ----
def oracle_sync(pairs):
    """[(source log, target log)] -> what tests/sync_oracle.js answers per pair."""
    with tempfile.TemporaryDirectory() as td:
        inp, out = os.path.join(td, "in.json"), os.path.join(td, "out.json")
        with open(inp, "w") as f:
            json.dump({"pairs": [{"source": s, "target": t} for s, t in pairs]}, f)
        H.run_node(["tests/sync_oracle.js", inp, out])
        with open(out) as f:
            return json.load(f)["pairs"]


def flat_logs(case):
    return [log for doc in case["docs"] for log in doc]


def with_oracle(case):
    logs = flat_logs(case)
    case["oracle"] = oracle_sync([(logs[s], logs[t]) for s, t in case["pairs"]])
    return case


# ---- hand-made logs ----
def change(actor, seq, deps, ctr, make_list=False):
    op = ({"opId": "%d@%s" % (ctr, actor), "action": "makeList", "obj": "_root", "key": "text"} if make_list else
          {"opId": "%d@%s" % (ctr, actor), "action": "set", "obj": TEXT, "elemId": "_head", "insert": True, "value": chr(97 + (ctr + seq) % 26)})
    return {"actor": actor, "seq": seq, "deps": dict(deps), "startOp": ctr, "ops": [op]}


TEXT = "1@a"  # the text list of every hand-made document: made by change 1 of actor `a`


def first_change():
    return change("a", 1, {}, 1, make_list=True)


def run_of(actor, n, deps_of, seq0=1, ctr0=1000):
    """n one-op changes of `actor`, seq0 .. ; deps_of(k) = deps of the k-th (0-based)."""
    return [change(actor, seq0 + k, deps_of(k), ctr0 + k) for k in range(n)]


@functools.lru_cache(maxsize=None)
def chunk_edge_case():
    """A single actor's run of 63 / 64 / 65 / 129 missing changes, and runs of 135 whose first failing change stands at lane 0, at lane 63 and at the first
    lane of the second chunk of the 64-change steps (it waits for a change of an actor that first appears AFTER the run's actor)."""
    a1 = first_change()
    docs, pairs = [], []
    for n in (63, 64, 65, 129):
        src = [a1] + run_of("b", n, lambda k: {"a": 1})
        docs.append([src, [a1]])
        pairs.append((2 * len(docs) - 2, 2 * len(docs) - 1))
    for f in (0, 63, 64):
        have = run_of("b", 5, lambda k: {"a": 1})
        c1 = change("c", 1, {"a": 1}, 5000)
        rest = run_of("b", 135, lambda k: {"a": 1, "c": 1} if k == f else {"a": 1}, seq0=6, ctr0=1005)
        docs.append([[a1] + have + [c1] + rest, [a1] + have])
        pairs.append((2 * len(docs) - 2, 2 * len(docs) - 1))
    return with_oracle({"docs": docs, "pairs": pairs})


def actor_names(n):
    """n actor ids whose rank order (UTF-16 order) is their index order; `a` (rank 0) makes the list."""
    return ["a"] + ["p%02d" % k for k in range(1, n)]


@functools.lru_cache(maxsize=None)
def actor_order_case():
    """Documents of 1, 3, 4, 7, 8, 15 and 17 actors (envelope rows of 4 .. 20 u16, past one row of 16) whose first-appearance order in the source is the
    REVERSE of the rank order; every actor's second change waits for the first change of the actor that appears next, so every run but the last needs a
    second pass.  The last document: a dep column that is not monotone along a run (p01: deps on p02 of 0, 2, 1, 0), the target already holding p02's first."""
    a1 = first_change()
    docs, pairs = [], []
    for n in (1, 3, 4, 7, 8, 15, 17):
        names = actor_names(n)
        if n == 1:
            src = [a1] + run_of("a", 5, lambda k: {"a": k + 1}, seq0=2, ctr0=2)
        else:
            order = names[:0:-1]  # p(n-1) .. p01: descending rank
            firsts = [change(x, 1, {"a": 1}, 100 + 10 * i) for i, x in enumerate(order)]
            seconds = [change(x, 2, {"a": 1, order[i + 1]: 1} if i + 1 < len(order) else {"a": 1}, 101 + 10 * i) for i, x in enumerate(order)]
            src = [a1] + firsts + seconds
        docs.append([src, [a1]])
        pairs.append((2 * len(docs) - 2, 2 * len(docs) - 1))
    p2 = run_of("p02", 2, lambda k: {"a": 1}, ctr0=300)
    p1 = [change("p01", 1, {"a": 1}, 200), change("p01", 2, {"a": 1, "p02": 2}, 201), change("p01", 3, {"a": 1, "p02": 1}, 202), change("p01", 4, {"a": 1}, 203)]
    docs.append([[a1, p1[0]] + p2 + p1[1:], [a1, p2[0]]])
    pairs.append((2 * len(docs) - 2, 2 * len(docs) - 1))
    return with_oracle({"docs": docs, "pairs": pairs})


@functools.lru_cache(maxsize=None)
def target_edge_case():
    """An empty target; a target ahead of its source; src == dst; a log that is a source and a target at once (4 -> 5 and 5 -> 6 both read the base as it is: 6 gets what 5 holds now)."""
    a1 = first_change()
    b = run_of("b", 4, lambda k: {"a": 1})
    docs = [[[a1] + b, []], [[a1] + b[:2], [a1] + b], [[a1] + b, [a1] + b[:1], [a1]]]
    pairs = [(0, 1), (2, 3), (4, 4), (4, 5), (5, 6)]
    return with_oracle({"docs": docs, "pairs": pairs})


def ping_pong(rounds, independent):
    """`rounds` rounds of two actors answering each other (a_k waits for b_k-1, b_k for a_k), then `independent` changes of a third actor that wait for
    nothing, pulled by a fresh replica: T = rounds * (rounds + 1) + independent attempts."""
    src, ctr = [], 1
    for k in range(1, rounds + 1):
        src.append(change("a", k, {"b": k - 1} if k > 1 else {}, ctr, make_list=(k == 1)))
        src.append(change("b", k, {"a": k}, ctr + 1))
        ctr += 2
    src += run_of("c", independent, lambda k: {}, ctr0=ctr)
    return [src, []]


GUARD_SHAPES = [(99, 0, 9900), (100, 0, 10100), (99, 101, 10001), (99, 102, 10002)]  # (rounds, independent changes, attempts T)


@functools.lru_cache(maxsize=None)
def guard_case():
    """The four ping-pong shapes around the reference's guard, and a source holding a change with a dep nobody can meet (a log no replica could have applied)."""
    docs = [ping_pong(r, i) for r, i, _ in GUARD_SHAPES]
    a1 = first_change()
    docs.append([[a1, change("b", 1, {"a": 7}, 50), change("b", 2, {"a": 1}, 51)], [a1]])
    pairs = [(2 * d, 2 * d + 1) for d in range(len(docs))]
    return with_oracle({"docs": docs, "pairs": pairs})


@functools.lru_cache(maxsize=None)
def redeal_case(config, replicas=None, both_ways=False):
    """Replicas that have seen different, causally closed parts of a generated history (helpers.redeal_logs).  both_ways: the bidirectional sync of replicas
    (0, 1) — and (2, 3) — as the pairs (l, r), (r, l) of one call.  Otherwise EVERY ordered pair of a document in one call: a log is the target of one pair only,
    so the document carries, behind its re-dealt logs, one more copy of the target per ordered pair."""
    gen = H.oracle_gen(config, docs=2, seed=11, ops=160 if config == "rich" else None, replicas=replicas)
    rng = random.Random(5)
    docs, pairs, base = [], [], 0
    for d in gen["docs"]:
        n = len(d["logs"])
        logs = []
        while len(logs) < n:  # (sub-logs without the makeList change are left out by redeal_logs)
            logs += H.redeal_logs(d["logs"], rng, n - len(logs))
        if both_ways:
            for l in range(0, n - 1, 2):
                pairs += [(base + l, base + l + 1), (base + l + 1, base + l)]
        else:
            for s in range(n):
                for t in range(n):
                    if s != t:
                        logs.append(list(logs[t]))
                        pairs.append((base + s, base + len(logs) - 1))
        docs.append(logs)
        base += len(logs)
    return with_oracle({"docs": docs, "pairs": pairs})


def typed_log(n_changes, actor="a", first_ctr=1, make_list=True, deps_of=None):
    """One change per keystroke (test_emu_biglog._typed_log, the way tests/make_wide_envelope_golden.py's documents are made): change 1 makes the list, every
    further one inserts one character at the head."""
    log, ctr = [], first_ctr
    for k in range(n_changes):
        log.append(change(actor, 1 + k, deps_of(k) if deps_of else {}, ctr, make_list=(k == 0 and make_list)))
        ctr += 1
    return log


def wide_case_docs():
    """Seqs beyond 65 535 (the wide envelope column): the source holds 65 560 changes of `a` and three of `b` that wait for a's 65 550th; the target has a's
    first 65 530."""
    a = typed_log(65560)
    b = typed_log(3, actor="b", first_ctr=70001, make_list=False, deps_of=lambda k: {"a": 65550})
    return {"docs": [[a[:65550] + b + a[65550:], a[:65530]]], "pairs": [(0, 1)]}


def wide_case():
    """wide_case_docs() with the oracle's answer from the committed fixture (tests/make_sync_wide_golden.py), refused if it was made for other logs."""
    case = wide_case_docs()
    g = H._load_golden("sync_wide_ref.json")
    assert g["inputs_sha16"] == H.inputs_sha16(case["docs"]), "tests/golden/sync_wide_ref.json was made for other logs: rerun tests/make_sync_wide_golden.py"
    case["oracle"] = g["oracle"]
    return case


def session_script(n_docs=4, replicas=3, rounds=12, seed=3):
    """The reference fuzzer's step (test/fuzz.ts:165-199) as a fixed script: per round and document one replica makes a change() — an insert, sometimes with a
    mark over the first characters (no deletes: every index stays valid on every replica) — and two random replicas sync in both directions; three more rounds
    without an edit sync all pairs."""
    rng = random.Random(seed)
    out = []
    for k in range(rounds):
        steps = []
        for d in range(n_docs):
            ops = [{"path": ["text"], "action": "insert", "index": rng.randint(0, 5), "values": [chr(97 + (k + d) % 26)]}]
            if rng.random() < 0.4:
                ops.append({"path": ["text"], "action": "addMark", "markType": rng.choice(["strong", "em"]), "startIndex": rng.randint(0, 2), "endIndex": rng.randint(3, 5)})
            left = rng.randrange(replicas)
            steps.append({"edit": {"replica": rng.randrange(replicas), "ops": ops}, "sync": [left, (left + 1 + rng.randrange(replicas - 1)) % replicas]})
        out.append(steps)
    for l, r in ((0, 1), (0, 2), (1, 2)):
        out.append([{"edit": None, "sync": [l, r]} for _ in range(n_docs)])
    return {"docs": n_docs, "replicas": replicas, "text": "ABCDE", "rounds": out}


@functools.lru_cache(maxsize=None)
def session_oracle():
    script = session_script()
    with tempfile.TemporaryDirectory() as td:
        inp, out = os.path.join(td, "in.json"), os.path.join(td, "out.json")
        with open(inp, "w") as f:
            json.dump(script, f)
        H.run_node(["tests/sync_oracle.js", "--session", inp, out])
        with open(out) as f:
            return script, json.load(f)


# ---- running a case ----
def encode(case):
    return wire.encode_docs(case["docs"], text_objs=[case.get("text_obj")] * len(case["docs"]) if case.get("text_obj") else None)


def by_key(log):
    return {(c["actor"], c["seq"]): c for c in log}


def text_obj_of(case):
    for log in flat_logs(case):
        for c in log:
            for op in c["ops"]:
                if op["action"] == "makeList":
                    return op["opId"]
    return None


def expected_status(o, max_attempts):
    """What the reference's loop does, as a per-pair status: stuck (a pass admits nothing) or more attempts than the guard allows = not converged."""
    if o["stuck"] or (max_attempts and o["attempts"] > max_attempts):
        return abi.ERR_SYNC_NOT_CONVERGED
    return 0


def check_order(case, batch, more, status, max_attempts=REFERENCE_GUARD):
    """Comparison 1: the Changes decoded from `more` are deep-equal to the oracle's `applied`, in order (the guard-free twin's order at max_attempts = 0);
    a failed pair and every log that is no target are empty.  Returns the grown logs (target ++ applied) per log of the batch."""
    logs = flat_logs(case)
    grown = [list(log) for log in logs]
    targets = set()
    for p, (s, t) in enumerate(case["pairs"]):
        o = case["oracle"][p]
        want_status = expected_status(o, max_attempts)
        assert int(status[p]) == want_status, "pair %d (%d -> %d): status %d, expected %d (T = %r)" % (p, s, t, int(status[p]), want_status, o["attempts"])
        if max_attempts == REFERENCE_GUARD:
            assert o["threw"] == (want_status != 0), "pair %d: the harness %s" % (p, "threw" if o["threw"] else "did not throw")
        targets.add(t)
        got = wire.decode_changes(more, t, text_obj=text_obj_of(case))
        if want_status != 0 or s == t:
            assert got == [], "pair %d: a failed pair contributes an empty log" % p
            continue
        order = o["applied"] if max_attempts == REFERENCE_GUARD else o["twin"]
        keyed = by_key(logs[s])
        want = [keyed[(a, q)] for a, q in order]
        assert [(c["actor"], c["seq"]) for c in got] == [(c["actor"], c["seq"]) for c in want], "pair %d (%d -> %d): admitted order differs" % (p, s, t)
        assert got == want, "pair %d: the Changes of `more` differ from the source's" % p
        grown[t] = logs[t] + want
    for l in range(batch.n_logs):
        if l not in targets:
            assert int(more.log_off[l + 1]) == int(more.log_off[l]) and int(more.chg_off[l + 1]) == int(more.chg_off[l]), "log %d is no target and must be empty" % l
    assert more.max_actors == batch.max_actors and (more.chg_env_hi is None) == (batch.chg_env_hi is None)
    return grown


def regroup(case, per_log):
    out, at = [], 0
    for doc in case["docs"]:
        out.append(per_log[at:at + len(doc)])
        at += len(doc)
    return out


def check_grown(case, grown_batch, grown_logs, res, pat):
    """Comparisons 2 and 3: after the append, the merge WITH admission says OK for every target and shows what the oracle shows for target ++ applied, and
    the grown logs' patch streams are the oracle's."""
    docs = regroup(case, grown_logs)
    expected = H.oracle_apply(docs, patches=True)
    flat = flat_logs(case)
    ok_targets = {t for s, t in case["pairs"] if len(grown_logs[t]) > len(flat[t])}
    log = 0
    for d, exp in enumerate(expected):
        for r, e in enumerate(exp):
            if "error" in e and grown_logs[log] and log not in ok_targets:  # (a hand-made source no replica could have applied: the merge's admission says so too)
                assert int(res.logs[log]["status"]) in (abi.ERR_SEQ_GAP, abi.ERR_MISSING_DEP), e
            elif grown_logs[log]:  # (a replica that holds nothing yet has no text list to show)
                assert "error" not in e, e
                H.check_log(grown_batch, res, log, e)
            else:
                assert int(res.logs[log]["status"]) == 0
            log += 1
    if pat is not None:  # (helpers.check_patch_streams log by log: a log the reference throws on has no stream)
        log = 0
        for exp in expected:
            for e in exp:
                if "error" not in e:
                    got, want = H.norm_patches(wire.decode_patches(grown_batch, pat, log)), H.norm_patches(e["patches"])
                    assert got == want, "log %d: the patch stream differs (%d records, expected %d)" % (log, len(got), len(want))
                log += 1


def more_from_columns(batch, cols, log_off, chg_off):
    """wire.Batch of a `more` given as raw columns (the emulation's output), with the tables of `batch`."""
    T, NC, es = int(log_off[-1]), int(chg_off[-1]), abi.env_stride(batch.max_actors)
    return wire.Batch(log_off, cols["op_id"][:T], cols["ref_a"][:T], cols["ref_b"][:T], cols["payload"][:T], cols["action"][:T], cols["mark_type"][:T], cols["side_a"][:T],
                      cols["side_b"][:T], chg_off, cols["chg_hdr"][:NC], cols["chg_env"][:NC * es], batch.max_actors, None, batch.values, batch.urls, batch.log_doc,
                      batch.doc_actors, batch.doc_comments, batch.keys, batch.map_values, chg_env_hi=cols["chg_env_hi"][:NC * es] if batch.chg_env_hi is not None else None)
