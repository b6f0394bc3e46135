"""Logs for the order words of a resident batch (merge_core.h ptx_order_word: per element its row and document position, and the tombstone words, kept by the
batch's first merge so that later merges run nothing of P3), shared by tests/test_emu_order_words.py and its GPU twin tests/test_gpu_order_words.py.

The logs of tests/order_check_cases.py come first, unchanged (n and D at the edges of P3a's steps and of its rest loop); behind them the cases the words add:
n at the edges of a 16-byte group of words and of a tombstone word, the deletions, the tree shapes that take P3c / P3d
down each of their paths, and the logs that fail; and, in a batch of their own (step_edge), n at the edges of a step of the reader's load loop.  Every expected answer
is the oracle's.

S is the number of items of one P3a step of the body under test and T its threads, as in order_check_cases; a step of the reader's load loop is
T threads x 2 loads x 4 words = 8 T elements."""
import functools
import random

import helpers as H
import order_check_cases as M
from peritext_amd import abi, wire

SMALL_BUCKET, HUGE_BUCKET = 8, 256  # merge_core.h PTX_SMALL_BUCKET, PTX_HUGE_BUCKET


def load_step(T):
    return 8 * T


def tree_log(parents, dels, seed, n_marks=M.N_MARKS):
    """ONE replica log of one actor: insert i is a child of insert parents[i] (-1: HEAD; parents[i] < i), then one delete per entry of `dels` (an insert's
    index; twice is fine), then n_marks addMark ops."""
    rnd = random.Random(seed)
    n = len(parents)
    ids = ["%d@doc1" % (2 + i) for i in range(n)]
    ops = [{"opId": "1@doc1", "action": "makeList", "obj": "_root", "key": "text"}]
    for i, p in enumerate(parents):
        assert -1 <= p < i
        ops.append({"opId": ids[i], "action": "set", "obj": "1@doc1", "elemId": "_head" if p < 0 else ids[p], "insert": True, "value": "abcdefghij"[rnd.randrange(10)]})
    changes = [{"actor": "doc1", "seq": 1, "deps": {}, "startOp": 1, "ops": ops}]
    ctr, seq = n + 2, 2
    for t in dels:
        changes.append({"actor": "doc1", "seq": seq, "deps": {}, "startOp": ctr, "ops": [{"opId": "%d@doc1" % ctr, "action": "del", "obj": "1@doc1", "elemId": ids[t]}]})
        ctr += 1
        seq += 1
    for m in range(n_marks if n else 0):
        changes.append({"actor": "doc1", "seq": seq, "deps": {}, "startOp": ctr,
                        "ops": [{"opId": "%d@doc1" % ctr, "action": "addMark", "obj": "1@doc1", "start": {"type": "before", "elemId": ids[rnd.randrange(n)]},
                                 "end": {"type": "endOfText"}, "markType": ("strong", "em")[m % 2]}]})
        ctr += 1
        seq += 1
    return changes


def three_actor_log(rounds, seed):
    """doc1 types three characters; then `rounds` times doc0, doc1 and doc2 — none knowing the others' op of the round — each insert a child of ONE element at ONE
    counter (concurrent siblings: the actor alone orders them), in an arrival order that changes from round to round; a delete and two mark ops behind."""
    rnd = random.Random(seed)
    ops = [{"opId": "1@doc1", "action": "makeList", "obj": "_root", "key": "text"}]
    ids = []
    for i in range(3):
        ids.append("%d@doc1" % (2 + i))
        ops.append({"opId": ids[-1], "action": "set", "obj": "1@doc1", "elemId": "_head" if i == 0 else ids[-2], "insert": True, "value": "abc"[i]})
    changes = [{"actor": "doc1", "seq": 1, "deps": {}, "startOp": 1, "ops": ops}]
    seq = {"doc0": 1, "doc1": 2, "doc2": 1}
    ctr = 5
    for r in range(rounds):
        parent = ids[rnd.randrange(len(ids))]
        deps = {a: s - 1 for a, s in seq.items() if s > 1}
        actors = ["doc0", "doc1", "doc2"]
        rnd.shuffle(actors)
        for a in actors:
            ids.append("%d@%s" % (ctr, a))
            changes.append({"actor": a, "seq": seq[a], "deps": {k: v for k, v in deps.items() if k != a}, "startOp": ctr,
                            "ops": [{"opId": ids[-1], "action": "set", "obj": "1@doc1", "elemId": parent, "insert": True, "value": "xyz"[r % 3]}]})
        for a in actors:
            seq[a] += 1
        ctr += 1
    deps = {a: s - 1 for a, s in seq.items() if a != "doc1"}
    changes.append({"actor": "doc1", "seq": seq["doc1"], "deps": deps, "startOp": ctr, "ops": [{"opId": "%d@doc1" % ctr, "action": "del", "obj": "1@doc1", "elemId": ids[4]}]})
    for m in range(2):
        ctr += 1
        seq["doc1"] += 1
        changes.append({"actor": "doc1", "seq": seq["doc1"], "deps": {}, "startOp": ctr,
                        "ops": [{"opId": "%d@doc1" % ctr, "action": "addMark", "obj": "1@doc1", "start": {"type": "before", "elemId": ids[rnd.randrange(len(ids))]},
                                 "end": {"type": "endOfText"}, "markType": ("strong", "em")[m]}]})
    return changes


SIZES = (0, 1, 3, 4, 5, 31, 32, 33, 63, 64, 65)  # n of the added logs: the edges of a 16-byte group of words and of a tombstone word


def step_edge_sizes(T):
    """n one short of, at and one past a full step of the reader's load loop."""
    L = load_step(T)
    return (L - 1, L, L + 1)


def added_logs(T):
    """-> [(name, log)] behind order_check_cases' own."""
    out = []
    for k, n in enumerate(SIZES):  # (order_check_cases' mix of parents; three deletes where there is room: a double delete and the last insert)
        out.append(("n=%d" % n, M.build_log(n, min(n, 3), 8100 + 13 * k)))
    chain = list(range(-1, 39))
    out.append(("D=0", tree_log(chain, [], 8301)))
    out.append(("D>n+1", M.build_log(12, 12 + 1 + T + 3, 8302)))  # (deletes beyond d_fused, more than one pass of the workgroup)
    out.append(("all deleted", tree_log(chain, list(range(40)), 8303)))  # V = 0
    out.append(("double delete", tree_log(chain, [7, 7, 39, 0, 0], 8304)))
    out.append(("chain", tree_log(list(range(-1, 329)), [5, 300], 8305)))  # typed left to right: the longest walks, the most jumping rounds
    out.append(("all children of HEAD", tree_log([-1] * (HUGE_BUCKET + 44), [0, 299, 150], 8306)))  # one bucket beyond PTX_HUGE_BUCKET: the bitmap rank
    # parents with PTX_SMALL_BUCKET children and with one more, an only child and a medium bucket between them
    par = [-1, 0, 1] + [0] * (SMALL_BUCKET - 1) + [1] * SMALL_BUCKET + [2] * 40 + [5, 30, 30]
    out.append(("small buckets", tree_log(par, [3, 12, 60], 8307)))
    out.append(("three actors", three_actor_log(9, 8308)))
    return out


@functools.lru_cache(maxsize=None)
def shapes(S, T):
    """-> (Batch of one log per case, [the oracle's {spans, text} per log], [name per log])."""
    sh = M.shape_list(S, T)
    logs = [M.build_log(n, D, 7300 + 17 * i) for i, (n, D) in enumerate(sh)]  # (order_check_cases.shapes' own logs)
    names = ["n=%d D=%d" % s for s in sh]
    for name, log in added_logs(T):
        names.append(name)
        logs.append(log)
    exp = [e[0] for e in H.oracle_apply([[l] for l in logs], no_patches=True)]
    for name, e in zip(names, exp):
        assert not e.get("error"), (name, e.get("error"))
    batch = wire.encode_docs([[l] for l in logs])
    batch.log_hdr = None  # (the library takes the census: the header's bounds come from the op ids alone)
    return batch, exp, names


@functools.lru_cache(maxsize=None)
def step_edge(T):
    """-> (Batch, [the oracle's answer per log], [name per log]): three logs at the edge of a step of the reader's load loop, a batch of their own.  With 192
    threads that is 1 535 / 1 536 / 1 537 elements, whose LDS window no longer lets nine logs share a CU: the library gives such a batch to the general build,
    which holds no order words — the three-wave lean build never takes a second step of that loop on the device (a log it takes has at most some 1 500
    elements); the emulation, whose step is 8 elements, does."""
    names = ["n=%d" % n for n in step_edge_sizes(T)]
    # (three deletes — or as many as it takes to pass the 2 048 rows from which the library launches three waves per log)
    logs = [M.build_log(n, max(3, 2052 - n) if T == 192 else 3, 8200 + 7 * k) for k, n in enumerate(step_edge_sizes(T))]
    exp = [e[0] for e in H.oracle_apply([[l] for l in logs], no_patches=True)]
    for name, e in zip(names, exp):
        assert not e.get("error"), (name, e.get("error"))
    batch = wire.encode_docs([[l] for l in logs])
    batch.log_hdr = None
    return batch, exp, names


@functools.lru_cache(maxsize=None)
def failing(S, T):
    """-> (Batch, [the oracle's answer per log], [expected status per log], [the edit or None]): order_check_cases' failing logs — an unknown parent, a delete of
    an unknown element, a parent's row after the child's, a delete's row before its target's, in the fused loop and on the rest path, between good logs — and one
    log that fails in P1: an op id on two rows, which the row pass names PTX_ERR_DUPLICATE_OP (the wire format's own rule; the oracle keys ops by id and has no
    such log, so this one status is the header's, peritext_hip.h)."""
    batch, exp, codes, fails = M.failing(S, T)
    n = S + 1
    specs = [(n, n, None)] + [(n, n + 1 + T + 1 if f.startswith("rest_") else n, f) for f in M.FAILS] + [(n, n + 1 + T + 1, None)]
    logs = [M.build_log(nn, D, 7900 + 19 * i, fail=f) for i, (nn, D, f) in enumerate(specs)]  # (order_check_cases.failing's own logs)
    dup = M.build_log(n, 4, 8400)
    dup[-3]["ops"][0]["opId"] = dup[-4]["ops"][0]["opId"]  # the last delete repeats the id of the one before it
    logs.append(dup)
    full = wire.encode_docs([[l] for l in logs])
    full.log_hdr = None
    assert full.n_logs == batch.n_logs + 1 and full.op_id[: batch.n_ops].tobytes() == batch.op_id.tobytes()
    return full, list(exp) + [None], list(codes) + [abi.ERR_DUPLICATE_OP], list(fails) + ["p1_duplicate_id"]


def bad_comment():
    """-> (Batch, bad log, its row, [the oracle's answer per log]): tests/mark_operand_cases.py's three logs with comment ops, the middle one with a comment id
    beyond its header's n_comment_ids — it passes P3 (its order words stand) and raises PTX_ERR_BAD_OP in P5a, in every merge."""
    import mark_operand_cases as MO

    return MO.bad_comment()
