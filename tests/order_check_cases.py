"""Logs for the row-order checks of P3a / P3b that a standing log of a resident batch does not run again (merge_core.h PtxMergeArgs::order_checks_once), shared
by tests/test_emu_order_checks.py and its GPU twin tests/test_gpu_order_checks.py: hand-sized replica logs of n inserts and D deletes at the edges of P3a's steps
and of its rest loop, with every kind of parent and target, each with the oracle's answer; and the logs that pass the row pass and fail in P3a or P3b.

S is the number of items of one P3a step of the body under test (threads x PTX_U), T its threads: the emulation walks S = 2, T = 1; the one-, two- and three-wave
lean builds S = 64, 256 and 384."""
import functools
import random

import helpers as H
from peritext_amd import abi, wire

N_MARKS = 2  # (a couple of mark ops behind the deletes: P5a runs, the log's word has something to stand for)


def step_values(S):
    """n and D each: 0, 1, S - 1, S, S + 1, 2S - 1, 2S, 2S + 1, 3S + 1 — odd and even step counts, each edge of a step from both sides."""
    return sorted({0, 1, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 3 * S + 1})


def shape_list(S, T):
    """(n, D): every n of step_values with D = 0, D = n, D = n + 1 (all fused), D = n + 2 (a rest loop of one item) and D = n + 1 + T + 1 (a rest loop of more than
    one pass of the workgroup).  D = n takes D through step_values too.  A log without an insert has no delete that passes."""
    out = []
    for n in step_values(S):
        for D in (0, n, n + 1, n + 2, n + 1 + T + 1):
            if (n or not D) and (n, D) not in out:
                out.append((n, D))
    return out


def build_log(n, D, seed, fail=None):
    """ONE replica log of n inserts, D deletes and N_MARKS mark ops (when n > 0), two actors where n allows it.  Inserts: doc1 types a chain — every parent the
    log's last insert — with a HEAD parent at the start and at every seventh insert; doc0 then inserts two elements behind elements of doc1, and doc1 one behind
    doc0's last (another actor's element).  Deletes: the first two hit ONE element (deleting twice is fine), the third the log's last insert, the rest random ones.
    fail: None, or the one edit that makes the log fail (see failing())."""
    rnd = random.Random(seed)
    nb = 2 if n >= 6 else 0          # doc0's inserts
    n1 = n - nb - (1 if nb else 0)   # doc1's first run
    ops = [{"opId": "1@doc1", "action": "makeList", "obj": "_root", "key": "text"}]
    ids = []
    ctr = 2
    for i in range(n1):
        ids.append("%d@doc1" % ctr)
        ops.append({"opId": ids[-1], "action": "set", "obj": "1@doc1", "elemId": "_head" if i % 7 == 0 else ids[-2], "insert": True, "value": "abcdefghij"[rnd.randrange(10)]})
        ctr += 1
    changes = [{"actor": "doc1", "seq": 1, "deps": {}, "startOp": 1, "ops": ops}]
    seq = 2
    if nb:
        ops0 = []
        for k in range(nb):
            ids.append("%d@doc0" % ctr)
            ops0.append({"opId": ids[-1], "action": "set", "obj": "1@doc1", "elemId": ids[rnd.randrange(n1)] if k == 0 else ids[-2], "insert": True, "value": "XY"[k]})
            ctr += 1
        changes.append({"actor": "doc0", "seq": 1, "deps": {"doc1": 1}, "startOp": ctr - nb, "ops": ops0})
        ids.append("%d@doc1" % ctr)
        changes.append({"actor": "doc1", "seq": seq, "deps": {"doc0": 1}, "startOp": ctr,
                        "ops": [{"opId": ids[-1], "action": "set", "obj": "1@doc1", "elemId": ids[-2], "insert": True, "value": "Z"}]})
        ctr += 1
        seq += 1
    assert len(ids) == n
    first_del = len(changes)
    for d in range(D):
        target = ids[n // 2] if d < 2 else ids[-1] if d == 2 else ids[rnd.randrange(n)]
        changes.append({"actor": "doc1", "seq": seq, "deps": {}, "startOp": ctr, "ops": [{"opId": "%d@doc1" % ctr, "action": "del", "obj": "1@doc1", "elemId": target}]})
        ctr += 1
        seq += 1
    for m in range(N_MARKS if n else 0):
        a = rnd.randrange(n)
        changes.append({"actor": "doc1", "seq": seq, "deps": {}, "startOp": ctr,
                        "ops": [{"opId": "%d@doc1" % ctr, "action": "addMark", "obj": "1@doc1", "start": {"type": "before", "elemId": ids[a]}, "end": {"type": "endOfText"},
                                 "markType": ("strong", "em")[m % 2]}]})
        ctr += 1
        seq += 1
    last = lambda k: changes[k]["ops"][0]  # noqa: E731
    if fail == "parent_out_of_bounds":      # a parent id beyond the header's bounds: key 0
        changes[0]["ops"][1 + n1 // 2]["elemId"] = "99999@doc1"
    elif fail == "parent_never_inserted":   # within the bounds, the id of a delete op: no element has it
        changes[0]["ops"][1 + n1 // 2]["elemId"] = last(first_del)["opId"]
    elif fail == "parent_inserted_later":   # the id of the insert that follows
        changes[0]["ops"][1 + n1 // 2]["elemId"] = ids[n1 // 2 + 1]
    elif fail == "delete_unknown":
        last(first_del + D // 2)["elemId"] = "99999@doc1"
    elif fail in ("delete_inserted_later", "rest_delete_inserted_later"):  # an insert behind everything, deleted by a delete before it
        later = "%d@doc1" % ctr
        changes.append({"actor": "doc1", "seq": seq, "deps": {}, "startOp": ctr,
                        "ops": [{"opId": later, "action": "set", "obj": "1@doc1", "elemId": ids[0], "insert": True, "value": "!"}]})
        last(first_del + (D // 2 if fail == "delete_inserted_later" else D - 1))["elemId"] = later
    elif fail == "rest_delete_unknown":     # the last delete: on the rest path when D > n + 1
        last(first_del + D - 1)["elemId"] = "99999@doc1"
    else:
        assert fail is None
    return changes


def _batch(logs):
    batch = wire.encode_docs([[l] for l in logs])
    batch.log_hdr = None  # (the library takes the census: the header's bounds come from the op ids alone)
    return batch


@functools.lru_cache(maxsize=None)
def shapes(S, T):
    """-> (Batch of one log per shape, [the oracle's {spans, text} per log], [(n, D)])."""
    sh = shape_list(S, T)
    logs = [build_log(n, D, 7300 + 17 * i) for i, (n, D) in enumerate(sh)]
    exp = [e[0] for e in H.oracle_apply([[l] for l in logs], no_patches=True)]
    batch = _batch(logs)
    for l, (n, D) in enumerate(sh):
        assert int(batch.log_off[l + 1] - batch.log_off[l]) == 1 + n + D + (N_MARKS if n else 0)
        assert not exp[l].get("error"), (n, D, exp[l].get("error"))
    return batch, exp, sh


FAILS = ("parent_out_of_bounds", "parent_never_inserted", "parent_inserted_later", "delete_unknown", "delete_inserted_later", "rest_delete_unknown",
         "rest_delete_inserted_later")


def _code(exp):
    err = exp.get("error")
    if not err:
        return 0
    assert "not found" in err, err  # micromerge.ts:752, the one error P3a and P3b raise
    return abi.ERR_ELEM_NOT_FOUND


@functools.lru_cache(maxsize=None)
def failing(S, T):
    """-> (Batch, [the oracle's answer per log], [the status the oracle's answer stands for], [the edit or None]): logs that pass the row pass — their rows are
    well-formed, their headers exact, their ids distinct — and fail in P3a or P3b, between good ones.  n = S + 1 inserts (a second step); the deletes of the
    rest-path cases reach more than one pass of the workgroup behind the fused ones."""
    n = S + 1
    specs = [(n, n, None)] + [(n, n + 1 + T + 1 if f.startswith("rest_") else n, f) for f in FAILS] + [(n, n + 1 + T + 1, None)]
    logs = [build_log(nn, D, 7900 + 19 * i, fail=f) for i, (nn, D, f) in enumerate(specs)]
    exp = [e[0] for e in H.oracle_apply([[l] for l in logs], no_patches=True)]
    codes = [_code(e) for e in exp]
    assert [c != 0 for c in codes] == [f is not None for _, _, f in specs], codes  # the oracle itself accepts or refuses each case as intended
    return _batch(logs), exp, codes, [f for _, _, f in specs]
