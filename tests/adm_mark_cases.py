"""Logs for the admission marks of a resident batch (merge_core.h ptx_adm_mark), shared by tests/test_emu_adm_marks.py and its GPU twin
tests/test_gpu_adm_marks.py: a three-actor replica log cut into a BASE (its first m changes) and a GROWN log (its first m + s changes), the appended part intact
or with one change made inadmissible.  Everything expected of a grown log is the oracle's answer for the whole grown log; which change fails first — and so the
error row — is pinned by two more oracle replays per mutated log (the changes before it are accepted, with it they are rejected)."""
import copy
import functools

import numpy as np

import helpers as H
from peritext_amd import abi, wire

KINDS = ("seq_gap", "seq_repeat", "dep_missing")
SUFFIXES = (1, 255, 256, 257, 768, 769)  # in changes: one, and the edges of one step of a wave (256 changes) and of three waves' (768)


def _mutated(log, lo, hi, kind, n_by_actor):
    """`log` with one change of [lo, hi) made inadmissible; returns (log, index of that change)."""
    log = list(log)
    if kind == "seq_gap":  # a seq skipped, at the end of the range
        p = hi - 1
        c = copy.deepcopy(log[p])
        c["seq"] += 1
    elif kind == "seq_repeat":  # the seq of the actor's previous change again, as early in the range as an actor has one
        p = next(i for i in list(range(lo, hi)) + list(range(lo - 1, -1, -1)) if log[i]["seq"] > 1)
        c = copy.deepcopy(log[p])
        c["seq"] -= 1
    else:  # a dependency on a change no prefix of this log holds, in the middle of the range
        p = (lo + hi) // 2
        c = copy.deepcopy(log[p])
        other = sorted(a for a in n_by_actor if a != c["actor"])[0]
        c["deps"] = dict(c.get("deps") or {})
        c["deps"][other] = n_by_actor[other] + 3
    log[p] = c
    return log, p


def _code(exp):
    err = exp.get("error")
    if not err:
        return 0
    for needle, code in (("Expected sequence number", abi.ERR_SEQ_GAP), ("Missing dependency", abi.ERR_MISSING_DEP)):
        if needle in err:
            return code
    raise AssertionError("unexpected oracle error: " + err)


@functools.lru_cache(maxsize=None)
def cases(ops, max_changes=None):
    """-> dict(base=Batch, grown=Batch, cases=[dict(m, s, kind, merged, p, exp, code, row)]): log l of both batches belongs to case l.
    merged: the base is merged before it grows (False: a never-merged base — its marks are still zero).  kind 'bad_base': the inadmissible change sits in the BASE.
    max_changes: only the cases whose grown log has at most so many changes (short logs: the one-wave build)."""
    gen = H.oracle_gen("mini", 1, 7, ops, 3)
    full = gen["docs"][0]["logs"][0]
    ct = len(full)
    n_by_actor = {}
    for c in full:
        n_by_actor[c["actor"]] = n_by_actor.get(c["actor"], 0) + 1
    assert len(n_by_actor) == 3 and ct >= 769 + 1, (ct, n_by_actor)
    m_of = {1: ct - 1, 255: 90, 256: 64, 257: 33, 768: ct - 768 if ct - 768 < 61 else 61, 769: 1}  # mark positions 1 and C - 1 among them
    spec = [(m_of[s], s, k, True) for s in SUFFIXES for k in ("valid",) + KINDS]
    spec += [(0, 257, "valid", True), (0, 90, "seq_gap", True)]             # mark position 0: the base is an empty log
    spec += [(64, 256, "valid", False), (33, 257, "dep_missing", False)]   # a base that was never merged
    spec += [(90, 255, "bad_base", True), (90, 1, "bad_base", True)]        # a base that failed: nothing of it is marked
    if max_changes is not None:
        spec = [x for x in spec if x[0] + x[1] <= max_changes]
    out, base_logs, grown_logs = [], [], []
    for m, s, kind, merged in spec:
        grown, p = full[: m + s], None
        if kind == "bad_base":
            grown, p = _mutated(grown, 0, m, "seq_gap", n_by_actor)
        elif kind != "valid":
            grown, p = _mutated(grown, m, m + s, kind, n_by_actor)
        base_logs.append(grown[:m])
        grown_logs.append(grown)
        out.append(dict(m=m, s=s, kind=kind, merged=merged, p=p))
    probes = []
    for c, g in zip(out, grown_logs):
        if c["p"] is not None:
            probes += [g[: c["p"]], g[: c["p"] + 1]]
    exp = H.oracle_apply([[l] for l in grown_logs + probes], no_patches=True)
    actors = sorted(n_by_actor)
    comments = sorted({op["attrs"]["id"] for c in full for op in c["ops"] if op.get("markType") == "comment"})
    enc = lambda logs: wire.encode_docs([[l] for l in logs], extra_actors=[actors] * len(logs), extra_comments=[comments] * len(logs))  # noqa: E731
    base, grown = enc(base_logs), enc(grown_logs)
    base.log_hdr = grown.log_hdr = None  # (the library takes the census)
    assert base.max_actors == 3 and grown.max_actors == 3
    k = len(grown_logs)
    for l, c in enumerate(out):
        c["exp"] = exp[l][0]
        c["code"] = _code(c["exp"])
        c["row"] = None
        if c["p"] is not None:
            before, with_it = exp[k][0], exp[k + 1][0]
            k += 2
            # the oracle itself: the changes before p are admitted, p is not, and for the reason the whole log is rejected for
            assert _code(before) == 0 and _code(with_it) == c["code"] != 0, (c, before.get("error"), with_it.get("error"))
            c0 = int(grown.chg_off[l])
            c["row"] = int(grown.chg_nops[c0: c0 + c["p"]].sum())
        else:
            assert c["code"] == 0, c
    rejected = {kd: sum(1 for c in out if c["kind"] == kd and c["code"] != 0) for kd in KINDS}
    assert all(rejected.values()), "vacuous: the oracle rejected no log of some mutation kind: %r" % (rejected,)
    return dict(base=base, grown=grown, cases=out)


def clock_record(batch, log, n_changes=None):
    """The record a fully admitted log must carry, from the batch's own envelope columns: [changes, rows, clock0 | clock1 << 16, clock2]."""
    c0, c1 = int(batch.chg_off[log]), int(batch.chg_off[log + 1])
    if n_changes is not None:
        c1 = c0 + n_changes
    cnt = np.bincount(batch.chg_actor[c0:c1].astype(np.int64), minlength=3)
    return [c1 - c0, int(batch.chg_nops[c0:c1].sum()), int(cnt[0]) | (int(cnt[1]) << 16), int(cnt[2])]


def check_grown(case, batch, res, log):
    """One log of a merge of the grown batch against the oracle's answer for the whole log: status = error code, error row, result rows."""
    st, row = int(res.logs["status"][log]), int(res.logs["reserved"][log, 1])
    assert st == case["code"], (case["m"], case["s"], case["kind"], st, case["code"], case["exp"].get("error"))
    if case["code"]:
        assert row == case["row"], (case["m"], case["s"], case["kind"], row, case["row"])
    else:
        H.check_log(batch, res, log, case["exp"])
