"""Logs for the operand words of a resident batch's mark ops (merge_core.h ptx_mark_operand_pack), shared by tests/test_emu_mark_operands.py and its GPU twin
tests/test_gpu_mark_operands.py: hand-sized replica logs (n inserts, D deletes, K mark ops, one makeList row) at the edges of P5a's blocks and steps, with every
kind of operand the second form of its loop has to tell apart, each with the oracle's answer; and the logs that pass the row pass and fail later."""
import copy
import functools

import helpers as H
from peritext_amd import abi, wire

# (n, D, K, edit): a block of P5a is one wave's 64 lanes, a step one block per wave — K = 0, 1, 63, 64, 65, 127, 128, 129 for every build, 191, 192, 193 and 385 for
# the three-wave one; few inserts, so that the one-wave build's 512 rows and its LDS window admit them all.  The random logs have four type runs of uneven lengths.
SHAPES = (
    (17, 0, 0, None), (24, 1, 1, None), (24, 0, 63, None), (31, 2, 64, None), (24, 0, 65, None), (19, 3, 127, None), (40, 0, 128, None), (24, 1, 129, None),
    (24, 0, 191, None), (33, 2, 192, None), (24, 0, 193, None), (24, 5, 385, None),
    (24, 0, 70, "no_em"), (24, 1, 70, "no_strong"), (24, 0, 66, "no_comment"), (24, 2, 130, "no_link"), (24, 0, 9, "only_comment"),
    (20, 2, 48, "operands"), (20, 0, 200, "operands"),
)


def _retype(op, mt, j):
    op["markType"] = mt
    op.pop("attrs", None)
    if mt == "link" and op["action"] == "addMark":
        op["attrs"] = {"url": "%s.com" % "ABC"[j % 3]}
    if mt == "comment":
        op["attrs"] = {"id": "comment-%d" % (j % 3)}


def _edit(log, n, D, K, edit):
    marks = [c["ops"][0] for c in log[1 + D: 1 + D + K]]
    el = lambda i: "%d@doc1" % (2 + i)  # noqa: E731  the element id of character i
    if edit and edit.startswith("no_"):  # one run empty: its ops go to the next type
        gone = edit[3:]
        for j, op in enumerate(marks):
            if op["markType"] == gone:
                _retype(op, {"em": "strong", "strong": "em", "comment": "link", "link": "comment"}[gone], j)
    if edit == "only_comment":
        for j, op in enumerate(marks):
            _retype(op, "comment", j)
    if edit == "operands":
        later = "%d@doc1" % (n + 2 + D + K)  # the id of the insert that follows every mark op
        bf = lambda e: {"type": "before", "elemId": e}  # noqa: E731
        af = lambda e: {"type": "after", "elemId": e}  # noqa: E731
        eot, sot = {"type": "endOfText"}, {"type": "startOfText"}
        hand = [
            (bf("9999@doc1"), af(el(5))),   # a start whose counter is beyond the header's: key 0
            (bf(el(2)), af("9999@doc1")),   # ... an end
            (bf("7@zz"), af(el(9))),        # an actor the header does not know
            (bf(el(3)), bf("7@zz")),
            (bf(later), af(el(12))),        # a start on an element inserted later in the log: the op never starts
            (af(later), eot),
            (bf(el(4)), af(later)),         # ... an end on it: never reached, the mark runs to the end of the text
            (bf(el(1)), bf(later)),
            (bf(el(6)), bf(el(6))),         # start and end on the same slot
            (af(el(6)), af(el(6))),
            (bf(el(7)), eot),               # an end-of-text end
            (af(el(0)), eot),
            (sot, af(el(8))),               # a start side that is neither before nor after
            (eot, af(el(8))),
            (eot, eot),
            (bf(el(10)), sot),              # ... and an end side
            (af(el(3)), bf(el(15))),        # an `after` start, a `before` end
        ]
        step = max(1, K // (2 * len(hand)))
        for h, (st, en) in enumerate(hand * 2):  # every kind twice, on whatever type the op has: once early, once late in the runs
            op = marks[min(K - 1, h * step)]
            op["start"], op["end"] = copy.deepcopy(st), copy.deepcopy(en)
        for j in range(K - 12, K):  # comment ops on several ids
            _retype(marks[j], "comment", j)
        ctr = n + 2 + D + K
        log.append({"actor": "doc1", "seq": len(log) + 1, "deps": {}, "startOp": ctr,
                    "ops": [{"opId": later, "action": "set", "obj": "1@doc1", "elemId": el(11), "insert": True, "value": "z"}]})
    return log


def _logs():
    return [_edit(H.synthetic_marks_log(n, K, 5200 + 11 * i, n_deletes=D, max_span=9), n, D, K, edit) for i, (n, D, K, edit) in enumerate(SHAPES)]


# what the one-wave lean build takes: at most 512 rows and an LDS window of at most 160 KiB / 25 (tests/test_emu_mark_operands.py checks the windows of these)
SHORT = tuple(i for i, (n, D, K, edit) in enumerate(SHAPES) if 2 + n + D + K <= 512 and K <= 200)


@functools.lru_cache(maxsize=None)
def shapes(which=None):
    """-> (Batch of one log per shape, [the oracle's {spans, text} per log], [(n, D, K, edit)])."""
    logs = _logs()
    sel = list(which) if which is not None else list(range(len(SHAPES)))
    logs = [logs[i] for i in sel]
    exp = H.oracle_apply([[l] for l in logs], no_patches=True)
    batch = wire.encode_docs([[l] for l in logs])
    batch.log_hdr = None  # (the library takes the census: the header's bounds come from the op ids alone)
    for l, i in enumerate(sel):
        n, D, K, edit = SHAPES[i]
        assert int(batch.log_off[l + 1] - batch.log_off[l]) == 1 + n + D + K + (1 if edit == "operands" else 0)
        assert not exp[l][0].get("error"), exp[l][0].get("error")
    return batch, [e[0] for e in exp], [SHAPES[i] for i in sel]


def _code(exp):
    err = exp.get("error")
    if not err:
        return 0
    assert "List element not found" in err, err
    return abi.ERR_ELEM_NOT_FOUND


@functools.lru_cache(maxsize=None)
def failing():
    """-> (Batch, [the oracle's answer per log], [the status the oracle's answer stands for]): logs that pass the row pass — their rows are well-formed, their
    headers exact, their ids distinct — and fail later, between good ones: a delete of an element nobody inserted, with mark ops behind it and without."""
    specs = ((24, 3, 70, True), (24, 0, 70, False), (24, 2, 0, True), (30, 4, 129, True), (24, 1, 5, False))
    logs = []
    for i, (n, D, K, bad) in enumerate(specs):
        log = H.synthetic_marks_log(n, K, 6100 + 13 * i, n_deletes=D, max_span=9)
        if bad:
            log[1 + D // 2]["ops"][0]["elemId"] = "9999@doc1"
        logs.append(log)
    exp = [e[0] for e in H.oracle_apply([[l] for l in logs], no_patches=True)]
    batch = wire.encode_docs([[l] for l in logs])
    batch.log_hdr = None
    codes = [_code(e) for e in exp]
    assert [c != 0 for c in codes] == [s[3] for s in specs], codes
    return batch, exp, codes


@functools.lru_cache(maxsize=None)
def bad_comment():
    """-> (Batch with the encoder's headers, bad log, its offending row, [the oracle's answer per log]): three logs with comment ops; the header of the middle
    one declares one comment id less than its ops use, and exactly one op — the last of the log's comment ops with the largest id — is beyond it.  The header is
    the caller's promise (peritext_hip.h: a comment id beyond n_comment_ids is PTX_ERR_BAD_OP, named at its row); the other two logs answer like the oracle."""
    logs = [H.synthetic_marks_log(24, 90, 6400 + i, n_deletes=1, max_span=9) for i in range(3)]
    for l, log in enumerate(logs):
        marks = [c["ops"][0] for c in log[2:]]
        for j, op in enumerate(marks):
            if op["markType"] == "comment":
                op["attrs"] = {"id": "comment-%d" % (j % 3)}
        _retype(marks[77], "comment", 0)
        marks[77]["attrs"] = {"id": "comment-zz%d" % l}  # (a fourth id, used once per log: the doc-local rank of the largest id a log uses is its own)
    exp = [e[0] for e in H.oracle_apply([[l] for l in logs], no_patches=True)]
    batch = wire.encode_docs([[l] for l in logs])
    batch.log_hdr = batch.log_hdr.copy()
    lo, hi = int(batch.log_off[1]), int(batch.log_off[2])
    is_c = (batch.mark_type[lo:hi] == abi.MARK_COMMENT) & ((batch.action[lo:hi] == abi.ACT_ADDMARK) | (batch.action[lo:hi] == abi.ACT_REMOVEMARK))
    top = int(batch.payload[lo:hi][is_c].max())
    rows = [r for r in range(hi - lo) if is_c[r] and int(batch.payload[lo + r]) == top]
    assert len(rows) == 1 and int(batch.log_hdr["n_comment_ids"][1]) == top + 1
    batch.log_hdr["n_comment_ids"][1] = top
    return batch, 1, rows[0], exp
