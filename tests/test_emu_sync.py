"""The sync of replica logs (peritext_amd/csrc/sync_core.h: getMissingChanges + applyChanges of reference/test/merge.ts:4-38 for many replica pairs) on
the CPU emulation, in every lane order.  Expected values never come from the code under test: tests/sync_oracle.js runs oracle/harness.js's
getMissingChanges / applyChanges and a guard-free twin of that loop over the oracle's own applyChange.  Per pair: (1) the Changes of `more` are deep-equal
to the oracle's `applied`, in order; (2) after the append, the merge WITH admission says OK and shows the oracle's spans for target ++ applied; (3) the
grown log's patch stream is the oracle's.  tests/test_gpu_sync.py repeats the cases through the C ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import sync_cases as SC
from peritext_amd import abi, wire

EMU_SYNC_LIB = os.path.join(H.ROOT, "tests", "emu", "libperitext_emu_sync.so")
pytestmark = [pytest.mark.skipif(not os.path.exists(EMU_SYNC_LIB), reason="tests/emu/libperitext_emu_sync.so not built (run __graft_entry__.build())"),
              pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")]


def emu_sync(batch, pairs, max_attempts=SC.REFERENCE_GUARD, reverse=0):
    """ptx_sync_replicas over a wire.Batch through the host emulation: (return code, `more` as a wire.Batch, status per pair)."""
    lib = C.CDLL(EMU_SYNC_LIB)
    lib.ptx_emu_sync.restype = C.c_int
    src = np.ascontiguousarray([s for s, _ in pairs], dtype=np.uint32)
    dst = np.ascontiguousarray([t for _, t in pairs], dtype=np.uint32)
    P, L = len(pairs), batch.n_logs
    in_range = [s for s in src if s < L]
    rows = int(sum(int(batch.log_off[s + 1] - batch.log_off[s]) for s in in_range)) + 1
    chgs = int(sum(int(batch.chg_off[s + 1] - batch.chg_off[s]) for s in in_range)) + 1 if batch.chg_off is not None else 1
    es = abi.env_stride(max(batch.max_actors, 1))
    cols = {"op_id": np.zeros(rows, np.uint64), "ref_a": np.zeros(rows, np.uint64), "ref_b": np.zeros(rows, np.uint64), "payload": np.zeros(rows, np.uint32),
            "action": np.zeros(rows, np.uint8), "mark_type": np.zeros(rows, np.uint8), "side_a": np.zeros(rows, np.uint8), "side_b": np.zeros(rows, np.uint8),
            "chg_hdr": np.zeros(chgs, np.uint32), "chg_env": np.zeros(chgs * es, np.uint16), "chg_env_hi": np.zeros(chgs * es, np.uint16)}
    status, n_adm, n_rows = (np.full(max(P, 1), 0xA5A5A5A5, np.uint32) for _ in range(3))
    log_off, chg_off = np.zeros(L + 1, np.uint64), np.zeros(L + 1, np.uint64)
    s = H.batch_struct(batch)
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    rc = lib.ptx_emu_sync(C.byref(s), C.c_uint32(P), vp(src), vp(dst), C.c_uint32(max_attempts), C.c_int(reverse), vp(status), vp(n_adm), vp(n_rows), vp(log_off), vp(chg_off),
                          vp(cols["op_id"]), vp(cols["ref_a"]), vp(cols["ref_b"]), vp(cols["payload"]), vp(cols["action"]), vp(cols["mark_type"]), vp(cols["side_a"]),
                          vp(cols["side_b"]), vp(cols["chg_hdr"]), vp(cols["chg_env"]), vp(cols["chg_env_hi"]))
    if rc != 0:
        return rc, None, None
    return 0, SC.more_from_columns(batch, cols, log_off, chg_off), status[:P]


def run_case(case, reverse, max_attempts=SC.REFERENCE_GUARD, grown=True, big=False, patches=True):
    batch = SC.encode(case)
    rc, more, status = emu_sync(batch, case["pairs"], max_attempts, reverse)
    assert rc == 0
    grown_logs = SC.check_order(case, batch, more, status, max_attempts)
    if grown:
        gb = H.concat_batches(batch, more)
        res = H.emu_merge_big(gb, reverse=reverse, admission=True) if big else H.emu_merge(gb, reverse=reverse, admission=True)
        SC.check_grown(case, gb, grown_logs, res, H.emu_replay(gb, res, reverse=reverse) if patches else None)
    return batch, more, status


REVERSE = [0, 1, 2]


@pytest.mark.parametrize("reverse", REVERSE)
@pytest.mark.parametrize("config,replicas", [("mini", None), ("rich", None), ("rich", 4)])
def test_redealt_logs_every_ordered_pair_in_one_call(config, replicas, reverse):
    run_case(SC.redeal_case(config, replicas), reverse)


@pytest.mark.parametrize("reverse", REVERSE)
@pytest.mark.parametrize("config,replicas", [("mini", None), ("rich", None), ("rich", 4)])
def test_redealt_logs_bidirectional_pairs_in_one_call(config, replicas, reverse):
    """(l, r) and (r, l) of one call both read the base as it is: what r receives from l is never missing for l (test/fuzz.ts:198-199)."""
    run_case(SC.redeal_case(config, replicas, both_ways=True), reverse)


@pytest.mark.parametrize("reverse", REVERSE)
def test_chunk_edges_of_a_run(reverse):
    case = SC.chunk_edge_case()
    _, more, _ = run_case(case, reverse)
    assert [int(more.chg_off[t + 1] - more.chg_off[t]) for _, t in case["pairs"]] == [63, 64, 65, 129, 136, 136, 136]
    assert [o["attempts"] for o in case["oracle"]] == [63, 64, 65, 129, 136 + 135, 136 + 135 - 63, 136 + 135 - 64]  # the failing change costs one more pass over what is behind it


@pytest.mark.parametrize("reverse", REVERSE)
def test_actor_order_and_envelope_strides(reverse):
    case = SC.actor_order_case()
    batch, more, _ = run_case(case, reverse)
    assert sorted({abi.env_stride(len(a)) for a in batch.doc_actors}) == [4, 8, 12, 16, 20]
    # the missing bag follows first appearance, not rank: the first admitted change of the 17-actor document is the highest rank's
    t = case["pairs"][6][1]
    assert int(more.chg_actor[int(more.chg_off[t])]) == 16


@pytest.mark.parametrize("reverse", REVERSE)
def test_target_edge_cases(reverse):
    case = SC.target_edge_case()
    _, more, status = run_case(case, reverse)
    assert [int(more.chg_off[t + 1] - more.chg_off[t]) for _, t in case["pairs"]] == [5, 0, 0, 3, 1] and not status.any()


@pytest.mark.parametrize("reverse", REVERSE)
def test_the_attempt_guard(reverse):
    """reference/test/merge.ts:18 throws once the 10 002nd attempt has been made, also when it emptied the queue: T = 9 900 and 10 001 pass, 10 002 and 10 100
    are PTX_ERR_SYNC_NOT_CONVERGED; a change nobody can admit is the same status at any max_attempts."""
    case = SC.guard_case()
    assert [o["attempts"] for o in case["oracle"][:4]] == [t for _, _, t in SC.GUARD_SHAPES]
    assert [o["threw"] for o in case["oracle"]] == [False, True, False, True, True] and case["oracle"][4]["stuck"]
    assert len(case["oracle"][3]["applied"]) == 300  # the guard fires although that attempt emptied the queue
    _, _, status = run_case(case, reverse, grown=(reverse == 0))
    assert [int(s) for s in status] == [0, abi.ERR_SYNC_NOT_CONVERGED, 0, abi.ERR_SYNC_NOT_CONVERGED, abi.ERR_SYNC_NOT_CONVERGED]
    _, more, status = run_case(case, reverse, max_attempts=0, grown=False)  # unbounded: the guard-free twin loop's order
    assert [int(s) for s in status] == [0, 0, 0, 0, abi.ERR_SYNC_NOT_CONVERGED]
    assert int(more.chg_off[3 + 1] - more.chg_off[3]) == 200
    for bound, want in ((10099, abi.ERR_SYNC_NOT_CONVERGED), (10100, 0)):  # clipped exactly where the guard would fire
        rc, _, status = emu_sync(SC.encode(case), case["pairs"][1:2], bound, reverse)
        assert rc == 0 and int(status[0]) == want


def test_wide_envelope_and_saturated_narrow_value():
    case = SC.wide_case()
    batch = SC.encode(case)
    assert batch.chg_env_hi is not None and int(batch.chg_seq.max()) == 65560
    rc, more, status = emu_sync(batch, case["pairs"])
    assert rc == 0 and more.chg_env_hi is not None
    # (comparison 1 on keys and envelopes: decoding 65 000 changes twice would dominate the test)
    keys = list(zip([batch.doc_actors[0][int(x)] for x in more.chg_actor], [int(x) for x in more.chg_seq]))
    assert int(status[0]) == 0 and keys == [tuple(k) for k in case["oracle"][0]["applied"]] and len(keys) == 33
    assert int(more.chg_seq.max()) == 65560 and wire.decode_changes(more, 1, text_obj="1@a") == [SC.by_key(case["docs"][0][0])[k] for k in keys]
    gb = H.concat_batches(batch, more)
    res = H.emu_merge_big(gb, admission=True)
    assert int(res.logs["status"][1]) == 0 and int(res.logs["n_visible"][1]) == 65530 + 33 - 1
    # a narrow envelope with a saturated value in either log: PTX_ERR_CAPACITY for that pair only
    small = SC.target_edge_case()
    for log, word in ((0, 0), (1, 1)):  # the source's first seq; a dep of the chained target
        nb = SC.encode(small)
        pairs = [(0, 1), (5, 6)] if log == 0 else [(4, 5), (0, 1)]
        victim = pairs[0][log]
        nb.chg_env[int(nb.chg_off[victim]) * abi.env_stride(nb.max_actors) + word] = abi.ENV_SATURATED
        rc, more, status = emu_sync(nb, pairs)
        assert rc == 0 and [int(s) for s in status] == [abi.ERR_CAPACITY, 0]
        assert int(more.chg_off[pairs[0][1] + 1] - more.chg_off[pairs[0][1]]) == 0 and int(more.chg_off[-1]) > 0


def test_argument_checks():
    case = SC.target_edge_case()
    batch = SC.encode(case)
    assert emu_sync(batch, [(0, 1), (4, 1)])[0] == abi.ERR_INVALID_ARG  # a log that is a target twice
    assert emu_sync(batch, [(0, 7)])[0] == abi.ERR_INVALID_ARG and emu_sync(batch, [(9, 1)])[0] == abi.ERR_INVALID_ARG
    bare = wire.Batch(batch.log_off, batch.op_id, batch.ref_a, batch.ref_b, batch.payload, batch.action, batch.mark_type, batch.side_a, batch.side_b, None, None, None, 0,
                      None, batch.values, batch.urls, batch.log_doc, batch.doc_actors, batch.doc_comments)
    assert emu_sync(bare, [(0, 1)])[0] == abi.ERR_INVALID_ARG  # a batch without the envelope
    rc, more, status = emu_sync(batch, [])
    assert rc == 0 and int(more.log_off[-1]) == 0 and len(status) == 0


def test_sanitizer_program(tmp_path):
    """tests/emu/emu_sync_main.cc: plan + gather over chunk-edge and ping-pong envelopes it builds itself, against a sequential queue inside the file, compiled
    with -fsanitize=address,undefined and run as a child process (the LDS block and the scratch slices are exactly as large as the host library makes them)."""
    exe = str(tmp_path / "emu_sync_main")
    src = os.path.join(H.ROOT, "tests", "emu", "emu_sync_main.cc")
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "sync emulation ok" in r.stdout


def test_twelve_round_session_against_the_oracle_playing_the_same_script():
    """The reference fuzzer's step (test/fuzz.ts:165-199) for a fixed script, every piece from the emulation: change() on one replica per document, a
    bidirectional sync as the pairs (l, r), (r, l) of one call, append; every round's logs are the oracle's, and all replicas end on the same digest
    (tests/test_gpu_sync.py plays the same script with the logs resident)."""
    import change_script as CS

    script, oracle = SC.session_oracle()
    D, R = script["docs"], script["replicas"]
    actors = ["doc%d" % (r + 1) for r in range(R)]
    batch = wire.encode_docs([[[oracle["initial"]] for _ in range(R)] for _ in range(D)], extra_actors=[actors] * D)
    for k, steps in enumerate(script["rounds"]):
        if steps[0]["edit"] is not None:
            calls = [[] for _ in range(D * R)]
            for d, st in enumerate(steps):
                calls[d * R + st["edit"]["replica"]] = [st["edit"]["ops"]]
            made, status = H.emu_change(batch, H.emu_merge(batch, admission=True), wire.encode_input_ops(batch, calls, actors * D))
            assert not status.any()
            batch = H.concat_batches(batch, made)
        pairs = []
        for d, st in enumerate(steps):
            l, r = st["sync"]
            pairs += [(d * R + l, d * R + r), (d * R + r, d * R + l)]
        rc, more, status = emu_sync(batch, pairs, reverse=k % 3)
        assert rc == 0 and not status.any()
        batch = H.concat_batches(batch, more)
        for d in range(D):
            for r in range(R):
                log = wire.decode_changes(batch, d * R + r)
                assert [[c["actor"], c["seq"]] for c in log] == oracle["rounds"][k][d]["logs"][r], "round %d document %d replica %d" % (k, d, r)
                made_by_oracle = oracle["rounds"][k][d]["made"]
                if made_by_oracle is not None and r == steps[d]["edit"]["replica"]:
                    assert CS.norm_change(made_by_oracle) in [CS.norm_change(c) for c in log]
    res = H.emu_merge(batch, admission=True)
    assert (res.logs["status"] == 0).all()
    for d in range(D):
        assert len({(int(res.logs["digest"][d * R + r][0]), int(res.logs["digest"][d * R + r][1])) for r in range(R)}) == 1, "document %d has not converged" % d
