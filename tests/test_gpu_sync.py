"""The sync of replica logs through the C ABI on a real MI355X (ptx_sync_replicas -> ptx_batch_append_device -> ptx_merge): the cases of
tests/test_emu_sync.py, expected values from tests/sync_oracle.js (oracle/harness.js's getMissingChanges + applyChanges over the oracle's applyChange).
Per pair: the Changes of `more` deep-equal to the oracle's `applied` in order; the grown target merges WITH admission to the oracle's spans; its patch
stream is the oracle's.  And the reference fuzzer's whole step (test/fuzz.ts:165-199) for a fixed script with the logs resident: change() -> sync ->
append -> merge, every round against the oracle playing the same script, converged at the end."""
import numpy as np
import pytest

import change_script as CS
import helpers as H
import sync_cases as SC
from peritext_amd import abi, wire

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from peritext_amd.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def tables(b):
    return (b.values, b.urls, b.log_doc, b.doc_actors, b.doc_comments, b.keys, b.map_values)


def gpu_sync(eng, batch, pairs, max_attempts=SC.REFERENCE_GUARD, merge=True, patches=True):
    """upload, ptx_sync_replicas, ptx_batch_append_device, merge, replay: (more, status, grown batch, merge result, patch streams)."""
    db = eng.upload(batch)
    more_h = grown_h = dr = None
    try:
        more_h, status = eng.sync_replicas(db, pairs, max_attempts)
        more = eng.download_batch(more_h, *tables(batch))
        if not merge:
            return more, status, None, None, None
        grown_h = eng.append_device(db, more_h)
        dr = eng.alloc_result(grown_h)
        eng.merge(grown_h, dr)
        eng.sync()
        grown = eng.download_batch(grown_h, *tables(batch))
        res = eng.download(grown_h, dr)
        pat = eng.replay_patches(grown_h, dr) if patches else None
        return more, status, grown, res, pat
    finally:
        if dr is not None:
            eng.free_result(dr)
        for h in (grown_h, more_h, db):
            if h is not None:
                eng.free_batch(h)


def run_case(eng, case, max_attempts=SC.REFERENCE_GUARD, merge=True, patches=True):
    batch = SC.encode(case)
    more, status, grown, res, pat = gpu_sync(eng, batch, case["pairs"], max_attempts, merge, patches)
    grown_logs = SC.check_order(case, batch, more, status, max_attempts)
    if merge:
        want = H.concat_batches(batch, more)  # the append itself: log l of the grown batch = log l of the base + log l of `more`
        assert np.array_equal(grown.log_off, want.log_off) and np.array_equal(grown.op_id, want.op_id) and np.array_equal(grown.chg_hdr, want.chg_hdr)
        SC.check_grown(case, grown, grown_logs, res, pat)
    return batch, more, status


@pytest.mark.parametrize("config,replicas,both_ways", [("mini", None, False), ("mini", None, True), ("rich", None, False), ("rich", 4, True)])
def test_redealt_logs(eng, config, replicas, both_ways):
    run_case(eng, SC.redeal_case(config, replicas, both_ways))


def test_chunk_edges_actor_order_and_target_edges(eng):
    case = SC.chunk_edge_case()
    _, more, _ = run_case(eng, case)
    assert [int(more.chg_off[t + 1] - more.chg_off[t]) for _, t in case["pairs"]] == [63, 64, 65, 129, 136, 136, 136]
    case = SC.actor_order_case()
    _, more, _ = run_case(eng, case)
    assert int(more.chg_actor[int(more.chg_off[case["pairs"][6][1]])]) == 16  # first appearance, not rank
    case = SC.target_edge_case()
    _, more, status = run_case(eng, case)
    assert [int(more.chg_off[t + 1] - more.chg_off[t]) for _, t in case["pairs"]] == [5, 0, 0, 3, 1] and not status.any()


def test_the_attempt_guard(eng):
    """T = 9 900 and 10 001 pass, 10 002 and 10 100 are PTX_ERR_SYNC_NOT_CONVERGED at the reference's 10 001; unbounded, the 10 100 case gives the guard-free
    twin loop's order; a change nobody can admit is status 8 at both settings, and the kernel terminates."""
    case = SC.guard_case()
    assert [o["attempts"] for o in case["oracle"][:4]] == [t for _, _, t in SC.GUARD_SHAPES]
    _, _, status = run_case(eng, case)
    assert [int(s) for s in status] == [0, abi.ERR_SYNC_NOT_CONVERGED, 0, abi.ERR_SYNC_NOT_CONVERGED, abi.ERR_SYNC_NOT_CONVERGED]
    _, more, status = run_case(eng, case, max_attempts=0, merge=False)
    assert [int(s) for s in status] == [0, 0, 0, 0, abi.ERR_SYNC_NOT_CONVERGED] and int(more.chg_off[3 + 1] - more.chg_off[3]) == 200


def test_wide_envelope_saturation_and_argument_checks(eng):
    from peritext_amd.engine import PtxError

    case = SC.wide_case()
    batch = SC.encode(case)
    assert batch.chg_env_hi is not None
    more, status, grown, res, _ = gpu_sync(eng, batch, case["pairs"], patches=False)
    keys = list(zip([batch.doc_actors[0][int(x)] for x in more.chg_actor], [int(x) for x in more.chg_seq]))
    assert int(status[0]) == 0 and keys == [tuple(k) for k in case["oracle"][0]["applied"]] and len(keys) == 33 and more.chg_env_hi is not None
    assert wire.decode_changes(more, 1, text_obj="1@a") == [SC.by_key(case["docs"][0][0])[k] for k in keys]
    assert int(res.logs["status"][1]) == 0 and int(res.logs["n_visible"][1]) == 65530 + 33 - 1
    # a narrow envelope with a saturated value: PTX_ERR_CAPACITY for that pair only
    small = SC.target_edge_case()
    nb = SC.encode(small)
    nb.chg_env[int(nb.chg_off[0]) * abi.env_stride(nb.max_actors)] = abi.ENV_SATURATED
    more, status, _, _, _ = gpu_sync(eng, nb, [(0, 1), (5, 6)], merge=False)
    assert [int(s) for s in status] == [abi.ERR_CAPACITY, 0] and int(more.chg_off[2] - more.chg_off[1]) == 0 and int(more.chg_off[-1]) == 1
    # argument checks
    good = SC.encode(small)
    db = eng.upload(good)
    bare = wire.Batch(good.log_off, good.op_id, good.ref_a, good.ref_b, good.payload, good.action, good.mark_type, good.side_a, good.side_b, None, None, None, 0,
                      None, good.values, good.urls, good.log_doc, good.doc_actors, good.doc_comments)
    db_bare = eng.upload(bare)
    try:
        for h, pairs in ((db, [(0, 1), (4, 1)]), (db, [(0, 7)]), (db_bare, [(0, 1)])):  # a target twice; no such log; no envelope
            with pytest.raises(PtxError) as ei:
                eng.sync_replicas(h, pairs)
            assert ei.value.status == abi.ERR_INVALID_ARG
        h, status = eng.sync_replicas(db, [])
        assert eng.n_ops(h) == 0 and eng.n_logs(h) == good.n_logs and len(status) == 0
        eng.free_batch(h)
    finally:
        eng.free_batch(db)
        eng.free_batch(db_bare)


def test_twelve_round_session_stays_on_the_device(eng):
    """Four 3-replica documents, 12 rounds: ptx_change on one replica per document, a random bidirectional sync, append, merge — the logs never leave the
    device except to be checked: every round's logs against the oracle playing the same script; after the all-pairs sync ptx_count_converged = 4."""
    import torch

    script, oracle = SC.session_oracle()
    D, R = script["docs"], script["replicas"]
    actors = ["doc%d" % (r + 1) for r in range(R)]
    first = oracle["initial"]
    batch = wire.encode_docs([[[first] for _ in range(R)] for _ in range(D)], extra_actors=[actors] * D)
    cur = eng.upload(batch)
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    dr = None
    try:
        for k, steps in enumerate(script["rounds"]):
            dr = eng.alloc_result(cur)
            eng.merge(cur, dr)
            eng.sync()
            if steps[0]["edit"] is not None:
                calls = [[] for _ in range(D * R)]
                for d, st in enumerate(steps):
                    calls[d * R + st["edit"]["replica"]] = [st["edit"]["ops"]]
                made_h, status = eng.change(cur, dr, wire.encode_input_ops(batch, calls, actors * D))
                assert not status.any()
                nxt = eng.append_device(cur, made_h)
                eng.free_batch(made_h)
                eng.free_batch(cur)
                cur = nxt
            eng.free_result(dr)
            dr = None
            pairs = []
            for d, st in enumerate(steps):
                l, r = st["sync"]
                pairs += [(d * R + l, d * R + r), (d * R + r, d * R + l)]
            more_h, status = eng.sync_replicas(cur, pairs)
            assert not status.any()
            nxt = eng.append_device(cur, more_h)
            eng.free_batch(more_h)
            eng.free_batch(cur)
            cur = nxt
            got = eng.download_batch(cur, *tables(batch))
            for d in range(D):
                for r in range(R):
                    log = wire.decode_changes(got, d * R + r)
                    assert [[c["actor"], c["seq"]] for c in log] == oracle["rounds"][k][d]["logs"][r], "round %d document %d replica %d" % (k, d, r)
                    made = oracle["rounds"][k][d]["made"]
                    if made is not None and r == steps[d]["edit"]["replica"]:
                        assert CS.norm_change(made) in [CS.norm_change(c) for c in log]
        dr = eng.alloc_result(cur)
        eng.merge(cur, dr)
        eng.count_converged(dr, R, count.data_ptr())
        eng.sync()
        res = eng.download(cur, dr)
        assert (res.logs["status"] == 0).all() and int(count.item()) == D
        final = eng.download_batch(cur, *tables(batch))
        exp = H.oracle_apply([[wire.decode_changes(final, d * R + r) for r in range(R)] for d in range(D)])
        for d in range(D):
            for r in range(R):
                H.check_log(final, res, d * R + r, exp[d][r])
    finally:
        if dr is not None:
            eng.free_result(dr)
        eng.free_batch(cur)
