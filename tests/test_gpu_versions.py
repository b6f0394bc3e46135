"""Resident logs at a past version through the C ABI on a real MI355X (ptx_batch_at_versions -> ptx_merge / ptx_root_map / ptx_replay_patches_from): the
cases of tests/test_emu_versions.py, expected values from tests/version_oracle.js (the oracle's own applyChange over the kept changes, then the rest).  Per
cut: status, n_kept, first_row and clocks_out are the oracle's; the Changes of the cut log deep-equal the oracle's kept list in order; the merge WITH
admission shows the oracle's spans; the root map is the oracle's root at the version; with THEN_REST the patch stream from first_row on is the oracle's patch
list of the rest.  And one small session with the logs resident: change -> sync -> append for a few rounds, then every replica cut at the clock it had
after every round."""
import json
import os
import tempfile

import numpy as np
import pytest

import helpers as H
import sync_cases as SC
import version_cases as VC
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


def cut_tables_of(batch, src):
    """The decode tables of a cut batch: log c belongs to the document of its source."""
    return (batch.values, batch.urls, [batch.log_doc[int(s)] for s in src], batch.doc_actors, batch.doc_comments, batch.keys, batch.map_values)


def gpu_versions(eng, batch, src, clocks=None, prefix=None, then_rest=False, merge=True, db=None):
    """upload, ptx_batch_at_versions, download; merge, root map and replay of the cut batch: (out, status, n_kept, first_row, clocks_out, res, rm, pat)."""
    own = db is None
    if own:
        db = eng.upload(batch)
    h = dr = None
    try:
        h, status, n_kept, first_row, clocks_out = eng.at_versions(db, src, clocks, prefix, then_rest)
        out = eng.download_batch(h, *cut_tables_of(batch, src))
        res = rm = pat = None
        if merge and len(src):
            dr = eng.alloc_result(h)
            eng.merge(h, dr)
            eng.sync()
            res = eng.download(h, dr)
            if then_rest:
                pat = eng.replay_patches(h, dr, first_row=first_row)
            else:
                rm = eng.root_map(h)
        return out, status, n_kept, first_row, clocks_out, res, rm, pat
    finally:
        if dr is not None:
            eng.free_result(dr)
        if h is not None:
            eng.free_batch(h)
        if own:
            eng.free_batch(db)


def run_case(eng, case, then_rest=False):
    batch = SC.encode(case)
    src, clocks, prefix = VC.cut_tables(case, batch)
    out, status, n_kept, first_row, clocks_out, res, rm, pat = gpu_versions(eng, batch, src, clocks, prefix, then_rest)
    VC.check_cuts(case, batch, out, status, n_kept, first_row, clocks_out, then_rest)
    VC.check_merged(case, out, res, status, rm, pat, then_rest)
    return batch, out, status, n_kept, first_row, clocks_out


MODES = [False, True]


@pytest.mark.parametrize("then_rest", MODES)
def test_log_sizes_keep_patterns_and_strides(eng, then_rest):
    case = VC.keep_pattern_case()
    _, out, status, n_kept, _, _ = run_case(eng, case, then_rest)
    assert not status.any()
    for c, name in enumerate(case["names"]):
        kind, n = name.split("/")
        assert int(n_kept[c]) == {"none": 0, "all": int(n), "second": (int(n) + 1) // 2}.get(kind, 1), name
    batch, _, status, n_kept, _, clocks_out = run_case(eng, VC.stride_case(), then_rest)
    assert batch.max_actors == 17 and [int(k) for k in n_kept] == [2] + [3] * (len(VC.STRIDE_ACTORS) - 1)
    for c, n in enumerate(VC.STRIDE_ACTORS):
        assert [int(a) for a in np.nonzero(clocks_out[c])[0]] == sorted({0, n - 1})


@pytest.mark.parametrize("then_rest", MODES)
@pytest.mark.parametrize("prefix", [False, True])
def test_changes_of_no_one_and_several_ops_at_the_step_edge(eng, prefix, then_rest):
    _, _, status, _, first_row, _ = run_case(eng, VC.multi_op_case(prefix), then_rest)
    assert not status.any()
    if prefix:
        assert int(first_row[2]) == int(first_row[3]) and int(first_row[1]) + 1 == int(first_row[2])


@pytest.mark.parametrize("then_rest", MODES)
def test_clocks_no_replica_could_have_had(eng, then_rest):
    case = VC.open_clock_case()
    oracle = VC.oracle_of(case, then_rest)
    assert [o["error"] and (o["error"]["kind"], o["error"]["at"]) for o in oracle] == [("Missing dependency", 0), ("Missing dependency", 62), ("Missing dependency", 69), None, None]
    _, out, status, n_kept, _, _ = run_case(eng, case, then_rest)
    assert [int(s) for s in status] == [abi.ERR_MISSING_DEP] * 3 + [0, 0] and [int(k) for k in n_kept] == [0, 0, 0, 62, 69]
    assert [int(out.chg_off[c + 1] - out.chg_off[c]) for c in range(5)] == [0, 0, 0] + ([138, 138] if then_rest else [62, 69])


def test_history_strip_of_131_prefixes_in_one_call(eng):
    case = VC.history_strip_case()
    _, _, status, n_kept, _, clocks_out = run_case(eng, case)
    assert not status.any() and [int(k) for k in n_kept] == list(range(131)) and [int(x) for x in clocks_out[129]] == [65, 64]
    run_case(eng, case, then_rest=True)


@pytest.mark.parametrize("then_rest", MODES)
@pytest.mark.parametrize("config,replicas", [("mini", None), ("rich", None), ("rich", 4)])
def test_redealt_logs_at_the_clocks_of_the_other_replicas(eng, config, replicas, then_rest):
    _, _, status, _, _, _ = run_case(eng, VC.redealt_case(config, replicas), then_rest)
    assert not status.any()


def test_wide_seqs(eng):
    """Seqs beyond 65 535 (the wide column): the expected keys from a sequential filter over the JSON logs (tests/test_emu_versions.py says why)."""
    case = SC.wide_case_docs()
    batch = SC.encode(case)
    assert batch.chg_env_hi is not None
    src_log = case["docs"][0][0]
    cuts = [{"a": 65545}, {"a": 65555, "b": 2}, {"a": 65536, "b": 0}, {"a": abi.VERSION_ALL, "b": abi.VERSION_ALL}]
    clocks = np.array([[c.get("a", 0), c.get("b", 0)] for c in cuts], dtype=np.uint32)
    out, status, n_kept, first_row, clocks_out, res, _, _ = gpu_versions(eng, batch, [0] * len(cuts), clocks)
    assert not status.any() and out.chg_env_hi is not None
    for c, clock in enumerate(cuts):
        kept = [(x["actor"], x["seq"]) for x in src_log if x["seq"] <= clock.get(x["actor"], 0)]
        c0, c1 = int(out.chg_off[c]), int(out.chg_off[c + 1])
        got = list(zip(["ab"[int(a)] for a in out.chg_actor[c0:c1]], [int(q) for q in out.chg_seq[c0:c1]]))
        assert got == kept and int(n_kept[c]) == len(kept) and int(first_row[c]) == len(kept)
        assert [int(q) for q in clocks_out[c]] == [max([q for a, q in kept if a == x] or [0]) for x in "ab"]
    assert VC.same_log(out, 3, batch, 0)
    assert [int(s) for s in res.logs["status"]] == [0] * 4 and [int(v) for v in res.logs["n_visible"]] == [int(k) - 1 for k in n_kept]


def test_saturation_bad_rank_invariants_and_argument_checks(eng):
    from peritext_amd.engine import PtxError

    case = VC.multi_op_case(False)
    nb = SC.encode(case)
    nb.chg_env[(int(nb.chg_off[1]) + 69) * abi.env_stride(nb.max_actors) + 1] = abi.ENV_SATURATED  # a dropped change's dep
    clocks = np.array([[abi.VERSION_ALL] * 2, [5, 0], [abi.VERSION_ALL] * 2], dtype=np.uint32)
    out, status, n_kept, first_row, clocks_out, _, _, _ = gpu_versions(eng, nb, [0, 1, 2], clocks, merge=False)
    assert [int(s) for s in status] == [0, abi.ERR_CAPACITY, 0] and int(out.chg_off[2] - out.chg_off[1]) == 0 and int(n_kept[1]) == 0 and not clocks_out[1].any()
    assert VC.same_log(out, 0, nb, 0) and VC.same_log(out, 2, nb, 2)
    nb = SC.encode(case)
    nb.chg_hdr[int(nb.chg_off[1]) + 3] |= np.uint32(5 << abi.CHG_ACTOR_SHIFT)  # an actor rank beyond max_actors
    out, status, _, _, _, _, _, _ = gpu_versions(eng, nb, [0, 1], prefix=[70, 2], merge=False)
    assert [int(s) for s in status] == [0, abi.ERR_BAD_OP] and int(out.chg_off[2] - out.chg_off[1]) == 0
    # the invariants that need no oracle
    batch = SC.encode(VC.redealt_case("rich", 4))
    L, na = batch.n_logs, batch.max_actors
    db = eng.upload(batch)
    bare = wire.Batch(batch.log_off, batch.op_id, batch.ref_a, batch.ref_b, batch.payload, batch.action, batch.mark_type, batch.side_a, batch.side_b, None, None, None, 0,
                      None, batch.values, batch.urls, batch.log_doc, batch.doc_actors, batch.doc_comments)
    db_bare = eng.upload(bare)
    try:
        for then_rest in MODES:
            out, status, n_kept, _, _, _, _, _ = gpu_versions(eng, batch, list(range(L)) * 2, np.full((2 * L, na), abi.VERSION_ALL, np.uint32), None, then_rest, merge=False, db=db)
            assert not status.any() and all(VC.same_log(out, c, batch, c % L) for c in range(2 * L))
            out, status, n_kept, first_row, clocks_out, _, _, _ = gpu_versions(eng, batch, list(range(L)), np.zeros((L, na), np.uint32), None, then_rest, merge=False, db=db)
            assert not status.any() and not n_kept.any() and not first_row.any() and not clocks_out.any()
            assert all(VC.same_log(out, c, batch, c) for c in range(L)) if then_rest else int(out.log_off[-1]) == 0 and int(out.chg_off[-1]) == 0
        n = int(batch.chg_off[1] - batch.chg_off[0])
        ks = list(range(n + 2))
        out, status, n_kept, first_row, _, _, _, _ = gpu_versions(eng, batch, [0] * len(ks), None, ks, True, merge=False, db=db)
        assert not status.any() and [int(k) for k in n_kept] == [min(k, n) for k in ks] and all(VC.same_log(out, c, batch, 0) for c in range(len(ks)))
        nops = batch.chg_nops[:n]
        assert [int(r) for r in first_row] == [int(nops[:k].sum()) for k in ks]
        # argument checks
        ck, pf = np.zeros((1, na), np.uint32), np.zeros(1, np.uint32)
        for h, args in ((db, ([L], ck, None)), (db, ([0], ck, pf)), (db, ([0], None, None)), (db_bare, ([0], None, pf))):  # no such log; both; neither; no envelope
            with pytest.raises(PtxError) as ei:
                eng.at_versions(h, *args)
            assert ei.value.status == abi.ERR_INVALID_ARG
        h, status, _, _, _ = eng.at_versions(db, [], prefix=[])
        assert eng.n_ops(h) == 0 and eng.n_logs(h) == 0 and len(status) == 0
        eng.free_batch(h)
    finally:
        eng.free_batch(db)
        eng.free_batch(db_bare)


def session_oracle(script, marks):
    """The oracle playing the session (tests/sync_oracle.js --session gives every round's logs), then cutting every replica's final log at the prefixes
    `marks[k][log]` it had after every round (tests/version_oracle.js): the documents at those versions and the patches from there to the end."""
    with tempfile.TemporaryDirectory() as td:
        inp, out = os.path.join(td, "in.json"), os.path.join(td, "out.json")
        with open(inp, "w") as f:
            json.dump(script, f)
        H.run_node(["tests/sync_oracle.js", "--session", inp, out])
        with open(out) as f:
            return json.load(f)


def test_a_session_cut_at_the_clock_of_every_round(eng):
    """Four 3-replica documents, six rounds of ptx_change + bidirectional sync + append with the logs resident.  After every round a prefix cut over the
    whole of every log records the replica's clock (clocks_out); at the end every replica is cut at each of those clocks, with and without THEN_REST: every
    document and every diff stream against the oracle playing the same script and cutting its own final logs by the definition."""
    script = SC.session_script(rounds=6)
    script["rounds"] = script["rounds"][:6]  # (the three all-pairs rounds behind them are the sync tests' business)
    oracle = session_oracle(script, None)
    D, R = script["docs"], script["replicas"]
    actors = ["doc%d" % (r + 1) for r in range(R)]
    batch = wire.encode_docs([[[oracle["initial"]] for _ in range(R)] for _ in range(D)], extra_actors=[actors] * D)
    cur = eng.upload(batch)
    dr = None
    round_clocks = []
    try:
        for k, steps in enumerate(script["rounds"]):
            dr = eng.alloc_result(cur)
            eng.merge(cur, dr)
            eng.sync()
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
            h, status, n_kept, _, clocks_out = eng.at_versions(cur, list(range(D * R)), prefix=[0xFFFFFFFF] * (D * R))
            eng.free_batch(h)
            assert not status.any()
            assert [int(n) for n in n_kept] == [len(oracle["rounds"][k][d]["logs"][r]) for d in range(D) for r in range(R)]
            round_clocks.append(clocks_out.copy())
        final = eng.download_batch(cur, batch.values, batch.urls, batch.log_doc, batch.doc_actors, batch.doc_comments, batch.keys, batch.map_values)
        final_logs = [wire.decode_changes(final, l) for l in range(D * R)]
        assert [[[c["actor"], c["seq"]] for c in final_logs[d * R + r]] for d in range(D) for r in range(R)] == [oracle["rounds"][-1][d]["logs"][r] for d in range(D) for r in range(R)]
        # every replica at the clock it had after every round: the cuts of one call
        src = [l for k in range(len(round_clocks)) for l in range(D * R)]
        clocks = np.concatenate(round_clocks)
        case = {"docs": [final_logs[d * R:(d + 1) * R] for d in range(D)],
                "cuts": [{"log": l, "clock": {final.doc_actors[final.log_doc[l]][a]: int(q) for a, q in enumerate(round_clocks[k][l]) if q}} for k in range(len(round_clocks)) for l in range(D * R)]}
        text_obj = SC.text_obj_of(case)
        assert text_obj is not None
        for then_rest in MODES:
            out, status, n_kept, first_row, clocks_out, res, rm, pat = gpu_versions(eng, final, src, clocks, None, then_rest, db=cur)
            assert not status.any() and np.array_equal(clocks_out, clocks), "a replica's own past clock is closed, and the cut's effective clock"
            # the version a replica had after round k is the prefix of its log it had applied by then
            assert [int(n) for n in n_kept] == [len(oracle["rounds"][k][l // R]["logs"][l % R]) for k in range(len(round_clocks)) for l in range(D * R)]
            VC.check_cuts(case, final, out, status, n_kept, first_row, clocks_out, then_rest)
            VC.check_merged(case, out, res, status, rm, pat, then_rest)
    finally:
        if dr is not None:
            eng.free_result(dr)
        eng.free_batch(cur)
