"""Resident logs at a past version (peritext_amd/csrc/version_core.h: clock cuts and prefix cuts, optionally the rest behind the kept changes) on the CPU
emulation, in every lane order.  Expected values never come from the code under test: tests/version_oracle.js chooses the kept changes from the definition
and applies them to a fresh document with the oracle's own applyChange.  Per cut: (1) status, n_kept, first_row and clocks_out are the oracle's; (2) the
Changes decoded from the cut log deep-equal the oracle's kept list, in order; (3) the merge WITH admission says OK and shows the oracle's spans; (4) the root
map of the cut batch is the oracle's root at that version; (5) with THEN_REST the merged spans are the source's present spans and the patch stream from
first_row on is the oracle's patch list of the rest.  tests/test_gpu_versions.py repeats the cases through the C ABI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
import sync_cases as SC
import version_cases as VC
from peritext_amd import abi, wire

EMU_VERSIONS_LIB = os.path.join(H.ROOT, "tests", "emu", "libperitext_emu_versions.so")
needs_emu = [pytest.mark.skipif(not os.path.exists(EMU_VERSIONS_LIB), reason="tests/emu/libperitext_emu_versions.so not built (run __graft_entry__.build())"),
             pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")]


def emu(fn):
    for m in needs_emu:
        fn = m(fn)
    return fn


def test_the_entry_point_is_declared():
    """The symbol stands in the C header, with its constants, and in the ctypes prototypes (no skip: this one does not need the emulation library)."""
    with open(os.path.join(H.ROOT, "include", "peritext_hip.h")) as f:
        header = f.read()
    assert re.search(r"ptx_status\s+ptx_batch_at_versions\s*\(", header)
    assert re.search(r"#define\s+PTX_VERSION_ALL\s+0xFFFFFFFFu", header) and re.search(r"#define\s+PTX_VERSIONS_THEN_REST\s+1u", header)
    assert re.search(r"#define\s+PTX_ABI_VERSION\s+7u", header), "the addition is purely additive"
    assert "ptx_batch_at_versions" in abi.FUNCTIONS and len(abi.FUNCTIONS["ptx_batch_at_versions"][1]) == 12
    assert abi.VERSION_ALL == 0xFFFFFFFF and abi.VERSIONS_THEN_REST == 1


def emu_versions(batch, src, clocks=None, prefix=None, then_rest=False, reverse=0, flags=None):
    """ptx_batch_at_versions over a wire.Batch through the host emulation: (return code, the cut batch, status, n_kept, first_row, clocks_out)."""
    lib = C.CDLL(EMU_VERSIONS_LIB)
    lib.ptx_emu_versions.restype = C.c_int
    src = np.ascontiguousarray(src, dtype=np.uint32)
    P, L, na = len(src), batch.n_logs, max(batch.max_actors, 1)
    in_range = [s for s in src if s < L]
    rows = int(sum(int(batch.log_off[s + 1] - batch.log_off[s]) for s in in_range)) + 1
    chgs = int(sum(int(batch.chg_off[s + 1] - batch.chg_off[s]) for s in in_range)) + 1 if batch.chg_off is not None else 1
    es = abi.env_stride(na)
    cols = {"op_id": np.zeros(rows, np.uint64), "ref_a": np.zeros(rows, np.uint64), "ref_b": np.zeros(rows, np.uint64), "payload": np.zeros(rows, np.uint32),
            "action": np.zeros(rows, np.uint8), "mark_type": np.zeros(rows, np.uint8), "side_a": np.zeros(rows, np.uint8), "side_b": np.zeros(rows, np.uint8),
            "chg_hdr": np.zeros(chgs, np.uint32), "chg_env": np.zeros(chgs * es, np.uint16), "chg_env_hi": np.zeros(chgs * es, np.uint16)}
    status, n_kept, first_row = (np.full(max(P, 1), 0xA5A5A5A5, np.uint32) for _ in range(3))
    clocks_out = np.full(max(P * na, 1), 0xA5A5A5A5, np.uint32)
    log_off, chg_off = np.zeros(P + 1, np.uint64), np.zeros(P + 1, np.uint64)
    ck = None if clocks is None else np.ascontiguousarray(clocks, dtype=np.uint32)
    pf = None if prefix is None else np.ascontiguousarray(prefix, dtype=np.uint32)
    s = H.batch_struct(batch)
    vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)  # noqa: E731
    rc = lib.ptx_emu_versions(C.byref(s), C.c_uint32(P), vp(src), vp(ck), vp(pf), C.c_uint32((abi.VERSIONS_THEN_REST if then_rest else 0) if flags is None else flags),
                              C.c_int(reverse), vp(status), vp(n_kept), vp(first_row), vp(clocks_out), vp(log_off), vp(chg_off), vp(cols["op_id"]), vp(cols["ref_a"]),
                              vp(cols["ref_b"]), vp(cols["payload"]), vp(cols["action"]), vp(cols["mark_type"]), vp(cols["side_a"]), vp(cols["side_b"]), vp(cols["chg_hdr"]),
                              vp(cols["chg_env"]), vp(cols["chg_env_hi"]))
    if rc != 0:
        return rc, None, None, None, None, None
    return 0, VC.cut_batch(batch, src, cols, log_off, chg_off), status[:P], n_kept[:P], first_row[:P], clocks_out[:P * na].reshape(P, na)


def run_case(case, reverse, then_rest=False, big=False, merge=True):
    batch = SC.encode(case)
    src, clocks, prefix = VC.cut_tables(case, batch)
    rc, out, status, n_kept, first_row, clocks_out = emu_versions(batch, src, clocks, prefix, then_rest, reverse)
    assert rc == 0
    VC.check_cuts(case, batch, out, status, n_kept, first_row, clocks_out, then_rest)
    if merge:
        res = H.emu_merge_big(out, reverse=reverse, admission=True) if big else H.emu_merge(out, reverse=reverse, admission=True)
        rm = None if then_rest else H.emu_root_map(out, reverse=reverse)
        pat = H.emu_replay(out, res, reverse=reverse, first_row=first_row) if then_rest else None
        VC.check_merged(case, out, res, status, rm, pat, then_rest)
    return batch, out, status, n_kept, first_row, clocks_out


REVERSE = [0, 1, 2]
MODES = [False, True]


@emu
@pytest.mark.parametrize("then_rest", MODES)
@pytest.mark.parametrize("reverse", REVERSE)
def test_log_sizes_and_keep_patterns(reverse, then_rest):
    case = VC.keep_pattern_case()
    _, out, status, n_kept, _, _ = run_case(case, reverse, then_rest)
    assert not status.any()
    want = {"none": lambda n: 0, "all": lambda n: n, "second": lambda n: (n + 1) // 2, "lane0": lambda n: 1, "lane63": lambda n: 1, "lane64": lambda n: 1}
    for c, name in enumerate(case["names"]):
        kind, n = name.split("/")
        assert int(n_kept[c]) == want[kind](int(n)), name
        assert int(out.chg_off[c + 1] - out.chg_off[c]) == (int(n) if then_rest else int(n_kept[c])), name
    # where the lone kept change stands in its source: lane 0, lane 63, the first lane of the second step
    logs = SC.flat_logs(case)
    for name, lane in (("lane0/136", 0), ("lane63/64", 63), ("lane63/136", 63), ("lane64/65", 64), ("lane64/129", 64)):
        assert logs[case["cuts"][case["names"].index(name)]["log"]][lane]["actor"] == "a"


@emu
@pytest.mark.parametrize("then_rest", MODES)
@pytest.mark.parametrize("prefix", [False, True])
@pytest.mark.parametrize("reverse", REVERSE)
def test_changes_of_no_one_and_several_ops_at_the_step_edge(reverse, prefix, then_rest):
    case = VC.multi_op_case(prefix)
    batch, out, status, _, first_row, _ = run_case(case, reverse, then_rest)
    assert not status.any()
    assert [int(batch.chg_nops[int(batch.chg_off[0]) + k]) for k in (62, 63, 64, 65)] == [4, 1, 0, 3]
    assert [int(batch.chg_nops[int(batch.chg_off[1]) + k]) for k in (62, 63, 64, 65)] == [1, 0, 3, 2]
    if prefix:  # a change without ops shares its successor's first row: the prefixes 64 and 65 of the first log hold the same rows
        assert int(first_row[2]) == int(first_row[3]) and int(first_row[1]) + 1 == int(first_row[2])


@emu
@pytest.mark.parametrize("then_rest", MODES)
@pytest.mark.parametrize("reverse", REVERSE)
def test_envelope_strides(reverse, then_rest):
    case = VC.stride_case()
    batch, out, status, n_kept, _, clocks_out = run_case(case, reverse, then_rest)
    assert sorted({abi.env_stride(len(a)) for a in batch.doc_actors}) == [4, 8, 12, 16, 20] and batch.max_actors == 17
    assert [int(k) for k in n_kept] == [2] + [3] * (len(VC.STRIDE_ACTORS) - 1)
    for c, n in enumerate(VC.STRIDE_ACTORS):
        assert [int(a) for a in np.nonzero(clocks_out[c])[0]] == sorted({0, n - 1})


@emu
@pytest.mark.parametrize("then_rest", MODES)
@pytest.mark.parametrize("reverse", REVERSE)
def test_clocks_no_replica_could_have_had(reverse, then_rest):
    """The missing dep at lane 0, at lane 63 and in the second step: PTX_ERR_MISSING_DEP and an empty log, where the oracle's applyChange throws "Missing
    dependency" at exactly that change of the kept list; the closed cuts of the same call are untouched."""
    case = VC.open_clock_case()
    oracle = VC.oracle_of(case, then_rest)
    assert [o["error"] and (o["error"]["kind"], o["error"]["at"]) for o in oracle] == [("Missing dependency", 0), ("Missing dependency", 62), ("Missing dependency", 69), None, None]
    logs = SC.flat_logs(case)
    assert [[i for i, c in enumerate(log) if c["deps"]] for log in logs] == [[0], [63], [70]]  # where the waiting change stands in its source
    _, out, status, n_kept, _, _ = run_case(case, reverse, then_rest)
    assert [int(s) for s in status] == [abi.ERR_MISSING_DEP] * 3 + [0, 0] and [int(k) for k in n_kept] == [0, 0, 0, 62, 69]
    assert [int(out.chg_off[c + 1] - out.chg_off[c]) for c in range(5)] == [0, 0, 0] + ([138, 138] if then_rest else [62, 69])


@emu
@pytest.mark.parametrize("reverse", REVERSE)
def test_history_strip_of_131_prefixes_in_one_call(reverse):
    case = VC.history_strip_case()
    _, out, status, n_kept, _, clocks_out = run_case(case, reverse)
    assert not status.any() and [int(k) for k in n_kept] == list(range(131))
    assert [int(x) for x in clocks_out[129]] == [65, 64] and [int(x) for x in clocks_out[0]] == [0, 0]
    run_case(case, reverse, then_rest=True)


@emu
@pytest.mark.parametrize("then_rest", MODES)
@pytest.mark.parametrize("reverse", REVERSE)
@pytest.mark.parametrize("config,replicas", [("mini", None), ("rich", None), ("rich", 4)])
def test_redealt_logs_at_the_clocks_of_the_other_replicas(config, replicas, reverse, then_rest):
    _, _, status, _, _, _ = run_case(VC.redealt_case(config, replicas), reverse, then_rest)
    assert not status.any()


@pytest.fixture(scope="module")
def wide():
    case = SC.wide_case_docs()
    return case, SC.encode(case)


@emu
@pytest.mark.parametrize("reverse", REVERSE)
def test_wide_seqs(wide, reverse):
    """Seqs beyond 65 535 (the wide column).  The expected keys come from a sequential filter over the JSON logs here (applying 65 000 changes one by one in
    the oracle would dominate the suite); the merged cut shows as many characters as the kept changes insert."""
    case, batch = wide
    assert batch.chg_env_hi is not None
    src_log = case["docs"][0][0]
    cuts = [{"a": 65545}, {"a": 65555, "b": 2}, {"a": 65536, "b": 0}, {"a": abi.VERSION_ALL, "b": abi.VERSION_ALL}]
    clocks = np.array([[c.get("a", 0), c.get("b", 0)] for c in cuts], dtype=np.uint32)
    rc, out, status, n_kept, first_row, clocks_out = emu_versions(batch, [0] * len(cuts), clocks, reverse=reverse)
    assert rc == 0 and not status.any() and out.chg_env_hi is not None
    for c, clock in enumerate(cuts):
        kept = [(x["actor"], x["seq"]) for x in src_log if x["seq"] <= clock.get(x["actor"], 0)]
        c0, c1 = int(out.chg_off[c]), int(out.chg_off[c + 1])
        got = list(zip(["ab"[int(a)] for a in out.chg_actor[c0:c1]], [int(q) for q in out.chg_seq[c0:c1]]))
        assert got == kept and int(n_kept[c]) == len(kept) and int(first_row[c]) == len(kept)
        assert [int(q) for q in clocks_out[c]] == [max([q for a, q in kept if a == x] or [0]) for x in "ab"]
    assert VC.same_log(out, 3, batch, 0)
    if reverse == 0:
        res = H.emu_merge_big(out, admission=True)
        assert [int(s) for s in res.logs["status"]] == [0] * 4 and [int(v) for v in res.logs["n_visible"]] == [int(k) - 1 for k in n_kept]


@emu
@pytest.mark.parametrize("reverse", REVERSE)
def test_saturated_narrow_value(reverse):
    """A narrow envelope with a saturated value anywhere in the source log — a kept change's seq, a dropped change's dep — is that cut's PTX_ERR_CAPACITY;
    the other cuts of the call are untouched."""
    case = VC.multi_op_case(False)
    for chg, word in ((0, 0), (69, 1)):
        nb = SC.encode(case)
        nb.chg_env[(int(nb.chg_off[1]) + chg) * abi.env_stride(nb.max_actors) + word] = abi.ENV_SATURATED
        clocks = np.array([[abi.VERSION_ALL] * 2, [5, 0], [abi.VERSION_ALL] * 2], dtype=np.uint32)
        rc, out, status, n_kept, first_row, clocks_out = emu_versions(nb, [0, 1, 2], clocks, reverse=reverse)
        assert rc == 0 and [int(s) for s in status] == [0, abi.ERR_CAPACITY, 0]
        assert int(out.chg_off[2] - out.chg_off[1]) == 0 and int(n_kept[1]) == 0 and int(first_row[1]) == 0 and not clocks_out[1].any()
        assert VC.same_log(out, 0, nb, 0) and VC.same_log(out, 2, nb, 2)
    nb = SC.encode(case)
    nb.chg_hdr[int(nb.chg_off[1]) + 3] |= np.uint32(5 << abi.CHG_ACTOR_SHIFT)  # an actor rank beyond max_actors
    rc, out, status, _, _, _ = emu_versions(nb, [0, 1], prefix=[70, 2], reverse=reverse)
    assert rc == 0 and [int(s) for s in status] == [0, abi.ERR_BAD_OP] and int(out.chg_off[2] - out.chg_off[1]) == 0


@emu
@pytest.mark.parametrize("reverse", REVERSE)
def test_invariants_that_need_no_oracle(reverse):
    """An all-PTX_VERSION_ALL clock reproduces the source log's columns and envelope byte for byte; so does a prefix cut with THEN_REST, for every k; a
    clock of zeros is an empty log with status OK.  A log is the source of many cuts of one call."""
    for case in (VC.multi_op_case(False), VC.redealt_case("rich", 4), VC.stride_case()):
        batch = SC.encode(case)
        L, na = batch.n_logs, batch.max_actors
        for then_rest in MODES:
            rc, out, status, n_kept, _, _ = emu_versions(batch, list(range(L)) * 2, np.full((2 * L, na), abi.VERSION_ALL, np.uint32), then_rest=then_rest, reverse=reverse)
            assert rc == 0 and not status.any()
            assert all(VC.same_log(out, c, batch, c % L) for c in range(2 * L))
            assert [int(k) for k in n_kept] == [int(batch.chg_off[l + 1] - batch.chg_off[l]) for l in range(L)] * 2
            rc, out, status, n_kept, first_row, clocks_out = emu_versions(batch, list(range(L)), np.zeros((L, na), np.uint32), then_rest=then_rest, reverse=reverse)
            assert rc == 0 and not status.any() and not n_kept.any() and not first_row.any() and not clocks_out.any()
            if then_rest:
                assert all(VC.same_log(out, c, batch, c) for c in range(L))
            else:
                assert int(out.log_off[-1]) == 0 and int(out.chg_off[-1]) == 0
    batch = SC.encode(VC.multi_op_case(True))
    n = int(batch.chg_off[3] - batch.chg_off[2])
    ks = list(range(n + 2))
    rc, out, status, n_kept, first_row, _ = emu_versions(batch, [2] * len(ks), prefix=ks, then_rest=True, reverse=reverse)
    assert rc == 0 and not status.any() and [int(k) for k in n_kept] == [min(k, n) for k in ks]
    assert all(VC.same_log(out, c, batch, 2) for c in range(len(ks)))
    nops = batch.chg_nops[int(batch.chg_off[2]):int(batch.chg_off[3])]
    assert [int(r) for r in first_row] == [int(nops[:k].sum()) for k in ks]


@emu
def test_argument_checks():
    case = VC.multi_op_case(False)
    batch = SC.encode(case)
    ck, pf = np.zeros((1, batch.max_actors), np.uint32), np.zeros(1, np.uint32)
    assert emu_versions(batch, [3], ck)[0] == abi.ERR_INVALID_ARG  # no such log
    assert emu_versions(batch, [0], ck, pf)[0] == abi.ERR_INVALID_ARG and emu_versions(batch, [0])[0] == abi.ERR_INVALID_ARG  # both, neither
    assert emu_versions(batch, [0], ck, flags=2)[0] == abi.ERR_INVALID_ARG
    bare = wire.Batch(batch.log_off, batch.op_id, batch.ref_a, batch.ref_b, batch.payload, batch.action, batch.mark_type, batch.side_a, batch.side_b, None, None, None, 0,
                      None, batch.values, batch.urls, batch.log_doc, batch.doc_actors, batch.doc_comments)
    assert emu_versions(bare, [0], prefix=pf)[0] == abi.ERR_INVALID_ARG  # a batch without the envelope
    rc, out, status, _, _, _ = emu_versions(batch, [])
    assert rc == 0 and out.n_logs == 0 and int(out.log_off[-1]) == 0 and len(status) == 0


@emu
def test_sanitizer_program(tmp_path):
    """tests/emu/emu_versions_main.cc: plan + gather over generated logs against a sequential filter inside the file, compiled with
    -fsanitize=address,undefined and run as a child process (the LDS block and the scratch slices are exactly as large as the host library makes them)."""
    exe = str(tmp_path / "emu_versions_main")
    src = os.path.join(H.ROOT, "tests", "emu", "emu_versions_main.cc")
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "version emulation ok" in r.stdout
