"""The last phase of the merge kernel (LWW trees, tiles of the visible axis, spans, digest) at the exact edges of the visible length, on the CPU emulation:
every batch of tests/lww_edge_cases.py in every lane order, in the general and the lean body, with and without admission, through the HBM-staged path, and in
the smallest window the host would give it against the CU's whole LDS.  Expected values are the oracle's; tests/test_gpu_lww_edges.py repeats the batches in
every build of the kernel on the GPU, where the paths of a fixed workgroup size run."""
import os
import re

import numpy as np
import pytest

import helpers as H
import lww_edge_cases as LC
from peritext_amd import abi

T4, T1 = LC.T4, LC.T1
needs_emu = [pytest.mark.skipif(not os.path.exists(H.EMU_LIB), reason="tests/emu/libperitext_emu.so not built (run __graft_entry__.build())"),
             pytest.mark.skipif(not H.have_node(), reason="node (oracle runtime) not installed")]


def emu(fn):
    for m in needs_emu:
        fn = m(fn)
    return fn


def test_the_tile_sizes_are_the_kernels():
    """abi.LWW_TILE_4 / LWW_TILE_1, from which every edge size of the suite is taken, are merge_core.h's PTX_TILE_4 / PTX_TILE_1; the digest's flush still changes
    at 48 visible characters (no skip: this one needs no library)."""
    with open(os.path.join(H.ROOT, "peritext_amd", "csrc", "merge_core.h")) as f:
        core = f.read()
    assert int(re.search(r"#define\s+PTX_TILE_4\s+(\d+)u", core).group(1)) == abi.LWW_TILE_4 == T4
    assert int(re.search(r"#define\s+PTX_TILE_1\s+(\d+)u", core).group(1)) == abi.LWW_TILE_1 == T1
    assert re.search(r"if \(V >= 48u\) \{", core) and {47, 48, 49} <= set(LC.V_VALUES)
    assert {T4 - 1, T4, T4 + 1, 2 * T4 - 1, 2 * T4, 2 * T4 + 1, T1 - 1, T1, T1 + 1, 2 * T1 - 1, 2 * T1, 2 * T1 + 1, 2 * T1 + 2, 2 * T1 + 3, 4 * T1, 4 * T1 + 1} <= set(LC.V_VALUES)


@emu
def test_every_document_has_the_visible_length_it_is_there_for():
    cases, batches = LC.suite()
    for c in cases:
        assert [len(e["text"]) for e in c.expected] == [c.v] * len(c.logs), c.id
    assert sorted({c.v for c in cases if c.id[0] == "A"}) == sorted(LC.V_VALUES)
    assert sum(len(b.cases) for b in batches) == len(cases) and all(b.batch.n_logs < 64 for b in batches)
    for b in batches:  # a batch stays inside its regime: its launch is shaped by that regime's largest log
        assert {LC.regime_of(c.v) for c in b.cases} == {b.regime}, b.name
        for log, h in enumerate(b.batch.log_hdr):
            c = next(c for c in b.cases if c.id == b.case_of_log[log])
            assert {t for k, t in enumerate(LC.TYPES) if h["n_mark"][k]} == set(c.types), c.id
            assert int(h["n_ins"]) == c.v + (0 if c.id[0] == "N" else 3) and int(h["n_del"]) == (0 if c.id[0] == "N" else 3), c.id


@emu
def test_the_suite_covers_what_it_promises():
    """From the oracle's output: at every edge some document has a span that starts there and some document a span that runs through it; all fifteen non-empty
    sets of mark types occur at 2 T4 (the "mid" form: a tree per present type) and around it; at every V that is a whole tree or tile, a single mark covers the
    whole document in some document of every type; family B flips its winner with the actors' names."""
    cases, _ = LC.suite()
    for e in LC.EDGES:
        starts = [c.id for c in cases if c.v > e and any(e in LC.span_starts(x) for x in c.expected)]
        through = [c.id for c in cases if c.v > e and any(a < e < a + len(s["text"]) for x in c.expected for a, s in zip(LC.span_starts(x), x["spans"]))]
        assert starts and through, e
        marked_through = [c.id for c in cases if c.v > e and any(a < e < a + len(s["text"]) and s["marks"] for x in c.expected for a, s in zip(LC.span_starts(x), x["spans"]))]
        assert marked_through, e  # ... one that carries marks over the edge: what prev_attr hands from tile to tile
    for v in (T4 + 1, 2 * T4 - 1, 2 * T4, 2 * T4 + 1):
        assert {c.types for c in cases if c.id[0] == "A" and c.v == v} == set(LC.ALL_SUBSETS), v
    for v in (T4, 2 * T4, T1, 2 * T1):
        assert {c.whole for c in cases if c.id[0] in "AN" and c.v == v and c.whole} == set(LC.TYPES), v
    assert {c.whole for c in cases if c.v == 4 * T1} - {None}
    for c in cases:
        if c.whole in ("strong", "em") and c.v >= 31:  # the whole-document mark shows wherever no later op of its type reaches: from the first character on
            assert c.whole in c.expected[0]["spans"][0]["marks"], c.id
    # a type that covers a region alone (besides the whole-document mark): some span carries exactly that type
    for ty in LC.TYPES:
        assert any(set(s["marks"]) == {ty if ty != "comment" else "comments"} or set(s["marks"]) == {ty} for c in cases if c.v == 2 * T4 and len(c.types) > 1 and c.whole != ty
                   for s in c.expected[0]["spans"]), ty
    by_id = {c.id: c for c in cases}
    for v in LC.V_FAMILY_B:
        for kind in ("strong-em", "link-comment"):
            ab, ba = by_id["B-v%d-%s-ab" % (v, kind)], by_id["B-v%d-%s-ba" % (v, kind)]
            assert H.norm_spans(ab.expected[0]["spans"]) == H.norm_spans(ab.expected[1]["spans"])  # the order of application does not matter ...
            assert H.norm_spans(ab.expected[0]["spans"]) != H.norm_spans(ba.expected[0]["spans"]), (v, kind)  # ... the actors' rank does


@emu
@pytest.mark.skipif(not os.path.exists(os.path.join(H.ROOT, "oracle", "_ref", "micromerge.js")), reason="oracle/_ref not built (the type-erased reference)")
def test_the_reference_gives_the_same_spans():
    cases, _ = LC.suite()
    ref = H.oracle_apply([c.logs for c in cases], impl="ref", no_patches=True)
    for c, exp in zip(cases, ref):
        for mine, theirs in zip(c.expected, exp):
            assert "error" not in theirs, c.id
            assert H.norm_spans(mine["spans"]) == H.norm_spans(theirs["spans"]) and mine["text"] == theirs["text"], c.id


@emu
@pytest.mark.parametrize("admission", [False, True], ids=["no-admission", "admission"])
@pytest.mark.parametrize("lean", [False, True], ids=["general", "lean"])
@pytest.mark.parametrize("reverse", [0, 1, 2])
@pytest.mark.parametrize("name", LC.batch_names())
def test_every_batch_in_every_lane_order_and_body(name, reverse, lean, admission):
    b = LC.batch(name)
    LC.check_batch(b, H.emu_merge(b.batch, reverse=reverse, lean=lean, admission=admission))


@emu
@pytest.mark.parametrize("name", LC.batch_names())
def test_every_batch_through_the_hbm_staged_path(name):
    b = LC.batch(name)
    LC.check_batch(b, H.emu_merge_big(b.batch, admission=True))


def _rows(res):
    logs = res.logs.copy()
    logs["reserved"] = 0  # (the LDS the log used: what the two windows differ in)
    return logs.tobytes(), res.values.tobytes(), res.spans.tobytes(), res.cintervals.tobytes()


@emu
@pytest.mark.parametrize("lean", [False, True], ids=["general", "lean"])
@pytest.mark.parametrize("name", LC.batch_names())
def test_the_smallest_window_and_the_whole_lds_give_the_same_rows(name, lean):
    """The "mid" form and the double tile are taken where the launch's window has room for them: in the window the host sizes for the batch (the largest
    ptx_lds_need of its logs) and in the CU's whole LDS both outcomes of that test occur, and the rows must not depend on it."""
    b = LC.batch(name)
    need = max(LC.lds_need(b.batch))
    small = H.emu_merge(b.batch, lds_bytes=need, lean=lean)
    whole = H.emu_merge(b.batch, lds_bytes=160 * 1024, lean=lean)
    LC.check_batch(b, small)
    LC.check_batch(b, whole)
    assert _rows(small) == _rows(whole)
    used_small, used_whole = small.logs["reserved"][:, 0].astype(np.int64), whole.logs["reserved"][:, 0].astype(np.int64)
    assert (used_small <= need).all() and (used_whole >= used_small).all()


@emu
@pytest.mark.parametrize("name", [n for n in LC.batch_names() if not n.endswith(("v-le-65", "v-le-t4"))])
def test_every_log_in_a_window_of_exactly_its_own_need(name):
    """The batch's window is its largest log's: the smaller logs always have room to spare there.  Here every log runs in the window ptx_lds_need gives for it
    alone (one run of the batch per distinct need; the logs that need more fail with PTX_ERR_CAPACITY in that run and are not looked at): there the mid form and the
    double tile are refused for want of room, in the batches named at the end."""
    b = LC.batch(name)
    need = LC.lds_need(b.batch)
    whole = H.emu_merge(b.batch, lds_bytes=160 * 1024).logs["reserved"][:, 0]
    tighter = 0
    for w in sorted(set(need)):
        res = H.emu_merge(b.batch, lds_bytes=w)
        for log in (l for l, n in enumerate(need) if n == w):
            try:
                H.check_log(b.batch, res, log, b.expected[log])
            except AssertionError as err:
                raise AssertionError("%s in a window of %d bytes: %s" % (b.case_of_log[log], w, err)) from None
            assert int(res.logs["reserved"][log][0]) <= w
            tighter += int(res.logs["reserved"][log][0]) < int(whole[log])
    # (beyond 2 T1 + 3 characters the recycled element region holds the double tile in every window, up to T1 there is no larger form to take, and family B's few
    # mark ops leave the room for the mid form everywhere)
    if name in ("A-v-le-2t4", "A-v-t1+1", "A-v-le-2t1", "A-v-le-2t1+3"):
        assert tighter, name


@emu
def test_the_kernel_tables_follow_the_hosts_window_rule():
    """lww_edge_cases.GENERAL_KERNEL / LEAN_KERNEL / NATURAL, which tests/test_gpu_lww_edges.py observes on the GPU, are what the host's rule (launch_by_rule: the
    window from ptx_lds_need, the threads from the rows, the seven-wave and the lean builds from the logs per CU) gives for the batches as they are today."""
    _, batches = LC.suite()
    assert set(LC.GENERAL_KERNEL) == set(LC.LEAN_KERNEL) == set(LC.NATURAL) == {b.name for b in batches}
    for b in batches:
        assert tuple(LC.launch_by_rule(b.batch, t)[0] for t in LC.GENERAL_THREADS) == LC.GENERAL_KERNEL[b.name], b.name
        assert {LC.launch_by_rule(b.batch, t, 160 * 1024)[0] for t in LC.GENERAL_THREADS} == {LC.G}, b.name
        assert tuple(LC.launch_by_rule(b.batch, t, lean_context=True)[0] for t in LC.LEAN_THREADS) == LC.LEAN_KERNEL[b.name], b.name
        general, lean = LC.launch_by_rule(b.batch), LC.launch_by_rule(b.batch, lean_context=True)
        assert (general[1], general[2], general[0], lean[0]) == LC.NATURAL[b.name] and lean[1:] == general[1:], b.name
