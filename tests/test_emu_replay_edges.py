"""The patch replay at its word, chunk, tile and extent edges on the CPU emulation: the batches of tests/replay_edge_cases.py (expected streams: the oracle's, one
run for the module) through ptx_replay_walk compiled with -DPTX_EMU over every store — the LDS store in its plain form, with the tables in global memory
(`gwin`) and wide (a 32 767-char ballast log beside the batch, by the driver's own rule), and the HBM store (tests/emu/emu_replay_hbm.cc) — in every lane order
the drivers offer (0: ascending, 1: descending, 2: permuted), in a window of exactly the batch's need and in 160 KB; tails (first_row); the overflow extents
against a restatement of the reserve rule; and a coverage test that holds the cases to what they promise (the slots they aim at, the dropped / kept twins, the
table sizes, the capacity regimes).  tests/test_gpu_replay_edges.py runs the same batches through the library on the GPU.

Measured here (one CPU core): the oracle's single run over the 229 documents 14 s (the three 16 K-element documents of family P do not dominate it: all four
stay); the type-erased reference over the same 15 s; the superblock document of family K (131 202 chars: HBM-staged merge, then the HBM-state replay in two lane
orders) 11 s; the 32 767-char ballast beside a batch 1 to 6 s per batch (10 s beside the 16 K-element documents); the whole file 200 s."""
import os
import re
import time

import numpy as np
import pytest

import helpers as H
import replay_edge_cases as RC
import replay_hbm_docs as D
from peritext_amd import abi, wire

emu = pytest.mark.skipif(not (os.path.exists(H.EMU_LIB) and os.path.exists(D.EMU_HBM_LIB)), reason="tests/emu/*.so not built (run __graft_entry__.build())")
CSRC = os.path.join(H.ROOT, "peritext_amd", "csrc")
_MERGED = {}


def _merged(b):
    """the emulation's merge of a batch (once per module: the replay under test reads it, nothing here checks it)"""
    if b.name not in _MERGED:
        res = H.emu_merge_big(b.batch) if b.big else H.emu_merge(b.batch)
        assert (res.logs["status"] == 0).all(), b.name
        _MERGED[b.name] = res
    return _MERGED[b.name]


def _needs(batch):
    """(everything in the LDS, the tables in global memory) per log: ptx_replay_lds_need_hdr, as replay_edge_cases.lds_need restates it — held here, for every
    log, to the library's own answers in the two forms it exports: everything in the LDS (ptx_emu_replay_lds_need) and wide with the tables in global memory
    (ptx_emu_replay_lds_need_wide)"""
    import ctypes as C

    lib = H._emu(H.EMU_LIB)
    lib.ptx_emu_replay_lds_need.restype, lib.ptx_emu_replay_lds_need.argtypes = C.c_uint64, [C.c_uint64] * 5
    lib.ptx_emu_replay_lds_need_wide.restype, lib.ptx_emu_replay_lds_need_wide.argtypes = C.c_uint64, [C.c_uint64] * 4
    out = []
    for log, h in enumerate(batch.log_hdr):
        n, K, Kc = int(h["n_ins"]), int(h["n_mark"].sum()), int(h["n_mark"][abi.MARK_COMMENT])
        Kid = int(h["n_comment_ids"]) if Kc else 0
        assert RC.lds_need_of(batch, log) == int(lib.ptx_emu_replay_lds_need(n, K, Kc, 0, Kid))
        assert RC.lds_need_of(batch, log, True, True) == int(lib.ptx_emu_replay_lds_need_wide(n, K, Kc, Kid))
        out.append((RC.lds_need_of(batch, log), RC.lds_need_of(batch, log, True)))
    return out


def test_the_constants_are_the_headers():
    """the sizes every case is built from, against the text of replay_core.h, replay_hbm_core.h and the host's rule (no skip: this one needs no library)"""
    core, hbm, host = (open(os.path.join(CSRC, f)).read() for f in ("replay_core.h", "replay_hbm_core.h", "peritext_hip.hip"))
    assert int(re.search(r"#define\s+PTX_RCHUNK\s+(\d+)u", core).group(1)) == RC.RCHUNK
    assert int(re.search(r"#define\s+PTX_HBM_TILE\s+(\d+)u", hbm).group(1)) == RC.HBM_TILE
    assert int(re.search(r"#define\s+PTX_REPLAY_GWIN_ABOVE\s+(\d+)u", host).group(1)) == RC.GWIN_ABOVE
    assert "ptx_a16((wide ? 24 : 16) * PTX_RCHUNK) + ptx_a16(PTX_RCHUNK) +" in core and "(gscratch ? 0 : ptx_a16(4 * (2 * n + 2)) + ptx_a16((wide ? 16 : 8) * (Kl + 1))" in core
    assert re.search(r"nws = \(\(2 \* n \+ 2\) >> 5\) \+ 2", core) and re.search(r"\(w_\) \+ 1u\) << 4\)", core) and RC.WORD == 32  # 32 slots, 16 elements a word
    assert re.search(r"ptx_replay_kernel\w*, dim3\(\w+\), dim3\(PTX_REPLAY_THREADS\)", host) and re.search(r"#define\s+PTX_REPLAY_THREADS\s+64\b", host) and RC.LANES == 64
    assert re.search(r"PTX_FOR\(j, 64u\)", hbm) and re.search(r"\(L\.nblk \+ 63u\) >> 6", hbm) and RC.BLOCK_WORDS == 64 and RC.SUPERBLOCK == 64 * 64 * 32
    assert re.search(r"h\.n_ins > (\d+)u \|\| N > 65534u", core).group(1) == str(RC.WIDE_ABOVE) and RC.K_BALLAST == RC.WIDE_ABOVE + 1
    assert re.search(r"h->off\[l \+ 1\] = h->off\[l\] \+ 2 \* \(n - skip\) \+ 16;", host)  # the guessed capacity of family X
    assert re.search(r"rate = 3u \* \(npatch / \(t0 > first \? t0 - first \+ 1u : 1u\) \+ 1u\);\s*rate = rate < 8u \? 8u : rate;", core)
    assert re.search(r"rate \*= ext_left == 2u \? 1u : 16u;\s*const uint64_t want64 = \(uint64_t\)rate \* \(N - t0\) \+ 1024u;", core)
    assert re.search(r"arena_cap = attempt == 0 && !no_arena_env \? total \+ 65536 : 0;", host)
    assert {15, 16, 17, 31, 32, 33, 47, 48, 49} == set(RC.W_SIZES) and {1, 63, 64, 65, 129} == set(RC.L_TABLES) and {31, 32, 33, 64, 65} == set(RC.C_KC)
    assert {511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 16 * RC.HBM_TILE - 1, 16 * RC.HBM_TILE, 16400} == set(RC.P_SIZES)


@emu
def test_the_need_table_is_the_kernels():
    """replay_edge_cases.NEED, the literal table the GPU file takes its builds from, against ptx_replay_lds_need_hdr; every regime is there"""
    got = {b.name: tuple(max(n[k] for n in _needs(b.batch)) for k in (0, 1)) for b in RC.batches()}
    assert got == RC.NEED, got
    builds = {name: RC.build_of(name, "default") for name in RC.NEED}
    assert {"ptx_replay_kernel", "ptx_replay_kernel_gwin"} == set(builds.values())
    assert all(builds[name + "+big"] == "ptx_replay_kernel_gwin" and builds[name] == "ptx_replay_kernel" for name in RC.STEERED)
    assert RC.build_of("P-big", "lds-only") == "ptx_replay_kernel_hbm" and RC.build_of("P-mid", "lds-only") == "ptx_replay_kernel"
    for b in RC.batches():  # a batch stays on one side: every log of P-big is beyond the LDS with everything in it
        if b.name == "P-big":
            assert all(n[0] > RC.LDS_CU >= n[1] for n in _needs(b.batch))


@emu
def test_the_reference_gives_the_same_streams():
    """the oracle's streams, which everything here is compared with, against the type-erased reference's (where it has been built)"""
    if not os.path.exists(os.path.join(H.ROOT, "oracle", "_ref", "micromerge.js")):
        pytest.skip("oracle/_ref not built (the reference is not on this machine)")
    cases, _ = RC.suite()
    ref = H.oracle_apply([c.logs for c in cases], impl="ref", patches=True, timeout=1800)
    for c, exp in zip(cases, ref):
        for mine, theirs in zip(c.expected, exp):
            assert "error" not in theirs, c.id
            assert H.norm_patches(mine["patches"]) == H.norm_patches(theirs["patches"]), c.id
            assert H.norm_spans(mine["spans"]) == H.norm_spans(theirs["spans"]), c.id


@emu
@pytest.mark.parametrize("reverse", [0, 1, 2])
@pytest.mark.parametrize("form", ["plain", "gwin", "hbm"])
@pytest.mark.parametrize("name", RC.batch_names())
def test_every_batch_in_every_store_and_lane_order(name, form, reverse):
    b = RC.batch(name)
    res = _merged(b)
    if form == "hbm":
        return RC.check_batch(b, D.emu_replay_hbm(b.batch, res, reverse=reverse))
    need = RC.NEED[name][form == "gwin"]
    if need > RC.LDS_CU:  # (P-big with everything in the LDS: refused, no records)
        pat = H.emu_replay(b.batch, res, reverse=reverse)
        assert (pat.logs["status"] == abi.ERR_CAPACITY).all() and not pat.logs["n_patches"].any()
        return
    for window in (need, RC.LDS_CU):  # exactly what the host gives the launch, and the CU's whole LDS
        RC.check_batch(b, H.emu_replay(b.batch, res, lds_bytes=window, reverse=reverse, gwin=form == "gwin"))


@emu
@pytest.mark.parametrize("name", RC.batch_names())
def test_every_batch_beside_the_ballast_takes_the_wide_build(name):
    """typed_log(32 767) as one more log: the driver's rule (ptx_replay_wants_wide, as the host's) replays the whole batch with 32-bit ranks and slots; the
    ballast's own stream is the known one"""
    b = RC.batch(name)
    batch, at = RC.with_ballast(b)
    assert int(batch.log_hdr["n_ins"][at]) == RC.K_BALLAST
    res = H.emu_merge_big(batch)
    assert (res.logs["status"] == 0).all()
    for reverse in (0, 2):
        pat = H.emu_replay(batch, res, reverse=reverse)
        RC.check_batch(RC.rebatched(b, batch), pat)
        assert H.norm_patches(wire.decode_patches(batch, pat, at)) == RC.typed_stream(RC.K_BALLAST)


def _tail_check(b, pat, first):
    assert int(pat.logs["status"][0]) == 0
    got = H.norm_patches(wire.decode_patches(b.batch, pat, 0))
    want = H.norm_patches(RC.tail_expected(first))
    assert int(pat.logs["n_patches"][0]) == len(pat.of_log(0)) and got == want, (first, len(got), len(want))


@emu
@pytest.mark.parametrize("first", RC.R_FIRST)
def test_tails_are_the_oracles_records_of_the_rows_asked_for(first):
    """first_row on the 97-row log of one op per change: exactly what the oracle produces after a prefix of `first` changes, in every store and lane order"""
    b = RC.batch("R-tail")
    res = _merged(b)
    fr = np.array([first], np.uint32)
    for reverse in (0, 1, 2):
        _tail_check(b, H.emu_replay(b.batch, res, reverse=reverse, first_row=fr), first)
        _tail_check(b, H.emu_replay(b.batch, res, reverse=reverse, first_row=fr, gwin=True), first)
        _tail_check(b, D.emu_replay_hbm(b.batch, res, reverse=reverse, first_row=fr), first)


def _x_run(name, form, reverse=0):
    """one X log alone as the host launches it: its guessed capacity 2 N + 16 and an arena of all capacities + 65 536 records"""
    b = RC.batch("X-%s" % name)
    res = _merged(b)
    N = int(b.batch.log_off[1])
    cap = 2 * N + 16
    if form == "hbm":
        return b, cap, D.emu_replay_hbm_with_arena(b.batch, res, cap=cap, arena=cap + 65536, reverse=reverse)
    return b, cap, H.emu_replay_with_arena(b.batch, res, cap=cap, arena=cap + 65536, reverse=reverse, gwin=form == "gwin")


@emu
@pytest.mark.parametrize("form", ["plain", "gwin", "hbm"])
@pytest.mark.parametrize("name", list(RC.X_LOGS))
def test_capacity_regimes(name, form):
    """The extents each X log takes are those of the reserve rule restated (replay_edge_cases.reserve_model) over the oracle's records per row; a log whose
    records were all written gives the oracle's stream from capacity + extents; one that lost records reports PTX_ERR_CAPACITY with the exact count — whatever
    room it is granted afterwards — and gives the stream in the second run with exact capacities (what the host launches then)."""
    b, cap, (pat, ext) = _x_run(name, form)
    per_row = RC.case("X-%s" % name).note["per_row"]
    exts, produced, room, lost = RC.reserve_model(per_row, cap + 65536)
    assert (len(exts), lost) == RC.X_REGIME[name] and produced == len(b.expected[0][0]["patches"]) == sum(per_row)
    assert int(pat.logs["n_patches"][0]) == produced
    taken = [int(x) != D.NONE64 for x in ext[0, :2]]
    if lost:
        assert int(pat.logs["status"][0]) == abi.ERR_CAPACITY, "records were lost: no extent granted later brings them back"
    else:
        assert taken == [len(exts) > 0, len(exts) > 1] and (not exts or int(ext[0, 2]) == exts[0][1])
        RC.check_batch(b, pat)
    again = (D.emu_replay_hbm if form == "hbm" else H.emu_replay)(b.batch, _merged(b))  # no arena: twice where 2 N + 16 is too little
    assert again.launches == (2 if produced > cap else 1)
    RC.check_batch(b, again)


@emu
def test_the_capacity_logs_in_one_batch_with_and_without_an_arena():
    """the four X logs beside each other: one arena of all capacities + 65 536 records (the extents of `extents` fit it), and none at all"""
    b = RC.batch("X")
    res = _merged(b)
    for lib in (H, D):
        again = (lib.emu_replay_hbm if lib is D else lib.emu_replay)(b.batch, res)
        assert again.launches == 2
        RC.check_batch(b, again)


@emu
def test_the_suite_does_what_it_promises():
    cases, batches = RC.suite()
    by_id = {c.id: c for c in cases}
    # every slot a case aims at is where the merge resolves the op's boundaries to (slot = 2 * rank + side; 0xFFFF: none, endOfText)
    n_aims = 0
    for b in batches:
        res = _merged(b)
        for log, cid in enumerate(b.case_of_log):
            c, b0 = by_id[cid], int(b.batch.log_off[log])
            big = int(b.batch.log_hdr["n_ins"][log]) > RC.WIDE_ABOVE
            for row, sa, sb in c.aims or ():
                v = int(res.ref_slots[b0 + row])
                assert not big and (v & 0xFFFF, v >> 16) == (sa, sb), (cid, row, sa, sb, v & 0xFFFF, v >> 16)
                n_aims += 1
    assert n_aims > 5000
    # W: per type and edge, ops that start at 30 / 32 / 34 and 62 / 64 / 66 and end at every reachable slot of 30 .. 35 and 62 .. 67, endOfText included
    for ty in RC.TYPES:
        got = {(sa, sb) for c in cases if c.family == "W" and c.note["ty"] == ty for _, sa, sb in c.aims}
        ends = (30, 32, 34, 62, 64, 66) if ty in ("strong", "em") else (31, 33, 35, 63, 65, 67)
        assert {(s, RC.NONE16) for s in (30, 32, 34, 62, 64, 66)} <= got and {(0, e) for e in ends} <= got and {(32, 64 if ty in ("strong", "em") else 63)} <= got
        assert {(32, 32), (64, 64)} <= got if ty in ("strong", "em") else {(32, 31), (64, 63)} <= got  # start == end / end just before the start
        assert any(sb < sa for sa, sb in got)  # an end met before the start
    assert {c.note["n"] for c in cases if c.family == "W"} == set(RC.W_SIZES)
    # Z: a dropped variant has exactly one mark patch fewer than each of its kept twins (which delete one element less), whose extra patch is one char wide
    twins = 0
    for c in cases:
        if c.family == "Z" and c.note["twin"]:
            marks, dropped = ([p for p in x.expected[0]["patches"] if p["action"] in ("addMark", "removeMark")] for x in (c, by_id[c.note["twin"]]))
            assert len(marks) == len(dropped) + 1, c.id
            assert len(marks) >= 2 and marks[-2]["endIndex"] - marks[-2]["startIndex"] == 1, (c.id, marks[-2:])
            twins += 1
    assert twins == 2 * 2 * sum(len(k) for _, _, k in RC.Z_RUNS.values())
    # L: the table of applied ops of the type holds T entries when the first op of the typing actor arrives; the swapped twin's stream differs
    for c in cases:
        if c.family == "L" and c.id.endswith("-ab"):
            b = next(b for b in batches if c.id in b.case_of_log)
            log = b.case_of_log.index(c.id)
            b0, first = int(b.batch.log_off[log]), c.aims[0][0]
            ty = RC.TYPES.index(c.note["ty"])
            code = {"strong": abi.MARK_STRONG, "em": abi.MARK_EM, "link": abi.MARK_LINK}[c.note["ty"]]
            before = sum(1 for r in range(first) if int(b.batch.action[b0 + r]) in (abi.ACT_ADDMARK, abi.ACT_REMOVEMARK) and int(b.batch.mark_type[b0 + r]) == code)
            assert before == c.note["T"] and ty < 3, c.id
            twin = by_id[c.id[:-3] + "-ba"]
            assert H.norm_patches(c.expected[0]["patches"]) != H.norm_patches(twin.expected[0]["patches"]), c.id
    assert {c.note["T"] for c in cases if c.family == "L"} == set(RC.L_TABLES)
    # C: the comment-op counts; R: the row counts; P: the element counts
    for c in cases:
        if c.family == "C" and "kc" in c.note:
            assert sum(1 for _ in c.aims) == c.note["kc"], c.id
        if c.family == "R":
            assert sum(len(ch["ops"]) for ch in c.logs[0]) == c.note["rows"], c.id
    pb = RC.batch("P-small").batch, RC.batch("P-mid").batch, RC.batch("P-big").batch
    assert sorted(int(n) for x in pb for n in x.log_hdr["n_ins"]) == sorted(RC.P_SIZES + (16400,))
    # X: the three regimes (test_capacity_regimes holds the emulation's extents to them)
    assert [RC.X_REGIME[n] for n in ("inside", "extents", "burst")] == [(0, 0), (2, 0), (0, 277)]


@emu
def test_a_document_of_more_than_one_superblock():
    """Family K: 131 072 + 130 typed chars, deletes at ranks 0, 131 071, 131 072 and the last, a strong mark across the superblock edge, inserts behind the
    deleted elements' neighbours: the stream of a plain list model (validated against the oracle on a 300-element miniature by suite()).  Its state exceeds the
    LDS in every form, so only the HBM store holds it: spre[1] and the prefixes of the second superblock's blocks carry non-zero values here."""
    RC.suite()  # (the miniature)
    log, want = RC.k_super()
    batch = wire.encode_docs([[log]])
    assert RC.lds_need_of(batch, 0, gscratch=True, wide=True) > RC.LDS_CU
    t0 = time.time()
    res = H.emu_merge_big(batch)
    assert int(res.logs["status"][0]) == 0
    for reverse in (0, 2):
        pat = D.emu_replay_hbm(batch, res, reverse=reverse)
        assert int(pat.logs["status"][0]) == 0 and int(pat.logs["n_patches"][0]) == len(want)
        assert H.norm_patches(wire.decode_patches(batch, pat, 0)) == H.norm_patches(want)
    print("\nfamily K in the emulation: %.1f s" % (time.time() - t0))
