"""The references and case builders of tests/layout_cases.py, held to something independent of them on the CPU — so that a wrong reference cannot make
tests/test_gpu_layout_kernels.py pass: the emulation's rows of the download base against what the reference itself answered, wire.census against a count
over the Change JSON, Batch.tile against an encode of the documents repeated, helpers.concat_batches against one encode of the whole logs, the convergence
count against a plain loop.  The builders' shapes (row counts, which row carries which maximum, offset counts, log counts) are asserted here, so the edges
the GPU module is about cannot drift."""
import json
import os

import numpy as np
import pytest

import helpers as H
import layout_cases as LC
from peritext_amd import abi, wire


# ---- 1. result offsets and compaction ----
def test_result_base_holds_every_kind_of_log_and_the_emulation_agrees_with_the_reference():
    kinds = [k for k, _ in LC.result_base_docs()]
    assert kinds[:2] == ["empty", "fails"] and kinds[-2:] == ["fails", "empty"] and len(kinds) == 8
    assert set(kinds) == {"empty", "fails", "all_deleted", "several_spans", "comments", "ordinary"}
    base = LC.result_base()
    exp = LC.emu_results(base)
    plain = H.emu_merge(base)
    LC.assert_logs_equal(exp.logs, plain.logs)  # (admission changes nothing for these logs)
    rows = np.diff(base.log_off.astype(np.int64))
    assert rows[0] == 0 and rows[-1] == 0
    for l, k in enumerate(kinds):
        r = exp.logs[l]
        if k == "fails":
            assert int(r["status"]) != 0 and (int(r["n_visible"]), int(r["n_spans"]), int(r["n_cintervals"])) == (0, 0, 0)
        else:
            assert int(r["status"]) == 0
    want = LC.result_base_expected()
    assert sorted(want) == [l for l, k in enumerate(kinds) if k not in ("empty", "fails")]
    for l, e in want.items():
        H.check_log(base, exp, l, e)
    by_kind = {k: exp.logs[l] for l, k in enumerate(kinds)}
    assert int(by_kind["all_deleted"]["n_visible"]) == 0 and int(by_kind["all_deleted"]["n_spans"]) == len(want[2]["spans"])
    assert int(by_kind["several_spans"]["n_spans"]) >= 3
    assert int(by_kind["comments"]["n_cintervals"]) > 0
    assert int(by_kind["empty"]["n_visible"]) == 0 and int(by_kind["empty"]["n_ops"]) == 0


def test_result_ranges_cross_the_chunk_and_stay_on_their_download_path():
    base = LC.result_base()
    n_logs = base.n_logs * LC.RESULT_COPIES
    assert n_logs > 2 * LC.CHUNK + 1 and max(LC.RANGE_SIZES) + 1 <= n_logs  # (first = 1 with the largest range stays inside)
    assert base.n_ops * LC.RESULT_COPIES <= LC.SMALL_DOWNLOAD_ROWS  # every range: the staging-block path
    assert base.n_ops * LC.RESULT_COPIES_LARGE > LC.SMALL_DOWNLOAD_ROWS and base.n_logs * LC.RESULT_COPIES_LARGE > 2 * LC.CHUNK  # the whole download: exact totals
    assert {LC.CHUNK - 1, LC.CHUNK, LC.CHUNK + 1, 2 * LC.CHUNK - 1, 2 * LC.CHUNK, 2 * LC.CHUNK + 1, 63, 64, 65, 0, 1} == set(LC.RANGE_SIZES)


def test_tiled_expectation_is_the_emulation_of_the_tiled_batch():
    """TiledExpectation (prefix sums of tiled counts, pieces put back to back) against the emulation run on the tiled batch itself, compacted by a plain loop."""
    base = LC.result_base()
    copies = 5
    te = LC.TiledExpectation(base, LC.emu_results(base), copies)
    tiled = base.tile(copies)
    full = LC.emu_results(tiled)
    assert te.n_logs == tiled.n_logs and np.array_equal(te.log_off, tiled.log_off)
    for first, n in ((0, tiled.n_logs), (1, 17), (tiled.n_logs - 9, 9), (3, 0)):
        LC.assert_logs_equal(te.logs[first:first + n], full.logs[first:first + n])
        offs = te.offsets(first, n)
        dense = te.dense(first, n)
        run = [0, 0, 0]
        parts = ([], [], [])
        for p in range(n):
            rows = wire.canonical_of_log(tiled, full, first + p)
            for k in range(3):
                assert int(offs[k][p]) == run[k]
                run[k] += len(rows[k])
                parts[k].append(rows[k])
        for k in range(3):
            assert len(offs[k]) == n + 1 and offs[k].dtype == np.uint64 and int(offs[k][n]) == run[k]
            assert dense[k].tobytes() == b"".join(x.tobytes() for x in parts[k])
        assert te.op_rows(first, n) == int(tiled.log_off[first + n]) - int(tiled.log_off[first])
    big = LC.TiledExpectation(base, LC.emu_results(base), LC.RESULT_COPIES)
    assert {0, 1023, 1024, 1025, 2048} <= set(big.sample(1, 2049))
    assert {p % 8 for p in big.sample(0, 64)} == set(range(8))  # one copy of every base log


# ---- 2. the device census ----
def test_census_cases_have_their_sizes_and_their_maxima_at_the_stride_edges():
    cases = LC.census_cases()
    batch = LC.census_batch()
    rows = np.diff(batch.log_off.astype(np.int64))
    assert [c[0] for c in cases] == rows.tolist()
    assert set(LC.CENSUS_SIZES) <= set(rows.tolist()) and LC.CENSUS_SIZES == (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025)
    seen = {"counter": set(), "actor": set(), "comment": set()}
    for l, (n, pc, pa, pm, flags) in enumerate(cases):
        got = LC.maxima_rows(batch, l)
        assert got[:2] == (pc, pa), (l, got)
        if pm is not None:
            assert got[2] == pm, (l, got)
        for kind, p in zip(("counter", "actor", "comment"), (pc, pa, pm)):
            if p is not None:
                seen[kind].add("last" if p == n - 1 and p not in LC.STRIDE_EDGES else p)
                if p == n - 1:
                    seen[kind].add("last")
    for kind in seen:
        assert seen[kind] >= {0, 63, 64, 255, 256, "last"}, (kind, seen[kind])
    by_flag = {c[4]: l for l, c in enumerate(cases)}
    hdr = batch.log_hdr
    assert int(hdr["n_comment_ids"][by_flag["no_comments"]]) == 0 and int(hdr["n_mark"][by_flag["no_comments"]][abi.MARK_COMMENT]) == 0
    m = by_flag["maps"]
    act = batch.action[int(batch.log_off[m]):int(batch.log_off[m + 1])]
    n_map = int(np.isin(act, (abi.ACT_MAPSET, abi.ACT_MAPDEL, abi.ACT_MAKELIST)).sum())
    assert n_map >= 3 and (act == abi.ACT_MAPSET).any()
    assert int(hdr["n_ins"][m]) + int(hdr["n_del"][m]) + int(hdr["n_mark"][m].sum()) == len(act) - n_map  # map rows count in none of the six counters
    for t in range(4):  # all four mark types, added and removed, and deletes, somewhere
        assert (hdr["n_mark"][:, t] > 0).any()
    assert (batch.action == abi.ACT_REMOVEMARK).any() and (hdr["n_del"] > 0).any()


def test_census_reference_against_a_count_over_the_changes():
    """wire.census (the GPU module's reference for ptx_census_kernel) against the fields counted over the Change JSON."""
    docs, _ = LC.census_docs()
    batch = LC.census_batch()
    again = wire.census(batch.log_off, batch.op_id, batch.action, batch.mark_type, batch.payload)
    assert np.array_equal(again, batch.log_hdr)
    for l, d in enumerate(docs):
        h = LC.census_of_changes(d[0], batch.doc_actors[l], batch.doc_comments[l])
        got = batch.log_hdr[l]
        assert (int(got["n_ins"]), int(got["n_del"]), got["n_mark"].tolist(), int(got["max_counter"]), int(got["max_actor"]), int(got["n_comment_ids"])) == \
            (h["n_ins"], h["n_del"], h["n_mark"], h["max_counter"], h["max_actor"], h["n_comment_ids"]), l


def test_census_logs_are_valid_documents():
    """Every log of the census cases merges (the headless one is no document of its own, only rows for the census: left out); the device merges them from both uploads and compares."""
    cases = LC.census_cases()
    batch = LC.census_batch()
    res = LC.emu_results(batch)
    for l, c in enumerate(cases):
        if c[4] != "headless":
            assert int(res.logs["status"][l]) == 0, (l, c, int(res.logs["status"][l]))


# ---- 3. the tiled upload ----
def test_tile_shapes_and_the_tiling_reference():
    assert tuple(n * c + 1 for n, c in LC.TILE_SHAPES) == LC.TILE_OFFSET_COUNTS == (255, 256, 257, 512, 513, 1025)
    for n_logs, copies in LC.TILE_SHAPES:
        docs = LC.small_docs(n_logs)
        batch = wire.encode_docs(docs)
        rows, chgs = np.diff(batch.log_off.astype(np.int64)), np.diff(batch.chg_off.astype(np.int64))
        assert batch.n_logs == n_logs and rows[0] == 0 and rows[-1] == 0
        assert (chgs == 0).sum() >= 2 and (chgs[1:-1] == 0).any()  # repeated chg_off entries, also inside
        tiled = batch.tile(copies)
        assert len(tiled.log_off) == n_logs * copies + 1 == len(tiled.chg_off)
        if n_logs * copies <= 256:  # (the encode of the repeated documents: the small shapes are enough to hold Batch.tile to it)
            LC.assert_batches_equal(tiled, wire.encode_docs(docs * copies), what="tile %d x %d" % (n_logs, copies))


# ---- 4. append ----
def test_concat_batches_against_one_encode_of_the_whole_logs():
    with open(os.path.join(H.GOLDEN, "ptxgen_rich_700.json")) as f:
        g = json.load(f)
    full = wire.encode_docs([d["logs"] for d in g["docs"]])
    nch = np.diff(full.chg_off.astype(np.int64))
    for cut in (nch * 2 // 3, nch * 0, nch, np.arange(len(nch)) % 3):
        head, tail = wire.split_batch(full, cut)
        LC.assert_batches_equal(LC.appended(head, tail), full, what="concat")
    parts = LC.split_in_four(full)
    grown = parts[0]
    for p in parts[1:]:
        grown = LC.appended(grown, p)
    LC.assert_batches_equal(grown, full, what="four parts")


def test_append_cases_have_their_row_counts_log_counts_and_strides():
    whole, base, more = LC.append_rows_case()
    sides = set(LC.APPEND_ROW_PAIRS)
    assert {(0, 0), (0, 5), (5, 0)} <= sides
    for n in (1, 255, 256, 257, 600):
        assert any(a == n for a, _ in sides) and any(b == n for _, b in sides), n
    LC.assert_batches_equal(LC.appended(base, more), whole, what="rows")
    assert abi.env_stride(whole.max_actors) == 4
    w9, b9, m9 = LC.append_rows_case(extra_actors=6)
    assert w9.max_actors == 9 and abi.env_stride(9) == 12 and b9.max_actors == m9.max_actors == 9
    LC.assert_batches_equal(LC.appended(b9, m9), w9, what="nine actors")
    for n in LC.APPEND_LOG_COUNTS:
        w, b, m = LC.append_logs_case(n)
        assert w.n_logs == b.n_logs == m.n_logs == n
        LC.assert_batches_equal(LC.appended(b, m), w, what="%d logs" % n)
    assert LC.APPEND_LOG_COUNTS == (255, 256, 257)


def test_wide_column_cases():
    _, base, more = LC.append_rows_case()
    assert base.chg_env_hi is None and more.chg_env_hi is None
    wb, wm, zb = LC.with_wide_column(base, True), LC.with_wide_column(more, True), LC.with_wide_column(base, False)
    assert wb.chg_env_hi.any() and wm.chg_env_hi.any() and zb.chg_env_hi is not None and not zb.chg_env_hi.any()
    assert np.array_equal(zb.chg_env, base.chg_env) and np.array_equal(zb.chg_hdr, base.chg_hdr)
    assert int(wb.chg_seq.max()) > 65535 and np.array_equal(wb.chg_deps, base.chg_deps)
    es = abi.env_stride(base.max_actors)
    for b, m in ((wb, more), (base, wm), (wb, wm), (zb, more)):
        out = LC.appended(b, m)
        assert out.chg_env_hi is not None and len(out.chg_env_hi) == len(out.chg_env)
        # the side without the column contributes zeros, the side with it its own values: row by row
        hi = out.chg_env_hi.reshape(-1, es)
        for l in range(b.n_logs):
            d0, nb_, nm_ = int(out.chg_off[l]), int(b.chg_off[l + 1] - b.chg_off[l]), int(m.chg_off[l + 1] - m.chg_off[l])
            for side, k0, cnt, at in ((b, int(b.chg_off[l]), nb_, d0), (m, int(m.chg_off[l]), nm_, d0 + nb_)):
                want = np.zeros((cnt, es), np.uint16) if side.chg_env_hi is None else side.chg_env_hi.reshape(-1, es)[k0:k0 + cnt]
                assert np.array_equal(hi[at:at + cnt], want)
    assert LC.appended(base, more).chg_env_hi is None
    e = LC.empty_base(more.n_logs)
    assert e.n_ops == 0 and e.chg_off is None and LC.appended(e, more) is more


# ---- 5. convergence counts ----
@pytest.mark.parametrize("replicas", LC.CONVERGED_REPLICAS)
def test_converged_count_reference_against_a_plain_loop(replicas):
    seen = set()
    for n_docs in LC.CONVERGED_DOCS:
        for variant in range(3):
            dg, kinds = LC.synthetic_digests(n_docs, replicas, variant)
            assert dg.shape == (n_docs + 1, replicas, 2) and dg.dtype == np.uint64
            want = 0
            for d in range(n_docs):
                first = (int(dg[d, 0, 0]), int(dg[d, 0, 1]))
                want += first != (0, 0) and all((int(dg[d, r, 0]), int(dg[d, r, 1])) == first for r in range(replicas))
            assert LC.converged_count(dg, n_docs) == want
            last = (int(dg[n_docs, 0, 0]), int(dg[n_docs, 0, 1]))
            assert last != (0, 0) and all((int(dg[n_docs, r, 0]), int(dg[n_docs, r, 1])) == last for r in range(replicas))  # the document behind the last would count
            for d, k in kinds.items():
                seen.add((k, "last" if d == n_docs - 1 else d))
                if k in LC.DIVERGENCE_KINDS:
                    differs = {(r, w) for r in range(replicas) for w in range(2) if dg[d, r, w] != dg[d, 0, w]}
                    assert len(differs) == 1
                    r, w = next(iter(differs))
                    assert {"first_word": w == 0, "second_word": w == 1, "last_replica": r == replicas - 1}[k]
                elif k == "zero_first_word":
                    assert not dg[d, :, 0].any() and dg[d, :, 1].all()
    assert {("failed", 3), ("failed", 253), ("zero_first_word", 2), ("zero_first_word", 258)} <= seen
    if replicas > 1:
        for k in LC.DIVERGENCE_KINDS:  # every kind of divergence at every edge
            assert {e for kk, e in seen if kk == k} >= {0, 63, 64, 255, 256, "last"}, k


def test_convergence_documents():
    docs = LC.convergence_docs()
    assert len(docs) == 8 and all(len(d) == 3 for d in docs)
    batch = wire.encode_docs(docs)
    res = LC.emu_results(batch)
    dg, st = res.logs["digest"].reshape(8, 3, 2), res.logs["status"].reshape(8, 3)
    conv = (dg == dg[:, :1, :]).all(axis=(1, 2)) & (st == 0).all(axis=1)
    assert conv.tolist() == [False, True, True, False, True, True, True, False]
    assert (st[3] != 0).all() and (st[[0, 7]] == 0).all()  # one document fails in every replica; the lagging ones merge, to another digest
    assert LC.converged_logs_count(res.logs, 3) == 5 and LC.converged_logs_count(res.logs, 1) == 21
    assert tuple(8 * c for c in LC.CONVERGENCE_COPIES) == (56, 64, 72, 248, 256, 264)
    assert LC.PACK_COUNTS == (0, 1, 255, 256, 257)


# ---- 6. the patch pack ----
def test_patch_pack_case_puts_an_empty_and_a_failing_log_at_both_ends():
    batch, want = LC.patch_pack_case()
    rows = np.diff(batch.log_off.astype(np.int64))
    assert rows[0] == 0 and rows[-1] == 0 and sorted(want) == list(range(2, batch.n_logs - 2))
    res = LC.emu_results(batch)
    assert int(res.logs["status"][1]) != 0 and int(res.logs["status"][-2]) != 0 and (res.logs["status"][2:-2] == 0).all()
    pat = H.emu_replay(batch, H.emu_merge(batch))
    for log, patches in want.items():
        assert H.norm_patches(wire.decode_patches(batch, pat, log)) == H.norm_patches(patches)
