"""The kernels written directly in peritext_amd/csrc/peritext_hip.hip — no CPU build, reached by the rest of the suite only as a side effect — through the C ABI on a
real MI355X, at their block, wave and chunk edges (tests/layout_cases.py: the case builders and numpy references, held to independent ones by
tests/test_layout_cases.py):

  1. ptx_result_offsets_kernel / ptx_result_compact_kernel   download_range past one and two 1 024-log chunks, both download paths
  2. ptx_census_kernel (compute = 1)                         log headers against wire.census, maxima at rows 0 / 63 / 64 / 255 / 256 / last
  3. ptx_tile_offsets_kernel                                 upload(copies) read back, 255 .. 1 025 offsets
  4. ptx_append_offsets_kernel / ptx_append_rows_kernel / ptx_append_hi   append and append_device, empty sides, 255 / 256 / 257 logs, the wide column
  5. ptx_count_converged*_kernel / ptx_pack_digests_kernel   lagging and failed documents at the wave and block edges
  6. ptx_patch_pack_kernel                                   the packed copy as large as the longest stream, one more, the total less one, the total

Every check is array or byte equality.  Expected rows come from the CPU emulation of the merge (run in a child process: tests/test_gpu_parity.py asserts that
it is never loaded beside the HIP library), expected offsets are prefix sums of ITS counts, never of what the library returned."""
import os

import numpy as np
import pytest

import helpers as H
import layout_cases as LC
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


def _merged_logs_and_rows(eng, db):
    """Merge a resident batch into fresh result buffers: (ptx_log_result rows, the whole download)."""
    dr = eng.alloc_result(db)
    try:
        eng.merge(db, dr)
        eng.sync()
        return eng.download_logs(dr, eng.n_logs(db)), eng.download(db, dr)
    finally:
        eng.free_result(dr)


def _assert_same_results(a, b):
    """Two downloads of the same logs: every log row, offset and dense row, byte for byte."""
    for k in ("logs", "value_off", "span_off", "cint_off", "values", "spans", "cintervals"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


# ---- 1. result offsets and compaction past one chunk ----
@pytest.fixture(scope="module")
def base_and_emulation():
    return LC.result_base(), LC.emu_results_in_child("result_base")


@pytest.fixture(scope="module")
def resident(eng, base_and_emulation):
    """The base tiled to 2 056 logs, merged once: (batch handle, result handle, the emulation's result tiled in numpy)."""
    base, exp = base_and_emulation
    te = LC.TiledExpectation(base, exp, LC.RESULT_COPIES)
    db = eng.upload(base, copies=LC.RESULT_COPIES)
    dr = eng.alloc_result(db)
    eng.merge(db, dr)
    eng.sync()
    yield db, dr, te
    eng.free_result(dr)
    eng.free_batch(db)


@pytest.mark.parametrize("first_name", LC.RANGE_FIRSTS)
@pytest.mark.parametrize("n", LC.RANGE_SIZES)
def test_download_range_offsets_and_rows(eng, resident, n, first_name):
    """value_off / span_off / cint_off = exclusive prefix sums of the emulation's n_visible / n_spans / n_cintervals over the range (the carry between the offsets
    kernel's 1 024-log chunks, its last entry), dense arrays of exactly the totals, the log rows and every dense row the emulation's."""
    db, dr, te = resident
    assert eng.n_logs(db) == te.n_logs and te.n_logs > 2 * LC.CHUNK + 1
    first = te.first_of(first_name, n)
    assert te.op_rows(first, n) <= LC.SMALL_DOWNLOAD_ROWS  # the staging-block path
    got = eng.download_range(db, dr, first, n)
    te.check(got, first, n)
    assert got.logs.tobytes() == eng.download_logs(dr, te.n_logs)[first:first + n].tobytes()  # (reserved[0] too: the plain copy of the same rows)


def test_small_range_after_a_large_one(eng, resident):
    """The context keeps its staging blocks between downloads: a small range read after a large one must hold none of the large one's rows."""
    db, dr, te = resident
    for first, n in ((0, 2049), (1, 1), (te.n_logs - 2049, 2049), (2, 0), (5, 3), (0, te.n_logs), (te.n_logs - 1, 1)):
        te.check(eng.download_range(db, dr, first, n), first, n)


def test_whole_download_beyond_65536_rows_and_2048_logs(eng, base_and_emulation):
    """The exact-totals path (offsets first, dense arrays allocated to the totals) over more than ten chunks of logs; then small ranges on the same engine."""
    base, exp = base_and_emulation
    te = LC.TiledExpectation(base, exp, LC.RESULT_COPIES_LARGE)
    db = eng.upload(base, copies=LC.RESULT_COPIES_LARGE)
    dr = eng.alloc_result(db)
    try:
        assert eng.n_logs(db) == te.n_logs > 2 * LC.CHUNK and eng.n_ops(db) == te.op_rows(0, te.n_logs) > LC.SMALL_DOWNLOAD_ROWS
        eng.merge(db, dr)
        eng.sync()
        te.check(eng.download(db, dr), 0, te.n_logs)
        for first, n in ((te.n_logs - 1025, 1025), (1, 2049), (te.n_logs - 1, 1)):
            assert te.op_rows(first, n) <= LC.SMALL_DOWNLOAD_ROWS
            te.check(eng.download_range(db, dr, first, n), first, n)
    finally:
        eng.free_result(dr)
        eng.free_batch(db)


# ---- 2. the device census against wire.census ----
def _assert_headers(got, want, what):
    assert got.dtype == want.dtype == abi.LOG_HDR_DTYPE and len(got) == len(want), what
    for f in abi.LOG_HDR_DTYPE.names:
        bad = np.flatnonzero((got[f] != want[f]).reshape(len(got), -1).any(axis=1))
        assert len(bad) == 0, "%s: %s of logs %s: %s, expected %s" % (what, f, bad.tolist(), got[f][bad].tolist(), want[f][bad].tolist())


def test_census_on_the_device_at_its_stride_edges(eng):
    """Upload without log headers: the census kernel's six counters and three maxima (wave shuffles, LDS atomics, a 256-row stride) against wire.census, for logs
    of 0 .. 1 025 rows whose maxima stand at rows 0 / 63 / 64 / 255 / 256 / last; the launch shape, the kernel chosen and the merge results are those of the
    same batch uploaded with the encoder's headers."""
    batch = LC.census_batch()
    want = wire.census(batch.log_off, batch.op_id, batch.action, batch.mark_type, batch.payload)
    db_hdr = eng.upload(batch)
    db_dev = eng.upload(LC.batch_without(batch, "log_hdr"))
    try:
        got = eng.download_batch(db_dev)
        _assert_headers(got.log_hdr, want, "upload without headers")
        LC.assert_batches_equal(got, batch, what="upload without headers")
        assert eng.launch_shape(db_dev) == eng.launch_shape(db_hdr)
        assert eng.batch_kernel_name(db_dev) == eng.batch_kernel_name(db_hdr)
        (logs_a, res_a), (logs_b, res_b) = _merged_logs_and_rows(eng, db_hdr), _merged_logs_and_rows(eng, db_dev)
        assert logs_a.tobytes() == logs_b.tobytes()
        _assert_same_results(res_a, res_b)
        ok = [l for l, c in enumerate(LC.census_cases()) if c[4] != "headless"]
        assert (logs_a["status"][ok] == 0).all()
    finally:
        eng.free_batch(db_hdr)
        eng.free_batch(db_dev)


def test_census_of_appended_and_wrapped_batches(eng):
    """The same headers from the census of the grown logs (append: compute = 1 on base + more) and of caller-owned device columns (wrap_device)."""
    batch = LC.census_batch()
    want = wire.census(batch.log_off, batch.op_id, batch.action, batch.mark_type, batch.payload)
    nch = np.diff(batch.chg_off.astype(np.int64))
    head, tail = wire.split_batch(batch, np.where(np.arange(len(nch)) % 4 == 3, nch, nch * (np.arange(len(nch)) % 4) // 3))
    assert head.log_hdr is None and tail.log_hdr is None and 0 < head.n_ops < batch.n_ops
    db_head = eng.upload(head)
    db_grown = eng.append(db_head, tail)
    try:
        got = eng.download_batch(db_grown)
        _assert_headers(got.log_hdr, want, "append")
        LC.assert_batches_equal(got, batch, what="append")
    finally:
        eng.free_batch(db_grown)
        eng.free_batch(db_head)
    cols = LC.device_columns(batch)
    db = eng.wrap_device(batch.n_logs, batch.n_ops, {k: v.data_ptr() for k, v in cols.items()})
    try:
        got = eng.download_batch(db)
        _assert_headers(got.log_hdr, want, "wrap_device")
        LC.assert_batches_equal(got, LC.batch_without(batch, "chg_off", "chg_hdr", "chg_env"), what="wrap_device")
    finally:
        eng.free_batch(db)
    del cols


# ---- 3. the tiled upload read back ----
@pytest.mark.parametrize("n_logs,copies", LC.TILE_SHAPES, ids=["%dx%d_offsets%d" % (n, c, n * c + 1) for n, c in LC.TILE_SHAPES])
def test_tiled_upload_read_back(eng, n_logs, copies):
    """download_batch(upload(batch, copies)) == batch.tile(copies), column for column (log_off and chg_off from ptx_tile_offsets_kernel, whose thread
    i == n_logs * copies writes the end offset), with the encoder's headers tiled by copies and with headers computed on the device."""
    batch = wire.encode_docs(LC.small_docs(n_logs))
    want = batch.tile(copies)
    assert len(want.log_off) == n_logs * copies + 1
    for b in (batch, LC.batch_without(batch, "log_hdr")):
        db = eng.upload(b, copies=copies)
        try:
            assert eng.n_logs(db) == n_logs * copies and eng.n_ops(db) == want.n_ops and eng.n_changes(db) == int(want.chg_off[-1])
            got = eng.download_batch(db)
        finally:
            eng.free_batch(db)
        LC.assert_batches_equal(got, want, what="headers %s" % ("given" if b.log_hdr is not None else "computed"))


# ---- 4. append at its edges ----
def _append_case(name):
    """(base, more, whole or None): whole = one encode of the whole logs where the grown logs are valid documents (merged and compared by digest)."""
    if name == "rows":
        whole, base, more = LC.append_rows_case()
        return base, more, whole
    if name == "rows_nine_actors_stride_12":
        whole, base, more = LC.append_rows_case(extra_actors=6)
        assert abi.env_stride(whole.max_actors) == 12
        return base, more, whole
    if name.startswith("logs_"):
        whole, base, more = LC.append_logs_case(int(name[5:]))
        return base, more, whole
    whole, base, more = LC.append_rows_case()
    if name == "wide_on_base":
        return LC.with_wide_column(base, True), more, None
    if name == "wide_on_more":
        return base, LC.with_wide_column(more, True), None
    if name == "wide_on_both":
        return LC.with_wide_column(base, True), LC.with_wide_column(more, True), None
    if name == "zero_wide_on_base":
        return LC.with_wide_column(base, False), more, whole
    assert name == "empty_base_without_envelope"
    return LC.empty_base(whole.n_logs), whole, whole


APPEND_CASES = ["rows", "rows_nine_actors_stride_12"] + ["logs_%d" % n for n in LC.APPEND_LOG_COUNTS] + \
    ["wide_on_base", "wide_on_more", "wide_on_both", "zero_wide_on_base", "empty_base_without_envelope"]


@pytest.mark.parametrize("name", APPEND_CASES)
def test_append_columns(eng, name):
    """append (host `more`) and append_device (resident `more`): every column of the grown batch is helpers.concat_batches(base, more); the wide envelope column
    is there exactly when either side has it, zeros for the side without; the headers are the census of the grown logs; valid documents merge to the digests
    of the whole logs uploaded at once."""
    base, more, whole = _append_case(name)
    want = LC.appended(base, more)
    if whole is not None and name != "zero_wide_on_base":
        LC.assert_batches_equal(want, whole, what="reference")
    handles = []
    try:
        db_base = eng.upload(base)
        handles.append(db_base)
        db_more = eng.upload(more)
        handles.append(db_more)
        grown = [eng.append(db_base, more)]
        handles.append(grown[0])
        grown.append(eng.append_device(db_base, db_more))
        handles.append(grown[1])
        for how, h in zip(("append", "append_device"), grown):
            assert eng.n_logs(h) == want.n_logs and eng.n_ops(h) == want.n_ops and eng.n_changes(h) == int(want.chg_off[-1])
            LC.assert_batches_equal(eng.download_batch(h), want, what=how)
        if whole is not None:
            db_whole = eng.upload(whole)
            handles.append(db_whole)
            logs_w, res_w = _merged_logs_and_rows(eng, db_whole)
            for h in grown:
                logs_g, res_g = _merged_logs_and_rows(eng, h)
                assert np.array_equal(logs_g["status"], logs_w["status"]) and np.array_equal(logs_g["digest"], logs_w["digest"])
                for k in ("value_off", "span_off", "cint_off", "values", "spans", "cintervals"):
                    assert getattr(res_g, k).tobytes() == getattr(res_w, k).tobytes(), k
    finally:
        for h in handles:
            eng.free_batch(h)


@pytest.mark.parametrize("name", ["rows", "logs_257"])
def test_three_chained_appends(eng, name):
    """Four quarters of every log appended one after the other (append, append_device, append) against ONE encode of the whole logs."""
    _, _, whole = _append_case(name)
    parts = LC.split_in_four(whole)
    cur = eng.upload(parts[0])
    extra = []
    try:
        for k, p in enumerate(parts[1:]):
            if k == 1:
                dp = eng.upload(p)
                extra.append(dp)
                nxt = eng.append_device(cur, dp)
            else:
                nxt = eng.append(cur, p)
            eng.free_batch(cur)
            cur = nxt
        LC.assert_batches_equal(eng.download_batch(cur), whole, what="three appends")
        db_whole = eng.upload(whole)
        extra.append(db_whole)
        logs_w, _ = _merged_logs_and_rows(eng, db_whole)
        logs_g, _ = _merged_logs_and_rows(eng, cur)
        assert np.array_equal(logs_g["status"], logs_w["status"]) and np.array_equal(logs_g["digest"], logs_w["digest"])
    finally:
        eng.free_batch(cur)
        for h in extra:
            eng.free_batch(h)


# ---- 5. convergence counts and digest packing ----
@pytest.mark.parametrize("replicas", LC.CONVERGED_REPLICAS)
@pytest.mark.parametrize("n_docs", LC.CONVERGED_DOCS)
def test_count_converged_digests_at_wave_and_block_edges(eng, n_docs, replicas):
    """Synthetic digests: divergent documents at 0 / 63 / 64 / 255 / 256 / last (one word of one replica), failed documents ({0, 0}) that never count, a zero
    first word that does; the count is written, not added to what the counter held."""
    import torch

    count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    for variant in range(3):
        dg, _ = LC.synthetic_digests(n_docs, replicas, variant)
        want = LC.converged_count(dg, n_docs)
        t = torch.from_numpy(dg.view(np.int64).copy()).cuda()
        torch.cuda.synchronize()
        for _ in range(2):  # twice into the same counter
            eng.count_converged_digests(t.data_ptr(), n_docs * replicas, replicas, count.data_ptr())
            eng.sync()
            assert int(count.item()) == want, (variant, int(count.item()), want)


@pytest.mark.parametrize("copies", LC.CONVERGENCE_COPIES, ids=["%d_docs" % (8 * c) for c in LC.CONVERGENCE_COPIES])
def test_count_converged_on_merged_results(eng, copies):
    """Real results of a tiled base whose first and last documents lag and one of whose documents fails in every replica: as documents of three replicas and
    as documents of one (every log that merged), against numpy over download_logs and against what the emulation says of the base."""
    import torch

    batch = wire.encode_docs(LC.convergence_docs())
    db = eng.upload(batch, copies=copies)
    dr = eng.alloc_result(db)
    count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    try:
        eng.merge(db, dr)
        eng.sync()
        logs = eng.download_logs(dr, eng.n_logs(db))
        for replicas, per_copy in ((3, 5), (1, 21)):  # (tests/test_layout_cases.py: the emulation's count for one copy of the base)
            want = LC.converged_logs_count(logs, replicas)
            assert want == per_copy * copies
            for _ in range(2):
                eng.count_converged(dr, replicas, count.data_ptr())
                eng.sync()
                assert int(count.item()) == want, (replicas, int(count.item()), want)
    finally:
        eng.free_result(dr)
        eng.free_batch(db)


@pytest.mark.parametrize("first", [0, 3])
@pytest.mark.parametrize("count", LC.PACK_COUNTS)
def test_pack_digests(eng, count, first):
    import torch

    sentinel = 0x5A5A5A5A5A5A5A5A
    batch = wire.encode_docs(LC.convergence_docs())
    db = eng.upload(batch, copies=12)
    dr = eng.alloc_result(db)
    try:
        assert eng.n_logs(db) >= first + count
        eng.merge(db, dr)
        eng.sync()
        logs = eng.download_logs(dr, eng.n_logs(db))
        assert logs["digest"].any()
        dst = torch.full((2 * count + 8,), sentinel, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        eng.pack_digests(dr, first, count, dst.data_ptr())
        eng.sync()
        out = dst.cpu().numpy().view(np.uint64)
        assert np.array_equal(out[:2 * count].reshape(-1, 2), logs["digest"][first:first + count])
        assert (out[2 * count:] == np.uint64(sentinel)).all()  # nothing behind 2 * count touched
    finally:
        eng.free_result(dr)
        eng.free_batch(db)


# ---- 6. patch packing at the buffer's edges ----
def _streams(eng, batch):
    db = eng.upload(batch)
    dr = eng.alloc_result(db)
    try:
        eng.merge(db, dr)
        eng.sync()
        return eng.replay_patches(db, dr)
    finally:
        eng.free_result(dr)
        eng.free_batch(db)


@pytest.fixture(scope="module")
def whole_stream(eng):
    """The streams of the patch-pack case packed in one go, checked against the reference-made fixture's patches."""
    assert "PTX_REPLAY_PACK_RECORDS" not in os.environ and "PTX_REPLAY_NO_ARENA" not in os.environ
    batch, want = LC.patch_pack_case()
    pat = _streams(eng, batch)
    return batch, want, pat


def _check_streams(batch, want, pat):
    last = batch.n_logs - 1
    for log in (1, last - 1):  # the failing logs: no records
        assert int(pat.logs["status"][log]) != 0 and int(pat.patch_off[log + 1]) == int(pat.patch_off[log])
    for log in (0, last):  # the empty logs
        assert int(pat.logs["status"][log]) == 0 and int(pat.logs["n_patches"][log]) == 0 and int(pat.patch_off[log + 1]) == int(pat.patch_off[log])
    ok = pat.logs["status"] == 0
    assert np.array_equal(np.diff(pat.patch_off.astype(np.int64)), np.where(ok, pat.logs["n_patches"], 0).astype(np.int64))
    assert len(pat.patches) == int(pat.patch_off[-1])
    for log, patches in want.items():
        got, exp = H.norm_patches(wire.decode_patches(batch, pat, log)), H.norm_patches(patches)
        assert len(got) == len(exp), "log %d: %d patches, expected %d" % (log, len(got), len(exp))
        for i, (x, y) in enumerate(zip(got, exp)):
            assert x == y, "log %d patch %d: %r != %r" % (log, i, x, y)


def test_patch_streams_packed_in_one_go(whole_stream):
    _check_streams(*whole_stream)


@pytest.mark.parametrize("cap", ["longest", "longest_plus_1", "total_minus_1", "total"])
def test_patch_pack_with_a_short_packed_copy(eng, whole_stream, monkeypatch, cap):
    """PTX_REPLAY_PACK_RECORDS: the packed copy holds as many records as the longest log's stream, one more, the whole stream less one, the whole stream — the
    ranges of logs packed per step end on other logs each time; offsets and records must be those of the one-go stream, byte for byte."""
    batch, want, whole = whole_stream
    per_log = np.diff(whole.patch_off.astype(np.int64))
    longest, total = int(per_log.max()), int(whole.patch_off[-1])
    assert 0 < longest < total - 1
    records = {"longest": longest, "longest_plus_1": longest + 1, "total_minus_1": total - 1, "total": total}[cap]
    monkeypatch.setenv("PTX_REPLAY_PACK_RECORDS", str(records))
    pat = _streams(eng, batch)
    assert pat.launches == whole.launches
    assert np.array_equal(pat.patch_off, whole.patch_off) and pat.logs.tobytes() == whole.logs.tobytes()
    assert pat.patches.tobytes() == whole.patches.tobytes()
    _check_streams(batch, want, pat)
