"""The patch replay at its word, chunk, tile and extent edges in every build the library launches: the batches of tests/replay_edge_cases.py (expected streams:
the oracle's, one run of about 14 s for the module) through ptx_merge and ptx_replay_patches on the GPU.  tests/test_emu_replay_edges.py runs the same batches
through the CPU emulation, which compiles the walk for any workgroup size and serialises its lanes; the four kernels as hipcc builds them — the waits of the
coherent accessors, the LDS atomics, the one-wave scans — run only here.

Four contexts, one Engine each: flags 0 (ptx_replay_kernel up to a working set of 5 632 bytes per log, ptx_replay_kernel_gwin above it); PTX_FLAG_REPLAY_LDS_ONLY
(ptx_replay_kernel whatever the working set; what does not fit one CU's LDS that way goes to the HBM-state kernel); PTX_FLAG_REPLAY_HBM_STATE (every log through
ptx_replay_kernel_hbm); and flags 0 with typed_log(32 767) appended to the batch (ptx_replay_kernel_wide for all of it).  Which build a batch takes follows from
the flags and the literal need table replay_edge_cases.NEED (held to ptx_replay_lds_need_hdr by the emulation file: nothing here loads an emulation library);
the library reports the logs the HBM-state kernel took (hbm_logs) and the launches, both asserted.

Wall time on an MI355X: the file 43 s, 6 of them the oracle's one run (inside the first case); a case of a small batch 0.01 to 0.05 s, 1 s with the ballast
(encoding and uploading 32 767 rows); the four 16 K-element documents 1.5 s per context, 2.4 s with the ballast; the tails 0.01 s per context; the superblock
document of family K (131 202 chars) 3.5 s, most of it the encoding and the decoding of 131 000 records in Python."""
import numpy as np
import pytest

import helpers as H
import replay_edge_cases as RC
from peritext_amd import abi, wire

pytestmark = pytest.mark.gpu

CONTEXTS = {"default": 0, "lds-only": abi.FLAG_REPLAY_LDS_ONLY, "hbm": abi.FLAG_REPLAY_HBM_STATE, "ballast": 0}
TWO_LAUNCHES = ("X-burst", "X-burst-then-quiet", "X")  # a log of these loses records in the first launch: once more with exact capacities


@pytest.fixture(scope="module")
def engines():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    assert H.have_node(), "these cases need node, the oracle's runtime: a skipped case would hide exactly what this file exists to show"
    from peritext_amd.engine import Engine

    made = {}

    def get(context):
        if context not in made:
            made[context] = Engine(0, flags=CONTEXTS[context])  # raises if libperitext_hip.so is missing or no gfx950 is visible: no fallback
        return made[context]

    yield get
    for e in made.values():
        e.close()


def _replay(e, batch, first_row=None):
    """merge, then the streams (whole, or from first_row on)"""
    db = e.upload(batch)
    dr = e.alloc_result(db)
    try:
        e.merge(db, dr)
        status = e.download_logs(dr, batch.n_logs)["status"]
        assert not status.any(), status
        return e.replay_patches(db, dr, first_row=first_row)
    finally:
        e.free_result(dr)
        e.free_batch(db)


def _in_context(context, b):
    """(the wire.Batch the context replays, the log of the ballast or None)"""
    return RC.with_ballast(b) if context == "ballast" else (b.batch, None)


def _check_context(context, b, batch, at, pat, launches):
    hbm = {"ptx_replay_kernel_hbm": b.batch.n_logs}.get(RC.build_of(b.name, context), 0)
    assert pat.hbm_logs == hbm, (b.name, context, pat.hbm_logs)
    assert pat.launches == launches, (b.name, context, pat.launches)
    if at is not None:  # the ballast's own stream: makeList, then insert k at index k
        assert int(pat.logs["status"][at]) == 0 and H.norm_patches(wire.decode_patches(batch, pat, at)) == RC.typed_stream(RC.K_BALLAST)


@pytest.mark.parametrize("name", RC.batch_names())
@pytest.mark.parametrize("context", list(CONTEXTS))
def test_every_batch_in_every_build(engines, context, name):
    b = RC.batch(name)
    batch, at = _in_context(context, b)
    pat = _replay(engines(context), batch)
    _check_context(context, b, batch, at, pat, 2 if name in TWO_LAUNCHES else 1)
    RC.check_batch(RC.rebatched(b, batch), pat)


@pytest.mark.parametrize("context", list(CONTEXTS))
def test_tails_are_the_oracles_records_of_the_rows_asked_for(engines, context):
    """ptx_replay_patches_from on the 97-row log of one op per change: exactly what the oracle produces after a prefix of first_row changes"""
    b = RC.batch("R-tail")
    batch, at = _in_context(context, b)
    rows = np.diff(batch.log_off.astype(np.int64))
    for first in RC.R_FIRST:
        fr = rows.copy()  # (the ballast: nothing asked for)
        fr[0] = first
        pat = _replay(engines(context), batch, first_row=fr)
        assert int(pat.logs["status"][0]) == 0 and (at is None or int(pat.logs["n_patches"][at]) == 0)
        got, want = H.norm_patches(wire.decode_patches(batch, pat, 0)), H.norm_patches(RC.tail_expected(first))
        assert int(pat.logs["n_patches"][0]) == len(pat.of_log(0)) and got == want, (context, first, len(got), len(want))


@pytest.mark.parametrize("context", ["default", "hbm"])
def test_the_capacity_logs_when_there_is_no_arena(engines, context, monkeypatch):
    """PTX_REPLAY_NO_ARENA=1 plays a device too full for the overflow arena: the logs that outgrow 2 N + 16 records take the second launch"""
    b = RC.batch("X")
    monkeypatch.setenv("PTX_REPLAY_NO_ARENA", "1")
    pat = _replay(engines(context), b.batch)
    assert pat.launches == 2
    RC.check_batch(b, pat)


def test_a_document_of_more_than_one_superblock(engines):
    """Family K, default flags: 131 202 typed chars, deletes and inserts on both sides of the superblock edge of `present` (element 131 072), a strong mark
    across it.  Its replay state needs 262 472 bytes of LDS even in the form with the tables in global memory — 8 bytes per 32 elements (4 102 words) + 28 per 32
    slots (8 202 words) — against the 163 840 of one CU, so the HBM-state kernel takes it; the stream is the list model's (replay_edge_cases.k_script, validated against the oracle on a miniature)."""
    RC.suite()
    log, want = RC.k_super()
    batch = wire.encode_docs([[log]])
    n = RC.K_SUPER_N
    need = 8 * ((n >> 5) + 2) + 28 * (((2 * n + 2) >> 5) + 2)  # `present` + defined, mb, cw, cnt of ptx_replay_lds_need (the chunk buffers and the header aside)
    assert need > RC.LDS_CU
    pat = _replay(engines("default"), batch)
    assert pat.hbm_logs == 1 and pat.launches == 1 and int(pat.logs["status"][0]) == 0 and int(pat.logs["n_patches"][0]) == len(want)
    assert H.norm_patches(wire.decode_patches(batch, pat, 0)) == H.norm_patches(want)
