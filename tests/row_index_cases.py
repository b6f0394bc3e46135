"""Logs for the row index of a resident batch (merge_core.h ptx_row_index_off), shared by tests/test_emu_row_index.py and its GPU twin
tests/test_gpu_row_index.py: hand-sized replica logs (n inserts, D deletes, K mark ops, one makeList row: N = 1 + n + D + K rows) at the edges of the indexed
row pass, each with the oracle's answer, and the logs that fail one of P1's checks."""
import functools

import helpers as H
from peritext_amd import wire

# (n, D, K): inserts 0, 1, 3, 4, 5 (less than, exactly and more than one 16-byte load); one below, at and one above a full 16-byte step of a team of 64, 128 and
# 192 threads (256, 512, 768 words); mark ops 0, 31, 32, 33 (the words of the add / remove bitmap); no deletes; 257 and 1 025 rows (k full steps of the full row
# pass plus one row: its leader takes the makeList by hand)
SHAPES = (
    (0, 0, 0), (1, 0, 0), (3, 0, 31), (4, 1, 32), (5, 0, 33),
    (255, 3, 0), (256, 0, 5), (257, 9, 31),
    (511, 0, 32), (512, 7, 33), (513, 0, 0),
    (767, 5, 10), (768, 0, 0), (769, 11, 40),
    (200, 20, 36), (700, 100, 224),
    (256, 0, 0), (257, 2, 0),
)
# what the one-wave lean build takes: at most 512 rows, and a window of at most 160 KiB / 25 (more than 24 logs per CU) — a log of more than a few elements that
# has mark ops asks for the four resident LWW trees on top, 7.6 KB and more
SHORT = tuple(i for i, (n, D, K) in enumerate(SHAPES) if 1 + n + D + K <= 512 and (n <= 5 or K == 0))


@functools.lru_cache(maxsize=None)
def shapes(which=None):
    """-> (Batch of one log per shape, [the oracle's {spans, text} per log], [(n, D, K)])."""
    sel = [SHAPES[i] for i in (which if which is not None else range(len(SHAPES)))]
    logs = [H.synthetic_marks_log(n, K, 4100 + 7 * i, n_deletes=D, max_span=12) for i, (n, D, K) in enumerate(sel)]
    exp = H.oracle_apply([[l] for l in logs], no_patches=True)
    batch = wire.encode_docs([[l] for l in logs])
    batch.log_hdr = None  # (the library takes the census)
    for l, (n, D, K) in enumerate(sel):
        assert int(batch.log_off[l + 1] - batch.log_off[l]) == 1 + n + D + K
        assert not exp[l][0].get("error"), exp[l][0].get("error")
    return batch, [e[0] for e in exp], sel
