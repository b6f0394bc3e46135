"""The four lean builds of the merge kernel (ptx_merge_kernel_lean64 / 128 / 192 / 256: ptx_merge_log<0, T, false, true>, chosen for contexts created with
PTX_FLAG_NO_ELEM_RANK) against the oracle, at the row counts that select each of them and at the step, tile and alignment edges only these builds have.

Every case: an engine with FLAG_NO_ELEM_RANK and one with FLAG_NO_ELEM_RANK | FLAG_NO_ADMISSION; the kernel's name and the workgroup size asserted against
the literals of the case tables below; EVERY log compared with the oracle by helpers.check_log (status, decoded spans, raw value / span / comment-interval
rows, digest).  Expected documents come from the in-repo oracle (helpers.oracle_gen(impl="oracle"), one generation shared by both engines and by every case
that names the same document) or from a committed reference-made fixture — never from another build of the kernel.  Every batch has fewer than 64 logs, so
the host cannot split it into launch groups (the second launch of a split batch is the general `_rest` build).

  A  shapes the library chooses itself: 64 threads up to 512 rows, 128 up to 2 048, 192 up to 4 608 (256 where the log's window exceeds 160 KB / 7), 256 up to
     12 288.  A generated log has ops + 1 rows (the first is the makeList).
  B  every lean build (forced workgroup size) across the regimes of the visible length V the tail phases branch on.
  C  a head-row log (rows = k whole steps + 1: every load of the row pass moves one row on) at every alignment of its first row in the batch's columns, as the
     first and as the last log.

What the window rule keeps out of a lean build (the host takes lean64 / 128 / 192 only where more than 24 waves share a CU: a window of at most 6 400 / 11 520 /
17 920 bytes after rounding to the CU's 1 280-byte granule; lean256 whatever the window):
  * lean64 never sees a document with mark ops and more than 128 inserted characters: ptx_lds_need budgets the 512-character tile (a tree of 4 096 bytes, its
    attributes 2 052, its bits 144) as soon as n_ins > 128, and a recycled element region large enough to hold them is itself more than 6 400 bytes.  So V > 128
    with marks — the "mid" form, the lean-only `!kLongDocs` path with four types, one and several tiles, comment-only documents of that length — runs in
    the general build at 64 threads, natural or forced.  Without mark ops the bound is 520 inserts (6 400 bytes with no delete and one actor): V > 512 is
    reached there by an insert-only log.
  * lean128 never sees V > 1 024: 1 025 inserts need 12 256 bytes even without a single mark op or delete.
  * lean192 never takes the "mid" form (compiled out), and V > 1 024 reaches it only for documents of few deletes (window <= 17 920 bytes).
The pairs of section B that therefore assert the general build's name are marked in B_KERNEL."""
import json
import os

import numpy as np
import pytest

import helpers as H
from peritext_amd import abi, wire

pytestmark = pytest.mark.gpu

LEAN_FLAGS = (abi.FLAG_NO_ELEM_RANK, abi.FLAG_NO_ELEM_RANK | abi.FLAG_NO_ADMISSION)


def _gen(kw):
    """The oracle's documents for one table entry (lru_cached by helpers.oracle_gen: a table entry is generated once per run, whichever cases use it)."""
    assert H.have_node(), "these cases need node, the oracle's runtime: a skipped case would hide exactly what this file exists to show"
    if "fixture" in kw:
        with open(os.path.join(H.GOLDEN, kw["fixture"])) as f:
            g = json.load(f)
        assert g.get("impl", "ref") == "ref"
        return g
    return H.oracle_gen(impl="oracle", **kw)


def _rows(batch):
    return [int(x) for x in np.diff(batch.log_off.astype(np.int64))]


def _types(batch):
    """mark types with ops, per log (strong, em, comment, link as the header counts them)"""
    return [int((h["n_mark"] > 0).sum()) for h in batch.log_hdr]


def _run(docs, expected, kernel, threads, force=0):
    """Merge `docs` under both lean contexts; the kernel's name and workgroup size as given; every log against `expected` (flat, in log order)."""
    from peritext_amd.engine import Engine

    batch = wire.encode_docs(docs)
    assert batch.n_logs == len(expected) and batch.n_logs < 64
    for flags in LEAN_FLAGS:
        with Engine(0, flags=flags) as e:
            if force:
                e.set_launch_shape(force, 0)
            db = e.upload(batch)
            dr = e.alloc_result(db)
            try:
                assert e.batch_kernel_name(db) == kernel
                assert e.launch_shape(db)[0] == threads
                e.merge(db, dr)
                res = e.download(db, dr)
            finally:
                e.free_result(dr)
                e.free_batch(db)
        for log, exp in enumerate(expected):
            H.check_log(batch, res, log, exp)
    return batch


def _docs(gen):
    return [d["logs"] for d in gen["docs"]], [e for d in gen["docs"] for e in d["expected"]]


# ---- the documents (generator parameters; rows N, visible characters V and mark types were taken from the oracle's output on the CPU) ----
C2_255 = dict(config="config2", docs=4, seed=1, ops=255)
C2_256 = dict(config="config2", docs=4, seed=1, ops=256)
C2_260 = dict(config="config2", docs=4, seed=1, ops=260)
C2_511 = dict(config="config2", docs=4, seed=1, ops=511)
C2_512 = dict(config="config2", docs=4, seed=1, ops=512)
RICH_200 = dict(config="rich", docs=1, seed=13, ops=200)
RICH_256_HEAD = dict(config="rich", docs=1, seed=3, ops=256, mix=(50, 20, 18, 12))
RICH_300 = dict(config="rich", docs=1, seed=13, ops=300)
RICH_512 = dict(config="rich", docs=1, seed=3, ops=512)
C3_1024 = dict(config="config3", docs=2, seed=2, ops=1024)
C3_2047 = dict(config="config3", docs=1, seed=12, ops=2047)
C3_2048 = dict(config="config3", docs=1, seed=12, ops=2048)
RICH_1024 = dict(config="rich", docs=1, seed=3, ops=1024)
RICH_1200 = dict(config="rich", docs=1, seed=13, ops=1200)
RICH_600_STRONG_LINK = dict(config="rich", docs=1, seed=13, ops=600, marks=("strong", "link"))
C4_FULL = dict(config="config4", docs=1, seed=5)
C4_4607 = dict(config="config4", docs=1, seed=15, ops=4607, replicas=1)
C4_2100 = dict(config="config4", docs=1, seed=1, ops=2100)
C5_FIXTURE = dict(fixture="ptxgen_config5_8192.json")
C5_4608 = dict(config="config5", docs=1, seed=14, ops=4608)
C5_4609 = dict(config="config5", docs=1, seed=14, ops=4609)
RICH4K = dict(config="rich4k", docs=1, seed=4)
C5_TEXT = dict(config="config5", docs=1, seed=14, ops=4700, mix=(55, 10, 20, 15))
RICH_1500_FEW_DELETES = dict(config="rich", docs=1, seed=13, ops=1500, mix=(78, 4, 11, 7))
RICH_2600 = dict(config="rich", docs=1, seed=13, ops=2600)
TEXT_900 = dict(config="rich", docs=1, seed=13, ops=900, mix=(90, 10, 0, 0), replicas=1)
INSERTS_516 = dict(config="rich", docs=1, seed=13, ops=516, mix=(100, 0, 0, 0), replicas=1)
COMMENTS_1024 = dict(config="rich", docs=1, seed=1, ops=1024, mix=(45, 15, 25, 15), marks=("comment",))


# ---- A: the shapes the library chooses itself ----
# (id, kernel, threads, document, rows of every log, V of every log within [lo, hi], mark types with ops in every log)
A_CASES = [
    # one wave.  256 rows: one whole step, no head row; 257: head row + one whole step; 261: a ragged tail; 512: two whole steps, no head row
    ("lean64-config2-N256", "ptx_merge_kernel_lean64", 64, C2_255, 256, (1, 128), 0),
    ("lean64-config2-N257-head-row", "ptx_merge_kernel_lean64", 64, C2_256, 257, (1, 128), 0),
    ("lean64-config2-N261-ragged", "ptx_merge_kernel_lean64", 64, C2_260, 261, (1, 128), 0),
    ("lean64-config2-N512-two-steps", "ptx_merge_kernel_lean64", 64, C2_511, 512, (100, 256), 0),
    # all four mark types in the four-tree form (V <= 128), one-flush digest; the second with the head row
    ("lean64-rich-N201-four-trees", "ptx_merge_kernel_lean64", 64, RICH_200, 201, (65, 128), 4),
    ("lean64-rich-N257-head-row-four-trees", "ptx_merge_kernel_lean64", 64, RICH_256_HEAD, 257, (33, 128), 4),
    # two waves.  513 rows: head row + exactly one whole two-wave step, without marks and with all four types at 128 < V <= 256 (four types: not "mid")
    ("lean128-config2-N513-head-row", "ptx_merge_kernel_lean128", 128, C2_512, 513, (100, 256), 0),
    ("lean128-rich-N513-head-row-four-types", "ptx_merge_kernel_lean128", 128, RICH_512, 513, (129, 256), 4),
    ("lean128-config3-N1025-mid", "ptx_merge_kernel_lean128", 128, C3_1024, 1025, (129, 256), 2),  # strong and em only: the mid form; head row + two steps
    ("lean128-config3-N2048-last-rows", "ptx_merge_kernel_lean128", 128, C3_2047, 2048, (257, 512), 2),  # one tile
    ("lean128-rich-N1025-one-tile", "ptx_merge_kernel_lean128", 128, RICH_1024, 1025, (257, 512), 4),
    ("lean128-rich-N1201-two-tiles", "ptx_merge_kernel_lean128", 128, RICH_1200, 1201, (513, 1024), 4),  # more than one tile: the park words are cached
    ("lean128-rich-N601-strong-link", "ptx_merge_kernel_lean128", 128, RICH_600_STRONG_LINK, 601, (257, 512), 2),
    # three waves
    ("lean192-config3-N2049-first-rows", "ptx_merge_kernel_lean192", 192, C3_2048, 2049, (257, 512), 2),
    ("lean192-config4-N2101", "ptx_merge_kernel_lean192", 192, C4_2100, 2101, (1, 128), 4),
    ("lean192-config4-N4097-headline", "ptx_merge_kernel_lean192", 192, C4_FULL, 4097, (1, 128), 4),
    ("lean192-config4-N4608-last-rows", "ptx_merge_kernel_lean192", 192, C4_4607, 4608, (1, 128), 4),
    # four waves
    ("lean256-config5-N4609-first-rows", "ptx_merge_kernel_lean256", 256, C5_4608, 4609, (1, 128), 2),
    ("lean256-config5-N4610", "ptx_merge_kernel_lean256", 256, C5_4609, 4610, (1, 128), 2),
    ("lean256-config5-N8193-reference-made", "ptx_merge_kernel_lean256", 256, C5_FIXTURE, 8193, (1, 128), 2),
    ("lean256-rich4k-N4097-by-window", "ptx_merge_kernel_lean256", 256, RICH4K, 4097, (1025, 4096), 4),  # chosen through the LDS rule; double-size tiles
    ("lean256-config5-N4701-link-comment-text", "ptx_merge_kernel_lean256", 256, C5_TEXT, 4701, (1025, 4700), 2),
]


@pytest.mark.parametrize("kernel,threads,doc,rows,v,types", [pytest.param(*c[1:], id=c[0]) for c in A_CASES])
def test_shapes_the_library_chooses(kernel, threads, doc, rows, v, types):
    docs, expected = _docs(_gen(doc))
    batch = _run(docs, expected, kernel, threads)
    # the regime, from the oracle's own output: a later change of the generator must not empty the case
    assert _rows(batch) == [rows] * batch.n_logs
    assert all(v[0] <= len(e["text"]) <= v[1] for e in expected), [len(e["text"]) for e in expected]
    assert _types(batch) == [types] * batch.n_logs


def test_many_spans_of_link_and_comment_in_the_four_wave_build():
    """What "lean256-config5-N4701-link-comment-text" is there for: hundreds of spans of the two attribute-carrying types over thousands of characters."""
    _, expected = _docs(_gen(C5_TEXT))
    assert len(expected[0]["spans"]) > 300 and len(expected[0]["text"]) > 2048


# ---- B: every lean build across the regimes of the visible length ----
# regime -> (document, V of every log within [lo, hi], mark types with ops in every log)
B_REGIMES = {
    "v-le-128": (RICH_200, (65, 128), 4),
    "v-129-256-two-types": (C3_1024, (129, 256), 2),
    "v-129-256-four-types": (RICH_300, (129, 256), 4),
    "v-257-512": (RICH_1024, (257, 512), 4),
    "v-513-1024": (RICH_1200, (513, 1024), 4),
    "v-gt-1024-few-deletes": (RICH_1500_FEW_DELETES, (1025, 1500), 4),
    "v-gt-1024": (RICH_2600, (1025, 2600), 4),
    "no-marks-v-gt-512": (TEXT_900, (513, 900), 0),
    "no-marks-v-gt-512-inserts-only": (INSERTS_516, (513, 520), 0),
    "comments-only": (COMMENTS_1024, (257, 512), 1),
}
G, L64, L128, L192, L256 = "ptx_merge_kernel", "ptx_merge_kernel_lean64", "ptx_merge_kernel_lean128", "ptx_merge_kernel_lean192", "ptx_merge_kernel_lean256"
# regime -> the kernel at 64, 128, 192 and 256 threads.  G: the window rule (module docstring) sends the pair to the general build
B_KERNEL = {
    "v-le-128": (L64, L128, L192, L256),
    "v-129-256-two-types": (G, L128, L192, L256),  # 64: marks and more than 128 inserts
    "v-129-256-four-types": (G, L128, L192, L256),  # 64: the same
    "v-257-512": (G, L128, L192, L256),  # 64: the same
    "v-513-1024": (G, L128, L192, L256),  # 64: the same
    "v-gt-1024-few-deletes": (G, G, L192, L256),  # 64: the same; 128: more than 1 024 inserts
    "v-gt-1024": (G, G, G, L256),  # (a tenth of the ops deletes: 19 872 bytes, beyond the three-wave build's 17 920 too)
    "no-marks-v-gt-512": (G, L128, L192, L256),  # 64: more than 520 inserts
    "no-marks-v-gt-512-inserts-only": (L64, L128, L192, L256),
    "comments-only": (G, L128, L192, L256),  # 64: marks and more than 128 inserts
}
B_THREADS = (64, 128, 192, 256)


@pytest.mark.parametrize("regime", list(B_REGIMES))
@pytest.mark.parametrize("threads", B_THREADS)
def test_every_lean_build_across_the_visible_length_regimes(threads, regime):
    doc, v, types = B_REGIMES[regime]
    docs, expected = _docs(_gen(doc))
    batch = _run(docs, expected, B_KERNEL[regime][B_THREADS.index(threads)], threads, force=threads)
    assert all(v[0] <= len(e["text"]) <= v[1] for e in expected), [len(e["text"]) for e in expected]
    assert _types(batch) == [types] * batch.n_logs
    if regime == "comments-only":
        assert all(len(e["spans"]) > 100 for e in expected)
    if regime.startswith("no-marks"):
        assert all(len(e["spans"]) == 1 for e in expected)


def test_every_regime_runs_in_every_lean_build_that_can_reach_it():
    """The table the cases above assert, against the coverage this file promises (each entry of B_KERNEL is a case of its own that asserts the name: with the
    whole file passing, every pair listed here ran in that build).  What is absent: lean64 beyond 128 characters with marks and beyond 520 without, lean128
    beyond 1 024 characters — the window rule, see the module docstring."""
    ran = {r: tuple(k for k in names if k != "ptx_merge_kernel") for r, names in B_KERNEL.items()}
    by_regime = {}
    for r, names in ran.items():
        by_regime.setdefault(r.replace("-few-deletes", "").replace("-inserts-only", ""), set()).update(names)
    assert by_regime == {
        "v-le-128": {"ptx_merge_kernel_lean64", "ptx_merge_kernel_lean128", "ptx_merge_kernel_lean192", "ptx_merge_kernel_lean256"},
        "v-129-256-two-types": {"ptx_merge_kernel_lean128", "ptx_merge_kernel_lean192", "ptx_merge_kernel_lean256"},
        "v-129-256-four-types": {"ptx_merge_kernel_lean128", "ptx_merge_kernel_lean192", "ptx_merge_kernel_lean256"},
        "v-257-512": {"ptx_merge_kernel_lean128", "ptx_merge_kernel_lean192", "ptx_merge_kernel_lean256"},
        "v-513-1024": {"ptx_merge_kernel_lean128", "ptx_merge_kernel_lean192", "ptx_merge_kernel_lean256"},
        "v-gt-1024": {"ptx_merge_kernel_lean192", "ptx_merge_kernel_lean256"},
        "no-marks-v-gt-512": {"ptx_merge_kernel_lean64", "ptx_merge_kernel_lean128", "ptx_merge_kernel_lean192", "ptx_merge_kernel_lean256"},
        "comments-only": {"ptx_merge_kernel_lean128", "ptx_merge_kernel_lean192", "ptx_merge_kernel_lean256"},
    }
    assert set(B_KERNEL) == set(B_REGIMES) and all(len(n) == len(B_THREADS) for n in B_KERNEL.values())


# ---- C: where a head-row log stands in the batch ----
# the row pass of a head-row log starts at its SECOND row and reads the class bytes of four rows as one (unaligned) dword: every residue of the log's first row
# modulo 4, the log first in the batch and last (the shifted, clamped loads end where the columns end)
C_TARGETS = {
    "lean64-N257": ("ptx_merge_kernel_lean64", 64, RICH_256_HEAD, 257),
    "lean128-N513": ("ptx_merge_kernel_lean128", 128, RICH_512, 513),
    "lean256-N4097": ("ptx_merge_kernel_lean256", 256, RICH4K, 4097),
}
# one small single-log document of 100 + r rows before the target moves its first row to residue r (smaller than every target in rows and in LDS: the batch
# keeps the target's launch shape, which the case asserts)
C_FILLERS = {r: dict(config="config2", docs=1, seed=21 + r, ops=99 + r) for r in range(4)}


@pytest.mark.parametrize("place", ["first", "last-residue-0", "last-residue-1", "last-residue-2", "last-residue-3"])
@pytest.mark.parametrize("target", list(C_TARGETS))
def test_head_row_log_at_every_alignment_in_the_batch(target, place):
    kernel, threads, doc, rows = C_TARGETS[target]
    t_docs, t_exp = _docs(_gen(doc))
    residue = 1 if place == "first" else int(place[-1])
    f_docs, f_exp = _docs(_gen(C_FILLERS[residue]))
    assert len(f_exp) == 1
    if place == "first":
        batch = _run(t_docs + f_docs, t_exp + f_exp, kernel, threads)
        first = 0
    else:
        batch = _run(f_docs + t_docs, f_exp + t_exp, kernel, threads)
        first = 1
        assert _rows(batch)[0] == 100 + residue
        assert int(batch.log_off[-1]) == batch.n_ops  # the target's last log ends the columns
    assert int(batch.log_off[first]) % 4 == (0 if place == "first" else residue)
    assert _rows(batch)[first:first + len(t_exp)] == [rows] * len(t_exp)
    assert int(batch.action[int(batch.log_off[first])]) == abi.ACT_MAKELIST  # the head row itself
