"""The HBM-state patch replay (peritext_amd/csrc/replay_hbm_core.h: the replay state of a log in a slice of global scratch instead of the LDS) compiled with
-DPTX_EMU (tests/emu/emu_replay_hbm.cc, test tooling only): the reference-made fixtures, the reference's test cases and traces through the oracle, tail
streams, overflow extents, byte-equality with the LDS build's streams, and two documents beyond what one CU's LDS holds, record for record against the
oracle.  test_gpu_replay_hbm.py repeats the comparisons through ptx_replay_patches on a real MI355X."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import replay_hbm_docs as D
from peritext_amd import abi, wire

pytestmark = pytest.mark.skipif(not (os.path.exists(H.EMU_LIB) and os.path.exists(D.EMU_HBM_LIB)), reason="tests/emu/*.so not built (run __graft_entry__.build())")


def _load(name):
    with open(os.path.join(H.GOLDEN, name)) as f:
        return json.load(f)


def _same(a, b):
    return np.array_equal(a.logs, b.logs) and all(np.array_equal(D.stream(a, l), D.stream(b, l)) for l in range(len(a.logs)))


@pytest.mark.parametrize("name", ["patches_mini.json", "patches_rich_300.json"])
@pytest.mark.parametrize("reverse", [0, 1, 2])
def test_golden_patch_streams_with_the_state_in_scratch(name, reverse):
    """Fixtures produced by the reference itself, every log forced through the HBM-state replay: every patch of every replica log, in order, deep-equal."""
    g = _load(name)
    assert g["impl"] == "ref"
    batch = wire.encode_docs([d["logs"] for d in g["docs"]])
    res = H.emu_merge(batch, lds_bytes=160 * 1024, reverse=reverse)
    pat = D.emu_replay_hbm(batch, res, reverse=reverse)
    assert H.check_patch_streams(batch, pat, [d["expected"] for d in g["docs"]]) == batch.n_logs


def test_kat_and_trace_patch_streams():
    """The reference's 46 test cases and 9 traces: the stream of every replica log == the oracle's."""
    if not H.have_node():
        pytest.skip("node not installed")
    cases = H.load_kat()
    docs = [[r["log"] for r in c["replicas"]] for c in cases] + [t["logs"] for t in _load("reference_traces.json")]
    batch = wire.encode_docs(docs)
    expected = H.oracle_apply(docs, patches=True)
    assert all("error" not in e for exp in expected for e in exp), "no KAT / trace log fails"
    for reverse in (0, 1):
        res = H.emu_merge(batch, reverse=reverse)
        assert H.check_patch_streams(batch, D.emu_replay_hbm(batch, res, reverse=reverse), expected) == batch.n_logs


def test_streams_are_byte_equal_to_the_lds_build():
    """The same records in the same order as replay_core.h's build with the tables in global memory."""
    g = _load("patches_rich_300.json")
    batch = wire.encode_docs([d["logs"] for d in g["docs"]])
    res = H.emu_merge(batch, lds_bytes=160 * 1024)
    assert _same(D.emu_replay_hbm(batch, res), H.emu_replay(batch, res, gwin=True))


def test_tail_streams_are_the_suffix_of_the_whole_stream():
    """first_row: the records of the rows from first_row[l] on are exactly the tail of the log's whole stream, whatever the cut."""
    g = _load("patches_rich_300.json")
    batch = wire.encode_docs([d["logs"] for d in g["docs"]])
    res = H.emu_merge(batch, lds_bytes=160 * 1024)
    whole = D.emu_replay_hbm(batch, res)
    sizes = np.diff(batch.log_off.astype(np.int64))
    rng = np.random.default_rng(5)
    for cut in ("zero", "random", "last", "past"):
        first = {"zero": np.zeros_like(sizes), "random": rng.integers(0, np.maximum(sizes, 1)), "last": np.maximum(sizes - 1, 0), "past": sizes + 3}[cut]
        tail = D.emu_replay_hbm(batch, res, first_row=first)
        for log in range(batch.n_logs):
            a = D.stream(whole, log)
            assert tail.logs["status"][log] == whole.logs["status"][log]
            assert np.array_equal(D.stream(tail, log), a[a["row"] >= first[log]]), (cut, log, int(first[log]))


def test_overflow_extents_give_the_same_streams():
    """40 records of capacity per log: every log of the fixture continues in an overflow extent and the packed streams equal the ones replayed into ample room;
    with a starved arena the logs that got no extent report PTX_ERR_CAPACITY with exact counts; a log that starts quietly takes a second extent."""
    g = _load("patches_rich_300.json")
    batch = wire.encode_docs([d["logs"] for d in g["docs"]])
    res = H.emu_merge(batch)
    ref = D.emu_replay_hbm(batch, res)
    pat, ext = D.emu_replay_hbm_with_arena(batch, res, cap=40, arena=200000)
    assert np.all(ext[:batch.n_logs, 0] != np.uint64(D.NONE64)) and np.all(pat.logs["status"] == 0)
    assert _same(pat, ref)
    assert H.check_patch_streams(batch, pat, [d["expected"] for d in g["docs"]]) == batch.n_logs
    starved, ext2 = D.emu_replay_hbm_with_arena(batch, res, cap=40, arena=9000)
    got = ext2[:batch.n_logs, 0] != np.uint64(D.NONE64)
    assert got.any() and not got.all()
    assert np.array_equal(starved.logs["n_patches"][~got], ref.logs["n_patches"][~got]) and np.all(starved.logs["status"][~got] == abi.ERR_CAPACITY)
    assert np.all(starved.logs["status"][got] == 0)
    late = wire.encode_docs([[H.synthetic_marks_log(400, 300, 5, max_span=400)]])
    lres = H.emu_merge(late, lds_bytes=160 * 1024)
    lref = D.emu_replay_hbm(late, lres, cap=200000)
    lpat, lext = D.emu_replay_hbm_with_arena(late, lres, cap=40, arena=400000)
    assert int(lext[0, 1]) != D.NONE64 and int(lpat.logs[0]["status"]) == 0, (lext, lref.logs)
    n = int(lref.logs[0]["n_patches"])
    assert int(lpat.logs[0]["n_patches"]) == n and n > 40 + int(lext[0, 2])
    assert np.array_equal(lpat.patches[:n], lref.patches[:n])
    assert np.array_equal(lref.patches[:n], D.stream(H.emu_replay(late, lres, cap=200000, gwin=True), 0))


def test_mark_ranges_longer_than_one_tile():
    """A mark op whose range is longer than the tile of cw / cnt the LDS holds (1024 words = 32 768 boundary slots) is worked through tile by tile, the record
    count carried across: document-wide marks over a 40 000-character text with defined slots spread all over it, byte-equal to the LDS build's stream (which
    the oracle pins on the other documents) in all three loop orders."""
    changes = H.synthetic_marks_log(40000, 600, 11, n_deletes=500)
    ids = lambda i: "%d@doc1" % (2 + i)  # noqa: E731
    ctr = 40000 + 2 + 500 + 600
    seq = len(changes) + 1
    for k, (mt, act, a, e) in enumerate([("strong", "addMark", 10, 39990), ("link", "addMark", 0, 39999), ("comment", "addMark", 5, 39000), ("strong", "removeMark", 100, 38000),
                                         ("link", "addMark", 3, 39998), ("comment", "removeMark", 7, 39500), ("em", "addMark", 0, 39999)]):
        op = {"opId": "%d@doc1" % ctr, "action": act, "obj": "1@doc1", "start": {"type": "before", "elemId": ids(a)}, "markType": mt}
        op["end"] = {"type": "before", "elemId": ids(e)} if mt in ("strong", "em") else {"type": "after", "elemId": ids(e)}
        if mt == "link":
            op["attrs"] = {"url": "%s.org" % "xy"[k & 1]}
        if mt == "comment":
            op["attrs"] = {"id": "comment-1"}
        changes.append({"actor": "doc1", "seq": seq, "deps": {}, "startOp": ctr, "ops": [op]})
        ctr += 1
        seq += 1
    batch = wire.encode_docs([[changes]])
    res = H.emu_merge_big(batch)
    assert int(res.logs["status"][0]) == 0
    want = H.emu_replay(batch, res, gwin=True)
    assert int(want.logs["status"][0]) == 0 and int(want.logs["n_patches"][0]) > 41000
    for reverse in (0, 1, 2):
        assert _same(D.emu_replay_hbm(batch, res, reverse=reverse), want), reverse


def test_documents_beyond_one_cu_lds_against_the_oracle():
    """Docs A and B (replay_hbm_docs.py): their replay working set exceeds the 160 KB of one CU, so replay_core.h reports PTX_ERR_CAPACITY for them; with the state
    in scratch every record equals the oracle's, the counts too, and a second loop order gives the same bytes."""
    if not H.have_node():
        pytest.skip("node not installed")
    batch = D.batch()
    assert all(D.lds_working_set(batch, l) > 160 * 1024 for l in range(2))
    res = H.emu_merge_big(batch)
    assert np.all(res.logs["status"] == 0)
    refused = H.emu_replay(batch, res)  # the LDS build: beyond its capacity
    assert np.all(refused.logs["status"] == abi.ERR_CAPACITY) and np.all(refused.logs["n_patches"] == 0)
    expected = D.expected()
    assert all("error" not in e for exp in expected for e in exp)
    pat = D.emu_replay_hbm(batch, res)
    assert np.all(pat.logs["status"] == 0)
    assert [int(x) for x in pat.logs["n_patches"]] == [len(exp[0]["patches"]) for exp in expected]
    assert H.check_patch_streams(batch, pat, expected) == 2
    assert _same(D.emu_replay_hbm(batch, res, reverse=2), pat)


def _mini_doc(ops, first_text="ABCDE"):
    from test_emu_parity import _mini_doc as m
    return m(ops, first_text=first_text)


def test_failed_logs_have_no_stream_and_capacity_is_reported():
    docs = [
        [_mini_doc([{"action": "del", "elemId": "77@zz"}])],
        [_mini_doc([{"action": "set", "insert": True, "elemId": "6@a", "value": "ok"}])],
    ]
    batch = wire.encode_docs(docs)
    res = H.emu_merge(batch)
    pat = D.emu_replay_hbm(batch, res)
    assert int(pat.logs[0]["status"]) == abi.ERR_ELEM_NOT_FOUND and int(pat.logs[0]["n_patches"]) == 0
    assert int(pat.logs[1]["status"]) == 0 and int(pat.logs[1]["n_patches"]) == 7  # makeList + 5 chars + 1
    small = D.emu_replay_hbm(batch, res, cap=3)  # a too-small record capacity: the count is still exact, the status says the rows are truncated
    assert int(small.logs[1]["status"]) == abi.ERR_CAPACITY and int(small.logs[1]["n_patches"]) == 7


def test_a_log_of_more_than_32766_elements_needs_the_high_halves_of_its_slots():
    """A result without ref_slots_hi cannot say where the marks of such a log are: PTX_ERR_CAPACITY, as from the LDS build."""
    batch = wire.encode_docs([[H.synthetic_marks_log(33000, 20, 3)]])
    res = H.emu_merge_big(batch, refs_hi=False)
    pat = D.emu_replay_hbm(batch, res)
    assert int(pat.logs[0]["status"]) == abi.ERR_CAPACITY and int(pat.logs[0]["n_patches"]) == 0
    with_hi = H.emu_merge_big(batch)
    assert _same(D.emu_replay_hbm(batch, with_hi), H.emu_replay(batch, with_hi, gwin=True))


def test_state_scratch_size():
    """ptx_replay_hbm_units: linear in the document (about 9.5 bytes per element for a text without comment ops: 8 of them the per-slot link urls), a fixed LDS footprint."""
    lib = D._lib()
    small, big = int(lib.ptx_emu_replay_hbm_units(1000, 10, 0, 0)), int(lib.ptx_emu_replay_hbm_units(1000000, 10, 0, 0))
    assert 4 * small < 12 * 1000 and 9 * 1000000 < 4 * big < 10 * 1000000
    assert int(lib.ptx_emu_replay_hbm_lds_bytes()) <= 12288


def test_the_driver_is_clean_under_the_sanitizers(tmp_path):
    """The driver built with -fsanitize=address,undefined (host build only) replays the rich fixture, overflow extents and a tail included, without a report."""
    from test_emu_sanitizer import _lib
    asan, ubsan = _lib("libasan.so"), _lib("libubsan.so")
    if not asan or not ubsan:
        pytest.skip("no libasan / libubsan in this image")
    so = str(tmp_path / "libperitext_emu_replay_hbm_asan.so")
    p = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-shared", "-fPIC", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-o", so,
                        os.path.join(H.ROOT, "tests", "emu", "emu_replay_hbm.cc")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    code = (
        "import json, os, sys\n"
        "sys.path.insert(0, %r)\n"
        "import numpy as np\n"
        "import helpers as H, replay_hbm_docs as D\n"
        "from peritext_amd import wire\n"
        "g = json.load(open(os.path.join(H.GOLDEN, 'patches_rich_300.json')))\n"
        "batch = wire.encode_docs([d['logs'] for d in g['docs']])\n"
        "res = H.emu_merge(batch)\n"
        "for rev in (0, 2):\n"
        "    pat = D.emu_replay_hbm(batch, res, reverse=rev, lib_path=%r)\n"
        "    assert H.check_patch_streams(batch, pat, [d['expected'] for d in g['docs']]) == batch.n_logs\n"
        "D.emu_replay_hbm_with_arena(batch, res, cap=40, arena=200000, lib_path=%r)\n"
        "D.emu_replay_hbm(batch, res, first_row=np.full(batch.n_logs, 100), lib_path=%r)\n"
        "big = wire.encode_docs([[H.synthetic_marks_log(70000, 300, 3, n_deletes=200)]])\n"
        "bres = H.emu_merge_big(big)\n"
        "assert int(D.emu_replay_hbm(big, bres, lib_path=%r).logs[0]['status']) == 0\n"
        "print('clean')\n"
    ) % (os.path.join(H.ROOT, "tests"), so, so, so, so)
    preload = ":".join([asan, ubsan] + [x for x in os.environ.get("LD_PRELOAD", "").split(":") if x])  # (the sanitizer runtime first, what was preloaded stays)
    env = dict(os.environ, LD_PRELOAD=preload, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", PYTHONPATH=H.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=H.ROOT, timeout=900)
    assert r.returncode == 0 and "clean" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
