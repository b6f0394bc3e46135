"""The admission marks of a resident batch (merge_core.h ptx_adm_mark) on the GPU: a batch that was merged before is not walked again, a batch grown
by an append is walked from where its base's merges stopped — and every answer is still the oracle's for the whole log.  The logs are those of
tests/test_emu_adm_marks.py (tests/adm_mark_cases.py: 96 to 1 100 ops, three actors, appended parts of 1 to 769 changes, intact or inadmissible in three ways)
plus documents of four, five and nine actors.  Nothing expected here comes from this library: a second merge is compared with the oracle like the first.

What this file shows is that the ANSWERS do not depend on the marks.  That a grown log really walks its suffix only — and not, after a wrong record, the whole log
through the exact walk, which would answer the same — is shown by the emulation twin alone: it reads the records back and counts the exact walks; the library
exports neither."""
import numpy as np
import pytest

import adm_mark_cases as M
import helpers as H
from peritext_amd import abi, wire

pytestmark = pytest.mark.gpu
OPS = 1100
NO_RANK = abi.FLAG_NO_ELEM_RANK


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch  # (first, as in the other GPU modules: the wrapped batch below lives in torch tensors)

    assert torch.cuda.is_available(), "GPU tests need a real MI355X"


def _engine(flags=0, threads=0):
    from peritext_amd.engine import Engine

    e = Engine(0, flags=flags)
    if threads:
        e.set_launch_shape(threads, 0)
    return e


def _merge(e, db):
    dr = e.alloc_result(db)
    try:
        e.merge(db, dr)
        return e.download(db, dr)
    finally:
        e.free_result(dr)


def _same(a, b):
    for k in ("logs", "values", "spans", "cintervals", "elem_rank"):
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()), k


def _cases(short=False):
    """short: the cases whose grown log has at most 350 changes (up to 441 rows: one wave per log, a window the one-wave lean build takes)"""
    assert H.have_node(), "these cases need node, the oracle's runtime"
    cs = M.cases(OPS, 350 if short else None)
    rows = np.diff(cs["grown"].log_off.astype(np.int64))
    assert 96 <= int(rows.min()) and int(rows.max()) <= (512 if short else 1101)
    return cs


def _check_all(cs, res):
    for l, c in enumerate(cs["cases"]):
        M.check_grown(c, cs["grown"], res, l)


# (f) the build a batch takes is what it was before the marks: the names are literals here, asserted before the first merge and after the last
# (the 64- and 128-thread shapes are the library's own choice for logs of up to 512 / 2 048 rows; 192 threads are forced: its own choice from 2 049 rows on)
@pytest.mark.parametrize("flags,force,threads,kernel", [(0, 0, 128, ("ptx_merge_kernel_w7", "ptx_merge_kernel")), (NO_RANK, 0, 64, ("ptx_merge_kernel_lean64",)),
                                                        (NO_RANK, 0, 128, ("ptx_merge_kernel_lean128",)), (NO_RANK, 192, 192, ("ptx_merge_kernel_lean192",))],
                         ids=["general", "lean64", "lean128", "lean192"])
def test_repeated_merges_answer_like_the_oracle_every_time(flags, force, threads, kernel):
    """(a) three merges of one batch — the first walks every log and marks those that pass, the others walk only the failing ones: status, counts, digests and
    rows identical each time and the oracle's; one failing log per kind of fault (and more) fails identically all three times."""
    cs = _cases(short=threads == 64)
    assert {c["kind"] for c in cs["cases"] if c["code"]} >= set(M.KINDS)
    with _engine(flags, force) as e:
        db = e.upload(cs["grown"])
        try:
            name = e.batch_kernel_name(db)
            assert name in kernel and e.launch_shape(db)[0] == threads
            runs = [_merge(e, db) for _ in range(3)]
            assert e.batch_kernel_name(db) == name
        finally:
            e.free_batch(db)
    _check_all(cs, runs[0])
    _same(runs[0], runs[1])
    _same(runs[0], runs[2])
    _check_all(cs, runs[2])


def test_a_context_without_admission_marks_nothing():
    """(b) a PTX_FLAG_NO_ADMISSION context merges a batch that holds inadmissible logs first (and takes them); a context that admits then still reports each of them,
    and the first context's answer is afterwards what it was."""
    cs = _cases()
    with _engine(NO_RANK) as e1, _engine(NO_RANK | abi.FLAG_NO_ADMISSION) as e0:
        db = e1.upload(cs["grown"])
        try:
            r0 = _merge(e0, db)
            assert (r0.logs["status"] == 0).all()
            r1 = _merge(e1, db)
            _check_all(cs, r1)
            _same(r0, _merge(e0, db))
            _same(r1, _merge(e1, db))
        finally:
            e1.free_batch(db)


@pytest.mark.parametrize("how", ["append", "append_device"])
@pytest.mark.parametrize("base", ["merged", "never_merged"])
def test_appends_walk_from_the_base_s_marks(how, base):
    """(c) ptx_batch_append / ptx_batch_append_device onto a base that was merged (its valid logs marked, its failed logs — kind 'bad_base' — not) and onto one no
    merge has seen; appended parts valid and invalid, of every length of the case table.  The grown batch answers like a fresh upload of the concatenated logs
    under PTX_FLAG_READMIT and like the oracle, at the first merge and at the second.  (The "failed base" is the 'bad_base' logs of the merged base.)"""
    cs = _cases()
    grown, cases = cs["grown"], cs["cases"]
    head, tail = wire.split_batch(grown, [c["m"] for c in cases])
    with _engine(NO_RANK | abi.FLAG_READMIT) as f:
        db = f.upload(grown)
        try:
            fresh = _merge(f, db)
            fresh_name = f.batch_kernel_name(db)
        finally:
            f.free_batch(db)
    _check_all(cs, fresh)
    with _engine(NO_RANK) as e:
        dh = e.upload(head)
        dt = dg = None
        try:
            if base == "merged":
                rh = _merge(e, dh)
                for l, c in enumerate(cases):
                    assert (int(rh.logs["status"][l]) != 0) == (c["kind"] == "bad_base"), c
            if how == "append":
                dg = e.append(dh, tail)
            else:
                dt = e.upload(tail)
                dg = e.append_device(dh, dt)
            assert e.batch_kernel_name(dg) == fresh_name
            r1, r2 = _merge(e, dg), _merge(e, dg)
            if base == "merged":
                _same(rh, _merge(e, dh))  # (the base itself is as it was)
        finally:
            for h in (dg, dt, dh):
                if h is not None:
                    e.free_batch(h)
    _same(r1, fresh)
    _same(r2, fresh)
    _check_all(cs, r1)


def _gen_docs(replicas, seed, docs=2, ops=300):
    gen = H.oracle_gen("mini", docs, seed, ops, replicas)
    batch = wire.encode_docs([d["logs"] for d in gen["docs"]])
    assert batch.max_actors == replicas
    return batch, [x for d in gen["docs"] for x in d["expected"]]


def _check_expected(batch, res, expected):
    for l, exp in enumerate(expected):
        H.check_log(batch, res, l, exp)


def test_an_append_that_brings_in_a_fourth_actor():
    """(c) the base holds the changes of three actors of a four-actor document, the append the first changes of the fourth: the marks of a document of more than
    three actors carry no clock, so the grown logs are walked whole — and answer like the oracle, twice.  (Base and append are both encoded for four actors: an
    append whose max_actors differs from its base's is refused by ptx_batch_append, so a batch can never go from three to four.)"""
    batch, expected = _gen_docs(4, 21, docs=1)
    cut = []
    for l in range(batch.n_logs):
        a = batch.chg_actor[int(batch.chg_off[l]): int(batch.chg_off[l + 1])]
        seen, k = set(), len(a)
        for i, x in enumerate(a):
            seen.add(int(x))
            if len(seen) == 4:
                k = i
                break
        cut.append(k)
    assert all(0 < k for k in cut) and any(k < int(batch.chg_off[l + 1] - batch.chg_off[l]) for l, k in enumerate(cut))
    head, tail = wire.split_batch(batch, cut)
    with _engine(0) as e:
        dh = e.upload(head)
        dg = None
        try:
            assert (_merge(e, dh).logs["status"] == 0).all()
            dg = e.append(dh, tail)
            assert e.batch_kernel_name(dg) == "ptx_merge_kernel_many"
            r1, r2 = _merge(e, dg), _merge(e, dg)
        finally:
            if dg is not None:
                e.free_batch(dg)
            e.free_batch(dh)
    _check_expected(batch, r1, expected)
    _same(r1, r2)


@pytest.mark.parametrize("replicas,kernel", [(5, "ptx_merge_kernel_many"), (9, "ptx_merge_kernel_many_wide")])
def test_many_actor_batches_twice_and_after_an_append(replicas, kernel):
    """(d) documents of five and nine actors (the builds whose marks say "all of the log" or nothing): merged twice, then cut in half, the halves appended, merged
    twice again — with one log's envelope made inadmissible, which must fail every time while its neighbours pass."""
    import copy

    gen = H.oracle_gen("mini", 2, 30 + replicas, 300, replicas)
    docs = [list(d["logs"]) for d in gen["docs"]]
    expected = [x for d in gen["docs"] for x in d["expected"]]
    broken = copy.deepcopy(docs[-1][-1])
    broken[5]["seq"] += 1  # a seq skipped in the last log
    docs[-1][-1] = broken
    want_bad = M._code(H.oracle_apply([[broken]], no_patches=True)[0][0])
    assert want_bad == abi.ERR_SEQ_GAP  # (the oracle's own verdict)
    batch = wire.encode_docs(docs)
    assert batch.max_actors == replicas
    bad = batch.n_logs - 1
    nch = np.diff(batch.chg_off.astype(np.int64))
    head, tail = wire.split_batch(batch, nch // 2)

    def check(res):
        assert int(res.logs["status"][bad]) == want_bad
        for l, exp in enumerate(expected):
            if l != bad:
                H.check_log(batch, res, l, exp)

    with _engine(0) as e:
        db = e.upload(batch)
        dh = e.upload(head)
        dg = None
        try:
            assert e.batch_kernel_name(db) == kernel
            r1, r2 = _merge(e, db), _merge(e, db)
            _merge(e, dh)
            dg = e.append(dh, tail)
            assert e.batch_kernel_name(dg) == kernel
            g1, g2 = _merge(e, dg), _merge(e, dg)
        finally:
            for h in (dg, dh, db):
                if h is not None:
                    e.free_batch(h)
    check(r1)
    for r in (r2, g1, g2):
        _same(r1, r)


def test_readmit_contexts_and_wrapped_batches_behave_as_before():
    """(e) a PTX_FLAG_READMIT context walks every log in every launch and leaves the marks alone: the oracle's answers three times, before and after a context
    that keeps marks has merged the same batch.  A batch wrapped around caller-owned device columns is merged twice and answers like an upload merged without
    admission, and like the oracle where the ops are intact — trivially so as far as marks go: ptx_batch_wrap_device takes no chg_* columns, so a wrapped batch has
    no envelope to admit.  That a batch which does not own its columns gets no mark array is the `owns` test in the host's census_and_shape; no test can reach it."""
    import torch

    cs = _cases()
    grown = cs["grown"]
    with _engine(NO_RANK | abi.FLAG_READMIT) as f, _engine(NO_RANK) as e, _engine(NO_RANK | abi.FLAG_NO_ADMISSION) as n:
        db = e.upload(grown)
        try:
            name = e.batch_kernel_name(db)
            assert f.batch_kernel_name(db) == name
            a = [_merge(f, db), _merge(f, db)]
            b = _merge(e, db)
            a.append(_merge(f, db))
            plain = _merge(n, db)
        finally:
            e.free_batch(db)
        _check_all(cs, b)
        for r in a:
            _same(r, b)
        cols = {}
        for k in ("log_off", "op_id", "ref_a", "ref_b", "payload", "action", "mark_type", "side_a", "side_b"):
            x = getattr(grown, k)
            as_signed = {np.dtype("uint64"): np.int64, np.dtype("uint32"): np.int32, np.dtype("uint8"): np.uint8}[x.dtype]
            pad = np.zeros(8, dtype=x.dtype)  # (the byte columns are read a dword at a time)
            cols[k] = torch.from_numpy(np.concatenate([x, pad]).view(as_signed).copy()).cuda()
        torch.cuda.synchronize()
        dw = e.wrap_device(grown.n_logs, grown.n_ops, {k: v.data_ptr() for k, v in cols.items()})
        try:
            assert e.batch_kernel_name(dw) == n.batch_kernel_name(dw)
            w1, w2 = _merge(e, dw), _merge(e, dw)
        finally:
            e.free_batch(dw)
        del cols
    _same(w1, w2)
    _same(w1, plain)
    for l, c in enumerate(cs["cases"]):
        if not c["code"]:
            H.check_log(grown, w1, l, c["exp"])
