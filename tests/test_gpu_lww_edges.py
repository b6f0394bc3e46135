"""The last phase of the merge kernel (LWW trees, tiles of the visible axis, spans, digest) at the exact edges of the visible length, in every build of the kernel
the library launches: the batches of tests/lww_edge_cases.py (expected values: the oracle's) through the C ABI on the GPU.  tests/test_emu_lww_edges.py runs the same
batches on the CPU emulation, which only ever instantiates the body for any workgroup size; what a fixed workgroup size compiles in runs only here: the early
loads of the one- and two-wave builds, the char-per-lane query of lean64 / lean192 beyond T4 characters, the digest's DPP flush, one or two mark ops per thread
and step, the cached park words of the builds that tile long documents, and everything the three-wave build leaves out.

Every case is one engine and every batch of the suite — a few hundred small logs — under one launch shape: the shapes the library chooses (four contexts), every
workgroup size of the general build in the library's own window and in the CU's whole LDS, every lean build.  The kernel's name and the workgroup size are
asserted against the literal tables of lww_edge_cases (GENERAL_KERNEL, LEAN_KERNEL, NATURAL; tests/test_emu_lww_edges.py holds them to the host's window rule),
every log against the oracle by helpers.check_log.  Nothing here loads the emulation library: the window each batch gets is a literal too (NATURAL)."""
import pytest

import helpers as H
import lww_edge_cases as LC
from peritext_amd import abi

pytestmark = pytest.mark.gpu

LDS_WHOLE = 160 * 1024
RAN = {}  # (context, threads, lds) -> {batch: kernel}, as observed by the cases of this file that ran


def _run(context, flags, threads, lds, want_kernel, want_threads):
    """Every batch under ptx_set_launch_shape(threads, lds) in a context with `flags`: name, workgroup size and window as expected, every log against the oracle."""
    from peritext_amd.engine import Engine

    assert H.have_node(), "these cases need node, the oracle's runtime: a skipped case would hide exactly what this file exists to show"
    seen = RAN.setdefault((context, threads, lds), {})
    with Engine(0, flags=flags) as e:
        if threads or lds:
            e.set_launch_shape(threads, lds)
        for b in LC.batches():
            db = e.upload(b.batch)
            dr = e.alloc_result(db)
            try:
                kernel = e.batch_kernel_name(db)
                t, l = e.launch_shape(db)
                e.merge(db, dr)
                res = e.download(db, dr)
            finally:
                e.free_result(dr)
                e.free_batch(db)
            assert kernel == want_kernel(b.name), (b.name, kernel)
            assert t == want_threads(b.name) and l == (lds or LC.NATURAL[b.name][1]), (b.name, t, l)
            LC.check_batch(b, res)
            seen[b.name] = kernel


@pytest.mark.parametrize("flags", [0, abi.FLAG_NO_ADMISSION, abi.FLAG_NO_ELEM_RANK, abi.FLAG_NO_ELEM_RANK | abi.FLAG_NO_ADMISSION],
                         ids=["general", "general-no-admission", "lean", "lean-no-admission"])
def test_the_shapes_the_library_chooses(flags):
    lean = bool(flags & abi.FLAG_NO_ELEM_RANK)
    _run("lean" if lean else "general", flags, 0, 0, lambda name: LC.NATURAL[name][3 if lean else 2], lambda name: LC.NATURAL[name][0])


@pytest.mark.parametrize("lds", [0, LDS_WHOLE], ids=["own-window", "whole-lds"])
@pytest.mark.parametrize("threads", LC.GENERAL_THREADS)
def test_every_workgroup_size_of_the_general_build(threads, lds):
    k = LC.GENERAL_THREADS.index(threads)
    _run("general", 0, threads, lds, (lambda name: LC.G) if lds else (lambda name: LC.GENERAL_KERNEL[name][k]), lambda name: threads)


@pytest.mark.parametrize("threads", LC.LEAN_THREADS)
def test_every_lean_build(threads):
    k = LC.LEAN_THREADS.index(threads)
    _run("lean", abi.FLAG_NO_ELEM_RANK, threads, 0, lambda name: LC.LEAN_KERNEL[name][k], lambda name: threads)


def test_every_lean_build_ran_every_regime_it_can_reach():
    """The tables the cases above assert, against the coverage this file promises (every entry is asserted by the case of its launch shape: with the whole file
    passing, every pair listed here ran in that build; what this session's cases observed is compared too).  What is absent is the window rule's doing: lean64
    beyond T4 inserts with marks, lean128 beyond 2 T1 inserts (V + 3 of them: from V = 2 T1 - 2 on), lean192 from 1 500 inserts on."""
    reach = {}
    for name, kernels in LC.LEAN_KERNEL.items():
        for kernel in kernels:
            if kernel != LC.G:
                reach.setdefault(kernel, set()).add(name.split("-", 1)[1])
    every = {r for r, _ in LC.REGIMES}
    assert reach == {
        LC.L64: {"v-le-65", "v-le-t4"},  # (T4 characters exactly: the documents without a delete)
        LC.L128: every - {"v-le-2t1", "v-le-2t1+3", "v-gt-2t1+3"},
        LC.L192: every - {"v-gt-2t1+3"},
        LC.L256: every,
    }
    assert {n for n, k in LC.LEAN_KERNEL.items() if k[0] == LC.L64} == {"A-v-le-65", "N-v-le-t4"}
    # the builds the general context takes: both at every regime
    assert {k for ks in LC.GENERAL_KERNEL.values() for k in ks} == {LC.G, LC.W7}
    for (context, threads, lds), seen in RAN.items():
        for name, kernel in seen.items():
            if context == "lean" and threads:
                assert kernel == LC.LEAN_KERNEL[name][LC.LEAN_THREADS.index(threads)]
            elif threads:
                assert kernel == (LC.G if lds else LC.GENERAL_KERNEL[name][LC.GENERAL_THREADS.index(threads)])
            else:
                assert kernel == LC.NATURAL[name][3 if context == "lean" else 2]
