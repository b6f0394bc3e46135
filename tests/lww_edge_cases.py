"""The last phase of the merge kernel (P5b + P6 of ptx_merge_log_body, peritext_amd/csrc/merge_core.h: LWW winners per visible char, spans, digest) at the exact
edges of the visible length V it branches on: the cases tests/test_emu_lww_edges.py (CPU emulation) and tests/test_gpu_lww_edges.py (the library on the GPU) share.

Every edge size comes from abi.LWW_TILE_4 (T4 below: up to that many characters four trees are resident) and abi.LWW_TILE_1 (T1: the tile of longer documents,
twice that where the launch's window has room).  Expected spans and text come only from the in-repo oracle (helpers.oracle_apply(..., no_patches=True)), one run
for the whole suite, never from a build of the kernel.

Family A: single-replica documents (helpers.mini_doc): V + 3 inserts, three deletes (the two characters behind the text and one in its middle), then the mark
ops of marks_for(); at one character behind each edge also documents that carry a single mark over the whole text and no span boundary at any edge (their ids
end in "whole-only").  Family N: the marks of family A over exactly T4 inserts and no delete, every set of mark types (with V + 3 inserts a document of T4
characters has more than T4 elements, which the one-wave lean build's window never holds beside mark ops).  Family B: two actors whose mark ops are concurrent
and carry the same counters, so the actor's rank decides the LWW winner; built twice, with the actors' names swapped.

The documents are grouped into BATCHES by the regime of V, fewer than 64 logs each: a launch is shaped by its largest log, so a batch of one regime runs in that
regime's launch shape and LDS window, and a batch of fewer than 64 logs is never split into a second launch group."""
import dataclasses
import functools

import helpers as H
from peritext_amd import abi, wire

T4, T1 = abi.LWW_TILE_4, abi.LWW_TILE_1
TYPES = ("strong", "em", "comment", "link")  # in the order of the kernel's mark-type codes (the bits of its `present4`)

# the visible lengths: the digest's flush changes at 48, a wave is 64 chars wide, the four-tree form ends at T4, the "mid" form at 2 T4, tiles of T1 or 2 T1;
# the three tails behind 2 T1 are the three residues of the three-chars-per-step query
V_VALUES = (1, 2, 3, 31, 32, 33, 47, 48, 49, 63, 64, 65, T4 - 1, T4, T4 + 1, 2 * T4 - 1, 2 * T4, 2 * T4 + 1, T1 - 1, T1, T1 + 1, 2 * T1 - 1, 2 * T1, 2 * T1 + 1,
            2 * T1 + 2, 2 * T1 + 3, 3 * T1 - 1, 3 * T1, 3 * T1 + 1, 4 * T1 - 1, 4 * T1, 4 * T1 + 1)
V_ALL_SUBSETS = (T4, T4 + 1, 2 * T4 - 1, 2 * T4, 2 * T4 + 1, T1, 2 * T1, 2 * T1 + 1)  # every subset of the four mark types here
ALL_SUBSETS = tuple(tuple(t for k, t in enumerate(TYPES) if (m >> k) & 1) for m in range(16))
FEW_SUBSETS = ((), ("strong",), ("strong", "em"), ("comment",), TYPES)
EDGES = (64, T4, 2 * T4, T1, 2 * T1, 3 * T1, 4 * T1)  # visible positions where a wave, a tree or a tile starts (and V - 1, per document)
V_WHOLE_ONLY = (T4 + 1, 2 * T4 + 1, T1 + 1, 2 * T1 + 1, 2 * T1 + 3, 3 * T1 + 1, 4 * T1 + 1)  # one char behind each edge (and the tail of three behind 2 T1)
V_FAMILY_B = (T4 + 1, 2 * T4, T1 + 1, 2 * T1 + 1)
# regime name -> largest V.  Beside the lengths the kernel branches on, a regime ends where the window of its largest log would keep a lean build out that its
# smaller logs can reach (V + 3 inserts: more than T4 from V = T4 - 2 on; the tails of three behind T1 and 2 T1 from the documents of another tile behind them)
REGIMES = (("v-le-65", 65), ("v-le-t4", T4), ("v-le-2t4", 2 * T4), ("v-le-t1", T1), ("v-t1+1", T1 + 1), ("v-le-2t1", 2 * T1), ("v-le-2t1+3", 2 * T1 + 3),
           ("v-gt-2t1+3", 1 << 30))


def regime_of(v):
    return next(name for name, top in REGIMES if v <= top)


def edges_of(v):
    """the edges a document of v visible characters has inside it"""
    return sorted({e for e in EDGES + (v - 1,) if 0 < e < v})


class _Doc:
    """V visible characters over V + 3 elements: element `mid` and the last two are deleted (or, deleted=False, over V elements).  Visible position p <->
    element index."""

    def __init__(self, v, deleted=True):
        self.v, self.mid = v, v // 2 if deleted else v

    def el(self, p):
        return "%d@a" % ((p if p < self.mid else p + 1) + 2)

    def deletes(self):
        return [{"action": "del", "elemId": "%d@a" % (i + 2)} for i in (self.v + 1, self.v + 2, self.mid)]

    def mark(self, action, ty, lo, hi, attrs=None, eot=False):
        """a mark op over the visible positions [lo, hi) clipped to the text, or None if nothing is left.  The boundary rule of the reference's changeMark: strong
        and em end `before` the next element (or at endOfText), link and comment `after` their last."""
        lo, hi = max(lo, 0), min(hi, self.v)
        if lo >= hi:
            return None
        op = {"action": action, "markType": ty, "start": {"type": "before", "elemId": self.el(lo)}}
        if ty in ("strong", "em"):
            op["end"] = {"type": "endOfText"} if eot or hi == self.v else {"type": "before", "elemId": self.el(hi)}
        else:
            op["end"] = {"type": "endOfText"} if eot else {"type": "after", "elemId": self.el(hi - 1)}
        if attrs:
            op["attrs"] = attrs
        return op


def marks_for(v, types, whole, deleted=True):
    """The mark ops of one family-A document, in opId order.  Per present type:
      * `whole`: one mark over the whole document, the smallest opId (a tree's root where V is a tile; later ops win over it where they reach);
      * a region this type alone covers besides the whole-document mark (types that shared every range would not tell a shared tree from their own);
      * at every edge e: a mark straddling e, one ending exactly at e (`before el(e)` / `after el(e - 1)`), one starting exactly at e.  strong: the one that ends
        at e is a removeMark, em: the one that starts at e, so each leaves a span boundary exactly at e; at the first two edges a wider removeMark straddles e
        between them (larger opId than the addMark under it, smaller than the marks at e).  Links carry a different url on each side of e, comments distinct ids.
        Which of the two marks that meet at e has the larger opId alternates with the edge and the type: a range clipped one character long or short on either
        side would hand that character to the wrong winner;
      * a mark that ends at endOfText (below the marks at the edges: V - 1 is one of them)."""
    d = _Doc(v, deleted)
    ops = []
    for ty in types:
        k = TYPES.index(ty)
        attrs = (lambda tag, _ty=ty: {"url": "%s.example" % tag} if _ty == "link" else {"id": "c-%s" % tag} if _ty == "comment" else None)
        if ty == whole:
            ops.append(d.mark("addMark", ty, 0, v, attrs("whole"), eot=ty in ("strong", "em")))
        ops.append(d.mark("addMark", ty, 8 + 5 * k, 11 + 5 * k, attrs("own")))
        ops.append(d.mark("addMark", ty, v - 2 - k, v, attrs("tail"), eot=True))
        for i, e in enumerate(edges_of(v)):
            ops.append(d.mark("addMark", ty, e - 4 - k, e + 4 + k, attrs("x%d" % e)))
            if ty in ("strong", "em"):
                if i < 2:
                    ops.append(d.mark("removeMark", ty, e - 3, e + 3))
                at_e = [d.mark("removeMark" if ty == "strong" else "addMark", ty, e - 2, e), d.mark("addMark" if ty == "strong" else "removeMark", ty, e, e + 2)]
            else:
                at_e = [d.mark("addMark", ty, e - 2 - k, e, attrs("l%d" % e)), d.mark("addMark", ty, e, e + 2 + k, attrs("r%d" % e))]
            ops += at_e if (i + k) % 2 == 0 else at_e[::-1]
    return [op for op in ops if op is not None]


def family_a_doc(v, types, whole):
    d = _Doc(v)
    text = "".join("abcdefghijklmnopqrstuvwxyz"[i % 26] for i in range(v + 3))
    return H.mini_doc(d.deletes() + marks_for(v, types, whole), first_text=text)


def family_n_doc(v, types, whole):
    """the same marks over a text of exactly V inserts and no delete"""
    text = "".join("abcdefghijklmnopqrstuvwxyz"[i % 26] for i in range(v))
    return H.mini_doc(marks_for(v, types, whole, deleted=False), first_text=text)


def concurrent_change(log, ops, actor="b"):
    """`log` (helpers.mini_doc) followed by ONE change of `actor` that knows only a's first change: concurrent to a's second, its op counters those of a's mark
    ops (the ops behind the deletes of a's second change, which must hold at least as many)."""
    c1, c2 = log
    n_del = sum(1 for op in c2["ops"] if op["action"] == "del")
    start = c2["startOp"] + n_del
    assert len(ops) <= len(c2["ops"]) - n_del
    made = []
    for k, op in enumerate(ops):
        o = dict(op)
        o["opId"] = "%d@%s" % (start + k, actor)
        o["obj"] = c1["ops"][0]["opId"]
        made.append(o)
    return [c1, c2, {"actor": actor, "seq": 1, "deps": {c1["actor"]: 1}, "startOp": start, "ops": made}]


def rename_actors(log, names):
    """the same log with its actors renamed (opIds, element references, deps): the rank of the actors, which breaks a tie of counters, changes with it"""
    def sid(x):
        if isinstance(x, str) and "@" in x:
            c, a = x.split("@", 1)
            return "%s@%s" % (c, names.get(a, a))
        return x

    def sop(op):
        o = dict(op)
        for key in ("opId", "obj", "elemId"):
            if key in o:
                o[key] = sid(o[key])
        for key in ("start", "end"):
            if key in o and "elemId" in o[key]:
                o[key] = dict(o[key], elemId=sid(o[key]["elemId"]))
        return o

    return [dict(c, actor=names.get(c["actor"], c["actor"]), deps={names.get(a, a): s for a, s in c["deps"].items()}, ops=[sop(o) for o in c["ops"]]) for c in log]


def family_b_docs(v):
    """Two documents of V visible characters whose tile start (or tree half) e lies under concurrent ops of the same counter, each as written (`a` types, `b`
    answers) and with the two names swapped; each document as two logs, b's change applied last and a's second change applied last."""
    d = _Doc(v)
    e = max(x for x in (T4, T1, 2 * T1) if x < v)  # (V = 2 T4: the two halves of the 256-leaf tree)
    url = lambda u: {"url": "%s.example" % u}  # noqa: E731
    pairs = [
        # a adds strong, b removes it over an overlapping range across e (same counter: the larger actor wins where both reach)
        ([d.mark("addMark", "strong", e - 6, e + 3), d.mark("addMark", "em", e - 1, e + 1)], [d.mark("removeMark", "strong", e - 2, e + 7), d.mark("addMark", "em", e, e + 5)]),
        # two links with different urls across e, and a comment each
        ([d.mark("addMark", "link", e - 5, e + 2, url("a")), d.mark("addMark", "comment", e - 3, e, {"id": "c-a"})],
         [d.mark("addMark", "link", e - 2, e + 6, url("b")), d.mark("addMark", "comment", e - 1, e + 3, {"id": "c-b"})]),
    ]
    text = "".join("abcdefghijklmnopqrstuvwxyz"[i % 26] for i in range(v + 3))
    docs = []
    for ops_a, ops_b in pairs:
        c1, c2, cb = concurrent_change(H.mini_doc(d.deletes() + ops_a, first_text=text), ops_b)
        for names in ({}, {"a": "b", "b": "a"}):
            docs.append([rename_actors(log, names) for log in ([c1, c2, cb], [c1, cb, c2])])
    return docs


@dataclasses.dataclass
class Case:
    id: str
    v: int
    types: tuple  # mark types with ops
    whole: str  # the type whose mark covers the whole document (family A), or None
    logs: list  # the document: its replicas' logs
    expected: list = None  # per log, the oracle's {spans, text}


@dataclasses.dataclass
class Batch:
    name: str
    regime: str
    cases: list
    batch: wire.Batch
    expected: list  # flat, in log order
    case_of_log: list  # the case id behind every log



def _cases():
    out = []
    for n, v in enumerate(V_VALUES):
        for s, types in enumerate(ALL_SUBSETS if v in V_ALL_SUBSETS else FEW_SUBSETS):
            whole = types[(n + s) % len(types)] if types else None  # rotates with V (and with the subset: every type is the root somewhere)
            out.append(Case("A-v%d-%s" % (v, "+".join(types) or "none"), v, types, whole, [family_a_doc(v, types, whole)]))
    # every document above has a span boundary at every edge; these carry ONE mark over all of them (and a short one of the same type far from them): what the
    # last character of a tile hands to the first of the next must be taken for equal
    for v in V_WHOLE_ONLY:
        for ty in TYPES:
            d = _Doc(v)
            attrs = {"url": "whole.example"} if ty == "link" else {"id": "c-whole"} if ty == "comment" else None
            ops = [d.mark("addMark", ty, 0, v, attrs, eot=ty in ("strong", "em")), d.mark("addMark", ty, 20, 23, attrs)]
            text = "".join("abcdefghijklmnopqrstuvwxyz"[i % 26] for i in range(v + 3))
            out.append(Case("A-v%d-%s-whole-only" % (v, ty), v, (ty,), ty, [H.mini_doc(d.deletes() + ops, first_text=text)]))
    for s, types in enumerate(ALL_SUBSETS):
        whole = types[s % len(types)] if types else None
        out.append(Case("N-v%d-%s" % (T4, "+".join(types) or "none"), T4, types, whole, [family_n_doc(T4, types, whole)]))
    for v in V_FAMILY_B:
        for k, logs in enumerate(family_b_docs(v)):
            out.append(Case("B-v%d-%s-%s" % (v, ("strong-em", "link-comment")[k // 2], ("ab", "ba")[k % 2]), v, (("strong", "em"), ("comment", "link"))[k // 2], None, logs))
    return out


def _grouped(cases):
    """(batch name, regime, its cases): family by family, regime by regime"""
    out = []
    for fam in "ANB":
        for regime, _ in REGIMES:
            mine = [c for c in cases if c.id[0] == fam and regime_of(c.v) == regime]
            if mine:
                assert sum(len(c.logs) for c in mine) < 64, (fam, regime)
                out.append(("%s-%s" % (fam, regime), regime, mine))
    return out


@functools.lru_cache(maxsize=None)
def batch_names():
    """the names of the batches (parametrize ids): they need the case lists, not the oracle"""
    return [name for name, _, _ in _grouped(_cases())]


@functools.lru_cache(maxsize=None)
def suite():
    """Every case with the oracle's answer (one run of the oracle for all of them), and the batches they run in.  Shared by every test of a session: treat as
    read-only."""
    assert H.have_node(), "the expected spans come from the oracle, which needs node: a skipped suite would hide exactly what these files exist to show"
    cases = _cases()
    for c, exp in zip(cases, H.oracle_apply([c.logs for c in cases], no_patches=True)):
        assert len(exp) == len(c.logs) and all("error" not in e for e in exp), c.id
        c.expected = exp
    batches = []
    for name, regime, mine in _grouped(cases):
        b = wire.encode_docs([c.logs for c in mine])
        batches.append(Batch(name, regime, mine, b, [e for c in mine for e in c.expected], [c.id for c in mine for _ in c.logs]))
        assert b.n_logs == len(batches[-1].expected) < 64
    assert [b.name for b in batches] == batch_names()
    return cases, batches


def batches():
    return suite()[1]


def batch(name):
    return next(b for b in batches() if b.name == name)


def check_batch(b, res):
    """every log of a batch against the oracle (helpers.check_log: status, decoded spans, raw value / span / comment-interval rows, digest)"""
    for log, exp in enumerate(b.expected):
        try:
            H.check_log(b.batch, res, log, exp)
        except AssertionError as err:
            raise AssertionError("%s (batch %s): %s" % (b.case_of_log[log], b.name, err)) from None


def span_starts(exp):
    at, run = [], 0
    for s in exp["spans"]:
        at.append(run)
        run += len(s["text"])
    return at


def lds_need(b):
    """ptx_lds_need of every log of a wire.Batch (the emulation library's export): what the host sizes the launch's window with"""
    import ctypes as C

    lib = H._emu(H.EMU_LIB)
    lib.ptx_emu_lds_need.restype = C.c_uint64
    lib.ptx_emu_lds_need.argtypes = [C.c_uint64] * 7
    out = []
    for log in range(b.n_logs):
        h = b.log_hdr[log]
        out.append(int(lib.ptx_emu_lds_need(int(b.log_off[log + 1] - b.log_off[log]), int(h["n_ins"]), int(h["n_del"]), int(h["n_mark"].sum()), int(h["n_mark"][2]),
                                            (int(h["max_counter"]) + 1) * (int(h["max_actor"]) + 1), int(h["n_comment_ids"]))))
    return out


# ---- which build of the merge kernel a batch runs in (the host's rule, peritext_hip.hip: shape_launch, wants_w7, wants_lean) ----
LDS_CU, LDS_GRANULE = 160 * 1024, 1280


def launch_by_rule(b, threads=0, lds=0, lean_context=False):
    """(kernel name, threads, window) of a wire.Batch of small id keys and at most three actors under ptx_set_launch_shape(threads, lds): the window is the
    largest ptx_lds_need of the batch (4 096 bytes at the least) unless forced; the threads follow the longest log (64 up to 512 rows, 128 up to 2 048, 192 up
    to 4 608 — 256 where the window exceeds a seventh of the CU's LDS) unless forced; the seven-waves-per-SIMD builds where more than 24 waves share a CU by
    that window rounded to the CU's granule; a lean build in a context without elem_rank: lean256 at 256 threads whatever the window, lean64 / 128 / 192 where
    the seven-wave rule holds."""
    window = lds or min(max(max(lds_need(b)), 4096), LDS_CU)
    rows = max(int(b.log_off[i + 1] - b.log_off[i]) for i in range(b.n_logs))
    t = 64 if rows <= 512 else 128 if rows <= 2048 else 192 if rows <= 4608 else 256 if rows <= 12288 else 512
    if t == 192 and window > LDS_CU // 7:
        t = 256
    t = threads or t
    w7 = (LDS_CU // (-(-window // LDS_GRANULE) * LDS_GRANULE)) * ((t + 63) // 64) > 24
    assert b.max_actors <= 3 and all((int(h["max_counter"]) + 1) * (int(h["max_actor"]) + 1) <= 65536 for h in b.log_hdr)
    if lean_context and t == 256:
        return "ptx_merge_kernel_lean256", t, window
    if lean_context and w7 and t in (64, 128, 192):
        return "ptx_merge_kernel_lean%d" % t, t, window
    return "ptx_merge_kernel_w7" if w7 else "ptx_merge_kernel", t, window


# The builds each batch runs in, as literals (derived from the rule above, held to it by tests/test_emu_lww_edges.py and observed on the GPU by
# tests/test_gpu_lww_edges.py).  G: the general build, W7: the same at seven waves per SIMD; L64 .. L256: the lean builds.
G, W7 = "ptx_merge_kernel", "ptx_merge_kernel_w7"
L64, L128, L192, L256 = "ptx_merge_kernel_lean64", "ptx_merge_kernel_lean128", "ptx_merge_kernel_lean192", "ptx_merge_kernel_lean256"
GENERAL_THREADS = (64, 128, 192, 256, 512)
LEAN_THREADS = (64, 128, 192, 256)
# batch -> the kernel of a general context at 64, 128, 192, 256 and 512 threads in the library's own window (in a forced window of the CU's whole LDS: G everywhere)
GENERAL_KERNEL = {
    "A-v-le-65": (W7, W7, W7, W7, W7),
    "A-v-le-t4": (G, W7, W7, W7, W7),  # a window of 7 328 bytes: 21 logs per CU
    "A-v-le-2t4": (G, W7, W7, W7, W7),
    "A-v-le-t1": (G, W7, W7, W7, W7),
    "A-v-t1+1": (G, W7, W7, W7, W7),
    "A-v-le-2t1": (G, G, W7, W7, W7),  # 12 288 bytes: 12 logs per CU
    "A-v-le-2t1+3": (G, G, W7, W7, W7),
    "A-v-gt-2t1+3": (G, G, G, G, W7),  # 24 176 bytes: 6 logs per CU
    "N-v-le-t4": (W7, W7, W7, W7, W7),
    "B-v-le-2t4": (G, W7, W7, W7, W7),
    "B-v-t1+1": (G, W7, W7, W7, W7),
    "B-v-le-2t1+3": (G, G, W7, W7, W7),
}
# batch -> the kernel of a context without elem_rank at 64, 128, 192 and 256 threads.  G: the window rule keeps the pair out of the lean build (marks and more than
# T4 inserts: beyond lean64's 6 400 bytes; more than 2 T1 inserts: beyond lean128's 11 520; 1 500 inserts and more: beyond lean192's 17 920)
LEAN_KERNEL = {
    "A-v-le-65": (L64, L128, L192, L256),
    "A-v-le-t4": (G, L128, L192, L256),
    "A-v-le-2t4": (G, L128, L192, L256),
    "A-v-le-t1": (G, L128, L192, L256),
    "A-v-t1+1": (G, L128, L192, L256),
    "A-v-le-2t1": (G, G, L192, L256),
    "A-v-le-2t1+3": (G, G, L192, L256),
    "A-v-gt-2t1+3": (G, G, G, L256),
    "N-v-le-t4": (L64, L128, L192, L256),
    "B-v-le-2t4": (G, L128, L192, L256),
    "B-v-t1+1": (G, L128, L192, L256),
    "B-v-le-2t1+3": (G, G, L192, L256),
}
# batch -> (threads, LDS window in bytes, kernel of a general context, kernel of a context without elem_rank) in the shape the library chooses itself
NATURAL = {
    "A-v-le-65": (64, 5376, W7, L64),
    "A-v-le-t4": (64, 7328, G, G),
    "A-v-le-2t4": (64, 8000, G, G),
    "A-v-le-t1": (128, 8000, W7, L128),
    "A-v-t1+1": (128, 7184, W7, L128),
    "A-v-le-2t1": (128, 12288, G, G),
    "A-v-le-2t1+3": (128, 12304, G, G),
    "A-v-gt-2t1+3": (256, 24176, G, L256),  # 2 153 rows: three waves by the rows, four by the window (more than a seventh of the CU's LDS)
    "N-v-le-t4": (64, 5264, W7, L64),
    "B-v-le-2t4": (64, 7840, G, G),
    "B-v-t1+1": (128, 7056, W7, L128),
    "B-v-le-2t1+3": (128, 12528, G, G),
}
