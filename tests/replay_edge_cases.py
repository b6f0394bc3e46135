"""The patch replay (ptx_replay_walk, peritext_amd/csrc/replay_core.h, over the LDS store of that file and the HBM store of replay_hbm_core.h) at the exact positions
it branches on: the cases tests/test_emu_replay_edges.py (CPU emulation, every store, every lane order) and tests/test_gpu_replay_edges.py (the library on the GPU,
every build) share.

Every size comes from the constants below, which mirror the two headers (test_emu_replay_edges.py holds them to the header text): a word of `defined` is 32
boundary slots = 16 elements; one lane pass is 64 words = 2 048 slots = 1 024 elements; PTX_RCHUNK = 32 rows are resolved together; PTX_HBM_TILE = 1 024 words =
16 384 elements of a mark op's range are worked through at a time; `present` prefixes restart per block of 64 words (2 048 elements) and per superblock of 64
blocks (131 072 elements).  Expected streams come only from the in-repo oracle (helpers.oracle_apply(..., patches=True)), ONE run for the whole suite (about
14 s for the 229 documents, see suite()), never from a build of the kernel; family K's two long documents have answers known without it.

Documents are built by Doc: n elements named by their FINAL rank (the replay's state is indexed by final rank: boundary slot = 2 * rank + side, side 0 = before,
1 = after), all typed by one actor, a chosen few of them (`late`) inserted later, a chosen set deleted.  A mark op is stated by the slots it aims at
(Doc.by_slots); every case records them (`aims`) and the emulation test holds them to the merge's resolved references (res.ref_slots).  The reference's boundary
rule (changeMark): every mark starts `before` an element; strong / em end `before` one (even slots) or at endOfText, link / comment end `after` one (odd slots).

  W  slot-word edges: marks that start and end at slots 30 .. 34 and 62 .. 66, per type, in documents of 15 .. 49 elements; late inserts left / right of the edge
  Z  zero-width patches and open_top: two defined slots with only tombstones between (dropped) or exactly one visible char (kept)
  L  ops that lose: concurrent ops of one type, the larger ids applied first, tables of 1 / 63 / 64 / 65 / 129 applied ops; each with the actors' names swapped
  C  comments: 31 .. 65 comment ops, an id added / removed / added, a removeMark of an unknown id, inserts under 1 / 64 / 65 live ids, the id Kid - 1
  R  row chunks: logs of 1 .. 65 rows, mark ops at rows 31 / 32 / 63 / 64, and a 97-row log of one op per change for the tails (first_row)
  X  capacity: logs inside their guessed capacity, through both overflow extents, and past them (second launch)
  P  lane-pass, summary and tile edges: 511 .. 16 400 elements
  K  known answers: the 32 767-char ballast that selects the wide build, and a document of more than one superblock

_grouped() puts them into batches by replay working set (ptx_replay_lds_need_hdr), fewer than 64 logs each: the host shapes a launch by its largest log, so a batch at or below
5 632 bytes runs the plain build, one above it the _gwin build (the plain one under PTX_FLAG_REPLAY_LDS_ONLY); the "+big" batches put one 1 025-element document
beside small edge logs, which steers those through _gwin too.  NEED is the literal table of the largest needs; build_of() the context -> build mapping."""
import bisect
import dataclasses
import functools

import helpers as H
import replay_hbm_docs as D
from lww_edge_cases import rename_actors
from peritext_amd import wire

WORD = 32         # boundary slots per word of `defined` / `mb` (one word per lane): 16 elements
LANES = 64        # one lane pass: 64 words = 2 048 slots = 1 024 elements
RCHUNK = 32       # PTX_RCHUNK
HBM_TILE = 1024   # PTX_HBM_TILE, words: 16 384 elements
BLOCK_WORDS = 64  # words of `present` (32 elements each) per block of the HBM store: 2 048 elements; 64 blocks per superblock
SUPERBLOCK = BLOCK_WORDS * 64 * 32  # 131 072 elements
GWIN_ABOVE = 5632  # PTX_REPLAY_GWIN_ABOVE (peritext_hip.hip): the largest working set of a launch above which the host takes the _gwin build
LDS_CU = 160 * 1024
WIDE_ABOVE = 32766  # ptx_replay_wants_wide: more elements than this (or more than 65 534 rows) and the whole launch takes the wide build
TYPES = ("strong", "em", "link", "comment")
NONE16 = 0xFFFF


class Doc:
    """n elements named by final rank; those of `late` are inserted by insert(r) (directly behind the closest existing element to their left, where RGA puts
    the newest element), the others typed in order in the first change.  per_op: every op is a change of its own (every prefix of the log is then a log)."""

    def __init__(self, n, late=(), per_op=False, actor="a"):
        self.n, self.actor, self.per_op = n, actor, per_op
        self.ops = [{"opId": "1@%s" % actor, "action": "makeList", "obj": "_root", "key": "text"}]
        self.id_of, self.have, self.aims = {}, [], []
        self.late = set(late)
        prev = "_head"
        for r in range(n):
            if r not in self.late:
                prev = self._op({"action": "set", "elemId": prev, "insert": True, "value": "abcdefghijklmnopqrstuvwxyz"[r % 26]})
                self.id_of[r] = prev
                self.have.append(r)
        self.n_first = len(self.ops)

    def _op(self, op):
        o = dict(op, opId="%d@%s" % (len(self.ops) + 1, self.actor), obj="1@%s" % self.actor)
        self.ops.append(o)
        return o["opId"]

    def insert(self, r, value="X"):
        assert r in self.late and r not in self.id_of
        k = bisect.bisect_left(self.have, r)
        self.id_of[r] = self._op({"action": "set", "elemId": self.id_of[self.have[k - 1]] if k else "_head", "insert": True, "value": value})
        self.have.insert(k, r)

    def delete(self, r):
        self._op({"action": "del", "elemId": self.id_of[r]})

    def by_slots(self, action, ty, sa, sb, tag="t", rule=True):
        """a mark op from boundary slot sa to slot sb (None: endOfText).  rule: the slots are ones changeMark can produce for the type"""
        assert not rule or (sa % 2 == 0 and (sb is None or sb % 2 == (0 if ty in ("strong", "em") else 1))), (ty, sa, sb)
        b = lambda s: {"type": "after" if s & 1 else "before", "elemId": self.id_of[s >> 1]}  # noqa: E731
        op = {"action": action, "markType": ty, "start": b(sa), "end": {"type": "endOfText"} if sb is None else b(sb)}
        if ty == "link" and action == "addMark":
            op["attrs"] = {"url": "%s.example" % tag}
        if ty == "comment":
            op["attrs"] = {"id": tag}
        self.aims.append((len(self.ops), sa, NONE16 if sb is None else sb))
        self._op(op)

    def span(self, action, ty, lo, hi, tag="t"):
        """over the elements of final rank [lo, hi) by the boundary rule (hi = None: to endOfText)"""
        self.by_slots(action, ty, 2 * lo, None if hi is None else 2 * hi if ty in ("strong", "em") else 2 * hi - 1, tag)

    def log(self, foreign=None):
        """the replica's log; foreign: (changes of other actors, applied between this actor's first change and the rest); rows of the aims follow"""
        a = self.actor
        if self.per_op:
            assert foreign is None
            return [{"actor": a, "seq": k + 1, "deps": {}, "startOp": k + 1, "ops": [op]} for k, op in enumerate(self.ops)]
        log = [{"actor": a, "seq": 1, "deps": {}, "startOp": 1, "ops": self.ops[:self.n_first]}]
        shift = 0
        for ch in foreign or ():
            log.append(ch)
            shift += len(ch["ops"])
        if len(self.ops) > self.n_first:
            log.append({"actor": a, "seq": 2, "deps": {a: 1}, "startOp": self.n_first + 1, "ops": self.ops[self.n_first:]})
        self.aims = [(row + shift, sa, sb) for row, sa, sb in self.aims]
        return log


@dataclasses.dataclass
class Case:
    id: str
    logs: list             # the document: its replicas' logs (one each here)
    aims: list = None      # of log 0: (row, start slot, end slot or NONE16) of every mark op built by slots
    note: dict = dataclasses.field(default_factory=dict)
    expected: list = None  # per log, the oracle's {patches, spans, text}

    @property
    def family(self):
        return self.id[0]


def _case(cid, doc, foreign=None, **note):
    log = doc.log(foreign)
    return Case(cid, [log], doc.aims, note)


def _flip(k):
    return "addMark" if k % 2 == 0 else "removeMark"


# ---- W: slot-word edges ----
W_SIZES = (15, 16, 17, 31, 32, 33, 47, 48, 49)
W_EDGES = (32, 64)


def _w_round(d, ty, ok, k0):
    """the shapes of family W over the elements `ok` says exist; returns the number of ops made"""
    even = ty in ("strong", "em")
    k = [k0]

    def put(sa, sb):
        if ok(sa >> 1) and (sb is None or ok(sb >> 1)):
            tag = "u%d" % (k[0] % 2) if ty == "link" else "c%d" % (k[0] % 3)
            d.by_slots(_flip(k[0] // 2 if ty == "comment" else k[0]), ty, sa, sb, tag)  # (comments: add, add, remove, remove, ... over three ids)
            k[0] += 1

    ends = lambda e: (e - 2, e, e + 2) if even else (e - 1, e + 1, e + 3)  # noqa: E731
    for e in W_EDGES:
        for s in (e - 2, e, e + 2):
            put(s, None)                 # starts beside the edge, ends at endOfText
        for x in ends(e):
            put(0, x)                    # [0, 32) exactly one whole word; ending at 30 .. 34 (31, 33, 35 for the `after` types)
        put(e, e if even else e - 1)     # start == end: the start test fires first (the `after` types: end one slot before the start)
        put(e + 2, e if even else e + 1)  # end before start: covers nothing, defines the end slot
    for s in (30, 32, 34):
        for x in ends(64):
            put(s, x)
    return k[0] - k0


def _w_cases():
    out = []
    for side, lates in (("right", (16, 32)), ("left", (15, 31))):
        for n in W_SIZES:
            for ty in TYPES:
                late = [r for r in lates if r < n]
                d = Doc(n, late)
                k = _w_round(d, ty, lambda r: r < n and r not in late, 0)
                for r in late:  # read the inherited marks across (right) or just below (left) the word edge
                    d.insert(r)
                _w_round(d, ty, lambda r: r < n, k + 1)
                out.append(_case("W-%s-n%d-%s" % (side, n, ty), d, n=n, ty=ty))
    return out


# ---- Z: zero-width patches, open_top ----
Z_N = 130
# name -> (s1, s2, ranks where one visible char is left for the "kept" variants).  The elements of rank [s1 / 2, (s2 + 1) / 2) lie between the two slots.
Z_RUNS = {
    "inside": (36, 44, (19,)),           # both slots in word 1
    "to-last-slot": (40, 63, (20, 31)),  # the run ends at the last slot of word 1 (an `after` slot)
    "from-first-slot": (64, 80, (32, 39)),  # ... starts at the first slot of word 2
    "span1": (62, 98, (32, 47)),         # s1 the highest defined slot of word 1, word 2 wholly empty, s2 in word 3: one char at the first / last rank of word 2
    "span2": (62, 130, (32, 47)),        # two empty words
    "span5": (62, 226, (32, 47)),        # five
    "halves": (20, 70, (15, 16, 31, 32)),  # the char at rank 15 / 16 / 31 / 32: the low or high half of a `present` word (w & 1)
}


def _z_doc(ty, mode, s1, s2, keep):
    d = Doc(Z_N)
    other = "em" if ty != "em" else "strong"
    if mode == "remove-over-on":
        d.span("addMark", ty, 0, None, "z")
    # s2 becomes a defined slot without a change to `ty`: an op of another type whose end is met before its start defines the end slot only
    d.by_slots("addMark", other if s2 % 2 == 0 else "link", 2 * (Z_N - 1), s2, "definer")
    for r in range(s1 >> 1, (s2 + 1) >> 1):
        if r != keep:
            d.delete(r)
    end = s2 + 12
    end += 1 if (end % 2 == 0) != (ty in ("strong", "em")) else 0  # (six elements behind s2, by the type's boundary rule)
    d.by_slots("addMark" if mode == "add-over-off" else "removeMark", ty, s1, end, "z")
    return d


def _z_cases():
    out = []
    for ty in ("strong", "comment"):
        for mode in ("add-over-off", "remove-over-on"):
            for name, (s1, s2, keeps) in Z_RUNS.items():
                for keep in (None,) + keeps:
                    cid = "Z-%s-%s-%s-%s" % (ty, mode, name, "dropped" if keep is None else "kept%d" % keep)
                    out.append(_case(cid, _z_doc(ty, mode, s1, s2, keep), s1=s1, s2=s2, twin=None if keep is None else cid.rsplit("-", 1)[0] + "-dropped"))
    return out


# ---- L: ops that lose ----
L_N = 82
L_TABLES = (1, 63, 64, 65, 129)
L_KEYS = {True: ((32, 96), (30, 64), (34, 66), (32, 64), (98, 128)), False: ((32, 97), (30, 63), (34, 65), (32, 33), (98, 127))}  # even ends / odd ends
L_MINE = {True: ((10, 130), (40, 70), (32, 64), (30, 66), (0, None), (64, 96), (20, 34), (62, 100)),
          False: ((10, 131), (40, 71), (32, 63), (30, 65), (0, None), (64, 97), (20, 33), (62, 101))}


def _l_docs(ty, T):
    """[the log as written, the same with the actors' names swapped].  `a` types the text; `b`, who knows only that, makes T ops of the type — counters from
    the first free one on — whose key intervals begin and end at slots 30 .. 34 / 62 .. 66 / 96 .. 98 and cover whole words between; `a` answers with eight ops of the SAME
    counters and two inserts.  The replica applies b's change first: a's op j meets a table of T + j applied ops and loses to every b op of a counter at least
    its own (b > a), of a larger one with the names swapped."""
    even = ty in ("strong", "em")
    late = (18, 36)  # (no op of the family names their slots)
    d = Doc(L_N, late)
    b = Doc(L_N, late, actor="a")  # (only to build b's ops with a's element ids)
    keys = sorted({0, T // 2, T - 1} | {i for i in (62, 63, 64) if i < T})
    for i in range(T):
        if i in keys:
            sa, sb = L_KEYS[even][keys.index(i) % 5]
            b.by_slots(_flip(keys.index(i) + 1), ty, sa, sb, "k%d" % (keys.index(i) % 2))  # (the first one removes where a's first op, of the same counter, adds)
        else:
            r = 70 + i % 8
            b.span("addMark", ty, r, r + 1, "f%d" % (i % 3))
    theirs = [dict(op, opId="%d@b" % (b.n_first + 1 + i)) for i, op in enumerate(b.ops[b.n_first:])]  # (the counters a's second change starts with)
    cb = {"actor": "b", "seq": 1, "deps": {"a": 1}, "startOp": b.n_first + 1, "ops": theirs}
    for j, (sa, sb) in enumerate(L_MINE[even]):
        d.by_slots(_flip(j), ty, sa, sb, "k%d" % (j % 2))
    for r in late:  # (links: the inserted chars inherit the winner's url)
        d.insert(r)
    log = d.log([cb])
    return [Case("L-%s-t%d-ab" % (ty, T), [log], d.aims, {"T": T, "ty": ty}),
            Case("L-%s-t%d-ba" % (ty, T), [rename_actors(log, {"a": "b", "b": "a"})], d.aims, {"T": T, "ty": ty})]


def _l_cases():
    return [c for ty in ("strong", "em", "link") for T in L_TABLES for c in _l_docs(ty, T)]


# ---- C: comments ----
C_KC = (31, 32, 33, 64, 65)
C_LIVE = (1, 64, 65)


def _c_cases():
    out = []
    for kc in C_KC:
        d = Doc(41, (20,))
        for i in range(kc - 7):
            d.span("addMark", "comment", 2 + i % 5, 29 + i % 7, "c%03d" % i)
        d.span("addMark", "comment", 5, 26, "x")      # one id added, removed and added again over overlapping ranges: the last-applied covering op decides
        d.span("removeMark", "comment", 10, 16, "x")
        d.span("addMark", "comment", 15, 31, "x")
        d.span("removeMark", "comment", 3, 13, "ghost")  # an id nobody added
        d.span("addMark", "comment", 18, 23, "zzz")    # the largest id of the document: Kid - 1
        d.span("removeMark", "comment", 0, 41, "c000")
        d.span("removeMark", "comment", 12, 24, "zzz")
        d.insert(20)
        out.append(_case("C-kc%d" % kc, d, kc=kc))
    for live in C_LIVE:
        d = Doc(41, (20, 21))
        for i in range(live):
            d.span("addMark", "comment", 10 - i % 3, 30 + i % 4, "i%03d" % i)
        d.insert(20)
        d.span("removeMark", "comment", 0, 41, "i000")
        d.insert(21)
        out.append(_case("C-live%d" % live, d, live=live))
    return out


# ---- R: row chunks and tails ----
R_ROWS = (1, 31, 32, 33, 63, 64, 65)
R_TAIL_ROWS = 97
R_MARK_ROWS = (31, 32, 63, 64, 95, 96)  # the last row of a chunk and the first of the next


def _r_doc(N, per_op=False):
    m = min(N - 1, 12)
    plan = ["mark" if t in R_MARK_ROWS else ("insert", "mark", "delete", "mark")[t % 4] for t in range(m + 1, N)]
    n = m + plan.count("insert")
    d = Doc(n, range(m, n), per_op=per_op)
    nxt = m
    for t, what in zip(range(m + 1, N), plan):
        if what == "insert":
            d.insert(nxt)
            nxt += 1
        elif what == "delete":
            d.delete((t * 7) % m)  # (typed in the first chunk; again and again: a tombstone gives no record)
        else:
            ty = TYPES[(t // 2) % 4]
            lo = (t * 3) % (m - 1)
            d.span(_flip(t // 8), ty, lo, None if t % 3 == 0 else min(lo + 1 + t % 5, m - 1), "r%d" % (t % 3))
    assert len(d.ops) == N
    return d


R_FIRST = (0, 1, 31, 32, 33, 64, R_TAIL_ROWS - 1, R_TAIL_ROWS, R_TAIL_ROWS + 5)


def _r_cases():
    out = [_case("R-rows%d" % N, _r_doc(N), rows=N) for N in R_ROWS]
    tail = _r_doc(R_TAIL_ROWS, per_op=True)
    log = tail.log()
    out.append(Case("R-tail%d" % R_TAIL_ROWS, [log], tail.aims, {"rows": R_TAIL_ROWS}))
    for f in R_FIRST:  # the prefixes: what the oracle has produced before row f is what a tail from f leaves out
        if 0 < f < R_TAIL_ROWS:
            out.append(Case("R-prefix%d" % f, [log[:f]], None, {"rows": f, "prefix": True}))
    return out


# ---- X: capacity ----
X_M = 100


def reserve_model(per_row, arena_cap):
    """ptx_replay_reserve restated for a whole stream (first_row = 0): per_row[t] records of row t -> (the extents taken: (chunk start, records), records
    produced, room at the end, records lost).  Capacity 2 N + 16; before the chunk at t0: rate = max(8, 3 * (npatch / (t0 + 1 or 1) + 1)); an extent is asked for
    while any is left, no record is lost yet and npatch + 32 * rate > room: rate (times 16 for the second) * (N - t0) + 1 024 records."""
    N = len(per_row)
    room, left, npatch, used, exts = 2 * N + 16, 2, 0, 0, []
    for t0 in range(0, N, RCHUNK):
        rate = max(8, 3 * (npatch // (t0 + 1 if t0 else 1) + 1))
        if npatch > room:  # records are lost already
            left = 0
        if left and npatch + rate * RCHUNK > room:
            want = rate * (1 if left == 2 else 16) * (N - t0) + 1024
            if used + want <= arena_cap:
                used, room, left = used + want, room + want, left - 1
                exts.append((t0, want))
            else:
                left = 0
        for r in per_row[t0:t0 + RCHUNK]:
            npatch += r
    return exts, npatch, room, max(0, npatch - room)


# The construction: X_M = 100 single-char strong marks on the even chars of 200 chars (every even slot 0 .. 400 becomes a defined one), 301 rows and 301 records so
# far; then rows of three kinds: "whole": an em toggle over the whole text, 200 records; ("part", q): a link over the first q chars with a url that alternates,
# q records; "quiet": a strong toggle on char 0, one record.
#   inside   301 + one whole op: N = 302, capacity 2 N + 16 = 620, 501 records.  Before the last chunk (t0 = 288): 288 + 32 * 8 = 544 <= 620: no extent.
#   extents  301 + 96 x part 12 + 64 x part 60 + 24 x whole: N = 485, capacity 986.  t0 = 320 (529 records): rate 8, 529 + 256 <= 986; t0 = 352 (913): rate
#            3 * (913 / 353 + 1) = 9, 913 + 288 > 986: first extent 9 * 133 + 1 024 = 2 221, room 3 207; t0 = 384 (1 297): rate 12, 1 681 <= 3 207; t0 = 416
#            (2 593): rate 3 * (2 593 / 417 + 1) = 21, 2 593 + 672 > 3 207: second extent 21 * 16 * 69 + 1 024 = 24 208; 10 093 records in the end, none lost.
#   burst    301 + three whole ops: N = 304, capacity 624; t0 = 288: 544 <= 624, no extent; the last chunk brings 901 records: 277 lost, PTX_ERR_CAPACITY, and the
#            host launches again with exact capacities.
#   burst-then-quiet  the same followed by 40 quiet rows: N = 344, capacity 704; the chunk at 288 ends at 917 records, 213 of them lost; before the chunk at 320
#            917 + 32 * 9 > 704 would ask for an extent — which would make room for the COUNT (941 <= 704 + 1 240: status 0) but not bring the lost records
#            back.  A log that has lost records takes no extent any more: 941 - 704 = 237 records beyond its room in the end, PTX_ERR_CAPACITY, and the second
#            launch.
X_LOGS = {
    "inside": ["whole"],
    "extents": [("part", 12)] * 96 + [("part", 60)] * 64 + ["whole"] * 24,
    "burst": ["whole"] * 3,
    "burst-then-quiet": ["whole"] * 3 + ["quiet"] * 40,
}
X_REGIME = {"inside": (0, 0), "extents": (2, 0), "burst": (0, 277), "burst-then-quiet": (0, 237)}  # name -> (extents taken, records lost in the first launch)


def x_per_row(name):
    return [1] * (1 + 3 * X_M) + [2 * X_M if r == "whole" else 1 if r == "quiet" else r[1] for r in X_LOGS[name]]


def _x_cases():
    out = []
    for name, rows in X_LOGS.items():
        d = Doc(2 * X_M)
        for k in range(X_M):
            d.span("addMark", "strong", 2 * k, 2 * k + 1)
        n = {"whole": 0, "quiet": 0, "part": 0}
        for r in rows:
            kind = r if isinstance(r, str) else r[0]
            if kind == "whole":
                d.span(_flip(n[kind]), "em", 0, None)
            elif kind == "quiet":
                d.span(_flip(n[kind] + 1), "strong", 0, 1)
            else:
                d.span("addMark", "link", 0, r[1], "u%d" % (n[kind] % 2))
            n[kind] += 1
        out.append(_case("X-%s" % name, d, per_row=x_per_row(name)))
    return out


# ---- P: lane-pass, summary and tile edges ----
P_SIZES = (511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 16383, 16384, 16400)
P_TILE_RUN = (16380, 16390)  # elements between a defined slot in the last word of the first tile and the next defined slot, in the next tile


def _p_doc(n, hollow=False):
    """hollow: the elements between the two slots around the tile edge are deleted (16 400 elements only)"""
    late = sorted({n // 2} | {r for r in (2040, 2048) if r < n and n >= 2049})
    d = Doc(n, late)
    d.span("addMark", "link", 5, n - 2, "far")   # two defined slots, 10 and 2 n - 5, with nothing defined between: more than 32 words apart from 513 elements on
    d.insert(n // 2)                             # ... inherits the link from slot 10: the search for the closest defined slot climbs the summaries
    d.span("addMark", "strong", 3, None)         # slot 6 opens a record; from slot 10 the next defined slot is the far one
    d.delete(7)
    d.delete(n - 2)
    if n >= 16400:  # more than 1 024 words apart, nothing defined between: slots 10 and 32 790 climb two levels
        d.span("removeMark", "link", 5, 16396)
    if n > LANES * 16:
        d.by_slots("removeMark", "strong", 0, 2 * LANES * 16)       # exactly 64 words: [0, 2 048)
    if n > (LANES + 1) * 16 + 15:
        d.by_slots("addMark", "em", 0, 2 * (LANES + 1) * 16)        # 65 words: [0, 2 080)
        d.by_slots("addMark", "comment", 32, 2 * (LANES + 1) * 16 + 31, "p")  # 65 words from the second on
    if n > P_TILE_RUN[1]:
        lo, hi = P_TILE_RUN
        if hollow:
            for r in range(lo, hi):
                d.delete(r)
        d.span("addMark", "em", lo, hi)  # defines slots 32 760 (word 1 023) and 32 780 (word 1 024)
    d.span("addMark", "comment", 0, None, "whole")       # whole-document ops: their records straddle the lane pass and (16 K elements) the tile edge
    d.span("removeMark", "strong", 0, None)
    d.span("addMark", "link", 0, n - 1, "far")            # the same url where the first link reaches, another state elsewhere: the per-slot url pass
    d.span("removeMark", "em", 1, None)
    if n >= 2049:  # an insert and a delete in words 63 and 64 of `present` (block edge of the HBM store), then ops that read visible indices across it
        d.insert(2040)
        d.insert(2048)
        d.delete(2041)
        if n > 2060:
            d.delete(2049)
        d.span("addMark", "em", 2030, min(2060, n) if n > 2060 else None)
        d.span("removeMark", "comment", 2047, None, "whole")
    d.span("addMark", "link", 2, n - 1, "other")
    return d


def _p_cases():
    out = [_case("P-n%d" % n, _p_doc(n), n=n) for n in P_SIZES]
    out.append(_case("P-n16400-hollow", _p_doc(16400, hollow=True), n=16400))
    return out


# ---- K: known answers without the oracle ----
K_BALLAST = WIDE_ABOVE + 1  # typed_log(32 767): one log of more elements than the narrow builds take makes the whole launch wide
K_SUPER_N = SUPERBLOCK + 130


def k_script(n, edge):
    """(the log, its patch stream by a plain list model): n chars typed in order; the elements at ranks 0, edge - 1, edge and n - 1 deleted; one strong mark from
    element edge - 72 to element edge + 78; a char inserted behind each deleted element's left neighbour (behind the head for rank 0)."""
    log = D.typed_log(n)
    ids = ["%d@doc1" % (2 + i) for i in range(n)]
    patches = [{"action": "makeList"}] + [{"path": ["text"], "action": "insert", "index": i, "values": ["abcdefghij"[i % 10]], "marks": {}} for i in range(n)]
    order = list(range(n))     # the list model: elements in document order (tombstones included) ...
    alive = [True] * n         # ... by element number: visible?
    ctr, seq, ops = n + 2, 2, []

    def index_of(pos):
        return sum(1 for e in order[:pos] if alive[e])

    def push(op):
        nonlocal ctr
        ops.append(dict(op, opId="%d@doc1" % ctr, obj="1@doc1"))
        ctr += 1

    dels = [0, edge - 1, edge, n - 1]
    for e in dels:
        push({"action": "del", "elemId": ids[e]})
        patches.append({"path": ["text"], "action": "delete", "index": index_of(order.index(e)), "count": 1})
        alive[e] = False
    lo, hi = edge - 72, edge + 78
    push({"action": "addMark", "markType": "strong", "start": {"type": "before", "elemId": ids[lo]}, "end": {"type": "before", "elemId": ids[hi]}})
    patches.append({"action": "addMark", "markType": "strong", "path": ["text"], "startIndex": index_of(order.index(lo)), "endIndex": index_of(order.index(hi))})
    for e in dels:
        pos = order.index(e)  # the new element goes directly behind the left neighbour: where the deleted element stands
        parent = order[pos - 1] if pos else None
        assert parent is None or parent < n  # (a typed element)
        push({"action": "set", "elemId": "_head" if parent is None else ids[parent], "insert": True, "value": "N"})
        # it takes the marks of the closest defined slot to its left: strong iff the mark's start stands before it and the mark's end does not
        strong = order.index(lo) < pos <= order.index(hi)
        patches.append({"path": ["text"], "action": "insert", "index": index_of(pos), "values": ["N"], "marks": {"strong": {"active": True}} if strong else {}})
        order.insert(pos, len(alive))
        alive.append(True)
    log.append({"actor": "doc1", "seq": seq, "deps": {}, "startOp": n + 2, "ops": ops})
    return log, patches


@functools.lru_cache(maxsize=None)
def k_super():
    return k_script(K_SUPER_N, SUPERBLOCK)


@functools.lru_cache(maxsize=None)
def k_ballast_log():
    return D.typed_log(K_BALLAST)


def typed_stream(n):
    """the known answer of typed_log(n)"""
    return [{"action": "makeList"}] + [{"path": ["text"], "action": "insert", "index": i, "values": ["abcdefghij"[i % 10]], "marks": {}} for i in range(n)]


K_MINI = (300, 150)


# ---- batches ----
@dataclasses.dataclass
class Batch:
    name: str
    cases: list
    batch: wire.Batch
    expected: list     # per document: [the oracle's answer per log]
    case_of_log: list
    big: bool = False  # beyond what the merge kernel holds in one CU's LDS: the emulation merges it through the HBM-staged path


STEERED = ("W-right", "Z-comment", "L-link", "C", "R")  # the small batches that also run beside one 1 025-element document ("+big": the _gwin build by default)


def _grouped(cases):
    by = lambda pred: [c for c in cases if pred(c)]  # noqa: E731
    groups = [("W-%s" % s, by(lambda c, s=s: c.id.startswith("W-%s-" % s))) for s in ("right", "left")]
    groups += [("Z-%s" % t, by(lambda c, t=t: c.id.startswith("Z-%s-" % t))) for t in ("strong", "comment")]
    groups += [("L-%s" % t, by(lambda c, t=t: c.id.startswith("L-%s-" % t))) for t in ("strong", "em", "link")]
    groups += [("C", by(lambda c: c.family == "C")), ("R", by(lambda c: c.family == "R" and not c.note.get("prefix") and "tail" not in c.id))]
    groups += [("R-tail", by(lambda c: c.id.startswith("R-tail")))]
    groups += [("X-%s" % n, by(lambda c, n=n: c.id == "X-%s" % n)) for n in X_LOGS]
    groups += [("X", by(lambda c: c.family == "X"))]
    groups += [("P-small", by(lambda c: c.family == "P" and c.note["n"] <= 1025)), ("P-mid", by(lambda c: c.family == "P" and 1025 < c.note["n"] <= 2049)),
               ("P-big", by(lambda c: c.family == "P" and c.note["n"] > 2049))]
    big = next(c for c in cases if c.id == "P-n1025")
    groups += [(name + "+big", mine + [big]) for name, mine in groups if name in STEERED]
    for name, mine in groups:
        assert mine and len(mine) < 64, name
    return groups


@functools.lru_cache(maxsize=None)
def _cases():
    return _w_cases() + _z_cases() + _l_cases() + _c_cases() + _r_cases() + _x_cases() + _p_cases()


@functools.lru_cache(maxsize=None)
def batch_names():
    return [name for name, _ in _grouped(_cases())]


ORACLE_SECONDS = {}


@functools.lru_cache(maxsize=None)
def suite():
    """Every case with the oracle's answer — ONE run of the oracle for all of them and the miniature of family K — and the batches they run in.  Shared by every
    test of a session: treat as read-only."""
    import time

    assert H.have_node(), "the expected streams come from the oracle, which needs node: a skipped suite would hide exactly what these files exist to show"
    cases = _cases()
    mini_log, mini_patches = k_script(*K_MINI)
    t0 = time.time()
    answers = H.oracle_apply([c.logs for c in cases] + [[mini_log]], patches=True, timeout=1800)
    ORACLE_SECONDS["run"] = time.time() - t0
    for c, exp in zip(cases, answers):
        assert len(exp) == len(c.logs) and all("error" not in e for e in exp), c.id
        c.expected = exp
    # the list model of family K against the oracle on a 300-element miniature of the same script
    assert H.norm_patches(answers[-1][0]["patches"]) == H.norm_patches(mini_patches), "k_script's list model"
    batches = []
    for name, mine in _grouped(cases):
        b = wire.encode_docs([c.logs for c in mine])
        batches.append(Batch(name, mine, b, [c.expected for c in mine], [c.id for c in mine for _ in c.logs], big=name == "P-big"))
        assert b.n_logs == len(mine) < 64
    assert [b.name for b in batches] == batch_names()
    return cases, batches


def batches():
    return suite()[1]


def batch(name):
    return next(b for b in batches() if b.name == name)


def case(cid):
    return next(c for c in suite()[0] if c.id == cid)


def check_batch(b, pat, logs=None):
    """status, n_patches and every decoded patch of every log, in order, against the oracle (the comment ids of one insert, which an atomic counter places, in
    id order: wire.decode_patches sorts them)"""
    for log, (cid, exp) in enumerate(zip(b.case_of_log, b.expected)):
        if logs is not None and log not in logs:
            continue
        assert int(pat.logs["status"][log]) == 0, "%s (batch %s): status %d" % (cid, b.name, int(pat.logs["status"][log]))
        want = H.norm_patches(exp[0]["patches"])
        assert int(pat.logs["n_patches"][log]) == len(pat.of_log(log)), cid
        got = H.norm_patches(wire.decode_patches(b.batch, pat, log))
        assert len(got) == len(want), "%s (batch %s): %d patches, expected %d" % (cid, b.name, len(got), len(want))
        for i, (x, y) in enumerate(zip(got, want)):
            assert x == y, "%s (batch %s) patch %d: %r != %r" % (cid, b.name, i, x, y)


def tail_expected(first):
    """the oracle's records of R-tail's rows from `first` on: its whole stream without what it produced for the prefix of `first` one-op changes"""
    whole = case("R-tail%d" % R_TAIL_ROWS).expected[0]["patches"]
    if first <= 0:
        return whole
    if first >= R_TAIL_ROWS:
        return []
    return whole[len(case("R-prefix%d" % first).expected[0]["patches"]):]


def rebatched(b, batch):
    """the Batch with another encoding of its documents (with_ballast's)"""
    return dataclasses.replace(b, batch=batch)


def with_ballast(b):
    """the batch with typed_log(32 767) appended as one more document: (wire.Batch, log index of the ballast)"""
    return wire.encode_docs([c.logs for c in b.cases] + [[k_ballast_log()]]), len(b.cases)


# ---- which build a batch runs in ----
def lds_need(n, K, Kc, Kid, gscratch=False, wide=False):
    """ptx_replay_lds_need (replay_core.h) restated: the header (48 bytes), `present` (8 bytes a word of 32 elements), defined / mb / cw / cnt (4 + 16 + 4 + 4
    bytes a word of 32 slots), the chunk buffers, the comment ops' intervals, chains and add bits, and — unless they live in global memory (gscratch: the
    _gwin and _wide builds) — the per-slot urls, the table of applied LWW ops, the comment ops' ids and the last op per id; every array 16-byte aligned.
    test_emu_replay_edges.py holds it to the emulation library's exports in the two forms they give (everything in the LDS; wide with gscratch)."""
    a16 = lambda x: (x + 15) & ~15  # noqa: E731
    nwe, nws, Kl, sw = (n >> 5) + 2, ((2 * n + 2) >> 5) + 2, K - Kc, 4 if wide else 2
    tables = 0 if gscratch else a16(4 * (2 * n + 2)) + a16((16 if wide else 8) * (Kl + 1)) + a16(2 * (Kc + 1)) + a16(2 * (Kid + 1))
    return (a16(48) + a16(8 * nwe) + a16(4 * nws) + a16(16 * nws) + 2 * a16(4 * (nws + 1)) + tables + a16((24 if wide else 16) * RCHUNK) + a16(RCHUNK)
            + 2 * a16(sw * (Kc + 1)) + a16(2 * (Kc + 1)) + a16(4 * ((Kc >> 5) + 1)))


def lds_need_of(batch, log, gscratch=False, wide=False):
    """ptx_replay_lds_need_hdr of one log of a wire.Batch"""
    from peritext_amd import abi

    h = batch.log_hdr[log]
    Kc = int(h["n_mark"][abi.MARK_COMMENT])
    return lds_need(int(h["n_ins"]), int(h["n_mark"].sum()), Kc, int(h["n_comment_ids"]) if Kc else 0, gscratch, wide)



# batch -> (largest ptx_replay_lds_need_hdr of its logs with everything in the LDS, the same with the tables in global memory), bytes
NEED = {
    "W-right": (1600, 1056), "W-left": (1632, 1056), "Z-strong": (2128, 1008), "Z-comment": (2112, 1008), "L-strong": (2704, 896), "L-em": (2704, 896),
    "L-link": (2704, 896), "C": (1856, 1216), "R": (1168, 768), "R-tail": (1408, 816), "X-inside": (3600, 1136), "X-extents": (5072, 1136), "X-burst": (3616, 1136),
    "X-burst-then-quiet": (3936, 1136), "X": (5072, 1136),
    "P-small": (11104, 2800), "P-mid": (21360, 4848),
    "P-big": (164880, 33536),  # with everything in the LDS beyond one CU's 163 840 bytes: the HBM-state kernel under PTX_FLAG_REPLAY_LDS_ONLY
    "W-right+big": (11104, 2800), "Z-comment+big": (11104, 2800), "L-link+big": (11104, 2800), "C+big": (11104, 2800), "R+big": (11104, 2800),
}


def build_of(name, context):
    """the replay kernel of every log of a batch by the host's rule (ptx_replay_patches, peritext_hip.hip) in the contexts of test_gpu_replay_edges.py"""
    plain, gwin = NEED[name]
    if context == "hbm":
        return "ptx_replay_kernel_hbm"
    if context == "ballast":
        return "ptx_replay_kernel_wide"
    if context == "lds-only":
        return "ptx_replay_kernel" if plain <= LDS_CU else "ptx_replay_kernel_hbm"
    return "ptx_replay_kernel" if plain <= GWIN_ABOVE else "ptx_replay_kernel_gwin" if gwin <= LDS_CU else "ptx_replay_kernel_hbm"
