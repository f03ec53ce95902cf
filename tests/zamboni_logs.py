"""Hand-built logs that force every branch of zamboni's append rules (scourNode mergeTree.ts:1322-1398, pack
1401-1453, canAppend textSegment.ts:63-68 / sharedSequence.ts:57-60 / permutationvector.ts:87-93) — test
infrastructure for tests/test_ref_zamboni.py and tools/make_ref_goldens.py --zamboni.

The generator never inserts more than 8 units at a time, so on its logs the length half of canAppend
(TextSegmentGranularity 256, SubSequence MaxRun 128) is always true. Here every case is one small document:
its rows are inserted under a minSeq that stays at 0 (they sit in the collaboration window, one zamboni heap
entry per leaf: addToLRUSet queues a block once, under the seq of its first edit), then NOOPs move the minSeq
past them (`cut`: the index of the first such record) and, with a minSeq that keeps rising (setMinSeq calls
zamboni only when it moves), drain the heap two entries per call. A leaf is scoured once per step: a scoured
block is not scoured again until an edit lands in it.

Each case carries the branch it forces and a witness: a predicate over the parsed canonical dump of the
REFERENCE (oplog.parse_dump) that proves the branch was taken. Lengths below are adjacent rows of one leaf in
document order, equal properties, no newline, unless stated.

Case list (name: rows -> result; the branch)

Granularity, text (TextSegmentGranularity 256; the serial part of scour_par's walk: the run grows)
  g_256_256: [256,256] -> 512; both sides <= 256
  g_257_257: [257,257] apart; both sides > 256
  g_257_256: [257,256] -> 513; g_256_257: [256,257] -> 513; one side <= 256
  g_run_grows: [100,100,100,300] -> [300,300]; the run is 300 long when it meets the last row (a per-pair test
      of the rows' own lengths would merge all four)
  g_run_256: [200,56,300] -> 556; g_run_257: [200,57,300] -> [257,300]; the run reaches 256 / 257
  g_long_short_long: [300,100,300] -> [400,300]
  g_refused_restarts: [300,300,10] -> [300,310]; a refused row becomes prevSegment
  g_refused_mid: [300,300,300,5,300] -> [300,300,305,300]
Granularity, SubSequence (MaxRun 128; a {items} document): s_128_128 -> 256, s_129_129 apart, s_129_128 /
  s_128_129 -> 257, s_run_grows [50,50,50,150] -> [150,150], s_run_128 [100,28,150] -> 278, s_run_129
  [100,29,150] -> [129,150], s_long_short_long [150,50,150] -> [200,150], s_refused_restarts [150,150,10] ->
  [150,160], s_refused_mid [150,150,150,5,150] -> [150,150,155,150]
Granularity, PermutationSegment: perm_300_300: two unallocated rows of 300 -> 600 (no length rule)
Newline
  nl_tail: ["ab","c\\n","de"] -> ["abc\\n","de"]; the newline test runs on a run whose tail came from an appended
      row (RF_NLK / RF_NL hand-over)
  nl_split_left: "a\\nb" split at 2 by an insert that is removed and unlinked by a first step; a later row "cd"
      and a second step: ["a\\n","bcd"]; the left part of a split ends with a newline its whole did not
  nl_split_right: "ab\\n" split at 1 the same way: ["ab\\n","cd"]; "a" + "b\\n" merges, the next row stays apart
  s_nl_tail: the items [[1,2],[3,10],[4,5]] of a SubSequence document (unit 10 is "\\n") -> one row of 6
Markers: mk_between ["ab",M,"cd","ef"] -> ["ab",M,"cdef"]; mk_first [M,"ab","cd"] -> [M,"abcd"]; mk_last
  ["ab","cd",M] -> ["abcd",M]: nothing appends to a marker or is appended onto one
prevSegment resets
  rs_unlinked: [A,R,B], R removed at the minSeq: R is unlinked, A and B stay apart (the leaf is scoured once)
  rs_held: [A,H,B], H above the minSeq at the step: three rows
  rs_pending: [A,P,B], P a local pending insert of the replica (long id 5): three rows, P unacked
  rs_pending_acked: the same, then P's ack and a second step: one row
  A zero-length right part of a split is left in a leaf only by insertAtReferencePositionLocal on a reference
  past its segment's end (MT_OPF_ATREF records, local references on): the refrefs fixtures hold such inserts
  (tests/test_ref_refs.py, atref_past_end); sequenced ops alone never leave one, so no case here builds one.
Properties
  pr_equal: three rows with {k0: 1} -> one row
  pr_ninth_key: rows A, B, C with ten keys k0..k9; A and B agree on k0..k8's values and differ in k9, B and C are
      equal: [A, B+C]; matchProperties compares past the first group of 8 key slots (profiles with 24 key slots)
  pr_one_side: A with {k0: 1}, B and C without -> [A, B+C]
Leaf boundaries
  lb_two_leaves: nine rows of 20 appended: leaves of 4 and 5 after the 8 -> 4+4 split. The step scours the first
      leaf (one row left: underflow), pack scours both leaves in one wave and joins them into one leaf: two rows,
      80 and 100, in the same leaf (the witness uses `leaf`), not merged: no pair across a leaf boundary in a
      scour. pk_long_runs shows the same over 7 leaves.
Pack (a root whose sibling leaves' rows all become mergeable at one step; the scour of the first popped leaf leaves
fewer than 4 rows, so pack scours every sibling in one wave and redistributes). A block that reaches 8 children
splits at once (blockInsert), so a parent holds at most 7 leaves of at most 7 rows at rest: the cases build 7
leaves, not 8. The rows are prepended, so row order is the reverse of arena order, and the one heap entry (the
block was queued once, before its splits) names the oldest row, in the last leaf.
  pk_long_runs: 31 rows of 7: leaves of 7,4,4,4,4,4,4. The last leaf is scoured alone (4 jobs), then the wave over
      all 7 plans, per run, "both to top" (2 copy jobs) then "extend at top" (1 each): 7 jobs for the first leaf
      and 4 for each of five more, 27 jobs in one walk. After: 7 rows (49, then 28 x 6) in ONE leaf, every one
      short enough to append to its neighbour, none appended: no pair across a leaf boundary in the wave
  pk_pairs: 30 rows "?x","?y\\n" alternating: leaves of 6,4,4,4,4,4,4. Runs of exactly two, each "both to top": 2
      jobs a pair, 13 pairs in the wave: 26 jobs in one walk. After: 15 rows in 3 leaves of 5
  The flush at nj > W::N - 2 (more than 62 jobs) is not reached by either, and cannot be reached from any log: a
  wave scours at most 8 leaves of 8 rows; pack only follows the scour of one of them, which leaves that leaf
  nothing to append; a run of r rows plans at most r jobs (2 for its first append, 1 for each later one), so the
  other leaves plan at most 7 x 8 = 56 jobs (42 with the 7-by-7 bound above).
Arena branches (visible only through wrong text: the witness is the text)
  ar_both_to_top: [60,60,60,60] inserted second, first, third, fourth: the head's text is neither at the arena top
      nor followed by its successor's: "both to top", then "extend at top" twice
  ar_prepend: [60,60,60,60] prepended: the head's text is the last in the arena: "extend at top" three times
  ar_append: [60,60,60,60] appended: "already contiguous" three times
  pk_pairs / pk_long_runs with a small arena (ARENA_CASES; acap chosen in tests/test_ref_zamboni.py small_arena
  from the host core's arena_top before and after the step): the arena compacts in the middle of the pack's walk,
  with copies still planned and heads already moved to the top ("GC in the middle of the walk")
"""
from __future__ import annotations

from typing import Callable, List, NamedTuple, Optional

from fluidframework_amd import oplog as ol

LOCAL = 5  # the long id of the replica in the local-pending cases
NL_ITEM = 10  # a SubSequence unit equal to "\n"
ALL = frozenset({"small", "matrix", "flat", "tiled"})
WIDE_KEYS = frozenset({"flat", "tiled"})  # profiles with 24 property key slots per document


class Case(NamedTuple):
    name: str
    branch: str
    log: ol.DocLog
    cut: int            # index of the first record that moves the minSeq
    witness: Callable   # (hdr, segs) -> bool, over the parsed canonical dump
    profiles: frozenset
    kind: str           # "text" | "run" | "perm"


def _txt(n: int, salt: int) -> str:
    return "".join(chr(97 + (salt * 7 + j * (1 + salt % 3)) % 26) for j in range(n))


def _items(n: int, salt: int) -> list:
    return [11 + (salt * 13 + j) % 200 for j in range(n)]


class _Doc:
    """Sequenced records of client 1 (refSeq = seq - 1) under a held minSeq, then steps of NOOPs."""

    def __init__(self, it: ol.Interner, local: int = 0):
        self.log = ol.DocLog(it, local_long_id=local)
        self.seq = 0
        self.min = 0
        self.length = 0
        self.cut: Optional[int] = None

    def _hdr(self, client):
        self.seq += 1
        return dict(client=client, seq=self.seq, ref_seq=self.seq - 1, min_seq=self.min)

    def ins(self, pos: int, text=None, items=None, perm=None, marker=None, props=None, client: int = 1):
        self.log.add(ol.OP_INSERT, pos1=pos, text=text, items=items, perm=perm, marker=marker, props=props,
                     **self._hdr(client))
        self.length += 1 if marker is not None else perm if perm is not None else len(items if items is not None
                                                                                     else text)

    def rem(self, a: int, b: int, client: int = 1):
        self.log.add(ol.OP_REMOVE, pos1=a, pos2=b, **self._hdr(client))
        self.length -= b - a

    def local_ins(self, pos: int, text: str):
        self.log.add(ol.OP_INSERT | ol.OPF_LOCAL, pos1=pos, text=text)
        self.length += len(text)

    def ack_ins(self, pos: int, text: str, ref_seq: int):
        self.seq += 1
        self.log.add(ol.OP_INSERT, client=self.log.local_long_id, seq=self.seq, ref_seq=ref_seq, min_seq=self.min,
                     pos1=pos, text=text)

    def step(self, to: Optional[int] = None, drain: int = 6):
        """NOOPs: the minSeq moves to `to` (default: the last record's seq), then rises by one per NOOP."""
        if self.cut is None:
            self.cut = len(self.log.ops)
        to = self.seq if to is None else to
        for i in range(drain):
            self.seq += 1
            self.min = min(self.seq - 1, to + i)
            self.log.add(ol.OP_NOOP, client=1, seq=self.seq, ref_seq=self.seq - 1, min_seq=self.min)

    def rows(self, specs, order: str = "append", **kw):
        """Insert the rows `specs` (document order): appended one after another, or prepended last to first (the
        arena then holds them in reverse document order). A spec: str (text), list (items), int (a
        PermutationSegment's row count), None (a marker), or (spec, props)."""
        seq = list(specs) if order == "append" else list(reversed(specs))
        for s in seq:
            props = None
            if isinstance(s, tuple):
                s, props = s
            pos = self.length if order == "append" else 0
            if s is None:
                self.ins(pos, marker=0, props=props, **kw)
            elif isinstance(s, str):
                self.ins(pos, text=s, props=props, **kw)
            elif isinstance(s, list):
                self.ins(pos, items=s, props=props, **kw)
            else:
                self.ins(pos, perm=s, props=props, **kw)


def _lens(want):
    return lambda hdr, segs: [s["len"] for s in segs] == list(want)


def _texts(want):
    return lambda hdr, segs: [s["text"] for s in segs] == list(want)


def _merged(specs, groups):
    """The rows `specs` merged by `groups` (row counts): the texts / item lists / lengths of the result"""
    out, i = [], 0
    for g in groups:
        part = specs[i: i + g]
        i += g
        out.append(sum(part) if isinstance(part[0], int) else "".join(part) if isinstance(part[0], str)
                   else [x for p in part for x in p])
    assert i == len(specs)
    return out


def _content(want):
    """witness: the rows' contents (texts, item ids, PermutationSegment lengths) are exactly `want`"""
    def w(hdr, segs):
        got = []
        for s in segs:
            got.append(s["text"] if s["kind"] == ol.SEG_TEXT else s["items"] if s["kind"] == ol.SEG_RUN
                       else None if s["kind"] == ol.SEG_MARKER else s["len"])
        return got == list(want) and all(s["removedSeq"] is None for s in segs)
    return w


def _gran(it, name, branch, lens, groups, kind, order):
    d = _Doc(it)
    if kind == "text":
        specs = [_txt(n, i + len(name)) for i, n in enumerate(lens)]
    elif kind == "run":
        specs = [_items(n, i + len(name)) for i, n in enumerate(lens)]
    else:
        specs = list(lens)
    d.rows(specs, order)
    d.step()
    want = _merged(specs, groups)
    sizes = _merged(list(lens), groups)
    return Case(name, branch, d.log, d.cut,
                lambda h, s, a=_content(want), b=_lens(sizes): a(h, s) and b(h, s) and len({x["leaf"] for x in s}) == 1,
                ALL, kind)


def _gran_cases(it, prefix, kind, g) -> List[Case]:
    """the granularity shapes around g (256 for text, 128 for SubSequence items)"""
    big, small, rest = g + 44 * g // 256, 100 * g // 256, g - 2 * (100 * g // 256)
    t = [
        (f"{g}_{g}", "both sides <= granularity", [g, g], [2], "append"),
        (f"{g + 1}_{g + 1}", "both sides > granularity: kept apart", [g + 1, g + 1], [1, 1], "prepend"),
        (f"{g + 1}_{g}", "one side <= granularity", [g + 1, g], [2], "append"),
        (f"{g}_{g + 1}", "one side <= granularity", [g, g + 1], [2], "prepend"),
        ("run_grows", "the run has grown past the granularity when it meets the last row",
         [small, small, small, big], [3, 1], "append"),
        (f"run_{g}", "the run reaches the granularity exactly", [2 * small, rest, big], [3], "prepend"),
        (f"run_{g + 1}", "the run reaches the granularity + 1", [2 * small, rest + 1, big], [2, 1], "append"),
        ("long_short_long", "a long row absorbs a short one, then refuses a long one", [big, small, big], [2, 1],
         "prepend"),
        ("refused_restarts", "a refused row becomes prevSegment", [big, big, 10], [1, 2], "append"),
        ("refused_mid", "refused rows restart the run in the middle of a leaf", [big, big, big, 5, big], [1, 1, 2, 1],
         "prepend"),
    ]
    return [_gran(it, f"{prefix}_{n}", br, lens, groups, kind, order) for n, br, lens, groups, order in t]


def _simple(it, name, branch, specs, want, kind="text", order="append", profiles=ALL) -> Case:
    d = _Doc(it)
    d.rows(specs, order)
    d.step()
    return Case(name, branch, d.log, d.cut, _content(want), profiles, kind)


def _nl_split(it, name, whole, at, want) -> Case:
    d = _Doc(it)
    d.ins(0, text=whole)
    d.ins(at, text="X")          # splits the row
    d.rem(at, at + 1)            # "X" removed
    d.step(drain=3)              # first step: "X" is unlinked; it resets prevSegment, the parts stay apart
    d.ins(d.length, text="cd")   # an edit in the leaf: it will be scoured again
    d.step(drain=4)
    return Case(name, "the newline flag of the parts of a split row", d.log, d.cut, _texts(want), ALL, "text")


def _pack(it, name, branch, specs, witness) -> Case:
    d = _Doc(it)
    d.rows(specs, "prepend")
    d.step(drain=len(specs) // 2 + 4)
    return Case(name, branch, d.log, d.cut, witness, ALL, "text")


def _pk_long_witness(specs):
    def w(hdr, segs):
        text = "".join(specs)
        return (hdr["nleaf"] == 1 and "".join(s["text"] for s in segs) == text
                and [s["len"] for s in segs] == [49] + [28] * 6 and {s["leaf"] for s in segs} == {0})
    return w


def _pk_pairs_witness(specs):
    def w(hdr, segs):
        want = [specs[i] + specs[i + 1] for i in range(0, len(specs), 2)]
        return [s["text"] for s in segs] == want and [s["leaf"] for s in segs] == [0] * 5 + [1] * 5 + [2] * 5
    return w


def cases() -> List[Case]:
    it = ol.Interner()
    for v in range(300):  # SubSequence items: the integer v has item id v (a unit 10 is "\n")
        assert it.item(v) == v
    out: List[Case] = []
    out += _gran_cases(it, "g", "text", 256)
    out += _gran_cases(it, "s", "run", 128)
    out.append(_gran(it, "perm_300_300", "PermutationSegment.canAppend has no length rule", [300, 300], [2], "perm",
                     "append"))
    # newline
    out.append(_simple(it, "nl_tail", "the newline test on a run whose tail came from an appended row",
                       ["ab", "c\n", "de"], ["abc\n", "de"]))
    out.append(_nl_split(it, "nl_split_left", "a\nb", 2, ["a\n", "bcd"]))
    out.append(_nl_split(it, "nl_split_right", "ab\n", 1, ["ab\n", "cd"]))
    out.append(_simple(it, "s_nl_tail", "SubSequence.canAppend has no newline rule",
                       [[1, 2], [3, NL_ITEM], [4, 5]], [[1, 2, 3, NL_ITEM, 4, 5]], kind="run"))
    # markers
    out.append(_simple(it, "mk_between", "a marker between two texts", ["ab", None, "cd", "ef"], ["ab", None, "cdef"]))
    out.append(_simple(it, "mk_first", "a marker first in the leaf", [None, "ab", "cd"], [None, "abcd"],
                       order="prepend"))
    out.append(_simple(it, "mk_last", "a marker last in the leaf", ["ab", "cd", None], ["abcd", None]))
    # prevSegment resets
    d = _Doc(it)
    d.rows(["abc", "RR", "def"])
    d.rem(3, 5)
    d.step()
    out.append(Case("rs_unlinked", "an unlinked row resets prevSegment", d.log, d.cut, _content(["abc", "def"]), ALL,
                    "text"))
    d = _Doc(it)
    d.rows(["abc", "def"])
    d.ins(3, text="HH")
    d.step(to=2, drain=1)
    out.append(Case("rs_held", "a row above the minSeq resets prevSegment", d.log, d.cut,
                    lambda h, s: [x["text"] for x in s] == ["abc", "HH", "def"] and s[1]["seq"] > h["minSeq"]
                    and s[0]["seq"] <= h["minSeq"] and s[2]["seq"] <= h["minSeq"], ALL, "text"))
    for acked in (False, True):
        d = _Doc(it, local=LOCAL)
        d.rows(["abc", "def"])
        d.local_ins(3, "PP")
        d.step(to=2, drain=1)
        if acked:
            d.ack_ins(3, "PP", ref_seq=2)
            d.step(drain=3)
            w = _content(["abcPPdef"])
        else:
            def w(h, s):
                return ([x["text"] for x in s] == ["abc", "PP", "def"] and s[1]["seq"] == -1 and s[1]["ngroups"] > 0
                        and s[0]["seq"] <= h["minSeq"] and s[2]["seq"] <= h["minSeq"])
        out.append(Case("rs_pending_acked" if acked else "rs_pending", "a local pending row resets prevSegment" +
                        ("; acked, it merges at the next step" if acked else ""), d.log, d.cut, w, ALL, "text"))
    # properties
    out.append(_simple(it, "pr_equal", "equal property sets merge", [("ab", {"k0": 1}), ("cd", {"k0": 1}),
                                                                       ("ef", {"k0": 1})], ["abcdef"]))
    ten = {f"k{i}": 1 for i in range(10)}
    out.append(_simple(it, "pr_ninth_key", "matchProperties past the first group of 8 key slots",
                       [("ab", ten), ("cd", dict(ten, k9=2)), ("ef", dict(ten, k9=2))], ["ab", "cdef"],
                       profiles=WIDE_KEYS))
    out.append(_simple(it, "pr_one_side", "one side with properties, one without",
                       [("ab", {"k0": 1}), "cd", "ef"], ["ab", "cdef"]))
    # leaf boundaries
    nine = [_txt(20, 40 + i) for i in range(9)]
    d = _Doc(it)
    d.rows(nine)
    d.step()
    out.append(Case("lb_two_leaves", "no pair across a leaf boundary in a scour", d.log, d.cut,
                    lambda h, s: [x["text"] for x in s] == ["".join(nine[:4]), "".join(nine[4:])]
                    and s[0]["leaf"] == s[1]["leaf"] and h["nleaf"] == 1, ALL, "text"))
    # pack
    long_runs = [_txt(7, 60 + i) for i in range(31)]
    out.append(_pack(it, "pk_long_runs", "pack scours 8 sibling leaves in one wave: long runs", long_runs,
                     _pk_long_witness(long_runs)))
    pairs = [("x" if i % 2 == 0 else "y\n") for i in range(30)]
    pairs = [chr(65 + i // 2 % 26) + p for i, p in enumerate(pairs)]
    out.append(_pack(it, "pk_pairs", "pack scours 8 sibling leaves in one wave: runs of two", pairs,
                     _pk_pairs_witness(pairs)))
    # arena
    specs = [_txt(60, 80 + i) for i in range(4)]
    d = _Doc(it)
    d.ins(0, text=specs[1])
    d.ins(0, text=specs[0])      # the head's text lies after its successor's, and not at the arena top
    d.ins(120, text=specs[2])
    d.ins(180, text=specs[3])
    d.step()
    out.append(Case("ar_both_to_top", "both to top, then extend at top", d.log, d.cut, _content(["".join(specs)]), ALL,
                    "text"))
    for order in ("prepend", "append"):
        specs = [_txt(60, 84 + i) for i in range(4)]
        out.append(_simple(it, f"ar_{order}", "extend at top" if order == "prepend" else "already contiguous", specs,
                           ["".join(specs)], order=order))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


ARENA_CASES = ("pk_pairs", "pk_long_runs")  # replayed once more with an arena that compacts inside the pack's walk


def batch(which: Optional[List[Case]] = None) -> ol.Batch:
    cs = cases() if which is None else which
    return ol.Batch.from_logs([c.log for c in cs])


def interner() -> ol.Interner:
    return cases()[0].log.interner


def split_at_cut(cs: List[Case]):
    """The batch in two parts, cut just before each document's minSeq step"""
    b = batch(cs)
    head, tail = [], []
    for d, c in enumerate(cs):
        ops, text, props, kv = b.doc_arrays(d)
        head.append((ops[: c.cut], text, props, kv))
        tail.append((ops[c.cut:], text, props, kv))
    return ol.Batch.from_arrays(head, b.local_long_id), ol.Batch.from_arrays(tail, b.local_long_id)
