"""Hand-built logs for the slots a range op carries through its two boundary splits (mt_core.h range_op, split_slot's
`track`) — test infrastructure for tests/test_range_slots.py.

A remove or an annotate whose ends fall inside rows splits the first row at start, then the last row at end
(ensureIntervalBoundary twice, mergeTree.ts:2274-2278), then visits the rows between. The engine finds both rows in one
scan and follows their slots through the splits instead of looking them up by id afterwards: a split opens a slot after
the row it splits (the later rows of that leaf move one slot), and a leaf that reaches 8 rows splits 4 + 4 (children
4..7 move to a new leaf, which may split the parent node in turn). Every case is one small document, the smallest
shape at which one of those moves changes where the first or the last row sits.

Layout. Rows appended under a held minSeq sit four to a leaf (a leaf of 8 splits 4 + 4): base row r is child r % 4 of
leaf r // 4. `fill(i, k)` inserts k two-unit rows on the boundary before row i (inside a leaf: i % 4 != 0), so that
leaf holds 4 + k rows. Rows are addressed by their index in document order after the fills; (i, off) is the position
off units into row i. Each case states the row counts of the leaves it is about before and after the op and where
(leaf, child) the first and last touched rows end up; tests/test_range_slots.py checks them on the oracle's dumps, so
a case that does not reach its shape fails there.

Cases (every one as <name>_rem, <name>_ann on a text document and <name>_prm, a remove on a PermutationSegment
document, unless stated)
  onerow: both ends inside one row (tf == tg): both splits are of that row
  onerow_full: the same in a leaf of 7 rows, the row at child 5: the first split splits the leaf and both parts move
  sameleaf: first and last row in one leaf of 4: the first split shifts the last row one slot
  full_stay: leaf of 7, first row child 0, last row child 2: the leaf splits 4 + 4, the last row stays (child 3)
  full_move: leaf of 7, first row child 0, last row child 5: the last row moves to the new leaf
  full_both: leaf of 7, first row child 4, last row child 6: both parts of the first row and the last row move
  diffleaf: first row in a leaf of 7, last row two leaves on: the first split adds a leaf between them (the last
      row's leaf moves one place in document order, its slot stays)
  second_full_stays / second_full_moves: leaf of 6 holding both rows: the first split makes it 7, the second splits
      it; the first row's right part stays in the old leaf (child 2) / moves to the new one (child 4 -> 0)
  second_full_other: the first row in a leaf of 4, the last in another leaf of 7: only the second split splits a leaf
  parent_split / parent_split_same: 11 leaves, the second interior node holds 7: the first split's leaf split gives
      it 8 children and it splits 4 + 4; the last row in a later leaf / in the same leaf
  inv_removed / inv_removed_leaves: a row (three rows over two leaves) between first and last removed before the
      op's refSeq
  inv_pending / inv_pending_full: a row of another client inserted after the op's refSeq between first and last; the
      same in a leaf that row fills to 7, so the first split splits a leaf holding an invisible row
  start_boundary / start_boundary_full: start on a row boundary, only the end splits; in a leaf of 7 the end's
      split moves the first row (child 4) to the new leaf
  end_boundary / end_boundary_full: end on a row boundary, only the start splits; in a leaf of 7 the last row
      (child 6) moves to the new leaf
  local / local_full: replica 5's local op (pending), then its ack
  replace / replace_local: a replaceRange group (a remove and an insert under one sequence number) of client 2 /
      of replica 5 with its ack (_rem and _prm only)
"""
from __future__ import annotations

from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

from fluidframework_amd import oplog as ol
import range_logs as rl
import zamboni_logs as zl

LOCAL = rl.LOCAL
OPS = ("rem", "ann", "prm")


class Case(NamedTuple):
    name: str
    branch: str
    log: ol.DocLog
    cut: int                      # index of the range op's (first) record
    kind: str                     # "text" | "perm"
    sel: Optional[Callable]       # (hdr, segs) -> indices of the rows the op touched, in the final dump
    pre: Dict[int, int]           # leaf ordinal -> rows, before the op
    post: Dict[int, int]          # leaf ordinal -> rows, after the log
    ends: Optional[Tuple[Tuple[int, int], Tuple[int, int]]]  # (leaf, child) of the first and last touched row
    ntouched: Optional[int]
    nleaf: Tuple[int, int]        # leaves before the op, after the log


class _S(rl._R):
    """range_logs._R over a text or a PermutationSegment document, with the rows' lengths kept in document order"""

    def __init__(self, it, kind: str, local: int = 0):
        super().__init__(it, local=local)
        self.kind = kind
        self.rows: List[int] = []
        self.vis: List[bool] = []

    def seg(self, L: int, salt: int) -> dict:
        return dict(text=zl._txt(L, salt)) if self.kind == "text" else dict(perm=L)

    def at(self, i: int, off: int = 0) -> int:
        return sum(L for L, v in zip(self.rows[:i], self.vis[:i]) if v) + off

    def base_rows(self, n: int, unit: int = 3):
        for r in range(n):
            self.log.add(ol.OP_INSERT, pos1=self.at(len(self.rows)), **self.seg(unit, r), **self.hdr(1))
            self.rows.append(unit)
            self.vis.append(True)

    def fill(self, i: int, k: int, L: int = 2, client: int = 1, ref_seq=None, seen: bool = True):
        """k rows of L units on the boundary before row i; seen = False: the op under test does not see them"""
        for q in range(k):
            self.log.add(ol.OP_INSERT, pos1=self.at(i), **self.seg(L, 100 + q), **self.hdr(client, ref_seq))
            self.rows.insert(i, L)
            self.vis.insert(i, seen)

    def gone(self, i: int, client: int = 3):
        """row i removed whole by another client"""
        self.remove(self.at(i), self.at(i + 1), client)
        self.vis[i] = False


def _case(it, out, name, branch, build, pre, post, ends, ntouched, nleaf, ops=OPS, local=0):
    """build(d) lays the document out and returns (start, end, ref_seq or None) of the op under test"""
    for op in ops:
        d = _S(it, "perm" if op == "prm" else "text", local)
        a, b, ref = build(d)
        full = f"{name}_{op}"
        d.mark()
        if local:
            pend = d.local(ol.OP_ANNOTATE if op == "ann" else ol.OP_REMOVE, a, b, {"w": rl.tag(full)} if op == "ann" else None)
            seq = d.ack(pend)
        elif op == "ann":
            seq = d.annotate(a, b, {"w": rl.tag(full)}, ref_seq=ref)
        else:
            seq = d.remove(a, b, ref_seq=ref)
        sel = rl._sel_value(it, "w", rl.tag(full)) if op == "ann" else rl._sel_removed(seq)
        out.append(Case(full, branch, d.log, d.cut, d.kind, sel, pre, post, ends, ntouched, nleaf))


def _replace(it, out, name, branch, local):
    """SharedString.replaceRange: one message, a remove of [start, end) and an insert at start (mt_oplog.h
    MT_OPF_GROUPED); both ends inside rows of a leaf of 7"""
    for op in ("rem", "prm"):
        d = _S(it, "perm" if op == "prm" else "text", LOCAL if local else 0)
        d.base_rows(40)
        d.fill(9, 3)
        a, b = d.at(8, 1), d.at(13, 2)
        new = d.seg(2, 77)
        d.mark()
        if local:
            ref = d.seq
            d.log.add(ol.OP_REMOVE | ol.OPF_LOCAL, pos1=a, pos2=b)
            d.log.add(ol.OP_INSERT | ol.OPF_LOCAL, pos1=a, **new)
            d.seq += 1
            h = dict(client=LOCAL, seq=d.seq, ref_seq=ref, min_seq=d.min)
        else:
            h = d.hdr(2)
        d.log.add(ol.OP_REMOVE | ol.OPF_GROUPED, pos1=a, pos2=b, **h)
        d.log.add(ol.OP_INSERT, pos1=a, **new, **h)
        # [8l, 8r, F, F | F, 9, 10l, 10r, 11], then the new row after 8l (a leaf of 5)
        out.append(Case(f"{name}_{op}", branch, d.log, d.cut, d.kind, rl._sel_removed(d.seq), {2: 7}, {2: 5, 3: 5},
                        ((2, 2), (3, 2)), 6, (10, 11)))


def _build(n, fills=(), a=None, b=None, gone=(), late=None, late_k=1):
    """n base rows, fills [(row, k)], rows `gone` removed by client 3; `late`: a row index before which client 3
    inserts late_k rows after the op's refSeq; the op covers (row, off) a .. (row, off) b"""
    def f(d):
        d.base_rows(n)
        for i, k in fills:
            d.fill(i, k)
        for i in gone:
            d.gone(i)
        ref = None
        if late is not None:
            ref = d.seq
            d.fill(late, late_k, client=3, seen=False)
        return d.at(*a), d.at(*b), ref
    return f


def _all():
    it = ol.Interner()
    out: List[Case] = []
    F93 = [(9, 3)]  # leaf 2 = rows 8 (base 8), 9 10 11 (fill), 12 13 14 (base 9 10 11); leaf 3 starts at row 15
    F92 = [(9, 2)]  # leaf 2 = rows 8, 9 10 (fill), 11 12 13 (base 9 10 11)
    c = lambda *x, **kw: _case(it, out, *x, **kw)  # noqa: E731
    c("onerow", "both ends inside one row", _build(40, a=(9, 1), b=(9, 2)), {2: 4}, {2: 6}, ((2, 2), (2, 2)), 1, (10, 10))
    c("onerow_full", "one row at child 5 of a leaf of 7", _build(40, F93, (13, 1), (13, 2)), {2: 7}, {2: 4, 3: 5},
      ((3, 2), (3, 2)), 1, (10, 11))
    c("sameleaf", "the first split shifts the last row one slot", _build(40, a=(9, 1), b=(11, 2)), {2: 4}, {2: 6},
      ((2, 2), (2, 4)), 3, (10, 10))
    c("full_stay", "the leaf splits, the last row stays", _build(40, F93, (8, 1), (10, 1)), {2: 7}, {2: 5, 3: 4},
      ((2, 1), (2, 3)), 3, (10, 11))
    c("full_move", "the leaf splits, the last row moves to the new leaf", _build(40, F93, (8, 1), (13, 2)), {2: 7},
      {2: 4, 3: 5}, ((2, 1), (3, 2)), 6, (10, 11))
    c("full_both", "the leaf splits, both rows move to the new leaf", _build(40, F93, (12, 1), (14, 2)), {2: 7},
      {2: 4, 3: 5}, ((3, 1), (3, 3)), 3, (10, 11))
    c("diffleaf", "the first split adds a leaf before the last row's", _build(40, F93, (8, 1), (20, 2)), {2: 7, 4: 4},
      {2: 4, 3: 4, 5: 5}, ((2, 1), (5, 1)), 13, (10, 11))
    c("second_full_stays", "the second split splits the leaf holding the first row's right part (it stays)",
      _build(40, F92, (9, 1), (12, 2)), {2: 6}, {2: 4, 3: 4}, ((2, 2), (3, 1)), 4, (10, 11))
    c("second_full_moves", "the second split splits the leaf holding the first row's right part (it moves)",
      _build(40, F92, (11, 1), (13, 2)), {2: 6}, {2: 4, 3: 4}, ((3, 0), (3, 2)), 3, (10, 11))
    c("second_full_other", "only the second split splits a leaf", _build(40, [(17, 3)], (9, 1), (21, 2)), {2: 4, 4: 7},
      {2: 5, 4: 4, 5: 4}, ((2, 2), (5, 1)), 13, (10, 11))
    c("parent_split", "the first split's leaf split splits the parent node", _build(44, [(21, 3)], (20, 1), (28, 2)),
      {5: 7, 6: 4}, {5: 4, 6: 4, 7: 5}, ((5, 1), (7, 1)), 9, (11, 12))
    c("parent_split_same", "the same with the last row in the leaf that splits", _build(44, [(21, 3)], (20, 1), (25, 2)),
      {5: 7}, {5: 4, 6: 5}, ((5, 1), (6, 2)), 6, (11, 12))
    c("inv_removed", "a removed row between first and last", _build(40, a=(9, 1), b=(11, 2), gone=(10,)), {2: 4},
      {2: 6}, ((2, 2), (2, 4)), 2, (10, 10))
    c("inv_removed_leaves", "removed rows over two leaves between first and last",
      _build(40, a=(9, 1), b=(13, 2), gone=(10, 11, 12)), {2: 4, 3: 4}, {2: 5, 3: 5}, ((2, 2), (3, 1)), 2, (10, 10))
    c("inv_pending", "a later row of another client between first and last", _build(40, a=(9, 1), b=(11, 2), late=10),
      {2: 5}, {2: 7}, ((2, 2), (2, 4)), 2, (10, 10))
    c("inv_pending_full", "the first split splits a leaf that holds an invisible row",
      _build(40, F92, (8, 1), (13, 2), late=11), {2: 7}, {2: 4, 3: 5}, ((2, 1), (3, 2)), 5, (10, 11))
    c("start_boundary", "only the end splits", _build(40, a=(9, 0), b=(11, 2)), {2: 4}, {2: 5}, ((2, 1), (2, 3)), 3,
      (10, 10))
    c("start_boundary_full", "only the end splits, its leaf split moves the first row", _build(40, F93, (12, 0), (14, 2)),
      {2: 7}, {2: 4, 3: 4}, ((3, 0), (3, 2)), 3, (10, 11))
    c("end_boundary", "only the start splits", _build(40, a=(9, 1), b=(12, 0)), {2: 4}, {2: 5}, ((2, 2), (2, 4)), 3,
      (10, 10))
    c("end_boundary_full", "only the start splits, its leaf split moves the last row", _build(40, F93, (8, 1), (15, 0)),
      {2: 7}, {2: 4, 3: 4}, ((2, 1), (3, 3)), 7, (10, 11))
    c("local", "a local op and its ack", _build(40, a=(9, 1), b=(11, 2)), {2: 4}, {2: 6}, ((2, 2), (2, 4)), 3, (10, 10),
      local=LOCAL)
    c("local_full", "a local op in a leaf of 7 and its ack", _build(40, F93, (8, 1), (13, 2)), {2: 7}, {2: 4, 3: 5},
      ((2, 1), (3, 2)), 6, (10, 11), local=LOCAL)
    _replace(it, out, "replace", "a replaceRange group of another client", False)
    _replace(it, out, "replace_local", "a replaceRange group of the replica and its ack", True)
    names = [x.name for x in out]
    assert len(set(names)) == len(names)
    return out


_CACHE: List[Case] = []


def cases() -> List[Case]:
    if not _CACHE:
        _CACHE.extend(_all())
    return list(_CACHE)


def batch(cs: List[Case]) -> ol.Batch:
    return ol.Batch.from_logs([c.log for c in cs])


def leaf_rows(segs) -> Dict[int, int]:
    """leaf ordinal -> its row count, from a parsed dump"""
    out: Dict[int, int] = {}
    for s in segs:
        out[s["leaf"]] = out.get(s["leaf"], 0) + 1
    return out


def place(segs, i: int) -> Tuple[int, int]:
    """(leaf ordinal, child index) of row i of a parsed dump"""
    return segs[i]["leaf"], sum(1 for s in segs[:i] if s["leaf"] == segs[i]["leaf"])
