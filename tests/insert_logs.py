"""Hand-built logs that pin insert placement, row splits and node splits (blockInsert mergeTree.ts:2174-2257,
breakTie 2281-2310, rightExcursion 2346-2376, insertingWalk 2378-2520, splitLeafSegment 2258-2272, split 2522-2550)
-- test infrastructure for tests/test_ref_inserts.py and tools/make_ref_goldens.py --inserts.

Every insert of the engine takes find_reach / find_reach_tiled, insert_row, continue_from, split_row_par,
leaf_insert_slot, split_node and (tiled) rope_insert_after: lane-parallel code that only the GPU build compiles.
The generator's inserts are 1 to 8 units at scattered positions, and the other hand-built fixtures append. Every
case here is one document under a minSeq held at 0 unless stated, so tombstones stay and the final dump shows the
tree as the inserts left it. Base rows are client 1's, appended, four to a leaf (a leaf of 8 splits 4 + 4): row r at
slot (r // 4) * 8 + r % 4, slot 256 is row 128. The witnesses read leaves and slots from the dump (slots()), they
do not assume them. The insert under test writes the text "#" (an item 299, a PermutationSegment of 2 rows, a marker
with the property {"w": ...}) unless stated; `cut` is the record of the insert under test.

What the reference does at a tie (pos == 0 in front of a row the op does not see): a row removed at or below the
refSeq is passed; a local op stops (it sees everything); a remote op stops at an acked row and passes a pending row
of the replica. At the end of a leaf with pos == 0 a remote op asks continueFrom: the walk goes on into the next leaf
only if the first LOCALLY VISIBLE row after the leaf is a pending one; otherwise the new row is appended to the leaf.
So a run of tombstones is passed only up to its leaf's end unless a pending row follows it, and an insert at a
leaf-aligned position lands at the end of the leaf before.

Case list

Tie walk (one-unit rows)
  t_conc_2 / t_conc_5 / t_conc_40: clients 2.. insert at position 20 with one refSeq: later seqs land before earlier
      ones; with 40 they span more than two leaves. t_conc_5_local: the replica then inserts locally at 20 (first).
  t_own_then_other: client 2's own inserts (seen) and client 3's (not seen) interleaved at one position
  t_tomb_3 / t_tomb_9 / t_tomb_40 / t_tomb_70 / t_tomb_140: that many rows from row 21 (23 for 9) removed at or below
      the refSeq. The walk passes them up to the end of their leaf and continueFrom says no (the next locally visible
      row is acked): the row is appended to the leaf, behind 3 (for 9: 1) tombstones. With 70 / 140 the continueFrom
      scan passes one / two 256-slot boundaries before it finds the acked row (rows from 101 / 121).
  t_tomb_40_pend / t_tomb_70_pend / t_tomb_140_pend: the same runs (leaf-aligned at their end) with a pending row of
      the replica behind them: continueFrom says yes at every leaf's end, the walk passes all of them and the
      pending row, and leaves its leaf (9 or more leaves)
  t_tomb_after_ref: the rows removed after the refSeq are visible to the op: the row goes before the first
  t_tomb_unas: rows the replica removed locally (unacked) under a remote insert: before the first; t_tomb_unas_rev:
      a local insert over rows a remote client removed: behind them, to the end of the leaf
  t_pending_1 / t_pending_5 / t_pending_12: that many local pending inserts at position 20 (the end of leaf 4) when
      a remote insert arrives there: it goes behind all of them; with 5 the pending rows fill a leaf of their own,
      with 12 three (continueFrom yes at each leaf's end, then no: the row is appended to the last)
  t_pending_3_acked: three pending rows that end their leaf, the next leaf begins with an acked row: no
  t_pending_far_yes / t_pending_far_no: the end of leaf 4, then 140 tombstones (280 slots), then a pending row /
      none: continueFrom's scan goes past slot 256 either way (a second trip on flat builds, leaf after leaf on tiled)
  t_pending_acked_mid: five pending rows, the third acked before the remote insert arrives: it stops there
  t_leaf_end_block / t_leaf_end_root: the tie at the last row of a leaf that is the last child of its level-1
      block (row 15 / row 63: also the last under its level-2 node); the next leaf begins with tombstones, then a
      pending row
  t_pos0_tomb / t_pos0_pending / t_end_tomb / t_end_pending: position 0 and position = length with those mixes
  t_marker_inside: markers around the position, the reaching row is a marker
  t_perm: PermutationSegment rows; t_items: a {items} document (tombstones and a pending row at the tie)
Search alignment (rows of three units, the insert at offset 1 inside the row unless stated; flat and tiled)
  a_last_of_block: row 127, slot 251 (a leaf at rest holds at most 7 rows: slot 255 is never occupied between ops)
  a_first_of_block: row 128, slot 256; a_block_2 / a_block_3: rows 256 and 384, slots 512 and 768
  a_exact_total: position = the visible total of block 0 (a tie between rows 127 and 128)
  a_zero_blocks: 300 invisible rows before the first visible one
  a_quad0 .. a_quad3: rows 40 .. 43
  a_chunk_edge: rows 255 and 256: the last row of a chunk's 64th leaf and the first of the next chunk
  a_window_only: every case here whose minSeq stays 0 is one; a_settled_then_window: 1,000 settled rows, 50 window
      rows, the insert inside row 1,020 (flat and tiled: the small profiles hold no 1,050 rows)
Row split
  s_off_1 / s_off_mid / s_off_len1: a row of 9 units split at 1, 4, 8
  s_child0 .. s_child6: a leaf of 7 rows (the root), row j split: the leaf splits (willSplit), the left part moves
      with j < 4
  s_count1 .. s_count7: a leaf of c rows, row c // 2 split (gap taken up to 5, refused at 6, willSplit at 7);
      s_count6_lo / s_count6_hi: rows 1 and 5 of 6
  s_groups_rem / s_groups_ann / s_groups_both: the row carries pending local groups of the replica (a remove; an
      annotate; an annotate, a remove and an annotate), a remote insert splits it, the acks arrive;
      s_groups_local: an annotate group, split by a local insert
  s_overlap_3 / s_overlap_7: a row removed by 3 / 7 clients after the op's refSeq, split by the lagging client
  s_perm_unalloc: a PermutationSegment without a start. s_perm_alloc needs handle records (pcap engines only): the
      handle fixtures (tests/test_ref_handles.py) split allocated rows; no case here.
  s_items; s_nl: "ab\\n" split at 1 and "a\\nb" at 2 by rows that stay, then the minSeq moves
  s_props_8 (all profiles) / s_props_24 (24-slot profiles)
  s_window_stable: a settled row of a leaf of 7 split (flat and tiled); s_window_row: the same unsettled
  s_free0 / s_free1 / s_free2 / s_free5: that many rows unlinked by a minSeq step before an insert splits a row
      (distinct properties and texts everywhere)
  s_zero_len: an insert of length 0 is not expressible on the wire; MT_NOOP_SPLIT is a MergeTree-level record of
      the tree fixtures (tests/test_ref_tree.py). No case.
Node split
  n_height2 / n_height3: 130 / 520 appended rows; n_height4 (tiled-only, 2,100 rows)
  n_front: 300 inserts at position 0
  n_cursor_fwd / n_cursor_back: 300 one-unit inserts at a moving cursor in the middle of 100 rows by client 2, then a
      minSeq step; n_cursor_fwd_local / n_cursor_back_local: by the replica, acks lagging 5; n_cursor_two: clients 2
      and 3 at two cursors, flat and tiled
      (300 inserts each)
  n_cascade2_c<i>_lo / n_cascade2_c<i>_hi (i = 0, 3, 4, 6): one insert splits full leaf i of a full level-1 block, and
      the block with it (new row at j < 4, j >= 4)
  n_cascade3_lo / n_cascade3_hi: the same under a level-2 root of 7 blocks (116 base rows): it splits too
  n_cascade2_pack / n_cascade3_pack: the _c0_lo logs with distinct properties; afterwards three of every four rows of
      the old block are removed and the minSeq moves: zamboni scours and packs the sibling leaves of each parent, so
      the leaf ordinals (PACK_LEAVES) show which leaves share a parent: two parents of four leaves pack to a leaf of
      4 rows each. n_cascade2_avoid_pack / n_cascade3_avoid_pack: leaf 1 was not split beforehand, the parent ends
      with 7 leaves and packs to one leaf of 7: tests/test_ref_inserts.py asserts that the ordinals differ
  n_rope_split_lo / n_rope_split_hi (tiled): 256 appended rows are 64 leaves; leaf 10 / 50 splits: the 65th leaf
      enters at index 11 / 51; then an insert in each half. Chunk membership is not in the dump: the witness is the
      leaf ordinals
  n_rope_many (tiled): 1,100 rows inserted in one place, then an insert near each end and in the middle
Text length
  x_len_1 / 63 / 64 / 65 / 128 / 129 and x_len_<n>_nl (ending in "\\n", then an appendable row and a minSeq step)
  x_len_64_items / x_len_65_items
  x_arena_gc: an insert of 65 units after 300 units of text became garbage; the tests replay it once more with an
      arena that cannot hold it without a compaction
Caps (CAP_NAMES): cap_nodes: 800 inserts at scattered rows; cap_rows_cursor: n_cursor_fwd continued to 1,400 inserts.
The deviations from the planned list are recorded in DESIGN.md §6.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np

from fluidframework_amd import oplog as ol
import zamboni_logs as zl
from zamboni_logs import Case
from range_logs import _R, slots, BLOCK, MAXN, LOCAL, TILED  # noqa: F401

ALL = zl.ALL
WIDE_KEYS = zl.WIDE_KEYS
BIG = frozenset({"flat", "tiled"})
UNAS = -1
HASH_ITEM = 299


class _I(_R):
    """range_logs._R with inserts of any kind at any perspective, and local inserts with their acks"""

    def put(self, pos, client=2, ref_seq=None, text=None, items=None, perm=None, marker=None, props=None) -> int:
        self.log.add(ol.OP_INSERT, pos1=pos, text=text, items=items, perm=perm, marker=marker, props=props,
                     **self.hdr(client, ref_seq))
        return self.seq

    def lput(self, pos, text=None, items=None, props=None):
        self.log.add(ol.OP_INSERT | ol.OPF_LOCAL, pos1=pos, text=text, items=items, props=props)
        return (pos, text, items, props, self.seq)

    def lack(self, p) -> int:
        pos, text, items, props, ref = p
        self.log.add(ol.OP_INSERT, pos1=pos, text=text, items=items, props=props,
                     **self.hdr(self.log.local_long_id, ref))
        return self.seq

    def lrem(self, a, b):
        return self.local(ol.OP_REMOVE, a, b)


def _find(segs, text="#"):
    return [i for i, s in enumerate(segs) if s["text"] == text]


def _gone(s, ref):
    return s["removedSeq"] is not None and 0 < s["removedSeq"] <= ref


def _placed(index=None, passed=None, tomb_before=None, ref=None, pend_before=None, leaves_before=None, last_in_leaf=None,
            first_in_leaf=None, nrows=None, straddle=False, extra=None, text="#"):
    """witness: the one row `text` is row `index`; directly before it lie `tomb_before` rows removed at or below `ref`
    (exactly: the row before those is not one) / `pend_before` pending rows, which span at least `leaves_before`
    leaves and lie on both sides of a 256-slot boundary (`straddle`); it is the last / first row of its leaf"""
    def w(h, segs):
        at = _find(segs, text)
        if len(at) != 1:
            return False
        i = at[0]
        sl = slots(segs)
        if index is not None and i != index:
            return False
        if nrows is not None and len(segs) != nrows:
            return False
        run = list(range(i - passed, i)) if passed else []
        if tomb_before is not None:
            run = list(range(i - tomb_before, i))
            if i < tomb_before or not all(_gone(segs[k], ref) for k in run):
                return False
            if i > tomb_before and _gone(segs[i - tomb_before - 1], ref):
                return False
        if pend_before is not None:
            run = list(range(i - pend_before, i))
            if i < pend_before or not all(segs[k]["seq"] == UNAS for k in run):
                return False
            if i > pend_before and segs[i - pend_before - 1]["seq"] == UNAS:
                return False
        if leaves_before is not None and len({segs[k]["leaf"] for k in run}) < leaves_before:
            return False
        if straddle and (not run or sl[run[0]] // BLOCK == sl[i] // BLOCK):
            return False
        if last_in_leaf is not None and (i + 1 == len(segs) or segs[i + 1]["leaf"] != segs[i]["leaf"]) != last_in_leaf:
            return False
        if first_in_leaf is not None and (i == 0 or segs[i - 1]["leaf"] != segs[i]["leaf"]) != first_in_leaf:
            return False
        return extra is None or bool(extra(h, segs, i))
    return w


def _case(out, name, branch, d, w, profiles=ALL, kind="text"):
    assert d.cut is not None, name
    out.append(Case(name, branch, d.log, d.cut, w, profiles, kind))


def tie_cases(it) -> List[Case]:
    out: List[Case] = []
    for k in (2, 5, 40):
        d = _I(it)
        d.base(40, unit=1)
        R = d.seq
        for c in range(2, 2 + k):
            if c == 1 + k:
                d.mark()
            d.put(20, c, R, text=chr(48 + c - 2) if k < 40 else chr(0x100 + c))
        want = [chr(48 + c - 2) if k < 40 else chr(0x100 + c) for c in range(1 + k, 1, -1)]
        _case(out, f"t_conc_{k}", "concurrent inserts at one position: later seqs first", d,
              lambda h, s, want=want, k=k: [x["text"] for x in s[20:20 + k]] == want and len(s) == 40 + k
              and [x["seq"] for x in s[20:20 + k]] == sorted((x["seq"] for x in s[20:20 + k]), reverse=True)
              and len({x["leaf"] for x in s[20:20 + k]}) >= (3 if k == 40 else 1))
        if k == 5:
            d2 = _I(it, local=LOCAL)
            d2.base(40, unit=1)
            R = d2.seq
            for j, c in enumerate((2, 3, 4, 6, 7)):
                d2.put(20, c, R, text=chr(48 + j))
            d2.mark()
            d2.lput(20, "#")
            _case(out, "t_conc_5_local", "a local insert sees every row: it stops at the first", d2,
                  _placed(index=20, nrows=46, extra=lambda h, s, i: s[i]["seq"] == UNAS and s[i + 1]["text"] == "4"))
    d = _I(it)
    d.base(40, unit=1)
    R = d.seq
    d.put(20, 2, R, text="o")     # [o]
    d.put(20, 3, R, text="x")     # [x o]
    d.put(21, 2, R, text="p")     # client 2 sees o: [x o p]
    d.put(20, 3, R, text="y")     # client 3 sees x: before it: [y x o p]
    d.put(21, 3, R, text="z")     # behind y, before x: [y z x o p]
    d.mark()
    d.put(21, 2, R, text="#")     # client 2 sees o, p: position 21 is behind o: [y z x o # p]
    d.put(20, 2, R, text="q")     # before y
    _case(out, "t_own_then_other", "own later inserts are seen, another client's are not", d,
          lambda h, s: [x["text"] for x in s[20:27]] == list("qyzxo#p"))

    def tomb(n, a, total, pend, name, straddle=False, cross=0):
        """rows [a, a + n) of `total` removed by client 3; pend: the replica holds a pending row behind them"""
        d = _I(it, local=LOCAL)
        d.base(total, unit=1)
        if pend:
            d.lput(a + n, "P")  # appended to the leaf of row a + n - 1
        S = d.remove(a, a + n, 3)
        d.mark()
        d.put(a, 2, S, text="#")
        if pend:
            w = _placed(index=a + n + 1, passed=n + 1, ref=S, leaves_before=(n + 3) // 4, straddle=straddle, last_in_leaf=True,
                        extra=lambda h, s, i: s[i - 1]["text"] == "P" and s[i - 1]["seq"] == UNAS
                        and all(_gone(x, S) for x in s[a:a + n]) and s[a - 1]["leaf"] != s[i]["leaf"])
        else:
            left = min(n, (-a) % 4)  # the tombstones up to the end of row a's leaf
            w = _placed(index=a + left, tomb_before=left, ref=S, last_in_leaf=True, nrows=total + 1,
                        extra=lambda h, s, i: _gone(s[i + 1], S) == (n > left) and s[a + n + 1]["seq"] > 0
                        and s[a + n + 1]["removedSeq"] is None and all(_gone(x, S) for x in s[i + 1:a + n + 1])
                        # the acked row continueFrom finds lies `cross` 256-slot boundaries ahead
                        and slots(s)[a + n + 1] // BLOCK - slots(s)[i] // BLOCK == cross
                        and (cross < 2 or slots(s)[a + n + 1] - slots(s)[i] > BLOCK))
        _case(out, name, f"{n} rows removed at or below the refSeq in front of the insert" +
              (", a pending row behind them" if pend else ""), d, w)
    tomb(3, 21, 40, False, "t_tomb_3")
    tomb(9, 23, 60, False, "t_tomb_9")
    tomb(40, 21, 100, False, "t_tomb_40")
    tomb(70, 101, 300, False, "t_tomb_70", cross=1)
    tomb(140, 121, 300, False, "t_tomb_140", cross=2)
    tomb(40, 20, 100, True, "t_tomb_40_pend")
    tomb(70, 100 - 2, 300, True, "t_tomb_70_pend", straddle=True)
    tomb(140, 120, 300, True, "t_tomb_140_pend", straddle=True)

    d = _I(it)
    d.base(40, unit=1)
    R = d.seq
    d.remove(21, 30, 3)
    d.mark()
    d.put(21, 2, R, text="#")
    _case(out, "t_tomb_after_ref", "rows removed after the refSeq are visible: the insert goes before the first", d,
          _placed(index=21, nrows=41, extra=lambda h, s, i: all(x["removedSeq"] is not None for x in s[22:31])))
    d = _I(it, local=LOCAL)
    d.base(40, unit=1)
    p = d.lrem(21, 30)
    d.mark()
    d.put(21, 2, text="#")
    d.ack(p)
    _case(out, "t_tomb_unas", "rows under a local pending remove are visible to a remote insert", d,
          _placed(index=21, nrows=41, extra=lambda h, s, i: all(x["removedSeq"] is not None for x in s[22:31])))
    d = _I(it, local=LOCAL)
    d.base(40, unit=1)
    S = d.remove(21, 30, 3)
    d.mark()
    p = d.lput(21, "#")
    d.lack(p)
    _case(out, "t_tomb_unas_rev", "a local insert passes rows a remote client removed, to the end of the leaf", d,
          _placed(index=24, tomb_before=3, ref=S, last_in_leaf=True, nrows=41))

    def pending(k, name, acked_mid=False):
        d = _I(it, local=LOCAL)
        d.base(40, unit=1)
        ps = [d.lput(20, chr(65 + j)) for j in range(k)]  # document order: the last one first
        if acked_mid:
            for p in ps[:3]:  # acks come in order: A, B, C are acked; the run is E D | C B A
                d.lack(p)
        d.mark()
        d.put(20, 2, text="#")
        return d
    for k, leaves in ((1, 1), (5, 2), (12, 3)):
        d = pending(k, f"t_pending_{k}")
        _case(out, f"t_pending_{k}", f"a remote insert passes {k} pending rows", d,
              _placed(index=20 + k, pend_before=k, leaves_before=leaves, nrows=41 + k, last_in_leaf=True,
                      extra=lambda h, s, i: s[i + 1]["text"] != "" and s[i + 1]["seq"] > 0))
    d = pending(3, "t_pending_3_acked")
    _case(out, "t_pending_3_acked", "the pending rows end their leaf, an acked row follows: continueFrom says no", d,
          _placed(index=23, pend_before=3, leaves_before=1, nrows=44, last_in_leaf=True))
    d = pending(5, "t_pending_acked_mid", acked_mid=True)
    _case(out, "t_pending_acked_mid", "an acked row in the middle of the pending rows stops the walk", d,
          _placed(index=22, pend_before=2, nrows=46, extra=lambda h, s, i: [x["text"] for x in s[20:26]] ==
                  ["E", "D", "#", "C", "B", "A"] and s[23]["seq"] > 0))
    for yes in (True, False):
        d = _I(it, local=LOCAL)
        d.base(300, unit=1)
        if yes:
            d.lput(160, "P")
        S = d.remove(20, 160, 3)
        d.mark()
        d.put(20, 2, S, text="#")
        if yes:
            w = _placed(index=161, ref=S, straddle=False, last_in_leaf=True, extra=lambda h, s, i, S=S: s[160]["text"] == "P"
                        and slots(s)[i] - slots(s)[19] > BLOCK and all(_gone(x, S) for x in s[20:160]))
        else:
            w = _placed(index=20, tomb_before=0, ref=S, last_in_leaf=True, extra=lambda h, s, i, S=S: all(
                _gone(x, S) for x in s[21:161]) and slots(s)[161] - slots(s)[i] > BLOCK and s[161]["seq"] > 0)
        _case(out, "t_pending_far_" + ("yes" if yes else "no"), "continueFrom looks more than 256 slots ahead", d, w)
    for name, row, total in (("t_leaf_end_block", 15, 40), ("t_leaf_end_root", 63, 140)):
        d = _I(it, local=LOCAL)
        d.base(total, unit=1)
        d.lput(row + 3, "P")     # behind rows row+1, row+2 of the next leaf
        S = d.remove(row + 1, row + 3, 3)
        d.mark()
        d.put(row + 1, 2, S, text="#")
        _case(out, name, "the tie at the last row of the last leaf of its block; tombstones, then a pending row", d,
              _placed(index=row + 4, ref=S, nrows=total + 2, extra=lambda h, s, i, row=row, S=S: s[i - 1]["text"] == "P"
                      and _gone(s[i - 2], S) and _gone(s[i - 3], S) and s[row]["leaf"] + 1 == s[i]["leaf"]
                      and s[row]["leaf"] % 4 == 3))
    # position 0 and position = length
    d = _I(it, local=LOCAL)
    d.base(40, unit=1)
    S = d.remove(0, 6, 3)
    d.mark()
    d.put(0, 2, S, text="#")
    _case(out, "t_pos0_tomb", "position 0, tombstones at the front", d, _placed(tomb_before=None, nrows=41, extra=lambda
          h, s, i, S=S: i <= 6 and all(_gone(x, S) for x in s[:i])))
    d = _I(it, local=LOCAL)
    d.base(40, unit=1)
    for j in range(3):
        d.lput(0, chr(65 + j))
    d.mark()
    d.put(0, 2, text="#")
    _case(out, "t_pos0_pending", "position 0, pending rows at the front", d, _placed(index=3, pend_before=3, nrows=44))
    d = _I(it, local=LOCAL)
    d.base(40, unit=1)
    S = d.remove(34, 40, 3)
    d.mark()
    d.put(34, 2, S, text="#")
    _case(out, "t_end_tomb", "position = length, tombstones at the tail", d,
          _placed(nrows=41, extra=lambda h, s, i, S=S: i >= 34 and all(_gone(x, S) for x in s[34:i])))
    d = _I(it, local=LOCAL)
    d.base(40, unit=1)
    for j in range(3):
        d.lput(40, chr(65 + j))
    d.mark()
    d.put(40, 2, text="#")
    _case(out, "t_end_pending", "position = length, pending rows at the tail", d,
          _placed(index=43, pend_before=3, nrows=44))
    # markers
    d = _I(it)
    d.base(40, marker_every=2)
    d.mark()
    P = [0]
    for r in range(40):
        P.append(P[-1] + (1 if r % 2 == 1 else 1 + r % 3))
    d.put(P[22], 2, marker=0, props={"w": "t_marker_inside"})
    _case(out, "t_marker_inside", "the reaching row is a marker, P + v == pos", d,
          lambda h, s, pr=(it.key("w"), it.value("t_marker_inside")): len(s) == 41 and s[22]["kind"] == ol.SEG_MARKER
          and pr in [tuple(p) for p in s[22]["props"]] and s[21]["kind"] == ol.SEG_MARKER
          and s[23]["kind"] != ol.SEG_MARKER and s[24]["kind"] == ol.SEG_MARKER)
    # PermutationSegment rows and a {items} document: tombstones and a tie
    d = _I(it)
    d.base(40, kind="perm", unit=1)
    S = d.remove(21, 23, 3)
    d.mark()
    d.put(21, 2, S, perm=2)
    _case(out, "t_perm", "PermutationSegment rows: tombstones in front of the insert", d,
          lambda h, s, S=S: len(s) == 41 and s[23]["len"] == 2 and _gone(s[21], S) and _gone(s[22], S)
          and s[23]["leaf"] == s[22]["leaf"], kind="perm")
    d = _I(it, local=LOCAL)
    d.base(40, kind="run", unit=1)
    d.lput(24, items=[298])
    S = d.remove(21, 24, 3)
    d.mark()
    d.put(21, 2, S, items=[HASH_ITEM])
    _case(out, "t_items", "a {items} document: tombstones and a pending row in front of the insert", d,
          lambda h, s, S=S: len(s) == 42 and s[25]["items"] == [HASH_ITEM] and s[24]["items"] == [298]
          and s[24]["seq"] == UNAS and all(_gone(x, S) for x in s[21:24]), kind="run")
    return out


def _inside(it, out, name, branch, total, row, profiles=ALL, pre=None, off=1, slot=None):
    d = _I(it)
    P = d.base(total, unit=3)
    gone = pre(d, P) if pre else 0
    d.mark()
    d.put(P[row] + off - gone, 2, text="#")
    if off:
        w = _placed(index=row + 1, nrows=total + 2, extra=lambda h, s, i: s[i - 1]["len"] == off
                    and s[i + 1]["len"] == 3 - off and (slot is None or slots(s)[i - 1] == slot))
    else:
        w = _placed(nrows=total + 1, extra=lambda h, s, i: i in (row, row + 1) and (
            slot is None or slots(s)[row - 1] == slot - 5))
    _case(out, name, branch, d, w, profiles)


def align_cases(it) -> List[Case]:
    out: List[Case] = []
    _inside(it, out, "a_last_of_block", "the reaching row is the last occupied slot of block 0", 160, 127, slot=251)
    _inside(it, out, "a_first_of_block", "the reaching row is slot 256", 160, 128, slot=256)
    _inside(it, out, "a_block_2", "the reaching row is slot 512", 400, 256, slot=512)
    _inside(it, out, "a_block_3", "the reaching row is slot 768", 400, 384, slot=768)
    _inside(it, out, "a_exact_total", "pos equals the visible total of block 0", 160, 128, off=0, slot=256)

    def zero(d, P):
        d.remove(0, P[300], 3)
        return P[300]
    _inside(it, out, "a_zero_blocks", "300 invisible rows before the first visible one", 340, 300, pre=zero)
    for q in range(4):
        _inside(it, out, f"a_quad{q}", f"the reaching row at quad offset {q}", 60, 40 + q, slot=80 + q)
    d = _I(it)
    P = d.base(300, unit=3)
    d.mark()
    d.put(P[256] + 1, 2, text="#")
    d.put(P[255] + 2, 2, text="$")
    _case(out, "a_chunk_edge", "the last row of a chunk's 64th leaf, and the first row of the next chunk", d,
          lambda h, s: len(s) == 304 and s[256]["text"] == "$" and s[259]["text"] == "#" and s[255]["leaf"] == 63
          and s[258]["leaf"] == 64 and s[255]["len"] == 2 and s[258]["len"] == 1)
    d = _I(it)
    for r in range(1000):
        d.ins(d.length, text=zl._txt(1, r), props={"p": r})
    d.step(drain=2)
    d.cut = None
    for r in range(1000, 1050):
        d.ins(d.length, text=zl._txt(3, r), props={"p": r})
    d.mark()
    d.put(1000 + 3 * 20 + 1, 2, text="#")
    _case(out, "a_settled_then_window", "1,000 settled rows, then 50 window rows, pos in the window part", d,
          _placed(index=1021, nrows=1052, extra=lambda h, s, i: h["minSeq"] >= 1000 and s[i]["seq"] > h["minSeq"]
                  and s[999]["seq"] <= h["minSeq"] < s[1000]["seq"]), BIG)
    return out


def _one_leaf(it, c, j, off, unit=3, local=0):
    d = _I(it, local=local)
    P = d.base(c, unit=unit, props=lambda r: {"p": r})
    d.mark()
    d.put(P[j] + off, 2, text="#")
    return d


def _split_w(c, j, off, unit=3):
    def w(h, s):
        i = j + 1
        lv = [x["leaf"] for x in s]
        ok = (len(s) == c + 2 and s[i]["text"] == "#" and s[j]["len"] == off and s[i + 1]["len"] == unit - off
              and s[j]["props"] == s[i + 1]["props"] and s[j]["seq"] == s[i + 1]["seq"])
        if c + 2 < 8:
            return ok and h["nleaf"] == 1
        if c == 6:   # the split makes 7, the insert 8: 4 + 4
            return ok and lv == [0] * 4 + [1] * 4
        return ok and h["nleaf"] == 2 and lv.count(0) + lv.count(1) == 9  # the split makes 8: 4 + 4, then the insert
    return w


def split_cases(it) -> List[Case]:
    out: List[Case] = []
    for nm, off in (("1", 1), ("mid", 4), ("len1", 8)):
        _case(out, f"s_off_{nm}", f"a row of 9 units split at {off}", _one_leaf(it, 3, 1, off, unit=9),
              _split_w(3, 1, off, unit=9))
    for j in range(7):
        _case(out, f"s_child{j}", f"row {j} of a leaf of 7 split: the leaf splits", _one_leaf(it, 7, j, 1),
              _split_w(7, j, 1))
    for c in range(1, 8):
        _case(out, f"s_count{c}", f"a leaf of {c} rows, row {c // 2} split", _one_leaf(it, c, c // 2, 2),
              _split_w(c, c // 2, 2))
    _case(out, "s_count6_lo", "a leaf of 6, row 1 split", _one_leaf(it, 6, 1, 1), _split_w(6, 1, 1))
    _case(out, "s_count6_hi", "a leaf of 6, row 5 split", _one_leaf(it, 6, 5, 1), _split_w(6, 5, 1))

    # pending local groups on the split row
    def groups(name, kinds, local_split):
        d = _I(it, local=LOCAL)
        P = d.base(12, unit=5)
        ps = []
        for n, kd in enumerate(kinds):
            if kd == "rem":
                ps.append(d.local(ol.OP_REMOVE, P[5], P[6]))
            else:
                ps.append(d.local(ol.OP_ANNOTATE, P[5], P[6], {"g": f"{name}:{n}"}))
        d.mark()
        removed = "rem" in kinds
        if local_split:
            lp = d.lput(P[5] + 2, "#")
        else:
            d.put(P[5] + 2, 2, text="#")
        for p in ps:
            d.ack(p)
        if local_split:
            d.lack(lp)
        nann = sum(1 for kd in kinds if kd == "ann")

        def w(h, s):
            return (len(s) == 14 and s[6]["text"] == "#" and s[5]["len"] == 2 and s[7]["len"] == 3
                    and all(x["ngroups"] == 0 for x in s) and s[5]["props"] == s[7]["props"]
                    and len(s[5]["props"]) == (1 if nann else 0)
                    and (s[5]["removedSeq"] is not None) == removed and s[5]["removedSeq"] == s[7]["removedSeq"])
        _case(out, name, "a row with pending local groups is split, then the acks arrive (split_groups)", d, w)
    groups("s_groups_rem", ["rem"], False)
    groups("s_groups_ann", ["ann"], False)
    groups("s_groups_both", ["ann", "rem", "ann"], False)
    groups("s_groups_local", ["ann"], True)
    for nrem in (3, 7):
        d = _I(it)
        P = d.base(12, unit=5)
        R = d.seq
        for c in range(3, 3 + nrem):
            d.remove(P[5], P[6], c, ref_seq=R)
        d.mark()
        d.put(P[5] + 2, 2, R, text="#")
        _case(out, f"s_overlap_{nrem}", f"a row removed by {nrem} clients after the refSeq split by a lagging client", d,
              lambda h, s, nrem=nrem: len(s) == 14 and s[6]["text"] == "#" and s[5]["len"] == 2 and s[7]["len"] == 3
              and len(s[5]["overlap"]) == nrem - 1 and s[5]["overlap"] == s[7]["overlap"]
              and s[5]["removedSeq"] == s[7]["removedSeq"] is not None)
    d = _I(it)
    P = d.base(12, kind="perm", unit=5)
    d.mark()
    d.put(P[5] + 2, 2, perm=2)
    _case(out, "s_perm_unalloc", "a PermutationSegment without a start split", d,
          lambda h, s: [x["len"] for x in s[4:9]] == [5, 2, 2, 3, 5] and s[5]["start"] == s[7]["start"] ==
          ol.HANDLE_UNALLOCATED, kind="perm")
    d = _I(it)
    P = d.base(12, kind="run", unit=5)
    d.mark()
    d.put(P[5] + 2, 2, items=[HASH_ITEM])
    _case(out, "s_items", "a SubSequence row split", d,
          lambda h, s: [len(x["items"]) for x in s[4:9]] == [5, 2, 1, 3, 5] and s[6]["items"] == [HASH_ITEM]
          and s[5]["items"] + s[7]["items"] == zl._items(5, 5), kind="run")
    d = _I(it)
    d.rows(["ab\n", "a\nb", "zz"])
    d.mark()
    d.put(1, 2, text="X")   # "a" X "b\n"
    d.put(6, 2, text="Y")   # "a\n" Y "b"
    d.step(drain=4)
    _case(out, "s_nl", "the halves of split rows keep or lose the newline flag: zamboni's appends show it", d,
          lambda h, s: [x["text"] for x in s] == ["aXb\n", "a\n", "Ybzz"])
    for nk, profs in ((8, ALL), (24, WIDE_KEYS)):
        d = _I(it)
        keys = {f"k{q}": q + nk for q in range(nk)}
        P = d.base(12, unit=5, props=lambda r: keys if r == 5 else {"k0": r})
        d.mark()
        d.put(P[5] + 2, 2, text="#")
        _case(out, f"s_props_{nk}", f"a row with {nk} keys split", d,
              lambda h, s, nk=nk: len(s) == 14 and s[6]["text"] == "#" and len(s[5]["props"]) == nk
              and s[5]["props"] == s[7]["props"] and len(s[6]["props"]) == 0, profs)
    for name, settle, profs in (("s_window_stable", True, BIG), ("s_window_row", False, ALL)):
        d = _I(it)
        P = d.base(40, unit=3, props=lambda r: {"p": r})
        for q in range(3):
            d.put(P[9], 1, text="QZQ"[q] * 2, props={"p": 100 + q})  # leaf 2 holds 7 rows; later rows moved by 6
        if settle:
            d.step(drain=2)
            d.cut = None
        d.mark()
        d.put(P[10] + 6 + 1, 2, text="#")
        _case(out, name, "a " + ("settled" if settle else "window") + " row split while its leaf splits", d,
              lambda h, s, settle=settle: len(s) == 45 and s[14]["text"] == "#" and s[13]["len"] == 1
              and s[15]["len"] == 2 and [x["leaf"] for x in s[8:17]] == [2] * 4 + [3] * 5
              and (h["minSeq"] >= s[13]["seq"]) == settle, profs)
    for nfree in (0, 1, 2, 5):
        d = _I(it)
        P = d.base(40, unit=3, props=lambda r: {"p": r})
        if nfree:
            d.remove(P[30], P[30 + nfree], 3)
        d.step(drain=2)
        d.cut = None
        d.mark()
        d.put(P[10] + 1, 2, text="#", props={"p": 500})
        d.put(P[12] + 1 + 1, 2, text="$", props={"p": 501})
        d.put(P[14] + 2 + 2, 3, text="%", props={"p": 502})
        _case(out, f"s_free{nfree}", f"{nfree} free row ids on the stack when an insert splits a row", d,
              lambda h, s, nfree=nfree: len(s) == 46 - nfree and [x["text"] for x in (s[11], s[15], s[19])] ==
              ["#", "$", "%"] and len({(tuple(map(tuple, x["props"])), x["text"]) for x in s}) == len(s)
              and h["minSeq"] > 40)
    return out


def _cursor(it, name, mode, n, profiles=ALL, step=True):
    """n one-unit inserts at a moving cursor in the middle of 100 rows"""
    d = _I(it, local=LOCAL if mode == "local" else 0)
    d.base(100, unit=1)
    fwd = "fwd" in name or "rows" in name
    d.mark()
    pend = []
    for k in range(n):
        ch = chr(0x3b1 + k % 300)
        if mode == "two":
            # client 2 types forward at 50, client 3 backward at 20 (in front of client 2's cursor: it shifts by k)
            d.put(50 + 2 * k, 2, text=ch)
            d.put(20, 3, text=chr(0x5d0 + k % 300))
        elif mode == "local":
            pend.append(d.lput(50 + k if fwd else 50, ch))
            if len(pend) > 5:
                d.lack(pend.pop(0))
        else:
            d.put(50 + k if fwd else 50, 2, text=ch)
    for p in pend:
        d.lack(p)
    if step:
        d.step(drain=8)
    return d


def node_cases(it) -> List[Case]:
    out: List[Case] = []
    for name, n, profs in (("n_height2", 130, ALL), ("n_height3", 520, ALL), ("n_height4", 2100, TILED)):
        d = _I(it)
        d.base(n, unit=1)
        d.mark()
        d.put(n // 2, 2, text="#")
        _case(out, name, f"{n} appended rows", d, _placed(index=n // 2, nrows=n + 1, extra=lambda h, s, i, n=n:
              h["nleaf"] == (n - 4) // 4 + 1 and [x["leaf"] for x in s[:8]] == [0] * 4 + [1] * 4), profs)
    d = _I(it)
    for k in range(300):
        if k == 150:
            d.mark()
        d.put(0, 2, text=chr(0x3b1 + k))
    _case(out, "n_front", "300 inserts at position 0: every split is of the first leaf", d,
          lambda h, s: [x["text"] for x in s] == [chr(0x3b1 + k) for k in range(299, -1, -1)] and h["nleaf"] >= 60)
    typed = [chr(0x3b1 + k) for k in range(300)]
    for name, mode in (("n_cursor_fwd", "remote"), ("n_cursor_back", "remote"), ("n_cursor_fwd_local", "local"),
                       ("n_cursor_back_local", "local"), ("n_cursor_two", "two")):
        d = _cursor(it, name, mode, 300)
        if mode == "two":
            w = lambda h, s: h["length"] == 700 and "".join(x["text"] for x in s)[20:320] == "".join(  # noqa: E731
                chr(0x5d0 + k) for k in range(299, -1, -1)) and "".join(x["text"] for x in s)[350:650] == "".join(
                typed) and len(s) < 700
        else:
            want = "".join(typed if "fwd" in name else reversed(typed))
            w = lambda h, s, want=want: h["length"] == 400 and "".join(x["text"] for x in s)[50:350] == want \
                and len(s) < 400 and all(x["seq"] != UNAS for x in s)  # noqa: E731
        # two clients' 600 inserts pass the small profiles' nodes: flat and tiled
        _case(out, name, "300 one-unit inserts at a moving cursor, then the minSeq step merges them", d, w,
              BIG if mode == "two" else ALL)
    # Cascades. Appended rows leave level-1 blocks of 4 leaves (16 rows). Four inserts into each of leaves 3, 2, 1 of
    # block 0 split them: the block holds 7 leaves, child i at positions 4 i .. 4 i + 3. Three more rows fill child
    # `idx` to 7 rows; the insert under test makes it 8: the leaf splits and its parent with it (8 leaves). With 36
    # base rows the root then takes a third child; with 116 the level-2 root holds 7 blocks, takes an eighth and
    # splits too (n_cascade3). `avoid`: leaf 1 is not split beforehand, so the parent ends with 7 leaves, unsplit.
    def cascade(nbase, idx, j, avoid=False, pack=False):
        d = _I(it)
        d.base(nbase, unit=1, props=(lambda r: {"p": r}) if pack else None)  # distinct properties: no row merges
        for leaf in (3, 2, 1):
            for q in range(4):
                if not (avoid and leaf == 1):
                    d.put(4 * leaf + 1, 1, text=chr(65 + leaf), props={"p": 200 + 4 * leaf + q} if pack else None)
        for q in range(3):
            d.put(4 * idx + 1, 1, text="a", props={"p": 300 + q} if pack else None)
        d.mark()
        d.put(4 * idx + j, 2, text="#")
        if pack:  # every row of old block 0 but each fourth is removed; the minSeq moves: zamboni scours and packs
            n0 = 32 - (4 if avoid else 0)
            for r in range(n0 - 1, -1, -1):
                if r % 4 != 0:
                    d.remove(r, r + 1, 3)
            d.step(drain=12)
        return d
    for idx in (0, 3, 4, 6):
        for nm, j in (("lo", 1), ("hi", 5)):
            _case(out, f"n_cascade2_c{idx}_{nm}", f"one insert splits full leaf {idx} of a full level-1 block, and the block",
                  cascade(36, idx, j), lambda h, s, idx=idx, j=j: s[4 * idx + j]["text"] == "#" and len(s) == 52
                  and [x["leaf"] for x in s[4 * idx:4 * idx + 8]] == [idx] * 4 + [idx + 1] * 4 and h["nleaf"] == 13)
    for nm, j in (("lo", 1), ("hi", 5)):
        _case(out, f"n_cascade3_{nm}", "one insert splits a leaf, its level-1 block and the level-2 node above",
              cascade(116, 0, j), lambda h, s, j=j: s[j]["text"] == "#" and len(s) == 132
              and [x["leaf"] for x in s[:8]] == [0] * 4 + [1] * 4 and h["nleaf"] == 33)

    def survivors(s):
        return [(x["text"], x["leaf"]) for x in s if x["removedSeq"] is None]
    for nm, nbase in (("n_cascade2", 36), ("n_cascade3", 116)):
        for avoid in (False, True):
            d = cascade(nbase, 0, 1, avoid=avoid, pack=True)
            _case(out, nm + ("_avoid_pack" if avoid else "_pack"), "after the cascade" + (" that was avoided" if avoid else "")
                  + ", rows are removed and the minSeq moves: zamboni packs sibling leaves, so the leaf ordinals show "
                  "which leaves share a parent", d, lambda h, s, nbase=nbase, avoid=avoid: h["minSeq"] > nbase + 20
                  and all(x["removedSeq"] is None for x in s) and PACK_LEAVES[avoid] == [
                      x["leaf"] for x in s[:len(PACK_LEAVES[avoid])]])
    for nm, leaf in (("lo", 10), ("hi", 50)):
        d = _I(it)
        d.base(256, unit=1)  # 64 leaves: a full chunk
        for q in range(4):
            d.put(4 * leaf + 1, 1, text="R")  # the leaf splits: the 65th leaf enters at index leaf + 1
        d.mark()
        d.put(4 * 20 + 1, 2, text="#")
        d.put(4 * 45 + 2, 2, text="$")
        _case(out, f"n_rope_split_{nm}", f"the 65th leaf enters a full chunk at index {leaf + 1}, then a search in each half",
              d, lambda h, s, leaf=leaf: h["nleaf"] == 65 and len(s) == 262 and [x["text"] for x in s].count("R") == 4
              and [x["leaf"] for x in s[4 * leaf + (2 if leaf > 45 else 0):][:8]] == [leaf] * 4 + [leaf + 1] * 4
              and s[81]["text"] == "#" and "$" in [x["text"] for x in s[182:188]], TILED)
    d = _I(it)
    d.base(40, unit=1)
    for k in range(1100):
        d.put(20, 1, text=chr(0x400 + k % 256))
    d.mark()
    d.put(22, 2, text="#")
    d.put(600, 2, text="$")
    d.put(1118, 2, text="%")
    _case(out, "n_rope_many", "1,100 rows inserted in one place (chunk splits), then a search in each part", d,
          lambda h, s: len(s) == 1143 and s[22]["text"] == "#" and s[600]["text"] == "$" and s[1118]["text"] == "%"
          and h["nleaf"] > 3 * 64, TILED)
    return out


def text_cases(it) -> List[Case]:
    out: List[Case] = []
    for n in (1, 63, 64, 65, 128, 129):
        for nl in (False, True):
            d = _I(it)
            d.base(12, unit=2)
            t = zl._txt(n, n)
            if nl:
                t = t[:-1] + "\n"
            d.mark()
            d.put(12, 2, text=t)
            d.put(12 + n, 2, text="tail")
            d.step(drain=4)
            _case(out, f"x_len_{n}" + ("_nl" if nl else ""), f"an insert of {n} units" +
                  (" ending in a newline" if nl else ""), d,
                  lambda h, s, t=t, nl=nl: any(x["text"].endswith(t) and y["text"].startswith("tail")
                                               for x, y in zip(s, s[1:])) if nl else any(
                      t + "tail" in x["text"] for x in s))
    for n in (64, 65):
        d = _I(it)
        d.base(12, kind="run", unit=2)
        d.mark()
        v = [(7 * q) % 250 + 11 for q in range(n - 1)] + [zl.NL_ITEM]
        d.put(12, 2, items=v)
        d.put(12 + n, 2, items=[HASH_ITEM])
        d.step(drain=4)
        _case(out, f"x_len_{n}_items", f"a SubSequence insert of {n} items (the newline is not special)", d,
              lambda h, s, v=v: any(x["items"][q:q + len(v) + 1] == v + [HASH_ITEM] for x in s
                                    for q in range(len(x["items"]) - len(v))), kind="run")
    return out


ARENA_CASE = "x_arena_gc"


def arena_cases(it) -> List[Case]:
    """three rows of 100 units are removed and unlinked by a minSeq step (their text is garbage in the arena), then an
    insert of 65 units: with the arena capacity tests/test_ref_inserts.py small_arena gives the replay (the arena top
    at `cut` plus 32 units), arena_alloc must compact to place it"""
    d = _I(it)
    d.base(12, unit=2, props=lambda r: {"p": r})
    for q in range(3):
        d.put(6, 1, text=zl._txt(100, 50 + q), props={"p": 100 + q})
    d.remove(6, 306, 3)
    d.step(drain=3)
    d.cut = None
    d.mark()
    t = zl._txt(65, 65)
    d.put(6, 2, text=t, props={"p": 500})
    return [Case(ARENA_CASE, "an insert of 65 units whose arena_alloc compacts the arena", d.log, d.cut,
                 lambda h, s: len(s) == 13 and s[3]["text"] == t and h["length"] == 24 + 65, ALL, "text")]


def cap_cases(it) -> List[Case]:
    d = _I(it)
    d.base(100, unit=1)
    d.mark()
    for k in range(800):
        d.put((k * 37) % (100 + k), 2, text=chr(0x3b1 + k % 300), props={"p": k})
    c1 = Case("cap_nodes", "inserts until the small profile runs out of nodes", d.log, d.cut,
              lambda h, s: len(s) >= 900, ALL, "text")
    d = _cursor(it, "cap_rows_cursor", "remote", 1390, step=False)
    c2 = Case("cap_rows_cursor", "the cursor case continued past the small profile's row capacity", d.log, d.cut,
              lambda h, s: len(s) == 1490, ALL, "text")
    return [c1, c2]


# the leaf ordinals of the first rows after the pack, as the reference gives them (False: the cascade; True: avoided)
PACK_LEAVES = {False: [0] * 4 + [1] * 4 + [2] * 4, True: [0] * 7 + [1] * 4 + [2]}
CAP_NAMES = ("cap_nodes", "cap_rows_cursor")
_CACHE = {}


def _all():
    if not _CACHE:
        it = ol.Interner()
        for v in range(300):  # SubSequence items: the integer v has item id v
            assert it.item(v) == v
        cs = tie_cases(it) + align_cases(it) + split_cases(it) + node_cases(it) + text_cases(it) + arena_cases(it)
        caps = cap_cases(it)
        names = [c.name for c in cs + caps]
        assert len(set(names)) == len(names)
        assert tuple(c.name for c in caps) == CAP_NAMES
        _CACHE["cases"], _CACHE["caps"] = cs, caps
    return _CACHE


def cases() -> List[Case]:
    """the cases every build must replay to the reference's digest"""
    return list(_all()["cases"])


def caps() -> List[Case]:
    return list(_all()["caps"])


def batch(which: Optional[List[Case]] = None) -> ol.Batch:
    cs = cases() if which is None else which
    return ol.Batch.from_logs([c.log for c in cs])


def split_at_cut(cs: List[Case]):
    """The batch in two parts, cut just before each document's insert under test"""
    b = batch(cs)
    head, tail = [], []
    for d, c in enumerate(cs):
        ops, text, props, kv = b.doc_arrays(d)
        head.append((ops[: c.cut], text, props, kv))
        tail.append((ops[c.cut:], text, props, kv))
    return ol.Batch.from_arrays(head, b.local_long_id), ol.Batch.from_arrays(tail, b.local_long_id)


def census(parsed, logs) -> dict:
    """Over parsed dumps [(hdr, segs)] and the op arrays of their logs. From the dumps, for every row R with a
    sequence number: the run of rows directly in front of it that an insert walk passes (removed below R's seq, or
    pending) -> `tie_left_leaf`: runs that begin in another leaf than R's; `tomb8` / `tomb64` / `tomb128`: runs of
    more than 8 / 64 / 128 tombstones; `near256`: rows that arrived after their successor (not appended) within 4
    slots of a multiple of 256; `splits`: adjacent rows that are the halves of one row (equal seq and client, a
    newer row between or beside them). From the logs: `hot_positions`: (document, position) pairs that take more than
    100 inserts; `long_texts`: inserts of 64 units or more."""
    out = dict(tie_left_leaf=0, tomb8=0, tomb64=0, tomb128=0, near256=0, splits=0, hot_positions=0, long_texts=0)
    for hdr, segs in parsed:
        sl = slots(segs)
        run = []  # the passable rows directly in front of row i: tombstones and pending rows
        for i, s in enumerate(segs):
            if s["seq"] > 0:
                tombs = [k for k in run if segs[k]["removedSeq"] is not None]
                if all(segs[k]["removedSeq"] < s["seq"] for k in tombs):  # the row arrived after the removes
                    out["tomb8"] += len(tombs) > 8
                    out["tomb64"] += len(tombs) > 64
                    out["tomb128"] += len(tombs) > 128
                    out["tie_left_leaf"] += bool(run) and segs[run[0]]["leaf"] != s["leaf"]
                nxt = segs[i + 1] if i + 1 < len(segs) else None
                if nxt is not None and 0 < nxt["seq"] < s["seq"] and (sl[i] % BLOCK < 4 or sl[i] % BLOCK >= BLOCK - 4):
                    out["near256"] += 1
                if i + 2 < len(segs) and segs[i + 2]["seq"] == s["seq"] and segs[i + 2]["client"] == s["client"] \
                        and segs[i + 1]["seq"] != s["seq"] and s["kind"] != ol.SEG_MARKER:
                    out["splits"] += 1
            if (s["removedSeq"] is not None and s["removedSeq"] > 0) or s["seq"] == UNAS:
                run.append(i)
            else:
                run = []
    for ops in logs:
        ins = ops[(ops["kind"] & 7) == ol.OP_INSERT]
        out["long_texts"] += int((ins["text_len"] >= 64).sum())
        if len(ins):
            _, n = np.unique(ins["pos1"], return_counts=True)
            out["hot_positions"] += int((n > 100).sum())
    return out
