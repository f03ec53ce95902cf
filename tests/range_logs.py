"""Hand-built logs whose removes and annotates span many leaves (markRangeRemoved mergeTree.ts:2640-2752,
annotateRange 2598-2638, nodeMap 2936-2998, ackPendingSegment 1729-1790) — test infrastructure for
tests/test_ref_ranges.py and tools/make_ref_goldens.py --ranges.

The generator caps a remove at 16 units and an insert at 8, so none of its range edits covers more than two or
three leaves. The engine serves a wide range with lane-parallel code that exists only in the GPU build (a find
pass over wave blocks of 256 slots, a visit loop of 256 slots a trip, remove_run with a lane per row, ack with a
lane per member row, 64 members a pass); the host core takes the serial twins. Every case here is one document
whose rows are appended under a minSeq held at 0: zamboni runs only when the minSeq moves, so the final dump shows
the tree as the edits left it, and the layout is computable: appended rows sit four to a leaf (a leaf of 8 splits
4 + 4), row r at slot (r // 4) * 8 + r % 4, so slot 256 is row 128 and a wave block holds 128 rows. The witnesses
read the slots from the dump's `leaf` field (slots()), they do not assume them.

Each case carries a witness: a predicate over the parsed canonical dump of the REFERENCE that proves the branch was
taken ("N rows carry removedSeq S, their leaves span K, rows on both sides of slot 256 k are among them"). A wide
annotate writes a value "w:<case>..." no other op writes, so the rows it touched can be counted in a dump. Rows are
1 + r % 3 units long unless stated; `cut` is the index of the case's first wide op (for an ack case: of the ack), where
the two-submit tests cut the log.

Case list (every width case twice: <name>_rem, a sequenced remote remove on an observer replica, and <name>_ann, an
annotate; rows [a, b) of n)

Width and alignment
  w_leaf1: rows [8, 12) of 40: one whole leaf
  w_leaf2: rows [8, 16) of 40: exactly two leaves
  w_l33: rows [0, 129) of 160: 33 leaves, the last row is the first past slot 256 (find: first row latched in block
      0, last in block 1; the visit's second trip holds one row)
  w_edge256: rows [127, 129) of 160: first row = the last slot below 256 (251), last row = slot 256
  w_blocks3: rows [2, 290) of 300: 72 leaves, three wave blocks
  w_whole: rows [0, 300) of 300, end = length
  w_pastend: rows [100, 160) of 160 with end = length + 50 (clipped)
  w_empty_start: start = length, end = length + 5; w_empty_end: end = start; w_empty_neg: end < start: nothing changes
  w_sp_bb / w_sp_bi / w_sp_ib / w_sp_ii: rows 20..140 of 160 three units each, {start, end} x {on a row boundary,
      inside a row}
  w_fullleaf: start inside a row of a leaf that holds 7 rows (three rows inserted into leaf 2 of 300 rows), end
      inside row 290: the first split splits the leaf and shifts every later slot before the end is split
  w_onerow: both ends inside one row of three units (tf == tg), the small control
  w_sameleaf: start inside row 9, end inside row 11 of 40 (one leaf): the start split shifts the last row one slot
  w_sameleaf_full: the same in a leaf of 7 rows (start inside row 8, end inside row 11): the start split splits the
      leaf and the last row moves to the new leaf before the end is split
  w_quad0 .. w_quad3: start at rows 8, 9, 10, 11 (quad offsets 0..3 of a leaf), end at row 141 of 160
Perspective mixes (300 rows; the wide op of client 2 visits at least 100 rows)
  p_later_inserts: 40 rows inserted by client 3 after the op's refSeq, inside the range (skipped)
  p_own_later: 30 later inserts of client 2 itself (seen: refSeq below them, own client) and 30 of client 3 (not
      seen) interleaved; the op covers everything client 2 sees
  p_removed_before: every third row of the range removed by client 3 before the refSeq (skipped)
  p_overlap: every fourth row removed by client 3 after the refSeq: the remove pushes client 2 onto their overlap
      lists (the annotate annotates them)
  p_unas: replica 5 holds local pending removes of rows [50, 60) and [200, 210) when client 2's remove of rows
      [10, 290) lands (the `unas` branch: removedSeq takes the remote seq), then the local removes are acked
  p_unas_rev: replica 5 holds a local pending remove of rows [10, 290) when client 2 removes rows [100, 104) and then
      all 300 rows; then the ack
  p_invisible256: rows [20, 200) removed by client 3 before the refSeq (360 consecutive invisible slots: the visit
      passes a whole block with an empty ballot), the op covers rows [5, 290)
  p_twice: client 2 removes rows [50, 150), then rows [10, 250) of what it sees: the range passes over rows it
      removed itself
  p_markers: a marker every seventh row; p_perm: PermutationSegment rows (remove only); p_items: a {items}
      document (SubSequence rows)
Local groups (replica 5; the base rows are client 1's; <n> = 65, 129, 300 rows)
  lg_rem_<n>: a local remove of n rows, its ack, a NOOP step
  lg_ann2_<n>: a local annotate with two keys the rows already hold, its ack, the step
  lg_annrw_<n>: the same with combiningOp rewrite
  lg_ann_newkey: a local annotate of 129 rows with a key the document has not seen (key_slot inside ack_rows)
  lg_two_ann: local annotates of rows [0, 200) and [100, 300), acked in order (two groups on the shared rows, the
      membership log compacts with a live group behind the acked one)
  lg_ann_rem: a local annotate of rows [0, 200), a local remove of rows [100, 300), acked in order
  lg_regen: a local remove of rows [10, 140), then a reconnect (regeneratePendingOp: one MT_OPF_REGEN record, the ack
      one member record per regenerated op: 130, one per row)
Delta stream (every case's stream is in the fixture; these set its size): w_whole_rem is one REMOVE event over 300
  segments, w_whole_ann / w_blocks3_ann one ANNOTATE event with property deltas over 300 / 288.
Afterwards
  af_drain: a whole-document remove of 300 rows, then NOOPs that take the minSeq past it: every row unlinks, the
      tree drains to the reference's empty shape
  af_merge: 300 rows with equal properties, a whole-document annotate, the same step: rows merge up to the
      granularity rule
Tiled-only (one-unit rows with distinct properties; profile "tiled", both builds)
  t_settled_2060: 2,200 rows, settled 1,500 at a time (NOOPs move the minSeq past the inserts: the rows are STABLE,
      and the window set never holds more than one stretch), client 2 removes 2,060:
      more window-set entries than the narrow build holds (2,048): it hands the document to the wide build
  Ends in different chunks: every 300-row case above replays in the tiled profile too, its ends 70 leaves apart.
  Ends in different 64-chunk groups need 64 x 64 leaves = 16k rows between them, over 16k records: left out.
  tiles_cover false (a remote refSeq below the minSeq) cannot be reached by an op of a well-formed log: the
      minSeq never passes a connected client's refSeq; mt_core.h names it "reads only". No case.
Caps (CAP_CASES; the test accepts the reference's digest or MT_E_CAPACITY at the record that needs the room)
  cap_window_4200: 4,300 settled rows, client 2 removes 4,200 (tiled)
  cap_overlap_80x10: clients 2..11 remove the same 80 rows concurrently: the tenth remove is the ninth overlap entry
      of each row
  cap_group_small: replica 5 annotates 300 rows three times locally, then removes them locally: the remove's 300
      membership entries pass the small profile's 1,024
Local references (REF_NAMES; MT_OP_REF records replay only where rcap > 0: the host core with rcap, one GPU batch)
  rf_wide_remove: references on rows 5, 100, 127, 128, 129, 200, 260, 295 (three wave blocks, and outside the
      range), alternately SlideOnRemove and simple, then client 2 removes rows [2, 290); the fixture holds the
      reference's LocalReference.toPosition of each
  rf_wide_remove_drain: the same, then NOOPs take the minSeq past the remove: the rows unlink
The deviations from the planned list are recorded in DESIGN.md §6.
"""
from __future__ import annotations

from typing import List, Optional

from fluidframework_amd import oplog as ol
import zamboni_logs as zl
from zamboni_logs import Case

LOCAL = 5
ALL = zl.ALL
TILED = frozenset({"tiled"})
MAXN = 8           # row slots of a leaf (mt_core.h)
BLOCK = 256        # slots of a wave block: 64 lanes x 4 (range_op's find pass and visit loop)
OPF_REGEN = ol.OPF_REGEN


def slots(segs) -> List[int]:
    """slot of every row of a parsed dump: leaf ordinal x 8 + its index in the leaf"""
    out, at = [], {}
    for s in segs:
        j = at.get(s["leaf"], 0)
        at[s["leaf"]] = j + 1
        out.append(s["leaf"] * MAXN + j)
    return out


def tag(name: str, i: int = 0) -> str:
    return f"w:{name}" + (f":{i}" if i else "")


class _R(zl._Doc):
    """zamboni_logs._Doc with sequenced ops at any refSeq, annotates, local range ops and their acks"""

    def hdr(self, client, ref_seq=None):
        self.seq += 1
        return dict(client=client, seq=self.seq, ref_seq=self.seq - 1 if ref_seq is None else ref_seq, min_seq=self.min)

    def mark(self):
        self.cut = len(self.log.ops)

    def base(self, n: int, kind: str = "text", unit: Optional[int] = None, props=None, marker_every: int = 0):
        """n appended rows of client 1; returns the row starts P (P[r]: position of row r, P[n]: the length)"""
        P = [0]
        for r in range(n):
            L = unit or 1 + r % 3
            pr = props(r) if callable(props) else props
            if marker_every and r % marker_every == marker_every - 1:
                L = 1
                self.ins(self.length, marker=0, props=pr)
            elif kind == "text":
                self.ins(self.length, text=zl._txt(L, r), props=pr)
            elif kind == "run":
                self.ins(self.length, items=zl._items(L, r), props=pr)
            else:
                self.ins(self.length, perm=L, props=pr)
            P.append(P[-1] + L)
        return P

    def insert(self, pos, text, client, ref_seq=None):
        self.log.add(ol.OP_INSERT, pos1=pos, text=text, **self.hdr(client, ref_seq))

    def remove(self, a, b, client=2, ref_seq=None) -> int:
        self.log.add(ol.OP_REMOVE, pos1=a, pos2=b, **self.hdr(client, ref_seq))
        return self.seq

    def annotate(self, a, b, props, client=2, ref_seq=None, combining=ol.COMBINE_NONE) -> int:
        self.log.add(ol.OP_ANNOTATE, pos1=a, pos2=b, props=props, combining=combining, **self.hdr(client, ref_seq))
        return self.seq

    def local(self, kind, a, b, props=None, combining=ol.COMBINE_NONE):
        """a local range op of the replica; returns what its ack needs"""
        self.log.add(kind | ol.OPF_LOCAL, pos1=a, pos2=b, props=props, combining=combining)
        return (kind, a, b, props, combining, self.seq)

    def ack(self, pending) -> int:
        kind, a, b, props, combining, ref = pending
        self.log.add(kind, pos1=a, pos2=b, props=props, combining=combining, **self.hdr(self.log.local_long_id, ref))
        return self.seq


def _sel_removed(seq):
    return lambda hdr, segs: [i for i, s in enumerate(segs) if s["removedSeq"] == seq]


def _sel_value(it, key, value):
    pair = (it.key(key), it.value(value))
    return lambda hdr, segs: [i for i, s in enumerate(segs) if pair in [tuple(p) for p in s["props"]]]


def _W(sel, n=None, nmin=None, leaves=None, straddle=False, blocks=None, at=None, extra=None):
    """witness: the rows `sel` picks are n (at least nmin), span at least `leaves` leaves and `blocks` wave blocks,
    lie on both sides of a 256-slot boundary (`straddle`), their first and last slots are `at`"""
    def w(hdr, segs):
        idx = sel(hdr, segs)
        sl = slots(segs)
        ts = [sl[i] for i in idx]
        if n is not None and len(idx) != n:
            return False
        if nmin is not None and len(idx) < nmin:
            return False
        if (n or nmin) and not ts:
            return False
        if leaves is not None and len({segs[i]["leaf"] for i in idx}) < leaves:
            return False
        if straddle and min(ts) // BLOCK == max(ts) // BLOCK:
            return False
        if blocks is not None and len({t // BLOCK for t in ts}) < blocks:
            return False
        if at is not None and (min(ts), max(ts)) != at:
            return False
        return extra is None or bool(extra(hdr, segs, idx))
    return w


def _pos(P, spec):
    """(row, offset) -> position; an int is a position"""
    return spec if isinstance(spec, int) else P[spec[0]] + spec[1]


def _width(it, name, branch, n, a, b, wkw, kind="text", unit=None, pre=None, ops=("rem", "ann"), profiles=ALL,
           marker_every=0, touched=None) -> List[Case]:
    out = []
    for op in ops:
        d = _R(it)
        P = d.base(n, kind, unit, marker_every=marker_every)
        if pre:
            pre(d, P)
        d.mark()
        pa = a(P) if callable(a) else _pos(P, a)
        pb = b(P) if callable(b) else _pos(P, b)
        full = f"{name}_{op}"
        if op == "rem":
            sel = _sel_removed(d.remove(pa, pb))
        else:
            d.annotate(pa, pb, {"w": tag(full)})
            sel = _sel_value(it, "w", tag(full))
        kw = dict(wkw)
        if touched is not None:
            kw["n"] = touched
        out.append(Case(full, branch, d.log, d.cut, _W(sel, **kw), profiles, kind))
    return out


def _unchanged(n):
    return lambda hdr, segs, idx: len(segs) == n


def _fill_leaf2(d, P):
    """three rows of client 1 inside leaf 2 (rows 8..11): the leaf holds 7"""
    for k in range(3):
        d.insert(P[9], "QZ"[k % 2] * 2, 1)
    # the rows after position P[9] moved by 6 units


def _fullleaf_split(h, s, idx):
    """leaf 2 held rows 8, Q, Q, Q, 9, 10, 11; the start split of row 10 made it 8 rows: it split 4 + 4, so leaf 2 is
    [8, Q, Q, Q], leaf 3 is [9, 10 left, 10 right, 11] (one leaf more than the 75 appended), and the first touched
    row is 10's right part at slot 3 * 8 + 2"""
    lv = [x["leaf"] for x in s]
    return (len(s) == 305 and h["nleaf"] == 76 and lv.count(2) == 4 and lv.count(3) == 4 and idx[0] == 14
            and slots(s)[idx[0]] == 26 and [x["len"] for x in s[12:16]] == [3, 1, 2, 3]
            and [x["text"] for x in s[9:12]] == ["QQ", "ZZ", "QQ"])


def _sameleaf(first_row, last_row, nrows):
    """both ends inside rows of one leaf: the start split moves the last row (to the next slot, or with a full leaf
    to the new sibling) before the end is split; the touched rows are the right part of the first row .. the left
    part of the last, and the rows around them keep their lengths"""
    def w(h, s, idx):
        a, b = idx[0], idx[-1]
        return (len(s) == nrows + 2 and idx == list(range(a, b + 1)) and s[a - 1]["len"] + s[a]["len"] == 3
                and s[b]["len"] + s[b + 1]["len"] == 3 and a == first_row + 1
                and all(x["len"] == 3 for x in s[a + 1:b] if x["text"][0] not in "QZ"))
    return w


def width_cases(it) -> List[Case]:
    out = []
    out += _width(it, "w_sameleaf", "both ends inside rows of one leaf: the start split shifts the last row", 40,
                  (9, 1), (11, 2), dict(n=3, extra=_sameleaf(9, 11, 40)), unit=3)
    out += _width(it, "w_sameleaf_full", "the same in a leaf of 7 rows: the start split moves the last row to a new leaf",
                  40, (8, 1), lambda P: P[11] + 6 + 2, dict(n=7, extra=_sameleaf(8, 14, 43)), unit=3, pre=_fill_leaf2)
    out += _width(it, "w_leaf1", "one whole leaf", 40, (8, 0), (12, 0), dict(n=4, at=(16, 19)))
    out += _width(it, "w_leaf2", "exactly two leaves", 40, (8, 0), (16, 0), dict(n=8, at=(16, 27)))
    out += _width(it, "w_l33", "33 leaves, ending on the first row past slot 256", 160, (0, 0), (129, 0),
                  dict(n=129, leaves=33, straddle=True, at=(0, 256)))
    out += _width(it, "w_edge256", "first row the last slot below 256, last row slot 256", 160, (127, 0), (129, 0),
                  dict(n=2, straddle=True, at=(251, 256)))
    out += _width(it, "w_blocks3", "three wave blocks", 300, (2, 0), (290, 0), dict(n=288, leaves=65, blocks=3))
    out += _width(it, "w_whole", "the whole document", 300, (0, 0), (300, 0), dict(n=300, leaves=75, blocks=3))
    out += _width(it, "w_pastend", "end past the length: clipped", 160, (100, 0), lambda P: P[160] + 50,
                  dict(n=60, straddle=True))
    out += _width(it, "w_empty_start", "start = length: nothing changes", 160, (160, 0), lambda P: P[160] + 5,
                  dict(n=0, extra=_unchanged(160)))
    out += _width(it, "w_empty_end", "end = start: nothing changes", 160, (50, 0), (50, 0),
                  dict(n=0, extra=_unchanged(160)))
    out += _width(it, "w_empty_neg", "end < start: nothing changes", 160, (130, 0), (20, 0),
                  dict(n=0, extra=_unchanged(160)))
    for nm, oa, ob in (("bb", 0, 0), ("bi", 0, 1), ("ib", 2, 0), ("ii", 1, 2)):
        out += _width(it, f"w_sp_{nm}", "start " + ("inside a row" if oa else "on a row boundary") + ", end " +
                      ("inside a row" if ob else "on a row boundary"), 160, (20, oa), (140, ob),
                      dict(n=120 + (1 if ob else 0), straddle=True,
                           extra=lambda h, s, idx, k=160 + (1 if oa else 0) + (1 if ob else 0): len(s) == k), unit=3)
    out += _width(it, "w_fullleaf", "the first split splits a full leaf and shifts every later slot", 300,
                  lambda P: P[10] + 6 + 1, lambda P: P[290] + 6 + 1, dict(n=281, leaves=65, blocks=3,
                  extra=_fullleaf_split), unit=3, pre=_fill_leaf2)
    out += _width(it, "w_onerow", "both ends inside one row (the small control)", 40, (9, 1), (9, 2),
                  dict(n=1, extra=lambda h, s, idx: len(s) == 42 and s[idx[0]]["len"] == 1), unit=3)
    for q in range(4):
        out += _width(it, f"w_quad{q}", f"the visit starts at quad offset {q}", 160, (8 + q, 0), (141, 0),
                      dict(n=133 - q, straddle=True, at=(16 + q, 35 * 8)))
    return out


def _persp(it, name, branch, build, nmin, kind="text", local=0, ops=("rem", "ann"), marker_every=0, wkw=None,
           base_props=None) -> List[Case]:
    """build(d, P, op, full) appends the mix and the wide op(s); returns the selector of the rows the wide op touched"""
    out = []
    for op in ops:
        d = _R(it, local=local)
        P = d.base(300, kind, marker_every=marker_every, props=base_props)
        full = f"{name}_{op}"
        sel = build(d, P, op, full)
        kw = dict(nmin=nmin, straddle=True)
        kw.update(wkw or {})
        out.append(Case(full, branch, d.log, d.cut, _W(sel, **kw), ALL, kind))
    return out


def _wide(d, it, op, full, a, b, client=2, ref_seq=None, i=0):
    if op == "rem":
        return _sel_removed(d.remove(a, b, client, ref_seq))
    d.annotate(a, b, {"w": tag(full, i)}, client, ref_seq)
    return _sel_value(it, "w", tag(full, i))


def persp_cases(it) -> List[Case]:
    out = []

    def later_inserts(d, P, op, full):
        R = d.seq
        for r in range(240, 40, -5):  # descending: earlier positions keep their base coordinates
            d.insert(P[r], "L", 3)
        d.mark()
        return _wide(d, it, op, full, P[30], P[260], ref_seq=R)
    out += _persp(it, "p_later_inserts", "rows inserted after the refSeq by another client", later_inserts, 230,
                  wkw=dict(n=230))

    def own_later(d, P, op, full):
        R = d.seq
        own = 0
        for k, r in enumerate(range(290, 50, -4)):  # 60 inserts, alternately client 2's (at refSeq R) and client 3's
            if k % 2 == 0:
                d.insert(P[r], "o", 2, ref_seq=R)
                own += 1
            else:
                d.insert(P[r], "x", 3, ref_seq=R)
        d.mark()
        return _wide(d, it, op, full, 0, P[300] + own, ref_seq=R)
    out += _persp(it, "p_own_later", "the op's own client's later inserts are seen, another client's are not",
                  own_later, 330, wkw=dict(n=330))

    def removed_before(d, P, op, full):
        gone = 0
        for r in range(258, 30, -3):
            d.remove(P[r], P[r + 1], 3)
            gone += P[r + 1] - P[r]
        d.mark()
        return _wide(d, it, op, full, P[30], P[260] - gone)
    out += _persp(it, "p_removed_before", "rows removed before the refSeq", removed_before, 150,
                  wkw=dict(n=230 - 76))

    def overlap(d, P, op, full):
        R = d.seq
        for r in range(256, 30, -4):
            d.remove(P[r], P[r + 1], 3)
        d.mark()
        sel = _wide(d, it, op, full, P[30], P[260], ref_seq=R)
        if op == "ann":
            return sel
        return lambda h, s: [i for i, x in enumerate(s) if x["removedSeq"] is not None and
                             (x["removedSeq"] == d.seq or len(x["overlap"]) == 1)]
    out += _persp(it, "p_overlap", "rows removed after the refSeq by another client: overlap push", overlap, 230,
                  wkw=dict(n=230, extra=lambda h, s, idx: True))

    def invisible(d, P, op, full):
        d.remove(P[20], P[200], 3)
        d.mark()
        return _wide(d, it, op, full, P[5], P[290] - (P[200] - P[20]))
    out += _persp(it, "p_invisible256", "more than 256 consecutive invisible slots inside the range", invisible, 105,
                  wkw=dict(n=105, blocks=2, extra=lambda h, s, idx: max(
                      b - a for a, b in zip([slots(s)[i] for i in idx], [slots(s)[i] for i in idx][1:])) > BLOCK + 8))

    def twice(d, P, op, full):
        d.remove(P[50], P[150], 2)
        d.mark()
        return _wide(d, it, op, full, P[10], P[250] - (P[150] - P[50]))
    out += _persp(it, "p_twice", "a range over rows the same client already removed", twice, 140, wkw=dict(n=140))

    def plain(d, P, op, full):
        d.mark()
        return _wide(d, it, op, full, P[3], P[297])
    out += _persp(it, "p_markers", "markers in the range", plain, 294, marker_every=7, wkw=dict(n=294))
    out += _persp(it, "p_perm", "PermutationSegment rows in the range", plain, 294, kind="perm", ops=("rem",),
                  wkw=dict(n=294))
    out += _persp(it, "p_items", "a {items} document", plain, 294, kind="run", wkw=dict(n=294))

    # local pending removes under a remote remove, and the reverse
    d = _R(it, local=LOCAL)
    P = d.base(300)
    p1 = d.local(ol.OP_REMOVE, P[200], P[210])
    p0 = d.local(ol.OP_REMOVE, P[50], P[60])
    d.mark()
    s = d.remove(P[10], P[290], 2)
    d.ack(p1), d.ack(p0)
    out.append(Case("p_unas", "a remote remove over rows under a local pending remove", d.log, d.cut,
                    _W(_sel_removed(s), n=280, blocks=3,  # the 20 rows took the remote's seq, not their acks'
                       extra=lambda h, segs, idx: all(x["removedSeq"] in (None, s) and x["ngroups"] == 0 for x in segs)),
                    ALL, "text"))
    d = _R(it, local=LOCAL)
    P = d.base(300)
    p0 = d.local(ol.OP_REMOVE, P[10], P[290])
    d.mark()
    s1 = d.remove(P[100], P[104], 2)
    s2 = d.remove(0, P[300] - (P[104] - P[100]), 2)
    d.ack(p0)
    out.append(Case("p_unas_rev", "remote removes land inside and over a wide local pending remove", d.log, d.cut,
                    _W(lambda h, segs: [i for i, x in enumerate(segs) if x["removedSeq"] in (s1, s2)], n=300, blocks=3,
                       extra=lambda h, segs, idx: sum(1 for x in segs if x["removedSeq"] == s1) == 4), ALL, "text"))
    return out


def _local_case(it, name, branch, nrows, kind, props=None, combining=ol.COMBINE_NONE, base_props=None) -> Case:
    d = _R(it, local=LOCAL)
    P = d.base(300 if nrows > 129 else 160, props=base_props)
    a = 0 if nrows >= 300 else 3
    pend = d.local(kind, P[a], P[a + nrows], props, combining)
    d.mark()
    s = d.ack(pend)
    d.step(drain=2)
    if kind == ol.OP_REMOVE:  # the step unlinks the first of the rows; the others still carry the ack's seq
        total = 300 if nrows > 129 else 160
        w = lambda h, segs: h["minSeq"] >= s and h["length"] == P[total] - (P[a + nrows] - P[a]) and \
            0 < sum(1 for x in segs if x["removedSeq"] == s) <= nrows and len(segs) < total and \
            all(x["removedSeq"] in (None, s) and x["ngroups"] == 0 for x in segs)  # noqa: E731
    else:
        k, v = list(props.items())[-1]
        pair = (it.key(k), it.value(v))
        w = lambda h, segs: h["minSeq"] >= s and all(x["ngroups"] == 0 for x in segs) and \
            sum(x["len"] for x in segs if pair in [tuple(p) for p in x["props"]]) == P[a + nrows] - P[a]  # noqa: E731
    return Case(name, branch, d.log, d.cut, w, ALL, "text")


def local_cases(it) -> List[Case]:
    out = []
    ab = lambda r: {"a": r % 5, "b": "v"}  # noqa: E731
    for n in (65, 129, 300):
        out.append(_local_case(it, f"lg_rem_{n}", f"ack of a local remove of {n} rows", n, ol.OP_REMOVE))
        out.append(_local_case(it, f"lg_ann2_{n}", f"ack of a local annotate of {n} rows, two keys", n, ol.OP_ANNOTATE,
                               {"a": 900 + n, "b": tag(f"lg_ann2_{n}")}, base_props=ab))
        out.append(_local_case(it, f"lg_annrw_{n}", f"ack of a local rewrite annotate of {n} rows", n, ol.OP_ANNOTATE,
                               {"a": 800 + n, "b": tag(f"lg_annrw_{n}")}, ol.COMBINE_REWRITE, base_props=ab))
    out.append(_local_case(it, "lg_ann_newkey", "ack of a local annotate with a key the document has not seen", 129,
                           ol.OP_ANNOTATE, {"z9": tag("lg_ann_newkey")}))
    for name, second in (("lg_two_ann", ol.OP_ANNOTATE), ("lg_ann_rem", ol.OP_REMOVE)):
        d = _R(it, local=LOCAL)
        P = d.base(300)
        p0 = d.local(ol.OP_ANNOTATE, P[0], P[200], {"w": tag(name)})
        p1 = d.local(second, P[100], P[300], {"w": tag(name, 1)} if second == ol.OP_ANNOTATE else None)
        mid = len(d.log.ops)
        d.mark()
        d.ack(p0)
        s1 = d.ack(p1)
        if second == ol.OP_ANNOTATE:
            w = _W(_sel_value(it, "w", tag(name, 1)), n=200, blocks=2,
                   extra=lambda h, segs, idx, pr=(it.key("w"), it.value(tag(name))): sum(
                       1 for x in segs if pr in [tuple(p) for p in x["props"]]) == 100 and
                   all(x["ngroups"] == 0 for x in segs))
        else:
            w = _W(_sel_removed(s1), n=200, blocks=2, extra=lambda h, segs, idx: all(x["ngroups"] == 0 for x in segs))
        assert mid == d.cut
        out.append(Case(name, "two overlapping wide local groups acked in order", d.log, d.cut, w, ALL, "text"))
    out.append(_regen_case(it))
    return out


REGEN_OPS = 130  # regeneratePendingOp makes one remove op per row of the group (client.ts resetPendingDeltaToOps)


def _regen_case(it) -> Case:
    """a wide local remove, a reconnect, the resubmitted message's ack: one member record per regenerated op
    (REGEN_OPS; tests/test_ref_ranges.py checks it against the host core's MT_DELTA_REGEN event, as
    tests/regen_inject.py counts them)"""
    d = _R(it, local=LOCAL)
    P = d.base(160)
    d.local(ol.OP_REMOVE, P[10], P[140])
    ref = d.seq
    d.log.add(ol.OP_REMOVE | ol.OPF_LOCAL | OPF_REGEN)
    d.mark()
    d.seq += 1
    for q in range(REGEN_OPS):
        d.log.add(ol.OP_REMOVE | (ol.OPF_GROUPED if q < REGEN_OPS - 1 else 0), client=LOCAL, seq=d.seq, ref_seq=ref,
                  min_seq=0, pos1=P[10], pos2=P[140])
    s = d.seq
    return Case("lg_regen", "a wide local remove, a reconnect, the regenerated ops' ack", d.log, d.cut,
                _W(_sel_removed(s), n=130, straddle=True,
                   extra=lambda h, segs, idx: all(x["ngroups"] == 0 and x["localRemovedSeq"] <= 0 for x in segs)),
                ALL, "text")


def after_cases(it) -> List[Case]:
    out = []
    d = _R(it)
    P = d.base(300)
    d.mark()
    d.remove(0, P[300], 2)
    d.step(drain=160)
    out.append(Case("af_drain", "every row unlinks, the tree drains", d.log, d.cut,
                    lambda h, segs: h["length"] == 0 and len(segs) == 0, ALL, "text"))
    d = _R(it)
    P = d.base(300, props={"k0": 1})
    d.mark()
    d.annotate(0, P[300], {"w": tag("af_merge")}, 2)
    d.step(drain=160)
    out.append(Case("af_merge", "rows merge up to the granularity rule across the whole document", d.log, d.cut,
                    lambda h, segs: h["length"] == P[300] and len(segs) < 40 and max(x["len"] for x in segs) > 256
                    and all(len(x["props"]) == 2 for x in segs), ALL, "text"))
    return out


SLIDE = 0x40  # ReferenceType.SlideOnRemove (ops.ts)
REF_ROWS = (5, 100, 127, 128, 129, 200, 260, 295)  # rows that hold a local reference: three wave blocks, and outside
REF_NAMES = ("rf_wide_remove", "rf_wide_remove_drain")


def ref_cases(it) -> List[Case]:
    """local references of the observer replica (MT_OP_REF records: client-feature builds, rcap > 0) on rows of
    three wave blocks, alternately SlideOnRemove and simple, then client 2 removes rows [2, 290): the references on
    the removed rows stay with them (LocalReference.toPosition of a removed segment's reference; the fixture holds
    the reference's answers); _drain then moves the minSeq past the remove: the rows unlink and their references
    slide or detach"""
    out = []
    for name, drain in zip(REF_NAMES, (False, True)):
        d = _R(it)
        P = d.base(300)
        for k, r in enumerate(REF_ROWS):
            d.log.add(ol.OP_REF | ol.OPF_LOCAL, pos1=P[r] + k % 2, pos2=SLIDE if k % 2 == 0 else 0)
        d.mark()
        s = d.remove(P[2], P[290], 2)
        if drain:
            d.step(drain=160)
            w = lambda h, segs: len(segs) <= 12 and h["length"] == P[2] + P[300] - P[290] and \
                all(x["removedSeq"] is None for x in segs)  # noqa: E731
        else:
            w = _W(_sel_removed(s), n=288, blocks=3)
        out.append(Case(name, "references on removed rows across a wide remove" + (", then the drain" if drain else ""),
                        d.log, d.cut, w, ALL, "text"))
    return out


def _settled(it, n, nrem, name, branch) -> Case:
    d = _R(it)
    for at in range(0, n, 1500):  # settled 1,500 at a time: the rows of one stretch are all the window set holds
        for r in range(at, min(n, at + 1500)):
            d.ins(d.length, text=zl._txt(1, r), props={"p": r})
        d.step(drain=2)
    d.mark()
    s = d.remove(20, 20 + nrem, 2)
    return Case(name, branch, d.log, d.cut, _W(_sel_removed(s), n=nrem), TILED, "text")


def tiled_cases(it) -> List[Case]:
    return [_settled(it, 2200, 2060, "t_settled_2060", "more window-set entries than the narrow build holds")]


def cap_cases(it) -> List[Case]:
    """(case, the record that needs the room) in CAP_AT"""
    out = [_settled(it, 4300, 4200, "cap_window_4200", "more window-set entries than WCAP")]
    d = _R(it)
    P = d.base(100)
    R = d.seq
    d.mark()
    seqs = [d.remove(P[10], P[90], c, ref_seq=R) for c in range(2, 12)]
    out.append(Case("cap_overlap_80x10", "the ninth overlap entry of 80 rows", d.log, len(d.log.ops) - 1,
                    _W(_sel_removed(seqs[0]), n=80, extra=lambda h, segs, idx: all(len(segs[i]["overlap"]) == 9
                                                                                   for i in idx)), ALL, "text"))
    d = _R(it, local=LOCAL)
    P = d.base(300)
    for i in range(3):
        d.local(ol.OP_ANNOTATE, 0, P[300], {"w": tag("cap_group_small", i)})
    d.mark()
    d.local(ol.OP_REMOVE, 0, P[300])
    out.append(Case("cap_group_small", "a local group past the small profile's membership log", d.log, d.cut,
                    lambda h, segs: len(segs) == 300 and all(x["ngroups"] == 4 and x["localRemovedSeq"] == 4
                                                             for x in segs), ALL, "text"))
    return out


CAP_NAMES = ("cap_window_4200", "cap_overlap_80x10", "cap_group_small")
_CACHE = {}


def _all():
    if not _CACHE:
        it = ol.Interner()
        for v in range(300):  # SubSequence items: the integer v has item id v
            assert it.item(v) == v
        cs = width_cases(it) + persp_cases(it) + local_cases(it) + after_cases(it) + ref_cases(it) + tiled_cases(it)
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
    """the cap cases: `cut` is the index of the record that needs the room"""
    return list(_all()["caps"])


def batch(which: Optional[List[Case]] = None) -> ol.Batch:
    cs = cases() if which is None else which
    return ol.Batch.from_logs([c.log for c in cs])


def split_at_cut(cs: List[Case]):
    """The batch in two parts, cut before each document's first wide op (an ack case: before the ack)"""
    b = batch(cs)
    head, tail = [], []
    for d, c in enumerate(cs):
        ops, text, props, kv = b.doc_arrays(d)
        head.append((ops[: c.cut], text, props, kv))
        tail.append((ops[c.cut:], text, props, kv))
    return ol.Batch.from_arrays(head, b.local_long_id), ol.Batch.from_arrays(tail, b.local_long_id)


def census(parsed, values) -> dict:
    """Over parsed dumps [(hdr, segs)] and their interner's value table: the ops whose touched rows a dump still
    shows (a remove by its removedSeq; an annotate by a value "w:..." only it writes) -> how many touched more than
    64 rows, more than 64 rows on both sides of a 256-slot boundary (`narrow_straddle`: at most 64 rows, on both sides:
    a generator op of a few rows does that where it happens to lie on slot 256 k), more than 256 rows; the widest."""
    wide = {i for i, v in enumerate(values) if v.startswith('"w:')}
    out = dict(over64=0, straddle=0, narrow_straddle=0, over256=0, widest=0, ops=0)
    for hdr, segs in parsed:
        sl = slots(segs)
        groups = {}
        for i, s in enumerate(segs):
            if s["removedSeq"] is not None:
                groups.setdefault(("r", s["removedSeq"]), []).append(sl[i])
            for k, v in s["props"]:
                if isinstance(v, int) and (v & ~ol.VALUE_FALSY) in wide:
                    groups.setdefault(("a", k, v), []).append(sl[i])
        for ts in groups.values():
            out["ops"] += 1
            out["over64"] += len(ts) > 64
            out["over256"] += len(ts) > 256
            out["straddle"] += len(ts) > 64 and min(ts) // BLOCK != max(ts) // BLOCK
            out["narrow_straddle"] += len(ts) <= 64 and min(ts) // BLOCK != max(ts) // BLOCK
            out["widest"] = max(out["widest"], len(ts))
    return out
