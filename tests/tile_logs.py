"""Hand-built logs for the marker queries: Client.findTile (client.ts:1075 -> MergeTree.findTile, mergeTree.ts:
1796-1822, search / backwardSearch 1030-1069, addNodeReferences 262-300) and Client.getStackContext (client.ts:948 ->
mergeTree.ts:1783-1793, applyRangeReference 245-260, recordRangeLeaf / rangeShift 987-1028) -- test infrastructure for
tests/test_ref_tiles.py and tools/make_ref_goldens.py --tiles.

Every case is one document: rows appended by client 1 under a minSeq held at 0, one unit each, four to a leaf (a leaf
of 8 splits 4 + 4), so row r sits at slot (r // 4) * 8 + r % 4 and a pass of the wave walk (8 leaves x 8 slots) holds 32
rows: rows 31 / 32 are the last and the first row of passes 0 and 1 (slots 59 / 64), rows 127 / 128 lie on both sides of
slot 256 (slots 251 / 256). A leaf at rest holds at most 7 rows, so slots 63 and 255 are never occupied; three more
rows inserted into the last leaf of a pass fill it to 7, which puts its last row at slot 62 / 254, next to the pass's
last lane. The witnesses read slots from the dump (range_logs.slots).

A case names its queries: `tiles` = [(label, pos or None, preceding)], `stacks` = [(label, pos or None)]; pos None is
the reference's undefined. The tile label is "pg" (and "row"), the range label "li" (and "q") unless stated.

Case list
Smallest shapes that can go wrong
  f_same_leaf: the tile in the stop row's leaf; the stop row a text row, and the stop row the tile itself
  f_prev_leaf: the tile in the leaf before / after the stop row's
  f_earlier_pass: the tile more than 64 slots before (forward) / after (backward) the stop row
  e_32_lo / e_32_hi / e_128_lo / e_128_hi: the tile is the last row below a pass boundary (rows 31, 127) or the
      first above it (rows 32, 128), the stop row on either side
  e_32_full / e_128_full: the last leaf below the boundary holds 7 rows: the tile at slot 62 / 254, the next row at
      slot 64 / 256
Row states
  r_removed_remote / r_removed_pending / r_removed_acked: the nearest tile is removed by another client / by the
      replica, unacked / by the replica, acked: skipped
  z_zero_last: the last row is a removed text row: the backward stop at pos = length
  z_zero_last_tile: the last row is a removed tile: the backward stop at pos = length is that row
Positions
  p_positions: pos undefined, 0, the length and above the length, both directions
Label and refType mismatches
  m_mismatch: between the tile and the stop row lie a marker with Tile and no properties, a marker with the label and
      refType Simple, and a text row that carries the label property; the tile holds a two-label array; a label no
      array holds; a marker with Tile | NestBegin
Several labels
  l_two: tiles of "pg" and of "row" interleaved, queried separately
Stacks
  s_bbe: begin begin end; the stop row a begin
  s_end_open: an end with nothing open (pushed), an end after it (pushed), a begin, its end
  s_both_bits: a marker with NestBegin | NestEnd (a begin), then an end
  s_two_labels: a begin with two range labels, an end with one of them
  s_removed_begin: a removed begin is skipped
  s_past_end: pos = length and past it
  s_deep70: 70 begins, then 70 ends in later passes (final depth 0, high-water 70)
  s_pass_pop: one pass pops what two earlier passes pushed
Profiles and routing
  x_items: a {items} document with markers
  x_perm: PermutationSegment rows with markers (the matrix build's batch)
  x_keys24: rows with 24 property keys (the profiles with 24 key slots)
  x_tiled_chunks: more than 64 leaves, tiles in two chunks of the tiled profile's rope
  x_promote: 800 scattered inserts: a small build hands the document to a larger one (PROMOTED)
  k_mkmask: an annotate changes referenceTileLabels / referenceRangeLabels on a marker: the engine refuses (REFUSED)
"""
from __future__ import annotations

from typing import Callable, List, NamedTuple, Optional

from fluidframework_amd import oplog as ol
import zamboni_logs as zl
from insert_logs import _I
from range_logs import slots, LOCAL

ALL = zl.ALL
WIDE_KEYS = zl.WIDE_KEYS
TK, RK = ol.TILE_LABELS_KEY, ol.RANGE_LABELS_KEY
TILE, BEGIN, END = ol.REF_TILE, ol.REF_NEST_BEGIN, ol.REF_NEST_END
UNAS = -1
REFUSED = ("k_mkmask",)
PROMOTED = ("x_promote",)


class TCase(NamedTuple):
    name: str
    branch: str
    log: ol.DocLog
    tiles: list         # [(label, pos | None, preceding)]
    stacks: list        # [(label, pos | None)]
    witness: Callable   # (hdr, segs) -> bool over the parsed canonical dump of the reference
    profiles: frozenset
    kind: str           # "text" | "run" | "perm"


def pg(*labels):
    return {TK: list(labels or ("pg",))}


def li(*labels):
    return {RK: list(labels or ("li",))}


def _doc(it, n, marks, kind="text", local=0, props=None):
    """n appended one-unit rows; marks: row -> (refType, props) makes that row a marker"""
    d = _I(it, local=local)
    for r in range(n):
        if r in marks:
            d.ins(d.length, marker=marks[r][0], props=marks[r][1])
        elif kind == "text":
            d.ins(d.length, text=zl._txt(1, r), props=props(r) if props else None)
        elif kind == "run":
            d.ins(d.length, items=zl._items(1, r))
        else:
            d.ins(d.length, perm=1)
    return d


def _tile_at(*rows, n=None, gone=()):
    """witness: exactly the rows `rows` are Tile markers (n rows in all); the rows `gone` are removed"""
    def w(h, s):
        at = [i for i, x in enumerate(s) if x["kind"] == ol.SEG_MARKER and x["refType"] & TILE]
        return at == sorted(rows) and (n is None or len(s) == n) and all(s[i]["removedSeq"] is not None for i in gone)
    return w


def _both(pos_list, label="pg"):
    return [(label, p, pre) for p in pos_list for pre in (True, False)]


def cases_(it) -> List[TCase]:
    out: List[TCase] = []

    def add(name, branch, d, tiles, stacks, w, profiles=ALL, kind="text"):
        out.append(TCase(name, branch, d.log, tiles, stacks, w, profiles, kind))

    add("f_same_leaf", "the tile and the stop row share a leaf", _doc(it, 40, {21: (TILE, pg())}),
        [("pg", 23, True), ("pg", 20, False), ("pg", 21, True), ("pg", 21, False), ("pg", 22, True), ("pg", 22, False)], [],
        lambda h, s: _tile_at(21, n=40)(h, s) and s[20]["leaf"] == s[21]["leaf"] == s[23]["leaf"]
        and s[23]["kind"] == ol.SEG_TEXT)
    add("f_prev_leaf", "the tile lies in the leaf next to the stop row's", _doc(it, 40, {19: (TILE, pg()), 24: (TILE, pg())}),
        [("pg", 21, True), ("pg", 22, False)], [],
        lambda h, s: _tile_at(19, 24, n=40)(h, s) and s[19]["leaf"] + 1 == s[21]["leaf"] == s[22]["leaf"] == s[24]["leaf"] - 1)
    add("f_earlier_pass", "the tile lies more than 64 slots from the stop row", _doc(it, 100, {3: (TILE, pg()), 95: (TILE, pg())}),
        [("pg", 90, True), ("pg", 5, False), ("pg", 50, True), ("pg", 50, False)], [],
        lambda h, s: _tile_at(3, 95, n=100)(h, s) and slots(s)[90] - slots(s)[3] > 128 and slots(s)[95] - slots(s)[5] > 128)
    for b in (32, 128):
        add(f"e_{b}_lo", f"the tile is the last row below the pass boundary at row {b}", _doc(it, b + 12, {b - 1: (TILE, pg())}),
            _both([b - 2, b - 1, b, b + 5, 0]), [],
            lambda h, s, b=b: _tile_at(b - 1)(h, s) and slots(s)[b - 1] == 2 * b - 5 and slots(s)[b] == 2 * b)
        add(f"e_{b}_hi", f"the tile is the first row above the pass boundary at row {b}", _doc(it, b + 12, {b: (TILE, pg())}),
            _both([b - 1, b, b + 1, b + 5, 0]), [],
            lambda h, s, b=b: _tile_at(b)(h, s) and slots(s)[b] == 2 * b and slots(s)[b - 1] == 2 * b - 5)

    for b in (32, 128):
        d = _doc(it, b + 12, {b - 1: (TILE, pg())})
        for q in range(3):  # into the leaf of rows b - 4 .. b - 1: 7 rows, the tile its last
            d.put(b - 3, 1, text="+")
        add(f"e_{b}_full", f"the leaf below the pass boundary at row {b} holds 7 rows: the tile at slot {2 * b - 2}", d,
            _both([b, b + 1, b + 2, b + 3, b + 8, 0, b - 3]), [],
            lambda h, s, b=b: _tile_at(b + 2)(h, s) and slots(s)[b + 2] == 2 * b - 2 and slots(s)[b + 3] == 2 * b
            and len(s) == b + 15)

    for nm in ("remote", "pending", "acked"):
        d = _doc(it, 40, {10: (TILE, pg()), 20: (TILE, pg()), 30: (TILE, pg())}, local=LOCAL)
        if nm == "remote":
            d.remove(20, 21, 3)
        else:
            p = d.lrem(20, 21)
            if nm == "acked":
                d.ack(p)
        add(f"r_removed_{nm}", f"the nearest tile is removed ({nm}): skipped", d, _both([24, 15, 19, 20]), [],
            lambda h, s, nm=nm: _tile_at(10, 20, 30, n=40, gone=[20])(h, s)
            and (s[20]["removedSeq"] == UNAS) == (nm == "pending")
            and (nm == "pending" or (s[20]["removedClient"] == LOCAL) == (nm == "acked")))
    d = _doc(it, 20, {5: (TILE, pg())})
    d.remove(19, 20, 3)
    add("z_zero_last", "a zero-length last row is the backward stop", d, _both([19, 18, 20]), [],
        lambda h, s: _tile_at(5, n=20, gone=[19])(h, s) and h["length"] == 19)
    d = _doc(it, 20, {5: (TILE, pg()), 19: (TILE, pg())})
    d.remove(19, 20, 3)
    add("z_zero_last_tile", "a removed tile as the last row: the backward stop counts whatever its length", d,
        _both([19, 18, 20, 6]), [], lambda h, s: _tile_at(5, 19, n=20, gone=[19])(h, s) and h["length"] == 19)

    add("p_positions", "pos undefined, 0, the length, above the length", _doc(it, 20, {0: (TILE, pg()), 10: (TILE, pg()), 19: (TILE, pg())}),
        _both([None, 0, 20, 23, 1, 19]), [], lambda h, s: _tile_at(0, 10, 19, n=20)(h, s) and h["length"] == 20)
    add("p_empty", "no tile at all; a label the document has never seen", _doc(it, 12, {}),
        _both([None, 0, 5, 12]), [("li", None), ("li", 3)], lambda h, s: _tile_at(n=12)(h, s))

    d = _doc(it, 40, {5: (TILE, pg("row", "pg")), 10: (TILE, None), 12: (0, pg()), 22: (0, pg()), 24: (TILE, None),
                      30: (TILE | BEGIN, pg("pg"))})
    d.annotate(14, 15, pg(), client=1)
    d.annotate(26, 27, pg(), client=1)
    add("m_mismatch", "impostors between the tile and the stop row; a two-label array; an unknown label", d,
        [("pg", 18, True), ("row", 18, True), ("zz", 18, True), ("pg", 20, False), ("row", 20, False), ("zz", None, False),
         ("pg", 12, True), ("pg", 10, True), ("pg", 24, False)], [],
        lambda h, s: _tile_at(5, 10, 24, 30, n=40)(h, s) and len(s[5]["props"]) == 1 and not s[10]["props"]
        and s[12]["kind"] == ol.SEG_MARKER and s[12]["refType"] == 0 and s[12]["props"]
        and s[14]["kind"] == ol.SEG_TEXT and s[14]["props"] == s[12]["props"] and s[30]["refType"] == TILE | BEGIN)
    add("l_two", "two labels in one document", _doc(it, 24, {5: (TILE, pg()), 8: (TILE, pg("row")), 12: (TILE, pg("row")),
                                                           15: (TILE, pg())}),
        _both([10, 13, 6], "pg") + _both([10, 13, 6], "row"), [], _tile_at(5, 8, 12, 15, n=24))

    # stacks
    def nest(*rows):
        def w(h, s):
            at = [i for i, x in enumerate(s) if x["kind"] == ol.SEG_MARKER and x["refType"] & (BEGIN | END)]
            return at == sorted(rows)
        return w
    add("s_bbe", "begin begin end; the stop row a begin", _doc(it, 12, {2: (BEGIN, li()), 5: (BEGIN, li()), 8: (END, li())}),
        [], [("li", p) for p in (None, 3, 6, 9, 5, 2, 8, 0)], nest(2, 5, 8))
    add("s_end_open", "an end with nothing open is pushed; an end after it too", _doc(
        it, 16, {3: (END, li()), 6: (END, li()), 9: (BEGIN, li()), 12: (END, li())}),
        [], [("li", p) for p in (None, 4, 7, 10, 13, 3)], nest(3, 6, 9, 12))
    add("s_both_bits", "NestBegin | NestEnd counts as a begin", _doc(it, 12, {4: (BEGIN | END, li()), 8: (END, li())}),
        [], [("li", p) for p in (None, 5, 9, 4)],
        lambda h, s: nest(4, 8)(h, s) and s[4]["refType"] == BEGIN | END)
    add("s_two_labels", "two range labels on one marker", _doc(it, 12, {2: (BEGIN, li("li", "q")), 6: (END, li("q"))}),
        [], [(lb, p) for lb in ("li", "q", "zz") for p in (None, 3, 7)],
        lambda h, s: nest(2, 6)(h, s) and s[2]["props"] != s[6]["props"])
    d = _doc(it, 12, {2: (BEGIN, li()), 5: (BEGIN, li()), 9: (END, li())})
    d.remove(2, 3, 3)
    add("s_removed_begin", "a removed begin is skipped", d, [], [("li", p) for p in (None, 3, 6, 10)],
        lambda h, s: nest(2, 5, 9)(h, s) and s[2]["removedSeq"] is not None)
    add("s_past_end", "pos = length and past the end", _doc(it, 12, {2: (BEGIN, li()), 11: (BEGIN, li())}),
        [], [("li", p) for p in (12, 17, 11)], lambda h, s: nest(2, 11)(h, s) and h["length"] == 12)
    marks = {r: (BEGIN, li()) for r in range(70)}
    marks.update({r: (END, li()) for r in range(100, 170)})
    add("s_deep70", "70 nested begins, then 70 ends in later passes", _doc(it, 200, marks),
        [], [("li", p) for p in (None, 85, 120, 69, 35, 169, 170)],
        lambda h, s: nest(*range(70), *range(100, 170))(h, s) and slots(s)[100] - slots(s)[69] > 56)
    add("s_pass_pop", "one pass pops what two earlier passes pushed", _doc(
        it, 80, {10: (BEGIN, li()), 40: (BEGIN, li()), 70: (END, li()), 71: (END, li())}),
        [], [("li", p) for p in (None, 50, 71, 72)],
        lambda h, s: nest(10, 40, 70, 71)(h, s) and slots(s)[10] // 64 == 0 and slots(s)[40] // 64 == 1
        and slots(s)[70] // 64 == slots(s)[71] // 64 == 2)

    # profiles and routing
    mk = {4: (TILE, pg()), 9: (BEGIN, li()), 30: (TILE, pg()), 33: (END, li())}
    qs = _both([20, 35, None])
    ss = [("li", p) for p in (None, 20, 34)]
    add("x_items", "a {items} document with markers", _doc(it, 40, mk, kind="run"), qs, ss,
        lambda h, s: _tile_at(4, 30, n=40)(h, s) and s[0]["kind"] == ol.SEG_RUN, kind="run")
    add("x_perm", "PermutationSegment rows with markers", _doc(it, 40, mk, kind="perm"), qs, ss,
        lambda h, s: _tile_at(4, 30, n=40)(h, s) and s[0]["kind"] == ol.SEG_PERM, kind="perm")
    keys = {f"k{q}": q for q in range(22)}
    add("x_keys24", "24 property keys: the label keys take the last slots", _doc(it, 40, mk, props=lambda r: keys), qs, ss,
        lambda h, s: _tile_at(4, 30, n=40)(h, s) and len(s[0]["props"]) == 22, WIDE_KEYS)
    mk = {10: (TILE, pg()), 20: (BEGIN, li()), 290: (TILE, pg()), 295: (END, li())}
    add("x_tiled_chunks", "more than 64 leaves: tiles in two chunks of the rope", _doc(it, 300, mk),
        _both([150, 5, 295, None]), [("li", p) for p in (None, 150, 296)],
        lambda h, s: _tile_at(10, 290, n=300)(h, s) and h["nleaf"] > 64 and s[10]["leaf"] < 64 < s[290]["leaf"])
    d = _doc(it, 100, {10: (TILE, pg()), 20: (BEGIN, li()), 90: (TILE, pg()), 95: (END, li())})
    for k in range(800):
        d.put(11 + (k * 37) % (70 + k), 2, text=chr(0x3b1 + k % 300), props={"p": k})
    add("x_promote", "800 scattered inserts: the small profile runs out of nodes", d,
        _both([500, 5, 899, None]), [("li", p) for p in (None, 500)],
        lambda h, s: len(s) >= 900 and [i for i, x in enumerate(s) if x["kind"] == ol.SEG_MARKER and x["refType"] & TILE][0] == 10)
    d = _doc(it, 20, {5: (TILE, pg()), 8: (BEGIN, li()), 12: (TILE, pg())})
    d.annotate(5, 6, pg("row"), client=2)
    d.annotate(8, 9, li("q"), client=2)
    add("k_mkmask", "an annotate changed the label keys on a marker: refused", d,
        [("pg", 10, True), ("row", 10, True), ("pg", 3, False)], [("li", None), ("q", 10)],
        lambda h, s: _tile_at(5, 12, n=20)(h, s) and s[5]["props"] != s[12]["props"])
    return out


_CACHE = {}


def _all():
    if not _CACHE:
        it = ol.Interner()
        for v in range(300):  # SubSequence items: the integer v has item id v
            assert it.item(v) == v
        cs = cases_(it)
        names = [c.name for c in cs]
        assert len(set(names)) == len(names)
        _CACHE["cases"], _CACHE["it"] = cs, it
    return _CACHE


def cases() -> List[TCase]:
    return list(_all()["cases"])


def interner() -> ol.Interner:
    return _all()["it"]


def batch(which: Optional[List[TCase]] = None) -> ol.Batch:
    cs = cases() if which is None else which
    return ol.Batch.from_logs([c.log for c in cs])


def queries(cs: Optional[List[TCase]] = None):
    """every query of the cases, in fixture order: (tile queries [(doc, label, pos, preceding)], stack queries
    [(doc, label, pos)]); doc indexes cs"""
    cs = cases() if cs is None else cs
    tq = [(d, lb, p, pre) for d, c in enumerate(cs) for lb, p, pre in c.tiles]
    sq = [(d, lb, p) for d, c in enumerate(cs) for lb, p in c.stacks]
    return tq, sq
