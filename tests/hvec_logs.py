"""Hand-built logs for the batched PermutationVector reads: handle ranges (HandleCache.getHandles, matrix
handlecache.ts:69-83, behind PermutationVector.getMaybeHandle, permutationvector.ts:157-161) and
PermutationVector.handleToPosition (permutationvector.ts:198-253) -- test infrastructure for tests/test_ref_hvec.py,
tests/test_napi_hvec.py and tools/make_ref_goldens.py --hvec.

Every case is one document of PermutationSegment rows whose replica is client 5. Rows appended by client 1 under a
minSeq held at 0 are one position each, four to a leaf (a leaf of 8 splits 4 + 4), so row r sits at slot (r // 4) * 8 +
r % 4 and a pass of the wave walks (8 leaves x 8 slots) holds 32 rows: rows 31 / 32, 63 / 64, 95 / 96 and 127 / 128 lie
on both sides of a pass boundary (slots 59 / 64, ..., 251 / 256). A leaf at rest holds at most 7 rows, so slots 63 and
255 are never occupied (tests/test_ref_tiles.py). A getAllocatedHandle record (a local NOOP, tests/handles_inject.py)
gives the row at its position the next handle of the document's HandleTable: 1, 2, 3, ... in record order while none
was freed; on a longer row it first splits a one-position row out. Only zamboni makes an allocated row longer than one
position: a step (NOOPs that move the minSeq) appends the rows of one leaf whose handles are consecutive
(PermutationSegment.canAppend, permutationvector.ts:87-93), never across a leaf boundary.

A case names its queries: `ranges` = [(start, end)], `handles` = [(handle, localSeq or None)]; None is the reference's
default argument, the replica's current localSeq. The witnesses read rows and slots from the reference's dump.

Case list
  e_empty: no row at all; the empty range, ranges past the end, handle 0 and handle 1 (which throw)
  u_one_unalloc: one unallocated row of 5: whole, inside, empty ranges at 0 / 2 / 5, the three invalid shapes (start < 0,
      end > length, end < start); handle 0 and a never-allocated handle throw
  l_row70: one allocated row of 70 (rounds of six one-position rows allocated beside the grown row in its leaf, then a
      step), an unallocated row of 9 behind it: the wave strides over one row longer than its 64 lanes
  l_row4100: the same to 4,100 positions: a window larger than a pass of the writer; ranges around 64 and 4,096
  a_alt_63 / 64 / 65 / 127 / 128 / 129 / 140: that many one-position rows, the even ones allocated: the whole, the last
      position, every range that straddles a pass boundary (rows 32, 64, 96, 128) by one position on either side, and the
      handles of the rows next to the boundaries. The last leaf keeps up to 7 rows until it splits, so row 64 of 65 and
      row 128 of 129 still sit in the leaf of the rows before them; a_alt_140 has every boundary row at its slot (the
      witness), and rows behind the last boundary
  i_inside: rows of 3 (unallocated), 1 (allocated), 6 (unallocated): a range that starts and ends inside rows, ranges
      confined to one row, empty ranges at 0, in the middle and at the length
  s_split: an allocated row of 4 (handles 1..4) split by a remote insert at 2: the halves carry start and start + 2
  z_merged: six allocated rows merged by a step into one row of 6 (handles 1..6)
  r_states: twelve allocated rows; rows 4, 5 removed by client 2 and still in the tree, row 8 under a pending local
      remove, a pending local insert of 3 at 2 with its middle position allocated: the local view skips the removed
      rows; handleToPosition finds the handles of removed rows, at every localSeq from 0 to the current one and at one
      past it (which throws)
  p_pending: eight allocated rows and five pending local ops (insert, remove, insert, remove, insert): every handle at
      every localSeq 0..5 and at 6 (which throws)
  f_unlinked: eight allocated rows, row 2 removed by client 1 and unlinked by a step: its handle 3 was freed and throws
  f_realloc: the same, then a row appended and allocated: it takes the freed handle 3, now behind handles 4..8
  x_chunks: 300 one-position rows, every third allocated: more than 64 leaves (two chunks of the tiled profile's rope)
  x_promote: 100 rows and 800 scattered one-position inserts, every 7th position allocated: a small build hands the
      document to a larger one (PROMOTED); the one case well over 300 rows, as the promotion needs
"""
from __future__ import annotations

from typing import Callable, List, NamedTuple, Optional

from fluidframework_amd import oplog as ol
import zamboni_logs as zl
from insert_logs import _I
from range_logs import slots, LOCAL

ALL = zl.ALL
UNALLOC = ol.HANDLE_UNALLOCATED
PROMOTED = ("x_promote",)
PCAP = 1 << 13  # handles per document (mt_caps.pcap): l_row4100 allocates 4,100
ALT = (63, 64, 65, 127, 128, 129, 140)
BOUNDARIES = (32, 64, 96, 128)  # the first row of a pass, four appended rows to a leaf


class HCase(NamedTuple):
    name: str
    branch: str
    log: ol.DocLog
    ranges: list        # [(start, end)]
    handles: list       # [(handle, localSeq | None)]
    witness: Callable   # (hdr, segs) -> bool over the parsed canonical dump of the reference
    profiles: frozenset


def alloc(d, *pos):
    """PermutationVector.getAllocatedHandle(pos) records"""
    for p in pos:
        d.log.add(ol.OP_NOOP | ol.OPF_LOCAL, pos1=p)


def lins(d, pos, n):
    """a pending local insert of one row of n positions"""
    d.log.add(ol.OP_INSERT | ol.OPF_LOCAL, pos1=pos, perm=n)


def _rows(it, n):
    d = _I(it, local=LOCAL)
    for _ in range(n):
        d.ins(d.length, perm=1)
    return d


def _grown(it, total):
    """one allocated row of `total` positions (handles 1..total): six one-position rows at a time are split out of a row
    appended behind the grown one, allocated in order, and appended to it by a step that scours their leaf"""
    d = _I(it, local=LOCAL)
    done = 0
    while done < total:
        k = min(6, total - done)
        d.ins(done, perm=k)
        alloc(d, *range(done, done + k))
        d.step(drain=2)
        done += k
    return d


def _starts(segs):
    return [s["start"] for s in segs]


def _invalid(length):
    return [(-1, 0), (-1, min(length, 2)), (0, length + 1), (length, length + 1), (1, 0), (length, length - 1)]


def cases_(it) -> List[HCase]:
    out: List[HCase] = []

    def add(name, branch, d, ranges, handles, w, profiles=ALL):
        out.append(HCase(name, branch, d.log, ranges, handles, w, profiles))

    d = _I(it, local=LOCAL)
    d.log.add(ol.OP_NOOP, client=1, seq=1, ref_seq=0, min_seq=0)
    add("e_empty", "no row at all", d, [(0, 0), (0, 1), (1, 1), (-1, 0), (1, 0)], [(0, None), (1, None), (1, 0), (1, 1)],
        lambda h, s: not s and h["length"] == 0)

    d = _I(it, local=LOCAL)
    d.ins(0, perm=5)
    add("u_one_unalloc", "one unallocated row", d, [(0, 5), (1, 4), (2, 3), (0, 0), (2, 2), (5, 5)] + _invalid(5),
        [(0, None), (1, None), (UNALLOC, None), (-1, None), (5, 0)],
        lambda h, s: len(s) == 1 and s[0]["len"] == 5 and s[0]["start"] == UNALLOC)

    for total, name in ((70, "l_row70"), (4100, "l_row4100")):
        d = _grown(it, total)
        d.ins(total, perm=9)
        L = total + 9
        rg = [(0, L), (0, total), (1, total - 1), (5, 9), (63, 66), (64, 65), (total - 1, total + 1), (total, L), (L, L),
              (0, 0), (0, 64), (0, 65), (1, 64), (1, 66)]
        if total > 4096:
            rg += [(0, 4096), (0, 4097), (4095, 4098), (3, 4099), (4096, 4096), (64, 4096 + 64), (4097, L)]
        add(name, f"one allocated row of {total} positions", d, rg + _invalid(L),
            [(1, None), (64, None), (65, None), (total, None), (total + 1, None), (0, None)]
            + ([(4096, None), (4097, None)] if total > 4096 else []),
            lambda h, s, total=total: [x["len"] for x in s] == [total, 9] and _starts(s) == [1, UNALLOC])

    for n in ALT:
        d = _rows(it, n)
        alloc(d, *range(0, n, 2))
        rg = [(0, n), (n - 1, n), (0, 1), (n, n)]
        hd = [(1, None), ((n + 1) // 2, None), ((n + 1) // 2 + 1, None)]
        for b in BOUNDARIES:
            if b < n:
                rg += [(b - 1, b + 1), (b - 1, b), (b, b + 1), (b - 2, b), (b, min(b + 2, n)), (0, b), (0, b + 1), (b, n),
                       (b - 1, n), (b, b)]
            for r in (b - 2, b):
                if r < n:
                    hd.append((r // 2 + 1, None))
        add(f"a_alt_{n}", f"{n} one-position rows, the even ones allocated", d, rg, hd,
            lambda h, s, n=n: len(s) == n and all(x["len"] == 1 for x in s)
            and _starts(s) == [r // 2 + 1 if r % 2 == 0 else UNALLOC for r in range(n)]
            and (n != 140 or all(slots(s)[b] == 2 * b and slots(s)[b - 1] == 2 * b - 5 for b in BOUNDARIES)))

    d = _I(it, local=LOCAL)
    d.ins(0, perm=10)
    alloc(d, 3)
    add("i_inside", "ranges that start and end inside rows", d,
        [(1, 7), (2, 5), (1, 2), (0, 3), (3, 4), (4, 10), (5, 8), (0, 10), (0, 0), (3, 3), (4, 4), (10, 10)] + _invalid(10),
        [(1, None), (2, None), (1, 0)],
        lambda h, s: [x["len"] for x in s] == [3, 1, 6] and _starts(s) == [UNALLOC, 1, UNALLOC])

    d = _rows(it, 4)
    alloc(d, 0, 1, 2, 3)
    d.step(drain=2)
    d.put(2, perm=2)
    add("s_split", "split halves carry start + pos", d, [(0, 6), (1, 5), (1, 2), (2, 4), (3, 5), (4, 6)],
        [(1, None), (2, None), (3, None), (4, None), (5, None)],
        lambda h, s: [x["len"] for x in s] == [2, 2, 2] and _starts(s) == [1, UNALLOC, 3])

    d = _rows(it, 6)
    alloc(d, *range(6))
    d.step(drain=2)
    add("z_merged", "zamboni appended consecutive handles", d, [(0, 6), (2, 5), (5, 6), (6, 6)],
        [(h, None) for h in range(0, 8)], lambda h, s: [x["len"] for x in s] == [6] and _starts(s) == [1])

    d = _rows(it, 12)
    alloc(d, *range(12))
    d.remove(4, 6, 2)          # rows 4, 5 by a remote client: still in the tree
    d.lrem(6, 7)               # row 8 (local position 6): localSeq 1
    lins(d, 2, 3)              # localSeq 2
    alloc(d, 3)                # the middle position of the pending insert: handle 13
    add("r_states", "removed rows still in the tree, a pending remove, a pending insert", d,
        [(0, 12), (0, 13)] + [(a, a + 3) for a in range(0, 10)] + [(12, 12), (4, 4)],
        [(h, q) for h in range(1, 15) for q in (None, 0, 1, 2, 3)],
        lambda h, s: len(s) == 15 and h["length"] == 12 and h["localSeq"] == 2
        and [i for i, x in enumerate(s) if x["removedSeq"] is not None] == [7, 8, 11]
        and s[11]["removedSeq"] == -1 and [s[i]["start"] for i in (2, 3, 4)] == [UNALLOC, 13, UNALLOC]
        and all(s[i]["localSeq"] == 2 for i in (2, 3, 4)) and s[7]["start"] == 5 and s[11]["start"] == 9)

    d = _rows(it, 8)
    alloc(d, *range(8))
    lins(d, 1, 2)   # localSeq 1: length 10
    d.lrem(4, 6)    # localSeq 2: rows 2, 3
    lins(d, 0, 1)   # localSeq 3
    d.lrem(8, 9)    # localSeq 4: row 7
    lins(d, 5, 4)   # localSeq 5
    alloc(d, 0)     # the pending insert at 0: handle 9
    add("p_pending", "pending local ops at several localSeq values", d, [(0, 12), (0, 13), (3, 9), (5, 9)],
        [(h, q) for h in range(1, 11) for q in (None, 0, 1, 2, 3, 4, 5, 6)],
        lambda h, s: h["localSeq"] == 5 and h["length"] == 12
        and sorted(x["localSeq"] for x in s if x["flags"] & ol.DF_LSEQ) == [1, 3, 5]
        and sorted(x["localRemovedSeq"] for x in s if x["flags"] & ol.DF_LRSEQ) == [2, 2, 4] and s[0]["start"] == 9)

    for nm in ("unlinked", "realloc"):
        d = _rows(it, 8)
        alloc(d, *range(8))
        d.rem(2, 3)
        d.step(drain=3)
        if nm == "realloc":
            d.ins(7, perm=1)
            alloc(d, 7)
        add(f"f_{nm}", "a freed handle" + (" allocated again to a later row" if nm == "realloc" else ""), d,
            [(0, 7 + (nm == "realloc")), (1, 4), (6, 7)], [(h, None) for h in range(0, 10)],
            lambda h, s, nm=nm: [x for x in _starts(s) if x != UNALLOC and x == 3] == ([3] if nm == "realloc" else [])
            and all(x["removedSeq"] is None for x in s) and sum(x["len"] for x in s) == 7 + (nm == "realloc")
            and (nm != "realloc" or _starts(s)[-1] == 3))

    d = _rows(it, 300)
    alloc(d, *range(0, 300, 3))
    add("x_chunks", "more than 64 leaves", d, [(0, 300), (100, 200), (255, 258), (299, 300), (127, 130)] + _invalid(300),
        [(1, None), (50, None), (86, None), (87, None), (100, None), (101, None)],
        lambda h, s: len(s) == 300 and h["nleaf"] > 64 and _starts(s)[297] == 100)

    d = _rows(it, 100)
    for k in range(800):
        d.put(11 + (k * 37) % (70 + k), perm=1)
    alloc(d, *range(0, 900, 7))
    add("x_promote", "800 scattered inserts: the small profile runs out of nodes", d,
        [(0, 900), (400, 500), (893, 900), (0, 1)] + _invalid(900), [(1, None), (64, None), (129, None), (130, None)],
        lambda h, s: len(s) == 900 and _starts(s)[889] == 128 and _starts(s)[7] == 2)
    return out


_CACHE = {}


def _all():
    if not _CACHE:
        it = ol.Interner()
        cs = cases_(it)
        names = [c.name for c in cs]
        assert len(set(names)) == len(names)
        _CACHE["cases"], _CACHE["it"] = cs, it
    return _CACHE


def cases() -> List[HCase]:
    return list(_all()["cases"])


def interner() -> ol.Interner:
    return _all()["it"]


def batch(which: Optional[List[HCase]] = None) -> ol.Batch:
    cs = cases() if which is None else which
    return ol.Batch.from_logs([c.log for c in cs])


def queries(cs: Optional[List[HCase]] = None):
    """every query of the cases, in fixture order: (range queries [(doc, start, end)], handleToPosition queries
    [(doc, handle, localSeq | None)]); doc indexes cs"""
    cs = cases() if cs is None else cs
    rq = [(d, a, b) for d, c in enumerate(cs) for a, b in c.ranges]
    hq = [(d, h, q) for d, c in enumerate(cs) for h, q in c.handles]
    return rq, hq
