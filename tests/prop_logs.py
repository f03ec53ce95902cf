"""Hand-built logs for the property manager's key-slot and pending-count rules (SegmentPropertiesManager,
segmentPropertiesManager.ts:19-128; Properties.combine / matchProperties, properties.ts:26-92) — test infrastructure
for tests/test_ref_props.py and tools/make_ref_goldens.py --props.

The engine serves every annotate and every insert with properties with lane-parallel code that exists only in the GPU
build (add_props_par: a lane per key slot and a lane per pair of the op, new slots in first-appearance order; the
annotate branch of ack_rows: a lane per member row); the host core, the oracle and the one-lane builds take the serial
twins. The generator's ops carry one or two pairs over six keys, so no other fixture fills the 8 or the 24 key slots,
holds a pending-key count above 1 or two outstanding local rewrites.

Every case is one small document (one to a few rows of six units, the minSeq held at 0 unless stated). Keys k0..k64
are interned first, so key ids ascend with the index. Pending counts and the rewrite count are not in the canonical
dump: a case that builds pending state ends with PROBE ops (remote annotates over the keys involved) and what they
could write is what the dump shows. Each case is built twice over: the records, and a model of every row's property
manager restated from the reference's text (_Row). The witness is a predicate over the REFERENCE's parsed dump (the
rows' property sets and "properties exist" flags are the model's), and, for the cases whose stream is recorded with
--deltas, over the reference's delta words (`dwitness`: every ANNOTATE event's seq and per-segment propertyDeltas key
sets are the model's; None where addProperties was blocked by a pending local rewrite). `cut` is where the two-submit
tests cut the log: between a local op and its ack where the case has one.

Case list
Key slots and width of an op (each also as <name>_mk: a marker row, <name>_it: a {items} document, <name>_pm: a
PermutationSegment document, but for w_insert_props: a PermutationSegment insert carries no properties on the wire;
the keys of an op are in an order that is not key-id order)
  w_nkv1 / w_nkv2 / w_nkv7 / w_nkv8: one remote annotate of that many new keys on a fresh row
  w_nkv9 / w_nkv23 / w_nkv24: the same, 24-slot profiles; an 8-slot build promotes exactly these documents
  w_fill_8 / w_fill_24: the slots fill over several ops ({k5}, then {k7, k0, k3}, ...), then one op touches all of
      them in yet another order
  w_ninth_late: eight keys live, then a ninth
  w_null_unknown: eight live keys, then {k8: null}: the reference's row is unchanged, the engine takes a ninth slot
  w_mixed_new_old: one op of 12 pairs alternating known and new keys, two nulls among them
  w_insert_props_8 / w_insert_props_24: an insert that carries that many properties (the row is placed by the same
      op: add_props' knownFl path), then an annotate of two of them
Pending-key counts (replica 5)
  p_shadow_many: a local annotate of 8 keys, a remote one of 12 that overlaps 5: the 5 keep their local values; after
      the ack a remote annotate writes all 15
  p_count_2 / p_count_3 / p_count_255: that many local annotates of k0 on one row; after each ack a probe of {k0, k1}
      (p_count_255: a probe after the first, the 254th and the last ack): k0 stays shadowed until the last ack
  p_partial_overlap: local {k0, k1, k2} and {k2, k3}, acked in order; after the first ack a probe writes k0, k1 only
  p_null_pending: a local {k0: null} shadows k0 against a remote write
  p_split_before_ack / p_split_after_ack: a row under a local annotate of 6 keys is split by a remote insert before /
      after the ack; both halves carry the counts, the ack reaches both (ngroups 0), probes on each half
  p_ack_many_rows: a local annotate of 5 keys over 70 rows, a shadowed probe, the ack, a probe that writes
  p_two_groups_one_row: local {k0, k1} on rows [0, 2) and {k2, k3} on rows [1, 3), a probe between the acks
  p_notcollab: a replica that never starts collaborating (local long id -1): no counts are kept, the remote op writes
Rewrite
  r_remote_many: a row of 10 keys takes a remote rewrite with 3 truthy values, a 0, a null and a new key
  r_remote_keeps_pending: the same while two of the absent keys have pending local updates: they survive
  r_remote_keeps_pending_8: the same over 7 keys and a new one: the 8-slot builds hold it without promotion
  r_local_blocks: an outstanding local rewrite: a remote annotate and a remote rewrite are dropped whole (their
      propertyDeltas are undefined); after the ack they apply
  r_two_local: two outstanding local rewrites: a remote op is blocked after the first ack, applies after the second
  r_local_then_local_plain: a local rewrite of {k0, k1, k2}, a local plain annotate of {k2, k3, k4}, the first ack, a
      remote annotate of k0..k5 (k2, k3, k4 shadowed), the second ack
  r_rewrite_empty: a remote rewrite with an empty property set: the properties object stays, empty (MT_DF_HAS_PROPS
      with nprops = 0)
  r_fresh_row: a rewrite on a row that never had properties
Combining ops (COMBINE_CASES: replayed with the value kinds declared; the oracle has no combining ops and the
reference replayer cannot word a derived previous value, so neither the oracle nor the delta stream is compared)
  c_incr_pending: an incr over 4 keys, 2 of them with pending local updates: all four are modified
  c_consensus_mixed: a consensus op over 6 keys, 3 present (kept) and 3 absent (three objects of one seq)
  c_incr_chain: incr over a string three times, over a consensus object, over nothing and over NaN
  c_nan_neighbours / c_cons_neighbours: rows A, B with equal properties, one key NaN / the same consensus object on
      both, a marker, rows C, D with an ordinary equal value; the minSeq passes them: A and B stay apart, C and D merge
      (nsegs 4); the SnapshotV1 summary keeps A and B apart too
Zamboni over many keys (24-slot profiles)
  z_24_equal: two rows with 24 equal pairs set in different op orders merge
  z_24_last_differs: two rows that differ only in the key of the 24th slot stay apart
  z_deleted_vs_never: a row whose key was set and deleted by null (properties {}), then two rows that never had
      properties: matchProperties({}, undefined) is false: [A, B + C]
Caps (CAP_NAMES; `cut` is the record that needs the room; outcomes in tests/test_ref_props.py and DESIGN.md §10)
  cap_25_keys: 24 keys in one op, then a 25th
  cap_null_unknown_24: 24 live keys, then {k24: null} (w_null_unknown at 24 / 25)
  cap_65_pairs: one op of 65 pairs over 65 keys (nkv > 64: add_props' serial route on the GPU too)
  cap_pk_256: 256 local annotates of one key on one row (the count is 8 bits); p_count_255 is the largest that replays
"""
from __future__ import annotations

from typing import Callable, List, NamedTuple, Optional

from fluidframework_amd import oplog as ol
import range_logs as rl
import zamboni_logs as zl

LOCAL = 5
ALL = zl.ALL
WIDE_KEYS = zl.WIDE_KEYS
NKEYS = 65
K = [f"k{i}" for i in range(NKEYS)]
REWRITE, INCR, CONSENSUS = ol.COMBINE_REWRITE, ol.COMBINE_INCR, ol.COMBINE_CONSENSUS
NAN = ol.Derived("nan", 0, 0)
KINDS = (("", "text"), ("_mk", "marker"), ("_it", "run"), ("_pm", "perm"))


class Case(NamedTuple):
    name: str
    branch: str
    log: ol.DocLog
    cut: int
    witness: Callable            # (hdr, segs) -> bool over the reference's parsed dump
    profiles: frozenset          # the profiles whose key slots hold the document (the others promote it)
    kind: str                    # "text" | "run" | "perm"
    feature: bool                # needs the client-feature engine (none does: no REGEN / REF records)
    dwitness: Optional[Callable]  # (decoded delta events) -> bool over the reference's stream, or None
    combining: bool              # holds incr / consensus ops


def _truthy(v) -> bool:
    return v is not None and bool(v)


class _Row:
    """One segment's SegmentPropertiesManager (segmentPropertiesManager.ts), restated"""

    def __init__(self, length: int):
        self.len = length
        self.props = None   # segment.properties (None: undefined)
        self.pk = {}        # pendingKeyUpdateCount
        self.prw = 0        # pendingRewriteCount
        self.groups = []    # pending local annotates this row is a member of

    def copy(self, length: int) -> "_Row":
        r = _Row(length)
        r.props = None if self.props is None else dict(self.props)
        r.pk, r.prw, r.groups = dict(self.pk), self.prw, list(self.groups)
        return r

    def add(self, kvs, comb, seq, collab, combine):
        """addProperties (35-111); seq None: UnassignedSequenceNumber. Returns the deltas ({key: previous value}),
        None where an outstanding local rewrite blocks the op"""
        if self.props is None:
            self.props, self.pk, self.prw = {}, {}, 0
        local = seq is None
        if self.prw > 0 and not local and collab:
            return None
        cop = comb if comb >= INCR else 0
        new = dict(kvs)

        def modify(k):
            return local or k not in self.pk or bool(cop)
        deltas = {}
        if comb == REWRITE:
            if collab and local:
                self.prw += 1
            for k in list(self.props):
                if not _truthy(new.get(k)) and modify(k):
                    deltas[k] = self.props.pop(k)
        for k, v in kvs:
            if collab:
                if local:
                    self.pk[k] = self.pk.get(k, 0) + 1
                elif not modify(k):
                    continue
            prev = self.props.get(k)
            deltas[k] = prev
            nv = combine(cop, prev, seq) if cop else v
            if nv is None:
                self.props.pop(k, None)
            else:
                self.props[k] = nv
        return deltas

    def ack(self, kvs, rewrite):
        """ackPendingProperties (19-33)"""
        if rewrite:
            self.prw -= 1
        for k, _ in kvs:
            if k in self.pk:
                self.pk[k] -= 1
                if self.pk[k] == 0:
                    del self.pk[k]


class _P(rl._R):
    """range_logs._R over rows of six units (a marker: one) with a model of every row's property manager"""

    def __init__(self, it, local: int = 0, kind: str = "text"):
        super().__init__(it, local=local)
        self.it = it
        self.kind = kind
        self.collab = local >= 0
        self.rows: List[_Row] = []
        self.events = []   # per annotate that touched a row: (seq or -1, [deltas key names or None per row])
        self.nval = 0
        self.maxpk = 0
        self.maxprw = 0

    def v(self):
        self.nval += 1
        return self.nval

    def vals(self, idx, order=None):
        """{k_i: a fresh value} for the key indices in the given order"""
        return {K[i]: self.v() for i in (order or idx)}

    def pos(self, r: int) -> int:
        return sum(x.len for x in self.rows[:r])

    def _combine(self, cop, prev, seq):
        """Properties.combine as addProperties calls it: newValue undefined (properties.ts:26-59)"""
        if cop == CONSENSUS:
            return prev if prev is not None else ol.Derived("cons", seq, 0)
        if prev is None or prev == NAN or isinstance(prev, (bool, int, float)):
            return NAN
        if isinstance(prev, ol.Derived):
            return ol.Derived("strcat", 0, 1) if prev.kind == "cons" else ol.Derived("strcat", prev.a, prev.b + 1)
        return ol.Derived("strcat", self.it.value(prev), 1)

    def row(self, props=None, client: int = 1) -> int:
        """append a row; returns its index"""
        salt = len(self.rows) + len(self.log.ops)
        L = 1 if self.kind == "marker" else 6
        if self.kind == "marker":
            self.ins(self.length, marker=0, props=props, client=client)
        elif self.kind == "run":
            self.ins(self.length, items=zl._items(L, salt), props=props, client=client)
        elif self.kind == "perm":
            self.ins(self.length, perm=L, props=props, client=client)
        else:
            self.ins(self.length, text=zl._txt(L, salt), props=props, client=client)
        r = _Row(L)
        if props is not None:  # TextSegment.make(text, props): addProperties without seq or window
            r.add(list(props.items()), 0, 0, False, self._combine)
        self.rows.append(r)
        return len(self.rows) - 1

    def marker(self):
        self.ins(self.length, marker=0)
        self.rows.append(_Row(1))

    def _apply(self, a, b, props, comb, seq, group=None):
        kvs = list(props.items())
        per = []
        for r in self.rows[a:b]:
            d = r.add(kvs, comb, seq, self.collab, self._combine)
            per.append(None if d is None else sorted(d))
            if group is not None and self.collab:
                r.groups.append(group)
            self.maxpk = max([self.maxpk] + list(r.pk.values()))
            self.maxprw = max(self.maxprw, r.prw)
        self.events.append((-1 if seq is None else seq, per))

    def ann(self, a, b, props, comb=ol.COMBINE_NONE, client: int = 2) -> int:
        """a remote annotate of rows [a, b)"""
        s = self.annotate(self.pos(a), self.pos(b), props, client=client, combining=comb)
        self._apply(a, b, props, comb, s)
        return s

    def lann(self, a, b, props, comb=ol.COMBINE_NONE):
        """a local annotate of rows [a, b); returns what its ack needs"""
        p = self.local(ol.OP_ANNOTATE, self.pos(a), self.pos(b), props, comb)
        self._apply(a, b, props, comb, None, group=id(p))
        return p

    def acked(self, p) -> int:
        kvs = list(p[3].items())
        for r in self.rows:
            if id(p) in r.groups:
                r.groups.remove(id(p))
                r.ack(kvs, p[4] == REWRITE)
        return self.ack(p)

    def split(self, r: int, off: int = 3, client: int = 3):
        """a remote insert inside row r: left part, the new row, right part (copyTo: properties and counts)"""
        self.insert(self.pos(r) + off, "X", client)
        self.length += 1
        row = self.rows[r]
        right = row.copy(row.len - off)
        row.len = off
        self.rows[r + 1: r + 1] = [_Row(1), right]

    def expected(self):
        return [(None if r.props is None else dict(r.props), len(r.groups)) for r in self.rows]


def props_of(it, seg) -> Optional[dict]:
    """a parsed dump row's property set by key name (None: no properties object)"""
    if not seg["flags"] & ol.DF_HAS_PROPS:
        return None
    return {it.keys[k]: v if isinstance(v, ol.Derived) else it.value_obj(v) for k, v in seg["props"]}


def _rows_witness(it, want, extra=None):
    def w(hdr, segs):
        got = [(props_of(it, s), s["ngroups"]) for s in segs]  # the dump's group count is one byte
        return got == [(p, n & 0xFF) for p, n in want] and (extra is None or bool(extra(hdr, segs)))
    return w


def _delta_witness(it, events):
    """every ANNOTATE event of the stream, in order: its seq, and per segment the key set of its propertyDeltas (None:
    undefined, the op was blocked)"""
    def w(ev):
        got = [(e[1], [None if s[3] is None else sorted(it.keys[k] for k, _ in s[3]) for s in e[2]])
               for e in ev if e[0] == 2]
        return got == [(s, [None if d is None else sorted(d) for d in per]) for s, per in events if per]
    return w


def _slots(log: ol.DocLog) -> int:
    """key slots the engine uses for a document: the distinct keys its records name (a null included)"""
    return len({k for k, _ in log.kv})


def _case(d: _P, name, branch, witness=None, combining=False, kind=None, extra=None) -> Case:
    it = d.it
    w = witness or _rows_witness(it, d.expected(), extra)
    prof = ALL if _slots(d.log) <= 8 else WIDE_KEYS
    cut = d.cut if d.cut is not None else len(d.log.ops) - 1
    kind = kind or {"marker": "text"}.get(d.kind, d.kind)
    return Case(name, branch, d.log, cut, w, prof, kind, False, None if combining else _delta_witness(it, d.events),
                combining)


def _scr(n: int, mul: int = 5, add: int = 3) -> List[int]:
    """0..n-1 in an order that is not ascending (n > 2)"""
    if n <= 2:
        return list(range(n))[::-1]
    while any(n % p == 0 and mul % p == 0 for p in (2, 3, 5, 7, 11, 23)):
        mul += 1
    return [(i * mul + add) % n for i in range(n)]


# ---- key slots and width ---------------------------------------------------------------------------------------------
def _w_nkv(n):
    def b(d):
        r = d.row()
        d.mark()
        d.ann(r, r + 1, d.vals(None, _scr(n)))
    return b


def _w_fill(n):
    def b(d):
        r = d.row()
        order = [5, 7, 0, 3] + [i for i in _scr(n, 7, 1) if i not in (5, 7, 0, 3)]
        d.ann(r, r + 1, d.vals(None, order[:1]))
        d.ann(r, r + 1, d.vals(None, order[1:4]))
        for at in range(4, n, 4 if n > 8 else 2):
            d.ann(r, r + 1, d.vals(None, order[at: at + (4 if n > 8 else 2)]))
        d.mark()
        d.ann(r, r + 1, d.vals(None, _scr(n, 11, 2)))
    return b


def _w_ninth_late(d):
    r = d.row()
    d.ann(r, r + 1, d.vals(None, _scr(8)))
    d.mark()
    d.ann(r, r + 1, {K[8]: d.v()})


def _w_null_unknown(d):
    r = d.row()
    d.ann(r, r + 1, d.vals(None, _scr(8, 3, 1)))
    d.mark()
    d.ann(r, r + 1, {K[8]: None})


def _w_mixed(d):
    r = d.row()
    d.ann(r, r + 1, d.vals(None, [10, 4, 0, 8, 2, 6]))
    d.mark()
    p = d.vals(None, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11])
    p[K[4]] = None   # a known key deleted
    p[K[7]] = None   # a null on a key the document has not seen
    d.ann(r, r + 1, p)


def _w_insert_props(n):
    def b(d):
        p = d.vals(None, _scr(n, 7, 2))
        p[K[1]] = None  # addProperties drops a null of the insert's own set
        r = d.row(props=p)
        d.mark()
        d.ann(r, r + 1, {K[n - 1]: d.v(), K[0]: d.v()})
    return b


WIDTH = [("w_nkv1", "one pair, a new key", _w_nkv(1)), ("w_nkv2", "two new keys", _w_nkv(2)),
         ("w_nkv7", "seven new keys", _w_nkv(7)), ("w_nkv8", "eight new keys: the 8 slots fill in one op", _w_nkv(8)),
         ("w_nkv9", "nine new keys in one op", _w_nkv(9)), ("w_nkv23", "23 new keys in one op", _w_nkv(23)),
         ("w_nkv24", "24 new keys: the 24 slots fill in one op", _w_nkv(24)),
         ("w_fill_8", "the 8 slots fill over several ops, not in key-id order", _w_fill(8)),
         ("w_fill_24", "the 24 slots fill over several ops, not in key-id order", _w_fill(24)),
         ("w_ninth_late", "eight keys live, then a ninth", _w_ninth_late),
         ("w_null_unknown", "a null on a key the document has not seen takes a slot", _w_null_unknown),
         ("w_mixed_new_old", "12 pairs alternating known and new keys, two nulls", _w_mixed),
         ("w_insert_props_8", "an insert with 8 properties", _w_insert_props(8)),
         ("w_insert_props_24", "an insert with 24 properties", _w_insert_props(24))]


def width_cases(it) -> List[Case]:
    out = []
    for name, branch, build in WIDTH:
        for suffix, kind in KINDS:
            if kind == "perm" and name.startswith("w_insert_props"):
                continue  # a PermutationSegment's wire form ([length, start]) carries no properties
            d = _P(it, kind=kind)
            build(d)
            out.append(_case(d, name + suffix, branch + {"": "", "_mk": " (a marker row)", "_it": " ({items})",
                                                         "_pm": " (PermutationSegment)"}[suffix]))
    return out


# ---- pending-key counts ----------------------------------------------------------------------------------------------
def pending_cases(it) -> List[Case]:
    out = []
    d = _P(it, LOCAL)
    r = d.row()
    p = d.lann(r, r + 1, d.vals(None, _scr(8)))
    d.mark()
    d.ann(r, r + 1, d.vals(None, [14, 3, 9, 4, 12, 5, 10, 6, 13, 7, 11, 8]))
    assert len(d.rows[0].pk) == 8
    d.acked(p)
    d.ann(r, r + 1, d.vals(None, _scr(15, 4, 1)))
    out.append(_case(d, "p_shadow_many", "a remote op of 12 keys over 5 pending ones"))

    for n in (2, 3, 255):
        d = _P(it, LOCAL)
        r = d.row()
        ps = [d.lann(r, r + 1, {K[0]: d.v()}) for _ in range(n)]
        local = d.rows[0].props[K[0]]
        d.mark()
        for i, p in enumerate(ps):
            d.acked(p)
            if n < 10 or i in (0, n - 2, n - 1):
                d.ann(r, r + 1, {K[0]: d.v(), K[1]: d.v()})
                assert (d.rows[0].props[K[0]] == local) == (i < n - 1)  # shadowed until the last ack
        out.append(_case(d, f"p_count_{n}", f"a pending count of {n} on one key"))

    d = _P(it, LOCAL)
    r = d.row()
    p1 = d.lann(r, r + 1, d.vals(None, [1, 0, 2]))
    p2 = d.lann(r, r + 1, d.vals(None, [3, 2]))
    keep = dict(d.rows[0].props)
    d.mark()
    d.acked(p1)
    d.ann(r, r + 1, d.vals(None, [3, 1, 2, 0]))
    assert all(d.rows[0].props[K[i]] == keep[K[i]] for i in (2, 3)) and d.rows[0].props[K[0]] != keep[K[0]]
    d.acked(p2)
    out.append(_case(d, "p_partial_overlap", "two pending ops that share one key"))

    d = _P(it, LOCAL)
    r = d.row(props={K[0]: 1, K[1]: 2})
    p = d.lann(r, r + 1, {K[0]: None})
    d.ann(r, r + 1, {K[0]: d.v(), K[1]: d.v()})
    assert K[0] not in d.rows[0].props
    d.mark()
    d.acked(p)
    out.append(_case(d, "p_null_pending", "a pending local null shadows the key"))

    for when in ("before", "after"):
        d = _P(it, LOCAL)
        d.row()
        r = d.row()
        d.row()
        p = d.lann(r, r + 1, d.vals(None, _scr(6)))
        if when == "before":
            d.split(r)
            assert len(d.rows) == 5 and d.rows[1].pk == d.rows[3].pk and len(d.rows[3].pk) == 6
            d.ann(1, 2, d.vals(None, [0, 1]))  # shadowed on the left half
        d.mark()
        d.acked(p)
        if when == "after":
            d.split(r)
        assert not d.rows[1].pk and not d.rows[3].pk and not d.rows[3].groups
        d.ann(1, 2, d.vals(None, [1, 0]))
        d.ann(3, 4, d.vals(None, [3, 2]))
        out.append(_case(d, f"p_split_{when}_ack", f"a row split {when} its pending annotate's ack"))

    d = _P(it, LOCAL)
    for _ in range(70):
        d.row()
    p = d.lann(0, 70, d.vals(None, [4, 0, 3, 1, 2]))
    d.ann(0, 70, d.vals(None, [2, 4]))  # shadowed on every row
    d.mark()
    d.acked(p)
    d.ann(0, 70, d.vals(None, [3, 0, 4, 1, 2]))
    out.append(_case(d, "p_ack_many_rows", "the ack of a local annotate of 5 keys over 70 rows"))

    d = _P(it, LOCAL)
    for _ in range(3):
        d.row()
    p1 = d.lann(0, 2, d.vals(None, [1, 0]))
    p2 = d.lann(1, 3, d.vals(None, [3, 2]))
    d.mark()
    d.acked(p1)
    d.ann(0, 3, d.vals(None, [2, 0, 3, 1]))
    d.acked(p2)
    out.append(_case(d, "p_two_groups_one_row", "two pending groups with disjoint keys on a shared row"))

    d = _P(it, -1)
    r = d.row()
    d.lann(r, r + 1, d.vals(None, _scr(8)))
    d.mark()
    d.ann(r, r + 1, d.vals(None, [14, 3, 9, 4, 12, 5, 10, 6, 13, 7, 11, 8]))
    assert not d.rows[0].pk
    out.append(_case(d, "p_notcollab", "not collaborating: no counts are kept"))
    return out


# ---- rewrite ---------------------------------------------------------------------------------------------------------
def rewrite_cases(it) -> List[Case]:
    out = []
    for name, pend, n in (("r_remote_many", False, 10), ("r_remote_keeps_pending", True, 10),
                          ("r_remote_keeps_pending_8", True, 7)):
        d = _P(it, LOCAL)
        r = d.row()
        d.ann(r, r + 1, d.vals(None, _scr(n, 3, 2)))
        p = d.lann(r, r + 1, d.vals(None, [n - 1, n - 2])) if pend else None
        d.mark()
        d.ann(r, r + 1, {K[2]: d.v(), K[n]: d.v(), K[3]: 0, K[0]: d.v(), K[4]: None, K[1]: d.v()}, REWRITE)
        assert sorted(d.rows[0].props) == sorted([K[i] for i in ((0, 1, n, 2, 3) + ((n - 2, n - 1) if pend else ()))])
        if pend:
            d.acked(p)
        out.append(_case(d, name, f"a remote rewrite over {n} keys" + (", two of them pending" if pend else "")))

    d = _P(it, LOCAL)
    r = d.row(props=d.vals(None, [4, 5]))
    p = d.lann(r, r + 1, d.vals(None, [1, 0]), REWRITE)
    d.ann(r, r + 1, d.vals(None, [2]))
    d.ann(r, r + 1, d.vals(None, [3]), REWRITE)
    assert sorted(d.rows[0].props) == [K[0], K[1]] and d.events[-1][1] == [None]
    d.mark()
    d.acked(p)
    d.ann(r, r + 1, d.vals(None, [2]))
    d.ann(r, r + 1, d.vals(None, [3]), REWRITE)
    out.append(_case(d, "r_local_blocks", "an outstanding local rewrite blocks remote ops whole"))

    d = _P(it, LOCAL)
    r = d.row()
    p1 = d.lann(r, r + 1, d.vals(None, [0]), REWRITE)
    p2 = d.lann(r, r + 1, d.vals(None, [1]), REWRITE)
    assert d.maxprw == 2
    d.mark()
    d.acked(p1)
    d.ann(r, r + 1, d.vals(None, [2]))
    d.acked(p2)
    d.ann(r, r + 1, d.vals(None, [3]))
    assert sorted(d.rows[0].props) == [K[1], K[3]]
    out.append(_case(d, "r_two_local", "two outstanding local rewrites"))

    d = _P(it, LOCAL)
    r = d.row(props=d.vals(None, [5, 0]))
    p1 = d.lann(r, r + 1, d.vals(None, [2, 0, 1]), REWRITE)
    p2 = d.lann(r, r + 1, d.vals(None, [4, 2, 3]))
    d.mark()
    d.acked(p1)
    d.ann(r, r + 1, d.vals(None, [5, 4, 3, 2, 1, 0]))
    d.acked(p2)
    out.append(_case(d, "r_local_then_local_plain",
                     "a local rewrite, a local plain annotate, a remote op between the acks"))

    d = _P(it)
    r = d.row()
    d.ann(r, r + 1, d.vals(None, [2, 0, 1]))
    d.mark()
    d.ann(r, r + 1, {}, REWRITE)
    assert d.rows[0].props == {}
    out.append(_case(d, "r_rewrite_empty", "a remote rewrite with an empty property set",
                     extra=lambda h, s: s[0]["flags"] & ol.DF_HAS_PROPS and s[0]["props"] == []))

    d = _P(it)
    r = d.row()
    d.mark()
    d.ann(r, r + 1, d.vals(None, [1, 0]), REWRITE)
    out.append(_case(d, "r_fresh_row", "a rewrite on a row that never had properties"))
    return out


# ---- combining ops ---------------------------------------------------------------------------------------------------
def combine_cases(it) -> List[Case]:
    out = []
    d = _P(it, LOCAL)
    r = d.row(props={K[0]: 1, K[1]: 2, K[2]: "s", K[3]: 3})
    p = d.lann(r, r + 1, {K[1]: 20, K[0]: 10})
    d.mark()
    d.ann(r, r + 1, {K[3]: 1, K[1]: 1, K[2]: 1, K[0]: 1}, INCR)
    assert d.rows[0].props == {K[0]: NAN, K[1]: NAN, K[2]: ol.Derived("strcat", it.value("s"), 1), K[3]: NAN}
    d.acked(p)
    out.append(_case(d, "c_incr_pending", "an incr modifies keys with pending local updates", combining=True))

    d = _P(it)
    r = d.row()
    d.ann(r, r + 1, {K[4]: 7, K[0]: "x", K[2]: True})
    d.mark()
    s = d.ann(r, r + 1, {K[5]: 1, K[4]: 1, K[3]: 1, K[2]: 1, K[1]: 1, K[0]: 1}, CONSENSUS)
    cons = ol.Derived("cons", s, 0)
    assert d.rows[0].props == {K[4]: 7, K[0]: "x", K[2]: True, K[5]: cons, K[3]: cons, K[1]: cons}
    out.append(_case(d, "c_consensus_mixed", "a consensus op over present and absent keys", combining=True))

    d = _P(it)
    r = d.row(props={K[0]: "a"})
    for _ in range(3):
        d.ann(r, r + 1, {K[0]: 1}, INCR)
    d.ann(r, r + 1, {K[1]: 1}, CONSENSUS)
    d.mark()
    d.ann(r, r + 1, {K[1]: 1}, INCR)
    d.ann(r, r + 1, {K[2]: 1}, INCR)
    d.ann(r, r + 1, {K[2]: 1}, INCR)
    assert d.rows[0].props == {K[0]: ol.Derived("strcat", it.value("a"), 3), K[1]: ol.Derived("strcat", 0, 1),
                               K[2]: NAN}
    out.append(_case(d, "c_incr_chain", "incr over a string, a consensus object, nothing and NaN", combining=True))

    for name, comb in (("c_nan_neighbours", INCR), ("c_cons_neighbours", CONSENSUS)):
        d = _P(it)
        base = {K[1]: 5} if comb == INCR else None
        a = d.row(props=base)
        d.row(props=base)
        d.marker()
        d.row(props={K[2]: 6})
        d.row(props={K[2]: 6})
        s = d.ann(a, a + 2, {K[0]: 1}, comb)
        val = NAN if comb == INCR else ol.Derived("cons", s, 0)
        pa = dict(base or {}, **{K[0]: val})

        def w(hdr, segs, pa=pa):
            return (hdr["nsegs"] == 4 and hdr["minSeq"] >= s and [x["len"] for x in segs] == [6, 6, 1, 12] and
                    [props_of(it, x) for x in segs] == [pa, pa, None, {K[2]: 6}])
        d.step(drain=4)
        out.append(_case(d, name, "matchProperties never matches " + ("NaN" if comb == INCR else "a consensus object"),
                         witness=w, combining=True))
    return out


COMBINE_CASES = ("c_incr_pending", "c_consensus_mixed", "c_incr_chain", "c_nan_neighbours", "c_cons_neighbours")


# ---- zamboni over many keys ------------------------------------------------------------------------------------------
def zamboni_cases(it) -> List[Case]:
    out = []
    for name, differs in (("z_24_equal", False), ("z_24_last_differs", True)):
        d = _P(it)
        a = d.row()
        b = d.row()
        vals = {K[i]: 100 + i for i in range(24)}
        o1 = _scr(24, 7, 5)
        d.ann(a, a + 1, {K[i]: vals[K[i]] for i in o1[:10]})
        d.ann(a, a + 1, {K[i]: vals[K[i]] for i in o1[10:]})
        last = K[o1[-1]]  # the key of the 24th slot
        vb = dict(vals, **({last: 999} if differs else {}))
        o2 = _scr(24, 11, 1)
        d.ann(b, b + 1, {K[i]: vb[K[i]] for i in o2[:5]})
        d.ann(b, b + 1, {K[i]: vb[K[i]] for i in o2[5:]})
        d.step(drain=4)

        def w(hdr, segs, differs=differs, vals=vals, vb=vb):
            want = [vals, vb] if differs else [vals]
            return [props_of(it, x) for x in segs] == want and [x["len"] for x in segs] == ([6, 6] if differs else [12])
        out.append(_case(d, name, "matchProperties over 24 key slots", witness=w))

    d = _P(it)
    a = d.row()
    d.row()
    d.row()
    d.ann(a, a + 1, {K[0]: 1})
    d.ann(a, a + 1, {K[0]: None})
    d.step(drain=4)
    out.append(_case(d, "z_deleted_vs_never", "matchProperties({}, undefined) is false",
                     witness=lambda h, s: [(props_of(it, x), x["len"]) for x in s] == [({}, 6), (None, 12)]))
    return out


# ---- caps ------------------------------------------------------------------------------------------------------------
CAP_NAMES = ("cap_25_keys", "cap_null_unknown_24", "cap_65_pairs", "cap_pk_256")


def cap_cases(it) -> List[Case]:
    out = []
    for name, last in (("cap_25_keys", 7), ("cap_null_unknown_24", None)):
        d = _P(it)
        r = d.row()
        d.ann(r, r + 1, d.vals(None, _scr(24, 5, 2)))
        d.mark()
        d.ann(r, r + 1, {K[24]: last})
        out.append(_case(d, name, "a 25th distinct key" + ("" if last else ", a null")))
    d = _P(it)
    r = d.row()
    d.mark()
    d.ann(r, r + 1, d.vals(None, _scr(65, 7, 3)))
    out.append(_case(d, "cap_65_pairs", "one op of 65 pairs: the serial route, the 25th key latches"))
    d = _P(it, LOCAL)
    r = d.row()
    for _ in range(255):
        d.lann(r, r + 1, {K[0]: d.v()})
    d.mark()
    d.lann(r, r + 1, {K[0]: d.v()})
    out.append(_case(d, "cap_pk_256", "the 256th pending update of one key"))
    return out


_CACHE = {}


def _all():
    if not _CACHE:
        it = ol.Interner()
        for v in range(300):  # SubSequence items: the integer v has item id v
            assert it.item(v) == v
        for i, k in enumerate(K):  # key ids ascend with the index
            assert it.key(k) == i + 1
        cs = width_cases(it) + pending_cases(it) + rewrite_cases(it) + combine_cases(it) + zamboni_cases(it)
        caps = cap_cases(it)
        names = [c.name for c in cs + caps]
        assert len(set(names)) == len(names)
        assert tuple(c.name for c in caps) == CAP_NAMES
        assert tuple(c.name for c in cs if c.combining) == COMBINE_CASES
        _CACHE["cases"], _CACHE["caps"] = cs, caps
    return _CACHE


def cases() -> List[Case]:
    """the cases every build must replay to the reference's dump"""
    return list(_all()["cases"])


def caps() -> List[Case]:
    """the cap cases: `cut` is the index of the record that needs the room"""
    return list(_all()["caps"])


def batch(which: Optional[List[Case]] = None) -> ol.Batch:
    cs = cases() if which is None else which
    return ol.Batch.from_logs([c.log for c in cs])


split_at_cut = rl.split_at_cut


def census(b: ol.Batch) -> dict:
    """Over a batch's logs (collaborating replicas' local ops are acked by their own long id): ops by pair count,
    documents by key slots used, the highest pending count of a key and the highest outstanding rewrite count"""
    tot = dict(p1=0, p2=0, p3_8=0, p9_24=0, p25=0, k_le8=0, k_8=0, k_9_23=0, k_24=0, k_over=0, maxpk=0, maxprw=0,
               maxkeys=0, maxpairs=0)
    for d in range(b.ndocs):
        ops, _, props, kv = b.doc(d)
        local = int(b.local_long_id[d])
        c = census_log(ops, props, kv, local)
        for k in ("p1", "p2", "p3_8", "p9_24", "p25"):
            tot[k] += c[k]
        n = len(c["keys"])
        tot["k_le8"] += n <= 8
        tot["k_8"] += n == 8
        tot["k_9_23"] += 9 <= n <= 23
        tot["k_24"] += n == 24
        tot["k_over"] += n > 24
        tot["maxkeys"] = max(tot["maxkeys"], n)
        tot["maxpk"] = max(tot["maxpk"], c["maxpk"])
        tot["maxprw"] = max(tot["maxprw"], c["maxprw"])
    # the upper bound of the widest bucket an op fell in
    widths = (("p1", 1), ("p2", 2), ("p3_8", 8), ("p9_24", 24), ("p25", 25))
    tot["maxpairs"] = max(b for k, b in widths if tot[k] or b == 1)
    return tot


def census_log(ops, props, kv, local: int) -> dict:
    """One document's records: its annotates and inserts with properties by pair count, the distinct keys they name
    (the key slots the engine uses), per key the most local annotates naming it that were outstanding at once (the
    pending count of a row they all cover) and the most outstanding local rewrites. `local`: the replica's long id: a
    sequenced annotate of that client acks the oldest pending one; a replica that does not collaborate keeps none"""
    out = dict(p1=0, p2=0, p3_8=0, p9_24=0, p25=0, keys=set(), maxpk=0, maxprw=0)
    pend = []
    for o in ops:
        kind = int(o["kind"])
        if kind & 7 not in (ol.OP_ANNOTATE, ol.OP_INSERT) or kind & 7 == ol.OP_INSERT and not o["props"]:
            continue
        if kind & 7 == ol.OP_ANNOTATE and not kind & ol.OPF_LOCAL and local > 0 and int(o["client"]) == local:
            if pend:
                pend.pop(0)
            continue
        ks, rw = [], False
        if o["props"]:
            pr = props[int(o["props"]) - 1]
            ks = [int(k) for k in kv[int(pr["kv_off"]): int(pr["kv_off"]) + int(pr["nkv"])]["key"]]
            rw = int(pr["combining"]) == REWRITE
        n = len(ks)
        if n:
            out["p1" if n == 1 else "p2" if n == 2 else "p3_8" if n <= 8 else "p9_24" if n <= 24 else "p25"] += 1
        out["keys"] |= set(ks)
        if kind & 7 == ol.OP_ANNOTATE and kind & ol.OPF_LOCAL and local >= 0:
            pend.append((ks, rw))
            for k in ks:
                out["maxpk"] = max(out["maxpk"], sum(k in p[0] for p in pend))
            out["maxprw"] = max(out["maxprw"], sum(p[1] for p in pend))
    return out
