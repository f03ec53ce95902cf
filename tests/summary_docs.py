"""Helpers of tests/test_batched_summaries.py: the host core's summary dump (mth_summary), the record-size formula of
the summary dump, and hand-built documents at the shapes where the lane-parallel summary writer can go wrong.

How the documents are built: every row is appended by a remote client with minSeq 0, so zamboni merges nothing, after
a prefix of PRE markers (leaves of their own, never mergeable). The LAST record carries min_seq = its own seq - 1:
every earlier row settles, zamboni visits at most the two oldest leaves (the markers) for that record, and the
other settled rows stay unmerged: they merge only in the summary. The last record is an insert of "!" at the end (a
window row) unless the shape needs another."""
import ctypes

import numpy as np

from fluidframework_amd import oplog as ol
import core_host

V1, LEGACY = ol.SUMMARY_V1, ol.SUMMARY_LEGACY
PRE = 12
ALPHA = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"
KEYS = [f"k{i}" for i in range(24)]


def host_lib():
    L = core_host.lib()
    L.mth_summary.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64]
    L.mth_summary.restype = ctypes.c_int64
    return L


def host_summary(st, d: int, mode: int) -> bytes:
    """mth_summary: sized, then filled into a window of exactly that size between canaries"""
    L = host_lib()
    n = L.mth_summary(st.h, d, mode, None, 0)
    assert n >= 24
    buf = np.full(n + 16, 0xA5, np.uint8)
    assert L.mth_summary(st.h, d, mode, buf[8:].ctypes.data_as(ctypes.c_void_p), n) == n
    assert (buf[:8] == 0xA5).all() and (buf[n + 8:] == 0xA5).all()
    return buf[8: n + 8].tobytes()


def record_size(seg) -> int:
    """40 + 4 nprops + 8 nderived + 4 for a handle + the text"""
    nd = sum(1 for _, v in seg["props"] if isinstance(v, ol.Derived) and v.kind != "nan")
    text = seg["len"] if seg["kind"] in (ol.SEG_TEXT, ol.SEG_RUN) else 0
    return 40 + 4 * len(seg["props"]) + 8 * nd + (4 if seg["flags"] & ol.DF_HANDLE else 0) + 2 * text


def text(n, k=0, nl=False):
    t = "".join(ALPHA[(k + 7 * i) % len(ALPHA)] for i in range(n))
    return t[:-1] + "\n" if nl else t


class Doc:
    def __init__(self, it, name, kind="text", pre=PRE, local=0):
        self.log = ol.DocLog(it, local_long_id=local)
        self.name, self.kind = name, kind
        self.seq = self.len = self.rows = 0
        self.want = None  # the lengths of the v1 summary's segments after the prefix, where the shape states them
        for _ in range(pre):
            self.marker(0)

    def kw(self, client=None, last=False):
        self.seq += 1
        return dict(client=client or 1 + self.seq % 2, seq=self.seq, ref_seq=self.seq - 1,
                    min_seq=self.seq - 1 if last else 0)

    def ins(self, n, props=None, nl=False, at=None, last=False, item=None):
        """a row of n units at the end (or at `at`): text, items of a SubSequence document, or permutation rows"""
        pos = self.len if at is None else at
        if self.kind == "text":
            body = dict(text=n if isinstance(n, str) else text(n, self.rows, nl))
            n = len(body["text"])
        elif self.kind == "run":
            body = dict(items=[(item if item is not None else 20 + (self.rows + i) % 40) for i in range(n)])
        else:
            body = dict(perm=n)
        self.log.add(ol.OP_INSERT, pos1=pos, props=props, **body, **self.kw(last=last))
        self.len += n
        self.rows += 1
        return pos

    def marker(self, ref_type, props=None):
        self.log.add(ol.OP_INSERT, pos1=self.len, marker=ref_type, props=props, **self.kw())
        self.len += 1
        self.rows += 1

    def annotate(self, a, b, props, combining=ol.COMBINE_NONE):
        self.log.add(ol.OP_ANNOTATE, pos1=a, pos2=b, props=props, combining=combining, **self.kw())

    def remove(self, a, b, last=False):
        self.log.add(ol.OP_REMOVE, pos1=a, pos2=b, **self.kw(last=last))
        self.len -= b - a

    def end(self):
        """the settling record: a window row at the end"""
        if self.kind == "text":
            self.ins("!", last=True)
        else:
            self.ins(1, last=True)
        return self


def docs(kinds=("text", "run", "perm")):
    """every hand-built document, in one interner"""
    it = ol.Interner()
    for k in KEYS:
        it.key(k)
    out = []

    def doc(name, kind="text", **kw):
        out.append(Doc(it, name, kind, **kw))
        return out[-1]

    def rows(name, lens, want=None, kind="text", **kw):
        d = doc(name, kind)
        for n in lens:
            d.ins(n, **kw)
        d.want = want
        return d.end()
    if "text" in kinds:
        doc("empty", pre=0)
        doc("one_row", pre=0).ins("x")  # 66 bytes as a dump and as a summary: the next window starts at 2 mod 4
        for n in (63, 64, 65, 129):  # one run across several passes
            rows(f"ones_{n}", [1] * n, [n])
        rows("len_100x3_300", [100, 100, 100, 300], [300, 300])
        rows("len_200_57_300", [200, 57, 300], [257, 300])
        rows("len_300_10_300", [300, 10, 300], [310, 300])
        rows("len_10_300_300", [10, 300, 300], [310, 300])
        rows("len_256x3", [256, 256, 256], [768])
        rows("len_257x2", [257, 257], [257, 257])
        rows("long_in_two_passes", [300] + [1] * 70 + [300] + [1] * 3, [370, 303])
        rows("odd_even", (1, 2, 3, 3, 4, 1, 1, 6, 5, 2, 7), [35])
        rows("big_texts", (255, 256, 257, 1000), [511, 257, 1000])
        d = doc("props_equal")
        for _ in range(3):
            d.ins(3, props={KEYS[1]: "a", KEYS[4]: 2})
        d.want = [9]
        d.end()
        d = doc("props_one_value_differs")
        d.ins(3, props={KEYS[1]: "a", KEYS[4]: 2})
        d.ins(3, props={KEYS[1]: "a", KEYS[4]: 3})
        d.want = [3, 3]
        d.end()
        d = doc("props_empty_vs_none")
        a = d.ins(3, props={KEYS[2]: 1})
        d.annotate(a, a + 3, {KEYS[2]: None})  # {} after the delete
        d.ins(3)
        d.ins(3)
        d.want = [3, 6]
        d.end()
        d = doc("props_8_descending")
        for _ in range(2):
            a = d.ins(3)
            for k in reversed(KEYS[:8]):
                d.annotate(a, a + 3, {k: k + "v"})
        d.want = [6]
        d.end()
        d = doc("markers_between")
        d.ins(2)
        d.marker(1, props={KEYS[2]: "tile"})
        d.marker(2)
        d.ins(2)
        d.ins(2)
        d.want = [2, 1, 1, 4]
        d.end()
        d = doc("window_insert_between")
        d.ins(4)
        d.ins(4)
        d.ins("WIN", at=PRE + 4, last=True)
        d.want = [4, 3, 4]
        d = doc("removed_above_msn_between")
        d.ins(4)
        d.ins(4)
        d.ins(4)
        d.remove(PRE + 4, PRE + 8, last=True)
        d.want = [4, 4, 4]
        d = doc("removed_below_msn_between")
        d.ins(4)
        d.ins(4)
        d.ins(4)
        d.remove(PRE + 4, PRE + 8)
        d.want = [8]
        d.end()
        d = doc("tombstones_70_between")
        d.ins(4)
        for _ in range(70):
            d.ins(1)
        d.ins(4)
        d.remove(PRE + 4, PRE + 74)
        d.want = [8]
        d.end()
        d = doc("local_insert_between")
        d.ins(4)
        d.ins(4)
        d.log.add(ol.OP_INSERT | ol.OPF_LOCAL, pos1=PRE + 4, text="LOC")
        d.want = [8]
        d.ins("!", at=PRE + 8, last=True)
        d = doc("local_pending_removal")
        d.ins(4)
        d.ins(4)
        d.ins(4)
        d.log.add(ol.OP_REMOVE | ol.OPF_LOCAL, pos1=PRE + 4, pos2=PRE + 8)
        d.want = [8]  # v1 elides the row, legacy merges it: [12]
        d.ins("!", at=PRE + 12, last=True)
    if "run" in kinds:
        rows("run_50x3_150", [50, 50, 50, 150], [150, 150], kind="run")
        rows("run_100_29_150", [100, 29, 150], [129, 150], kind="run")
        rows("run_150_10_150", [150, 10, 150], [160, 150], kind="run")
        rows("run_10_150_150", [10, 150, 150], [160, 150], kind="run")
        rows("run_128x3", [128, 128, 128], [384], kind="run")
        rows("run_129x2", [129, 129], [129, 129], kind="run")
        rows("run_ends_in_item_10", [3, 3, 3], [9], kind="run", item=10)
        rows("run_texts_around_128", [127, 128, 129, 300], [255, 129, 300], kind="run")
    if "perm" in kinds:
        rows("perm_300_300", [300, 300], [600], kind="perm")
    return out


def nl_and_marker_variants(base_rows: int, leaf_of_row):
    """documents of `base_rows` one-unit rows with a newline-ended row as the last row of the first pass and with a
    marker as the first row of the second; `leaf_of_row(i)`: the leaf ordinal of body row i in the plain document"""
    first = next(i for i in range(base_rows) if leaf_of_row(i) >= 8)
    it = ol.Interner()
    a = Doc(it, f"ones_{base_rows}_nl_ends_pass")
    for i in range(base_rows):
        a.ins("\n" if i == first - 1 else "q")
    a.want = [first, base_rows - first]
    a.end()
    b = Doc(it, f"ones_{base_rows}_marker_starts_pass")
    for i in range(base_rows):
        if i == first:
            b.marker(3)
        else:
            b.ins("q")
    b.want = [first, 1, base_rows - first - 1]
    b.end()
    return [a, b]


def neighbours(it):
    """two small text documents whose summaries are 2 mod 4 long, one in each mode (v1: 24 + 44 + 42, legacy: 24 + 42),
    so that the window after them starts at 2 mod 4"""
    a = Doc(it, "neighbour_v1", pre=0)
    a.ins("xy")
    b = Doc(it, "neighbour_legacy", pre=0)
    b.ins("x")
    return [a.end(), b.end()]


def handle_docs():
    """PermutationSegment rows with allocated handles (MT_OP_NOOP | MT_OPF_LOCAL records: getAllocatedHandle splits a
    one-row segment out and allocates its handle; engines with pcap > 0): a row of 4 whose first two rows are allocated
    in order (the handles follow: the two merge) and in reverse order (they do not)"""
    it = ol.Interner()
    out = []
    for name, order, want in (("handles_follow", (0, 1), [2, 2]), ("handles_do_not_follow", (1, 0), [1, 1, 2])):
        d = Doc(it, name, "perm")
        d.ins(4)
        for i in order:
            d.log.add(ol.OP_NOOP | ol.OPF_LOCAL, pos1=PRE + i)
        d.want = want
        out.append(d.end())
    return out + neighbours(it)


def census(hdr, segs):
    """(rows kept, segments emitted, runs that span two leaves, runs of more than 64 rows) of the v1 extraction over
    a parsed canonical dump, by the rule of snapshot.extract_segments"""
    from fluidframework_amd import snapshot as sn
    kept = nsegs = two = big = 0
    prev, leaves, rows = None, set(), 0

    def close():
        nonlocal two, big
        two += len(leaves) >= 2
        big += rows > 64
    for s in segs:
        removed = s["removedSeq"] is not None
        if s["seq"] == -1 or (removed and s["removedSeq"] <= hdr["minSeq"]):
            continue
        kept += 1
        if s["seq"] <= hdr["minSeq"] and not removed:
            if prev is not None and sn._can_append(prev, s) and sn._match_props(prev, s):
                prev = sn._appended(prev, s)
                leaves.add(s["leaf"])
                rows += 1
                continue
            if prev is not None:
                close()
            prev, leaves, rows = s, {s["leaf"]}, 1
            nsegs += 1
        else:
            if prev is not None:
                close()
            prev = None
            nsegs += 1
    if prev is not None:
        close()
    return kept, nsegs, two, big


def batch(ds) -> ol.Batch:
    return ol.Batch.from_logs([d.log for d in ds])
