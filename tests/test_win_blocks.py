"""The block boundaries of the tiled profile's window pass (mt_core.h win_pass / win_block / win_helper).

win_pass evaluates the window set W::N entries at a time (64 on the GPU, 1 on the host). In the tiled replay kernel a
set of more than 64 entries has its second block evaluated by the helper wave (two workgroup barriers per hand-off)
and everything past 128 entries by the replaying wave again; the tiled read kernels and the host core run every block
themselves. Nothing else in the suite names those boundaries.

Eight one-document logs, N in SIZES, built like tests/range_logs.py (replica 5 observes; the minSeq is held at 0, so
every row stays a window entry and zamboni never merges):
  - N rows of 1 + r % 3 units, inserted one per op at position 0 by clients 1 and 2 in turn;
  - one remove by client 3 over the middle half of what it sees under a refSeq that lags by 5 ops (by N - 1 where
    the log is shorter: N = 1 cannot lag);
  - one local insert of the replica inside the text, left unacked. `cut` is its index: the two-submit test cuts there.
The remove's window pass sees N entries: one trip for N <= 64 (no hand-off), the helper's block only for 65..128, a
third trip above 128; the local insert's pass sees N + the remove's splits, the reads N + 1 + every split. The witness
of each case checks those counts in the oracle's dump. Expected digests, lengths and texts are the oracle's
(tests/oracle_client.py, pinned to the reference); the remote perspective read is client 3 at its remove's refSeq,
which the engine answers (persp_logs.answered, mt_kernels.h persp_refused): it does not see the last rows inserted
nor the local insert, and sees its own remove."""
import ctypes
import functools

import numpy as np
import pytest

from fluidframework_amd import oplog as ol
import core_host
import oracle_client as oc
import persp_logs as pl
import zamboni_logs as zl
from range_logs import _R
from test_ref_zamboni import caps_tuple, profile_caps

LOCAL = 5
REMOVER = 3
LAG = 5
BLOCK = 64  # entries of one wave pass of the window set
SIZES = (1, 63, 64, 65, 127, 128, 129, 300)
M64 = (1 << 64) - 1


def trips(n: int) -> int:
    return (n + BLOCK - 1) // BLOCK


class WinCase:
    def __init__(self, it, n):
        self.n = n
        d = _R(it, local=LOCAL)
        lens = []
        for r in range(n):  # prepended: the document is row n-1 .. row 0
            t = zl._txt(1 + r % 3, r)
            d.insert(0, t, 1 + r % 2)
            lens.append(len(t))
        self.ref = d.seq - min(LAG, n - 1)
        seen = lens[: self.ref][::-1]  # client 3's view at ref: the rows up to it, in document order
        L = sum(seen)
        a, b = L // 4, max(L // 4 + 1, 3 * L // 4)
        edges = set(np.cumsum([0] + seen).tolist())
        self.rem_splits = (a not in edges) + (b not in edges)
        self.rem_len = b - a
        self.rem_seq = d.remove(a, b, REMOVER, ref_seq=self.ref)
        d.mark()
        # the replica's view: every row, without the removed units; the insert lands inside the first row of 2+ units
        hidden = sum(lens[self.ref:])  # rows client 3 did not see sit in front of its view
        rows, at = [], 0
        for ln in seen:  # what is left of each seen row, in document order
            lo, hi = max(at, a), min(at + ln, b)
            cutlen = max(0, hi - lo)
            rows.append(ln - cutlen if cutlen == 0 or cutlen == ln else None)  # None: a split row (two parts)
            at += ln
        front = lens[self.ref:][::-1]
        pos, self.loc_splits = 0, 0
        for ln in front + [x for x in rows if x]:
            if ln >= 2:
                pos += 1
                self.loc_splits = 1
                break
            pos += ln
        d.local_ins(pos, "LOC")
        self.log, self.cut = d.log, d.cut
        self.length_local = sum(lens) - (b - a) + 3
        self.length_remote = L - (b - a)
        assert hidden + L == sum(lens)

    @property
    def nrows(self) -> int:
        return self.n + 1 + self.rem_splits + self.loc_splits

    def witness(self, hdr, segs) -> bool:
        """the oracle's dump shows the rows this log was built to make: N + 1 + splits, the remove on the middle of
        them, one pending local row; and the window-set sizes fall in the block class N names"""
        removed = [s for s in segs if s["removedSeq"] == self.rem_seq]
        want = 1 if self.n <= BLOCK else 2 if self.n <= 2 * BLOCK else 3
        return (hdr["nsegs"] == len(segs) == self.nrows and hdr["minSeq"] == 0 and len(removed) >= 1
                and sum(s["len"] for s in removed) == self.rem_len and min(trips(self.n), 3) == want
                and sum(1 for s in segs if s["text"] == "LOC") == 1 and hdr["length"] == self.length_local)


@functools.lru_cache(maxsize=None)
def cases():
    it = ol.Interner()
    return [WinCase(it, n) for n in SIZES]


def batch(cs=None) -> ol.Batch:
    return ol.Batch.from_logs([c.log for c in (cases() if cs is None else cs)])


def split_at_cut(cs):
    b = batch(cs)
    head, tail = [], []
    for d, c in enumerate(cs):
        ops, text, props, kv = b.doc_arrays(d)
        head.append((ops[: c.cut], text, props, kv))
        tail.append((ops[c.cut:], text, props, kv))
    return ol.Batch.from_arrays(head, b.local_long_id), ol.Batch.from_arrays(tail, b.local_long_id)


@functools.lru_cache(maxsize=None)
def expected():
    """per case, from the oracle, once (shared, never changed): digest, dump, and (length, text) at the local
    perspective and at client 3's"""
    b = batch()
    out = []
    for d, c in enumerate(cases()):
        o = oc.OracleClient(c.log.interner)
        o.start_collab(LOCAL)
        assert o.replay_arrays(*b.doc(d)) == 0, f"the oracle refuses the log of N = {c.n}"
        out.append(dict(digest=o.digest() & M64, dump=o.dump(), local=(o.get_length(), o.get_text()),
                        remote=(o.get_length_at(c.ref, REMOVER), o.get_text_at(c.ref, REMOVER))))
    return out


def test_sizes_are_the_block_boundaries():
    assert [c.n for c in cases()] == [1, 63, 64, 65, 127, 128, 129, 300]
    assert [min(trips(c.n), 3) for c in cases()] == [1, 1, 1, 2, 2, 2, 3, 3]


@pytest.mark.parametrize("k", range(len(SIZES)), ids=[f"n{n}" for n in SIZES])
def test_oracle_accepts_the_log_and_the_witness_holds(k):
    c, e = cases()[k], expected()[k]
    hdr, segs = ol.parse_dump(e["dump"])
    print(c.n, "rows", hdr["nsegs"], "remove splits", c.rem_splits, "insert splits", c.loc_splits, "ref", c.ref)
    assert c.witness(hdr, segs), (c.n, hdr)
    # the oracle's own answers agree with what the builder computed from the log
    assert e["local"][0] == c.length_local == len(e["local"][1])
    assert e["remote"][0] == c.length_remote == len(e["remote"][1])
    assert "LOC" in e["local"][1] and "LOC" not in e["remote"][1]
    # the remote perspective is one the engine answers
    assert pl.answered(batch().doc(k)[0], LOCAL, c.ref, REMOVER)
    assert c.n < 2 or c.ref < c.rem_seq - 1, "the remove lags"


@pytest.mark.parametrize("dcap", [0, 1 << 14], ids=["plain", "deltas"])
def test_host_core_tiled(dcap):
    """the host core under HotHuge (W::N = 1: win_block and the tail, entry by entry), with and without the delta
    stream"""
    cs, ex = cases(), expected()
    dig, err, st = core_host.replay_batch(batch(), caps_tuple(profile_caps("tiled")), dcap=dcap)
    assert (err == 0).all(), [(cs[i].n, st.error_op(int(i))) for i in np.nonzero(err)[0]]
    st.L.mth_length.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
    for k, (c, e) in enumerate(zip(cs, ex)):
        assert int(dig[k]) & M64 == e["digest"] and st.dump(k) == e["dump"], c.n
        assert (st.length_local(k), st.text(k)) == e["local"], c.n
        assert (st.L.mth_length(st.h, k, c.ref, REMOVER), st.text(k, c.ref, REMOVER)) == e["remote"], c.n


# ---- GPU -----------------------------------------------------------------------------------------------------------
GPU_BUILDS = [("tiled-narrow", dict(wide=False), {}), ("tiled-wide", dict(wide=True), {}),
              ("tiled-deltas", {}, dict(dcap=1 << 14))]


def _check_gpu(eng, what):
    cs, ex = cases(), expected()
    err, err_op = eng.errors()
    assert (err == 0).all(), (what, [(cs[i].n, int(err[i]), int(err_op[i])) for i in np.nonzero(err)[0]])
    assert len(eng.promoted()) == 0, what
    dig = eng.digests()
    assert [int(x) & M64 for x in dig] == [e["digest"] for e in ex], what
    for k, e in enumerate(ex):
        assert eng.dump(k) == e["dump"], (what, cs[k].n)
    n, st = eng.get_lengths()
    texts, st2 = eng.get_texts()
    assert (st == 0).all() and (st2 == 0).all(), what
    assert [(int(a), t) for a, t in zip(n, texts)] == [e["local"] for e in ex], what
    refs, who = [c.ref for c in cs], [REMOVER] * len(cs)
    n, st = eng.get_lengths(None, refs, who)
    texts, st2 = eng.get_texts(None, refs, who)
    assert (st == 0).all() and (st2 == 0).all(), (what, "the remote perspective is answered")
    assert [(int(a), t) for a, t in zip(n, texts)] == [e["remote"] for e in ex], what
    for k in (0, 3, 6, 7):  # and through the single-document reads
        assert (eng.get_length(k, refs[k], REMOVER), eng.get_text(k, refs[k], REMOVER)) == ex[k]["remote"], what


def _engine(variant, extra):
    from fluidframework_amd.engine import Engine
    eng = Engine(len(SIZES), **variant, **dict(profile_caps("tiled"), **extra))
    eng.start_collab(np.full(len(SIZES), LOCAL, np.int32))
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("build", GPU_BUILDS, ids=[b[0] for b in GPU_BUILDS])
def test_gpu_one_submit(build):
    name, variant, extra = build
    eng = _engine(variant, extra)
    eng.replay(batch())
    _check_gpu(eng, name)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("build", GPU_BUILDS, ids=[b[0] for b in GPU_BUILDS])
def test_gpu_two_submits(build):
    """cut after the remove: the local insert's window pass runs in a submit of its own, on the set the first left"""
    name, variant, extra = build
    eng = _engine(variant, extra)
    head, tail = split_at_cut(cases())
    eng.replay(head)
    assert (eng.errors()[0] == 0).all()
    eng.replay(tail)
    _check_gpu(eng, name + " in two submits")
    eng.close()
