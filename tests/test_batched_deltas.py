"""Batched delta-event reads (mt_engine_deltas_batch; Engine.deltas_batch_raw / deltas_batch; oplog.filter_deltas).

The stream is the reference's "sequenceDelta" / "maintenance" callbacks in the MT_DELTA_* word format (mt_oplog.h),
which tests/test_ref_deltas.py pins to the reference on the host core and on the HIP engine one document at a time.
Here many documents are read in one call, from a cursor, whole or one kind of event only.

CPU tier: oplog.filter_deltas, the plain statement of the filter rules, on the refdelta_* fixtures' kept streams and on
the hand-decoded stream of test_ref_deltas.test_delta_stream_format_example.

GPU tier: every window equals the host core's words of the document (core_host.HostStore.deltas, pinned to the
reference), cut to the engine's dcap and passed through filter_deltas; with both event kinds also Engine.deltas(d) and
the fixtures' kept words. Both device forms (MT_VAR_DELTAS_PARALLEL) are held to the same words."""
import ctypes
import glob
import os

import numpy as np
import pytest

from fluidframework_amd import gen
from fluidframework_amd import oplog as ol
import core_host
import promotion_mix as pm
import test_ref_deltas as rd
from test_ref_goldens import caps_for

E = ol.DELTA_END
SEQ, MNT, BOTH = 1, 2, 3
E_ARG = 16  # MT_E_ARG (include/mt_engine.h)
SETS = ["c2_observer", "c3_lagged", "c5_perm", "c4_scaled"]
VP = ctypes.c_void_p

# test_delta_stream_format_example's stream, event by event
EXAMPLE = [[0, 1, 0, 5, 0, E, 1],
           [-2, 2, -1, 2, 0, -1, 3, 0, E, 2],
           [0, 2, 2, 2, 0, E, 1],
           [-2, 3, -1, 1, 0, -1, 1, 0, E, 2],
           [1, 3, 1, 1, 0, 1, 2, 0, E, 2]]


def flat(events):
    return [w for e in events for w in e]


def tup(c):
    return (c["ncap"], c["hcap"], c["acap"], c["mcap"], c["gcap"], c["ccap"])


def encode(events):
    """decode_deltas' list back into words"""
    out = []
    for op, seq, segs in events:
        out += [op, seq]
        for pos, ln, nd, pd in segs:
            out += [pos, ln, nd]
            for k, v in pd or []:
                x = (k << 16) | v
                out.append(x - (1 << 32) if x >> 31 else x)
        out += [E, len(segs)]
    return out


# ---- CPU tier: filter_deltas ------------------------------------------------------------------------------------
def kept_streams():
    for f in sorted(glob.glob(os.path.join(rd.GOLDEN, "refdelta_*.npz"))):
        z = np.load(f, allow_pickle=False)
        ko, kw = z["keep_off"], z["keep_words"]
        for d in range(len(ko) - 1):
            yield f"{os.path.basename(f)[9:-4]}/{d}", kw[ko[d]: ko[d + 1]].tolist()
    yield "example", flat(EXAMPLE)


def test_filter_deltas_partitions_the_events():
    seen = 0
    for name, w in kept_streams():
        events = ol.decode_deltas(w)
        assert ol.filter_deltas(w, BOTH) == (w, len(w)), name
        s, es = ol.filter_deltas(w, SEQ)
        m, em = ol.filter_deltas(w, MNT)
        assert es == em == len(w), name
        assert s == encode([e for e in events if e[0] >= 0]), name
        assert m == encode([e for e in events if e[0] < 0]), name
        assert len(s) + len(m) == len(w) and s and m, name
        seen += 1
    assert seen >= 13


def test_filter_deltas_example_by_hand():
    w = flat(EXAMPLE)
    assert ol.filter_deltas(w, SEQ) == (flat([EXAMPLE[0], EXAMPLE[2], EXAMPLE[4]]), len(w))
    assert ol.filter_deltas(w, MNT) == (flat([EXAMPLE[1], EXAMPLE[3]]), len(w))
    assert ol.filter_deltas(w, MNT, 17) == (EXAMPLE[3], len(w))
    assert ol.filter_deltas(w, SEQ, len(w)) == ([], len(w))
    assert ol.filter_deltas([], SEQ) == ([], 0) and ol.filter_deltas([], BOTH) == ([], 0)


def test_filter_deltas_drops_a_cut_tail_and_reports_its_start():
    w = flat(EXAMPLE)
    starts = np.cumsum([0] + [len(e) for e in EXAMPLE]).tolist()
    for cut in range(len(w) + 1):
        head = w[:cut]
        tail = max(s for s in starts if s <= cut)  # the start of the event the cut falls in (cut itself at a boundary)
        whole = [e for e, s in zip(EXAMPLE, starts) if s + len(e) <= cut]
        assert ol.filter_deltas(head, BOTH) == (head, cut)
        assert ol.filter_deltas(head, SEQ) == (flat([e for e in whole if e[0] >= 0]), tail), cut
        assert ol.filter_deltas(head, MNT) == (flat([e for e in whole if e[0] < 0]), tail), cut
    for name, w in kept_streams():  # the fixtures' streams cut where a 2^15-word log cuts them
        if len(w) > 1 << 15:
            head = w[: 1 << 15]
            s, end = ol.filter_deltas(head, SEQ)
            assert end <= len(head) and ol.filter_deltas(head, MNT)[1] == end, name
            assert ol.decode_deltas(head[:end]) and ol.filter_deltas(head[:end], SEQ) == (s, end), name


def test_filter_deltas_refuses_a_cursor_inside_an_event():
    w = flat(EXAMPLE)
    starts = set(np.cumsum([0] + [len(e) for e in EXAMPLE]).tolist())
    for c in range(-2, len(w) + 3):
        for kinds in (SEQ, MNT, BOTH):
            if c in starts:
                kept, end = ol.filter_deltas(w, kinds, c)
                assert end == len(w) and kept == ol.filter_deltas(w[c:], kinds)[0]
            else:
                with pytest.raises(ValueError):
                    ol.filter_deltas(w, kinds, c)
    for kinds in (0, 4, 7, -1):
        with pytest.raises(ValueError):
            ol.filter_deltas(w, kinds)


def test_filter_deltas_finds_event_ends_by_structure():
    """a property delta (key << 16 | value) with key 0x8000 and no previous value IS the word MT_DELTA_END (the
    interner hands out key ids up to 0xFFFE): an event's end comes from its segments' nd counts, never from the value"""
    ann = [2, 7, 0, 4, 2, E, 5, 4, 3, 1, E, E, 2]  # ANNOTATE, two segments; both deltas of key 0x8000 read as END
    w = EXAMPLE[0] + ann + EXAMPLE[1]
    assert len(ol.decode_deltas(w)) == 3
    assert ol.filter_deltas(w, SEQ) == (EXAMPLE[0] + ann, len(w))
    assert ol.filter_deltas(w, MNT) == (EXAMPLE[1], len(w))
    with pytest.raises(ValueError):
        ol.filter_deltas(w, SEQ, len(EXAMPLE[0]) + 7)  # after (END, 5): inside the event
    assert ol.filter_deltas(w[: len(EXAMPLE[0]) + 7], SEQ) == (EXAMPLE[0], len(EXAMPLE[0]))


# ---- hand-built logs: where the terminator falls in the stream ----------------------------------------------------
def build_log(it, n_mid, n_ann, n_end):
    """one 40-unit insert; n_mid one-unit inserts inside it, each splitting its tail (SPLIT + INSERT, 17 words); n_ann
    annotates of the first segment (8 words each); n_end inserts at the end (7 words each). minSeq stays 0: no zamboni"""
    log = ol.DocLog(it, local_long_id=0)
    seq = 0

    def add(kind, **kw):
        nonlocal seq
        seq += 1
        log.add(kind, client=1, seq=seq, ref_seq=seq - 1, min_seq=0, **kw)
    add(ol.OP_INSERT, pos1=0, text="a" * 40)
    for k in range(n_mid):
        add(ol.OP_INSERT, pos1=2 + 3 * k, text="X")
    for k in range(n_ann):
        add(ol.OP_ANNOTATE, pos1=0, pos2=2, props={"k": k + 1})
    for k in range(n_end):
        add(ol.OP_INSERT, pos1=40 + n_mid + k, text="z")
    return log


def host_words(logs, dcap=1 << 12):
    b = ol.Batch.from_logs(logs)
    _, err, st = core_host.replay_batch(b, core_host.DEFAULT_CAPS, dcap=dcap)
    assert (err == 0).all()
    return b, [st.deltas(d)[2].tolist() for d in range(b.ndocs)]


@pytest.fixture(scope="module")
def boundary_logs():
    """logs whose last event's terminator pair (MT_DELTA_END, nseg) sits at words 62/63, 63/64 and 64/65 (a wave's pass
    of 64 words ends between, after and before the two), each with SPLIT events; then a 31-word log and one of no
    records"""
    found, it = {}, gen.generator_interner()
    for n_mid in range(1, 5):
        for n_ann in range(0, 8):
            for n_end in range(1, 9):
                total = 7 + 17 * n_mid + 8 * n_ann + 7 * n_end
                if total - 2 in (62, 63, 64) and total - 2 not in found:
                    found[total - 2] = build_log(it, n_mid, n_ann, n_end)
    assert sorted(found) == [62, 63, 64]
    logs = [found[63], found[62], found[64], build_log(it, 1, 0, 1), ol.DocLog(it, local_long_id=0)]
    b, words = host_words(logs)
    for t, w in zip((63, 62, 64), words):
        assert len(w) == t + 2 and w[t] == E and w[t + 1] == 1, (t, len(w))
        assert any(e[0] < 0 for e in ol.decode_deltas(w))
    assert len(words[3]) == 31 and words[4] == []
    return b, words


def test_boundary_logs_put_the_terminator_where_stated(boundary_logs):
    b, words = boundary_logs
    assert [len(w) for w in words] == [65, 64, 66, 31, 0]
    for w in words:
        s, m = ol.filter_deltas(w, SEQ), ol.filter_deltas(w, MNT)
        assert s[1] == m[1] == len(w) and len(s[0]) + len(m[0]) == len(w)
        assert ol.filter_deltas(w[:-1], SEQ)[1] == max(len(w) - 7, 0)  # the last event is a 7-word INSERT


# ---- GPU tier -------------------------------------------------------------------------------------------------
def _engine(b, caps, dcap, **kw):
    from fluidframework_amd.engine import Engine
    eng = Engine(b.ndocs, dcap=dcap, **caps, **kw)
    eng.start_collab(b.local_long_id)
    return eng


def _clean(eng):
    err, err_op = eng.errors()
    assert (err == 0).all(), (err[err != 0][:8], err_op[err != 0][:8])


class Spec:
    """a fixture set replayed on the host core with a log that holds every word"""

    def __init__(self, name):
        self.name = name
        self.z, self.w, self.b = rd.load(name)
        self.caps = caps_for(self.w)
        self.full = int(self.z["nwords"].max())
        _, err, st = core_host.replay_batch(self.b, tup(self.caps), dcap=self.full)
        assert (err == 0).all()
        self.words, self.memo = [], {}
        for d in range(self.b.ndocs):
            n, _, w = st.deltas(d)
            assert n == self.z["nwords"][d]
            self.words.append(w.copy())
        self.bounds = [set(e for _, e, _ in ol._delta_event_spans(w.tolist())[0]) | {0} for w in self.words]

    def mixed_dcap(self):
        """a log size between the documents' word counts that cuts at least one saturating document inside an event"""
        n = np.sort(self.z["nwords"])
        dcap = int(n[len(n) // 2])
        while not any(len(w) > dcap and dcap not in bd for w, bd in zip(self.words, self.bounds)):
            dcap += 1
        sat = [len(w) > dcap for w in self.words]
        assert any(sat) and not all(sat)
        return dcap

    def want(self, d, dcap, kinds, from_word=0):
        key = (d, dcap, kinds, from_word)
        if key not in self.memo:
            kept, end = ol.filter_deltas(self.words[d][:dcap], kinds, from_word)
            self.memo[key] = (np.asarray(kept, np.int32), end)
        return self.memo[key]


_specs = {}


@pytest.fixture(scope="module", params=SETS)
def spec(request):
    if request.param not in _specs:
        _specs[request.param] = Spec(request.param)
    return _specs[request.param]


@pytest.fixture(scope="module")
def engines(spec):
    """the set replayed with a 2^15-word log (every document saturates) and with the mixed one"""
    out = {}
    for dcap in (1 << 15, spec.mixed_dcap()):
        eng = _engine(spec.b, spec.caps, dcap)
        eng.replay(spec.b)
        _clean(eng)
        out[dcap] = eng
    yield out
    for eng in out.values():
        eng.close()


def windows(off, words):
    return [words[off[i]: off[i + 1]] for i in range(len(off) - 1)]


@pytest.mark.gpu
def test_gpu_verbatim_parity(spec, engines):
    for dcap, eng in engines.items():
        off, words, end, emitted, st = eng.deltas_batch_raw()
        assert len(off) == spec.b.ndocs + 1 and off[0] == 0 and off[-1] == len(words)
        assert (st == 0).all() and np.array_equal(emitted, spec.z["nwords"])
        got = windows(off, words)
        for d in range(spec.b.ndocs):
            want = spec.words[d][:dcap]
            assert np.array_equal(got[d], want), (dcap, d, rd.first_diff(got[d], want))
            assert end[d] == len(want), (dcap, d)
            assert np.array_equal(got[d], eng.deltas(d)), (dcap, d)
        ko, kw = spec.z["keep_off"], spec.z["keep_words"]
        for d in range(len(ko) - 1):
            assert np.array_equal(got[d], kw[ko[d]: ko[d + 1]][:dcap]), (dcap, d)
        as_list = eng.deltas_batch()
        assert len(as_list) == spec.b.ndocs and all(np.array_equal(a, g) for a, g in zip(as_list, got))
    sat = emitted > max(engines)
    assert sat.any() and not sat.all()  # the mixed log: some documents saturate (one of them mid-event), some do not
    assert (np.asarray([len(w) for w in spec.words]) > 1 << 15).all()


@pytest.mark.gpu
@pytest.mark.parametrize("par", [1, 0], ids=["wave", "serial"])
def test_gpu_filtered_parity(spec, engines, par):
    from fluidframework_amd.engine import MT_VAR_DELTAS_PARALLEL
    cut = 0
    for dcap, eng in engines.items():
        eng.set_variant(MT_VAR_DELTAS_PARALLEL, par)
        try:
            for kinds in (SEQ, MNT):
                off, words, end, emitted, st = eng.deltas_batch_raw(kinds=kinds)
                assert (st == 0).all() and np.array_equal(emitted, spec.z["nwords"])
                got = windows(off, words)
                for d in range(spec.b.ndocs):
                    want, wend = spec.want(d, dcap, kinds)
                    assert np.array_equal(got[d], want), (dcap, kinds, d, rd.first_diff(got[d], want))
                    assert end[d] == wend, (dcap, kinds, d)
                    cut += wend < min(len(spec.words[d]), dcap)
            v = eng.deltas_batch_raw(kinds=BOTH)  # the verbatim form of this walk
            assert all(np.array_equal(g, spec.words[d][:dcap]) for d, g in enumerate(windows(v[0], v[1])))
        finally:
            eng.set_variant(MT_VAR_DELTAS_PARALLEL, 1)
    assert cut  # a dropped tail: `end` was its start


@pytest.mark.gpu
@pytest.mark.parametrize("par", [1, 0], ids=["wave", "serial"])
def test_gpu_terminator_at_the_pass_boundary(boundary_logs, par):
    from fluidframework_amd.engine import MT_VAR_DELTAS_PARALLEL
    b, words = boundary_logs
    caps = dict(ncap=192, hcap=256, acap=1 << 16, mcap=4096, gcap=1024, ccap=64)
    for dcap in (4096, 64, 63, 65):  # the whole streams; logs cut between, before and after the pair at 63 / 64
        eng = _engine(b, caps, dcap)
        eng.set_variant(MT_VAR_DELTAS_PARALLEL, par)
        eng.replay(b)
        _clean(eng)
        for kinds in (SEQ, MNT, BOTH):
            off, got, end, emitted, st = eng.deltas_batch_raw(kinds=kinds)
            assert (st == 0).all() and emitted.tolist() == [len(w) for w in words]
            for d, g in enumerate(windows(off, got)):
                want, wend = ol.filter_deltas(words[d][:dcap], kinds)
                assert g.tolist() == want and end[d] == wend, (dcap, kinds, d)
        # every cursor of every document at once: the boundaries answer, the others are refused alone
        docs = np.concatenate([np.full(min(len(w), dcap) + 3, d) for d, w in enumerate(words)])
        cur = np.concatenate([np.arange(-1, min(len(w), dcap) + 2) for w in words])
        off, got, end, _, st = eng.deltas_batch_raw(docs, cur, SEQ)
        for i, g in enumerate(windows(off, got)):
            w = words[docs[i]][:dcap]
            try:
                want, wend = ol.filter_deltas(w, SEQ, int(cur[i]))
            except ValueError:
                assert st[i] == E_ARG and len(g) == 0, (dcap, docs[i], cur[i])
                continue
            assert st[i] == 0 and g.tolist() == want and end[i] == wend, (dcap, docs[i], cur[i])
        eng.close()


@pytest.mark.gpu
def test_gpu_cursors(spec):
    """half of each log, a read from 0, the rest, a read from the returned cursor: together the one-shot read"""
    b = spec.b
    eng = _engine(b, spec.caps, spec.full)
    per = [b.doc_arrays(d) for d in range(b.ndocs)]
    half = []
    for ops, _, _, _ in per:
        h = len(ops) // 2
        while h > 0 and ops["kind"][h - 1] & 0x40:  # not inside a group op's members
            h -= 1
        half.append(h)
    docs = np.arange(b.ndocs)
    first = {}
    for part in (0, 1):
        arrays = [(ops[:h] if part == 0 else ops[h:], text, props, kv) for (ops, text, props, kv), h in zip(per, half)]
        eng.submit_docs(docs, ol.Batch.from_arrays(arrays, b.local_long_id))
        eng.run()
        eng.sync()
        _clean(eng)
        for kinds in (BOTH, SEQ):
            if part == 0:
                off, words, end, emitted, st = eng.deltas_batch_raw(kinds=kinds)
                assert (st == 0).all() and np.array_equal(end, emitted) and (end > 0).all() and (end < spec.full).all()
                first[kinds] = (windows(off, words), end)
                continue
            head, cur = first[kinds]
            off, words, end, emitted, st = eng.deltas_batch_raw(from_words=cur, kinds=kinds)
            assert (st == 0).all() and np.array_equal(emitted, spec.z["nwords"]) and np.array_equal(end, emitted)
            for d, tail in enumerate(windows(off, words)):
                want, _ = spec.want(d, spec.full, kinds)
                assert np.array_equal(np.concatenate([head[d], tail]), want), (kinds, d)
    # a cursor inside an event, a negative one and one past the end: refused alone, between two good neighbours
    cur = first[BOTH][1]
    d = 1
    nlog = len(spec.words[d])
    inside = next(c for c in range(int(cur[d]) + 1, nlog) if c not in spec.bounds[d])
    q = np.asarray([0, d, 2, d, 0, d, 2])
    fw = np.asarray([cur[0], inside, cur[2], -1, 0, nlog + 1, len(spec.words[2])])  # the last: doc 2's logged end
    for kinds in (BOTH, SEQ):
        off, words, end, _, st = eng.deltas_batch_raw(q, fw, kinds)
        assert st.tolist() == [0, E_ARG, 0, E_ARG, 0, E_ARG, 0]
        for i, g in enumerate(windows(off, words)):
            if st[i]:
                assert len(g) == 0
            else:
                want, wend = spec.want(int(q[i]), spec.full, kinds, int(fw[i]))
                assert np.array_equal(g, want) and end[i] == wend, (kinds, i)
    eng.close()


def _raw(eng, m, docs, fw, kinds, out, cap, want_end=True):
    off = np.full(m + 1, -7, np.int64)
    end, emitted = np.full(max(m, 1), -7, np.int64), np.full(max(m, 1), -7, np.int64)
    st = np.full(max(m, 1), -7, np.int32)

    def p(a):
        return None if a is None else a.ctypes.data_as(VP)
    n = eng.L.mt_engine_deltas_batch(eng.h, m, p(docs), p(fw), kinds, p(off), p(end) if want_end else None,
                                     p(emitted) if want_end else None, p(st), p(out), cap)
    return n, off, end, emitted, st


@pytest.mark.gpu
def test_gpu_call_contract():
    from fluidframework_amd.engine import EngineError
    sp = _specs.get("c3_lagged") or Spec("c3_lagged")
    dcap = 1 << 12
    eng = _engine(sp.b, sp.caps, dcap)
    eng.replay(sp.b)
    _clean(eng)
    rng = np.random.default_rng(11)
    docs = np.concatenate([rng.permutation(sp.b.ndocs)[:40], [5, 5, 5, 0, 127, 0]]).astype(np.int64)
    for kinds in (BOTH, MNT):
        got = eng.deltas_batch(docs, kinds=kinds)
        assert len(got) == len(docs)
        for i, d in enumerate(docs):
            assert np.array_equal(got[i], sp.want(int(d), dcap, kinds)[0]), (kinds, i)
    # docs = None is documents 0..m-1, for any m up to the engine's
    n, off, end, emitted, st = _raw(eng, 7, None, None, BOTH, None, 0)
    assert n == 7 * dcap and off.tolist() == [dcap * i for i in range(8)] and (st == 0).all()
    assert (end == dcap).all() and np.array_equal(emitted, sp.z["nwords"][:7])
    # m == 0 touches nothing
    n, off, end, emitted, st = _raw(eng, 0, None, None, BOTH, None, 0)
    assert n == 0 and off[0] == -7 and st[0] == -7
    # the size query, then a buffer one word short: nothing written, the total and the offsets still returned
    n, off, _, _, st = _raw(eng, len(docs), docs, None, SEQ, None, 0)
    want = [sp.want(int(d), dcap, SEQ)[0] for d in docs]
    assert n == sum(len(w) for w in want) and np.array_equal(np.diff(off), [len(w) for w in want])
    canary = np.full(n + 8, 0x5A5A5A5A, np.int32)
    n2, off2, _, _, st2 = _raw(eng, len(docs), docs, None, SEQ, canary, n - 1, want_end=False)
    assert n2 == n and np.array_equal(off2, off) and (st2 == 0).all() and (canary == 0x5A5A5A5A).all()
    n3, off3, _, _, _ = _raw(eng, len(docs), docs, None, SEQ, canary, n)
    assert n3 == n and np.array_equal(canary[:n], np.concatenate(want)) and (canary[n:] == 0x5A5A5A5A).all()
    # kinds 0 and unknown bits; a document out of range; an engine without a delta log
    for kinds in (0, 4, 7, -1):
        assert _raw(eng, 3, None, None, kinds, None, 0)[0] == -E_ARG
        with pytest.raises(EngineError):
            eng.deltas_batch_raw(kinds=kinds)
    assert _raw(eng, 1, np.asarray([sp.b.ndocs], np.int64), None, BOTH, None, 0)[0] == -E_ARG
    eng.close()
    plain = _engine(sp.b, sp.caps, 0)
    assert _raw(plain, 3, None, None, BOTH, None, 0)[0] == -E_ARG
    assert _raw(plain, 0, None, None, BOTH, None, 0)[0] == -E_ARG
    plain.close()


@pytest.mark.gpu
def test_gpu_promoted_documents():
    """small capacities: some documents replay again in larger profiles (one through two promotions), whose engines
    log four times as many words; the answers are cut at the caller's dcap and land at the caller's query index"""
    dcap = 4096
    b = pm.text_refs(pm.text_mix())
    _, err, st = core_host.replay_batch(b, pm.tup(pm.BIG), dcap=4 * dcap, rcap=32)
    assert (err == 0).all()
    words = [st.deltas(d)[2][: 4 * dcap] for d in range(b.ndocs)]
    emitted = [st.deltas(d)[0] for d in range(b.ndocs)]
    assert all(n > dcap for n in emitted)
    eng = _engine(b, pm.SMALL, dcap, rcap=32)
    eng.replay(b)
    _clean(eng)
    assert set(eng.promoted().tolist()) == set(pm.TEXT_PROMOTED)
    docs = np.asarray(sorted(pm.TEXT_PROMOTED) + list(range(b.ndocs)) + sorted(pm.TEXT_PROMOTED)[::-1], np.int64)
    for kinds in (BOTH, SEQ, MNT):
        off, got, end, em, status = eng.deltas_batch_raw(docs, kinds=kinds)
        assert (status == 0).all() and em.tolist() == [emitted[d] for d in docs]
        for i, g in enumerate(windows(off, got)):
            want, wend = ol.filter_deltas(words[docs[i]][:dcap], kinds)
            assert g.tolist() == want and end[i] == wend, (kinds, i, docs[i])
            if kinds == BOTH:
                assert np.array_equal(g, eng.deltas(int(docs[i])))
    # cursors are counted in the caller's log: one at dcap is the logged end, one past it is refused
    p = sorted(pm.TEXT_PROMOTED)[0]
    _, got, end, _, status = eng.deltas_batch_raw([p, p, 0], [dcap, dcap + 1, dcap], BOTH)
    assert status.tolist() == [0, E_ARG, 0] and len(got) == 0 and (end[0], end[2]) == (dcap, dcap)
    eng.close()
