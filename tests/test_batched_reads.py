"""The batched reads (include/mt_engine.h mt_engine_get_lengths / _get_texts / _get_containing_segments /
_resolve_remote_client_positions / _adjust_positions): many queries per launch, answered as the single-document
calls answer them.

CPU tier: the header declares the entry points and the library exports them. GPU tier: the REFERENCE's getText
fixtures (tests/golden/reftext_*.npz) through one get_texts call per placeholder; promoted documents
(tests/promotion_mix.py) over all documents, a shuffled subset and a list with repeats; refused perspectives per
query; and hand-built documents at the shapes where the fill kernel's packed copy (mt_core.h packed_copy) can go
wrong, against the single-document read and the host build of the core."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from fluidframework_amd import gen, native
from fluidframework_amd import oplog as ol
import core_host
import persp_logs as pl
import promotion_mix as pm
import test_ref_text as rt
from test_ref_goldens import caps_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mt_engine_get_lengths", "mt_engine_get_texts", "mt_engine_get_containing_segments",
         "mt_engine_resolve_remote_client_positions", "mt_engine_adjust_positions")
MT_E_UNSUPPORTED, MT_E_ARG = 4, 16
MT_VAR_TEXTS_PACKED = 4
SEG_FIELDS = ("rid", "gen", "offset", "length", "seq", "client", "removed_seq", "removed_client", "ordinal")


# ---- CPU tier ---------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_batched_reads():
    hdr = open(os.path.join(ROOT, "include", "mt_engine.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = native.build_replay()
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    for n in NAMES:
        assert re.search(rf"\b{n}\s*\(", hdr), f"{n} is not declared"
        assert n in exported, f"{n} is not exported"


def test_refusal_batch_holds_both_kinds_of_query():
    b, q = _refusal_queries()
    ok = np.asarray([pl.answered(b.doc(d)[0], int(b.local_long_id[d]), r, c) for d, r, c in q])
    assert ok.any() and (~ok).any()


# ---- helpers ----------------------------------------------------------------------------------------------------
def _engine(b, caps, **kw):
    from fluidframework_amd.engine import Engine
    eng = Engine(b.ndocs, **caps, **kw)
    eng.start_collab(b.local_long_id)
    eng.replay(b)
    err, err_op = eng.errors()
    assert (err == 0).all(), (err, err_op)
    return eng


def _seg(s):
    return None if s is None or s.rid < 0 else tuple(getattr(s, f) for f in SEG_FIELDS)


def _single(f, *a):
    """a single-document call's outcome: its value, or ("refused", code)"""
    from fluidframework_amd.engine import EngineError
    try:
        return f(*a)
    except EngineError as ex:
        return ("refused", ex.code)


# ---- the reference's getText fixtures ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("name", rt.NAMES)
def test_gpu_get_texts_matches_reference(name, waves):
    z, w, b = rt.load(name)
    eng = _engine(b, caps_for(w), waves=waves)
    q, ph = z["queries"], np.asarray([str(p) for p in z["placeholders"]])
    answers = [None] * len(q)
    for p in sorted(set(ph.tolist())):  # every query of the fixture under this placeholder: one call
        idx = np.nonzero(ph == p)[0]
        texts, st = eng.get_texts(docs=q[idx, 0], ref_seqs=q[idx, 1], long_clients=q[idx, 2], placeholder=p,
                                  starts=[None if a == rt.DEFAULT else int(a) for a in q[idx, 3]],
                                  ends=[None if e == rt.DEFAULT else int(e) for e in q[idx, 4]])
        assert (st == 0).all(), (p, idx[st != 0][:5])
        for i, t in zip(idx, texts):
            answers[i] = t
    it = iter(answers)
    rt.check(z, lambda *_: next(it))  # lengths, FNV-1a-64 and document 0's units, in the fixture's query order
    eng.close()


# ---- promoted documents -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text_eng():
    b = pm.text_mix()
    eng = _engine(b, pm.SMALL)
    assert set(eng.promoted().tolist()) == pm.TEXT_PROMOTED
    yield eng, b
    eng.close()


def _doc_lists(n):
    rng = np.random.default_rng(7)
    return [None, rng.permutation(n)[: n - 3], np.asarray([4, 0, 4, 1, 12, 1, 4, 3, 12, 0])]


@pytest.mark.gpu
def test_gpu_lengths_and_texts_of_promoted_documents(text_eng):
    eng, b = text_eng
    want_len = [eng.get_length(d) for d in range(b.ndocs)]
    want_text = [eng.get_text(d) for d in range(b.ndocs)]
    assert min(len(t) for t in want_text) > 0
    for docs in _doc_lists(b.ndocs):
        ids = range(b.ndocs) if docs is None else docs.tolist()
        n, st = eng.get_lengths(docs)
        assert (st == 0).all() and n.tolist() == [want_len[d] for d in ids]
        texts, st = eng.get_texts(docs)
        assert (st == 0).all() and texts == [want_text[d] for d in ids]


@pytest.mark.gpu
def test_gpu_get_texts_sizing(text_eng):
    """off is non-decreasing and ends at the return value; a cap one short writes nothing; out = NULL sizes"""
    eng, b = text_eng
    m = b.ndocs
    off, st = np.zeros(m + 1, np.int64), np.zeros(m, np.int32)

    def call(out, cap):
        p = None if out is None else out.ctypes.data_as(ctypes.c_void_p)
        return eng.L.mt_engine_get_texts(eng.h, m, None, None, None, None, None, None, 0,
                                         off.ctypes.data_as(ctypes.c_void_p), st.ctypes.data_as(ctypes.c_void_p), p, cap)
    total = call(None, 0)
    assert total == sum(eng.get_length(d) for d in range(m)) and off[0] == 0 and off[m] == total
    assert (np.diff(off) >= 0).all()
    buf = np.full(total + 8, 0xA5A5, "<u2")
    assert call(buf, total - 1) == total and (buf == 0xA5A5).all()
    assert call(buf, total) == total and (buf[total:] == 0xA5A5).all()
    assert buf[:total].tobytes().decode("utf-16-le") == "".join(eng.get_text(d) for d in range(m))
    # m == 0 touches nothing; a bad document id fails the call
    off[:] = -1
    assert eng.L.mt_engine_get_texts(eng.h, 0, None, None, None, None, None, None, 0, None, None, None, 0) == 0
    bad = np.asarray([0, m], np.int64)
    assert eng.L.mt_engine_get_lengths(eng.h, 2, bad.ctypes.data_as(ctypes.c_void_p), None, None,
                                       st.ctypes.data_as(ctypes.c_void_p), None) == MT_E_ARG


@pytest.mark.gpu
def test_gpu_containing_segments_of_promoted_documents(text_eng):
    eng, b = text_eng
    lens = [eng.get_length(d) for d in range(b.ndocs)]
    for docs in _doc_lists(b.ndocs):
        ids = list(range(b.ndocs)) if docs is None else docs.tolist()
        for at in (lambda n: 0, lambda n: n // 2, lambda n: n - 1, lambda n: n):
            pos = [at(lens[d]) for d in ids]
            segs, st = eng.get_containing_segments(pos, docs)
            assert (st == 0).all()
            for i, d in enumerate(ids):
                assert _seg(segs[i]) == _seg(eng.get_containing_segment(d, pos[i])), (d, pos[i])


@pytest.mark.gpu
def test_gpu_remote_positions_of_promoted_documents():
    b = pm.perm_mix()
    eng = _engine(b, pm.MAT, pcap=pm.PCAP)
    assert set(eng.promoted().tolist()) == pm.PERM_PROMOTED
    checked = 0
    for docs in _doc_lists_perm(b.ndocs):
        ids = list(range(b.ndocs)) if docs is None else docs.tolist()
        dq, pq, sq, cq = [], [], [], []
        for d in ids:
            ops = b.doc(d)[0]
            cur, _ = pl.window(ops)
            local = int(b.local_long_id[d])
            n = eng.get_length(d)
            for c in sorted(set(int(x) for x in ops["client"][(ops["kind"] & ol.OPF_LOCAL) == 0]) - {local}):
                for p in (0, n // 3, n - 1, n, n + 2):
                    dq.append(d), pq.append(p), sq.append(cur), cq.append(c)
        res, st1 = eng.resolve_remote_client_positions(pq, sq, cq, docs=dq)
        adj, st2 = eng.adjust_positions(pq, sq, cq, docs=dq)
        for i in range(len(dq)):
            one = _single(eng.resolve_remote_client_position, dq[i], pq[i], sq[i], cq[i])
            two = _single(eng.adjust_position, dq[i], pq[i], sq[i], cq[i])
            for got, stat, want in ((res, st1, one), (adj, st2, two)):
                if isinstance(want, tuple):
                    assert (int(stat[i]), int(got[i])) == (want[1], -1), (dq[i], pq[i], cq[i])
                else:
                    assert stat[i] == 0 and int(got[i]) == (-1 if want is None else want), (dq[i], pq[i], cq[i])
                    checked += 1
    assert checked > 100
    eng.close()


def _doc_lists_perm(n):
    return [None, np.asarray([4, 0, 1, 4, 5, 1])]


# ---- refused perspectives ---------------------------------------------------------------------------------------
def _refusal_queries():
    """one config-3 batch of 8 documents x 256 ops; (doc, refSeq, long client) for every long client of each log and
    refSeq in range(0, currentSeq + 1, 16)"""
    b = gen.generate(gen.config3(256), ids=np.arange(8), threads=4)
    q = []
    for d in range(b.ndocs):
        ops = b.doc(d)[0]
        cur, _ = pl.window(ops)
        for c in sorted(set(int(x) for x in ops["client"][(ops["kind"] & ol.OPF_LOCAL) == 0])):
            q += [(d, r, c) for r in range(0, cur + 1, 16)]
    return b, q


@pytest.mark.gpu
def test_gpu_lengths_refuse_per_query():
    from fluidframework_amd.engine import default_caps
    b, q = _refusal_queries()
    eng = _engine(b, default_caps(256))
    qa = np.asarray(q)
    n, st = eng.get_lengths(qa[:, 0], qa[:, 1], qa[:, 2])
    kinds = set()
    for i, (d, r, c) in enumerate(q):
        want = _single(eng.get_length, d, r, c)
        if isinstance(want, tuple):
            assert want[1] == MT_E_UNSUPPORTED and (int(st[i]), int(n[i])) == (MT_E_UNSUPPORTED, 0), (d, r, c)
        else:
            assert (int(st[i]), int(n[i])) == (0, want), (d, r, c)
        kinds.add(isinstance(want, tuple))
    assert kinds == {True, False}
    # the texts refuse the same queries, with an empty text each
    texts, st2 = eng.get_texts(qa[:, 0], qa[:, 1], qa[:, 2])
    assert (st2 == st).all() and all(t == "" for t, s in zip(texts, st) if s) and [len(t) for t in texts] == n.tolist()
    eng.close()


# ---- the tiled profile ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_batched_reads_tiled_profile():
    """the tiled profile's reads keep search scratch in the document block: queries that name one document run in
    successive launches, and answer as the single calls do, a document named five times included"""
    from fluidframework_amd.engine import default_caps
    b = gen.generate(gen.config3(512), ids=np.arange(3), threads=3)
    eng = _engine(b, default_caps(512, config=4))
    docs = [1, 0, 1, 2, 1, 0, 1, 1]
    cur = [pl.window(b.doc(d)[0])[0] for d in range(b.ndocs)]
    lens = [eng.get_length(d) for d in range(b.ndocs)]
    n, st = eng.get_lengths(docs)
    assert (st == 0).all() and n.tolist() == [lens[d] for d in docs]
    # a client that has sent nothing, at the current seq: sequenced content, through the position index
    n, st = eng.get_lengths(docs, [cur[d] for d in docs], 77)
    assert (st == 0).all() and n.tolist() == [eng.get_length(d, cur[d], 77) for d in docs]
    texts, st = eng.get_texts(docs)
    assert (st == 0).all() and texts == [eng.get_text(d) for d in docs]
    pos = [(i * lens[d]) // len(docs) for i, d in enumerate(docs)]
    segs, st = eng.get_containing_segments(pos, docs)
    assert (st == 0).all()
    assert [_seg(s) for s in segs] == [_seg(eng.get_containing_segment(d, p)) for d, p in zip(docs, pos)]
    res, st = eng.resolve_remote_client_positions(pos, [cur[d] for d in docs], 77, docs=docs)
    want = [eng.resolve_remote_client_position(d, p, cur[d], 77) for d, p in zip(docs, pos)]
    assert (st == 0).all() and res.tolist() == [-1 if w is None else w for w in want]
    eng.close()


# ---- copy edges -------------------------------------------------------------------------------------------------
ALPHA = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"


def _rows_log(it, texts, markers=()):
    """a document of one row per entry of `texts`, appended in order by two remote clients (minSeq stays 0: zamboni
    merges nothing); the entries at `markers` are Marker inserts"""
    log = ol.DocLog(it, local_long_id=0)
    pos = 0
    for i, t in enumerate(texts):
        kw = dict(client=1 + i % 2, seq=i + 1, ref_seq=i, min_seq=0, pos1=pos)
        if i in markers:
            log.add(ol.OP_INSERT, marker=i & 1, **kw)
            pos += 1
        else:
            log.add(ol.OP_INSERT, text=t, **kw)
            pos += len(t)
    return log


def _edge_docs():
    """(log, rows) per document: the smallest shapes at which the packed copy can go wrong"""
    it = ol.Interner()
    units = lambda n, k=0: [ALPHA[(k + i) % len(ALPHA)] for i in range(n)]
    long_seg = "".join(ALPHA[(3 * i) % len(ALPHA)] for i in range(301))
    docs = [
        (["abc", "de", "f", "ghijk"], ()),                # 0: an odd total (11): the next text starts on a 2-byte boundary
        ([], ()),                                         # 1: an empty document between two non-empty ones
        (["x"], ()),                                      # 2: one 1-unit segment
        (units(63), ()),                                  # 3-5: single-unit rows around a pass of 64
        (units(64, 5), ()),
        (units(65, 9), ()),
        (["ab", "", "cde", "", "", "f", "", "gh"], {1, 3, 4, 6}),  # 6: markers (the placeholder's pieces)
        (["pq", long_seg, "r"], ()),                      # 7: one segment longer than 128 units
        (units(200, 1), ()),                              # 8: several passes of single-unit rows
        (["", "", ""], {0, 1, 2}),                        # 9: markers only
    ]
    return [(_rows_log(it, t, mk), len(t)) for t, mk in docs]


# (start, end) per query, besides the default range: inside a piece, across pieces, swapped, past the end
EDGE_RANGES = ((None, None), (1, None), (None, 2), (1, 2), (3, 150), (64, 65), (62, 66), (150, 3), (-4, 7), (2, 100000),
               (5, 5))


@pytest.fixture(scope="module")
def edge_eng():
    from fluidframework_amd.engine import default_caps
    logs = _edge_docs()
    b = ol.Batch.from_logs([g for g, _ in logs])
    eng = _engine(b, default_caps(512))
    for d, (_, rows) in enumerate(logs):  # one row per insert: nothing merged, nothing split
        assert len(eng.segment_ids(d)) == rows, d
    assert (eng.stats()[[3, 4, 5], 1] >= [63, 64, 65]).all()
    _, err, host = core_host.replay_batch(b)
    assert (err == 0).all()
    yield eng, b, host
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [1, 0])
@pytest.mark.parametrize("placeholder", ["", "<>", "#"])
def test_gpu_get_texts_copy_edges(edge_eng, packed, placeholder):
    eng, b, host = edge_eng
    eng.set_variant(MT_VAR_TEXTS_PACKED, packed)
    docs, starts, ends = [], [], []
    for a, e in EDGE_RANGES:
        for d in range(b.ndocs):
            docs.append(d), starts.append(a), ends.append(e)
    texts, st = eng.get_texts(docs, placeholder=placeholder, starts=starts, ends=ends)
    assert (st == 0).all()
    for i, d in enumerate(docs):
        assert texts[i] == host.text_range(d, 0, -1, placeholder, starts[i], ends[i]), (d, starts[i], ends[i])
        assert texts[i] == eng.get_text(d, placeholder=placeholder, start=starts[i], end=ends[i]), (d, starts[i], ends[i])
    assert any(len(t) % 2 for t in texts) and max(len(t) for t in texts) > 128
    # each text alone starts at offset 0 (a 4-byte boundary), in the list above most start on odd offsets
    for d in range(b.ndocs):
        assert eng.get_texts([d], placeholder=placeholder)[0] == [host.text_range(d, 0, -1, placeholder)]
    # the view of a client that has sent nothing, at an early refSeq: the rows sequenced by then
    rs = [3, 30, 64]
    views, st = eng.get_texts([3, 4, 5], rs, [7, 7, 7], placeholder=placeholder)
    assert (st == 0).all()
    assert views == [host.text_range(d, r, 7, placeholder) for d, r in zip([3, 4, 5], rs)]
    assert [len(v) for v in views] == rs
