"""Batched PermutationVector reads against the REFERENCE (tests/golden/refhvec.npz from tools/make_ref_goldens.py --hvec
over tests/hvec_logs.py): HandleCache.getHandles ranges and PermutationVector.handleToPosition as restated over the
reference Client after replaying each hand-built log, and every document's HandleTable.snapshot(). The case list is the
docstring of tests/hvec_logs.py. Every comparison is exact, and no recorded query is left out: a recorded throw is
MT_E_ARG. Two kinds of recorded throw are the validity rule of the batched call, not behaviour observed from the
reference: HandleCache.getHandles checks nothing itself, so for an empty range outside [0, length] and for a reversed
range (end < start) its loop would run zero times and return []; the restatement in tools/ref_replay.mjs refuses
them (the fixture's `range_rule_throws` marks these queries). Every other throw is an assert or error of reference
code. The reference's raw segment.start + offset is normalised the way mt_engine_get_handle does: anything
isHandleValid refuses (Handle.unallocated + offset) is INT32_MIN.

CPU tier: the logs regenerate to the fixture's SHA-256 and every witness holds on the reference's dump; the host core
(Replica::get_handles, the serial form, and handle_to_position_wave on one lane) under every profile's capacities
answers every query as the reference did; the new C ABI symbols are exported.
GPU tier: every profile's kernels, with the wave forms and the serial ones (MT_VAR_HANDLES_PARALLEL): all range queries
in one call with repeated and shuffled documents, guard words around `out` and between the windows, the size query, a
cap one short, every window against the per-position get_handle loop; handles_to_positions against the fixture and the
single call; handle_tables against the fixture and handle_table; the promoted document through its chain."""
import ctypes
import functools
import os

import numpy as np
import pytest

from fluidframework_amd import native
from fluidframework_amd import oplog as ol
import core_host
import hvec_logs as hl
from make_goldens_sha import log_sha
from test_ref_zamboni import caps_tuple, profile_caps

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = hl.cases()
NAMES = [c.name for c in CASES]
MT_E_CAPACITY, MT_E_ARG = 5, 16
MT_VAR_HANDLES_PARALLEL = 8
PROFILES = ("small", "matrix", "flat", "tiled")
GUARD = 0x5A5A5A5A
NONE = -(1 << 31)  # Handle.unallocated, what an unallocated position reads as


def fixture():
    return np.load(os.path.join(GOLDEN, "refhvec.npz"), allow_pickle=False)


@functools.lru_cache(maxsize=None)
def expected():
    """the fixture's queries and the reference's answers, once (shared, never changed): range queries (doc, start, end,
    None if the reference throws else the normalised handles), position queries (doc, handle, localSeq or None for the
    default argument, None if it throws else the position), and each document's table"""
    z = fixture()
    ro, raw = z["range_off"], z["range_handles"]
    rq = []
    for i, (d, a, b, t) in enumerate(zip(z["range_doc"], z["range_start"], z["range_end"], z["range_throws"])):
        h = raw[ro[i]: ro[i + 1]]
        rq.append((int(d), int(a), int(b), None if t else np.where(h >= 1, h, NONE).astype(np.int32)))
    hq = [(int(d), int(h), None if q < 0 else int(q), None if t else int(p)) for d, h, q, t, p in zip(
        z["pos_doc"], z["pos_handle"], z["pos_local_seq"], z["pos_throws"], z["pos_answers"])]
    to = z["table_off"]
    tables = [z["tables"][to[i]: to[i + 1]].astype(np.int32) for i in range(len(NAMES))]
    return rq, hq, tables


def ref_dump(d: int):
    z = fixture()
    return ol.parse_dump(z["dumps"][z["dump_off"][d]: z["dump_off"][d + 1]].tobytes())


def test_logs_regenerate_to_the_fixture():
    z = fixture()
    assert [str(n) for n in z["names"]] == NAMES
    assert log_sha(hl.batch(CASES)) == str(z["log_sha256"]), "tests/hvec_logs.py no longer builds the fixture's logs"
    rq, hq = hl.queries(CASES)
    erq, ehq, tables = expected()
    assert rq == [q[:3] for q in erq] and hq == [q[:3] for q in ehq] and len(tables) == len(CASES)
    assert os.path.getsize(os.path.join(GOLDEN, "refhvec.npz")) < (1 << 18)


def test_every_case_is_listed_and_witnessed():
    rq, hq, tables = expected()
    for d, c in enumerate(CASES):
        stem = c.name.rstrip("0123456789").rstrip("_") if c.name[-1].isdigit() else c.name
        assert c.branch and (c.name in hl.__doc__ or stem in hl.__doc__), c.name
        assert c.ranges and c.handles, c.name
        hdr, segs = ref_dump(d)
        assert c.witness(hdr, segs), c.name
        # the recorded answers are the dump's own rows: every in-range position's handle, and the valid shapes
        flat = np.concatenate([np.full(s["len"], NONE, np.int64) if s["start"] == NONE else s["start"] + np.arange(s["len"])
                               for s in segs if s["removedSeq"] is None] + [np.zeros(0, np.int64)])
        assert len(flat) == hdr["length"], c.name
        for q in (q for q in rq if q[0] == d):
            ok = 0 <= q[1] <= q[2] <= hdr["length"]
            assert (q[3] is not None) == ok, (c.name, q[:3])
            if ok:
                assert (q[3] == flat[q[1]: q[2]]).all(), (c.name, q[:3])
        for q in (q for q in hq if q[0] == d):
            if q[2] is not None and q[2] > hdr["localSeq"]:
                assert q[3] is None, (c.name, q)
        # a table is handles[0] = the free-list head, then 0 per allocated handle or the next free one
        held = sorted(s["start"] + k for s in segs if s["start"] != NONE for k in range(s["len"]))
        assert held == [i for i in range(1, len(tables[d])) if tables[d][i] == 0], c.name
    # the answers themselves show the branches
    d = NAMES.index("l_row4100")
    assert max(len(q[3]) for q in rq if q[0] == d and q[3] is not None) == 4109
    d = NAMES.index("f_realloc")
    got = {q[1]: q[3] for q in hq if q[0] == d}
    assert got[3] == 7 and got[4] == 2 and got[0] is None and got[9] is None
    d = NAMES.index("f_unlinked")
    assert {q[1]: q[3] for q in hq if q[0] == d}[3] is None
    d = NAMES.index("r_states")  # handles of removed rows are found; one past the current localSeq throws
    got = {(q[1], q[2]): q[3] for q in hq if q[0] == d}
    assert got[(5, None)] is not None and got[(9, None)] is not None and got[(9, 0)] != got[(9, None)]
    assert all(got[(h, 3)] is None for h in range(1, 15)) and got[(14, None)] is None
    d = NAMES.index("p_pending")
    got = {(q[1], q[2]): q[3] for q in hq if q[0] == d}
    assert len({got[(8, s)] for s in range(6)}) >= 4 and all(got[(h, 6)] is None for h in range(1, 11))
    assert sum(q[3] is None for q in rq) >= 40 and sum(q[3] is None for q in hq) >= 40
    # the throws that are the batched call's rule and not reference behaviour: exactly the reversed ranges and the empty
    # ranges outside [0, length]
    z = fixture()
    for q, t, rule in zip(rq, z["range_throws"], z["range_rule_throws"]):
        length = ref_dump(q[0])[0]["length"]
        assert bool(rule) == (q[2] < q[1] or (q[1] == q[2] and not 0 <= q[1] <= length)) and (t or not rule), q[:3]


def test_the_c_abi_exports_the_batched_matrix_reads():
    L = ctypes.CDLL(native.lib_path("libmtreplay.so"))
    for sym in ("mt_engine_get_handles", "mt_engine_handles_to_positions", "mt_engine_handle_tables"):
        assert hasattr(L, sym), sym
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "mt_engine.h")).read()
    assert "MT_VAR_HANDLES_PARALLEL = 8" in hdr and "handlecache.ts:69-83" in hdr and "permutationvector.ts:198-253" in hdr


def _host_lib():
    L = core_host.lib()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    L.mth_get_handles.argtypes = [vp, i64, i32, i32, vp, i64, vp]
    L.mth_get_handles.restype = i64
    L.mth_handle_to_position.argtypes = [vp, i64, i32, i32, vp]
    L.mth_handle_to_position.restype = i32
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("profile", PROFILES)
def test_host_core_answers_as_the_reference(profile):
    L = _host_lib()
    b = hl.batch(CASES)
    rq, hq, tables = expected()
    ran = 0
    for d, c in enumerate(CASES):
        assert profile in c.profiles
        st = core_host.HostStore(1, caps_tuple(profile_caps(profile)), pcap=hl.PCAP)
        st.start_collab(0, c.log.local_long_id)
        err = st.replay(0, *b.doc(d))
        if c.name in hl.PROMOTED and profile == "small":
            assert err == MT_E_CAPACITY, c.name  # the GPU tier answers it from the engine it is promoted to
            continue
        assert err == 0, (c.name, err, st.error_op(0))
        ran += 1
        cur = ref_dump(d)[0]["localSeq"]
        for q in (q for q in rq if q[0] == d):
            n = max(q[2] - q[1], 0)
            buf = np.full(n + 2, GUARD, np.int32)
            rc = ctypes.c_int32(-1)
            got = L.mth_get_handles(st.h, 0, q[1], q[2], _p(buf[1:]), n, ctypes.byref(rc))
            assert buf[0] == GUARD and buf[-1] == GUARD, (c.name, q[:3])
            if q[3] is None:
                assert rc.value == MT_E_ARG and got == 0 and (buf == GUARD).all(), (c.name, q[:3])
                continue
            assert rc.value == 0 and got == n and (buf[1:-1] == q[3]).all(), (c.name, q[:3])
            for k in range(q[1], q[2]):  # position for position the single read
                one = ctypes.c_int32(0)
                assert L.mth_get_handle(st.h, 0, k, ctypes.byref(one)) == 0 and one.value == q[3][k - q[1]]
            if n > 1:  # a window one short is never overrun
                buf[:] = GUARD
                assert L.mth_get_handles(st.h, 0, q[1], q[2], _p(buf[1:]), n - 1, ctypes.byref(rc)) == n
                assert (buf[1:n] == q[3][:-1]).all() and buf[n] == GUARD
        for q in (q for q in hq if q[0] == d):
            out = ctypes.c_int32(-7)
            rc = L.mth_handle_to_position(st.h, 0, q[1], cur if q[2] is None else q[2], ctypes.byref(out))
            assert rc == (MT_E_ARG if q[3] is None else 0), (c.name, q)
            if q[3] is not None:
                assert out.value == q[3], (c.name, q)
        t = np.zeros(len(tables[d]) + 1, np.int32)
        assert L.mth_handle_table(st.h, 0, _p(t), len(t)) == len(tables[d]) and (t[:-1] == tables[d]).all(), c.name
    assert ran >= len(CASES) - 1


# ---- GPU tier: one build per profile (an engine with pcap > 0 replays in its profile's client-feature kernel) ----
BUILDS = [("small", "small"), ("matrix", "matrix"), ("flat", "flat"), ("tiled", "tiled")]
BUILD_IDS = [b[0] for b in BUILDS]


@functools.lru_cache(maxsize=None)
def _engine(build_id):
    """one replayed engine per build, shared by the checks below (they only read)"""
    from fluidframework_amd.engine import Engine
    profile = dict(BUILDS)[build_id]
    b = hl.batch(CASES)
    eng = Engine(b.ndocs, **dict(profile_caps(profile), pcap=hl.PCAP))
    eng.start_collab(b.local_long_id)
    eng.replay(b)
    err, err_op = eng.errors()
    assert (err == 0).all(), [(CASES[i].name, int(err[i]), int(err_op[i])) for i in np.nonzero(err)[0]]
    want = [NAMES.index(n) for n in hl.PROMOTED] if profile == "small" else []
    assert sorted(int(x) for x in eng.promoted()) == want, build_id
    assert (eng.digests() == fixture()["digests"]).all(), build_id
    return eng


@functools.lru_cache(maxsize=None)
def _single(build_id):
    """mt_engine_get_handle for every position of every document of the build's engine, once (the single call does not
    depend on MT_VAR_HANDLES_PARALLEL): every window of every range query is a slice of its document's vector"""
    eng = _engine(build_id)
    return [np.asarray([eng.get_handle(d, p) for p in range(ref_dump(d)[0]["length"])], np.int32).reshape(-1)
            for d in range(len(CASES))]


def _raw_get_handles(eng, docs, starts, ends, out, cap):
    m = len(docs)
    off, st = np.zeros(m + 1, np.int64), np.full(m, -1, np.int32)
    n = eng.L.mt_engine_get_handles(eng.h, m, _p(docs), _p(starts), _p(ends), _p(off), _p(st),
                                    None if out is None else _p(out), cap)
    return n, off, st


@pytest.mark.gpu
@pytest.mark.parametrize("par", [1, 0], ids=["wave", "serial"])
@pytest.mark.parametrize("build_id", BUILD_IDS)
def test_gpu_get_handles(build_id, par):
    eng = _engine(build_id)
    eng.set_variant(MT_VAR_HANDLES_PARALLEL, par)
    rq, _, _ = expected()
    order = np.random.default_rng(11).permutation(len(rq))  # shuffled: documents repeat, in any order
    qs = [rq[i] for i in order]
    docs = np.asarray([q[0] for q in qs], np.int64)
    a, b = np.asarray([q[1] for q in qs], np.int32), np.asarray([q[2] for q in qs], np.int32)
    assert max(np.bincount(docs)) >= 10 and (np.diff(docs) < 0).any()
    want = [np.zeros(0, np.int32) if q[3] is None else q[3] for q in qs]
    total = sum(len(w) for w in want)
    # the size query
    n, off, st = _raw_get_handles(eng, docs, a, b, None, 0)
    assert n == total and (np.diff(off) == [len(w) for w in want]).all()
    assert (st == [MT_E_ARG if q[3] is None else 0 for q in qs]).all()
    # a cap one short writes nothing; the filled query equals the size query; guard words either side
    g = np.full(total + 2, GUARD, np.int32)
    n2, off2, st2 = _raw_get_handles(eng, docs, a, b, g[1:], total - 1)
    assert n2 == total and (g == GUARD).all() and (off2 == off).all() and (st2 == st).all()
    n2, off2, st2 = _raw_get_handles(eng, docs, a, b, g[1:], total)
    assert n2 == total and g[0] == GUARD and g[-1] == GUARD and (off2 == off).all() and (st2 == st).all()
    assert (g[1:-1] == np.concatenate(want)).all(), build_id
    # the binding
    off3, st3, hd = eng.get_handles(a, b, docs)
    assert (off3 == off).all() and (st3 == st).all() and (hd == g[1:-1]).all()
    # guard words between the windows: every query alone, a guard word either side of its window
    for i in range(len(qs)):
        w = len(want[i])
        g = np.full(w + 2, GUARD, np.int32)
        n1, _, s1 = _raw_get_handles(eng, docs[i:i + 1], a[i:i + 1], b[i:i + 1], g[1:], w)
        assert n1 == w and s1[0] == st[i] and g[0] == GUARD and g[-1] == GUARD and (g[1:-1] == want[i]).all(), qs[i][:3]
    # every window equals the per-position get_handle loop, position for position
    single = _single(build_id)
    for q, w in zip(qs, want):
        assert (single[q[0]][q[1]: q[1] + len(w)] == w).all() and len(w) == (0 if q[3] is None else q[2] - q[1]), (
            build_id, q[:3])
    # docs=None: every document once; m == 0 touches nothing
    L = np.asarray([ref_dump(d)[0]["length"] for d in range(len(CASES))], np.int32)
    off4, st4, hd4 = eng.get_handles(0, L)
    off5, st5, hd5 = eng.get_handles(np.zeros(len(L), np.int32), L, list(range(len(L))))
    assert (off4 == off5).all() and (hd4 == hd5).all() and not st4.any() and off4[-1] == L.sum()
    assert eng.L.mt_engine_get_handles(eng.h, 0, None, None, None, None, None, None, 0) == 0
    eng.set_variant(MT_VAR_HANDLES_PARALLEL, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("par", [1, 0], ids=["wave", "serial"])
@pytest.mark.parametrize("build_id", BUILD_IDS)
def test_gpu_handles_to_positions(build_id, par):
    from fluidframework_amd.engine import EngineError
    eng = _engine(build_id)
    eng.set_variant(MT_VAR_HANDLES_PARALLEL, par)
    _, hq, _ = expected()
    order = np.random.default_rng(12).permutation(len(hq))
    qs = [hq[i] for i in order]
    docs = [q[0] for q in qs]
    cur = [ref_dump(d)[0]["localSeq"] for d in range(len(CASES))]
    pos, st = eng.handles_to_positions([q[1] for q in qs], [cur[q[0]] if q[2] is None else q[2] for q in qs], docs)
    for q, p, s in zip(qs, pos, st):
        assert (int(s), int(p)) == ((MT_E_ARG, -1) if q[3] is None else (0, q[3])), (build_id, NAMES[q[0]], q)
    # the default argument: each replica's current localSeq
    dq = [q for q in qs if q[2] is None]
    pos2, st2 = eng.handles_to_positions([q[1] for q in dq], None, [q[0] for q in dq])
    assert [(int(s), int(p)) for p, s in zip(pos2, st2)] == [(MT_E_ARG, -1) if q[3] is None else (0, q[3]) for q in dq]
    # the single call
    for q in qs:
        try:
            got = eng.handle_to_position(q[0], q[1], cur[q[0]] if q[2] is None else q[2])
        except EngineError as e:
            assert e.code == MT_E_ARG
            got = None
        assert got == q[3], (build_id, q)
    eng.set_variant(MT_VAR_HANDLES_PARALLEL, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("build_id", BUILD_IDS)
def test_gpu_handle_tables(build_id):
    eng = _engine(build_id)
    _, _, tables = expected()
    docs = list(np.random.default_rng(13).permutation(len(CASES))) + [3, 3, 0]
    off, flat = eng.handle_tables(docs)
    assert off[-1] == len(flat) == sum(len(tables[d]) for d in docs)
    for i, d in enumerate(docs):
        assert (flat[off[i]: off[i + 1]] == tables[d]).all(), (build_id, NAMES[d])
    for d in (0, 3, len(CASES) - 1):
        assert (eng.handle_table(d) == tables[d]).all()
    off2, flat2 = eng.handle_tables()
    assert (flat2 == np.concatenate(tables)).all() and (np.diff(off2) == [len(t) for t in tables]).all()
    # a cap one short writes nothing; guard words either side
    d64 = np.asarray(docs, np.int64)
    o = np.zeros(len(docs) + 1, np.int64)
    g = np.full(len(flat) + 2, GUARD, np.int32)
    assert eng.L.mt_engine_handle_tables(eng.h, len(docs), _p(d64), _p(o), _p(g[1:]), len(flat) - 1) == len(flat)
    assert (g == GUARD).all() and (o == off).all()
    assert eng.L.mt_engine_handle_tables(eng.h, len(docs), _p(d64), _p(o), _p(g[1:]), len(flat)) == len(flat)
    assert g[0] == GUARD and g[-1] == GUARD and (g[1:-1] == flat).all()


@pytest.mark.gpu
def test_gpu_promoted_document_answers_through_its_chain():
    eng = _engine("small")
    k = NAMES.index(hl.PROMOTED[0])
    assert [int(x) for x in eng.promoted()] == [k]
    rq, hq, tables = expected()
    mixed = [q for q in rq if q[0] in (k, NAMES.index("i_inside"))]  # with a document of the small engine itself
    assert sum(q[0] == k for q in mixed) >= 6
    off, st, hd = eng.get_handles([q[1] for q in mixed], [q[2] for q in mixed], [q[0] for q in mixed])
    for i, q in enumerate(mixed):
        assert int(st[i]) == (MT_E_ARG if q[3] is None else 0), q[:3]
        assert (hd[off[i]: off[i + 1]] == (np.zeros(0, np.int32) if q[3] is None else q[3])).all(), q[:3]
    group = [q for q in hq if q[0] in (k, NAMES.index("z_merged"))]
    pos, st = eng.handles_to_positions([q[1] for q in group], None, [q[0] for q in group])
    assert [(int(s), int(p)) for p, s in zip(pos, st)] == [(MT_E_ARG, -1) if q[3] is None else (0, q[3]) for q in group]
    off, flat = eng.handle_tables([k, 0, k])
    assert (flat[off[0]: off[1]] == tables[k]).all() and (flat[off[2]: off[3]] == tables[k]).all()


@pytest.mark.gpu
def test_gpu_engine_without_handles_refuses():
    from fluidframework_amd.engine import Engine
    eng = Engine(2, **profile_caps("small"))
    one, z64 = np.zeros(2, np.int32), np.zeros(3, np.int64)
    assert eng.L.mt_engine_get_handles(eng.h, 2, None, _p(one), _p(one), _p(z64), _p(one), None, 0) == -MT_E_ARG
    assert eng.L.mt_engine_handles_to_positions(eng.h, 2, None, _p(one), None, _p(one), _p(one)) == MT_E_ARG
    assert eng.L.mt_engine_handle_tables(eng.h, 2, None, _p(z64), None, 0) == -MT_E_ARG
    eng.close()
