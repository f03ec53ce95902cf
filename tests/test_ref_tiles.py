"""Marker queries against the REFERENCE (tests/golden/reftiles.npz from tools/make_ref_goldens.py --tiles over
tests/tile_logs.py): Client.findTile and Client.getStackContext as the reference Client itself answered them after
replaying each hand-built log. The case list is the docstring of tests/tile_logs.py. Every comparison is exact.

CPU tier: the logs regenerate to the fixture's SHA-256 and every witness holds on the reference's dump; the host core
(Replica::find_tile / stack_context, the serial forms) under every profile's capacities answers every recorded query as
the reference did, and refuses exactly the k_mkmask document; Interner.values_containing agrees with a brute-force scan.
GPU tier: every kernel build, with the wave forms and the serial ones (MT_VAR_TILES_PARALLEL): all queries of a label in
one call (documents repeat, the tiled one too), the same queries split over two calls, docs=None, the promoted document
through its chain; statuses are MT_E_UNSUPPORTED exactly on the k_mkmask document; a too-small cap writes nothing; a
guard word either side of every stack window stays untouched."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

from fluidframework_amd import oplog as ol
import core_host
import tile_logs as tl
from make_goldens_sha import log_sha
from test_ref_zamboni import BUILDS, BUILD_IDS, caps_tuple, profile_caps

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = tl.cases()
NAMES = [c.name for c in CASES]
IT = tl.interner()
MT_E_UNSUPPORTED, MT_E_CAPACITY = 4, 5
MT_VAR_TILES_PARALLEL = 7
PROFILES = ("small", "matrix", "flat", "tiled")
GUARD = 0x5A5A5A5A


def fixture():
    return np.load(os.path.join(GOLDEN, "reftiles.npz"), allow_pickle=False)


@functools.lru_cache(maxsize=None)
def expected():
    """the fixture's queries and the reference's answers, once (shared, never changed): tile queries (doc, label, pos,
    preceding, (found, pos, index)), stack queries (doc, label, pos, [(index, refType)])"""
    z = fixture()
    tq = [(int(d), str(lb), int(p), bool(pre), tuple(int(x) for x in a)) for d, lb, p, pre, a in zip(
        z["tile_doc"], z["tile_label"], z["tile_pos"], z["tile_preceding"], z["tile_answers"])]
    so = z["stack_off"]
    sq = [(int(d), str(lb), int(p), [tuple(int(x) for x in e) for e in z["stack_entries"][so[i]: so[i + 1]]])
          for i, (d, lb, p) in enumerate(zip(z["stack_doc"], z["stack_label"], z["stack_pos"]))]
    return tq, sq


@functools.lru_cache(maxsize=None)
def ref_rows(d: int):
    """the reference's parsed dump of fixture document d (None where the fixture keeps no whole dump)"""
    z = fixture()
    keep = [int(x) for x in z["keep"]]
    if d not in keep:
        return None
    k = keep.index(d)
    return ol.parse_dump(z["dumps"][z["dump_off"][k]: z["dump_off"][k + 1]].tobytes())[1]


def test_logs_regenerate_to_the_fixture():
    z = fixture()
    assert [str(n) for n in z["names"]] == NAMES
    assert log_sha(tl.batch(CASES)) == str(z["log_sha256"]), "tests/tile_logs.py no longer builds the fixture's logs"
    tq, sq = tl.queries(CASES)
    etq, esq = expected()
    assert [(d, lb, -1 if p is None else p, pre) for d, lb, p, pre in tq] == [q[:4] for q in etq]
    assert [(d, lb, -1 if p is None else p) for d, lb, p in sq] == [q[:3] for q in esq]


def test_every_case_is_listed_and_witnessed():
    for d, c in enumerate(CASES):
        stem = c.name.rstrip("0123456789").rstrip("_") if c.name[-1].isdigit() else c.name
        assert c.branch and (c.name in tl.__doc__ or stem in tl.__doc__ or c.name == "p_empty"), c.name
        assert c.tiles or c.stacks, c.name
        rows = ref_rows(d)
        if rows is not None:
            z = fixture()
            k = [int(x) for x in z["keep"]].index(d)
            assert c.witness(*ol.parse_dump(z["dumps"][z["dump_off"][k]: z["dump_off"][k + 1]].tobytes())), c.name
    tq, sq = expected()
    # the answers themselves show the branches: tiles found in an earlier pass, a stack 70 deep, pushed ends
    d = NAMES.index("f_earlier_pass")
    assert [a for q in tq if q[0] == d for a in [q[4]]][:2] == [(1, 3, 3), (1, 95, 95)]
    d = NAMES.index("s_deep70")
    assert max(len(q[3]) for q in sq if q[0] == d) == 70 and [len(q[3]) for q in sq if q[0] == d][0] == 0
    d = NAMES.index("s_end_open")
    assert [len(q[3]) for q in sq if q[0] == d][0] == 2 and all(rt == tl.END for _, rt in [q[3] for q in sq if q[0] == d][0])
    for name in tl.REFUSED:
        assert name in NAMES


def test_values_containing_is_the_brute_force_scan():
    it = IT
    for label in ("pg", "row", "li", "q", "zz", "p", ""):
        bits = it.values_containing(label)
        assert bits.dtype == np.uint32 and bits.shape == (ol.LABEL_SET_WORDS,)
        want = {i for i, sv in enumerate(it.values) if i and isinstance(json.loads(sv), list) and label in json.loads(sv)}
        got = {32 * w + b for w in np.nonzero(bits)[0] for b in range(32) if (int(bits[w]) >> b) & 1}
        assert got == want, label
    assert IT.values_containing("pg").any() and not IT.values_containing("zz").any()
    # an array value that is not a label list, and a string equal to a label, do not count
    it2 = ol.Interner()
    a, b, c = it2.value(["x", "y"]), it2.value("x"), it2.value([["x"], 1])
    bits = it2.values_containing("x")
    assert {32 * w + k for w in np.nonzero(bits)[0] for k in range(32) if (int(bits[w]) >> k) & 1} == {a}
    assert b != a and c != a


def _host_lib():
    L = core_host.lib()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    L.mth_find_tile.argtypes = [vp, i64, i32, i32, i32, vp, vp]
    L.mth_stack_context.argtypes = [vp, i64, i32, i32, vp, vp, i32, vp]
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _key(label_kind):
    return IT.key_ids.get(ol.TILE_LABELS_KEY if label_kind == "tile" else ol.RANGE_LABELS_KEY, 0)


def _check_tile(name, q, found, pos, ordinal, ref_type):
    d, lb, p, pre, (efound, epos, eidx) = q
    what = (name, NAMES[d], lb, p, pre)
    assert bool(found) == bool(efound), what
    if efound:
        assert (pos, ordinal) == (epos, eidx), what
        rows = ref_rows(d)
        if rows is not None:
            assert ref_type == rows[eidx]["refType"] and ref_type & tl.TILE, what


def _check_stack(name, q, entries):
    d, lb, p, want = q
    what = (name, NAMES[d], lb, p)
    assert [(int(e["ordinal"]), int(e["ref_type"])) for e in entries] == want, what
    rows = ref_rows(d)
    if rows is not None:  # the positions: the local lengths in front of each marker
        for e in entries:
            before = sum(r["len"] for r in rows[: int(e["ordinal"])] if r["removedSeq"] is None)
            assert int(e["pos"]) == before, what


@pytest.mark.parametrize("profile", PROFILES)
def test_host_core_answers_as_the_reference(profile):
    L = _host_lib()
    b = tl.batch(CASES)
    tq, sq = expected()
    sets = {lb: np.ascontiguousarray(IT.values_containing(lb)) for lb in {q[1] for q in tq} | {q[1] for q in sq}}
    ran = 0
    for d, c in enumerate(CASES):
        if profile not in c.profiles:
            continue
        st = core_host.HostStore(1, caps_tuple(profile_caps(profile)))
        st.start_collab(0, c.log.local_long_id)
        err = st.replay(0, *b.doc(d))
        if c.name in tl.PROMOTED and profile == "small":
            assert err == MT_E_CAPACITY, c.name  # the GPU tier answers it from the engine it is promoted to
            continue
        assert err == 0, (c.name, err, st.error_op(0))
        ran += 1
        refused = c.name in tl.REFUSED
        for q in (q for q in tq if q[0] == d):
            out = np.zeros(5, np.int32)
            rc = L.mth_find_tile(st.h, 0, q[2], int(q[3]), _key("tile"), _p(sets[q[1]]), _p(out))
            if refused:
                assert rc == 2 and out[0] == -1, (c.name, q)
                continue
            assert rc in (0, 1) and (rc == 1) == (out[0] >= 0), (c.name, q)
            _check_tile(profile, q, rc == 1, int(out[3]), int(out[2]), int(out[4]))
        for q in (q for q in sq if q[0] == d):
            dh = np.zeros(2, np.int32)
            rc = L.mth_stack_context(st.h, 0, q[2], _key("range"), _p(sets[q[1]]), None, 0, _p(dh))
            if refused:
                assert rc == 2 and not dh.any(), (c.name, q)
                continue
            assert len(q[3]) == dh[0] <= dh[1], (c.name, q, dh)
            buf = np.full((int(dh[1]) + 2) * 5, GUARD, np.int32)
            dh2 = np.zeros(2, np.int32)
            L.mth_stack_context(st.h, 0, q[2], _key("range"), _p(sets[q[1]]), _p(buf[5:]), int(dh[1]), _p(dh2))
            assert (dh2 == dh).all() and (buf[:5] == GUARD).all() and (buf[-5:] == GUARD).all(), (c.name, q)
            _check_stack(profile, q, buf[5:5 + 5 * int(dh[0])].view(ol.TILE_REF))
            if dh[1] > 1:  # a window one entry short is never overrun
                buf[:] = GUARD
                L.mth_stack_context(st.h, 0, q[2], _key("range"), _p(sets[q[1]]), _p(buf[5:]), int(dh[1]) - 1, _p(dh2))
                assert (dh2 == dh).all() and (buf[5 * int(dh[1]):] == GUARD).all(), (c.name, q)
    assert ran >= (len(CASES) - 2 if profile in ("flat", "tiled") else 20)
    d = NAMES.index("s_deep70")
    assert profile not in CASES[d].profiles or ran  # the deepest stack ran under this profile


# ---- GPU tier ----
def _gpu_cases(profile, perm_only):
    idx = [i for i, c in enumerate(CASES) if profile in c.profiles and (not perm_only or c.kind == "perm")]
    return idx, [CASES[i] for i in idx]


@functools.lru_cache(maxsize=None)
def _engine(build_id):
    """one replayed engine per build, shared by the checks below (they only read)"""
    from fluidframework_amd.engine import Engine
    name, profile, variant, perm_only = BUILDS[BUILD_IDS.index(build_id)]
    idx, cs = _gpu_cases(profile, perm_only)
    b = tl.batch(cs)
    eng = Engine(b.ndocs, **variant, **profile_caps(profile))
    eng.start_collab(b.local_long_id)
    eng.replay(b)
    err, err_op = eng.errors()
    assert (err == 0).all(), [(cs[i].name, int(err[i]), int(err_op[i])) for i in np.nonzero(err)[0]]
    want = [k for k, c in enumerate(cs) if c.name in tl.PROMOTED and name.startswith("small")]
    assert sorted(int(x) for x in eng.promoted()) == want, name
    z = fixture()
    assert (eng.digests() == z["digests"][idx]).all(), name
    return eng, idx, cs


def _by_label(qs, idx):
    """the fixture's queries on the build's documents, grouped by label (a call carries one label): label ->
    [(engine doc, query)]"""
    out = {}
    for q in qs:
        if q[0] in idx:
            out.setdefault(q[1], []).append((idx.index(q[0]), q))
    return out


def _find(eng, label, group):
    pos = [q[2] for _, q in group]
    return eng.find_tiles(label, [k for k, _ in group], pos, [q[3] for _, q in group], interner=IT)


def _check_find(name, cs, group, tiles, st):
    for (k, q), t, s in zip(group, tiles, st):
        refused = cs[k].name in tl.REFUSED
        assert int(s) == (MT_E_UNSUPPORTED if refused else 0), (name, cs[k].name, q)
        if refused:
            assert t["rid"] == -1, (name, q)
        else:
            _check_tile(name, q, t["rid"] >= 0, int(t["pos"]), int(t["ordinal"]), int(t["ref_type"]))


@pytest.mark.gpu
@pytest.mark.parametrize("par", [1, 0], ids=["wave", "serial"])
@pytest.mark.parametrize("build_id", BUILD_IDS)
def test_gpu_find_tiles(build_id, par):
    eng, idx, cs = _engine(build_id)
    profile = BUILDS[BUILD_IDS.index(build_id)][1]
    eng.set_variant(MT_VAR_TILES_PARALLEL, par)
    tq, _ = expected()
    groups = _by_label(tq, idx)
    assert "pg" in groups
    for label, group in groups.items():
        # one call: documents repeat (every case names its document several times; the tiled one too)
        docs = [k for k, _ in group]
        if label == "pg" and profile != "matrix":  # a document named three times or more in one call; the tiled one too
            kt = [c.name for c in cs].index("x_tiled_chunks")
            assert docs.count(kt) >= 3 and docs.count([c.name for c in cs].index("f_same_leaf")) >= 3, build_id
        tiles, st = _find(eng, label, group)
        _check_find(build_id, cs, group, tiles, st)
        # the handles are the rows' own
        for (k, q), t in list(zip(group, tiles))[:6]:
            if t["rid"] >= 0:
                ids = eng.segment_ids(k)
                assert tuple(int(x) for x in ids[int(t["ordinal"])]) == (int(t["rid"]), int(t["gen"]))
        # the same queries split over two calls
        h = len(group) // 2
        for part in (group[:h], group[h:]):
            if part:
                _check_find(build_id + " split", cs, part, *_find(eng, label, part))
    # docs=None: every document once, pos undefined; equal to naming them, and to the fixture where it asks that
    for pre in (True, False):
        t0, s0 = eng.find_tiles("pg", None, None, pre, interner=IT)
        t1, s1 = eng.find_tiles("pg", list(range(len(cs))), [None] * len(cs), pre, interner=IT)
        assert t0.tobytes() == t1.tobytes() and (s0 == s1).all() and len(t0) == len(cs)
        hit = 0
        for k, q in groups["pg"]:
            if q[2] == -1 and q[3] == pre:
                _check_find(build_id + " docs=None", cs, [(k, q)], t0[k:k + 1], s0[k:k + 1])
                hit += 1
        assert hit or build_id == "matrix"
    assert {cs[k].name for k in range(len(cs)) if eng.find_tiles("pg", [k], None, interner=IT)[1][0]} == (
        set(tl.REFUSED) & {c.name for c in cs})
    eng.set_variant(MT_VAR_TILES_PARALLEL, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("par", [1, 0], ids=["wave", "serial"])
@pytest.mark.parametrize("build_id", BUILD_IDS)
def test_gpu_stack_contexts(build_id, par):
    eng, idx, cs = _engine(build_id)
    eng.set_variant(MT_VAR_TILES_PARALLEL, par)
    _, sq = expected()
    groups = _by_label(sq, idx)
    assert "li" in groups
    kid = IT.key_ids[ol.RANGE_LABELS_KEY]
    for label, group in groups.items():
        docs = [k for k, _ in group]
        pos = [q[2] for _, q in group]
        buf, off, cnt, st = eng.stack_contexts_raw(label, docs, pos, interner=IT)
        assert len(buf) == off[-1] and (np.diff(off) >= cnt).all()
        for i, (k, q) in enumerate(group):
            refused = cs[k].name in tl.REFUSED
            assert int(st[i]) == (MT_E_UNSUPPORTED if refused else 0), (build_id, cs[k].name, q)
            if refused:
                assert cnt[i] == 0 and off[i + 1] == off[i]
            else:
                _check_stack(build_id, q, buf[off[i]: off[i] + cnt[i]])
        stacks, st2 = eng.stack_contexts(label, docs, pos, interner=IT)
        assert (st2 == st).all() and [s.tobytes() for s in stacks] == [
            buf[off[i]: off[i] + cnt[i]].tobytes() for i in range(len(group))]
        # split over two calls
        h = len(group) // 2
        for part in (group[:h], group[h:]):
            if part:
                ss, _ = eng.stack_contexts(label, [k for k, _ in part], [q[2] for _, q in part], interner=IT)
                for (k, q), s in zip(part, ss):
                    if cs[k].name not in tl.REFUSED:
                        _check_stack(build_id + " split", q, s)
        # a too-small cap writes nothing; guard entries either side of the buffer and of every window
        bits = np.ascontiguousarray(IT.values_containing(label))
        m = len(group)
        d64, p32 = np.asarray(docs, np.int64), np.asarray(pos, np.int32)
        total = int(off[-1])

        def call(dd, pp, n, out, cap):
            o, c, s = np.zeros(n + 1, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int32)
            r = eng.L.mt_engine_stack_contexts(eng.h, n, _p(dd), _p(pp), kid, _p(bits), _p(o), _p(c), _p(s),
                                               None if out is None else _p(out), cap)
            return r, o, c
        if total:
            g = np.full(5 * (total + 2), GUARD, np.int32)
            r, o, c = call(d64, p32, m, g[5:], total - 1)
            assert r == total and (g == GUARD).all() and (o == off).all() and (c == cnt).all()
            r, o, c = call(d64, p32, m, g[5:], total)
            assert r == total and (g[:5] == GUARD).all() and (g[-5:] == GUARD).all()
            assert all(g[5 + 5 * off[i]: 5 + 5 * (off[i] + cnt[i])].tobytes() == buf[off[i]: off[i] + cnt[i]].tobytes()
                       for i in range(m))
        for i in range(m):  # every window alone, a guard entry either side
            w = int(off[i + 1] - off[i])
            if not w:
                continue
            g = np.full(5 * (w + 2), GUARD, np.int32)
            r, o, c = call(d64[i:i + 1], p32[i:i + 1], 1, g[5:], w)
            assert r == w and c[0] == cnt[i] and (g[:5] == GUARD).all() and (g[-5:] == GUARD).all(), (build_id, group[i])
            assert g[5: 5 + 5 * int(cnt[i])].tobytes() == buf[off[i]: off[i] + cnt[i]].tobytes()
    # docs=None
    s0, st0 = eng.stack_contexts("li", None, None, interner=IT)
    s1, st1 = eng.stack_contexts("li", list(range(len(cs))), [None] * len(cs), interner=IT)
    assert [a.tobytes() for a in s0] == [a.tobytes() for a in s1] and (st0 == st1).all() and len(s0) == len(cs)
    for k, q in groups["li"]:
        if q[2] == -1 and cs[k].name not in tl.REFUSED:
            _check_stack(build_id + " docs=None", q, s0[k])
    eng.set_variant(MT_VAR_TILES_PARALLEL, 1)


@pytest.mark.gpu
def test_gpu_promoted_document_answers_through_its_chain():
    eng, idx, cs = _engine("small-waves8")
    k = [c.name for c in cs].index(tl.PROMOTED[0])
    assert [int(x) for x in eng.promoted()] == [k]
    tq, sq = expected()
    group = [(k, q) for q in tq if q[0] == idx[k]]
    assert len(group) >= 6
    mixed = group + [(0, q) for q in tq if q[0] == idx[0] and q[1] == "pg"]  # with a document of the small engine itself
    _check_find("promoted", cs, mixed, *_find(eng, "pg", mixed))
    for _, q in ((k, q) for q in sq if q[0] == idx[k]):
        _check_stack("promoted", q, eng.stack_contexts("li", [k], [q[2]], interner=IT)[0][0])
