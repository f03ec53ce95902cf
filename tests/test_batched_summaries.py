"""Batched summaries (include/mt_engine.h mt_engine_summaries): the summary dump (include/mt_oplog.h) of many documents
from one size launch and one fill launch: SnapshotV1.extractSync / SnapshotLegacy.extractSync done on the device.

CPU tier: the header and the export; a property test of the extraction rule (the summary format is a fixed point of
extract_segments; the closed-form length rule of Replica::summary_wave equals the greedy walk); the host core's
summary against snapshot.extract_segments of its own dump and against the REFERENCE's SnapshotV1 / legacy tree hashes;
hand-built documents have the shapes they are named for. GPU tier, under both writers (MT_VAR_SUMMARIES_PARALLEL): the
reference's hashes through Engine.summaries, promoted documents, the tiled profile, sizing and arguments,
snapshot.emit_batch(device=True), and the hand-built writer edges on both window alignments."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from fluidframework_amd import gen, native
from fluidframework_amd import oplog as ol
from fluidframework_amd import snapshot as sn
import core_host
import promotion_mix as pm
import summary_docs as sd
import test_legacy_ref as lr
import test_ref_goldens as rg
import test_snapshot_ref as sr
from test_batched_reads import _doc_lists, _engine
from test_ref_zamboni import caps_tuple, profile_caps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MT_E_ARG = 16
MT_VAR_SUMMARIES_PARALLEL = 6
WRITERS = [1, 0]
V1, LEGACY = sd.V1, sd.LEGACY
REF_SETS = list(sr.SETS)  # the ref_* sets (c4_large: the tiled profile) and "snap_body" (refsnap_body.npz)


# ---- A.1 header and export --------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mt_engine.h")).read(), flags=re.S)


def test_header_declares_and_library_exports_the_batched_summaries():
    lib = native.build_replay()
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    assert re.search(r"\bmt_engine_summaries\s*\(", _header()), "mt_engine_summaries is not declared"
    assert "mt_engine_summaries" in exported, "mt_engine_summaries is not exported"
    enums = re.findall(r"enum\s*\{([^}]*)\}", _header())
    assert any(re.search(r"\bMT_VAR_SUMMARIES_PARALLEL\s*=\s*6\b", e) and "MT_VAR_DUMPS_PARALLEL" in e for e in enums)


# ---- A.2 the rule, in pure Python -------------------------------------------------------------------------------
LENS = (1, 2, 127, 128, 129, 255, 256, 257, 300)


def _rand_rows(rng, run_doc):
    """a parsed-dump row list: settled members of two property sets, newline ends, markers, elided and window rows"""
    segs = []
    for _ in range(rng.randint(0, 14)):
        r = rng.random()
        n = rng.choice(LENS)
        s = dict(kind=ol.SEG_RUN if run_doc else ol.SEG_TEXT, flags=0, len=n, seq=0, client=0, removedSeq=None,
                 removedClient=None, overlap=[], props=[], refType=0, text=None, items=None)
        if r < 0.1:
            s.update(kind=ol.SEG_MARKER, len=1, refType=rng.randint(0, 2))
        else:
            if run_doc:
                s["items"] = [rng.choice((10, 11))] * n
            else:
                s["text"] = "t" * (n - 1) + ("\n" if rng.random() < 0.15 else "u")
            if r < 0.2:
                s["seq"] = -1                       # unacked: elided
            elif r < 0.3:
                s.update(removedSeq=3, removedClient=1, flags=ol.DF_REMOVED)   # removed at or below the MSN: elided
            elif r < 0.4:
                s.update(seq=9, client=2)           # a window insert
            elif r < 0.45:
                s.update(removedSeq=8, removedClient=1, flags=ol.DF_REMOVED)   # removed above the MSN: a window row
        if rng.random() < 0.25:
            s["flags"] |= ol.DF_HAS_PROPS
            s["props"] = [(1, 5)]
        segs.append(s)
    return dict(minSeq=5, currentSeq=9), segs


def _as_records(hdr, segs):
    """the segments extract_segments yields from `segs`, as the summary dump's records (mt_oplog.h): a settled run has
    seq 0, client -1 and no removal; a window row keeps its own"""
    out, prev = [], None
    for s in segs:
        removed = s["removedSeq"] is not None
        if s["seq"] == -1 or (removed and s["removedSeq"] <= hdr["minSeq"]):
            continue
        if s["seq"] <= hdr["minSeq"] and not removed:
            if prev is not None and sn._can_append(prev, s) and sn._match_props(prev, s):
                prev = sn._appended(prev, s)
                out[-1] = prev
            else:
                prev = dict(s, seq=0, client=-1)
                out.append(prev)
        else:
            prev = None
            out.append(dict(s, overlap=[]))
    return out


def _closed_form_heads(segs, G):
    """Replica::summary_wave's length rule over member rows that all pair (one chain): a long row starts a run iff an
    earlier long row exists in the chain or the chain before it is longer than G"""
    heads, pre, seen = [], 0, False
    for i, n in enumerate(segs):
        lng = n > G
        heads.append(i == 0 or (lng and (seen or pre > G)))
        pre += n
        seen |= lng
    return heads


def _greedy_heads(segs, G):
    heads, run = [], 0
    for i, n in enumerate(segs):
        h = i == 0 or not (run <= G or n <= G)
        run = n if h else run + n
        heads.append(h)
    return heads


def test_summary_format_is_a_fixed_point_and_the_closed_form_is_the_greedy_walk():
    rng = random.Random(20240611)
    it = ol.Interner()
    it.key("k0"), it.key("k1")
    for v in range(8):
        it.value(v)
    for i in range(13):
        it.item({"i": i})
    merged = 0
    for case in range(3000):
        hdr, segs = _rand_rows(rng, run_doc=case % 3 == 0)
        want = sn.extract_segments(hdr, segs, it, sr.long_name)
        recs = _as_records(hdr, segs)
        assert sn.extract_segments(hdr, recs, it, sr.long_name) == want
        assert sn.specs_from_summary(hdr, recs, it, sr.long_name) == want
        merged += len(segs) - len(want)
    assert merged > 3000
    for case in range(3000):
        G = (256, 128)[case % 2]
        chain = [rng.choice(LENS) for _ in range(rng.randint(1, 12))]
        assert _closed_form_heads(chain, G) == _greedy_heads(chain, G), (G, chain)


def _passes_heads(chain, G, cuts):
    """Replica::summary_wave's length rule with the chain cut into passes at `cuts`: a pass sees the rows before it only
    as the open run's grown length cR (the chain-continues branch: pre = E + cR, seen = a long row earlier in the
    pass or cR > G), and leaves the length of its last run behind"""
    heads, cR, start = [], 0, 0
    for end in list(cuts) + [len(chain)]:
        rows = chain[start:end]
        first = start == 0
        h = []
        for i, n in enumerate(rows):
            lng = n > G
            before = rows[:i]
            ch = max([j for j in range(i + 1) if first and j == 0], default=-1)  # the chain head, if in this pass
            if ch >= 0:
                pre, seen = sum(before), any(x > G for x in before)
            else:
                pre, seen = sum(before) + cR, any(x > G for x in before) or cR > G
            h.append((first and i == 0) or (lng and (seen or pre > G)))
        # the run the pass leaves open: from its last head on, or the carried run grown by the whole pass
        if rows:
            if any(h):
                last = max(j for j, x in enumerate(h) if x)
                cR = sum(rows[last:])
            else:
                cR += sum(rows)
        heads += h
        start = end
    return heads


def test_closed_form_with_a_carried_run_is_the_greedy_walk():
    rng = random.Random(77)
    carried = 0
    for case in range(4000):
        G = (256, 128)[case % 2]
        chain = [rng.choice(LENS) for _ in range(rng.randint(1, 14))]
        cuts = sorted(rng.sample(range(1, len(chain)), rng.randint(0, min(3, len(chain) - 1)))) if len(chain) > 1 else []
        assert _passes_heads(chain, G, cuts) == _greedy_heads(chain, G), (G, chain, cuts)
        carried += bool(cuts)
    assert carried > 2000


# ---- A.5 census of the reference's kept dumps --------------------------------------------------------------------
# per fixture file: (dumps, rows kept, segments emitted, runs that span two leaves, runs of more than 64 rows), by
# snapshot.extract_segments' rule over the reference's own final dumps. No generator set has a run of more than 64
# rows (the last column is zero everywhere): the hand-built documents carry that branch, and their census asserts it.
CENSUS = {
    "ref_c1_farm.npz": (4, 621, 621, 0, 0),
    "ref_c2_full.npz": (1, 416, 398, 8, 0),
    "ref_c2_observer.npz": (4, 250, 238, 4, 0),
    "ref_c3_lagged.npz": (4, 872, 767, 41, 0),
    "ref_c3_lagged_long.npz": (4, 862, 769, 39, 0),
    "ref_c4_scaled.npz": (4, 35361, 35261, 25, 0),
    "ref_c5_perm.npz": (4, 2689, 2551, 64, 0),
    "refcombine.npz": (4, 1736, 1634, 42, 0),
    "refsess_c2_sessions.npz": (2, 74, 73, 1, 0),
    "refsess_c3_sessions.npz": (2, 563, 488, 26, 0),
    "refsess_c4_sessions.npz": (2, 17005, 16960, 14, 0),
    "refsess_c5_sessions.npz": (2, 1286, 1222, 30, 0),
    "refsubseq_c2_observer.npz": (4, 250, 238, 4, 0),
    "refsubseq_c3_lagged.npz": (4, 872, 767, 41, 0),
    "refsubseq_c4_scaled.npz": (4, 35361, 35261, 25, 0),
}


def test_census_of_the_reference_dumps():
    from test_batched_dumps import _golden_keep_dumps
    got = {}
    for name, raw in _golden_keep_dumps():
        t = got.setdefault(name.split(":")[0], [0, 0, 0, 0, 0])
        t[0] += 1
        for i, x in enumerate(sd.census(*ol.parse_dump(raw))):
            t[i + 1] += x
    assert {k: tuple(v) for k, v in got.items()} == CENSUS
    assert all(v[4] == 0 for v in CENSUS.values()) and sum(v[3] for v in CENSUS.values()) > 300


def test_census_of_the_hand_built_documents():
    ds, b, st, sums = _edge()
    got = {doc.name: sd.census(*ol.parse_dump(st.dump(d))) for d, doc in enumerate(ds)}
    assert got["ones_65"][3] == 1 and got["ones_129"][3] == 1 and got["ones_64"][3] == 0  # runs of more than 64 rows
    assert all(got[f"ones_{n}"][2] >= 1 for n in (63, 64, 65, 129))                      # and across leaves
    assert got["ones_129"][:2] == (sd.PRE + 130, sd.PRE + 2)
    assert got["tombstones_70_between"][0] == sd.PRE + 3 and got["tombstones_70_between"][2] == 1


# ---- A.3 / A.4 the host core ------------------------------------------------------------------------------------
def _check_host(st, d, it, sha=None, legacy_too=True):
    """document d of a host store: its summary dumps against extract_segments of its dump; returns the v1 specs"""
    hdr, segs = ol.parse_dump(st.dump(d))
    specs = None
    for mode in (V1, LEGACY) if legacy_too else (V1,):
        raw = sd.host_summary(st, d, mode)
        sh, ss = ol.parse_dump(raw)
        got = sn.specs_from_summary(sh, ss, it, sr.long_name)
        want = sn.extract_segments(hdr, segs, it, sr.long_name) if mode == V1 else sn.extract_segments_legacy(hdr, segs, it)
        assert got == want, (d, mode)
        assert sh["nsegs"] == len(got) and sh["nleaf"] == 0
        assert {k: sh[k] for k in ("currentSeq", "minSeq")} == {k: hdr[k] for k in ("currentSeq", "minSeq")}
        assert len(raw) == 24 + sum(sd.record_size(s) for s in ss), (d, mode)
        assert all(not s["overlap"] and s["leaf"] == 0 for s in ss)
        if mode == V1:
            specs = got
            if sha is not None:
                assert sr.sha(sn.emit_v1(sh, None, it, sr.long_name, specs=got)) == sha, d
    return specs


@pytest.mark.parametrize("name", REF_SETS)
def test_host_core_summary_matches_reference(name):
    z, b, it, c = sr.fixture(name)
    assert sr.has_snapshots(z)
    st = core_host.HostStore(b.ndocs, caps_tuple(c))
    for d in range(b.ndocs):
        st.start_collab(d, int(b.local_long_id[d]))
        assert st.replay(d, *sr.prefix_arrays(b, d, int(z["snap_cut"][d]))) == 0
        _check_host(st, d, it, str(z["snap_sha256"][d]))


def _families():
    import test_ref_inserts as ti
    import test_ref_props as tp
    import test_ref_ranges as tr
    import test_ref_zamboni as tz
    return {"refzamboni": (tz, None), "refranges": (tr, None), "refinserts": (ti, None), "refprops": (tp, tp.KINDS)}


@pytest.mark.parametrize("family", ["refzamboni", "refranges", "refinserts", "refprops"])
def test_host_core_summary_matches_reference_hand_built_logs(family):
    mod, kinds = _families()[family]
    z = mod.fixture()
    idx, cs = mod.fitting("flat")
    assert len(idx) > 20
    for at in range(0, len(idx), 64):
        part = cs[at: at + 64]
        _, err, st = core_host.replay_batch(ol.Batch.from_logs([c.log for c in part]), caps_tuple(profile_caps("flat")),
                                            kinds=kinds)
        assert (err == 0).all()
        for k, c in enumerate(part):
            _check_host(st, k, c.log.interner, str(z["snap_sha256"][idx[at + k]]))


def _subseq_names():
    import test_ref_subseq as rs
    return rs.NAMES


@pytest.mark.parametrize("name", _subseq_names())
def test_host_core_summary_matches_reference_item_rows(name):
    import test_ref_subseq as rs
    z, w, b = rs.regenerate(name)
    it = rs.item_interner()
    st = core_host.HostStore(b.ndocs, caps_tuple(rg.caps_for(w)))
    for d in range(b.ndocs):
        st.start_collab(d, int(b.local_long_id[d]))
        assert st.replay(d, *sr.prefix_arrays(b, d, int(z["snap_cut"][d]))) == 0
        _check_host(st, d, it, str(z["snap_sha256"][d]))


@pytest.mark.parametrize("name", lr.NAMES)
def test_host_core_legacy_summary_matches_reference(name):
    z, w, b = lr.fixture(name)
    it = gen.generator_interner()
    st = core_host.HostStore(b.ndocs, caps_tuple(rg.caps_for(w)), dcap=lr.DCAP)
    done = 0
    for d in range(b.ndocs):
        st.start_collab(d, int(b.local_long_id[d]))
        assert st.replay(d, *lr.prefix(b, d, int(z["cut"][d]))) == 0
        if z["emit_error"][d]:
            continue
        _, _h, words = st.deltas(d)
        sh, ss = ol.parse_dump(sd.host_summary(st, d, LEGACY))
        ops, text, props, kv = lr.prefix(b, d, int(z["cut"][d]))
        msgs = sn.catchup_messages(ops, text, props, kv, words, it, sr.long_name, sh["minSeq"])
        tree = sn.emit_legacy(sh, None, it, msgs, specs=sn.specs_from_summary(sh, ss, it, sr.long_name))
        assert sr.sha(tree) == str(z["sha256"][d]), d
        done += 1
    assert done > 0


def _hsnap_prefixes():
    """the handle-summary fixture: (fixture, caps dict, caps, prefix batch, the reference's trees)"""
    import test_ref_hsnap as hs
    z, c, caps, b, trees = hs.load()
    pre = []
    for d in range(b.ndocs):
        ops, text, props, kv = b.doc_arrays(d)
        pre.append((ops[:int(z["cuts"][d])], text, props, kv))
    return hs, c, caps, ol.Batch.from_arrays(pre, b.local_long_id), trees


def test_host_core_summary_matches_reference_handle_summaries():
    """refhsnap_c5_perm stores the reference's trees themselves (PermutationSegment specs with allocated starts)"""
    hs, c, caps, pre, trees = _hsnap_prefixes()
    it = gen.generator_interner()
    _, err, st = core_host.replay_batch(pre, caps, pcap=hs.PCAP)
    assert (err == 0).all()
    for d in range(pre.ndocs):
        _check_host(st, d, it, sr.sha(trees[d]))


def test_handle_documents_have_the_shapes_they_are_named_for():
    ds = sd.handle_docs()
    _, err, st = core_host.replay_batch(sd.batch(ds), pcap=1 << 10)
    assert (err == 0).all()
    for d, doc in enumerate(ds[:2]):
        _check_host(st, d, doc.log.interner)
        segs = ol.parse_dump(st.dump(d))[1]
        assert [s["len"] for s in segs[sd.PRE:-1]] == [1, 1, 2] and all(s["flags"] & ol.DF_HANDLE for s in segs[sd.PRE:sd.PRE + 2])
        a, bb = segs[sd.PRE]["start"], segs[sd.PRE + 1]["start"]
        assert (bb == a + 1) == (doc.name == "handles_follow")
        ss = ol.parse_dump(sd.host_summary(st, d, V1))[1]
        assert [s["len"] for s in ss[sd.PRE:-1]] == doc.want, doc.name


# ---- D (CPU half): the hand-built documents ---------------------------------------------------------------------
_EDGE = {}


def _edge():
    """(documents, batch, host store, per document and mode the host core's summary)"""
    if not _EDGE:
        ds = sd.docs()
        b0 = sd.batch(ds)
        _, err, st = core_host.replay_batch(b0)
        assert (err == 0).all(), err
        for n in (63, 64, 65, 129):  # the same with a newline ending the first pass, and a marker starting the second
            plain = next(i for i, d in enumerate(ds) if d.name == f"ones_{n}")
            body = ol.parse_dump(st.dump(plain))[1][sd.PRE:]
            ds += sd.nl_and_marker_variants(n, lambda i: body[i]["leaf"])
        b = sd.batch(ds)
        _, err, st = core_host.replay_batch(b)
        assert (err == 0).all(), err
        _EDGE["v"] = (ds, b, st, [[sd.host_summary(st, d, m) for m in (V1, LEGACY)] for d in range(b.ndocs)])
    return _EDGE["v"]


def test_edge_documents_have_the_shapes_they_are_named_for():
    ds, b, st, sums = _edge()
    it = ds[0].log.interner
    spans = {}
    for d, doc in enumerate(ds):
        hdr, segs = ol.parse_dump(st.dump(d))
        inserts = sum(1 for r in doc.log.ops if (r[0] & 7) == ol.OP_INSERT)  # no insert here splits a row
        assert hdr["nsegs"] == inserts, (doc.name, "zamboni merged or unlinked rows")  # still separate
        _check_host(st, d, it)
        sh, ss = ol.parse_dump(sums[d][V1])
        if doc.want is not None:
            body = [s["len"] for s in ss[sd.PRE if doc.name not in ("empty", "one_row") else 0:]]
            assert body[:len(doc.want)] == doc.want, (doc.name, body)
        # the passes (8 leaves) the longest settled run spans, from the dump's leaf ordinals
        live = [s for s in segs if s["seq"] != -1 and not (s["removedSeq"] is not None and s["removedSeq"] <= hdr["minSeq"])]
        spans[doc.name] = len({s["leaf"] // 8 for s in live[sd.PRE:-1]}) if len(live) > sd.PRE + 1 else 0
    assert spans["ones_63"] >= 2 and spans["ones_129"] >= 3 and spans["tombstones_70_between"] >= 1
    assert len(sums[0][V1]) == 24 and len(sums[1][V1]) == 66
    by = {doc.name: d for d, doc in enumerate(ds)}
    d = by["local_pending_removal"]
    assert [s["len"] for s in ol.parse_dump(sums[d][LEGACY])[1][sd.PRE:]] == [12]
    d = by["removed_above_msn_between"]
    mid = ol.parse_dump(sums[d][V1])[1][sd.PRE + 1]
    assert mid["removedSeq"] == hdr_min(sums[d][V1]) + 1 and mid["flags"] & ol.DF_REMOVED
    # a whole pass of tombstones lies between the two rows of the one run
    hdr, segs = ol.parse_dump(st.dump(by["tombstones_70_between"]))
    gone = [s["leaf"] // 8 for s in segs if s["removedSeq"] is not None]
    assert len(gone) == 70 and any(gone.count(p) == sum(1 for s in segs if s["leaf"] // 8 == p) for p in set(gone))


def hdr_min(raw):
    return ol.parse_dump(raw)[0]["minSeq"]


# ---- helpers (GPU) ----------------------------------------------------------------------------------------------
def _summaries_both(eng, docs=None, legacy=False):
    got = []
    for par in WRITERS:
        eng.set_variant(MT_VAR_SUMMARIES_PARALLEL, par)
        got.append(eng.summaries(docs, legacy))
    assert got[0] == got[1], "the two writers differ"
    return got[0]


def _tree(raw, it):
    return sn.emit_from_summary(raw, it, sr.long_name)


def _both_alignments_and_own_dumps(eng, its, legacy):
    """every document of an engine alone in a call list and after a neighbour whose summary is 2 mod 4 long (its
    window then starts at 2 mod 4), under both writers, and against extract_segments of the engine's own dumps"""
    want = _summaries_both(eng, None, legacy)
    nb = next(d for d in range(len(want)) if len(want[d]) % 4 == 2)
    pairs = [x for d in range(len(want)) for x in (nb, d)]
    for par in WRITERS:
        eng.set_variant(MT_VAR_SUMMARIES_PARALLEL, par)
        raw, off = eng.summaries_raw(pairs, legacy)
        got = [raw[off[i]: off[i + 1]].tobytes() for i in range(len(pairs))]
        assert got[1::2] == want and all(x == want[nb] for x in got[0::2])
        assert {int(o) % 4 for o in off[1::2]} == {0, 2}
    for d, x in enumerate(eng.dumps()):
        hdr, segs = ol.parse_dump(x)
        ref = sn.extract_segments_legacy(hdr, segs, its[d]) if legacy else sn.extract_segments(hdr, segs, its[d], sr.long_name)
        assert _specs(want[d], its[d]) == ref, d
    return want


# ---- B: the reference's hashes ----------------------------------------------------------------------------------
def _prefix_engine(name, **kw):
    z, b, it, c = sr.fixture(name)
    cuts = [int(x) for x in z["snap_cut"]]
    pre = ol.Batch.from_arrays([sr.prefix_arrays(b, d, cuts[d]) for d in range(b.ndocs)], b.local_long_id)
    return z, it, _engine(pre, c, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", REF_SETS)
def test_gpu_summaries_match_reference(name):
    kw = rg.kernel_variants(name)[-1] if name in rg.NAMES else {}
    z, it, eng = _prefix_engine(name, **kw)
    got = _summaries_both(eng)
    assert [sr.sha(_tree(x, it)) for x in got] == [str(x) for x in z["snap_sha256"]]
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 4, 8])
def test_gpu_summaries_match_reference_on_every_small_build(waves):
    z, it, eng = _prefix_engine("c3_lagged", waves=waves)
    got = _summaries_both(eng)
    assert [sr.sha(_tree(x, it)) for x in got] == [str(x) for x in z["snap_sha256"]]
    eng.close()


@pytest.mark.gpu
def test_gpu_summaries_handle_rows_match_the_host_core():
    """allocated PermutationSegment handles (the pcap engine): runs whose handles follow merge, others do not"""
    import test_ref_handles as rh
    from fluidframework_amd.engine import Engine
    z, c, caps, b = rh.load()
    eng = Engine(b.ndocs, **dict(c, pcap=rh.PCAP))
    eng.start_collab(b.local_long_id)
    eng.replay(b)
    assert (eng.errors()[0] == 0).all()
    _, err, st = core_host.replay_batch(b, caps, pcap=rh.PCAP)
    assert (err == 0).all()
    handles = 0
    for mode in (V1, LEGACY):
        got = _summaries_both(eng, legacy=mode == LEGACY)
        assert got == [sd.host_summary(st, d, mode) for d in range(b.ndocs)]
        handles += sum(1 for x in got for s in ol.parse_dump(x)[1] if s["flags"] & ol.DF_HANDLE)
    assert handles > 0
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True])
def test_gpu_summaries_match_reference_on_both_tiled_builds(wide):
    assert rg.kernel_variants("c4_large") == [{"wide": False}, {"wide": True}]
    z, it, eng = _prefix_engine("c4_large", wide=wide)
    got = _summaries_both(eng)
    assert [sr.sha(_tree(x, it)) for x in got] == [str(x) for x in z["snap_sha256"]]
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["refzamboni", "refranges", "refinserts", "refprops"])
def test_gpu_summaries_match_reference_hand_built_logs(family):
    """the 24-slot flat profile: refprops holds the NaN and consensus-object neighbours (c_nan_neighbours,
    c_cons_neighbours: never merged) and rows with 24 keys"""
    from fluidframework_amd.engine import Engine
    mod, kinds = _families()[family]
    z = mod.fixture()
    idx, cs = mod.fitting("flat")
    if family == "refprops":
        assert {"c_nan_neighbours", "c_cons_neighbours", "z_24_equal"} <= {c.name for c in cs}
    nbs = sd.neighbours(ol.Interner())  # for the windows that start at 2 mod 4
    b = ol.Batch.from_logs([c.log for c in cs] + [x.log for x in nbs])
    # refranges holds reconnect (MT_OPF_REGEN) records, which replay in the client-feature build only (rcap > 0)
    eng = Engine(b.ndocs, **dict(profile_caps("flat"), **({"rcap": 64} if family == "refranges" else {})))
    if kinds is not None:
        eng.set_value_kinds(kinds)
    eng.start_collab(b.local_long_id)
    eng.replay(b)
    assert (eng.errors()[0] == 0).all()
    its = [c.log.interner for c in cs] + [x.log.interner for x in nbs]
    got = _both_alignments_and_own_dumps(eng, its, False)
    _both_alignments_and_own_dumps(eng, its, True)
    for k, c in enumerate(cs):
        assert sr.sha(_tree(got[k], c.log.interner)) == str(z["snap_sha256"][idx[k]]), c.name
    eng.close()


@pytest.mark.gpu
def test_gpu_summaries_match_reference_handle_summaries():
    from fluidframework_amd.engine import Engine
    hs, c, caps, pre, trees = _hsnap_prefixes()
    it = gen.generator_interner()
    eng = Engine(pre.ndocs, **dict(c, pcap=hs.PCAP))
    eng.start_collab(pre.local_long_id)
    eng.replay(pre)
    assert (eng.errors()[0] == 0).all()
    got = _summaries_both(eng)
    assert [sr.sha(_tree(x, it)) for x in got] == [sr.sha(t) for t in trees]
    eng.close()


@pytest.mark.gpu
def test_gpu_summaries_of_handle_documents():
    from fluidframework_amd.engine import Engine, default_caps
    ds = sd.handle_docs()
    b = sd.batch(ds)
    _, err, st = core_host.replay_batch(b, pcap=1 << 10)
    eng = Engine(b.ndocs, **dict(default_caps(512), pcap=1 << 10))
    eng.start_collab(b.local_long_id)
    eng.replay(b)
    assert (err == 0).all() and (eng.errors()[0] == 0).all()
    for mode in (V1, LEGACY):
        got = _both_alignments_and_own_dumps(eng, [x.log.interner for x in ds], mode == LEGACY)
        assert got == [sd.host_summary(st, d, mode) for d in range(b.ndocs)]
        for d, x in enumerate(eng.dumps()):
            hdr, segs = ol.parse_dump(x)
            ref = sn.extract_segments_legacy(hdr, segs, ds[d].log.interner) if mode == LEGACY else \
                sn.extract_segments(hdr, segs, ds[d].log.interner, sr.long_name)
            assert _specs(got[d], ds[d].log.interner) == ref
    eng.close()


# ---- C: plumbing ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text_eng():
    b = pm.text_mix()
    eng = _engine(b, pm.SMALL)
    assert set(eng.promoted().tolist()) == pm.TEXT_PROMOTED
    it = gen.generator_interner()
    want = []
    for mode in (V1, LEGACY):
        per = []
        for x in eng.dumps():
            hdr, segs = ol.parse_dump(x)
            per.append(sn.extract_segments(hdr, segs, it, sr.long_name) if mode == V1 else
                       sn.extract_segments_legacy(hdr, segs, it))
        want.append(per)
    yield eng, b, it, want
    eng.close()


def _specs(raw, it):
    return sn.specs_from_summary(*ol.parse_dump(raw), it, sr.long_name)


@pytest.mark.gpu
@pytest.mark.parametrize("par", WRITERS)
def test_gpu_summaries_of_promoted_documents(text_eng, par):
    eng, b, it, want = text_eng
    eng.set_variant(MT_VAR_SUMMARIES_PARALLEL, par)
    for mode in (V1, LEGACY):
        for docs in _doc_lists(b.ndocs):
            ids = range(b.ndocs) if docs is None else docs.tolist()
            got = eng.summaries(docs, legacy=mode == LEGACY)
            assert [_specs(x, it) for x in got] == [want[mode][d] for d in ids]


@pytest.mark.gpu
@pytest.mark.parametrize("par", WRITERS)
def test_gpu_summaries_sizing_and_arguments(text_eng, par):
    eng, b, it, _ = text_eng
    eng.set_variant(MT_VAR_SUMMARIES_PARALLEL, par)
    want = eng.summaries()
    m = b.ndocs
    off = np.zeros(m + 1, np.int64)
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def call(mm, docs, out, cap, mode=V1):
        return eng.L.mt_engine_summaries(eng.h, mm, vp(docs), mode, vp(off), vp(out), cap)
    total = call(m, None, None, 0)
    assert total == sum(len(x) for x in want) and off[0] == 0 and off[m] == total
    assert np.diff(off).tolist() == [len(x) for x in want]
    buf = np.full(total + 16, 0xA5, np.uint8)
    off[:] = -1
    assert call(m, None, buf, total - 1) == total and (buf == 0xA5).all() and off[m] == total
    assert call(m, None, buf, total) == total and (buf[total:] == 0xA5).all()
    assert buf[:total].tobytes() == b"".join(want)
    off[:] = -1
    assert eng.L.mt_engine_summaries(eng.h, 0, None, V1, None, None, 0) == 0
    assert call(0, None, buf, total) == 0 and (off == -1).all()
    for bad in ([0, m], [-1, 0]):
        assert call(2, np.asarray(bad, np.int64), None, 0) == -MT_E_ARG
    for mode in (-1, 2):
        assert call(m, None, None, 0, mode) == -MT_E_ARG
    big = np.zeros(m + 2, np.int64)
    assert eng.L.mt_engine_summaries(eng.h, m + 1, None, V1, vp(big), None, 0) == -MT_E_ARG
    assert eng.L.mt_engine_set_variant(eng.h, MT_VAR_SUMMARIES_PARALLEL, 2) == MT_E_ARG


@pytest.mark.gpu
def test_gpu_summaries_tiled_profile():
    from fluidframework_amd.engine import default_caps
    b = gen.generate(gen.config3(512), ids=np.arange(3), threads=3)
    eng = _engine(b, default_caps(512, config=4))
    it = gen.generator_interner()
    docs = [1, 0, 1, 2, 1, 0, 1, 1]
    for legacy in (False, True):
        want = []
        for x in eng.dumps():
            hdr, segs = ol.parse_dump(x)
            want.append(sn.extract_segments_legacy(hdr, segs, it) if legacy else
                        sn.extract_segments(hdr, segs, it, sr.long_name))
        assert [_specs(x, it) for x in _summaries_both(eng, docs, legacy)] == [want[d] for d in docs]
        assert [_specs(x, it) for x in _summaries_both(eng, None, legacy)] == want
    eng.close()


@pytest.mark.gpu
def test_gpu_emit_batch_on_the_device_gives_the_same_trees():
    z, it, eng = _prefix_engine("c3_lagged")
    docs = [5, 0, 7, 5, 2]
    for par in WRITERS:
        eng.set_variant(MT_VAR_SUMMARIES_PARALLEL, par)
        trees = sn.emit_batch(eng, None, it, sr.long_name, device=True)
        assert trees == sn.emit_batch(eng, None, it, sr.long_name)
        assert [sr.sha(t) for t in trees] == [str(x) for x in z["snap_sha256"]]
        assert sn.emit_batch(eng, docs, it, sr.long_name, legacy=True, device=True) == \
            sn.emit_batch(eng, docs, it, sr.long_name, legacy=True)
    eng.close()


# ---- D: writer edges --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_eng():
    from fluidframework_amd.engine import default_caps
    ds, b, st, sums = _edge()
    eng = _engine(b, default_caps(512))
    yield eng, ds, b, sums
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("par", WRITERS)
@pytest.mark.parametrize("mode", [V1, LEGACY])
def test_gpu_summaries_writer_edges(edge_eng, par, mode):
    eng, ds, b, sums = edge_eng
    it = ds[0].log.interner
    legacy = mode == LEGACY
    eng.set_variant(MT_VAR_SUMMARIES_PARALLEL, par)
    want = [sums[d][mode] for d in range(b.ndocs)]
    nb = 1 if not legacy else next(d for d in range(b.ndocs) if len(want[d]) % 4 == 2)
    assert len(want[nb]) % 4 == 2 and (legacy or len(want[nb]) == 66)  # v1: the 66-byte neighbour (legacy elides its row)
    # every document alone (its window starts 4-byte aligned) and after the neighbour (it starts at 2 mod 4)
    alone = eng.summaries_raw(None, legacy)
    assert [alone[0][alone[1][d]: alone[1][d + 1]].tobytes() for d in range(b.ndocs)] == want
    assert {int(o) % 4 for o in alone[1]} == {0, 2}
    pairs = [x for d in range(b.ndocs) for x in (nb, d)]
    raw, off = eng.summaries_raw(pairs, legacy)
    got = [raw[off[i]: off[i + 1]].tobytes() for i in range(len(pairs))]
    assert got[1::2] == want and all(x == want[nb] for x in got[0::2])
    assert {int(o) % 4 for o in off[1::2]} == {0, 2}  # both alignments in turn, every document on each
    for d in (0, 1, 5, b.ndocs - 1):
        assert eng.summaries([d], legacy) == [want[d]]
    # and against extract_segments of the engine's own dumps
    for d, x in enumerate(eng.dumps()):
        hdr, segs = ol.parse_dump(x)
        ref = sn.extract_segments_legacy(hdr, segs, it) if legacy else sn.extract_segments(hdr, segs, it, sr.long_name)
        assert _specs(want[d], it) == ref, ds[d].name
