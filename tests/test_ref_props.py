"""The property manager's key-slot and pending-count rules against the REFERENCE (tests/golden/refprops.npz from
tools/make_ref_goldens.py --props over tests/prop_logs.py).

add_props_par (a lane per key slot, a lane per pair of the op, new slots in first-appearance order) and the annotate
branch of ack_rows (a lane per member row) are compiled for the GPU only; the host core, the oracle and the one-lane
builds take add_props_serial / ack_props. The generator's ops carry at most two pairs over six keys, so no other
fixture fills the 8 or the 24 key slots, holds a pending count above 1 or two outstanding local rewrites. Pending
counts are not in the canonical dump: the cases end with probe ops whose outcome the dump and the delta stream's
propertyDeltas show. The case list is the docstring of tests/prop_logs.py. Every comparison is byte-exact.

CPU tier: the logs regenerate to the fixture's SHA-256; every witness holds on the reference's dump and delta words;
a census proves the widths and counts are there and that the generator's logs have none; the oracle (cases without
combining ops), the host core under every profile (with and without delta stream) and snapshot.emit equal the
reference; the cap cases give their stated outcome. GPU tier: every kernel build replays all cases in one batch to
the reference's digests, dumps (single and batched, both writers) and delta streams, in one submit and in two (cut
between a local op and its ack); the 8-slot builds promote exactly the documents with more than 8 keys."""
import functools
import json
import os

import numpy as np
import pytest

from fluidframework_amd import oplog as ol
from fluidframework_amd import snapshot as sn
import core_host
import oracle_client as oc
import prop_logs as pl
from make_goldens_sha import log_sha
from test_ref_ranges import MT_E_CAPACITY, cap_outcome
from test_ref_zamboni import BUILD_IDS, BUILDS, MT_VAR_DUMPS_PARALLEL, _check_state, caps_tuple, profile_caps

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = pl.cases()
CAPS = pl.caps()
EVERY = CASES + CAPS
NAMES = [c.name for c in EVERY]
KINDS = ol.value_kinds(EVERY[0].log.interner)
EIGHT = ("small", "matrix")  # the profiles with 8 key slots
# every cap case latches MT_E_CAPACITY at the record that needs the room (Case.cut) in every profile it reaches (an
# 8-slot GPU build promotes the key cases first; the 8-slot host profiles latch at their ninth key, record 1);
# DESIGN.md §10
KEY_CAPS = ("cap_25_keys", "cap_null_unknown_24", "cap_65_pairs")


def fixture():
    return np.load(os.path.join(GOLDEN, "refprops.npz"), allow_pickle=False)


def ref_dump(z, d: int) -> bytes:
    return z["dumps"][z["dump_off"][d]: z["dump_off"][d + 1]].tobytes()


def ref_deltas(z, d: int):
    return z["delta_words"][z["delta_off"][d]: z["delta_off"][d + 1]]


def fitting(profile: str, perm_only: bool = False, promote: bool = False):
    """(indices into the fixture, the cases) whose key slots a profile holds; `promote`: and the others"""
    idx = [d for d, c in enumerate(CASES) if (promote or profile in c.profiles) and (not perm_only or c.kind == "perm")]
    return idx, [CASES[d] for d in idx]


def test_logs_regenerate_to_the_fixture():
    z = fixture()
    assert [str(n) for n in z["names"]] == NAMES
    assert log_sha(pl.batch(EVERY)) == str(z["log_sha256"]), "tests/prop_logs.py no longer builds the fixture's logs"
    assert len(z["digests"]) == len(EVERY) == len(z["snap_sha256"]) == len(z["delta_hashes"]) == len(z["dump_off"]) - 1
    assert [int(n) < 0 for n in z["delta_nwords"]] == [c.combining for c in EVERY]
    assert os.path.getsize(os.path.join(GOLDEN, "refprops.npz")) < 64 << 10


def test_every_required_case_exists():
    width = ["w_nkv1", "w_nkv2", "w_nkv7", "w_nkv8", "w_nkv9", "w_nkv23", "w_nkv24", "w_fill_8", "w_fill_24",
             "w_ninth_late", "w_null_unknown", "w_mixed_new_old", "w_insert_props_8", "w_insert_props_24"]
    need = {n + s for n in width for s in ("", "_mk", "_it", "_pm")} - {"w_insert_props_8_pm", "w_insert_props_24_pm"}
    need |= {"p_shadow_many", "p_count_2", "p_count_3", "p_count_255", "p_partial_overlap", "p_null_pending",
             "p_split_before_ack", "p_split_after_ack", "p_ack_many_rows", "p_two_groups_one_row", "p_notcollab",
             "r_remote_many", "r_remote_keeps_pending", "r_remote_keeps_pending_8", "r_local_blocks", "r_two_local",
             "r_local_then_local_plain", "r_rewrite_empty", "r_fresh_row", "c_incr_pending", "c_consensus_mixed",
             "c_incr_chain", "c_nan_neighbours", "c_cons_neighbours", "z_24_equal", "z_24_last_differs",
             "z_deleted_vs_never"}
    assert need == set(c.name for c in CASES)
    assert tuple(c.name for c in CAPS) == pl.CAP_NAMES
    for c in EVERY:
        stem = c.name[:-3] if c.name.endswith(("_mk", "_it", "_pm")) else c.name
        assert c.branch and callable(c.witness) and stem.rstrip("0123456789").rstrip("_") in pl.__doc__, c.name
        assert len(c.log.ops) < 600, c.name
        assert c.combining or c.dwitness is not None
        # every cut with a local op before it lies between a local op and its ack
        assert 0 < c.cut < len(c.log.ops) or len(c.log.ops) == 2, c.name


@pytest.mark.parametrize("name", NAMES)
def test_witness_holds_on_the_reference(name):
    z = fixture()
    d = NAMES.index(name)
    hdr, segs = ol.parse_dump(ref_dump(z, d))
    c = EVERY[d]
    assert c.witness(hdr, segs), (c.branch, hdr, [(pl.props_of(c.log.interner, s), s["ngroups"]) for s in segs][:6])
    if c.dwitness is not None:
        assert len(ref_deltas(z, d)) == int(z["delta_nwords"][d])
        assert c.dwitness(ol.decode_deltas(ref_deltas(z, d))), c.branch


def test_shadowed_probes_leave_the_key_out_of_the_property_deltas():
    """p_count_3 in the reference's own words: the probes {k0, k1} after the first two acks report k1 alone, the
    probe after the last ack both keys; r_local_blocks' blocked ops report no property deltas at all"""
    z = fixture()
    it = EVERY[0].log.interner
    ev = [e for e in ol.decode_deltas(ref_deltas(z, NAMES.index("p_count_3"))) if e[0] == 2 and e[1] > 0]
    assert [sorted(it.keys[k] for k, _ in e[2][0][3]) for e in ev] == [["k1"], ["k1"], ["k0", "k1"]]
    ev = [e for e in ol.decode_deltas(ref_deltas(z, NAMES.index("r_local_blocks"))) if e[0] == 2 and e[1] > 0]
    assert [e[2][0][3] is None for e in ev] == [True, True, False, False]


def test_census_the_widths_and_counts_are_in_the_fixture():
    cen = pl.census(pl.batch(EVERY))
    print(cen)
    for k in ("p1", "p2", "p3_8", "p9_24", "p25", "k_le8", "k_8", "k_9_23", "k_24"):
        assert cen[k] > 0, (k, cen)
    assert cen["maxpk"] == 256 and cen["maxprw"] == 2
    assert pl.census(pl.batch(CASES))["maxpk"] == 255
    # and in the reference's dumps: rows that hold exactly 8 and exactly 24 pairs
    z = fixture()
    held = {len(s["props"]) for d in range(len(EVERY)) for s in ol.parse_dump(ref_dump(z, d))[1]}
    assert {0, 1, 2, 7, 8, 9, 23, 24} <= held and max(held) == 65


@pytest.mark.parametrize("name", ["ref_c2_observer", "ref_c3_lagged", "ref_c5_perm"])
def test_census_the_generator_fixtures_have_none(name):
    """the generator's logs (the first documents of each committed fixture set, regenerated): no op above 2 pairs, no
    document above 8 keys"""
    from fluidframework_amd import gen
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    w = gen.Workload(**json.loads(str(z["workload"])))
    cen = pl.census(gen.generate(w, ids=[int(i) for i in z["doc_ids"][:8]], threads=4))
    print(cen)
    assert cen["p1"] + cen["p2"] > 100 and cen["maxpairs"] <= 2 and cen["maxkeys"] <= 8, cen
    assert cen["k_8"] == cen["k_9_23"] == cen["k_24"] == cen["k_over"] == 0, cen
    # (maxpk / maxprw count a log's outstanding local annotates wherever they lie: in the generator's logs they lie on
    # different rows; its highest per-row counts are what the committed generator fixtures already replay)


@functools.lru_cache(maxsize=None)
def _plain():
    return [d for d, c in enumerate(EVERY) if not c.combining]


def test_oracle_matches_reference():
    """the oracle has no combining ops: the cases without them, the cap cases included (it has no caps)"""
    z = fixture()
    b = pl.batch(EVERY)
    for d in _plain():
        c = EVERY[d]
        o = oc.OracleClient(c.log.interner)
        o.start_collab(c.log.local_long_id)
        assert o.replay_arrays(*b.doc(d)) == 0, c.name
        assert o.dump() == ref_dump(z, d), c.name
        assert o.digest() == int(z["digests"][d]), c.name


def _dcap(z, idx) -> int:
    return 1 << int(np.ceil(np.log2(int(z["delta_nwords"][idx].max()) + 1)))


def _host(profile, extras):
    z = fixture()
    idx_all, cs_all = fitting(profile)
    step = 8 if profile == "tiled" else len(idx_all)  # a tiled replica's image is hundreds of MB: a few at a time
    for at in range(0, len(idx_all), step):
        idx, cs = idx_all[at: at + step], cs_all[at: at + step]
        _, err, st = core_host.replay_batch(pl.batch(cs), caps_tuple(profile_caps(profile)), kinds=KINDS, **extras)
        assert (err == 0).all(), [(cs[i].name, st.error_op(int(i))) for i in np.nonzero(err)[0]]
        for k, d in enumerate(idx):
            assert st.dump(k) == ref_dump(z, d), f"{profile} {extras}: {cs[k].name}"
            if extras.get("dcap") and not cs[k].combining:
                n, h, words = st.deltas(k)
                assert (n, h) == (int(z["delta_nwords"][d]), int(z["delta_hashes"][d])), f"{profile}: {cs[k].name}"
                assert words.tolist() == ref_deltas(z, d).tolist()
        del st
    return len(idx_all)


@pytest.mark.parametrize("profile", ["small", "matrix", "flat", "tiled"])
def test_host_core_matches_reference(profile):
    n = _host(profile, {})
    wide = sum(c.profiles == pl.WIDE_KEYS for c in CASES)
    assert wide >= 25 and n == len(CASES) - (wide if profile in EIGHT else 0)


@pytest.mark.parametrize("profile", ["small", "flat", "tiled"])
def test_host_core_with_deltas_matches_reference(profile):
    z = fixture()
    _host(profile, dict(dcap=_dcap(z, fitting(profile)[0])))


def test_wide_cases_do_not_fit_eight_key_slots():
    """the cases left out of the 8-slot profiles cannot run there at all (MT_E_CAPACITY at the record that names the
    ninth key), w_null_unknown among them: its ninth key is a null the reference keeps no trace of"""
    cs = [c for c in CASES if c.profiles == pl.WIDE_KEYS and not c.combining]
    _, err, st = core_host.replay_batch(pl.batch(cs), caps_tuple(profile_caps("small")))
    assert (err == MT_E_CAPACITY).all(), [c.name for c, e in zip(cs, err) if e != MT_E_CAPACITY]
    k = [c.name for c in cs].index("w_null_unknown")
    assert st.error_op(k) == cs[k].cut == len(cs[k].log.ops) - 1


def test_snapshot_emit_matches_reference():
    from test_snapshot_ref import long_name, sha
    z = fixture()
    for d, c in enumerate(EVERY):
        tree = sn.emit_from_dump(ref_dump(z, d), c.log.interner, long_name)
        assert sha(tree) == str(z["snap_sha256"][d]), c.name


@pytest.mark.parametrize("name", ["c_nan_neighbours", "c_cons_neighbours"])
def test_snapshots_keep_unmatchable_neighbours_apart(name):
    """both extractions (SnapshotV1 and legacy) keep the rows with NaN / the same consensus object apart and merge the
    pair with ordinary equal values: four segments, as the reference's summary"""
    z = fixture()
    c = EVERY[NAMES.index(name)]
    hdr, segs = ol.parse_dump(ref_dump(z, NAMES.index(name)))
    assert hdr["minSeq"] >= max(s["seq"] for s in segs) and len(segs) == 4
    from test_snapshot_ref import long_name
    assert [n for _, n in sn.extract_segments(hdr, segs, c.log.interner, long_name)] == [6, 6, 1, 12]
    assert [n for _, n in sn.extract_segments_legacy(hdr, segs, c.log.interner)] == [6, 6, 1, 12]
    # and rows the dump itself still holds apart with ordinary equal values do merge in the summary
    two = [dict(segs[3], len=6, text=segs[3]["text"][:6]), dict(segs[3], len=6, text=segs[3]["text"][6:])]
    assert [n for _, n in sn.extract_segments(hdr, segs[:3] + two, c.log.interner, long_name)] == [6, 6, 1, 12]


def cap_profiles(c):
    return ["flat", "tiled"] if c.name in KEY_CAPS else ["small", "flat", "tiled"]


@pytest.mark.parametrize("name", pl.CAP_NAMES)
def test_cap_cases_on_the_host_core(name):
    z = fixture()
    d = NAMES.index(name)
    c = EVERY[d]
    for profile in cap_profiles(c):
        dig, err, st = core_host.replay_batch(pl.batch([c]), caps_tuple(profile_caps(profile)))
        assert cap_outcome(c, int(err[0]), st.error_op(0), int(dig[0]), int(z["digests"][d])) == "capacity", profile
        del st
    if name in KEY_CAPS:  # the 8-slot profiles latch at their ninth key: the first annotate
        _, err, st = core_host.replay_batch(pl.batch([c]), caps_tuple(profile_caps("small")))
        assert (int(err[0]), st.error_op(0)) == (MT_E_CAPACITY, 1)


def test_pending_count_255_fits_every_profile():
    """p_count_255 holds 255 groups and 255 membership entries at once: what the host core reports is within every
    profile's gcap / mcap, so the case needs no capacities of its own"""
    c = EVERY[NAMES.index("p_count_255")]
    ops, text, props, kv = c.log.arrays()
    st = core_host.HostStore(1, caps_tuple(profile_caps("small")))
    st.start_collab(0, c.log.local_long_id)
    assert st.replay(0, ops[: c.cut], text, props, kv) == 0
    assert st.pending(0) == 255 and st.stats(0)["mem"] == 255
    for profile in ("small", "matrix", "flat", "tiled"):
        caps = profile_caps(profile)
        assert caps["gcap"] > 256 and caps["mcap"] > 256, profile


# ---- GPU -----------------------------------------------------------------------------------------------------------
def _engine(cs, profile, variant, **extra):
    from fluidframework_amd.engine import Engine
    b = pl.batch(cs)
    eng = Engine(b.ndocs, **variant, **dict(profile_caps(profile), **extra))
    eng.set_value_kinds(KINDS)
    eng.start_collab(b.local_long_id)
    return eng, b


def _promoted(profile, cs):
    """the documents a build must hand to a larger one: those with more than 8 keys, in an 8-slot build"""
    return [k for k, c in enumerate(cs) if profile not in c.profiles]


@pytest.mark.gpu
@pytest.mark.parametrize("build", BUILDS, ids=BUILD_IDS)
def test_gpu_matches_reference(build):
    name, profile, variant, perm_only = build
    z = fixture()
    idx, cs = fitting(profile, perm_only, promote=True)
    eng, b = _engine(cs, profile, variant)
    eng.replay(b)
    pro = _promoted(profile, cs)
    assert bool(pro) == (profile in EIGHT)
    _check_state(eng, z, idx, cs, name, ref_dump, pro)
    for par in (0, 1):  # mt_engine_dumps under both writers
        eng.set_variant(MT_VAR_DUMPS_PARALLEL, par)
        got = eng.dumps()
        for k, d in enumerate(idx):
            assert got[k] == ref_dump(z, d), f"{name}: dumps writer {par}: {cs[k].name}"
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("build", BUILDS, ids=BUILD_IDS)
def test_gpu_delta_stream_matches_reference(build):
    """dcap > 0: the client-feature build; a document is promoted only in an engine without client features, so the
    documents this build would promote are left to the builds that hold them"""
    name, profile, variant, perm_only = build
    z = fixture()
    idx, cs = fitting(profile, perm_only)
    eng, b = _engine(cs, profile, variant, dcap=_dcap(z, idx))
    eng.replay(b)
    _check_state(eng, z, idx, cs, name, ref_dump)
    n, h = eng.delta_state()
    plain = np.asarray([not c.combining for c in cs])
    bad = np.nonzero(plain & ((n != z["delta_nwords"][idx]) | (h != z["delta_hashes"][idx])))[0]
    assert len(bad) == 0, f"{name}: delta stream differs from the reference on {[cs[i].name for i in bad]}"
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("build", BUILDS, ids=BUILD_IDS)
def test_gpu_two_submits_match_reference(build):
    """the batch in two parts, cut between a local op and its ack (a case without one: before its last op): the
    pending counts persist between submits"""
    name, profile, variant, perm_only = build
    z = fixture()
    idx, cs = fitting(profile, perm_only)
    eng, _ = _engine(cs, profile, variant)
    head, tail = pl.split_at_cut(cs)
    eng.replay(head)
    err, _ = eng.errors()
    assert (err == 0).all()
    eng.replay(tail)
    _check_state(eng, z, idx, cs, name + " in two submits", ref_dump)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("build", [b for b in BUILDS if not b[3]], ids=[b[0] for b in BUILDS if not b[3]])
def test_gpu_cap_cases(build):
    """MT_E_CAPACITY at the record that needs the room in every build (an 8-slot build promotes the cases first; the
    promoted engine reports it); the matrix build replays PermutationSegment documents only: none is one"""
    name, profile, variant, perm_only = build
    z = fixture()
    idx = [NAMES.index(c.name) for c in CAPS]
    eng, b = _engine(CAPS, profile, variant)
    eng.replay(b)
    err, err_op = eng.errors()
    dig = eng.digests()
    for k, d in enumerate(idx):
        got = cap_outcome(CAPS[k], int(err[k]), int(err_op[k]), int(dig[k]), int(z["digests"][d]))
        assert got == "capacity", (name, CAPS[k].name)
    # a build cannot tell which capacity ran out: every latched document is handed to the next larger profile while
    # there is one (include/mt_engine.h mt_engine_sync), and latches there again
    pro = sorted(int(x) for x in eng.promoted())
    print(name, "promoted", pro)
    assert pro == [0, 1, 2, 3] if profile in EIGHT else pro in ([], [0, 1, 2, 3]), name
    eng.close()
