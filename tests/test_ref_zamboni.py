"""Zamboni's append rules against the REFERENCE on long and hand-built rows (tests/golden/refzamboni.npz from
tools/make_ref_goldens.py --zamboni over tests/zamboni_logs.py).

The generator's logs never make the length half of canAppend false (no row over 150 units), so scour's one serial
dependency (the run grows), the newline / marker / property / prevSegment-reset rules on rows it does not produce,
pack's wave over sibling leaves and the planned arena copies are pinned here, one small document per branch; the
case list is the docstring of tests/zamboni_logs.py. Every comparison is byte-exact.

CPU tier: the logs regenerate to the fixture's SHA-256; every case's witness holds on the reference's dump; the
oracle's dumps, the host core's dumps under every profile's capacities (with and without delta stream and local
references), its delta / maintenance stream and snapshot.emit's summaries equal the reference's; the pack cases
replay with an arena that compacts during the minSeq step. GPU tier: every kernel build replays all cases in one
batch to the reference's digests, dumps (single and batched, both writers) and delta streams, in one submit and
in two (cut before the minSeq step); the arena cases run with the small arena found on the CPU."""
import os

import numpy as np
import pytest

from fluidframework_amd import oplog as ol
from fluidframework_amd import snapshot as sn
import core_host
import oracle_client as oc
import zamboni_logs as zl
from make_goldens_sha import log_sha

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = zl.cases()
NAMES = [c.name for c in CASES]
DCAP = 1 << 12  # words of delta stream kept per document (the longest stream here is a few hundred words)
MT_VAR_DUMPS_PARALLEL = 5  # include/mt_engine.h


def profile_caps(profile: str) -> dict:
    from fluidframework_amd.engine import default_caps
    if profile == "small":      # 192 nodes, LDS-resident
        return default_caps(0)
    if profile == "matrix":     # 640 nodes; its default arena (16 units) holds no text
        return dict(default_caps(0, config=5), acap=1 << 16)
    if profile == "flat":       # 4,096 nodes, 24 key slots
        return dict(ncap=4096, hcap=8192, acap=1 << 17, mcap=4096, gcap=1024, ccap=64)
    return default_caps(0, config=4)  # tiled


def caps_tuple(c: dict) -> tuple:
    return tuple(c[k] for k in ("ncap", "hcap", "acap", "mcap", "gcap", "ccap"))


def fixture():
    return np.load(os.path.join(GOLDEN, "refzamboni.npz"), allow_pickle=False)


def ref_dump(z, d: int) -> bytes:
    return z["dumps"][z["dump_off"][d]: z["dump_off"][d + 1]].tobytes()


def fitting(profile: str, perm_only: bool = False):
    """(indices into CASES, the cases) that fit a profile"""
    idx = [i for i, c in enumerate(CASES) if profile in c.profiles and (not perm_only or c.kind == "perm")]
    return idx, [CASES[i] for i in idx]


def test_logs_regenerate_to_the_fixture():
    z = fixture()
    assert [str(n) for n in z["names"]] == NAMES
    assert log_sha(zl.batch(CASES)) == str(z["log_sha256"]), "tests/zamboni_logs.py no longer builds the fixture's logs"
    assert len(z["digests"]) == len(CASES) == len(z["snap_sha256"]) == len(z["delta_hashes"])


def test_every_required_branch_has_a_case():
    need = {"g_256_256", "g_257_257", "g_257_256", "g_256_257", "g_run_grows", "g_run_256", "g_run_257",
            "g_long_short_long", "g_refused_restarts", "g_refused_mid", "s_128_128", "s_129_129", "s_129_128",
            "s_128_129", "s_run_grows", "s_run_128", "s_run_129", "s_long_short_long", "s_refused_restarts",
            "s_refused_mid", "perm_300_300", "nl_tail", "nl_split_left", "nl_split_right", "s_nl_tail", "mk_between",
            "mk_first", "mk_last", "rs_unlinked", "rs_held", "rs_pending", "rs_pending_acked", "pr_equal",
            "pr_ninth_key", "pr_one_side", "lb_two_leaves", "pk_long_runs", "pk_pairs", "ar_both_to_top", "ar_prepend",
            "ar_append"}
    assert need <= set(NAMES)
    for c in CASES:
        assert c.branch and callable(c.witness) and c.name in zl.__doc__, c.name
        assert all(r[9] <= 300 for r in c.log.ops) and len(c.log.ops) < 100  # small documents (r[9]: text_len)


@pytest.mark.parametrize("name", NAMES)
def test_witness_holds_on_the_reference_dump(name):
    z = fixture()
    d = NAMES.index(name)
    hdr, segs = ol.parse_dump(ref_dump(z, d))
    assert CASES[d].witness(hdr, segs), (CASES[d].branch, hdr, [(s["len"], s["leaf"], s["text"][:16]) for s in segs])


def test_the_length_rule_refuses_pairs_in_the_fixture():
    """what no generator log shows: adjacent settled rows of one leaf, equal properties, kept apart by length alone"""
    z = fixture()
    refused = 0
    for d, c in enumerate(CASES):
        hdr, segs = ol.parse_dump(ref_dump(z, d))
        lim = 128 if c.kind == "run" else 256
        for a, b in zip(segs, segs[1:]):
            if (a["kind"] == b["kind"] != ol.SEG_PERM and a["kind"] != ol.SEG_MARKER and a["leaf"] == b["leaf"]
                    and a["len"] > lim and b["len"] > lim and not a["text"].endswith("\n")):
                refused += 1
    assert refused >= 12


def test_oracle_matches_reference():
    z = fixture()
    b = zl.batch(CASES)
    for d, c in enumerate(CASES):
        o = oc.OracleClient(c.log.interner)
        o.start_collab(c.log.local_long_id)
        assert o.replay_arrays(*b.doc(d)) == 0, c.name
        assert o.dump() == ref_dump(z, d), c.name
        assert o.digest() == int(z["digests"][d]), c.name


def _host(profile, extras):
    z = fixture()
    idx_all, cs_all = fitting(profile)
    step = 8 if profile == "tiled" else len(idx_all)  # a tiled replica's image is hundreds of MB: a few at a time
    for at in range(0, len(idx_all), step):
        idx, cs = idx_all[at: at + step], cs_all[at: at + step]
        _, err, st = core_host.replay_batch(zl.batch(cs), caps_tuple(profile_caps(profile)), **extras)
        assert (err == 0).all(), [cs[i].name for i in np.nonzero(err)[0]]
        for k, d in enumerate(idx):
            assert st.dump(k) == ref_dump(z, d), f"{profile} {extras}: {cs[k].name}"
            if extras.get("dcap"):
                n, h, _ = st.deltas(k)
                assert (n, h) == (int(z["delta_nwords"][d]), int(z["delta_hashes"][d])), f"{profile}: {cs[k].name}"
        del st
    return len(idx_all)


@pytest.mark.parametrize("profile", ["small", "matrix", "flat", "tiled"])
def test_host_core_matches_reference(profile):
    n = _host(profile, {})
    assert n == len(CASES) - (0 if profile in zl.WIDE_KEYS else 1)  # pr_ninth_key needs 24 key slots


@pytest.mark.parametrize("profile", ["small", "flat", "tiled"])
def test_host_core_with_deltas_and_references_matches_reference(profile):
    """dcap > 0 and rcap > 0: scour's delta (APPEND / UNLINK events in walk order) and reference code paths"""
    _host(profile, dict(dcap=DCAP, rcap=64))


def test_ninth_key_does_not_fit_eight_key_slots():
    """the case that compares past the first 8 key slots is left out of the 8-slot profiles because it cannot run
    there at all (MT_E_CAPACITY), not because it differs"""
    c = [x for x in CASES if x.name == "pr_ninth_key"]
    _, err, _ = core_host.replay_batch(zl.batch(c), caps_tuple(profile_caps("small")))
    assert err[0] == 5


def test_snapshot_emit_matches_reference():
    from test_snapshot_ref import long_name, sha
    z = fixture()
    for d, c in enumerate(CASES):
        tree = sn.emit_from_dump(ref_dump(z, d), c.log.interner, long_name)
        assert sha(tree) == str(z["snap_sha256"][d]), c.name
    # and from the host core's own dumps of a profile every case fits
    idx, cs = fitting("flat")
    _, err, st = core_host.replay_batch(zl.batch(cs), caps_tuple(profile_caps("flat")))
    for k, d in enumerate(idx):
        assert sha(sn.emit_from_dump(st.dump(k), cs[k].log.interner, long_name)) == str(z["snap_sha256"][d]), cs[k].name


def small_arena(name: str):
    """(case, acap, arena top before the step, arena top after the whole log with a large arena): an arena half
    that holds the document up to its minSeq step and half of what the step's appends copy, so the arena compacts
    in the middle of the step (the host core's arena_top, measured here, not assumed)"""
    c = CASES[NAMES.index(name)]
    ops, text, props, kv = zl.batch([c]).doc(0)
    st = core_host.HostStore(1, caps_tuple(profile_caps("small")))
    st.start_collab(0, c.log.local_long_id)
    assert st.replay(0, ops[: c.cut], text, props, kv) == 0
    t0 = st.stats(0)["arena_top"]
    assert st.replay(0, ops[c.cut:], text, props, kv) == 0
    t1 = st.stats(0)["arena_top"]
    assert t1 > t0
    return c, t0 + (t1 - t0) // 2, t0, t1


@pytest.mark.parametrize("name", zl.ARENA_CASES)
def test_host_core_compacts_the_arena_inside_the_step(name):
    z = fixture()
    c, acap, t0, t1 = small_arena(name)
    ops, text, props, kv = zl.batch([c]).doc(0)
    st = core_host.HostStore(1, caps_tuple(dict(profile_caps("small"), acap=acap)))
    st.start_collab(0, c.log.local_long_id)
    assert st.replay(0, ops[: c.cut], text, props, kv) == 0
    assert st.stats(0)["arena_top"] == t0 <= acap, "no compaction before the step"
    assert st.replay(0, ops[c.cut:], text, props, kv) == 0, "the small arena must suffice"
    assert t1 > acap and st.stats(0)["arena_top"] < t1, "the arena did not compact during the step"
    assert st.dump(0) == ref_dump(z, NAMES.index(name))


# ---- GPU -----------------------------------------------------------------------------------------------------------
# every kernel build (include/mt_engine.h mt_engine_set_variant), as test_ref_goldens.kernel_variants: (id, profile,
# engine arguments, PermutationSegment cases only)
BUILDS = [("small-waves1", "small", dict(waves=1), False), ("small-waves4", "small", dict(waves=4), False),
          ("small-waves8", "small", dict(waves=8), False), ("flat", "flat", {}, False), ("matrix", "matrix", {}, True),
          ("tiled-narrow", "tiled", dict(wide=False), False), ("tiled-wide", "tiled", dict(wide=True), False)]
BUILD_IDS = [b[0] for b in BUILDS]


def _engine(cs, profile, variant, **extra):
    from fluidframework_amd.engine import Engine
    b = zl.batch(cs)
    eng = Engine(b.ndocs, **variant, **dict(profile_caps(profile), **extra))
    eng.start_collab(b.local_long_id)
    return eng, b


def _check_state(eng, z, idx, cs, what, dump_of=ref_dump, promoted=()):
    """no error; exactly the documents `promoted` (indices into cs) needed a larger profile; digests and dumps equal
    the fixture's (dump_of(z, d): the reference's dump of fixture document d)"""
    err, err_op = eng.errors()
    assert (err == 0).all(), (what, [(cs[i].name, int(err[i]), int(err_op[i])) for i in np.nonzero(err)[0]])
    assert sorted(int(x) for x in eng.promoted()) == sorted(promoted), (what, "no other case needs a larger profile")
    bad = np.nonzero(eng.digests() != z["digests"][idx])[0]
    assert len(bad) == 0, f"{what}: HIP engine differs from the reference on {[cs[i].name for i in bad]}"
    for k, d in enumerate(idx):
        assert eng.dump(k) == dump_of(z, d), f"{what}: {cs[k].name}"


@pytest.mark.gpu
@pytest.mark.parametrize("build", BUILDS, ids=BUILD_IDS)
def test_gpu_matches_reference(build):
    name, profile, variant, perm_only = build
    z = fixture()
    idx, cs = fitting(profile, perm_only)
    eng, b = _engine(cs, profile, variant)
    eng.replay(b)
    _check_state(eng, z, idx, cs, name)
    for par in (0, 1):  # mt_engine_dumps under both writers
        eng.set_variant(MT_VAR_DUMPS_PARALLEL, par)
        got = eng.dumps()
        for k, d in enumerate(idx):
            assert got[k] == ref_dump(z, d), f"{name}: dumps writer {par}: {cs[k].name}"


@pytest.mark.gpu
@pytest.mark.parametrize("build", BUILDS, ids=BUILD_IDS)
def test_gpu_delta_stream_matches_reference(build):
    name, profile, variant, perm_only = build
    z = fixture()
    idx, cs = fitting(profile, perm_only)
    eng, b = _engine(cs, profile, variant, dcap=DCAP)
    eng.replay(b)
    _check_state(eng, z, idx, cs, name)
    n, h = eng.delta_state()
    bad = np.nonzero((n != z["delta_nwords"][idx]) | (h != z["delta_hashes"][idx]))[0]
    assert len(bad) == 0, f"{name}: delta stream differs from the reference on {[cs[i].name for i in bad]}"


@pytest.mark.gpu
@pytest.mark.parametrize("build", BUILDS, ids=BUILD_IDS)
def test_gpu_two_submits_match_reference(build):
    """the batch in two parts, cut just before each document's minSeq step: state persists between submits"""
    name, profile, variant, perm_only = build
    z = fixture()
    idx, cs = fitting(profile, perm_only)
    eng, _ = _engine(cs, profile, variant)
    head, tail = zl.split_at_cut(cs)
    eng.replay(head)
    err, _ = eng.errors()
    assert (err == 0).all()
    eng.replay(tail)
    _check_state(eng, z, idx, cs, name + " in two submits")


@pytest.mark.gpu
@pytest.mark.parametrize("name", zl.ARENA_CASES)
def test_gpu_compacts_the_arena_inside_the_step(name):
    """the pack's walk with copies planned and heads moved when the arena fills: the wave makes its planned copies,
    compacts and goes on serially (mt_core.h scour_par); no error, no promotion to a larger arena"""
    z = fixture()
    c, acap, _, _ = small_arena(name)
    d = NAMES.index(name)
    for waves in (1, 4, 8):
        eng, b = _engine([c], "small", dict(waves=waves), acap=acap)
        eng.replay(b)
        _check_state(eng, z, [d], [c], f"{name} acap {acap} waves {waves}")
        eng.close()
