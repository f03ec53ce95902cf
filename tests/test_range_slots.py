"""The slots a range op carries through its two boundary splits (mt_core.h range_op / split_slot `track`) against
the oracle, on the hand-built logs of tests/range_slot_logs.py (the case list is its docstring).

CPU tier: every case reaches its shape on the oracle's dumps (the leaves' row counts before and after the op, where the
first and last touched rows end up); the host core under the small, matrix and flat profiles' capacities, with and
without a delta stream (the serial visit), equals the oracle byte for byte. GPU tier: every kernel build of the
config-2/3 profile (1, 4 and 8 waves), the flat and the matrix build replay the cases in one batch and in two
submits cut before the op, with and without a delta log, to the oracle's errors, digests and dumps."""
import functools

import numpy as np
import pytest

from fluidframework_amd import oplog as ol
import core_host
import oracle_client as oc
import range_slot_logs as sl
from test_ref_zamboni import BUILDS, caps_tuple, profile_caps

CASES = sl.cases()
NAMES = [c.name for c in CASES]
GPU_BUILDS = [b for b in BUILDS if b[1] != "tiled"]  # the tiled profile has its own range op (range_op_tiled)
DCAP = 1 << 12


def _oracle(c, upto=None):
    o = oc.OracleClient(c.log.interner)
    o.start_collab(c.log.local_long_id)
    ops, text, props, kv = sl.batch([c]).doc(0)
    assert o.replay_arrays(ops if upto is None else ops[:upto], text, props, kv) == 0, c.name
    return o.dump(), o.digest()


@functools.lru_cache(maxsize=None)
def oracle_state():
    """(dump, digest) of every case on the oracle, once (shared, never changed)"""
    return [_oracle(c) for c in CASES]


def fitting(perm_only: bool):
    idx = [i for i, c in enumerate(CASES) if not perm_only or c.kind == "perm"]
    return idx, [CASES[i] for i in idx]


def test_every_listed_case_exists():
    stems = {n.rsplit("_", 1)[0] for n in NAMES}
    assert stems == {"onerow", "onerow_full", "sameleaf", "full_stay", "full_move", "full_both", "diffleaf",
                     "second_full_stays", "second_full_moves", "second_full_other", "parent_split", "parent_split_same",
                     "inv_removed", "inv_removed_leaves", "inv_pending", "inv_pending_full", "start_boundary",
                     "start_boundary_full", "end_boundary", "end_boundary_full", "local", "local_full", "replace",
                     "replace_local"}
    for c in CASES:
        assert c.name.rsplit("_", 1)[0] in sl.__doc__ and c.branch and len(c.log.ops) < 300, c.name
    assert sum(c.kind == "perm" for c in CASES) == len(stems)


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_shape_on_the_oracle(name):
    c = CASES[NAMES.index(name)]
    h0, s0 = ol.parse_dump(_oracle(c, c.cut)[0])
    h1, s1 = ol.parse_dump(oracle_state()[NAMES.index(name)][0])
    pre, post = sl.leaf_rows(s0), sl.leaf_rows(s1)
    print(name, pre, post)
    assert (h0["nleaf"], h1["nleaf"]) == c.nleaf
    assert {k: pre[k] for k in c.pre} == c.pre and {k: post[k] for k in c.post} == c.post
    idx = c.sel(h1, s1)
    print([sl.place(s1, i) for i in idx])
    assert len(idx) == c.ntouched
    if not name.startswith("inv_"):  # nothing invisible in between: the touched rows are consecutive
        assert idx == list(range(idx[0], idx[0] + len(idx)))
    assert (sl.place(s1, idx[0]), sl.place(s1, idx[-1])) == c.ends
    assert all(s["ngroups"] == 0 for s in s1)  # every local op was acked


@pytest.mark.parametrize("dcap", [0, DCAP], ids=["plain", "deltas"])
@pytest.mark.parametrize("profile", ["small", "matrix", "flat"])
def test_host_core_matches_the_oracle(profile, dcap):
    idx, cs = fitting(profile == "matrix")
    dig, err, st = core_host.replay_batch(sl.batch(cs), caps_tuple(profile_caps(profile)), dcap=dcap)
    assert (err == 0).all(), [(cs[i].name, st.error_op(int(i))) for i in np.nonzero(err)[0]]
    for k, d in enumerate(idx):
        assert int(dig[k]) == oracle_state()[d][1], f"{profile}: {cs[k].name}"
        assert st.dump(k) == oracle_state()[d][0], f"{profile}: {cs[k].name}"


def split_at_cut(cs):
    b = sl.batch(cs)
    head, tail = [], []
    for d, c in enumerate(cs):
        ops, text, props, kv = b.doc_arrays(d)
        head.append((ops[: c.cut], text, props, kv))
        tail.append((ops[c.cut:], text, props, kv))
    return ol.Batch.from_arrays(head, b.local_long_id), ol.Batch.from_arrays(tail, b.local_long_id)


def _check(eng, idx, cs, what):
    err, err_op = eng.errors()
    assert (err == 0).all(), (what, [(cs[i].name, int(err[i]), int(err_op[i])) for i in np.nonzero(err)[0]])
    assert len(eng.promoted()) == 0, what
    dig = eng.digests()
    bad = [cs[k].name for k, d in enumerate(idx) if int(dig[k]) != oracle_state()[d][1]]
    assert not bad, f"{what}: HIP engine differs from the oracle on {bad}"
    for k, d in enumerate(idx):
        assert eng.dump(k) == oracle_state()[d][0], f"{what}: {cs[k].name}"


@pytest.mark.gpu
@pytest.mark.parametrize("dcap", [0, DCAP], ids=["plain", "deltas"])
@pytest.mark.parametrize("build", GPU_BUILDS, ids=[b[0] for b in GPU_BUILDS])
def test_gpu_matches_the_oracle(build, dcap):
    """one submit, then a fresh engine with the batch cut before each document's range op; dcap > 0: the
    client-feature build, whose serial visit gets the carried slots too"""
    from fluidframework_amd.engine import Engine
    name, profile, variant, perm_only = build
    idx, cs = fitting(perm_only)
    b = sl.batch(cs)
    for parts in ([b], split_at_cut(cs)):
        eng = Engine(b.ndocs, **variant, **dict(profile_caps(profile), dcap=dcap))
        eng.start_collab(b.local_long_id)
        for p in parts:
            eng.replay(p)
        _check(eng, idx, cs, f"{name} dcap {dcap} in {len(parts)} submit(s)")
        eng.close()
