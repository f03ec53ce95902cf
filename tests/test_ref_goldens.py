"""Parity against the REFERENCE merge-tree itself (tests/golden/ref_*.npz).

The fixtures were produced by running the reference's own TypeScript (packages/dds/merge-tree/src,
type-erased offline by tools/ts_erase.py and replayed under node by tools/ref_replay.mjs; the
generating script is tools/make_ref_goldens.py) on logs from the in-repo generator, for every
config shape: the conflict farm (C1), observer replicas (C2), lagged editors with local-pending ops
and acks (C3, including the bench's 4,096-message length), coalescing-defeated long documents (C4
scaled) and PermutationSegment replicas (C5). Each fixture holds the reference's per-document
FNV-1a-64 digests of the canonical segment dump (text, lengths, seq/client/removal fields, overlap
lists, local seqs, pending-group counts, properties, LEAF-BLOCK ordinals) and, for the first few
documents, the full op logs and the reference's dumps.

CPU tier: the logs regenerate bit-identically (SHA-256), and the oracle and the host build of the
engine core reproduce every reference digest; the stored logs replay to the stored dumps byte for
byte. GPU tier: the HIP engine reproduces every reference digest.
"""
import dataclasses
import glob
import json
import os

import numpy as np
import pytest

from fluidframework_amd import gen
from fluidframework_amd import oplog as ol
import core_host
import oracle_client as oc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "ref_*.npz")))
NAMES = [os.path.basename(f)[4:-4] for f in FIXTURES]


def load(name):
    z = np.load(os.path.join(GOLDEN, f"ref_{name}.npz"), allow_pickle=False)
    w = gen.Workload(**json.loads(str(z["workload"])))
    return z, w


def regenerate(name):
    z, w = load(name)
    b = gen.generate(w, ids=z["doc_ids"], threads=8)
    return z, w, b


def caps_for(w: gen.Workload) -> dict:
    from fluidframework_amd.engine import default_caps
    if w.mode == gen.MTG_MATRIX:
        return default_caps(w.ops_per_doc, config=5)
    if w.distinct_props and w.ops_per_doc > 50_000:  # config 4 at scale: the tiled profile
        return default_caps(w.ops_per_doc, config=4)
    if w.distinct_props:  # config-4 shape: coalescing defeated, thousands of rows
        return dict(ncap=4096, hcap=8192, acap=1 << 17, mcap=4096, gcap=1024, ccap=64)
    return default_caps(w.ops_per_doc)


def _sha(b):
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "mrg", os.path.join(os.path.dirname(GOLDEN), "..", "tools", "make_ref_goldens.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.log_sha(b)


def test_fixture_set_complete():
    assert set(NAMES) >= {"c1_farm", "c2_observer", "c3_lagged", "c3_lagged_long", "c4_scaled", "c5_perm"}


@pytest.mark.parametrize("name", NAMES)
def test_oracle_and_host_core_match_reference(name):
    z, w, b = regenerate(name)
    assert _sha(b) == str(z["log_sha256"]), "generator no longer produces the fixture's op logs"
    assert (np.diff(b.op_off) == z["nevents"]).all()
    want = z["digests"]
    _, odig, oerr = oc.replay_batch(b, threads=8)
    assert (oerr == 0).all()
    bad = np.nonzero(odig != want)[0]
    assert len(bad) == 0, f"oracle differs from the reference on docs {bad[:8]}"
    c = caps_for(w)
    hdig, herr, _ = core_host.replay_batch(b, (c["ncap"], c["hcap"], c["acap"], c["mcap"], c["gcap"], c["ccap"]))
    assert (herr == 0).all()
    bad = np.nonzero(hdig != want)[0]
    assert len(bad) == 0, f"engine core (host build) differs from the reference on docs {bad[:8]}"


@pytest.mark.parametrize("name", NAMES)
def test_stored_logs_replay_to_reference_dumps(name):
    """The self-contained part of each fixture: stored op logs -> the reference's stored dumps."""
    z, w = load(name)
    props, kv = gen.props_table()
    n = len(z["keep_local"])
    off = z["keep_dump_off"]
    for d in range(n):
        ops = z["keep_ops"][z["keep_op_off"][d]: z["keep_op_off"][d + 1]]
        text = z["keep_text"][z["keep_text_off"][d]:]
        c = oc.OracleClient()
        c.start_collab(int(z["keep_local"][d]))
        c.replay_arrays(np.ascontiguousarray(ops), np.ascontiguousarray(text), props, kv)
        assert c.dump() == z["keep_dumps"][off[d]: off[d + 1]].tobytes(), f"doc {d}"


def kernel_variants(name):
    """The replay kernel builds a fixture's profile has (include/mt_engine.h mt_engine_set_variant): every one runs
    each fixture, whichever the engine would pick for the fixture's batch size. Config-2/3 profile: the LDS-image build
    (waves=1, mt_small_lds.hip), the 4-wave build (no spills) and the 8-wave build the config-3 bench runs; tiled profile (c4_large): the narrow LDS-heap kernel
    and the wide one; the other profiles have one build."""
    return variants_for(load(name)[1])


def variants_for(w):
    """kernel_variants for a workload (the fixtures of other families keep their own recipe)"""
    c = caps_for(w)
    if c["ncap"] <= 192 and w.mode != gen.MTG_MATRIX:
        return [dict(waves=1), dict(waves=4), dict(waves=8)]
    if c["ncap"] > 16384:
        return [dict(wide=False), dict(wide=True)]
    return [dict()]


VARIANT_CASES = [(n, v) for n in NAMES for v in kernel_variants(n)]


def variant_id(case):
    n, v = case
    return n + "".join(f"-{k}{int(x)}" for k, x in v.items())


@pytest.mark.gpu
@pytest.mark.parametrize("name,variant", VARIANT_CASES, ids=[variant_id(c) for c in VARIANT_CASES])
def test_gpu_engine_matches_reference(name, variant):
    from fluidframework_amd.engine import Engine
    z, w, b = regenerate(name)
    eng = Engine(b.ndocs, **variant, **caps_for(w))
    eng.start_collab(b.local_long_id)
    eng.replay(b)
    err, err_op = eng.errors()
    assert (err == 0).all(), (err[err != 0][:8], err_op[err != 0][:8])
    if variant.get("wide"):
        assert len(eng.promoted()) == 0
    gdig = eng.digests()
    bad = np.nonzero(gdig != z["digests"])[0]
    assert len(bad) == 0, f"HIP engine differs from the reference on docs {bad[:8]}"
    off = z["keep_dump_off"]
    for d in range(len(z["keep_local"])):
        assert eng.dump(d) == z["keep_dumps"][off[d]: off[d + 1]].tobytes()
