"""The batched delta-event read through node (addon.deltasBatch, ReplayEngine.deltaEvents; tests/napi_deltas.js).

CPU tier: the addon exports deltasBatch and the facade deltaEvents / DELTA_KINDS. GPU tier: over a handful of documents
the batched answers equal the per-document GpuClient.deltaEvents() of the same engine, whole, one kind at a time and
from a cursor."""
import json
import os
import shutil
import subprocess

import pytest

from fluidframework_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
SEQUENCE = ("INSERT", "REMOVE", "ANNOTATE", "REGEN")


def test_addon_and_facade_export_the_batched_read():
    addon = native.build_napi()
    r = subprocess.run([NODE, "-e", f"const a = require({json.dumps(addon)}); "
                        "const f = require('./fluidframework_amd/js/mergetree_gpu.js'); "
                        "console.log(JSON.stringify([typeof a.deltasBatch, typeof f.ReplayEngine.prototype.deltaEvents, "
                        "f.DELTA_KINDS]))"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout) == ["function", "function", {"SEQUENCE": 1, "MAINTENANCE": 2}]


@pytest.mark.gpu
def test_batched_delta_events_through_node():
    native.build_napi()
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "napi_deltas.js")], capture_output=True, text=True,
                       cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    single = out["single"]
    assert len(single) == 5 and single[4] == [] and all(single[d] for d in range(4))
    for d in range(4):  # the scenario has both kinds of event in every document
        ops = [e["operation"] for e in single[d]]
        assert {"INSERT", "ANNOTATE", "REMOVE", "SPLIT"} <= set(ops), (d, ops)
    assert out["batch"] == single
    assert out["listed"] == [single[3], single[1], single[3], single[4]]
    assert out["sequence"] == [[e for e in ev if e["operation"] in SEQUENCE] for ev in single]
    assert out["maintenance"] == [[e for e in ev if e["operation"] not in SEQUENCE] for ev in single]
    raw = out["raw"]
    assert raw["events"] == [single[2], single[0]] and raw["status"] == [0, 0]
    assert raw["off"][0] == 0 and raw["off"][2] == raw["nwords"] and raw["end"] == raw["emitted"]
    assert raw["end"] == [raw["off"][1], raw["off"][2] - raw["off"][1]]
    # from the cursor: exactly the events the later messages fired; the cursor inside an event is refused alone
    after = out["after"]
    assert out["tail"]["status"] == [0, 0, 16]  # MT_E_ARG
    for i in range(2):
        n = len(raw["events"][i])
        assert after[i][:n] == raw["events"][i] and len(after[i]) > n
        assert out["tail"]["events"][i] == after[i][n:]
    assert out["tail"]["events"][2] == []
    assert "mt_engine_deltas_batch" in out["kinds0"] and "mt_engine_deltas_batch" in out["nodcap"]
