"""The batched reads through node: ReplayEngine.getTexts() / getLengths() (fluidframework_amd/js/mergetree_gpu.js ->
mt_napi.node getTexts / getLengths -> mt_engine_get_texts / mt_engine_get_lengths) against each GpuClient's own
getText() / getLength(), and the addon's adjustPositions against adjustPosition."""
import json
import os
import shutil
import subprocess

import pytest

from fluidframework_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")

SCRIPT = r"""
const f = require('./fluidframework_amd/js/mergetree_gpu.js');
const eng = new f.ReplayEngine(4);
const c = [0, 1, 2, 3].map((d) => eng.client(d));
c[0].insertTextLocal(0, "hello world");
c[1].insertTextLocal(0, "abc");
c[3].insertTextLocal(0, "0123456789".repeat(20));   // document 2 stays empty
eng.startCollaboration(["u", "u", "u", "u"]);
c[0].insertTextLocal(5, ",");
c[1].removeRangeLocal(1, 2);
c[3].applyMsg({ clientId: "B", sequenceNumber: 1, referenceSequenceNumber: 0, minimumSequenceNumber: 0,
    type: "op", contents: { type: 0, pos1: 7, seg: "xyz" } });
const out = { texts: eng.getTexts(), each: c.map((x) => x.getText()), lengths: Array.from(eng.getLengths()),
    eachLength: c.map((x) => x.getLength()), some: eng.getTexts([3, 0, 3]) };
const addon = require(process.argv[1]);
const b = eng.longIndex("B");
const pos = [0, 7, 8, 300];
out.adjust = Array.from(addon.adjustPositions(eng.h, pos.map(() => 3), Int32Array.from(pos),
    Int32Array.from(pos.map(() => 1)), Int32Array.from(pos.map(() => b)))[0]);
out.adjustEach = pos.map((p) => { const v = addon.adjustPosition(eng.h, 3, p, 1, b); return v === undefined ? -1 : v; });
console.log(JSON.stringify(out));
"""


def test_addon_exports_the_batched_reads():
    addon = native.build_napi()
    r = subprocess.run([NODE, "-e", f"console.log(Object.keys(require({json.dumps(addon)})).join())"],
                       capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr
    assert {"getLengths", "getTexts", "adjustPositions"} <= set(r.stdout.strip().split(","))


@pytest.mark.gpu
def test_replay_engine_get_texts_through_node():
    addon = native.build_napi()
    r = subprocess.run([NODE, "-e", SCRIPT, addon], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["texts"] == out["each"] and out["each"][0] == "hello, world" and out["each"][2] == ""
    assert out["lengths"] == out["eachLength"] == [len(t) for t in out["each"]]
    assert out["some"] == [out["each"][3], out["each"][0], out["each"][3]]
    assert out["adjust"] == out["adjustEach"] and out["adjust"][0] == 0 and out["adjust"][-1] == -1
