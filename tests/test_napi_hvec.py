"""The PermutationVector read fixture through node: every handle range and handleToPosition query of
tests/golden/refhvec.npz (the reference's answers on the hand-built logs of tests/hvec_logs.py) and every handle table,
asked through fluidframework_amd/js/mergetree_gpu.js -> mt_napi.node -> mt_engine_get_handles /
mt_engine_handles_to_positions / mt_engine_handle_tables on the GPU, batched (ReplayEngine.getHandles /
handlesToPositions / handleTables) and per client (GpuClient.getHandles, getMaybeHandle position by position,
handleToPosition, handleTable), on engines of the small, matrix and tiled capacities (the small one promotes x_promote).
The logs and queries are exported at test time; tests/napi_hvec.js replays them. No query is left out: where the
reference throws, the batched answer is undefined and the client's call throws."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from fluidframework_amd import native
import hvec_logs as hl
from test_ref_hvec import CASES, NAMES, expected, ref_dump
from test_ref_zamboni import profile_caps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")
RUNS = ("small", "matrix", "tiled")
NEW = ("getHandles", "handlesToPositions", "handleTables")


def test_addon_exports_the_matrix_reads():
    addon = native.build_napi()
    r = subprocess.run([NODE, "-e", f"console.log(Object.keys(require({json.dumps(addon)})).join())"],
                       capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr
    assert set(NEW) <= set(r.stdout.strip().split(","))


def test_facade_and_typings_declare_the_matrix_reads():
    js = open(os.path.join(ROOT, "fluidframework_amd", "js", "mergetree_gpu.js")).read()
    dts = open(os.path.join(ROOT, "fluidframework_amd", "js", "mergetree_gpu.d.ts")).read()
    for name in NEW:
        assert re.search(rf"^    {name}\(", js, re.M) and re.search(rf"^    {name}\(", dts, re.M), name
    assert len(re.findall(r"^    getHandles\(", js, re.M)) == 2 == len(re.findall(r"^    getHandles\(", dts, re.M))


def _export(tmp):
    """the logs as raw arrays and the fixture's queries, once per run (every case fits every profile)"""
    rq, hq, _ = expected()
    b = hl.batch(CASES)
    runs = []
    for name in RUNS:
        d = os.path.join(tmp, name)
        os.makedirs(d)
        for f, a, t in (("ops", b.ops, None), ("op_off", b.op_off, "<i8"), ("text", b.text, "<u2"),
                        ("text_off", b.text_off, "<i8"), ("props", b.props, None), ("props_off", b.props_off, "<i8"),
                        ("kv", b.kv, None), ("kv_off", b.kv_off, "<i8")):
            (a if t is None else np.asarray(a).astype(t)).tofile(os.path.join(d, f + ".bin"))
        runs.append(dict(name=name, ndocs=b.ndocs, caps=dict(profile_caps(name), pcap=hl.PCAP),
                         local=[int(x) for x in b.local_long_id], ranges=[list(q[:3]) for q in rq],
                         positions=[list(q[:3]) for q in hq]))
    with open(os.path.join(tmp, "meta.json"), "w") as f:
        json.dump(dict(runs=runs), f)
    return runs


@pytest.mark.gpu
def test_fixture_queries_through_node(tmp_path):
    native.build_napi()
    runs = _export(str(tmp_path))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "napi_hvec.js"), str(tmp_path)], capture_output=True,
                       text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    rq, hq, tables = expected()
    lengths = [ref_dump(d)[0]["length"] for d in range(len(CASES))]
    for run in runs:
        o = out[run["name"]]
        assert not any(o["errors"]), (run["name"], o["errors"])
        assert len(o["ranges"]) == len(o["clientRanges"]) == len(rq) > 300
        assert len(o["positions"]) == len(o["clientPositions"]) == len(hq) > 250
        assert [len(v) for v in o["single"]] == lengths
        for q, a, c in zip(rq, o["ranges"], o["clientRanges"]):
            what = (run["name"], NAMES[q[0]], q[1:3])
            if q[3] is None:
                assert a is None and c is None, what
                continue
            assert a == c == [int(x) for x in q[3]] == o["single"][q[0]][q[1]: q[2]], what
        for q, a, c in zip(hq, o["positions"], o["clientPositions"]):
            assert a == c == q[3], (run["name"], NAMES[q[0]], q[1:3])
        want = [[int(x) for x in t] for t in tables]
        assert o["tables"] == o["clientTables"] == want, run["name"]
        assert o["someTables"] == [want[-1], want[0], want[-1]], run["name"]
