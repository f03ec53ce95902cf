#!/usr/bin/env python3
"""Marker queries on a replayed batch: the per-document dump walk against one batched find_tiles call.

Workload: config 3, 4,096 documents x 512 ops, in which every second one-unit text insert of a remote client is a
marker (tests/text_markers.py) and every marker carries referenceTileLabels ["pg"]; the markers' refTypes alternate
Simple / Tile, so half of them are paragraph tiles; the generator's rewrite annotates are made plain ones (a rewrite
over a marker deletes its label, and the engine then refuses the document); a document whose log the substitution
makes invalid keeps its marker-free log. Replayed once. The query per document: findTile(length // 2, "pg", preceding). Timed, wall clock around the calls after a warm-up, median of 5:
  (a) loop:      dump(d) for every document (what GpuClient.findTile read before: two launches and two stream waits
                 each), alone, and with the host's decode and walk of the records (Python here);
  (b) batched:   one mt_engine_find_tiles call for all documents, with the wave forms and with the serial ones
                 (MT_VAR_TILES_PARALLEL), into preallocated arrays; and Engine.find_tiles, which also builds the label set.
The answers of (a) and of (b) under both settings must be equal. With --trace DIR a second, separate step runs the same
measurement under `rocprofv3 --kernel-trace --stats` (tracing only) and the average kernel times join the JSON line.

    timeout 900 python tools/bench_tiles.py --trace /tmp/tiles_trace --out profiles/batched_tiles.json
"""
import argparse
import csv
import ctypes
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from fluidframework_amd import gen  # noqa: E402
from fluidframework_amd import oplog as ol  # noqa: E402
from fluidframework_amd.engine import Engine, MT_VAR_TILES_PARALLEL, default_caps  # noqa: E402
from bench_dumps import median_ms, step  # noqa: E402

LABEL = "pg"


def workload(ndocs, nops):
    """the batch and its interner: config 3 with markers, every marker labelled (one shared property record)"""
    import core_host
    import text_markers
    g = gen.generate(gen.config3(nops), ndocs)
    b = text_markers.with_markers(g)
    # a marker cannot be split, so the substitution can make a later insert of the log invalid (the oracle and the host
    # core both reject such a log): those documents, found by a host replay, keep their marker-free logs
    caps = default_caps(nops)
    _, err, _ = core_host.replay_batch(b, tuple(caps[k] for k in ("ncap", "hcap", "acap", "mcap", "gcap", "ccap")))
    ops = b.ops.copy()
    for d in np.nonzero(err)[0]:
        ops[b.op_off[d]: b.op_off[d + 1]] = g.ops[g.op_off[d]: g.op_off[d + 1]]
    b = ol.Batch(ops=ops, op_off=b.op_off, text=b.text, text_off=b.text_off, props=b.props, props_off=b.props_off,
                 kv=b.kv, kv_off=b.kv_off, local_long_id=b.local_long_id)
    it = gen.generator_interner()
    assert np.all(b.props_off == b.props_off[0]) and np.all(b.kv_off == b.kv_off[0]), "the generator shares its pools"
    p0, k0 = int(b.props_off[0]), int(b.kv_off[0])
    kv = np.concatenate([b.kv, np.array([(it.key(ol.TILE_LABELS_KEY), it.value([LABEL]))], ol.KV_DTYPE)])
    props = np.concatenate([b.props, np.array([(len(b.kv) - k0, 1, ol.COMBINE_NONE, 0)], ol.PROPS_DTYPE)])
    # a rewrite annotate over a marker deletes its label and makes the engine refuse the document's tile queries
    # (mkMask): the workload's rewrites become plain annotates (lengths and positions are unchanged)
    props["combining"][props["combining"] == ol.COMBINE_REWRITE] = ol.COMBINE_NONE
    ops = b.ops.copy()
    ops["props"][ops["seg_kind"] == ol.SEG_MARKER] = len(b.props) - p0 + 1  # 1-based
    return ol.Batch(ops=ops, op_off=b.op_off, text=b.text, text_off=b.text_off, props=props, props_off=b.props_off,
                    kv=kv, kv_off=b.kv_off, local_long_id=b.local_long_id), it


def walk(segs, pos, key, values):
    """the facade's findTile(pos, label, preceding = true) over a parsed dump: (ordinal, position) or None"""
    P, best = 0, None
    for i, s in enumerate(segs):
        v = s["len"] if s["removedSeq"] is None else 0
        tile = (s["kind"] == ol.SEG_MARKER and s["refType"] & ol.REF_TILE
                and any(k == key and (x & 0x7FFF) in values for k, x in s["props"]))
        if v > 0 and P <= pos < P + v:
            return (i, P) if tile else best
        if v > 0 and tile:
            best = (i, P)
        P += v
    return best


def measure(a):
    b, it = workload(a.docs, a.ops)
    eng = Engine(b.ndocs, **default_caps(a.ops))
    eng.start_collab(b.local_long_id)
    eng.replay(b)
    assert (eng.errors()[0] == 0).all()
    n = b.ndocs
    pos = np.ascontiguousarray(eng.get_lengths()[0] // 2, np.int32)
    key = it.key_ids[ol.TILE_LABELS_KEY]
    bits = np.ascontiguousarray(it.values_containing(LABEL))
    values = {32 * w + k for w in np.nonzero(bits)[0] for k in range(32) if (int(bits[w]) >> k) & 1}
    dumps, loop = [], []

    def run_dumps():
        dumps[:] = [eng.dump(d) for d in range(n)]

    def run_walks():
        loop[:] = [walk(ol.parse_dump(x)[1], int(pos[d]), key, values) for d, x in enumerate(dumps)]

    t_dumps = median_ms(run_dumps, a.reps)
    t_walks = median_ms(run_walks, 1)  # the host's share: Python here, measured once
    vp = ctypes.c_void_p
    out, st = np.zeros(n, ol.TILE_REF), np.zeros(n, np.int32)
    pre = np.ones(n, np.int32)

    def call():
        rc = eng.L.mt_engine_find_tiles(eng.h, n, None, pos.ctypes.data_as(vp), pre.ctypes.data_as(vp), key,
                                        bits.ctypes.data_as(vp), out.ctypes.data_as(vp), st.ctypes.data_as(vp))
        assert rc == 0

    calls, answers = {}, {}
    for name, v in (("wave", 1), ("serial", 0)):
        eng.set_variant(MT_VAR_TILES_PARALLEL, v)
        out[:] = 0
        calls[name] = median_ms(call, a.reps)
        assert not st.any()
        answers[name] = [(int(t["ordinal"]), int(t["pos"])) if t["rid"] >= 0 else None for t in out]
    assert answers["wave"] == answers["serial"] == loop, "the batched answers differ from the dump walk"
    eng.set_variant(MT_VAR_TILES_PARALLEL, 1)
    t_py = median_ms(lambda: eng.find_tiles(LABEL, None, pos, True, interner=it), a.reps)
    res = {"bench": "batched_tiles", "config": 3, "docs": n, "ops_per_doc": a.ops,
           "markers": int((b.ops["seg_kind"] == ol.SEG_MARKER).sum()), "found": sum(x is not None for x in loop),
           "dump_loop_ms": round(t_dumps, 3), "host_decode_walk_ms": round(t_walks, 3),
           "find_tiles_call_wave_ms": round(calls["wave"], 3), "find_tiles_call_serial_ms": round(calls["serial"], 3),
           "engine_find_tiles_ms": round(t_py, 3), "dump_loop_over_call_wave": round(t_dumps / calls["wave"], 1),
           "dump_loop_over_call_serial": round(t_dumps / calls["serial"], 1), "reps": a.reps}
    print(json.dumps(res), flush=True)
    eng.close()
    return 0


def kernel_times(trace_dir):
    """average microseconds per launch of k_find_tiles (both forms) and k_dump in a rocprofv3 --stats directory"""
    out = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            nm = row["Name"]
            par = nm.split(">(")[0].rstrip().endswith("true")
            if "k_find_tiles<" in nm:
                field = "k_find_tiles_wave_us" if par else "k_find_tiles_serial_us"
            elif "k_dump<" in nm:
                field = "k_dump_us"
            else:
                continue
            out[field] = round(float(row["AverageNs"]) / 1e3, 3)
            out[field.replace("_us", "_calls")] = int(row["Calls"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=4096)
    ap.add_argument("--ops", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step", choices=["measure"])
    ap.add_argument("--trace", help="a directory for a separate rocprofv3 --kernel-trace --stats run")
    ap.add_argument("--limit", type=int, default=420, help="seconds allowed to each GPU step")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.step == "measure":
        return measure(a)
    me = [sys.executable, os.path.abspath(__file__), "--step", "measure", "--docs", str(a.docs), "--ops", str(a.ops)]
    line = step(me + ["--reps", str(a.reps)], a.limit)
    if not line:
        return 2
    res = json.loads(line)
    if a.trace:  # stops here if the first step failed; the traced run is a process of its own
        os.makedirs(a.trace, exist_ok=True)
        traced = step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.trace, "--"] + me +
                      ["--reps", str(a.reps)], a.limit)
        if traced is None:
            return 3
        res.update(kernel_times(a.trace))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
