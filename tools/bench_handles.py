#!/usr/bin/env python3
"""Batched PermutationVector reads on a replayed batch against the single-document calls they stand beside.

Workload: config 5 (PermutationSegment rows), 4,096 documents x 1,500 ops with getAllocatedHandle records injected
(tests/handles_inject.py), replayed once. Timed, wall clock around the calls after a warm-up, median of `reps`:
  (1) handles:   every position of every document in one mt_engine_get_handles call (size query and fill), with the wave
                 form and the serial one (MT_VAR_HANDLES_PARALLEL), against the per-position mt_engine_get_handle loop;
  (2) positions: one handleToPosition per allocated handle of every document in one mt_engine_handles_to_positions call,
                 both forms, against the mt_engine_handle_to_position loop;
  (3) tables:    mt_engine_handle_tables for all documents against the per-document mt_engine_handle_table loop;
  (4) many queries per document: 64 handle ranges (and 64 handles) on each of 64 documents in one call: one wave per
                 query walks the document 64 times.
The single-call loops run over the first `--loop-docs` documents (one launch, one copy and one stream wait per
position is seconds for the whole batch) and are also given scaled to the batch by the position / handle count. The
answers of the loops and of both forms must be equal. With --trace DIR two more, separate steps run under `rocprofv3
--kernel-trace --stats` (tracing only), one workload each, so that a kernel's average is over launches of one size: the
whole-batch calls of (1) to (3) without the loops (DIR/batch), and the 64 x 64 calls of (4) alone (DIR/many, its kernel
times prefixed many_); the average kernel times join the JSON line.

    timeout 900 python tools/bench_handles.py --trace /tmp/handles_trace --out profiles/batched_handles.json
"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from fluidframework_amd import gen  # noqa: E402
from fluidframework_amd.engine import Engine, MT_VAR_HANDLES_PARALLEL, default_caps  # noqa: E402
from bench_dumps import median_ms, step  # noqa: E402

PCAP = 1 << 14
NONE = -(1 << 31)


def measure(a):
    import handles_inject
    caps = default_caps(a.ops, config=5)
    g = gen.generate(gen.config5(a.ops), a.docs)
    b = handles_inject.inject(g, tuple(caps[k] for k in ("ncap", "hcap", "acap", "mcap", "gcap", "ccap")))
    eng = Engine(b.ndocs, **dict(caps, pcap=PCAP))
    eng.start_collab(b.local_long_id)
    eng.replay(b)
    assert (eng.errors()[0] == 0).all()
    n, k = b.ndocs, min(a.loop_docs, b.ndocs)
    L = np.ascontiguousarray(eng.get_lengths()[0], np.int32)
    zero = np.zeros(n, np.int32)
    res = {"bench": "batched_handles", "config": 5, "docs": n, "ops_per_doc": a.ops, "positions": int(L.sum()),
           "loop_docs": k, "reps": a.reps}
    loops = a.parts == "all"
    if a.parts == "many":  # the 64 x 64 calls alone: the allocated handles come from the tables, read one by one
        nd = min(64, n)
        held = [np.nonzero(eng.handle_table(d)[1:] == 0)[0].astype(np.int32) + 1 for d in range(nd)]
        docs = np.repeat(np.arange(nd, dtype=np.int64), [len(h) for h in held])
        hs = np.ascontiguousarray(np.concatenate(held))
        many(eng, a, res, L, docs, hs, np.zeros(len(hs), np.int32))
        print(json.dumps(res), flush=True)
        eng.close()
        return 0

    # (1) the handles of every position
    got = {}
    for name, v in (("wave", 1), ("serial", 0)):
        eng.set_variant(MT_VAR_HANDLES_PARALLEL, v)
        res[f"get_handles_{name}_ms"] = round(median_ms(lambda: got.__setitem__(name, eng.get_handles(zero, L)), a.reps), 3)
    off, st, hd = got["wave"]
    assert not st.any() and (got["serial"][2] == hd).all() and (got["serial"][0] == off).all()
    if loops:
        loop = []
        t = median_ms(lambda: loop.__setitem__(slice(None), [eng.get_handle(d, p) for d in range(k) for p in range(L[d])]), 1)
        assert (np.asarray(loop, np.int32) == hd[: off[k]]).all(), "the batched handles differ from the get_handle loop"
        res["get_handle_loop_ms"] = round(t, 3)
        res["get_handle_loop_positions"] = int(off[k])
        res["get_handle_loop_scaled_ms"] = round(t * float(L.sum()) / max(int(off[k]), 1), 1)

    # (2) one handleToPosition per allocated handle
    docs = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))[hd != NONE]
    hs = np.ascontiguousarray(hd[hd != NONE])
    res["allocated_handles"] = int(len(hs))
    ls0 = np.zeros(len(hs), np.int32)  # localSeq 0: never past a replica's own, whatever it has pending
    got = {}
    for name, v in (("wave", 1), ("serial", 0)):
        eng.set_variant(MT_VAR_HANDLES_PARALLEL, v)
        res[f"handles_to_positions_{name}_ms"] = round(
            median_ms(lambda: got.__setitem__(name, eng.handles_to_positions(hs, ls0, docs)), a.reps), 3)
    pos, pst = got["wave"]
    assert not pst.any() and (got["serial"][0] == pos).all()
    if loops:
        m = int((docs < k).sum())
        loop = []
        t = median_ms(lambda: loop.__setitem__(slice(None), [eng.handle_to_position(int(docs[i]), int(hs[i]), 0)
                                                              for i in range(m)]), 1)
        assert (np.asarray(loop, np.int32) == pos[:m]).all(), "the batched positions differ from the single calls"
        res["handle_to_position_loop_ms"] = round(t, 3)
        res["handle_to_position_loop_handles"] = m
        res["handle_to_position_loop_scaled_ms"] = round(t * len(hs) / max(m, 1), 1)

    # (3) the handle tables
    eng.set_variant(MT_VAR_HANDLES_PARALLEL, 1)
    tabs = {}
    res["handle_tables_ms"] = round(median_ms(lambda: tabs.__setitem__("b", eng.handle_tables()), a.reps), 3)
    if loops:
        one = []
        res["handle_table_loop_ms"] = round(
            median_ms(lambda: one.__setitem__(slice(None), [eng.handle_table(d) for d in range(n)]), a.reps), 3)
        assert (np.concatenate(one) == tabs["b"][1]).all()
        many(eng, a, res, L, docs, hs, ls0)
    print(json.dumps(res), flush=True)
    eng.close()
    return 0


def many(eng, a, res, L, docs, hs, ls0):
    """(4) 64 queries on each of 64 documents"""
    n = len(L)
    nd = min(64, n)
    qd = np.repeat(np.arange(nd, dtype=np.int64), 64)
    qa = np.ascontiguousarray((np.tile(np.arange(64), nd) * L[qd] // 64).astype(np.int32))
    qb = np.ascontiguousarray(np.minimum(qa + 32, L[qd]).astype(np.int32))
    for name, v in (("wave", 1), ("serial", 0)):
        eng.set_variant(MT_VAR_HANDLES_PARALLEL, v)
        res[f"many_64x64_get_handles_{name}_ms"] = round(median_ms(lambda: eng.get_handles(qa, qb, qd), a.reps), 3)
        sel = np.nonzero(docs < nd)[0][: 64 * nd]
        res[f"many_64x64_positions_{name}_ms"] = round(
            median_ms(lambda: eng.handles_to_positions(hs[sel], ls0[sel], docs[sel]), a.reps), 3)
    eng.set_variant(MT_VAR_HANDLES_PARALLEL, 1)


def kernel_times(trace_dir, prefix=""):
    """average microseconds per launch of the new kernels (both forms) and of k_seg in a rocprofv3 --stats directory"""
    out = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            nm = row["Name"]
            par = nm.split(">(")[0].rstrip().endswith("true")
            for kern in ("k_handles", "k_handle_positions"):
                if kern + "<" in nm:
                    field = f"{kern}_{'wave' if par else 'serial'}_us"
                    break
            else:
                for kern in ("k_handle_sizes", "k_handle_table_sizes", "k_handle_tables"):
                    if kern + "<" in nm:
                        field = kern + "_us"
                        break
                else:
                    continue
            out[prefix + field] = round(float(row["AverageNs"]) / 1e3, 3)
            out[prefix + field.replace("_us", "_calls")] = int(row["Calls"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=4096)
    ap.add_argument("--ops", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-docs", type=int, default=64, help="documents the single-call loops run over")
    ap.add_argument("--step", choices=["measure"])
    ap.add_argument("--parts", choices=["all", "batch", "many"], default="all",
                    help="batch: the whole-batch calls without the loops; many: the 64 x 64 calls alone (the traced steps)")
    ap.add_argument("--trace", help="a directory for a separate rocprofv3 --kernel-trace --stats run")
    ap.add_argument("--limit", type=int, default=420, help="seconds allowed to each GPU step")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.step == "measure":
        return measure(a)
    me = [sys.executable, os.path.abspath(__file__), "--step", "measure", "--docs", str(a.docs), "--ops", str(a.ops),
          "--loop-docs", str(a.loop_docs)]
    line = step(me + ["--reps", str(a.reps)], a.limit)
    if not line:
        return 2
    res = json.loads(line)
    if a.trace:  # stops here if a step failed; each traced run is a process of its own, one workload each
        for parts, prefix in (("batch", ""), ("many", "many_")):
            d = os.path.join(a.trace, parts)
            os.makedirs(d, exist_ok=True)
            traced = step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + me +
                          ["--reps", "2", "--parts", parts], a.limit)
            if traced is None:
                return 3
            res.update(kernel_times(d, prefix))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
