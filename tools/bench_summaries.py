#!/usr/bin/env python3
"""Summarizing a replayed batch: batched dumps + extraction in Python against extraction on the device.

Workload: config 3, 4,096 documents x 512 ops, replayed once (the workload of tools/bench_dumps.py). Timed, wall clock
around the calls after a warm-up, median of 5:
  (a) snapshot.emit_batch on the dump path (Engine.dumps, then extract_segments per row in Python) against
      snapshot.emit_batch(device=True) (Engine.summaries: the segments extracted by k_summaries), under each writer
      (MT_VAR_SUMMARIES_PARALLEL); the trees must be equal;
  (b) the C calls alone into preallocated buffers: mt_engine_dumps, and mt_engine_summaries under each writer, with the
      size query's time beside it; the two writers' bytes must be equal;
  (c) summary bytes against dump bytes.
Prints one JSON line; --out appends it to a file.

This process starts no GPU work itself: every GPU step is a child process under its own `timeout -k 10`. With --trace
DIR a second, separate step runs the same measurement under `rocprofv3 --kernel-trace --stats` (tracing only) and the
kernels' average times join the JSON line: k_summary_sizes, k_summaries<true>, k_summaries<false>, and k_dumps beside
them. The lane-parallel writer is the default only while k_summaries<true> beats k_summaries<false> there.

    python tools/bench_summaries.py --trace /tmp/summaries_trace --out profiles/batched_summaries.json
"""
import argparse
import csv
import ctypes
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_dumps import median_ms, step  # noqa: E402


def long_name(i):
    return f"c{i}" if i >= 0 else "original"


def measure(a):
    import numpy as np

    from fluidframework_amd import gen, snapshot
    from fluidframework_amd.engine import Engine, MT_VAR_SUMMARIES_PARALLEL, default_caps

    b = gen.generate(gen.config3(a.ops), a.docs)
    eng = Engine(b.ndocs, **default_caps(a.ops))
    eng.start_collab(b.local_long_id)
    eng.replay(b)
    assert (eng.errors()[0] == 0).all()
    n = b.ndocs
    it = gen.generator_interner()
    vp = ctypes.c_void_p

    host = []

    def run_host():
        host[:] = snapshot.emit_batch(eng, None, it, long_name)
    t_host = median_ms(run_host, a.reps)

    off = np.zeros(n + 1, np.int64)
    dump_total = eng.L.mt_engine_dumps(eng.h, n, None, off.ctypes.data_as(vp), None, 0)
    dbuf = np.zeros(dump_total + 1, np.uint8)
    t_dumps_call = median_ms(lambda: eng.L.mt_engine_dumps(eng.h, n, None, off.ctypes.data_as(vp),
                                                           dbuf.ctypes.data_as(vp), dump_total), a.reps)
    total = eng.L.mt_engine_summaries(eng.h, n, None, 0, off.ctypes.data_as(vp), None, 0)
    buf = np.zeros(total + 1, np.uint8)

    def size_only():
        assert eng.L.mt_engine_summaries(eng.h, n, None, 0, off.ctypes.data_as(vp), None, 0) == total

    def fill():
        assert eng.L.mt_engine_summaries(eng.h, n, None, 0, off.ctypes.data_as(vp), buf.ctypes.data_as(vp), total) == total
    t_size = median_ms(size_only, a.reps)

    dev, call, raw = {}, {}, {}
    got = []

    def run_dev():
        got[:] = snapshot.emit_batch(eng, None, it, long_name, device=True)
    for name, v in (("parallel", 1), ("serial", 0)):
        eng.set_variant(MT_VAR_SUMMARIES_PARALLEL, v)
        dev[name] = median_ms(run_dev, a.reps)
        assert got == host, f"emit_batch(device=True) ({name} writer) differs from the dump path"
        buf[:] = 0
        call[name] = median_ms(fill, a.reps)
        raw[name] = buf[:total].tobytes()
    assert raw["parallel"] == raw["serial"], "the two writers' bytes differ"
    res = {"bench": "batched_summaries", "config": 3, "docs": n, "ops_per_doc": a.ops, "dump_bytes": int(dump_total),
           "summary_bytes": int(total), "bytes_ratio": round(total / dump_total, 4),
           "emit_batch_dumps_ms": round(t_host, 3), "emit_batch_device_parallel_ms": round(dev["parallel"], 3),
           "emit_batch_device_serial_ms": round(dev["serial"], 3),
           "speedup_parallel": round(t_host / dev["parallel"], 2), "speedup_serial": round(t_host / dev["serial"], 2),
           "dumps_call_ms": round(t_dumps_call, 3), "summaries_size_query_ms": round(t_size, 3),
           "summaries_call_parallel_ms": round(call["parallel"], 3),
           "summaries_call_serial_ms": round(call["serial"], 3), "reps": a.reps}
    print(json.dumps(res), flush=True)
    eng.close()
    return 0


def kernel_times(trace_dir):
    """average microseconds per launch of the summary kernels (and k_dumps) in a rocprofv3 --stats directory"""
    out = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            nm = row["Name"]
            par = nm.split(">(")[0].rstrip().endswith("true")
            if "k_summary_sizes" in nm:
                field = "k_summary_sizes_us"
            elif "k_summaries<" in nm:
                field = "k_summaries_parallel_us" if par else "k_summaries_serial_us"
            elif "k_dumps<" in nm:
                field = "k_dumps_parallel_us" if par else "k_dumps_serial_us"
            elif "k_dump_sizes" in nm:
                field = "k_dump_sizes_us"
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
