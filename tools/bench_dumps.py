#!/usr/bin/env python3
"""Dumping a replayed batch: the per-document loop against the batched dump.

Workload: config 3, 4,096 documents x 512 ops, replayed once (the workload of tools/bench_reads.py). Timed, wall
clock around the calls after a warm-up, median of 5:
  (a) loop:    dump(d) for every document (a size launch and a fill launch of one workgroup, two stream waits each);
  (b) batched: one dumps() (mt_engine_dumps: one size launch and one fill launch for all documents), under each writer
      (MT_VAR_DUMPS_PARALLEL: the lane-parallel writer and the serial one);
and the C call alone into a preallocated buffer under each writer, with the size query's time beside it. The loop and
both batched calls must give the same bytes. Prints one JSON line; --out appends it to a file.

This process starts no GPU work itself: every GPU step is a child process under its own `timeout -k 10`. The first is
the measurement (this file with --step measure). With --trace DIR a second, separate step runs the same measurement
under `rocprofv3 --kernel-trace --stats` (tracing slows the host, so the wall-clock figures come from the first step
only) and the kernels' average times join the JSON line: k_dump_sizes, k_dumps<true>, k_dumps<false> and the loop's
k_dump.

    python tools/bench_dumps.py --trace /tmp/dumps_trace --out profiles/batched_dumps.json
"""
import argparse
import csv
import ctypes
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(f, reps):
    f()  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def measure(a):
    import numpy as np

    from fluidframework_amd import gen
    from fluidframework_amd.engine import Engine, MT_VAR_DUMPS_PARALLEL, default_caps

    b = gen.generate(gen.config3(a.ops), a.docs)
    eng = Engine(b.ndocs, **default_caps(a.ops))
    eng.start_collab(b.local_long_id)
    eng.replay(b)
    assert (eng.errors()[0] == 0).all()
    n = b.ndocs

    loop = []

    def run_loop():
        loop[:] = [eng.dump(d) for d in range(n)]
    t_loop = median_ms(run_loop, a.reps)

    # the C call alone: the size query, and the whole call into a preallocated buffer
    off = np.zeros(n + 1, np.int64)
    vp = ctypes.c_void_p
    total = eng.L.mt_engine_dumps(eng.h, n, None, off.ctypes.data_as(vp), None, 0)
    assert total == sum(len(x) for x in loop)
    buf = np.zeros(total + 1, np.uint8)

    def size_only():
        assert eng.L.mt_engine_dumps(eng.h, n, None, off.ctypes.data_as(vp), None, 0) == total

    def fill():
        assert eng.L.mt_engine_dumps(eng.h, n, None, off.ctypes.data_as(vp), buf.ctypes.data_as(vp), total) == total
    t_size = median_ms(size_only, a.reps)

    batched, call = {}, {}
    got = []

    def run_batched():
        got[:] = eng.dumps()
    for name, v in (("parallel", 1), ("serial", 0)):
        eng.set_variant(MT_VAR_DUMPS_PARALLEL, v)
        batched[name] = median_ms(run_batched, a.reps)
        assert got == loop, f"the batched dump ({name} writer) differs from the loop"
        buf[:] = 0
        call[name] = median_ms(fill, a.reps)
        assert buf[:total].tobytes() == b"".join(loop), f"the {name} writer's bytes differ from the loop's"
    res = {"bench": "batched_dumps", "config": 3, "docs": n, "ops_per_doc": a.ops, "dump_bytes": int(total),
           "loop_ms": round(t_loop, 3), "batched_parallel_ms": round(batched["parallel"], 3),
           "batched_serial_ms": round(batched["serial"], 3),
           "speedup_parallel": round(t_loop / batched["parallel"], 2),
           "speedup_serial": round(t_loop / batched["serial"], 2), "dumps_size_query_ms": round(t_size, 3),
           "dumps_call_parallel_ms": round(call["parallel"], 3), "dumps_call_serial_ms": round(call["serial"], 3),
           "reps": a.reps}
    print(json.dumps(res), flush=True)
    eng.close()
    return 0


def kernel_times(trace_dir):
    """average microseconds per launch of the dump kernels in a rocprofv3 --stats directory"""
    out = {}
    names = (("k_dump_sizes", "k_dump_sizes_us"), ("k_dumps<", None), ("k_dump<", "k_dump_single_us"))
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            nm = row["Name"]
            for key, field in names:
                if key not in nm:
                    continue
                if field is None:  # k_dumps<HT, PAR>: the last template argument names the writer
                    field = "k_dumps_parallel_us" if nm.split(">(")[0].rstrip().endswith("true") else "k_dumps_serial_us"
                out[field] = round(float(row["AverageNs"]) / 1e3, 3)
                out[field.replace("_us", "_calls")] = int(row["Calls"])
                break
    return out


def step(cmd, limit):
    """one GPU step: a child of its own under `timeout -k 10`; its last output line, or None where it failed"""
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:] + f"\nstep failed with status {r.returncode}: {' '.join(cmd)}\n")
        return None
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    return lines[-1] if lines else ""


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
    return 0 if min(res["batched_parallel_ms"], res["batched_serial_ms"]) < res["loop_ms"] else 1


if __name__ == "__main__":
    sys.exit(main())
