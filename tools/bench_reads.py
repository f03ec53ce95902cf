#!/usr/bin/env python3
"""Reading a replayed batch back: the per-document loop against the batched reads.

Workload: config 3, 4,096 documents x 512 ops, replayed once. Timed, wall clock around the calls after a warm-up,
median of 5:
  (a) loop:    get_text(d) + get_length(d) for every document (one-workgroup launches, two or three stream waits each);
  (b) batched: one get_texts() + one get_lengths();
and the fill of (b) alone, with the packed copy and with the per-lane copy (MT_VAR_TEXTS_PACKED): the whole
mt_engine_get_texts call into a preallocated buffer, and that time less the size query's, which leaves the prefix sum,
k_texts and the copy back (the same bytes either way). Prints one JSON line; --out appends it to a file.

    timeout 600 python tools/bench_reads.py --out profiles/batched_reads.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fluidframework_amd import gen  # noqa: E402
from fluidframework_amd.engine import Engine, MT_VAR_TEXTS_PACKED, default_caps  # noqa: E402


def median_ms(f, reps):
    f()  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=4096)
    ap.add_argument("--ops", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()

    b = gen.generate(gen.config3(a.ops), a.docs)
    eng = Engine(b.ndocs, **default_caps(a.ops))
    eng.start_collab(b.local_long_id)
    eng.replay(b)
    assert (eng.errors()[0] == 0).all()
    n = b.ndocs

    loop = []
    batched = []

    def run_loop():
        loop[:] = [(eng.get_text(d), eng.get_length(d)) for d in range(n)]

    def run_batched():
        texts, _ = eng.get_texts()
        lens, _ = eng.get_lengths()
        batched[:] = list(zip(texts, lens.tolist()))

    t_loop = median_ms(run_loop, a.reps)
    t_batched = median_ms(run_batched, a.reps)
    assert loop == batched, "the batched reads differ from the loop"

    # the fill alone, both copies: the C call into a preallocated buffer (sizes, prefix sum, k_texts, copy back)
    off, st = np.zeros(n + 1, np.int64), np.zeros(n, np.int32)
    vp = ctypes.c_void_p
    total = eng.L.mt_engine_get_texts(eng.h, n, None, None, None, None, None, None, 0, off.ctypes.data_as(vp),
                                      st.ctypes.data_as(vp), None, 0)
    buf = np.zeros(total + 1, "<u2")

    def size_only():
        eng.L.mt_engine_get_texts(eng.h, n, None, None, None, None, None, None, 0, off.ctypes.data_as(vp),
                                  st.ctypes.data_as(vp), None, 0)

    def fill():
        eng.L.mt_engine_get_texts(eng.h, n, None, None, None, None, None, None, 0, off.ctypes.data_as(vp),
                                  st.ctypes.data_as(vp), buf.ctypes.data_as(vp), total)

    t_size = median_ms(size_only, a.reps)
    fills = {}
    units = {}
    for name, v in (("packed", 1), ("per_lane", 0)):
        eng.set_variant(MT_VAR_TEXTS_PACKED, v)
        buf[:] = 0
        fills[name] = median_ms(fill, a.reps)
        units[name] = buf[:total].tobytes()
    assert units["packed"] == units["per_lane"], "the two copies differ"
    res = {"bench": "batched_reads", "config": 3, "docs": n, "ops_per_doc": a.ops, "text_units": int(total),
           "loop_ms": round(t_loop, 3), "batched_ms": round(t_batched, 3), "speedup": round(t_loop / t_batched, 2),
           "texts_size_query_ms": round(t_size, 3), "texts_fill_packed_ms": round(fills["packed"], 3),
           "texts_fill_per_lane_ms": round(fills["per_lane"], 3),
           "fill_less_size_packed_ms": round(fills["packed"] - t_size, 3),
           "fill_less_size_per_lane_ms": round(fills["per_lane"] - t_size, 3), "reps": a.reps}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
    eng.close()
    return 0 if t_batched < t_loop else 1


if __name__ == "__main__":
    sys.exit(main())
