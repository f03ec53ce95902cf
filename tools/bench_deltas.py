#!/usr/bin/env python3
"""Batched delta-event reads (mt_engine_deltas_batch) on a replayed batch against the per-document read.

Workload: config 3, 4,096 documents x 512 ops, replayed once with a delta log (caps.dcap) that holds every word. Timed,
wall clock around the calls after a warm-up call, median of `reps`, all on one engine in one process:
  (0) the baseline: Engine.deltas(d) for every document, the only way to read the streams without the batched call
      (two mt_engine_deltas calls per document, each two copies and two stream waits);
  (1) verbatim: Engine.deltas_batch_raw() with both event kinds (a size call and a fill call);
  (2) one kind: the "sequenceDelta" events only and the "maintenance" events only, with the wave form and the serial
      one (MT_VAR_DELTAS_PARALLEL);
  (3) a cursor: every document read from its logged end (an empty window: what a host pays to learn that nothing
      happened), and from the middle boundary of its log, both forms.
The words of (1) must equal the loop's, and those of (2) oplog.filter_deltas of them on the first `--check-docs`
documents; both forms must agree everywhere. The bytes that cross to the host per mode (the words; the offsets, next
cursors, emitted counts and statuses are 28 bytes per query on top) join the JSON line.

    timeout 900 python tools/bench_deltas.py --out profiles/batched_deltas.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

from fluidframework_amd import gen  # noqa: E402
from fluidframework_amd import oplog as ol  # noqa: E402
from fluidframework_amd.engine import (DELTA_KINDS_MAINTENANCE, DELTA_KINDS_SEQUENCE, Engine,  # noqa: E402
                                       MT_VAR_DELTAS_PARALLEL, default_caps)
from bench_dumps import median_ms, step  # noqa: E402

BOTH = DELTA_KINDS_SEQUENCE | DELTA_KINDS_MAINTENANCE


def measure(a):
    b = gen.generate(gen.config3(a.ops), a.docs)
    eng = Engine(b.ndocs, dcap=a.dcap, **default_caps(a.ops))
    eng.start_collab(b.local_long_id)
    eng.replay(b)
    assert (eng.errors()[0] == 0).all()
    n = b.ndocs
    emitted = eng.delta_state()[0]
    res = {"bench": "batched_deltas", "config": 3, "docs": n, "ops_per_doc": a.ops, "dcap": a.dcap, "reps": a.reps,
           "words_emitted": int(emitted.sum()), "saturated_docs": int((emitted > a.dcap).sum())}

    loop = []
    res["deltas_loop_ms"] = round(median_ms(lambda: loop.__setitem__(slice(None), [eng.deltas(d) for d in range(n)]),
                                            a.reps), 3)
    got = {}

    def timed(name, par, **kw):
        eng.set_variant(MT_VAR_DELTAS_PARALLEL, par)
        res[f"{name}_ms"] = round(median_ms(lambda: got.__setitem__(name, eng.deltas_batch_raw(**kw)), a.reps), 3)
        res[f"{name}_bytes"] = 4 * int(len(got[name][1]))
        return got[name]

    off, words, end, em, st = timed("verbatim_wave", 1)
    assert not st.any() and np.array_equal(em, emitted) and np.array_equal(words, np.concatenate(loop))
    assert np.array_equal(timed("verbatim_serial", 0)[1], words)
    for kname, kinds in (("sequence", DELTA_KINDS_SEQUENCE), ("maintenance", DELTA_KINDS_MAINTENANCE)):
        w = timed(f"{kname}_wave", 1, kinds=kinds)
        s = timed(f"{kname}_serial", 0, kinds=kinds)
        assert all(np.array_equal(x, y) for x, y in zip(w, s)), kname
        for d in range(min(a.check_docs, n)):
            kept, e = ol.filter_deltas(loop[d], kinds)
            assert np.array_equal(w[1][w[0][d]: w[0][d + 1]], kept) and w[2][d] == e, (kname, d)
    # cursors: the logged end (nothing new), and the boundary nearest the middle of each log
    for fname, par in (("wave", 1), ("serial", 0)):
        e0 = timed(f"cursor_at_end_{fname}", par, from_words=end)
        assert not e0[4].any() and len(e0[1]) == 0
    mid = np.asarray([max((e for _, e, _ in ol._delta_event_spans(w.tolist())[0] if e <= len(w) // 2), default=0)
                      for w in loop], np.int64)
    for fname, par in (("wave", 1), ("serial", 0)):
        h = timed(f"cursor_mid_{fname}", par, from_words=mid)
        assert not h[4].any() and all(np.array_equal(h[1][h[0][d]: h[0][d + 1]], loop[d][mid[d]:]) for d in range(n))
    eng.set_variant(MT_VAR_DELTAS_PARALLEL, 1)
    res["loop_bytes"] = 4 * int(sum(len(x) for x in loop))
    res["speedup_verbatim_vs_loop"] = round(res["deltas_loop_ms"] / res["verbatim_wave_ms"], 1)
    print(json.dumps(res), flush=True)
    eng.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=4096)
    ap.add_argument("--ops", type=int, default=512)
    ap.add_argument("--dcap", type=int, default=1 << 15, help="delta log words per document")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--check-docs", type=int, default=32, help="documents checked against oplog.filter_deltas")
    ap.add_argument("--step", choices=["measure"])
    ap.add_argument("--limit", type=int, default=420, help="seconds allowed to the GPU step")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.step == "measure":
        return measure(a)
    line = step([sys.executable, os.path.abspath(__file__), "--step", "measure", "--docs", str(a.docs), "--ops",
                 str(a.ops), "--dcap", str(a.dcap), "--reps", str(a.reps), "--check-docs", str(a.check_docs)], a.limit)
    if not line:
        return 2
    print(line)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
