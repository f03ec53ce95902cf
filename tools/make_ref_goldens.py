"""Golden vectors from the REFERENCE merge-tree itself.

TEST INFRASTRUCTURE, dev container only. Steps:
  1. tools/ts_erase.py type-erases packages/dds/merge-tree/src/*.ts into /tmp/mt-oracle (outside the
     repo; the reference never travels, in any form);
  2. for every fixture set below, the in-repo generator (fluidframework_amd/gen.py, deterministic)
     makes the op logs; they are written as raw little-endian files to a scratch dir;
  3. node runs tools/ref_replay.mjs: each replica's log through the reference `Client`
     (applyMsg / insertSegmentLocal / removeRangeLocal / annotateRangeLocal) and its canonical
     segment dump (include/mt_oplog.h);
  4. the fixture `tests/golden/ref_<set>.npz` stores the workload recipe and document ids, a
     SHA-256 of the regenerated op-log bytes (so a generator change is detected, not silently
     re-pinned), the reference's per-document FNV-1a-64 digests, its dumps of the first docs, and
     the full op logs of those first docs (self-contained vectors).
The oracle (oracle/mt_oracle.c) is checked against the same digests here; tests/test_ref_goldens.py
checks the oracle and the host core on CPU and the HIP engine on the GPU.

usage: python tools/make_ref_goldens.py [--sets c2,c3,...] [--node node]
"""
from __future__ import annotations

import argparse
import dataclasses
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

from fluidframework_amd import gen  # noqa: E402
from fluidframework_amd import oplog as ol  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
ERASED = "/tmp/mt-oracle"
SCRATCH = "/tmp/mt-ref-batches"
KEEP_LOGS = 4  # documents whose full op logs + reference dumps are stored in the fixture

# fixture sets: (workload, document ids). Sizes keep each fixture well under a megabyte.
SETS = {
    "c1_farm": (gen.config1(2000), list(range(16))),                       # 2 farms x 8 replicas
    "c2_observer": (gen.config2(2000), list(range(96))),
    "c3_lagged": (gen.config3(1500), list(range(128))),
    "c3_lagged_long": (gen.config3(4096), list(range(1000, 1032))),         # the bench's doc length
    "c4_scaled": (gen.config4(20000), list(range(4))),                      # coalescing defeated, MSN advancing
    "c5_perm": (gen.config5(1500), list(range(64))),                        # PermutationSegment rows
    "c2_full": (gen.config2(10_000), list(range(16))),                      # config 2 at its full 10k msgs
    "c4_large": (gen.config4(300_000), [0, 1]),                             # >100k live rows: the tiled profile
}
KEEP = {"c4_large": 0, "c2_full": 1}  # stored full logs per set (default KEEP_LOGS): fixtures stay small


def write_batch(b: ol.Batch, interner: ol.Interner, d: str) -> None:
    os.makedirs(d, exist_ok=True)
    b.ops.tofile(os.path.join(d, "ops.bin"))
    b.op_off.astype("<i8").tofile(os.path.join(d, "op_off.bin"))
    b.text.astype("<u2").tofile(os.path.join(d, "text.bin"))
    b.text_off.astype("<i8").tofile(os.path.join(d, "text_off.bin"))
    b.props.tofile(os.path.join(d, "props.bin"))
    b.props_off.astype("<i8").tofile(os.path.join(d, "props_off.bin"))
    b.kv.tofile(os.path.join(d, "kv.bin"))
    b.kv_off.astype("<i8").tofile(os.path.join(d, "kv_off.bin"))
    b.local_long_id.astype("<i4").tofile(os.path.join(d, "local.bin"))
    meta = {"keys": interner.keys, "values": interner.values}
    if getattr(interner, "items", None):  # SubSequence items by id (ref_replay.mjs; none: an item is its id)
        meta["items"] = interner.items
    with open(os.path.join(d, "meta.json"), "w") as f:
        json.dump(meta, f)


def log_sha(b: ol.Batch) -> str:
    h = hashlib.sha256()
    for d in range(b.ndocs):
        ops, text, props, kv = b.doc(d)
        h.update(ops.tobytes())
        used = ops[(ops["kind"] & 7) == ol.OP_INSERT]
        for o in used:
            h.update(text[o["text_off"]: o["text_off"] + o["text_len"]].tobytes())
    return h.hexdigest()


def fnv1a64(bs: bytes) -> int:
    h = 0xcbf29ce484222325
    for x in bs:
        h = ((h ^ x) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def snapshot_cut(ops: np.ndarray, local: int, frac: float = 0.55) -> int:
    """A record index at which the replica has no pending local op and no group message is open, as
    close to `frac` of the log as possible: a snapshot drops unacked segments (snapshotV1.ts:187-192),
    so the rest of the log must not ack anything sent before the cut."""
    kind = ops["kind"]
    is_local = (kind & ol.OPF_LOCAL) != 0
    closes = (kind & ol.OPF_GROUPED) == 0
    sent = np.cumsum(is_local & closes)
    acked = np.cumsum(~is_local & closes & (ops["client"] == local) & ((kind & 7) != ol.OP_NOOP))
    ok = np.zeros(len(ops) + 1, bool)
    ok[0] = True
    ok[1:] = (sent == acked) & closes
    cand = np.nonzero(ok)[0]
    return int(cand[np.argmin(np.abs(cand - frac * len(ops)))])


def canonical_tree(tree: dict) -> str:
    """Order-insensitive form of a snapshot tree: each blob's JSON re-serialized with sorted keys
    (property-set key order is insertion order in the reference, key-id order here)."""
    from fluidframework_amd import snapshot as sn
    blobs = sn._blobs(tree)
    return json.dumps({k: json.loads(v) for k, v in blobs.items()}, sort_keys=True, separators=(",", ":"))


def run_reference(b: ol.Batch, d: str, node: str, cuts=None, interner=None, extra=()):
    write_batch(b, interner or gen.generator_interner(), d)
    if cuts is not None:
        with open(os.path.join(d, "snapshots.json"), "w") as f:
            json.dump([[i, int(c), int(b.local_long_id[i])] for i, c in enumerate(cuts)], f)
    t0 = time.time()
    r = subprocess.run([node, os.path.join(ROOT, "tools", "ref_replay.mjs"), ERASED, d, *extra], capture_output=True,
                       text=True)
    if r.returncode != 0:
        raise RuntimeError(f"reference replay failed: {r.stderr[-2000:]}")
    info = json.loads(r.stdout.strip().splitlines()[-1])
    errs = json.load(open(os.path.join(d, "ref_err.json")))["errors"]
    if errs:
        raise RuntimeError(f"reference threw on {len(errs)} docs: {list(errs.items())[:3]}")
    blob = np.fromfile(os.path.join(d, "ref_dumps.bin"), np.uint8)
    off = np.fromfile(os.path.join(d, "ref_dump_off.bin"), "<i8")
    dumps = [blob[off[i]: off[i + 1]].tobytes() for i in range(b.ndocs)]
    snaps = None
    if cuts is not None:
        sj = json.load(open(os.path.join(d, "ref_snapshots.json")))
        if sj["errors"]:
            raise RuntimeError(f"reference snapshot/load threw on {len(sj['errors'])} docs: {list(sj['errors'].items())[:2]}")
        lb = np.fromfile(os.path.join(d, "ref_loaded_dumps.bin"), np.uint8)
        lo = np.fromfile(os.path.join(d, "ref_loaded_off.bin"), "<i8")
        tail_err = np.full(b.ndocs, -1, np.int64)  # record (tail-relative) at which the loaded client threw
        for k, (at, _msg) in sj["tailErrors"].items():
            tail_err[int(k)] = at
        load_err = np.zeros(b.ndocs, bool)  # the reference could not load the snapshot it emitted
        for k in sj["loadErrors"]:
            load_err[int(k)] = True
        snaps = ([sj["trees"][str(i)] for i in range(b.ndocs)], [lb[lo[i]: lo[i + 1]].tobytes() for i in range(b.ndocs)],
                 tail_err, sj["tailErrors"], load_err, sj["loadErrors"])
    return dumps, info, time.time() - t0, snaps


def snap_body_logs(ndocs: int = 8, nmsg: int = 480, lag: int = 32):
    """Documents whose snapshot has a BODY holding collaboration-window segments (SURVEY.md §8(f)
    f1). Three 4,000-character inserts make a header chunk that stays below the MSN; every later edit
    (insert / remove / annotate, refSeq lagging up to `lag`) lands at or after position 12,000, so
    window segments only ever appear in body chunks. Even documents have one editing client that edits
    near the end (window segments trail the body, which the reference's loadBody can insert); odd
    documents have two editing anywhere after the header (its insertSegments under a
    (UniversalSequenceNumber, client) perspective then fails on the other client's window segments,
    snapshotLoader.ts:200-213). The replica is an observer (long id 0); positions come from an
    oracle replica's perspective lengths."""
    import oracle_client as oc
    it = gen.generator_interner()
    logs = []
    for d in range(ndocs):
        rng = np.random.default_rng(7100 + d)
        editors = [1] if d % 2 == 0 else [1, 2]
        log = ol.DocLog(it, local_long_id=0)
        obs = oc.OracleClient(it)
        obs.start_collab(0)
        st = {"seq": 0, "msn": 0}
        last_ref = {c: 0 for c in editors}
        seen = set()

        def send(kind, client, ref, **kw):
            st["seq"] += 1
            last_ref[client] = ref
            st["msn"] = min(last_ref.values())
            log.add(kind, client=client, seq=st["seq"], ref_seq=ref, min_seq=st["msn"], **kw)
            ops, text, props, kv = log.arrays()
            assert obs.replay_arrays(ops[-1:], text, props, kv) == 0
            seen.add(client)

        letters = np.array(list("abcdefghijklmnopqrstuvwxyz"))
        for k in range(3):
            send(ol.OP_INSERT, 1, st["seq"], pos1=4000 * k, text="".join(rng.choice(letters, 4000)))
        for _ in range(nmsg):
            c = int(rng.choice(editors))
            cur = st["seq"]
            ref = int(rng.integers(max(last_ref[c], st["msn"], cur - lag), cur + 1))
            if c not in seen:  # a client's first op sees the whole header text
                send(ol.OP_INSERT, c, cur, pos1=12000, text="first")
                continue
            L = obs.get_length_at(ref, c)
            lo = 12000 if len(editors) > 1 else max(12000, L - 40)  # one editor: edits near the end
            r = rng.random()
            if r < 0.6 or L <= 12001:
                t = "".join(rng.choice(letters, int(rng.integers(1, 20))))
                if rng.random() < 0.2:
                    t += "\n"
                send(ol.OP_INSERT, c, ref, pos1=L if len(editors) == 1 else int(rng.integers(lo, L + 1)), text=t)
            elif r < 0.9:
                a = int(rng.integers(lo, L))
                send(ol.OP_REMOVE, c, ref, pos1=a, pos2=min(L, a + int(rng.integers(1, 16))))
            else:
                a = int(rng.integers(lo, L))
                send(ol.OP_ANNOTATE, c, ref, pos1=a, pos2=min(L, a + int(rng.integers(1, 40))),
                     props={"bold": bool(rng.random() < 0.5), "size": int(rng.integers(8, 12))})
        logs.append(log)
    return ol.Batch.from_logs(logs), it


def make_snap_body(node: str) -> None:
    b, it = snap_body_logs()
    cuts = [snapshot_cut(b.doc(i)[0], 0, frac=0.85) for i in range(b.ndocs)]
    dumps, info, secs, (trees, loaded, tail_err, tail_msgs, load_err, load_msgs) = run_reference(
        b, os.path.join(SCRATCH, "snap_body"), node, cuts, interner=it)
    print(f"snap_body: {b.ndocs} docs; reference load failures on docs {np.nonzero(load_err)[0].tolist()}, "
          f"tail failures on {np.nonzero(tail_err >= 0)[0].tolist()}", flush=True)
    bodies = [len(sn_blobs(t)) - 1 for t in trees]
    print(f"  body chunks per doc: {bodies}")
    np.savez_compressed(
        os.path.join(GOLDEN, "refsnap_body.npz"),
        ops=b.ops, op_off=b.op_off, text=b.text, text_off=b.text_off, props=b.props, props_off=b.props_off,
        kv=b.kv, kv_off=b.kv_off, local=b.local_long_id, interner=json.dumps({"keys": it.keys, "values": it.values}),
        digests=np.asarray([fnv1a64(x) for x in dumps], np.uint64),
        snap_cut=np.asarray(cuts, np.int64),
        snap_sha256=np.asarray([hashlib.sha256(canonical_tree(t).encode()).hexdigest() for t in trees]),
        snap_loaded_digests=np.asarray([fnv1a64(x) for x in loaded], np.uint64),
        snap_tail_error=tail_err, snap_load_error=load_err, snap_trees=json.dumps(trees),
        source="tools/make_ref_goldens.py snap_body_logs + the reference's SnapshotV1 / SnapshotLoader under node",
    )


def sn_blobs(tree):
    from fluidframework_amd import snapshot as sn
    return sn._blobs(tree)


def words_fnv(w: np.ndarray) -> int:
    return fnv1a64(np.ascontiguousarray(w, "<i4").tobytes())


def make_deltas(names, node: str) -> None:
    """tests/golden/refdelta_<set>.npz: the reference's delta / maintenance callback stream
    (include/mt_oplog.h MT_DELTA_*, recorded by ref_replay.mjs --deltas) for every document of the set:
    per-document word counts and FNV-1a-64 of the words, and the full streams of the first documents."""
    for name in names:
        w, ids = SETS[name]
        b = gen.generate(w, ids=ids, threads=8)
        d = os.path.join(SCRATCH, name + "_deltas")
        write_batch(b, gen.generator_interner(), d)
        r = subprocess.run([node, os.path.join(ROOT, "tools", "ref_replay.mjs"), ERASED, d, "--deltas"],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"reference replay failed: {r.stderr[-2000:]}")
        errs = json.load(open(os.path.join(d, "ref_err.json")))["errors"]
        if errs:
            raise RuntimeError(f"reference threw on {len(errs)} docs: {list(errs.items())[:3]}")
        words = np.fromfile(os.path.join(d, "ref_deltas.bin"), "<i4")
        off = np.fromfile(os.path.join(d, "ref_delta_off.bin"), "<i8")
        per = [words[off[i]: off[i + 1]] for i in range(b.ndocs)]
        keep = min(2, b.ndocs)  # full streams of the first two documents
        np.savez_compressed(
            os.path.join(GOLDEN, f"refdelta_{name}.npz"),
            workload=json.dumps(dataclasses.asdict(w)), doc_ids=np.asarray(ids, np.int64), log_sha256=log_sha(b),
            nwords=np.diff(off).astype(np.int64), hashes=np.asarray([words_fnv(x) for x in per], np.uint64),
            keep_words=np.concatenate(per[:keep]).astype(np.int32), keep_off=off[: keep + 1].astype(np.int64),
            source=("packages/dds/merge-tree/src (reference, type-erased by tools/ts_erase.py) under node by "
                    "tools/ref_replay.mjs --deltas: mergeTreeDeltaCallback / mergeTreeMaintenanceCallback"),
        )
        print(f"refdelta_{name}: {b.ndocs} docs, {int(off[-1])} words", flush=True)


REF_SETS = ("c1_farm", "c2_observer", "c3_lagged", "c4_scaled", "c5_perm")


def run_refs(rb, d: str, node: str):
    write_batch(rb, gen.generator_interner(), d)
    r = subprocess.run([node, os.path.join(ROOT, "tools", "ref_replay.mjs"), ERASED, d], capture_output=True,
                       text=True)
    if r.returncode != 0:
        raise RuntimeError(f"reference replay failed: {r.stderr[-2000:]}")
    errs = json.load(open(os.path.join(d, "ref_err.json")))["errors"]
    if errs:
        raise RuntimeError(f"reference threw on {len(errs)} docs: {list(errs.items())[:3]}")
    rp = json.load(open(os.path.join(d, "ref_refpos.json")))
    nref = np.asarray([len(rp.get(str(i), [])) for i in range(rb.ndocs)], np.int32)
    pos = np.full((rb.ndocs, max(nref.max(), 1)), -1, np.int32)
    for i in range(rb.ndocs):
        pos[i, : nref[i]] = rp.get(str(i), [])
    blob = np.fromfile(os.path.join(d, "ref_dumps.bin"), np.uint8)
    off = np.fromfile(os.path.join(d, "ref_dump_off.bin"), "<i8")
    digests = np.asarray([fnv1a64(blob[off[i]: off[i + 1]].tobytes()) for i in range(rb.ndocs)], np.uint64)
    ins = json.load(open(os.path.join(d, "ref_refinside.json")))
    pe = json.load(open(os.path.join(d, "ref_refpastend.json")))
    inside = np.zeros(pos.shape, bool)
    past = np.zeros(pos.shape, bool)
    for i in range(rb.ndocs):
        inside[i, : nref[i]] = ins.get(str(i), [])
        past[i, : nref[i]] = pe.get(str(i), [])
    return nref, pos, digests, inside, past


def make_combine(node: str) -> None:
    """tests/golden/refcombine.npz: annotates with combining ops incr / consensus (tests/combine_inject.py) in
    config-3 and config-5 logs, replayed by the reference with tools/ref_replay.mjs --combine-watch: per document the
    first record after which a segment holds a value only Properties.combine makes (NaN, a {value, seq} object;
    -1: none) and, for the documents with none, the digest of the final replica; the replicas right before that record
    (prefix digests); and every document's final replica replayed past it, with the derived values dumped by content
    (final digests, two documents' dumps)."""
    import combine_inject
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    out = {}
    for name, w, n in (("c3", gen.config3(1500), 64), ("c5", gen.config5(1500), 32)):
        b = combine_inject.inject(gen.generate(w, ids=range(n), threads=8))
        d = os.path.join(SCRATCH, f"combine_{name}")
        write_batch(b, gen.generator_interner(), d)
        r = subprocess.run([node, os.path.join(ROOT, "tools", "ref_replay.mjs"), ERASED, d, "--combine-watch"],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"reference replay failed: {r.stderr[-2000:]}")
        errs = json.load(open(os.path.join(d, "ref_err.json")))["errors"]
        if errs:
            raise RuntimeError(f"reference threw on {len(errs)} docs: {list(errs.items())[:3]}")
        at = json.load(open(os.path.join(d, "ref_combine.json")))
        first = np.asarray([at.get(str(i), -1) for i in range(n)], np.int64)
        blob = np.fromfile(os.path.join(d, "ref_dumps.bin"), np.uint8)
        off = np.fromfile(os.path.join(d, "ref_dump_off.bin"), "<i8")
        dig = np.asarray([fnv1a64(blob[off[i]: off[i + 1]].tobytes()) if first[i] < 0 else 0 for i in range(n)],
                         np.uint64)
        # the whole logs, every replica dumped with its derived values by content (include/mt_oplog.h
        # MT_VALUE_DERIVED; tools/ref_replay.mjs derivedOf): the final replicas past the combined values
        df = os.path.join(SCRATCH, f"combine_{name}_full")
        write_batch(b, gen.generator_interner(), df)
        r = subprocess.run([node, os.path.join(ROOT, "tools", "ref_replay.mjs"), ERASED, df], capture_output=True,
                           text=True)
        if r.returncode != 0 or json.load(open(os.path.join(df, "ref_err.json")))["errors"]:
            raise RuntimeError(f"reference full replay failed: {r.stderr[-2000:]}")
        fb = np.fromfile(os.path.join(df, "ref_dumps.bin"), np.uint8)
        fo = np.fromfile(os.path.join(df, "ref_dump_off.bin"), "<i8")
        out[f"{name}_final_digests"] = np.asarray([fnv1a64(fb[fo[i]: fo[i + 1]].tobytes()) for i in range(n)],
                                                  np.uint64)
        keep = [i for i in range(n) if first[i] >= 0][:2]  # two documents' full dumps (self-contained vectors)
        out[f"{name}_keep_docs"] = np.asarray(keep, np.int64)
        out[f"{name}_keep_dumps"] = np.concatenate([fb[fo[i]: fo[i + 1]] for i in keep])
        out[f"{name}_keep_dump_off"] = np.cumsum([0] + [int(fo[i + 1] - fo[i]) for i in keep]).astype(np.int64)
        # the replicas right before that record (the prefix [0, first)): pins what the kept values did until then
        pre = ol.Batch.from_arrays([tuple(x if k else x[: (first[i] if first[i] >= 0 else len(x))]
                                          for k, x in enumerate(b.doc_arrays(i))) for i in range(n)], b.local_long_id)
        dp = os.path.join(SCRATCH, f"combine_{name}_pre")
        write_batch(pre, gen.generator_interner(), dp)
        r = subprocess.run([node, os.path.join(ROOT, "tools", "ref_replay.mjs"), ERASED, dp, "--combine-watch"],
                           capture_output=True, text=True)
        if r.returncode != 0 or json.load(open(os.path.join(dp, "ref_err.json")))["errors"]:
            raise RuntimeError(f"reference prefix replay failed: {r.stderr[-2000:]}")
        if json.load(open(os.path.join(dp, "ref_combine.json"))):
            raise RuntimeError("a prefix reaches a combined value")
        pb = np.fromfile(os.path.join(dp, "ref_dumps.bin"), np.uint8)
        po = np.fromfile(os.path.join(dp, "ref_dump_off.bin"), "<i8")
        out[f"{name}_prefix_digests"] = np.asarray([fnv1a64(pb[po[i]: po[i + 1]].tobytes()) for i in range(n)], np.uint64)
        out[f"{name}_workload"] = json.dumps(dataclasses.asdict(w))
        out[f"{name}_log_sha256"] = log_sha(b)
        out[f"{name}_first"] = first
        out[f"{name}_digests"] = dig
        ncomb = int(((b.props[b.ops["props"][b.ops["props"] > 0].astype(np.int64) - 1]["combining"]) >= 2).sum())
        print(f"refcombine {name}: {n} docs, {ncomb} combining annotates; {int((first >= 0).sum())} documents reach a "
              f"combined value", flush=True)
    np.savez_compressed(os.path.join(GOLDEN, "refcombine.npz"), **out,
                        source=("packages/dds/merge-tree/src (reference, type-erased by tools/ts_erase.py) under node "
                                "by tools/ref_replay.mjs (--combine-watch for first / prefix)"))


def make_zamboni(node: str) -> None:
    """tests/golden/refzamboni.npz: the hand-built zamboni edge logs (tests/zamboni_logs.py: append rules on long rows,
    newlines, markers, prevSegment resets, properties past 8 keys, leaf boundaries, pack) replayed by the reference:
    per document its digest, its whole canonical dump, the word count and FNV-1a-64 of its delta / maintenance stream
    (APPEND and UNLINK order) and the SHA-256 of its SnapshotV1 summary at the end of the log. Every case's witness
    must hold on the reference's dump."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_client as oc
    import zamboni_logs as zl
    cs = zl.cases()
    b = zl.batch(cs)
    it = cs[0].log.interner
    cuts = [int(n) for n in np.diff(b.op_off)]  # summarized at the end of the log
    d = os.path.join(SCRATCH, "zamboni")
    dumps, info, secs, (trees, loaded, tail_err, tail_msgs, load_err, load_msgs) = run_reference(
        b, d, node, cuts, interner=it, extra=("--deltas",))
    for c, x in zip(cs, dumps):
        if not c.witness(*ol.parse_dump(x)):
            raise RuntimeError(f"{c.name}: the witness does not hold on the reference's dump")
    words = np.fromfile(os.path.join(d, "ref_deltas.bin"), "<i4")
    woff = np.fromfile(os.path.join(d, "ref_delta_off.bin"), "<i8")
    per = [words[woff[i]: woff[i + 1]] for i in range(b.ndocs)]
    digests = np.asarray([fnv1a64(x) for x in dumps], np.uint64)
    _, odig, oerr = oc.replay_batch(b)
    np.savez_compressed(
        os.path.join(GOLDEN, "refzamboni.npz"), log_sha256=log_sha(b), names=np.asarray([c.name for c in cs]),
        digests=digests, dumps=np.frombuffer(b"".join(dumps), np.uint8),
        dump_off=np.concatenate([[0], np.cumsum([len(x) for x in dumps])]).astype(np.int64),
        delta_nwords=np.diff(woff).astype(np.int64), delta_hashes=np.asarray([words_fnv(x) for x in per], np.uint64),
        snap_sha256=np.asarray([hashlib.sha256(canonical_tree(t).encode()).hexdigest() for t in trees]),
        source=("packages/dds/merge-tree/src + sequence sharedSequence.ts SubSequence + matrix permutationvector.ts "
                "(reference, type-erased by tools/ts_erase.py) under node by tools/ref_replay.mjs --deltas with "
                "snapshots.json; logs: tests/zamboni_logs.py"))
    print(f"refzamboni: {b.ndocs} docs, {b.nops} records, every witness holds; oracle agrees on "
          f"{int((odig == digests).sum())}/{b.ndocs} digests; {len(load_msgs)} summaries do not load", flush=True)


RANGE_KEEP_ROWS = 100  # cases with fewer rows keep their whole dump in refranges.npz


def make_ranges(node: str) -> None:
    """tests/golden/refranges.npz: the hand-built wide range edits (tests/range_logs.py: removes and annotates over
    many leaves, perspective mixes, wide local groups and their acks, the drain afterwards, the cap cases) replayed by
    the reference: per document its digest, the word count and FNV-1a-64 of its delta stream, the SHA-256 of its
    SnapshotV1 summary at the end of the log, the whole dump of the documents that end with fewer than
    RANGE_KEEP_ROWS rows, and the positions of the reference cases' local references. Every case's witness must hold
    on the reference's dump."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_client as oc
    import range_logs as rl
    cs = rl.cases() + rl.caps()
    b = rl.batch(cs)
    it = cs[0].log.interner
    cuts = [int(n) for n in np.diff(b.op_off)]  # summarized at the end of the log
    d = os.path.join(SCRATCH, "ranges")
    dumps, info, secs, (trees, loaded, tail_err, tail_msgs, load_err, load_msgs) = run_reference(
        b, d, node, cuts, interner=it, extra=("--deltas",))
    parsed = [ol.parse_dump(x) for x in dumps]
    for c, p in zip(cs, parsed):
        if not c.witness(*p):
            raise RuntimeError(f"{c.name}: the witness does not hold on the reference's dump")
    words = np.fromfile(os.path.join(d, "ref_deltas.bin"), "<i4")
    woff = np.fromfile(os.path.join(d, "ref_delta_off.bin"), "<i8")
    per = [words[woff[i]: woff[i + 1]] for i in range(b.ndocs)]
    digests = np.asarray([fnv1a64(x) for x in dumps], np.uint64)
    _, odig, oerr = oc.replay_batch(b)
    if not ((odig == digests).all() and (oerr == 0).all()):
        raise RuntimeError(f"the oracle differs from the reference on {[c.name for c, a, r in zip(cs, odig, digests) if a != r]}")
    keep = [i for i, p in enumerate(parsed) if p[0]["nsegs"] < RANGE_KEEP_ROWS]
    # LocalReference.toPosition of every local reference of the reference cases (-1: detached), in creation order
    rp = json.load(open(os.path.join(d, "ref_refpos.json")))
    ref_docs = [i for i, c in enumerate(cs) if c.name in rl.REF_NAMES]
    if sorted(int(k) for k in rp) != ref_docs or any(len(rp[str(i)]) != len(rl.REF_ROWS) for i in ref_docs):
        raise RuntimeError(f"local references: expected {len(rl.REF_ROWS)} in documents {ref_docs}, got {rp}")
    np.savez_compressed(
        os.path.join(GOLDEN, "refranges.npz"), log_sha256=log_sha(b), names=np.asarray([c.name for c in cs]),
        digests=digests, nrows=np.asarray([p[0]["nsegs"] for p in parsed], np.int64),
        ref_docs=np.asarray(ref_docs, np.int64), ref_pos=np.asarray([rp[str(i)] for i in ref_docs], np.int32),
        keep=np.asarray(keep, np.int64), dumps=np.frombuffer(b"".join(dumps[i] for i in keep), np.uint8),
        dump_off=np.concatenate([[0], np.cumsum([len(dumps[i]) for i in keep])]).astype(np.int64),
        delta_nwords=np.diff(woff).astype(np.int64), delta_hashes=np.asarray([words_fnv(x) for x in per], np.uint64),
        snap_sha256=np.asarray([hashlib.sha256(canonical_tree(t).encode()).hexdigest() for t in trees]),
        source=("packages/dds/merge-tree/src + sequence sharedSequence.ts SubSequence + matrix permutationvector.ts "
                "(reference, type-erased by tools/ts_erase.py) under node by tools/ref_replay.mjs --deltas with "
                "snapshots.json; logs: tests/range_logs.py"))
    cen = rl.census(parsed, it.values)
    print(f"refranges: {b.ndocs} docs, {b.nops} records, every witness holds, the oracle agrees on every digest; "
          f"census {cen}; {len(keep)} whole dumps; {len(load_msgs)} summaries do not load", flush=True)


def make_reconnect(node: str) -> None:
    """tests/golden/refreconnect.npz: the hand-built reconnect cases (tests/reconnect_logs.py: what one pending group
    regenerates, findReconnectionPostition, reconnects before acks, the ring and the membership log at their limits, the
    cap cases) replayed by the reference with Client.regeneratePendingOp: per document its digest, row count and whole
    canonical dump (the oracle has no reconnect: nothing can stand in for a dump), the words of its delta stream with
    their count and FNV-1a-64 (the MT_DELTA_REGEN events: position, length and type of every regenerated op) and the
    SHA-256 of its SnapshotV1 summary at the end of the log. Every case's witness must hold on the reference's dump and
    its stated op counts must be the reference's."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import reconnect_logs as rc
    cs = rc.cases() + rc.caps()
    b = rc.batch(cs)
    it = cs[0].log.interner
    cuts = [int(n) for n in np.diff(b.op_off)]  # summarized at the end of the log
    d = os.path.join(SCRATCH, "reconnect")
    dumps, info, secs, (trees, loaded, tail_err, tail_msgs, load_err, load_msgs) = run_reference(
        b, d, node, cuts, interner=it, extra=("--deltas",))
    parsed = [ol.parse_dump(x) for x in dumps]
    words = np.fromfile(os.path.join(d, "ref_deltas.bin"), "<i4")
    woff = np.fromfile(os.path.join(d, "ref_delta_off.bin"), "<i8")
    per = [words[woff[i]: woff[i + 1]] for i in range(b.ndocs)]
    for c, p, w in zip(cs, parsed, per):
        if not c.witness(*p):
            raise RuntimeError(f"{c.name}: the witness does not hold on the reference's dump")
        got = tuple(len(e) for e in rc.regen_events(w))
        if got != c.nops:
            raise RuntimeError(f"{c.name}: the reference regenerates {got} ops, the case states {c.nops}")
    np.savez_compressed(
        os.path.join(GOLDEN, "refreconnect.npz"), log_sha256=log_sha(b), names=np.asarray([c.name for c in cs]),
        digests=np.asarray([fnv1a64(x) for x in dumps], np.uint64),
        nrows=np.asarray([p[0]["nsegs"] for p in parsed], np.int64), dumps=np.frombuffer(b"".join(dumps), np.uint8),
        dump_off=np.concatenate([[0], np.cumsum([len(x) for x in dumps])]).astype(np.int64),
        delta_nwords=np.diff(woff).astype(np.int64), delta_hashes=np.asarray([words_fnv(x) for x in per], np.uint64),
        delta_words=np.concatenate(per).astype(np.int32), delta_off=woff.astype(np.int64),
        snap_sha256=np.asarray([hashlib.sha256(canonical_tree(t).encode()).hexdigest() for t in trees]),
        source=("packages/dds/merge-tree/src + sequence sharedSequence.ts SubSequence + matrix permutationvector.ts "
                "(reference, type-erased by tools/ts_erase.py) under node by tools/ref_replay.mjs --deltas with "
                "snapshots.json: Client.regeneratePendingOp on reconnect; logs: tests/reconnect_logs.py"))
    print(f"refreconnect: {b.ndocs} docs, {b.nops} records, {sum(len(c.nops) for c in cs)} regenerated groups, "
          f"{sum(sum(c.nops) for c in cs)} regenerated ops, every witness and stated count holds; "
          f"{len(load_msgs)} summaries do not load", flush=True)


def make_inserts(node: str) -> None:
    """tests/golden/refinserts.npz: the hand-built insert cases (tests/insert_logs.py: tie walks over tombstones and
    pending rows, search alignment on 256-slot boundaries, row splits by offset, child index and child count, node
    splits, long texts, the cap cases) replayed by the reference: per document its digest, its row count, the word
    count and FNV-1a-64 of its delta / maintenance stream (INSERT positions, SPLIT events), the SHA-256 of its
    SnapshotV1 summary at the end of the log and the whole dump of the documents that end with fewer than
    RANGE_KEEP_ROWS rows. Every case's witness must hold on the reference's dump."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import insert_logs as il
    import oracle_client as oc
    cs = il.cases() + il.caps()
    b = il.batch(cs)
    it = cs[0].log.interner
    cuts = [int(n) for n in np.diff(b.op_off)]  # summarized at the end of the log
    d = os.path.join(SCRATCH, "inserts")
    dumps, info, secs, (trees, loaded, tail_err, tail_msgs, load_err, load_msgs) = run_reference(
        b, d, node, cuts, interner=it, extra=("--deltas",))
    parsed = [ol.parse_dump(x) for x in dumps]
    for c, p in zip(cs, parsed):
        if not c.witness(*p):
            raise RuntimeError(f"{c.name}: the witness does not hold on the reference's dump")
    words = np.fromfile(os.path.join(d, "ref_deltas.bin"), "<i4")
    woff = np.fromfile(os.path.join(d, "ref_delta_off.bin"), "<i8")
    per = [words[woff[i]: woff[i + 1]] for i in range(b.ndocs)]
    digests = np.asarray([fnv1a64(x) for x in dumps], np.uint64)
    _, odig, oerr = oc.replay_batch(b)
    if not ((odig == digests).all() and (oerr == 0).all()):
        raise RuntimeError(f"the oracle differs from the reference on {[c.name for c, a, r in zip(cs, odig, digests) if a != r]}")
    keep = [i for i, p in enumerate(parsed) if p[0]["nsegs"] < RANGE_KEEP_ROWS]
    np.savez_compressed(
        os.path.join(GOLDEN, "refinserts.npz"), log_sha256=log_sha(b), names=np.asarray([c.name for c in cs]),
        digests=digests, nrows=np.asarray([p[0]["nsegs"] for p in parsed], np.int64),
        keep=np.asarray(keep, np.int64), dumps=np.frombuffer(b"".join(dumps[i] for i in keep), np.uint8),
        dump_off=np.concatenate([[0], np.cumsum([len(dumps[i]) for i in keep])]).astype(np.int64),
        delta_nwords=np.diff(woff).astype(np.int64), delta_hashes=np.asarray([words_fnv(x) for x in per], np.uint64),
        snap_sha256=np.asarray([hashlib.sha256(canonical_tree(t).encode()).hexdigest() for t in trees]),
        source=("packages/dds/merge-tree/src + sequence sharedSequence.ts SubSequence + matrix permutationvector.ts "
                "(reference, type-erased by tools/ts_erase.py) under node by tools/ref_replay.mjs --deltas with "
                "snapshots.json; logs: tests/insert_logs.py"))
    cen = il.census(parsed, [b.doc(i)[0] for i in range(b.ndocs)])
    print(f"refinserts: {b.ndocs} docs, {b.nops} records, every witness holds, the oracle agrees on every digest; "
          f"census {cen}; {len(keep)} whole dumps; {len(load_msgs)} summaries do not load", flush=True)


def make_tiles(node: str) -> None:
    """tests/golden/reftiles.npz: the hand-built marker-query cases (tests/tile_logs.py) replayed by the reference, and
    the reference Client's own answers to each case's queries: Client.findTile as (found, pos, the tile's index in
    walkAllSegments order) and Client.getStackContext per label as the stack's (index, refType) pairs, bottom first.
    Every case's witness must hold on the reference's dump, which the fixture keeps whole."""
    import tile_logs as tl
    import oracle_client as oc
    cs = tl.cases()
    b = tl.batch(cs)
    it = tl.interner()
    tq, sq = tl.queries(cs)
    d = os.path.join(SCRATCH, "tiles")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "tilequeries.json"), "w") as f:
        json.dump({"tiles": [list(q) for q in tq], "stacks": [list(q) for q in sq]}, f)
    dumps, info, secs, _ = run_reference(b, d, node, interner=it)
    parsed = [ol.parse_dump(x) for x in dumps]
    for c, p in zip(cs, parsed):
        if not c.witness(*p):
            raise RuntimeError(f"{c.name}: the witness does not hold on the reference's dump")
    digests = np.asarray([fnv1a64(x) for x in dumps], np.uint64)
    _, odig, oerr = oc.replay_batch(b)
    if not ((odig == digests).all() and (oerr == 0).all()):
        raise RuntimeError(f"the oracle differs from the reference on {[c.name for c, a, r in zip(cs, odig, digests) if a != r]}")
    ans = json.load(open(os.path.join(d, "ref_tiles.json")))
    assert len(ans["tiles"]) == len(tq) and len(ans["stacks"]) == len(sq)
    flat = [x for st in ans["stacks"] for x in st]
    keep = [i for i, p in enumerate(parsed) if p[0]["nsegs"] < 400]
    np.savez_compressed(
        os.path.join(GOLDEN, "reftiles.npz"), log_sha256=log_sha(b), names=np.asarray([c.name for c in cs]),
        digests=digests, nrows=np.asarray([p[0]["nsegs"] for p in parsed], np.int64),
        keep=np.asarray(keep, np.int64), dumps=np.frombuffer(b"".join(dumps[i] for i in keep), np.uint8),
        dump_off=np.concatenate([[0], np.cumsum([len(dumps[i]) for i in keep])]).astype(np.int64),
        tile_doc=np.asarray([q[0] for q in tq], np.int32), tile_label=np.asarray([q[1] for q in tq]),
        tile_pos=np.asarray([-1 if q[2] is None else q[2] for q in tq], np.int32),
        tile_preceding=np.asarray([q[3] for q in tq], bool),
        tile_answers=np.asarray(ans["tiles"], np.int32).reshape(-1, 3),
        stack_doc=np.asarray([q[0] for q in sq], np.int32), stack_label=np.asarray([q[1] for q in sq]),
        stack_pos=np.asarray([-1 if q[2] is None else q[2] for q in sq], np.int32),
        stack_off=np.concatenate([[0], np.cumsum([len(st) for st in ans["stacks"]])]).astype(np.int64),
        stack_entries=np.asarray(flat, np.int32).reshape(-1, 2),
        source=("packages/dds/merge-tree/src (reference, type-erased by tools/ts_erase.py) under node by "
                "tools/ref_replay.mjs with tilequeries.json: Client.findTile / Client.getStackContext after each "
                "document's replay; logs: tests/tile_logs.py"))
    nf = int(sum(a[0] for a in ans["tiles"]))
    print(f"reftiles: {b.ndocs} docs, {b.nops} records, every witness holds, the oracle agrees on every digest; "
          f"{len(tq)} findTile queries ({nf} found), {len(sq)} getStackContext queries (deepest "
          f"{max((len(st) for st in ans['stacks']), default=0)}); {len(keep)} whole dumps", flush=True)


def make_hvec(node: str) -> None:
    """tests/golden/refhvec.npz: the hand-built PermutationVector read cases (tests/hvec_logs.py) replayed by the
    reference Client with PermutationVector's handle bookkeeping (tools/ref_replay.mjs --handles), and its answers to
    each case's queries (handlequeries.json): per handle range the raw segment.start + offset of every position or
    "throws", per (handle, localSeq) handleToPosition's result or "throws"; every document's HandleTable.snapshot().
    Every case's witness must hold on the reference's dump, which the fixture keeps whole. Every query has an answer or
    a recorded throw."""
    import hvec_logs as hl
    cs = hl.cases()
    b = hl.batch(cs)
    rq, hq = hl.queries(cs)
    d = os.path.join(SCRATCH, "hvec")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "handlequeries.json"), "w") as f:
        json.dump({"ranges": [list(q) for q in rq], "positions": [list(q) for q in hq]}, f)
    dumps, info, secs, _ = run_reference(b, d, node, interner=hl.interner(), extra=("--handles",))
    parsed = [ol.parse_dump(x) for x in dumps]
    for c, p in zip(cs, parsed):
        if not c.witness(*p):
            raise RuntimeError(f"{c.name}: the witness does not hold on the reference's dump: "
                               f"{p[0]} {[(x['len'], x['start']) for x in p[1]][:24]}")
    ans = json.load(open(os.path.join(d, "ref_hvec.json")))
    assert len(ans["ranges"]) == len(rq) and len(ans["positions"]) == len(hq), "a query has no answer"
    for q, a in zip(rq, ans["ranges"]):
        assert ("throws" in a) != ("handles" in a) and ("throws" in a or len(a["handles"]) == q[2] - q[1]), (q, a)
    for q, a in zip(hq, ans["positions"]):
        assert ("throws" in a) != ("pos" in a), (q, a)
    ht = json.load(open(os.path.join(d, "ref_handles.json")))
    tables = [np.asarray(ht[str(i)], np.int32) for i in range(b.ndocs)]
    flat = [x for a in ans["ranges"] for x in a.get("handles", [])]
    np.savez_compressed(
        os.path.join(GOLDEN, "refhvec.npz"), log_sha256=log_sha(b), names=np.asarray([c.name for c in cs]),
        digests=np.asarray([fnv1a64(x) for x in dumps], np.uint64),
        dumps=np.frombuffer(b"".join(dumps), np.uint8),
        dump_off=np.concatenate([[0], np.cumsum([len(x) for x in dumps])]).astype(np.int64),
        range_doc=np.asarray([q[0] for q in rq], np.int32), range_start=np.asarray([q[1] for q in rq], np.int32),
        range_end=np.asarray([q[2] for q in rq], np.int32),
        range_throws=np.asarray(["throws" in a for a in ans["ranges"]], bool),
        # throws that are the batched call's validity rule, not reference behaviour (a reversed range, an empty range
        # outside [0, length]: the reference's getHandles would return [] for them)
        range_rule_throws=np.asarray([bool(a.get("rule")) for a in ans["ranges"]], bool),
        range_off=np.concatenate([[0], np.cumsum([len(a.get("handles", [])) for a in ans["ranges"]])]).astype(np.int64),
        range_handles=np.asarray(flat, np.int64),  # raw: Handle.unallocated + offset where the segment has no handles
        pos_doc=np.asarray([q[0] for q in hq], np.int32), pos_handle=np.asarray([q[1] for q in hq], np.int32),
        pos_local_seq=np.asarray([-1 if q[2] is None else q[2] for q in hq], np.int32),  # -1: the default argument
        pos_throws=np.asarray(["throws" in a for a in ans["positions"]], bool),
        pos_answers=np.asarray([a.get("pos", -1) for a in ans["positions"]], np.int32),
        tables=np.concatenate(tables), table_off=np.cumsum([0] + [len(t) for t in tables]).astype(np.int64),
        source=("packages/dds/merge-tree/src + matrix handletable.ts (reference, type-erased by tools/ts_erase.py) under "
                "node by tools/ref_replay.mjs --handles with handlequeries.json: HandleCache.getHandles and "
                "PermutationVector.handleToPosition restated over the reference Client after each document's replay; "
                "a range throw marked in range_rule_throws (reversed, or empty outside [0, length]) is the batched call's "
                "validity rule, decided here and not observed: the reference's getHandles returns [] for such a range; "
                "logs: tests/hvec_logs.py"))
    nt, pt = int(sum("throws" in a for a in ans["ranges"])), int(sum("throws" in a for a in ans["positions"]))
    print(f"refhvec: {b.ndocs} docs, {b.nops} records, every witness holds; {len(rq)} handle ranges ({nt} throw, "
          f"{len(flat)} handles), {len(hq)} handleToPosition queries ({pt} throw); tables "
          f"{min(len(t) for t in tables)}..{max(len(t) for t in tables)} entries", flush=True)


def make_props(node: str) -> None:
    """tests/golden/refprops.npz: the hand-built property-manager cases (tests/prop_logs.py: key slots and op widths,
    pending-key counts, rewrites, combining ops, zamboni over 24 keys, the cap cases) replayed by the reference: per
    document its digest and whole canonical dump, the SHA-256 of its SnapshotV1 summary at the end of the log and, for
    every case without combining ops, the words of its delta stream, their count and FNV-1a-64 (the combining cases run
    without --deltas: the replayer cannot word a derived previous value; their count is -1). Every witness must hold
    on the reference's dump and stream."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_client as oc
    import prop_logs as pl
    cs = pl.cases() + pl.caps()
    it = cs[0].log.interner
    parts = {False: [i for i, c in enumerate(cs) if not c.combining], True: [i for i, c in enumerate(cs) if c.combining]}
    dumps, trees, per = [None] * len(cs), [None] * len(cs), [np.zeros(0, "<i4")] * len(cs)
    for comb, idx in parts.items():
        b = pl.batch([cs[i] for i in idx])
        cuts = [int(n) for n in np.diff(b.op_off)]  # summarized at the end of the log
        d = os.path.join(SCRATCH, "props_combine" if comb else "props")
        dd, info, secs, (tt, loaded, tail_err, tail_msgs, load_err, load_msgs) = run_reference(
            b, d, node, cuts, interner=it, extra=() if comb else ("--deltas",))
        if not comb:
            words = np.fromfile(os.path.join(d, "ref_deltas.bin"), "<i4")
            woff = np.fromfile(os.path.join(d, "ref_delta_off.bin"), "<i8")
        for k, i in enumerate(idx):
            dumps[i], trees[i] = dd[k], tt[k]
            if not comb:
                per[i] = words[woff[k]: woff[k + 1]]
    for c, x, w in zip(cs, dumps, per):
        if not c.witness(*ol.parse_dump(x)):
            raise RuntimeError(f"{c.name}: the witness does not hold on the reference's dump")
        if c.dwitness is not None and not c.dwitness(ol.decode_deltas(w)):
            raise RuntimeError(f"{c.name}: the witness does not hold on the reference's delta stream")
    digests = np.asarray([fnv1a64(x) for x in dumps], np.uint64)
    plain = [i for i in parts[False] if cs[i].name not in pl.CAP_NAMES]
    _, odig, oerr = oc.replay_batch(pl.batch([cs[i] for i in plain]))
    agree = int((odig == digests[plain]).sum())
    b = pl.batch(cs)
    np.savez_compressed(
        os.path.join(GOLDEN, "refprops.npz"), log_sha256=log_sha(b), names=np.asarray([c.name for c in cs]),
        digests=digests, dumps=np.frombuffer(b"".join(dumps), np.uint8),
        dump_off=np.concatenate([[0], np.cumsum([len(x) for x in dumps])]).astype(np.int64),
        delta_nwords=np.asarray([-1 if c.combining else len(w) for c, w in zip(cs, per)], np.int64),
        delta_hashes=np.asarray([words_fnv(x) for x in per], np.uint64),
        delta_words=np.concatenate(per).astype(np.int32),
        delta_off=np.concatenate([[0], np.cumsum([len(w) for w in per])]).astype(np.int64),
        snap_sha256=np.asarray([hashlib.sha256(canonical_tree(t).encode()).hexdigest() for t in trees]),
        source=("packages/dds/merge-tree/src + sequence sharedSequence.ts SubSequence + matrix permutationvector.ts "
                "(reference, type-erased by tools/ts_erase.py) under node by tools/ref_replay.mjs --deltas with "
                "snapshots.json; logs: tests/prop_logs.py"))
    print(f"refprops: {b.ndocs} docs, {b.nops} records, every witness holds; the oracle agrees on {agree}/{len(plain)} "
          f"digests of the cases without combining ops; census {pl.census(b)}", flush=True)


def make_refentry(node: str) -> None:
    """tests/golden/refentry_kat.npz: the refsByOffset-entry KATs (tests/refs_entry_logs.py) replayed by the
    reference: LocalReference.toPosition() of every reference (-2: addLocalReference threw) and the digests."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import refs_entry_logs as rel
    rb = rel.batch()
    nref, pos, digests, _, _ = run_refs(rb, os.path.join(SCRATCH, "refentry"), node)
    np.savez_compressed(
        os.path.join(GOLDEN, "refentry_kat.npz"), log_sha256=log_sha(rb), nref=nref, positions=pos, digests=digests,
        source=("packages/dds/merge-tree/src (reference, type-erased by tools/ts_erase.py) under node by "
                "tools/ref_replay.mjs: LocalReference + Client.addLocalReference / removeLocalReference, "
                "toPosition() at the end"))
    print(f"refentry_kat: {rb.ndocs} docs, {int(nref.sum())} references, {int((pos == -2).sum())} the reference "
          f"could not add, {int((pos == -1).sum())} detached", flush=True)


def make_refs(names, node: str, removals: bool = False) -> None:
    """tests/golden/refrefs_<set>.npz: local references (MT_OP_REF records injected by tests/refs_inject.py)
    replayed by the reference, then up to 4 insertAtReferencePositionLocal records per document appended
    at the end of its stream on references the first pass left attached. Stored: the targets, and after
    the whole stream LocalReference.toPosition() of every reference (-2: Client.addLocalReference threw, a
    reference defect: localReference.ts:195-201 pushes onto the missing `at` list of an offset that holds
    only slid references) and the reference's digests of the replicas."""
    import refs_inject
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_ref_goldens import caps_for
    for name in names:
        w, ids = SETS[name]
        b = gen.generate(w, ids=ids, threads=8)
        c = caps_for(w)
        rb = refs_inject.inject(b, (c["ncap"], c["hcap"], c["acap"], c["mcap"], c["gcap"], c["ccap"]))
        if removals:  # Client.removeLocalReference records (MT_REF_REMOVE) after the references' creation
            rb = refs_inject.add_removals(rb)
        _, pos1, _, inside, past = run_refs(rb, os.path.join(SCRATCH, name + "_refs"), node)
        targets = np.full((rb.ndocs, 4), -1, np.int32)
        for i in range(rb.ndocs):
            # attached references an insert can target: inside their segment, or past the end of a text
            # segment (the reference's splitAt makes an empty segment there, which the engine models); past
            # the end of a PermutationSegment or a Marker the reference corrupts or throws
            att = np.nonzero((pos1[i] >= 0) & inside[i])[0]
            if len(att):
                pick = np.random.default_rng(777 + i).choice(att, size=min(4, len(att)), replace=False)
                targets[i, : len(pick)] = pick
        rb2 = refs_inject.add_atref_inserts(rb, [t[t >= 0] for t in targets])
        nref, pos, digests, _, _ = run_refs(rb2, os.path.join(SCRATCH, name + "_refs2"), node)
        npast = int(sum(past[i, t[t >= 0]].sum() for i, t in enumerate(targets)))
        np.savez_compressed(
            os.path.join(GOLDEN, f"{'refunref' if removals else 'refrefs'}_{name}.npz"),
            nremove=int((((rb2.ops["kind"] & 7) == ol.OP_REF) & (rb2.ops["seg_kind"] == refs_inject.REF_REMOVE)).sum()),
            workload=json.dumps(dataclasses.asdict(w)), doc_ids=np.asarray(ids, np.int64), log_sha256=log_sha(rb2),
            nref=nref, positions=pos, digests=digests, atref_targets=targets, atref_past_end=npast,
            source=("packages/dds/merge-tree/src (reference, type-erased by tools/ts_erase.py) under node by "
                    "tools/ref_replay.mjs: LocalReference + Client.addLocalReference, "
                    "insertAtReferencePositionLocal, toPosition() at the end"),
        )
        print(f"{'refunref' if removals else 'refrefs'}_{name}: {rb2.ndocs} docs, {int(nref.sum())} references: {int((pos >= 0).sum())} attached, "
              f"{int((pos == -2).sum())} the reference could not add; {int((targets >= 0).sum())} inserts at "
              f"references, {npast} of them past their segment's end", flush=True)


TEXT_SETS = {"c3_markers": (gen.config3(1500), list(range(24))), "c5_perm": (gen.config5(1500), list(range(16)))}


def text_queries(b, seed: int):
    """getText queries per document: the local view under every placeholder ("", "#", "<>") with the default
    range, inside ranges, an empty range, a range whose end precedes its start (JavaScript substring swaps
    the ends), a negative start and an end past the text; plus the current-seq views of two remote clients.
    Lengths are not known here, so ranges are drawn up to 4,000 and the reference clips them."""
    q = []
    rng = np.random.default_rng(seed)
    for d in range(b.ndocs):
        ops = b.doc(d)[0]
        seq = int(ops["seq"][(ops["kind"] & 0x80) == 0].max())
        for ph in ("", "#", "<>"):
            q.append([d, 0, -1, ph, None, None])
            for _ in range(2):
                a, e = sorted(int(x) for x in rng.integers(0, 1500, 2))
                q.append([d, 0, -1, ph, a, e])
            a = int(rng.integers(0, 1500))
            q.append([d, 0, -1, ph, a, a])
            q.append([d, 0, -1, ph, a + 40, a])
            q.append([d, 0, -1, ph, -5, int(rng.integers(0, 1500))])
            q.append([d, 0, -1, ph, int(rng.integers(0, 1500)), 4000])
        clients = sorted({int(c) for c in ops["client"][(ops["kind"] & 0x80) == 0]} - {int(b.local_long_id[d])})
        for c in clients[:2]:
            q.append([d, seq, c, "#", None, None])
            a, e = sorted(int(x) for x in rng.integers(0, 1500, 2))
            q.append([d, seq, c, "", a, e])
    return q


def make_texts(node: str) -> None:
    """tests/golden/reftext_<set>.npz: MergeTreeTextHelper.getText(refSeq, clientId, placeholder, start, end)
    of the reference after each document's replay (tools/ref_replay.mjs textqueries.json), for logs with
    markers (tests/text_markers.py: remote length-1 text inserts made Marker inserts) and PermutationSegment
    logs. Stored: the queries, each answer's length and FNV-1a-64 over its UTF-16LE units, and the answers
    of document 0 in full."""
    import text_markers
    for name, (w, ids) in TEXT_SETS.items():
        b = gen.generate(w, ids=ids, threads=8)
        if name == "c3_markers":
            b = text_markers.with_markers(b)
        q = text_queries(b, 4242)
        d = os.path.join(SCRATCH, name + "_text")
        write_batch(b, gen.generator_interner(), d)
        with open(os.path.join(d, "textqueries.json"), "w") as f:
            json.dump(q, f)
        r = subprocess.run([node, os.path.join(ROOT, "tools", "ref_replay.mjs"), ERASED, d], capture_output=True,
                           text=True)
        if r.returncode != 0:
            raise RuntimeError(f"reference replay failed: {r.stderr[-2000:]}")
        errs = json.load(open(os.path.join(d, "ref_err.json")))["errors"]
        if errs:
            raise RuntimeError(f"reference threw on {len(errs)} docs: {list(errs.items())[:3]}")
        texts = json.load(open(os.path.join(d, "ref_texts.json")))
        assert len(texts) == len(q)
        units = [t.encode("utf-16-le") for t in texts]
        qa = np.asarray([[x[0], x[1], x[2], -(1 << 31) if x[4] is None else x[4], -(1 << 31) if x[5] is None else x[5]]
                         for x in q], np.int32)
        blob = np.frombuffer(b"".join(u for (x, u) in zip(q, units) if x[0] == 0), np.uint8)
        np.savez_compressed(
            os.path.join(GOLDEN, f"reftext_{name}.npz"),
            workload=json.dumps(dataclasses.asdict(w)), doc_ids=np.asarray(ids, np.int64), log_sha256=log_sha(b),
            markers=name == "c3_markers", queries=qa, placeholders=np.asarray([x[3] for x in q]),
            lengths=np.asarray([len(t) for t in texts], np.int64),
            fnv=np.asarray([fnv1a64(u) for u in units], np.uint64), doc0_units=blob,
            source=("packages/dds/merge-tree/src (reference, type-erased by tools/ts_erase.py) under node by "
                    "tools/ref_replay.mjs: MergeTreeTextHelper.getText after each document's replay"),
        )
        print(f"reftext_{name}: {b.ndocs} docs, {len(q)} queries, {sum(len(t) for t in texts)} units", flush=True)


TREE_SETS = ("c3_lagged", "c5_perm")


def make_tree(node: str) -> None:
    """tests/golden/reftree_<set>.npz: logs with MergeTree-level records (tests/tree_ops.py, mt_oplog.h
    MT_OPF_TREE: MergeTree.insertSegments / markRangeRemoved / annotateRange with explicit refSeq, clientId,
    seq) replayed by the reference; its digests, which must also equal the reference's digests of the
    unconverted logs (the conversion calls what the Client itself calls)."""
    import tree_ops
    for name in TREE_SETS:
        w, ids = SETS[name]
        b = tree_ops.to_tree_ops(gen.generate(w, ids=ids, threads=8))
        dumps, info, secs, _ = run_reference(b, os.path.join(SCRATCH, name + "_tree"), node)
        digests = np.asarray([fnv1a64(x) for x in dumps], np.uint64)
        orig = np.load(os.path.join(GOLDEN, f"ref_{name}.npz"))["digests"]
        if not np.array_equal(digests, orig):
            raise RuntimeError(f"{name}: the reference's digests of the MergeTree-level logs differ from its own "
                               f"digests of the Client-level logs on {int((digests != orig).sum())} docs")
        ntree = int(((b.ops["kind"] & tree_ops.OPF_TREE) != 0).sum())
        np.savez_compressed(
            os.path.join(GOLDEN, f"reftree_{name}.npz"),
            workload=json.dumps(dataclasses.asdict(w)), doc_ids=np.asarray(ids, np.int64), log_sha256=log_sha(b),
            digests=digests, ntree=ntree,
            source=("packages/dds/merge-tree/src (reference, type-erased by tools/ts_erase.py) under node by "
                    "tools/ref_replay.mjs: MergeTree.insertSegments / markRangeRemoved / annotateRange records"),
        )
        print(f"reftree_{name}: {b.ndocs} docs, {ntree} MergeTree-level records, digests equal the Client-level "
              f"logs' on every document", flush=True)


def make_handle_snaps(node: str) -> None:
    """tests/golden/refhsnap_c5_perm.npz: SharedMatrix vectors summarized with allocated handles and loaded again
    (VERDICT r4 #5). The refhandles logs (config 5 + getAllocatedHandle records) run under the reference with
    PermutationVector's bookkeeping (tools/ref_replay.mjs --handles); at a cut with nothing pending the replica is
    summarized as PermutationVector.snapshot does (SnapshotV1 segments, PermutationSegment specs [length, start],
    plus the HandleTable blob, permutationvector.ts:256-268), a fresh replica loads both as PermutationVector.load
    does (HandleTable.load, then Client.load under its delta hooks: loadBody's inserts reset their starts) and
    applies the rest of the log. Stored: the summaries (trees, blobs), the loaded replicas' final digests (dumps
    with allocated starts) and HandleTable.snapshot()s, and where the reference could not load or continue."""
    import handles_inject
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_ref_goldens import caps_for
    w, ids = SETS["c5_perm"]
    b = gen.generate(w, ids=ids, threads=8)
    c = caps_for(w)
    hb = handles_inject.inject(b, (c["ncap"], c["hcap"], c["acap"], c["mcap"], c["gcap"], c["ccap"]))
    cuts = []
    for i in range(hb.ndocs):  # getAllocatedHandle records are local but never sent: not pending ops
        ops = hb.doc(i)[0]
        keep = ~(((ops["kind"] & 7) == ol.OP_NOOP) & ((ops["kind"] & ol.OPF_LOCAL) != 0))
        idx = np.nonzero(keep)[0]
        c0 = snapshot_cut(ops[keep], int(hb.local_long_id[i]))
        cuts.append(int(idx[c0]) if c0 < len(idx) else len(ops))
    d = os.path.join(SCRATCH, "hsnap")
    # default chunk size: every summary is one header chunk (with 200-row chunks the reference's own loadBody
    # throws on all 64 documents: their body chunks hold window segments, snapshotLoader.ts:200-213)
    dumps, info, secs, snaps = run_reference(hb, d, node, cuts, extra=("--handles",))
    trees, loaded, tail_err, tail_msgs, load_err, load_msgs = snaps
    sh = json.load(open(os.path.join(d, "ref_snap_handles.json")))
    blobs = [np.asarray(sh[str(i)]["blob"], np.int32) for i in range(hb.ndocs)]
    finals = [np.asarray(sh[str(i)].get("final", []), np.int32) for i in range(hb.ndocs)]
    nstart = sum(1 for t in trees for v in json.loads(canonical_tree(t)).values() if isinstance(v, dict)
                 for seg in v.get("segments", v.get("segmentTexts", [])) if isinstance(seg, list) and len(seg) > 1
                 and seg[1] is not None and seg[1] >= 1)
    boff = np.cumsum([0] + [len(x) for x in blobs]).astype(np.int64)
    foff = np.cumsum([0] + [len(x) for x in finals]).astype(np.int64)
    np.savez_compressed(
        os.path.join(GOLDEN, "refhsnap_c5_perm.npz"), workload=json.dumps(dataclasses.asdict(w)),
        doc_ids=np.asarray(ids, np.int64), log_sha256=log_sha(hb), cuts=np.asarray(cuts, np.int64),
        trees=json.dumps(trees), blobs=np.concatenate(blobs), blob_off=boff, finals=np.concatenate(finals), final_off=foff,
        loaded_digests=np.asarray([fnv1a64(x) for x in loaded], np.uint64), tail_error=tail_err, load_error=load_err,
        source=("packages/dds/merge-tree/src + matrix handletable.ts (reference, type-erased by tools/ts_erase.py) "
                "under node by tools/ref_replay.mjs --handles with snapshots.json"),
    )
    print(f"refhsnap_c5_perm: {hb.ndocs} docs, {nstart} summarized segments with allocated starts, blobs "
          f"{min(len(x) for x in blobs)}..{max(len(x) for x in blobs)} entries; {int(load_err.sum())} do not load, "
          f"{int((tail_err >= 0).sum())} cannot apply their tail: {sorted(set(m for _, m in tail_msgs.values()))[:3]}",
          flush=True)


def make_handles(node: str) -> None:
    """tests/golden/refhandles_c5_perm.npz: config-5 logs (PermutationSegment rows) with injected
    PermutationVector.getAllocatedHandle records (tests/handles_inject.py) replayed by the reference Client with
    PermutationVector's handle bookkeeping (tools/ref_replay.mjs --handles: the reference's HandleTable,
    getAllocatedHandle / onDelta / onMaintenance restated). Stored: the digests of dumps that carry allocated
    starts (MT_DF_HANDLE) and every document's HandleTable.snapshot()."""
    import handles_inject
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_ref_goldens import caps_for
    w, ids = SETS["c5_perm"]
    b = gen.generate(w, ids=ids, threads=8)
    c = caps_for(w)
    hb = handles_inject.inject(b, (c["ncap"], c["hcap"], c["acap"], c["mcap"], c["gcap"], c["ccap"]))
    d = os.path.join(SCRATCH, "handles")
    write_batch(hb, gen.generator_interner(), d)
    r = subprocess.run([node, os.path.join(ROOT, "tools", "ref_replay.mjs"), ERASED, d, "--handles"],
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"reference replay failed: {r.stderr[-2000:]}")
    errs = json.load(open(os.path.join(d, "ref_err.json")))["errors"]
    if errs:
        raise RuntimeError(f"reference threw on {len(errs)} docs: {list(errs.items())[:3]}")
    blob = np.fromfile(os.path.join(d, "ref_dumps.bin"), np.uint8)
    off = np.fromfile(os.path.join(d, "ref_dump_off.bin"), "<i8")
    digests = np.asarray([fnv1a64(blob[off[i]: off[i + 1]].tobytes()) for i in range(hb.ndocs)], np.uint64)
    ht = json.load(open(os.path.join(d, "ref_handles.json")))
    tables = [np.asarray(ht[str(i)], np.int32) for i in range(hb.ndocs)]
    toff = np.cumsum([0] + [len(t) for t in tables]).astype(np.int64)
    nalloc = int((hb.ops["kind"] == (ol.OP_NOOP | ol.OPF_LOCAL)).sum())
    with_start = sum(1 for i in range(hb.ndocs) if len(tables[i]) > 1)
    np.savez_compressed(
        os.path.join(GOLDEN, "refhandles_c5_perm.npz"), workload=json.dumps(dataclasses.asdict(w)),
        doc_ids=np.asarray(ids, np.int64), log_sha256=log_sha(hb), digests=digests, nalloc=nalloc,
        tables=np.concatenate(tables), table_off=toff,
        source=("packages/dds/merge-tree/src + matrix handletable.ts (reference, type-erased by tools/ts_erase.py) "
                "under node by tools/ref_replay.mjs --handles"),
    )
    print(f"refhandles_c5_perm: {hb.ndocs} docs, {nalloc} getAllocatedHandle records, {with_start} docs allocated, "
          f"handle tables {min(len(t) for t in tables)}..{max(len(t) for t in tables)} entries", flush=True)


def make_relpos(node: str) -> None:
    """tests/golden/refrelpos.npz: logs whose ops name positions relative to markers (tests/relpos_logs.py,
    mt_oplog.h MT_SEG_RELPOS; Client.getValidOpRange resolves them with MergeTree.posFromRelativePos)
    replayed by the reference: its digests, and Client.posFromRelativePos of the live marker ids (before /
    after, with and without offsets) and of an id no marker holds, after each document's replay."""
    import relpos_logs
    b, interner, live = relpos_logs.build(24, 600, 7)
    d = os.path.join(SCRATCH, "relpos")
    rng = np.random.default_rng(99)
    q = []
    for i in range(b.ndocs):
        ids = live[i]
        pick = [ids[int(k)] for k in rng.choice(len(ids), size=min(6, len(ids)), replace=False)] if ids else []
        for mid in pick:
            q += [[i, mid, False, None], [i, mid, True, None], [i, mid, False, int(rng.integers(0, 5))],
                  [i, mid, True, int(rng.integers(0, 5))]]
        q.append([i, "no-such-marker", False, None])
    write_batch(b, interner, d)
    with open(os.path.join(d, "relqueries.json"), "w") as f:
        json.dump(q, f)
    r = subprocess.run([node, os.path.join(ROOT, "tools", "ref_replay.mjs"), ERASED, d], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"reference replay failed: {r.stderr[-2000:]}")
    errs = json.load(open(os.path.join(d, "ref_err.json")))["errors"]
    if errs:
        raise RuntimeError(f"reference threw on {len(errs)} docs: {list(errs.items())[:3]}")
    blob = np.fromfile(os.path.join(d, "ref_dumps.bin"), np.uint8)
    off = np.fromfile(os.path.join(d, "ref_dump_off.bin"), "<i8")
    digests = np.asarray([fnv1a64(blob[off[i]: off[i + 1]].tobytes()) for i in range(b.ndocs)], np.uint64)
    ans = json.load(open(os.path.join(d, "ref_relpos.json")))
    nrel = int(((b.ops["seg_kind"] & relpos_logs.SEG_RELPOS) != 0).sum())
    np.savez_compressed(
        os.path.join(GOLDEN, "refrelpos.npz"), ndocs=b.ndocs, nmsg=600, seed=7, log_sha256=log_sha(b),
        digests=digests, nrel=nrel, q_doc=np.asarray([x[0] for x in q], np.int32), q_id=np.asarray([x[1] for x in q]),
        q_before=np.asarray([x[2] for x in q]), q_offset=np.asarray([-1 if x[3] is None else x[3] for x in q], np.int32),
        answers=np.asarray(ans, np.int32),
        source=("packages/dds/merge-tree/src (reference, type-erased by tools/ts_erase.py) under node by "
                "tools/ref_replay.mjs: relativePos1/relativePos2 ops through Client.applyMsg, posFromRelativePos"),
    )
    print(f"refrelpos: {b.ndocs} docs, {nrel} ops with relative positions, {len(q)} posFromRelativePos queries",
          flush=True)


REGEN_SETS = ("c1_farm", "c3_lagged", "c3_lagged_long", "c5_perm")


def make_regen(names, node: str) -> None:
    """tests/golden/refregen_<set>.npz: one reconnect per document (tests/regen_inject.py: REGEN records
    for every op in flight at a seeded point; the acks of the resubmitted messages rewritten member by
    member) replayed by the reference with Client.regeneratePendingOp (tools/ref_replay.mjs --deltas):
    the digests of the replicas and their delta streams, which carry the regenerated ops
    (MT_DELTA_REGEN events) between the callbacks."""
    import regen_inject
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_ref_goldens import caps_for
    for name in names:
        w, ids = SETS[name]
        b = gen.generate(w, ids=ids, threads=8)
        c = caps_for(w)
        rb = regen_inject.inject(b, (c["ncap"], c["hcap"], c["acap"], c["mcap"], c["gcap"], c["ccap"]))
        d = os.path.join(SCRATCH, name + "_regen")
        write_batch(rb, gen.generator_interner(), d)
        r = subprocess.run([node, os.path.join(ROOT, "tools", "ref_replay.mjs"), ERASED, d, "--deltas"],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"reference replay failed: {r.stderr[-2000:]}")
        errs = json.load(open(os.path.join(d, "ref_err.json")))["errors"]
        if errs:
            raise RuntimeError(f"reference threw on {len(errs)} docs: {list(errs.items())[:3]}")
        blob = np.fromfile(os.path.join(d, "ref_dumps.bin"), np.uint8)
        off = np.fromfile(os.path.join(d, "ref_dump_off.bin"), "<i8")
        digests = np.asarray([fnv1a64(blob[off[i]: off[i + 1]].tobytes()) for i in range(rb.ndocs)], np.uint64)
        words = np.fromfile(os.path.join(d, "ref_deltas.bin"), "<i4")
        woff = np.fromfile(os.path.join(d, "ref_delta_off.bin"), "<i8")
        per = [words[woff[i]: woff[i + 1]] for i in range(rb.ndocs)]
        nregen = np.asarray([int(((rb.doc(i)[0]["kind"] & 0x90) == 0x90).sum()) for i in range(rb.ndocs)], np.int32)
        np.savez_compressed(
            os.path.join(GOLDEN, f"refregen_{name}.npz"),
            workload=json.dumps(dataclasses.asdict(w)), doc_ids=np.asarray(ids, np.int64), log_sha256=log_sha(rb),
            digests=digests, nwords=np.diff(woff).astype(np.int64),
            hashes=np.asarray([words_fnv(x) for x in per], np.uint64), nregen=nregen,
            source=("packages/dds/merge-tree/src (reference, type-erased by tools/ts_erase.py) under node by "
                    "tools/ref_replay.mjs --deltas: Client.regeneratePendingOp on reconnect"),
        )
        print(f"refregen_{name}: {rb.ndocs} docs, {int(nregen.sum())} regenerated groups", flush=True)


LEGACY_SETS = ("c1_farm", "c2_observer", "c3_lagged", "c3_lagged_long", "c4_scaled", "c2_full")
LEGACY_LOADER = 250  # the long id of the client that loads a legacy summary (a fresh one: catch-up ops are remote)


def make_legacy(names, node: str) -> None:
    """tests/golden/reflegacy_<set>.npz: SharedString's default (legacy) summary of every document after
    records [0, cut) (cut as for the v1 snapshots): the reference's SnapshotLegacy over its
    messagesSinceMSNChange (tools/ref_replay.mjs snapshotLegacyDoc), the tree's canonical SHA-256, and the
    digest of a fresh client (long id LEGACY_LOADER) that loaded it and applied its catch-up messages;
    documents whose summarizing SharedString throws (createOpsFromDelta on an annotate blocked by pending
    local rewrites) or whose tree does not load are flagged."""
    for name in names:
        w, ids = SETS[name]
        b = gen.generate(w, ids=ids, threads=8)
        cuts = [snapshot_cut(b.doc(i)[0], int(b.local_long_id[i])) for i in range(b.ndocs)]
        d = os.path.join(SCRATCH, name + "_legacy")
        write_batch(b, gen.generator_interner(), d)
        with open(os.path.join(d, "snapshots_legacy.json"), "w") as f:
            json.dump([[i, int(c), LEGACY_LOADER] for i, c in enumerate(cuts)], f)
        r = subprocess.run([node, os.path.join(ROOT, "tools", "ref_replay.mjs"), ERASED, d], capture_output=True,
                           text=True)
        if r.returncode != 0:
            raise RuntimeError(f"reference replay failed: {r.stderr[-2000:]}")
        sj = json.load(open(os.path.join(d, "ref_snapshots_legacy.json")))
        lb = np.fromfile(os.path.join(d, "ref_legacy_loaded_dumps.bin"), np.uint8)
        lo = np.fromfile(os.path.join(d, "ref_legacy_loaded_off.bin"), "<i8")
        emit_err = np.zeros(b.ndocs, bool)
        for k in sj["errors"]:
            emit_err[int(k)] = True
        load_err = np.zeros(b.ndocs, bool)
        for k in sj["loadErrors"]:
            load_err[int(k)] = True
        trees = [sj["trees"].get(str(i)) for i in range(b.ndocs)]
        np.savez_compressed(
            os.path.join(GOLDEN, f"reflegacy_{name}.npz"),
            workload=json.dumps(dataclasses.asdict(w)), doc_ids=np.asarray(ids, np.int64), log_sha256=log_sha(b),
            cut=np.asarray(cuts, np.int64), loader=LEGACY_LOADER,
            sha256=np.asarray([hashlib.sha256(canonical_tree(t).encode()).hexdigest() if t else "" for t in trees]),
            loaded_digests=np.asarray([fnv1a64(lb[lo[i]: lo[i + 1]].tobytes()) for i in range(b.ndocs)], np.uint64),
            emit_error=emit_err, load_error=load_err, keep_trees=json.dumps(trees[:2]),
            source=("packages/dds/merge-tree/src (reference, type-erased by tools/ts_erase.py) under node by "
                    "tools/ref_replay.mjs: SnapshotLegacy over SharedString's messagesSinceMSNChange, Client.load"),
        )
        print(f"reflegacy_{name}: {b.ndocs} docs; summarize throws on {int(emit_err.sum())}, load fails on "
              f"{int(load_err.sum())}; catch-up messages per doc "
              f"{[len(json.loads(sn_blobs(t)['catchupOps'])) if t else -1 for t in trees[:8]]}", flush=True)


def make_persp(node: str) -> None:
    """tests/golden/refpersp_<set>.npz: the reference's getLength, getContainingSegment + getPosition and
    getText answers at past (refSeq, clientId) perspectives inside and below the collaboration window
    (tests/persp_logs.py), after replaying whole and cut logs. Stored: the cuts, the queries, every answer
    (lengths; containing-segment tuples; text lengths and FNV-1a-64 of the UTF-16LE units)."""
    import persp_logs as pl
    for name in pl.SETS:
        b, cuts = pl.batch(name)
        q = pl.queries(b, 9000 + len(name))
        d = os.path.join(SCRATCH, name + "_persp")
        write_batch(b, gen.generator_interner(), d)
        lq = [[int(x[1]), int(x[2]), int(x[3])] for x in q if x[0] == pl.Q_LEN]
        sq = [[int(x[1]), int(x[4]), int(x[2]), int(x[3])] for x in q if x[0] == pl.Q_SEG]
        tq = [[int(x[1]), int(x[2]), int(x[3]), "", None if x[4] == -(1 << 31) else int(x[4]),
               None if x[5] == -(1 << 31) else int(x[5])] for x in q if x[0] == pl.Q_TEXT]
        for f, v in (("lenqueries.json", lq), ("queries.json", sq), ("textqueries.json", tq)):
            with open(os.path.join(d, f), "w") as fh:
                json.dump(v, fh)
        r = subprocess.run([node, os.path.join(ROOT, "tools", "ref_replay.mjs"), ERASED, d], capture_output=True,
                           text=True)
        if r.returncode != 0:
            raise RuntimeError(f"reference replay failed: {r.stderr[-2000:]}")
        errs = json.load(open(os.path.join(d, "ref_err.json")))["errors"]
        if errs:
            raise RuntimeError(f"reference threw on {len(errs)} docs: {list(errs.items())[:3]}")
        lens = json.load(open(os.path.join(d, "ref_lengths.json")))
        segs = json.load(open(os.path.join(d, "ref_answers.json")))
        texts = json.load(open(os.path.join(d, "ref_texts.json")))
        ans = np.zeros((len(q), 6), np.int64)
        il = iter(lens)
        isg = iter(segs)
        it = iter(texts)
        for i, x in enumerate(q):
            if x[0] == pl.Q_LEN:
                ans[i, 0] = next(il)
            elif x[0] == pl.Q_SEG:
                ans[i, :] = next(isg)
            else:
                t = next(it)
                ans[i, 0] = len(t)
                ans[i, 1] = np.int64(np.uint64(fnv1a64(t.encode("utf-16-le"))).view(np.int64))
        legal = np.asarray([pl.answered(b.doc(int(x[1]))[0], int(b.local_long_id[int(x[1])]), int(x[2]), int(x[3]))
                            for x in q])
        np.savez_compressed(
            os.path.join(GOLDEN, f"refpersp_{name}.npz"), cuts=cuts, log_sha256=log_sha(b), queries=q, answers=ans,
            source=("packages/dds/merge-tree/src (reference, type-erased by tools/ts_erase.py) under node by "
                    "tools/ref_replay.mjs: MergeTree.getLength / getContainingSegment + getPosition / "
                    "MergeTreeTextHelper.getText at past perspectives"))
        print(f"refpersp_{name}: {b.ndocs} docs, {len(q)} queries, {int(legal.sum())} at perspectives the engine "
              f"answers", flush=True)


def make_replaytool_seq(node: str) -> None:
    """tests/golden/refreplaytool_seq.npz: the reference tool's replicas (tools/ref_replay_tool.mjs) for recorded
    documents of a SharedObjectSequence and a SharedNumberSequence (tests/replaylog.py sequence_documents): per replica
    its getLength, getText (empty: no TextSegment) and its items (SharedSequence.getItems(0) over the reference Client)
    as the length and FNV-1a-64 of their JSON; the observers' items JSON in full."""
    import replaylog
    rows, obs, shas = [], [], []
    for k, msgs in enumerate(replaylog.sequence_documents()):
        d = os.path.join(SCRATCH, f"replaytool_seq_{k}")
        os.makedirs(d, exist_ok=True)
        blob = json.dumps(msgs)
        shas.append(hashlib.sha256(blob.encode()).hexdigest())
        with open(os.path.join(d, "messages.json"), "w") as f:
            f.write(blob)
        r = subprocess.run([node, os.path.join(ROOT, "tools", "ref_replay_tool.mjs"), ERASED,
                            os.path.join(d, "messages.json"), os.path.join(d, "out.json")], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"reference replay tool failed: {r.stderr[-2000:]}")
        reps = json.load(open(os.path.join(d, "out.json")))["replicas"]
        for path, client, text, length, items in reps:
            ij = json.dumps(items, separators=(",", ":"))
            rows.append([k, path, client, len(text), length, len(items), fnv1a64(ij.encode())])
            if client == "readonly":
                obs.append(ij)
        print(f"replaytool seq doc {k}: {len(reps)} replicas, lengths {sorted(set(x[3] for x in reps))}", flush=True)
    np.savez_compressed(
        os.path.join(GOLDEN, "refreplaytool_seq.npz"),
        doc=np.asarray([x[0] for x in rows], np.int32), path=np.asarray([x[1] for x in rows]),
        client=np.asarray([x[2] for x in rows]), text_len=np.asarray([x[3] for x in rows], np.int64),
        length=np.asarray([x[4] for x in rows], np.int64), nitems=np.asarray([x[5] for x in rows], np.int64),
        items_fnv=np.asarray([x[6] for x in rows], np.uint64), observer_items=np.asarray(obs),
        log_sha256=np.asarray(shas),
        source=("packages/dds/merge-tree/src + sequence sharedSequence.ts SubSequence (reference, type-erased by "
                "tools/ts_erase.py) under node by tools/ref_replay_tool.mjs: clientReplayTool.ts's reconstruction of "
                "object / number sequence trees over the reference Client"))


def make_replaytool(node: str) -> None:
    """tests/golden/refreplaytool.npz: the reference merge-tree client replay tool's per-client replicas
    (clientReplayTool.ts:113-258, restated over the reference Client by tools/ref_replay_tool.mjs) for the
    recorded-document logs of tests/replaylog.py: per replica its merge tree, client, getLength and the length
    and FNV-1a-64 (UTF-16LE) of getText; the logs' SHA-256; the observer's full texts; and `literal`: per log
    what the tool's loop does as written (tools/ref_replay_tool.mjs --literal: the exception that ends it, or
    its assert's outcome)."""
    import replaylog
    rows, texts, shas, literal = [], [], [], []
    for k, msgs in enumerate(replaylog.documents()):
        d = os.path.join(SCRATCH, f"replaytool_{k}")
        os.makedirs(d, exist_ok=True)
        blob = json.dumps(msgs)
        shas.append(hashlib.sha256(blob.encode()).hexdigest())
        with open(os.path.join(d, "messages.json"), "w") as f:
            f.write(blob)
        r = subprocess.run([node, os.path.join(ROOT, "tools", "ref_replay_tool.mjs"), ERASED,
                            os.path.join(d, "messages.json"), os.path.join(d, "out.json")], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"reference replay tool failed: {r.stderr[-2000:]}")
        reps = json.load(open(os.path.join(d, "out.json")))["replicas"]
        for path, client, text, length in (r[:4] for r in reps):
            rows.append([k, path, client, len(text), fnv1a64(text.encode("utf-16-le")), length])
            if client == "readonly":
                texts.append(text)
        print(f"replaytool doc {k}: {len(reps)} replicas, lengths {sorted(set(x[3] for x in reps))}", flush=True)
        # the tool's loop as written (clientReplayTool.ts:211 tests `!==`): what it does on the same log
        r = subprocess.run([node, os.path.join(ROOT, "tools", "ref_replay_tool.mjs"), ERASED,
                            os.path.join(d, "messages.json"), os.path.join(d, "literal.json"), "--literal"],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"reference replay tool (literal) failed: {r.stderr[-2000:]}")
        literal.append(json.load(open(os.path.join(d, "literal.json")))["literal"])
        print(f"replaytool doc {k}: the loop as written: {literal[-1]}", flush=True)
    np.savez_compressed(
        os.path.join(GOLDEN, "refreplaytool.npz"),
        doc=np.asarray([x[0] for x in rows], np.int32), path=np.asarray([x[1] for x in rows]),
        client=np.asarray([x[2] for x in rows]), text_len=np.asarray([x[3] for x in rows], np.int64),
        text_fnv=np.asarray([x[4] for x in rows], np.uint64), length=np.asarray([x[5] for x in rows], np.int64),
        observer_texts=np.asarray(texts), log_sha256=np.asarray(shas), literal=json.dumps(literal),
        source=("packages/dds/merge-tree/src (reference, type-erased by tools/ts_erase.py) under node by "
                "tools/ref_replay_tool.mjs: clientReplayTool.ts's reconstruction over the reference Client"))


SUBSEQ_SETS = ("c2_observer", "c3_lagged", "c4_scaled")


def make_subseq(node: str) -> None:
    """tests/golden/refsubseq_<set>.npz: the sets' logs with every TextSegment insert made a SubSequence insert of the
    same units as numbers (tests/subseq_logs.py: a SharedNumberSequence replica's log; sequence sharedSequence.ts:18-101)
    replayed by the reference Client with the sequence package's own SubSequence class (type-erased beside merge-tree):
    per-document digests (SubSequence rows dump as kind 3 with their items), SnapshotV1 summaries at a cut loaded by a
    fresh reference Client and replayed to the end (tree hashes, loaded digests), and the first documents' logs and
    dumps. The oracle must agree on every digest."""
    import oracle_client as oc
    import subseq_logs
    for name in SUBSEQ_SETS:
        w, ids = SETS[name]
        b = subseq_logs.to_run(gen.generate(w, ids=ids, threads=8))
        cuts = [snapshot_cut(b.doc(i)[0], int(b.local_long_id[i])) for i in range(b.ndocs)]
        dumps, info, secs, (trees, loaded, tail_err, tail_msgs, load_err, load_msgs) = run_reference(
            b, os.path.join(SCRATCH, name + "_subseq"), node, cuts)
        digests = np.asarray([fnv1a64(x) for x in dumps], np.uint64)
        orig = np.load(os.path.join(GOLDEN, f"ref_{name}.npz"))["digests"]
        _, odig, oerr = oc.replay_batch(b, threads=8)
        agree = int((odig == digests).sum())
        nrun = int(sum(x.count(bytes([3])) > 0 for x in dumps))
        print(f"refsubseq_{name}: {b.ndocs} docs, {b.nops} events, reference {info['seconds']:.2f}s; oracle agrees on "
              f"{agree}/{b.ndocs}; {int((digests != orig).sum())} digests differ from the TextSegment logs'; "
              f"{len(tail_msgs)} loaded replicas throw, {len(load_msgs)} snapshots do not load", flush=True)
        keep = b.subset(range(min(KEEP.get(name, KEEP_LOGS), b.ndocs)))
        np.savez_compressed(
            os.path.join(GOLDEN, f"refsubseq_{name}.npz"),
            workload=json.dumps(dataclasses.asdict(w)), doc_ids=np.asarray(ids, np.int64), log_sha256=log_sha(b),
            digests=digests, nevents=np.diff(b.op_off),
            keep_ops=keep.ops, keep_op_off=keep.op_off, keep_text=keep.text, keep_text_off=keep.text_off,
            keep_local=keep.local_long_id,
            keep_dumps=np.frombuffer(b"".join(dumps[: keep.ndocs]), np.uint8),
            keep_dump_off=np.concatenate([[0], np.cumsum([len(x) for x in dumps[: keep.ndocs]])]).astype(np.int64),
            snap_cut=np.asarray(cuts, np.int64),
            snap_sha256=np.asarray([hashlib.sha256(canonical_tree(t).encode()).hexdigest() for t in trees]),
            snap_loaded_digests=np.asarray([fnv1a64(x) for x in loaded], np.uint64),
            snap_tail_error=tail_err,
            snap_load_error=load_err,
            keep_snap_trees=json.dumps(trees[: keep.ndocs]),
            source=("packages/dds/merge-tree/src + packages/dds/sequence/src/sharedSequence.ts SubSequence (reference, "
                    "type-erased by tools/ts_erase.py) under node by tools/ref_replay.mjs; logs: tests/subseq_logs.py"),
        )
        del nrun


def item_queries(b, seed: int):
    """getItems(start, end) queries per document in the local view: the whole sequence (end undefined), ranges inside,
    a range starting at 0, an empty and a reversed range (none), a negative start, ends past the length; lengths are
    not known here, so ranges are drawn up to 1,500 and the reference clips them."""
    q = []
    rng = np.random.default_rng(seed)
    for d in range(b.ndocs):
        q.append([d, 0, None])
        for _ in range(6):
            a, e = sorted(int(x) for x in rng.integers(0, 1500, 2))
            q.append([d, a, e])
            q.append([d, a, None])
        a = int(rng.integers(0, 1500))
        q += [[d, 0, a], [d, a, a], [d, a + 9, a], [d, -3, int(rng.integers(1, 1500))], [d, a, 4000]]
    return q


def make_items(node: str) -> None:
    """tests/golden/refitems_c3_markers.npz: config-3 logs with markers (tests/text_markers.py) whose TextSegment
    inserts are SubSequence inserts (tests/subseq_logs.py), replayed by the reference: per-document digests and
    SharedSequence.getItems(start, end) answers (sharedSequence.ts:150-183 over the reference Client; its splice-based
    cut makes a marker inside the range shift the answer) as lengths, FNV-1a-64 over the item ids (uint16 LE), and
    document 0's answers in full."""
    import oracle_client as oc
    import subseq_logs
    import text_markers
    w, ids = TEXT_SETS["c3_markers"]
    b = subseq_logs.to_run(text_markers.with_markers(gen.generate(w, ids=ids, threads=8)))
    q = item_queries(b, 777)
    d = os.path.join(SCRATCH, "c3_markers_items")
    write_batch(b, gen.generator_interner(), d)
    with open(os.path.join(d, "itemqueries.json"), "w") as f:
        json.dump(q, f)
    dumps, info, secs, _ = run_reference(b, d, node)
    items = json.load(open(os.path.join(d, "ref_items.json")))
    assert len(items) == len(q)
    digests = np.asarray([fnv1a64(x) for x in dumps], np.uint64)
    _, odig, _ = oc.replay_batch(b, threads=8)
    units = [np.asarray(x, "<u2").tobytes() for x in items]
    qa = np.asarray([[x[0], x[1], -(1 << 31) if x[2] is None else x[2]] for x in q], np.int32)
    blob = np.frombuffer(b"".join(u for (x, u) in zip(q, units) if x[0] == 0), np.uint8)
    np.savez_compressed(
        os.path.join(GOLDEN, "refitems_c3_markers.npz"),
        workload=json.dumps(dataclasses.asdict(w)), doc_ids=np.asarray(ids, np.int64), log_sha256=log_sha(b),
        digests=digests, queries=qa, lengths=np.asarray([len(x) for x in items], np.int64),
        fnv=np.asarray([fnv1a64(u) for u in units], np.uint64), doc0_units=blob,
        source=("packages/dds/merge-tree/src + sequence sharedSequence.ts SubSequence (reference, type-erased by "
                "tools/ts_erase.py) under node by tools/ref_replay.mjs: SharedSequence.getItems after each replay"),
    )
    print(f"refitems_c3_markers: {b.ndocs} docs, {len(q)} queries, {sum(len(x) for x in items)} items; oracle agrees "
          f"on {int((odig == digests).sum())}/{b.ndocs} digests", flush=True)


SESSION_SETS = {  # name -> (workload, document ids): remote clients renamed per message (tests/session_logs.py, p = 1)
    "c3_sessions": (gen.config3(4096), list(range(16))),
    "c2_sessions": (gen.config2(2000), list(range(16))),
    "c4_sessions": (gen.config4(20000), list(range(2))),
    "c5_sessions": (gen.config5(1500), list(range(16))),
}


def make_sessions(node: str) -> None:
    """tests/golden/refsess_<set>.npz: documents whose remote clients reconnect under new long ids at every message
    that covers their previous one (hundreds to thousands of distinct clients per document: more than the engine's
    253 short-id slots), replayed by the reference: per-document digests (the dump's client fields are long ids, so
    every retired row's client must come back exactly), the distinct client counts, and the first documents' dumps."""
    import oracle_client as oc
    import session_logs
    for name, (w, ids) in SESSION_SETS.items():
        b = session_logs.with_sessions(gen.generate(w, ids=ids, threads=8), p=1.0)
        dumps, info, secs, _ = run_reference(b, os.path.join(SCRATCH, name), node)
        digests = np.asarray([fnv1a64(x) for x in dumps], np.uint64)
        _, odig, oerr = oc.replay_batch(b, threads=8)
        print(f"refsess_{name}: {b.ndocs} docs, {b.nops} events, clients per doc {min(b.nclients)}-{max(b.nclients)}; "
              f"reference {info['seconds']:.2f}s; oracle agrees on {int((odig == digests).sum())}/{b.ndocs}", flush=True)
        keep = min(2, b.ndocs)
        np.savez_compressed(
            os.path.join(GOLDEN, f"refsess_{name}.npz"),
            workload=json.dumps(dataclasses.asdict(w)), doc_ids=np.asarray(ids, np.int64), log_sha256=log_sha(b),
            digests=digests, nclients=np.asarray(b.nclients, np.int64), session_p=1.0,
            keep_dumps=np.frombuffer(b"".join(dumps[:keep]), np.uint8),
            keep_dump_off=np.concatenate([[0], np.cumsum([len(x) for x in dumps[:keep]])]).astype(np.int64),
            source=("packages/dds/merge-tree/src (reference, type-erased by tools/ts_erase.py) under node by "
                    "tools/ref_replay.mjs; logs: tests/session_logs.py over the in-repo generator"),
        )


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default=",".join(SETS))
    ap.add_argument("--node", default="node")
    ap.add_argument("--deltas", action="store_true", help="write the delta-stream fixtures (refdelta_*.npz) only")
    ap.add_argument("--refs", action="store_true", help="write the local-reference fixtures (refrefs_*.npz) only")
    ap.add_argument("--regen", action="store_true", help="write the reconnect fixtures (refregen_*.npz) only")
    ap.add_argument("--legacy", action="store_true", help="write the legacy-summary fixtures (reflegacy_*.npz) only")
    ap.add_argument("--texts", action="store_true", help="write the getText fixtures (reftext_*.npz) only")
    ap.add_argument("--handles", action="store_true", help="write the PermutationVector handle fixture only")
    ap.add_argument("--relpos", action="store_true", help="write the relative-position fixture (refrelpos.npz) only")
    ap.add_argument("--tree", action="store_true", help="write the MergeTree-level record fixtures (reftree_*.npz) only")
    ap.add_argument("--combine", action="store_true", help="write the incr / consensus combining-op fixture only")
    ap.add_argument("--hsnap", action="store_true", help="write the SharedMatrix summary-with-handles fixture only")
    ap.add_argument("--refentry", action="store_true", help="write the refsByOffset-entry KAT fixture only")
    ap.add_argument("--unref", action="store_true", help="write the removeLocalReference fixtures (refunref_*.npz) only")
    ap.add_argument("--persp", action="store_true", help="write the past-perspective read fixtures (refpersp_*.npz) only")
    ap.add_argument("--replaytool", action="store_true", help="write the client replay tool fixture only")
    ap.add_argument("--subseq", action="store_true", help="write the SubSequence fixtures (refsubseq_*.npz) only")
    ap.add_argument("--zamboni", action="store_true", help="write the zamboni edge-case fixture (refzamboni.npz) only")
    ap.add_argument("--ranges", action="store_true", help="write the wide range-edit fixture (refranges.npz) only")
    ap.add_argument("--reconnect", action="store_true", help="write the hand-built reconnect fixture (refreconnect.npz) only")
    ap.add_argument("--inserts", action="store_true", help="write the insert placement / split fixture (refinserts.npz) only")
    ap.add_argument("--tiles", action="store_true", help="write the marker-query fixture (reftiles.npz) only")
    ap.add_argument("--hvec", action="store_true", help="write the batched PermutationVector read fixture (refhvec.npz) only")
    ap.add_argument("--props", action="store_true", help="write the property-manager fixture (refprops.npz) only")
    ap.add_argument("--sessions", action="store_true", help="write the many-client fixtures (refsess_*.npz) only")
    args = ap.parse_args()
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ts_erase.py"), "--out", ERASED], check=True)
    if args.sessions:
        make_sessions(args.node)
        return
    if args.zamboni:
        make_zamboni(args.node)
        return
    if args.ranges:
        make_ranges(args.node)
        return
    if args.reconnect:
        make_reconnect(args.node)
        return
    if args.inserts:
        make_inserts(args.node)
        return
    if args.tiles:
        make_tiles(args.node)
        return
    if args.hvec:
        make_hvec(args.node)
        return
    if args.props:
        make_props(args.node)
        return
    if args.subseq:
        make_subseq(args.node)
        make_items(args.node)
        return
    if args.replaytool:
        make_replaytool(args.node)
        make_replaytool_seq(args.node)
        return
    if args.persp:
        make_persp(args.node)
        return
    if args.texts:
        make_texts(args.node)
        return
    if args.tree:
        make_tree(args.node)
        return
    if args.relpos:
        make_relpos(args.node)
        return
    if args.handles:
        make_handles(args.node)
        return
    if args.legacy:
        make_legacy([n for n in args.sets.split(",") if n in LEGACY_SETS], args.node)
        return
    if args.regen:
        make_regen([n for n in args.sets.split(",") if n in REGEN_SETS], args.node)
        return
    if args.refs:
        make_refs([n for n in args.sets.split(",") if n in REF_SETS], args.node)
        return
    if args.refentry:
        make_refentry(args.node)
        return
    if args.hsnap:
        make_handle_snaps(args.node)
        return
    if args.combine:
        make_combine(args.node)
        return
    if args.unref:
        make_refs([n for n in args.sets.split(",") if n in REF_SETS], args.node, removals=True)
        return
    if args.deltas:
        make_deltas([n for n in args.sets.split(",") if n in SETS], args.node)
        return
    import oracle_client as oc
    if "snap_body" in args.sets.split(","):
        make_snap_body(args.node)

    os.makedirs(GOLDEN, exist_ok=True)
    for name in args.sets.split(","):
        if name == "snap_body":
            continue
        w, ids = SETS[name]
        b = gen.generate(w, ids=ids, threads=8)
        cuts = [snapshot_cut(b.doc(i)[0], int(b.local_long_id[i])) for i in range(b.ndocs)]
        dumps, info, secs, (trees, loaded, tail_err, tail_msgs, load_err, load_msgs) = run_reference(
            b, os.path.join(SCRATCH, name), args.node, cuts)
        if load_msgs:
            print(f"  reference: {len(load_msgs)} snapshots do not load in the reference itself: "
                  f"{sorted(set(m for m in load_msgs.values()))[:2]}")
        if tail_msgs:
            print(f"  reference: {len(tail_msgs)} loaded replicas cannot apply the rest of their log: "
                  f"{sorted(set(m for _, m in tail_msgs.values()))[:3]}")
        digests = np.asarray([fnv1a64(x) for x in dumps], np.uint64)
        _, odig, oerr = oc.replay_batch(b, threads=8)
        agree = int((odig == digests).sum())
        print(f"{name}: {b.ndocs} docs, {b.nops} events, reference {info['seconds']:.2f}s; "
              f"oracle agrees on {agree}/{b.ndocs} digests", flush=True)
        keep = b.subset(range(min(KEEP.get(name, KEEP_LOGS), b.ndocs)))
        np.savez_compressed(
            os.path.join(GOLDEN, f"ref_{name}.npz"),
            workload=json.dumps(dataclasses.asdict(w)), doc_ids=np.asarray(ids, np.int64), log_sha256=log_sha(b),
            digests=digests, nevents=np.diff(b.op_off),
            keep_ops=keep.ops, keep_op_off=keep.op_off, keep_text=keep.text, keep_text_off=keep.text_off,
            keep_local=keep.local_long_id,
            keep_dumps=np.frombuffer(b"".join(dumps[: keep.ndocs]), np.uint8),
            keep_dump_off=np.concatenate([[0], np.cumsum([len(x) for x in dumps[: keep.ndocs]])]).astype(np.int64),
            # snapshots: the replica after records [0, cut) summarized by SnapshotV1, loaded by a fresh
            # client (same long id) that applies [cut, end): canonical tree hashes, loaded digests, and
            # the trees of the first docs
            snap_cut=np.asarray(cuts, np.int64),
            snap_sha256=np.asarray([hashlib.sha256(canonical_tree(t).encode()).hexdigest() for t in trees]),
            snap_loaded_digests=np.asarray([fnv1a64(x) for x in loaded], np.uint64),
            snap_tail_error=tail_err,
            snap_load_error=load_err,
            keep_snap_trees=json.dumps(trees[: keep.ndocs]),
            source=("packages/dds/merge-tree/src (reference, type-erased by tools/ts_erase.py, run under node "
                    f"{subprocess.run([args.node, '--version'], capture_output=True, text=True).stdout.strip()} by "
                    "tools/ref_replay.mjs)"),
        )


if __name__ == "__main__":
    main()
