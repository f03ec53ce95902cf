"use strict";
// The PermutationVector read fixture through node: the hand-built logs of tests/hvec_logs.py (written by
// tests/test_napi_hvec.py into the directory given as the argument: the batch's raw arrays and the fixture's queries) are
// replayed by ReplayEngines of the small, matrix and tiled capacities through the Node-API addon on the GPU, and every
// query is asked twice: batched (ReplayEngine.getHandles / handlesToPositions / handleTables, one call each) and through
// the document's GpuClient (getHandles, getMaybeHandle per position, handleToPosition, handleTable). The Python side
// compares the answers with the reference's (tests/golden/refhvec.npz). Prints one JSON line.
const fs = require("fs");
const path = require("path");
const { ReplayEngine, addon } = require("../fluidframework_amd/js/mergetree_gpu.js");

const dir = process.argv[2];
const meta = JSON.parse(fs.readFileSync(path.join(dir, "meta.json")));
const bytes = (d, f) => { const b = fs.readFileSync(path.join(d, f)); return new Uint8Array(b.buffer, b.byteOffset, b.length).slice(); };
const i64 = (d, f) => new BigInt64Array(bytes(d, f).buffer);
const u16 = (d, f) => new Uint16Array(bytes(d, f).buffer);
const undef = (v) => (v === null ? undefined : v);
const out = {};
for (const run of meta.runs) {
    const d = path.join(dir, run.name);
    const eng = new ReplayEngine(run.ndocs, run.caps);
    addon.startCollab(eng.h, Int32Array.from(run.local), 0, 0);
    addon.submit(eng.h, bytes(d, "ops.bin"), i64(d, "op_off.bin"), u16(d, "text.bin"), i64(d, "text_off.bin"),
        bytes(d, "props.bin"), i64(d, "props_off.bin"), bytes(d, "kv.bin"), i64(d, "kv_off.bin"));
    addon.run(eng.h);
    addon.sync(eng.h);
    const res = { errors: Array.from(addon.errors(eng.h)[0]) };
    // batched: every query of the run in one call each
    res.ranges = eng.getHandles(run.ranges.map(([doc, start, end]) => ({ doc, start, end })))
        .map((h) => (h === undefined ? null : Array.from(h)));
    res.positions = eng.handlesToPositions(run.positions.map(([doc, handle, ls]) => ({ doc, handle, localSeq: undef(ls) })))
        .map((p) => (p === undefined ? null : p));
    res.tables = eng.handleTables().map((t) => Array.from(t));
    res.someTables = eng.handleTables([run.ndocs - 1, 0, run.ndocs - 1]).map((t) => Array.from(t));
    // per client
    const clients = new Map();
    const client = (doc) => { if (!clients.has(doc)) clients.set(doc, eng.client(doc)); return clients.get(doc); };
    res.clientRanges = run.ranges.map(([doc, start, end]) => {
        try { return Array.from(client(doc).getHandles(start, end)); } catch (e) { return null; }
    });
    // getMaybeHandle position by position: each document's whole vector once, every window is a slice of it
    res.single = [];
    for (let doc = 0; doc < run.ndocs; doc++) {
        const c = client(doc), n = c.getLength(), v = new Array(n);
        for (let p = 0; p < n; p++) v[p] = c.getMaybeHandle(p);
        res.single.push(v);
    }
    res.clientPositions = run.positions.map(([doc, handle, ls]) => {
        try { return client(doc).handleToPosition(handle, undef(ls)); } catch (e) { return null; }
    });
    res.clientTables = Array.from({ length: run.ndocs }, (_, doc) => Array.from(client(doc).handleTable()));
    out[run.name] = res;
}
console.log(JSON.stringify(out));
