"use strict";
// The marker-query fixture through node: the hand-built logs of tests/tile_logs.py (written by tests/test_napi_tiles.py
// into the directory given as the argument: the batch's raw arrays, the interner's tables, the fixture's queries) are
// replayed by ReplayEngines of the small, flat and tiled capacities through the Node-API addon on the GPU, and every
// query is asked twice: batched (ReplayEngine.findTiles / stackContexts, one call per label) and through the document's
// GpuClient (findTile / getStackContext). The Python side compares the answers with the reference Client's own
// (tests/golden/reftiles.npz). For a document the engine refuses (an annotate changed the label key on a marker)
// GpuClient.findTile must still give its dump walk's answer. Prints one JSON line.
const fs = require("fs");
const path = require("path");
const { ReplayEngine, addon } = require("../fluidframework_amd/js/mergetree_gpu.js");

const dir = process.argv[2];
const meta = JSON.parse(fs.readFileSync(path.join(dir, "meta.json")));
const bytes = (d, f) => { const b = fs.readFileSync(path.join(d, f)); return new Uint8Array(b.buffer, b.byteOffset, b.length).slice(); };
const i64 = (d, f) => new BigInt64Array(bytes(d, f).buffer);
const u16 = (d, f) => new Uint16Array(bytes(d, f).buffer);
const undef = (p) => (p < 0 ? undefined : p);
const out = {};
for (const run of meta.runs) {
    const d = path.join(dir, run.name);
    const eng = new ReplayEngine(run.ndocs, run.caps);
    meta.keys.forEach((k, i) => { if (i) eng.interner.keys.set(k, i); });
    eng.interner.nk = meta.keys.length;
    meta.values.forEach((v, i) => { if (i) eng.interner.values.set(v, i); });
    eng.interner.nv = meta.values.length;
    addon.startCollab(eng.h, Int32Array.from(run.local), 0, 0);
    addon.submit(eng.h, bytes(d, "ops.bin"), i64(d, "op_off.bin"), u16(d, "text.bin"), i64(d, "text_off.bin"),
        bytes(d, "props.bin"), i64(d, "props_off.bin"), bytes(d, "kv.bin"), i64(d, "kv_off.bin"));
    addon.run(eng.h);
    addon.sync(eng.h);
    const res = { errors: Array.from(addon.errors(eng.h)[0]), tiles: [], stacks: [], clientTiles: [], clientStacks: [],
        fallback: [] };
    const labels = (qs) => [...new Set(qs.map((q) => q[1]))];
    res.tiles = new Array(run.tiles.length);
    for (const label of labels(run.tiles)) {
        const at = run.tiles.map((q, i) => i).filter((i) => run.tiles[i][1] === label);
        const r = eng.findTiles(at.map((i) => ({ doc: run.tiles[i][0], pos: undef(run.tiles[i][2]), preceding: run.tiles[i][3] })), label);
        at.forEach((i, k) => { res.tiles[i] = r[k] === undefined ? [0, -1, -1] : r[k].unsupported ? "unsupported" : [1, r[k].pos, r[k].ordinal]; });
    }
    res.stacks = new Array(run.stacks.length);
    for (const label of labels(run.stacks)) {
        const at = run.stacks.map((q, i) => i).filter((i) => run.stacks[i][1] === label);
        const r = eng.stackContexts(at.map((i) => ({ doc: run.stacks[i][0], pos: undef(run.stacks[i][2]) })), label);
        at.forEach((i, k) => { res.stacks[i] = r[k].unsupported ? "unsupported" : r[k].map((e) => [e.ordinal, e.refType]); });
    }
    const clients = new Map();
    const client = (doc) => { if (!clients.has(doc)) clients.set(doc, eng.client(doc)); return clients.get(doc); };
    for (const [doc, label, pos, pre] of run.tiles) {
        const c = client(doc);
        const a = c.findTile(undef(pos), label, pre);
        const segs = c.segments().segments;
        res.clientTiles.push(a === undefined ? [0, -1, -1] : [1, a.pos, segs.indexOf(a.tile)]);
        if (run.refused.includes(doc)) {
            const b = c._findTileByDump(undef(pos), label, pre);
            res.fallback.push((a === undefined) === (b === undefined) && (a === undefined || (a.tile === b.tile && a.pos === b.pos)));
        }
    }
    for (const [doc, label, pos] of run.stacks) {
        const c = client(doc);
        try {
            const st = c.getStackContext(undef(pos), [label, "no-such-label"]);
            const segs = c.segments().segments;
            res.clientStacks.push(st["no-such-label"].length === 0 ? st[label].map((s) => [segs.indexOf(s), s.refType]) : "extra");
        } catch (e) {
            res.clientStacks.push(/unsupported/.test(String(e.message)) ? "unsupported" : String(e.message));
        }
    }
    out[run.name] = res;
}
console.log(JSON.stringify(out));
