"use strict";
// The batched delta-event read from JavaScript: addon.deltasBatch and ReplayEngine.deltaEvents against the
// per-document GpuClient.deltaEvents of the same engine. Run by tests/test_napi_deltas.py (GPU tier); prints one
// JSON line of results.
const { ReplayEngine, DEFAULT_CAPS, DELTA_KINDS, decodeDeltas, addon } = require("../fluidframework_amd/js/mergetree_gpu.js");

const out = {};
const N = 5;
const eng = new ReplayEngine(N, { ...DEFAULT_CAPS, dcap: 4096 });
const c = Array.from({ length: N }, (_, d) => eng.client(d));
eng.startCollaboration(Array.from({ length: N }, () => "me"));
const seq = new Array(N).fill(0);
function msg(d, contents) {
    seq[d]++;
    c[d].applyMsg({ clientId: "B", sequenceNumber: seq[d], referenceSequenceNumber: seq[d] - 1, minimumSequenceNumber: 0,
        type: "op", contents });
}
// document d: a text, d inserts inside it (each splits a row), an annotate and a remove across rows; document 4 stays
// empty
for (let d = 0; d < N - 1; d++) {
    msg(d, { type: 0, pos1: 0, seg: "hello world, hello rows" });
    for (let k = 0; k < d; k++) msg(d, { type: 0, pos1: 2 + 3 * k, seg: "X" });
    msg(d, { type: 2, pos1: 1, pos2: 9, props: { bold: true, size: d } });
    msg(d, { type: 1, pos1: 4, pos2: 12 });
}
out.single = c.map((x) => x.deltaEvents());
out.batch = eng.deltaEvents();
out.listed = eng.deltaEvents([3, 1, 3, 4]);
out.sequence = eng.deltaEvents(undefined, { kinds: DELTA_KINDS.SEQUENCE });
out.maintenance = eng.deltaEvents(undefined, { kinds: DELTA_KINDS.MAINTENANCE });
const raw = addon.deltasBatch(eng.h, [2, 0]);
out.raw = { off: raw.off, end: raw.end, emitted: raw.emitted, status: Array.from(raw.status), nwords: raw.words.length,
    events: [0, 1].map((i) => decodeDeltas(raw.words.subarray(raw.off[i], raw.off[i + 1]), eng.interner)) };
// a cursor: more events in documents 2 and 0, read from the `end` of the call before; one cursor inside an event
msg(2, { type: 0, pos1: 1, seg: "Y" });
msg(0, { type: 1, pos1: 0, pos2: 2 });
eng.flush();
const tail = addon.deltasBatch(eng.h, [2, 0, 2], [raw.end[0], raw.end[1], 3], DELTA_KINDS.SEQUENCE | DELTA_KINDS.MAINTENANCE);
out.tail = { status: Array.from(tail.status),
    events: [0, 1, 2].map((i) => decodeDeltas(tail.words.subarray(tail.off[i], tail.off[i + 1]), eng.interner)) };
out.after = [2, 0].map((d) => c[d].deltaEvents());
try {
    addon.deltasBatch(eng.h, [0], undefined, 0);
    out.kinds0 = "accepted";
} catch (e) {
    out.kinds0 = e.message;
}
try {
    new ReplayEngine(1).deltaEvents();
    out.nodcap = "accepted";
} catch (e) {
    out.nodcap = e.message;
}
console.log(JSON.stringify(out));
