/*
 * mt_engine.h — C ABI of the MI355X merge-tree replay engine (libmtreplay.so).
 *
 * The reference has no FFI for this path: its boundary is the TypeScript module
 * @fluidframework/merge-tree (packages/dds/merge-tree/src/index.ts:6-22), whose `Client` is
 * called by SharedSegmentSequence (packages/dds/sequence/src/sequence.ts:579-616) and
 * SharedMatrix/PermutationVector (packages/dds/matrix/src/matrix.ts:568-578). The entry points
 * below are what a Node-API addon binding that module's hot path would call;
 * each cites the reference member it replaces. One engine = a batch of documents resident in
 * one GPU's HBM, one replica per document. All calls are synchronous unless noted; errors
 * are returned as MT_E_* status codes (no exceptions cross the ABI) and per-document replay
 * errors are latched and reported by mt_engine_errors (the reference throws synchronously).
 */
#ifndef MT_ENGINE_H
#define MT_ENGINE_H
#include <stdint.h>

#include "mt_oplog.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mt_engine mt_engine;

/* Per-document capacities (device memory is sized from these). */
typedef struct mt_caps {
    int32_t ncap; /* B-tree nodes per doc; row slots = 8 * ncap                        */
    int32_t hcap; /* zamboni LRU heap entries (collections.ts:212-264)                 */
    int32_t acap; /* text arena half size, UTF-16 units                                 */
    int32_t mcap; /* pending segment-group membership log entries                       */
    int32_t gcap; /* pending local ops (segment groups) in flight                       */
    int32_t ccap; /* distinct clients per doc (<= 254)                                  */
    int32_t dcap; /* delta event log words per doc; 0 = no delta events (mt_oplog.h)   */
    int32_t rcap; /* local references per doc (MT_OP_REF records); 0 = none           */
    int32_t pcap; /* PermutationVector handles per doc (getAllocatedHandle records); 0 = none */
} mt_caps;

/* status codes */
enum {
    MT_OK = 0,
    MT_E_INSERT_FAILED = 1, /* per doc: mergeTree.ts:2243-2249 "MergeTree insert failed"       */
    MT_E_ASSERT = 2,        /* per doc: a reference `assert` would have thrown                 */
    MT_E_INVALID_RANGE = 3, /* reserved (a local op getValidOpRange rejects is a no-op, client.ts:486) */
    MT_E_UNSUPPORTED = 4,   /* per doc: a path the engine does not model (mt_oplog.h)          */
    MT_E_CAPACITY = 5,      /* per doc: a capacity was exceeded even after promotion (mt_engine_sync) */
    MT_E_ARG = 16,          /* engine: bad argument                                            */
    MT_E_HIP = 17,          /* engine: HIP runtime error (mt_engine_last_error has the text)  */
    MT_E_NOMEM = 18,        /* engine: device allocation failed                                */
};

/* Create an engine with `ndocs` empty, non-collaborating replicas on HIP device `device`
 * (new Client() + MergeTree constructor, client.ts:75-84, mergeTree.ts:1143-1146). */
int32_t mt_engine_create(int32_t device, int64_t ndocs, const mt_caps* caps, mt_engine** out);
void mt_engine_destroy(mt_engine* e);
const char* mt_engine_last_error(const mt_engine* e);

/* Client.startOrUpdateCollaboration(longClientId, minSeq, currentSeq) for every doc
 * (client.ts:1053-1073); local_long_ids[d] is doc d's own long-client index. */
int32_t mt_engine_start_collab(mt_engine* e, const int32_t* local_long_ids, int32_t min_seq, int32_t cur_seq);
/* The same with each document's own minSeq and currentSeq (client.ts:1053-1073 per replica): a
 * batch of documents that join collaboration at different points of their streams (e.g. loaded from
 * summaries taken at different sequence numbers). Reset returns every document to these. */
int32_t mt_engine_start_collab_docs(mt_engine* e, const int32_t* local_long_ids, const int32_t* min_seqs,
                                    const int32_t* cur_seqs);

/* Stage a batch of per-doc event streams (host memory; copied to HBM). Doc d's events are
 * ops[op_off[d] .. op_off[d+1]), its pools start at text+text_off[d], props+props_off[d],
 * kv+kv_off[d] (pools may be shared between docs). Replaces the previous staged batch. */
int32_t mt_engine_submit(mt_engine* e, const mt_op_rec* ops, const int64_t* op_off, const uint16_t* text,
                         int64_t text_units, const int64_t* text_off, const mt_props_rec* props, int64_t nprops,
                         const int64_t* props_off, const mt_kv* kv, int64_t nkv, const int64_t* kv_off);

/* mt_engine_submit + mt_engine_run with the hand-off overlapped: the documents go in chunks (an eighth of the batch, at
 * least the documents the GPU holds at once), and chunk k's records replay while chunk k+1's are checked on the host
 * and copied (from pinned memory directly, from pageable memory through the engine's pinned staging buffers). The
 * same results as submit + run; returns once every record has been copied (the caller's buffers are free again), with
 * the replay running (mt_engine_sync waits). On MT_E_ARG (a record out of bounds) the chunks before the bad one have
 * been replayed and nothing stays staged. */
int32_t mt_engine_submit_run(mt_engine* e, const mt_op_rec* ops, const int64_t* op_off, const uint16_t* text,
                             int64_t text_units, const int64_t* text_off, const mt_props_rec* props, int64_t nprops,
                             const int64_t* props_off, const mt_kv* kv, int64_t nkv, const int64_t* kv_off);
/* Stage records for some documents only: docs[0..m) (increasing ids) and, for docs[k], the records
 * ops[op_off[k] .. op_off[k+1]) with pools at text+text_off[k], props+props_off[k], kv+kv_off[k]. The next
 * mt_engine_run replays those documents alone (one small launch); the others keep their state. What an interactive
 * host (the JS facade's reads) stages after a few edits; the reference applies each op as it arrives. */
int32_t mt_engine_submit_docs(mt_engine* e, int64_t m, const int64_t* docs, const mt_op_rec* ops, const int64_t* op_off,
                              const uint16_t* text, int64_t text_units, const int64_t* text_off,
                              const mt_props_rec* props, int64_t nprops, const int64_t* props_off, const mt_kv* kv,
                              int64_t nkv, const int64_t* kv_off);
/* The kind of each property value id (MT_VKIND_*, kinds[id & ~MT_VALUE_FALSY], n entries): what an "incr" combining
 * annotate makes of a key holding it (properties.ts:26-59: current + undefined). Without it an incr over a present
 * interned value latches MT_E_UNSUPPORTED. Takes effect at the next run. */
int32_t mt_engine_set_value_kinds(mt_engine* e, const uint8_t* kinds, int32_t n);
/* Pinned (page-locked) host memory for op logs a caller builds in place: the hand-off then copies by DMA alone. */
int32_t mt_host_alloc(int64_t bytes, void** out);
void mt_host_free(void* p);

/* Apply every staged event to its doc: Client.applyMsg for sequenced messages (client.ts:797),
 * insertSegmentLocal / removeRangeLocal / annotateRangeLocal for local edits (202/189/164).
 * Asynchronous on the engine's HIP stream; mt_engine_sync waits. */
int32_t mt_engine_run(mt_engine* e);
/* Wait for the replay. Capacity promotion (on unless MT_NO_PROMOTE=1): documents whose replay latched
 * MT_E_CAPACITY (nodes / row slots, heap, property key slots, text arena, membership log, pending
 * groups) replay again from their staged logs in an engine of the next profile (small -> 2,048 nodes and
 * 24 key slots -> 16,384 -> 262,144 tiled, 4x the arena, membership and pending-group capacities), as
 * often as needed; every per-document call below then answers for them from there. */
int32_t mt_engine_sync(mt_engine* e);
/* The documents the last mt_engine_sync promoted (writes up to cap ids); returns their count. */
int64_t mt_engine_promoted(const mt_engine* e, int64_t* docs_out, int64_t cap);
/* Device time of the last mt_engine_run's replay kernel (HIP events on the engine stream). */
float mt_engine_last_run_ms(const mt_engine* e);
/* The engine's hipStream_t (as void*), for callers that time or order work around it. */
void* mt_engine_stream(const mt_engine* e);

/* Return every doc to the state right after create/start_collab (same local ids), keeping the
 * staged batch, so a replay can be repeated (bench steps). Asynchronous. */
int32_t mt_engine_reset(mt_engine* e);
/* Per-doc work counters for roofline accounting: out3[3d..3d+2] = (sequenced messages applied,
 * sum over them of rows in the table before the message, rows written). */
int32_t mt_engine_work(mt_engine* e, int64_t* out3);
/* Per document, when the last replay's workgroup for it started and finished: out2[2d], out2[2d + 1] in ticks of
 * the GPU's constant 100 MHz clock (s_memrealtime; comparable across documents of one device): the per-document
 * time spread and the launch's tail. Promoted documents report their replay in the larger profile. */
int32_t mt_engine_doc_times(mt_engine* e, int64_t* out2);
/* Dispatch order of the replay kernel: workgroup b replays document order[b] (a permutation of [0, ndocs); NULL
 * restores document order). The GPU dispatches workgroups in index order as slots free up, so the documents in
 * decreasing order of expected cost make a longest-first list schedule. No effect on results. */
int32_t mt_engine_set_order(mt_engine* e, const int32_t* order);
/* Kernel build selection (no effect on results; no reference counterpart — the reference has one code path):
 *   MT_VAR_SMALL_WAVES (1 | 4 | 8): build of the config-2/3 replay kernel: 1 = the hot image in LDS (three documents
 *     per CU), 4 or 8 = HBM-resident at 4 or 8 waves per SIMD (default: 1 when the batch's documents fit three per
 *     CU, 4 when they fit 4 per SIMD, else 8; the MT_SMALL_WAVES environment variable sets it at create);
 *   MT_VAR_TILED_WIDE (0 | 1): the config-4 (tiled) kernel with the zamboni heap in HBM and the full window set
 *     (default 0: the narrow LDS-heap build, which promotes documents it cannot hold to the wide one).
 *   MT_VAR_CHUNK_DOCS (>= 0): documents per chunk of mt_engine_submit_run (0: automatic).
 *   MT_VAR_TEXTS_PACKED (0 | 1): how mt_engine_get_texts' fill kernel copies: 1 = the wave writes each pass of 64
 *     segments as one contiguous run, 0 = every lane copies its own segment's piece (the single-document read's
 *     copy); takes effect at the next mt_engine_get_texts.
 *   MT_VAR_DUMPS_PARALLEL (0 | 1): how mt_engine_dumps' fill kernel writes: 1 = every lane writes its own segment's
 *     record in 2- and 4-byte stores and the wave copies the texts together, 0 = one lane writes byte by byte (the
 *     single-document dump's writer); takes effect at the next mt_engine_dumps.
 *   MT_VAR_SUMMARIES_PARALLEL (0 | 1): how mt_engine_summaries' fill kernel writes: 1 = the wave decides a pass of 64
 *     rows at once, every run head and window row writes its own record and the wave copies the texts together,
 *     0 = one lane walks the rows and writes (the host core's writer); takes effect at the next mt_engine_summaries.
 *   MT_VAR_TILES_PARALLEL (0 | 1): how mt_engine_find_tiles and mt_engine_stack_contexts walk: 1 = the wave classifies a
 *     pass of 64 rows at once, 0 = the serial walk of the host core (a second device check, and the A/B baseline);
 *     takes effect at the next such call.
 *   MT_VAR_HANDLES_PARALLEL (0 | 1): how mt_engine_get_handles and mt_engine_handles_to_positions walk: 1 = the wave
 *     takes a pass of 64 rows at once (and writes a pass's handles together), 0 = the serial walk of the host core and
 *     the single call's leaf-per-pass search (a second device check, and the A/B baseline); takes effect at the next
 *     such call.
 *   MT_VAR_DELTAS_PARALLEL (0 | 1): how mt_engine_deltas_batch finds event ends and copies: 1 = the wave tests 64
 *     segment headers of an event at once and copies each run of kept events together, 0 = one lane walks segment by
 *     segment and copies word by word (a second device check, and the A/B baseline); takes effect at the next such
 *     call.
 * Takes effect at the next mt_engine_run / mt_engine_submit_run. */
enum { MT_VAR_SMALL_WAVES = 1, MT_VAR_TILED_WIDE = 2, MT_VAR_CHUNK_DOCS = 3, MT_VAR_TEXTS_PACKED = 4,
       MT_VAR_DUMPS_PARALLEL = 5, MT_VAR_SUMMARIES_PARALLEL = 6, MT_VAR_TILES_PARALLEL = 7,
       MT_VAR_HANDLES_PARALLEL = 8, MT_VAR_DELTAS_PARALLEL = 9 };
int32_t mt_engine_set_variant(mt_engine* e, int32_t key, int32_t value);

/* Per-doc latched error code (MT_E_*) and index of the event that raised it (-1 if none). */
int32_t mt_engine_errors(mt_engine* e, int32_t* err, int32_t* err_op);
/* The same for one document (an 8-byte read). */
int32_t mt_engine_doc_error(mt_engine* e, int64_t doc, int32_t* err, int32_t* err_op);
/* Per-doc FNV-1a-64 digest of the canonical segment dump (mt_oplog.h), computed on device. */
int32_t mt_engine_digests(mt_engine* e, uint64_t* out);
/* Canonical dump of one doc; returns bytes needed (writes if cap suffices), <0 on error. */
int64_t mt_engine_dump(mt_engine* e, int64_t doc, uint8_t* out, int64_t cap);
/* MergeTree.getLength(refSeq, clientId) (mergeTree.ts:1610); long_client < 0 = local view
 * (Client.getLength, client.ts:1051). */
int32_t mt_engine_get_length(mt_engine* e, int64_t doc, int32_t ref_seq, int32_t long_client, int32_t* out);
/* MergeTreeTextHelper.getText(refSeq, clientId) (textSegment.ts:154-172); long_client < 0 =
 * local view. Returns the length in UTF-16 units (writes at most cap), <0 on error. */
int64_t mt_engine_get_text(mt_engine* e, int64_t doc, int32_t ref_seq, int32_t long_client, uint16_t* out,
                           int64_t cap);
/* MergeTreeTextHelper.getText(refSeq, clientId, placeholder, start, end) (textSegment.ts:154-186): the text
 * of [start, end) under the perspective (getValidRange: MT_TEXT_DEFAULT start = 0, end = getLength), every
 * visited non-text segment (marker, permutation segment) adding `placeholder` cachedLength times
 * (gatherText 188-271; placeholder_len 0 = ""). JavaScript substring rules apply to a text segment's
 * piece (an end before the start swaps them). The placeholder "*" (Marker.toString()) returns
 * -MT_E_UNSUPPORTED. Returns the length in UTF-16 units (writes at most cap), <0 on error. */
#define MT_TEXT_DEFAULT INT32_MIN
int64_t mt_engine_get_text_range(mt_engine* e, int64_t doc, int32_t ref_seq, int32_t long_client,
                                 const uint16_t* placeholder, int32_t placeholder_len, int32_t start, int32_t end,
                                 uint16_t* out, int64_t cap);
/* SharedSequence.getItems(start, end) (sequence sharedSequence.ts:150-183; SharedObjectSequence /
 * SharedNumberSequence.getRange) of a SubSequence document (mt_oplog.h MT_SEG_RUN) in the local view: the item ids
 * (the host's item interner) of every visited SubSequence segment of [start, end), the ones before `start` in the
 * first of them spliced off and the result cut to end - start (end = MT_TEXT_DEFAULT: undefined, no cut; end <= start:
 * none). Returns the item count (writes at most cap), <0 on error. In such a document getText sees no TextSegment:
 * every visited segment gives the placeholder. */
int64_t mt_engine_get_items(mt_engine* e, int64_t doc, int32_t start, int32_t end, uint16_t* out, int64_t cap);
/* A segment handle (the reference returns live ISegment objects, mergeTree.ts:87-117): the row's
 * stable id and its generation. A handle stops resolving once zamboni merges the row into its
 * neighbour or unlinks it (mergeTree.ts:1322-1398), as a detached reference segment would. */
typedef struct mt_seg_ref {
    int32_t rid;    /* row id, -1: no segment at the position (the reference's `segment: undefined`) */
    int32_t gen;    /* row-id generation */
    int32_t offset; /* position - the segment's start */
    int32_t length; /* cachedLength */
    int32_t seq;    /* the segment's seq (-1: local, unacked) */
    int32_t client; /* long client index of its inserter, -1 = LocalClientId */
    int32_t removed_seq;    /* removedSeq: MT_NOT_REMOVED (the reference's undefined), -1 = a pending local remove */
    int32_t removed_client; /* long client index of the remover (0 when not removed), -1 = LocalClientId */
    int32_t ordinal;        /* the segment's index in walkAllSegments order (its canonical dump record) */
} mt_seg_ref;
#define MT_NOT_REMOVED INT32_MIN
/* MergeTree.getContainingSegment(pos, refSeq, clientId) (mergeTree.ts:1656-1667); long_client < 0 =
 * Client.getContainingSegment, the local view (client.ts:1006-1008). */
int32_t mt_engine_get_containing_segment(mt_engine* e, int64_t doc, int32_t pos, int32_t ref_seq, int32_t long_client,
                                         mt_seg_ref* out);
/* MergeTree.getPosition(segment, refSeq, clientId) (mergeTree.ts:1619-1636) of a handle;
 * MT_E_ARG if the handle no longer resolves. long_client < 0 = Client.getPosition (client.ts:291). */
int32_t mt_engine_get_position(mt_engine* e, int64_t doc, int32_t rid, int32_t gen, int32_t ref_seq,
                               int32_t long_client, int32_t* out);
/* MergeTree.posFromRelativePos(relativePos, refSeq, clientId) (mergeTree.ts:1976-1999; Client.posFromRelativePos
 * client.ts:308, SharedString.insertTextRelative / insertMarkerRelative): the position of the marker whose
 * property id_key (the interned "markerId" key) holds id_value, after it (+ cachedLength + offset) or before
 * it (- offset); *out = -1 if no marker holds the id; MT_E_UNSUPPORTED if several do. long_client < 0 = the
 * local view. */
int32_t mt_engine_pos_from_relative_pos(mt_engine* e, int64_t doc, int32_t id_key, int32_t id_value, int32_t before,
                                        int32_t has_offset, int32_t offset, int32_t ref_seq, int32_t long_client,
                                        int32_t* out);
/* MergeTree.resolveRemoteClientPosition(pos, refSeq, clientId) (mergeTree.ts:2140-2160; SharedSegmentSequence,
 * sequence.ts:314): the local position of what a remote client saw at `pos` under its (refSeq, client):
 * getPosition(segment) + offset in the local view, the local length when pos is that client's length, else
 * *out = -1 (undefined). A perspective persp_refused names (include note at mt_engine_get_length) returns
 * MT_E_UNSUPPORTED. */
int32_t mt_engine_resolve_remote_client_position(mt_engine* e, int64_t doc, int32_t pos, int32_t ref_seq,
                                                 int32_t long_client, int32_t* out);
/* PermutationVector.adjustPosition(pos, fromSeq, clientId) (permutationvector.ts:185-196; SharedMatrix.processCore,
 * matrix.ts:597-605): as resolveRemoteClientPosition for a segment that exists and is not removed, else -1. */
int32_t mt_engine_adjust_position(mt_engine* e, int64_t doc, int32_t pos, int32_t from_seq, int32_t long_client,
                                  int32_t* out);
/* ---- batched reads: m queries, one wave each, in one launch (two for the texts) and one stream wait --------
 * Query i names document docs[i] (docs == NULL: documents 0..m-1, and then m <= ndocs) under the perspective
 * (ref_seqs[i], long_clients[i]); both arrays NULL = the local view for every query, else both per query, with
 * long_clients[i] < 0 = the local view, as in the single-document calls. The queries only read: the flat
 * profiles' reads write nothing into the document block, so a document may appear several times, in any order
 * (the tiled profile's position index keeps its search scratch in the block: the engine runs the queries that
 * name one tiled document in successive launches, with the same results). status_out[i] is MT_OK or the code
 * the single call would have returned for the query (MT_E_UNSUPPORTED: a perspective persp_refused names, or a
 * placeholder run past PH_RUN_MAX); a failed query has length 0, a zero-length text, rid -1 or position -1, and
 * does not fail the call. status_out may be NULL only when long_clients is NULL. The return value is for
 * engine-level errors only (MT_E_ARG, MT_E_HIP, MT_E_NOMEM). m == 0 succeeds and touches nothing. Promoted
 * documents answer from their engines, each on its own stream; results land at the caller's query index. The
 * preconditions about a running replay and mt_engine_sync are those of the single-document reads. */
/* MergeTree.getLength(refSeq, clientId) (mergeTree.ts:1610; Client.getLength, client.ts:1051) per query. */
int32_t mt_engine_get_lengths(mt_engine* e, int64_t m, const int64_t* docs, const int32_t* ref_seqs,
                              const int32_t* long_clients, int32_t* len_out, int32_t* status_out);
/* MergeTreeTextHelper.getText(refSeq, clientId, placeholder, start, end) (textSegment.ts:154-186) per query:
 * starts / ends NULL = MT_TEXT_DEFAULT for every query; one placeholder per call, with the limits and the "*"
 * refusal of mt_engine_get_text_range. Returns the total in UTF-16 units (<0: -MT_E_*) and always fills
 * off_out[0..m]: query i's text is out[off_out[i] .. off_out[i+1]). `out` is written only when the total fits
 * cap: all or nothing, like mt_engine_dump; out == NULL is the size query. */
int64_t mt_engine_get_texts(mt_engine* e, int64_t m, const int64_t* docs, const int32_t* ref_seqs,
                            const int32_t* long_clients, const int32_t* starts, const int32_t* ends,
                            const uint16_t* placeholder, int32_t placeholder_len, int64_t* off_out,
                            int32_t* status_out, uint16_t* out, int64_t cap);
/* The canonical dump (mt_oplog.h) of every query's document: every segment in walkAllSegments order
 * (mergeTree.ts:3002-3016), what SnapshotV1.extractSync reads to write a summary (snapshotV1.ts:156-234). There is no
 * perspective and so no per-query status; docs[i] may be in any order and may repeat. Returns the total byte
 * count (<0: -MT_E_*; a document id out of range: -MT_E_ARG) and always fills off_out[0..m], in bytes: query i's
 * dump is out[off_out[i] .. off_out[i+1]), byte for byte what mt_engine_dump returns for that document; the
 * windows are contiguous and unpadded (so a window may start at 2 mod 4). `out` is written only when the total
 * fits cap: all or nothing, like mt_engine_get_texts; out == NULL is the size query. m == 0 returns 0 and
 * touches nothing. */
int64_t mt_engine_dumps(mt_engine* e, int64_t m, const int64_t* docs, int64_t* off_out, uint8_t* out, int64_t cap);
/* The summary dump (mt_oplog.h) of every query's document: the segments SnapshotV1.extractSync (snapshotV1.ts:156-234,
 * mode MT_SUMMARY_V1) or SnapshotLegacy.extractSync (snapshotlegacy.ts:179-242, mode MT_SUMMARY_LEGACY) yields,
 * filtered, coalesced (canAppend of the grown run + matchProperties) and concatenated on the device, in the canonical
 * dump's record layout: what a summary writer serializes, without the rows, overlap lists and local state it drops.
 * The call contract is mt_engine_dumps': any order, repeats, docs == NULL for documents 0..m-1, promoted documents
 * answer from their engines; returns the total byte count (<0: -MT_E_*; a document id out of range or an unknown
 * mode: -MT_E_ARG) and always fills off_out[0..m]; `out` is written only when the total fits cap (all or nothing);
 * out == NULL is the size query; m == 0 returns 0 and touches nothing. */
int64_t mt_engine_summaries(mt_engine* e, int64_t m, const int64_t* docs, int32_t mode, int64_t* off_out, uint8_t* out,
                            int64_t cap);
/* ---- batched marker queries: the local view only (Client.findTile and Client.getStackContext always ask as the
 * replica's own client under UniversalSequenceNumber), so there is no perspective and none is refused for one.
 * A label is a string inside an array-valued property (referenceTileLabels / referenceRangeLabels), which the host
 * interns as one value id; the device holds no strings. A call carries one label: label_key is the interned key, and
 * value_set a bitmap over the 2^15 host value ids (MT_LABEL_SET_WORDS words), bit v set when value v is an array that
 * holds the label (values the engine derives are never arrays and never match). docs == NULL: documents 0..m-1;
 * documents may repeat, in any order; pos[i] < 0 (or pos == NULL) is an undefined position. status_out[i] (required)
 * is MT_OK, or MT_E_UNSUPPORTED when an annotate changed label_key on a marker of the document: the reference's block
 * caches are then stale in a way that depends on its block-update history (as mt_engine_get_marker_from_id). Tiles and
 * range labels on local references (hierRefCount, mergeTree.ts:294-307) are not modelled. */
#define MT_LABEL_SET_WORDS 1024
#define MT_TILE_WORDS 5
typedef struct mt_tile_ref {
    int32_t rid;      /* row id of the marker, -1: none (or a refused query) */
    int32_t gen;      /* row-id generation (a handle, as mt_seg_ref) */
    int32_t ordinal;  /* the marker's index in walkAllSegments order (its canonical dump record) */
    int32_t pos;      /* its position in the local view (MergeTree.getPosition) */
    int32_t ref_type; /* its ReferenceType bits (ops.ts:6-15) */
} mt_tile_ref;
/* Client.findTile(startPos, tileLabel, preceding) (client.ts:1075-1078 -> MergeTree.findTile, mergeTree.ts:1796-1822)
 * per query: the nearest marker with the Tile refType and the label, at or before pos[i] (preceding[i] != 0; preceding
 * == NULL: every query) or at or after it; out[i].rid = -1 where the reference returns undefined. */
int32_t mt_engine_find_tiles(mt_engine* e, int64_t m, const int64_t* docs, const int32_t* pos, const int32_t* preceding,
                             int32_t label_key, const uint32_t* value_set, mt_tile_ref* out, int32_t* status_out);
/* Client.getStackContext(startPos, [rangeLabel]) (client.ts:948 -> MergeTree.getStackContext, mergeTree.ts:1783-1793)
 * per query: the stack of NestBegin / NestEnd markers with the label that are open at pos[i], bottom first. Works like
 * mt_engine_get_texts: off_out[0..m] is always filled, query i's window is out[off_out[i] .. off_out[i+1]) entries,
 * sized by the deepest the walk gets, and its first count_out[i] entries are the answer; returns the total entry count
 * (<0: -MT_E_*); `out` is written only when the total fits cap (all or nothing); out == NULL is the size query (one
 * launch); a call with `out` sizes and then fills (two launches); the label set is copied once per call. */
int64_t mt_engine_stack_contexts(mt_engine* e, int64_t m, const int64_t* docs, const int32_t* pos, int32_t label_key,
                                 const uint32_t* value_set, int64_t* off_out, int32_t* count_out, int32_t* status_out,
                                 mt_tile_ref* out, int64_t cap);
/* MergeTree.getContainingSegment(pos, refSeq, clientId) (mergeTree.ts:1656-1667) per query; out[i].rid = -1
 * where there is no segment at pos[i]. */
int32_t mt_engine_get_containing_segments(mt_engine* e, int64_t m, const int64_t* docs, const int32_t* pos,
                                          const int32_t* ref_seqs, const int32_t* long_clients, mt_seg_ref* out,
                                          int32_t* status_out);
/* MergeTree.resolveRemoteClientPosition(pos, refSeq, clientId) (mergeTree.ts:2140-2160) per query; out[i] = -1
 * for undefined. */
int32_t mt_engine_resolve_remote_client_positions(mt_engine* e, int64_t m, const int64_t* docs, const int32_t* pos,
                                                  const int32_t* ref_seqs, const int32_t* long_clients,
                                                  int32_t* out, int32_t* status_out);
/* PermutationVector.adjustPosition(pos, fromSeq, clientId) (permutationvector.ts:185-196) per query: what a
 * SharedMatrix host calls once per remote op (matrix.ts:597-605), for a batch of them; out[i] = -1 for undefined. */
int32_t mt_engine_adjust_positions(mt_engine* e, int64_t m, const int64_t* docs, const int32_t* pos,
                                   const int32_t* from_seqs, const int32_t* long_clients, int32_t* out,
                                   int32_t* status_out);
/* PermutationVector.handleToPosition(handle, localSeq) (permutationvector.ts:198-253; matrix.ts:532-533): the
 * segment whose allocated handles hold `handle` (walkAllSegments order), at findReconnectionPostition(segment,
 * localSeq) + offset (client.ts:675-705). MT_E_ARG if no segment holds it or local_seq is past the replica's
 * collabWindow.localSeq (the reference's asserts, permutationvector.ts:199, client.ts:676). */
int32_t mt_engine_handle_to_position(mt_engine* e, int64_t doc, int32_t handle, int32_t local_seq, int32_t* out);
/* Client.getMarkerFromId / MergeTree.getMarkerFromId (client.ts:312, mergeTree.ts:1965-1967): the marker whose
 * property id_key holds id_value (the engine's lookup, with mt_engine_pos_from_relative_pos's limits: several
 * markers, or an id an annotate changed, return MT_E_UNSUPPORTED); out->rid = -1 if none. */
int32_t mt_engine_get_marker_from_id(mt_engine* e, int64_t doc, int32_t id_key, int32_t id_value, mt_seg_ref* out);
/* Every segment's handle in walkAllSegments order (mergeTree.ts:3002-3016), i.e. aligned with the canonical
 * dump's records: out[2i] = rid, out[2i+1] = gen for at most cap segments; returns the segment count (<0 on
 * error). With the dump this is what Client.walkSegments / getPropertiesAtPosition / findTile read. */
int64_t mt_engine_segment_ids(mt_engine* e, int64_t doc, int32_t* out, int64_t cap);
/* Delta events (mt_oplog.h MT_DELTA_*; engines created with caps.dcap > 0): the stream a
 * SharedString "sequenceDelta" + "maintenance" listener would see (sequence.ts:136-150), batched.
 * mt_engine_delta_state: per doc the words emitted since create/reset (n_out, may exceed dcap) and
 * their FNV-1a-64 (hash_out). mt_engine_deltas: one doc's logged words, the first min(n, dcap); writes
 * at most cap of them and returns how many are logged (<0 on error). */
int32_t mt_engine_delta_state(mt_engine* e, int64_t* n_out, uint64_t* hash_out);
int64_t mt_engine_deltas(mt_engine* e, int64_t doc, int32_t* out, int64_t cap);
/* The delta streams of many documents in one call: what a host that forwards "sequenceDelta" (op >= 0 events:
 * INSERT, REMOVE, ANNOTATE, REGEN) and "maintenance" (op < 0: APPEND, SPLIT, UNLINK) to its listeners reads after
 * every replay (sequence.ts:136-150; MergeTreeMaintenanceType, mergeTreeDeltaCallback.ts:16-30), m queries, one wave
 * each. The call contract is that of mt_engine_handle_tables / mt_engine_get_texts: docs == NULL = documents 0..m-1;
 * documents may repeat, in any order; m == 0 returns 0 and touches nothing; an engine created without caps.dcap
 * returns -MT_E_ARG; the return value is the total word count (<0: -MT_E_* for engine-level errors only); off_out[0..m]
 * is always filled, query i's words are out[off_out[i] .. off_out[i+1]); `out` is written only when the total fits cap
 * (all or nothing); out == NULL is the size query. Promoted documents answer from their engines; as in
 * mt_engine_deltas the logged length is min(n, dcap) with the dcap of the engine the caller holds.
 *   from_words[i] (NULL: 0) is a cursor: a word index into the document's log that is an event boundary: word 0, the
 *     word after any event's nseg, or the logged end. Any other value (negative, past the logged end, inside an event)
 *     gives status_out[i] = MT_E_ARG and an empty window, and does not fail the call.
 *   kinds is a mask of MT_DELTA_KINDS_*; 0 or an unknown bit returns -MT_E_ARG. Both bits: the window is the words
 *     [from, logged end) verbatim, mt_engine_deltas' tail, a last event cut short by dcap included. One bit: the whole
 *     events of that kind from the cursor on, in order, each verbatim from its op word through its nseg word; a
 *     trailing event cut short by dcap is left out.
 *   end_out[i] (optional) is the next cursor: the logged end, or with one bit set the start of the cut-short trailing
 *     event if the walk met one.
 *   emitted_out[i] (optional) is the words emitted since create / reset (mt_engine_delta_state's n): emitted > dcap
 *     tells the caller the log saturated.
 *   status_out is required. */
#define MT_DELTA_KINDS_SEQUENCE 1    /* op >= 0: INSERT, REMOVE, ANNOTATE, REGEN */
#define MT_DELTA_KINDS_MAINTENANCE 2 /* op <  0: APPEND, SPLIT, UNLINK */
int64_t mt_engine_deltas_batch(mt_engine* e, int64_t m, const int64_t* docs, const int64_t* from_words, int32_t kinds,
                               int64_t* off_out, int64_t* end_out, int64_t* emitted_out, int32_t* status_out,
                               int32_t* out, int64_t cap);
/* Local references (MT_OP_REF records; engines created with caps.rcap > 0): per doc the number of
 * references (nref_out[d]) and, for reference i, LocalReference.toPosition() (localReference.ts:62-68:
 * Client.getPosition(segment) + getOffset(), -1 when detached) at pos_out[d * rcap + i]; the row length is
 * caps.rcap of the engine the caller created, for promoted documents too: a promoted document's row holds its
 * first rcap references, and nref_out[d] is its true count, which exceeds rcap when the document was promoted
 * because it ran out of reference slots (entries of a row past min(nref, rcap) are unspecified). References
 * follow their segment through splits and zamboni appends, and a remove slides SlideOnRemove ones to
 * the next (or last) segment and detaches the rest (mergeTree.ts:2703-2732, localReference.ts:
 * 251-342). -2: the reference's Client.addLocalReference threw for this reference (its offset holds
 * only slid references, so refsByOffset[offset].at is undefined, localReference.ts:195-201); the
 * reference keeps no such reference, and the engine leaves the tree untouched for it. */
int32_t mt_engine_ref_positions(mt_engine* e, int32_t* nref_out, int32_t* pos_out);
/* PermutationVector (engines created with caps.pcap > 0): the document's HandleTable.snapshot()
 * (handletable.ts:80-82: handles[0] = the free-list head, then 0 for an allocated handle or the next free one),
 * `len` entries; writes min(len, cap) and returns len (<0 on error). */
int64_t mt_engine_handle_table(mt_engine* e, int64_t doc, int32_t* out, int64_t cap);
/* PermutationVector.getMaybeHandle(pos) (permutationvector.ts:157-161, HandleCache.getHandle): the handle of
 * local position pos (segment start + offset; INT32_MIN = Handle.unallocated when the segment has none). */
int32_t mt_engine_get_handle(mt_engine* e, int64_t doc, int32_t pos, int32_t* out);
/* ---- batched matrix reads (engines created with caps.pcap > 0, else MT_E_ARG): the PermutationVector reads a
 * SharedMatrix host makes between replays, m queries in one call, one wave each, in the local view (no perspective).
 * The call contract is that of mt_engine_get_texts / mt_engine_find_tiles: docs == NULL = documents 0..m-1; documents
 * may repeat, in any order; m == 0 touches nothing; promoted documents answer from their engines; the queries that
 * name one tiled document go in successive launches; the return value is for engine-level errors only, and
 * status_out[i] (required) is MT_OK or the code the single call returns for the query (MT_E_ARG where the reference
 * asserts or throws), which does not fail the call. */
/* HandleCache.getHandles(start, end) (handlecache.ts:69-83, what fills the cache PermutationVector.getMaybeHandle reads,
 * permutationvector.ts:157-161; matrix.ts:168,179,278,280) per query: the handles of local positions [starts[i],
 * ends[i]), one segment walk per query instead of one getContainingSegment per position. Each handle is what
 * mt_engine_get_handle returns for its position: the segment's start + offset, and INT32_MIN for every position of a
 * segment without handles, whatever its offset (the reference computes Handle.unallocated + offset = -2^31 + offset
 * there, no valid handle either: isHandleValid is all that ever looks at it). A query is valid when 0 <= start <= end
 * <= getLength(); any other (the assert of getMaybeHandle, ensureRange's RangeError) has status MT_E_ARG and an empty
 * window. Returns the total handle count (<0: -MT_E_*) and always fills off_out[0..m]: query i's handles are
 * out[off_out[i] .. off_out[i+1]). `out` is written only when the total fits cap: all or nothing; out == NULL is the
 * size query. */
int64_t mt_engine_get_handles(mt_engine* e, int64_t m, const int64_t* docs, const int32_t* starts, const int32_t* ends,
                              int64_t* off_out, int32_t* status_out, int32_t* out, int64_t cap);
/* PermutationVector.handleToPosition(handle, localSeq) (permutationvector.ts:198-253; once per pending cell op on
 * reconnect, matrix.ts:532-533) per query, as mt_engine_handle_to_position: out[i] = the position, or -1 with status
 * MT_E_ARG where the reference asserts (permutationvector.ts:199, 245). local_seqs == NULL (or an entry
 * MT_LOCAL_SEQ_CURRENT) = the replica's collabWindow.localSeq, the reference's default argument. */
#define MT_LOCAL_SEQ_CURRENT INT32_MIN
int32_t mt_engine_handles_to_positions(mt_engine* e, int64_t m, const int64_t* docs, const int32_t* handles,
                                       const int32_t* local_seqs, int32_t* out, int32_t* status_out);
/* HandleTable.snapshot() (handletable.ts:80-82; permutationvector.ts:265, once per vector per summary) of every query's
 * document, as mt_engine_handle_table: off_out[0..m] in entries, query i's table is out[off_out[i] .. off_out[i+1]).
 * No perspective and no status; the sizing contract is mt_engine_dumps' (the total returned, all or nothing, out ==
 * NULL the size query). */
int64_t mt_engine_handle_tables(mt_engine* e, int64_t m, const int64_t* docs, int64_t* off_out, int32_t* out,
                                int64_t cap);
/* caps.rcap of the engine (the row length of mt_engine_ref_positions' pos_out) */
int32_t mt_engine_ref_capacity(const mt_engine* e);
/* Per-doc counters: nleaf, high-water row slots, high-water heap, events applied. */
int32_t mt_engine_stats(mt_engine* e, int32_t* out4_per_doc);
int64_t mt_engine_ndocs(const mt_engine* e);

#ifdef __cplusplus
}
#endif
#endif
