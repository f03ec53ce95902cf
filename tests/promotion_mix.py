"""Mixed batches whose large documents overflow the profile their engine starts in — test infrastructure for
tests/test_promotion_surface.py.

Capacity promotion (include/mt_engine.h mt_engine_sync): a document that latches MT_E_CAPACITY replays again in
an engine of the next profile (small or config-5 -> 2,048 nodes -> 16,384 nodes), with 4x the arena, membership
and pending-group capacities. `promoted_caps` restates that rule, so a test can create an engine directly at the
capacities a promoted document ends in and hand the same capacities to the host build of the engine core.

The large text documents' lengths are the smallest at which the host core (core_host.replay_batch) latches
MT_E_CAPACITY at the starting capacities (a binary search over the length; a longer log extends a shorter one, so
the latch is monotonic). The getAllocatedHandle records of a config-5 document are drawn anew for every length,
so there the length is one found by scanning lengths near the plain log's threshold (5,537 and 5,492 ops without
the records) for a latching length whose predecessor replays clean. In every case the B-tree nodes run out first
(the failing op needs node ncap + 1), before the row slots do. Measured with the host core:

    document                    ops     at the overflowed caps (err 5)       at the next caps (err 0)
    config4 id 0  small -> mid   1,730  192 nodes, 1,224 row slots high      193 nodes, 1,224 row slots
    config4 id 1  small -> mid   1,502  192 nodes, 1,224 row slots high      193 nodes, 1,232 row slots
    config4 id 2  small -> mid   1,314  192 nodes, 1,232 row slots high      (longer below)
    config4 id 2  mid -> big    16,839  2,048 nodes, 13,080 row slots high   2,050 nodes, 13,096 row slots
    config5 id 1  mat -> mid     5,529  640 nodes, 4,144 row slots high      640 nodes, 4,152 row slots
    config5 id 4  mat -> mid     5,416  640 nodes, 4,104 row slots high      641 nodes, 4,112 row slots

A generated log depends on its workload and document id only and a longer workload's log extends a shorter one's
(checked in the CPU tier), which the second-batch test uses for the records it stages on top."""
from __future__ import annotations

import numpy as np

from fluidframework_amd import gen
from fluidframework_amd import oplog as ol
from fluidframework_amd.engine import default_caps
import handles_inject
import refs_inject

KEYS = ("ncap", "hcap", "acap", "mcap", "gcap", "ccap")
NEXT_NCAP = {192: 2048, 640: 2048, 2048: 16384}  # HotSmall / HotMat -> HotMid -> HotBig (mt_replay.hip next_ncap)


def promoted_caps(c: dict) -> dict:
    n = NEXT_NCAP[c["ncap"]]
    return dict(ncap=n, hcap=max(c["hcap"], 2 * n), acap=min(4 * c["acap"], 1 << 23), mcap=min(4 * c["mcap"], 1 << 18),
                gcap=min(4 * c["gcap"], 1 << 16), ccap=c["ccap"])


def tup(c: dict) -> tuple:
    return tuple(c[k] for k in KEYS)


SMALL = default_caps(512)           # 192 nodes / 1,536 row slots
MID = promoted_caps(SMALL)          # 2,048 nodes
BIG = promoted_caps(MID)            # 16,384 nodes
MAT = default_caps(4096, config=5)  # 640 nodes (PermutationVector replicas)
MAT_MID = promoted_caps(MAT)

# text_mix: ten config-3 documents and three coalescing-defeated config-4 documents (document id, ops)
SMALL_OPS, NSMALL = 512, 10
MID_A, MID_B, CHAIN = (0, 1730), (1, 1502), (2, 16839)
CHAIN_SMALL_OPS = 1314  # where the chain document leaves the small profile
TEXT_AT = {1: MID_A, 4: CHAIN, 12: MID_B}  # batch index -> large document
TEXT_PROMOTED = {1, 4, 12}
TEXT_CHAIN = 4
TAIL_OPS = 300  # the second batch's records: MID_A and small document 0 generated this much longer

# perm_mix: six config-5 documents, two of them long (batch index -> (document id, ops))
PERM_OPS, NPERM = 1024, 6
PERM_AT = {1: (1, 5529), 4: (4, 5416)}
PERM_PROMOTED = {1, 4}
PCAP = 1 << 12  # as tests/test_ref_handles.py


def _one(w, did):
    return gen.generate(w, ids=[did], threads=1).doc_arrays(0)


def text_mix(extra=None) -> ol.Batch:
    """`extra` = (index, (ops, text, props, kv), local long id): one more document, inserted at that index."""
    small = gen.generate(gen.config3(SMALL_OPS), ids=np.arange(NSMALL), threads=4)
    docs = [small.doc_arrays(d) for d in range(NSMALL)]
    local = [int(x) for x in small.local_long_id]
    for at in sorted(TEXT_AT):
        did, n = TEXT_AT[at]
        docs.insert(at, _one(gen.config4(n), did))
        local.insert(at, 1)
    if extra is not None:
        docs.insert(extra[0], extra[1])
        local.insert(extra[0], extra[2])
    return ol.Batch.from_arrays(docs, np.asarray(local, np.int32))


def text_refs(b: ol.Batch) -> ol.Batch:
    """text_mix with 24 local references per document, about 40 % of them removed later"""
    return refs_inject.add_removals(refs_inject.inject(b, tup(BIG), nref=24))


def text_tails():
    """((batch index, whole log), ...) of one promoted and one unpromoted document of text_mix, each TAIL_OPS ops
    longer than in text_mix."""
    did, n = MID_A
    return ((0, _one(gen.config3(SMALL_OPS + TAIL_OPS), 0)), (1, _one(gen.config4(n + TAIL_OPS), did)))


def perm_mix(long_docs=None) -> ol.Batch:
    """`long_docs`: other lengths than PERM_AT's (the CPU tier checks that one op fewer fits)"""
    small = gen.generate(gen.config5(PERM_OPS), ids=np.arange(NPERM), threads=4)
    docs = [small.doc_arrays(d) for d in range(NPERM)]
    for at, (did, n) in (long_docs or PERM_AT).items():
        docs[at] = _one(gen.config5(n), did)
    b = ol.Batch.from_arrays(docs, small.local_long_id)
    return handles_inject.inject(b, tup(MAT_MID))


def incr_log() -> ol.DocLog:
    """A document with 14 distinct property keys (the small profile holds 8 key slots, the next 24) and, at its end,
    an "incr" annotate over a key that holds an interned string; over the generator's interner, so one value-kind
    table serves it and the generated documents of its batch."""
    it = gen.generator_interner()
    log = ol.DocLog(it, local_long_id=0)
    log.add(ol.OP_INSERT, client=1, seq=1, ref_seq=0, min_seq=0, pos1=0, text="0123456789" * 10,
            props={"s": "x", "i": 7})
    seq = 1
    for i in range(28):
        seq += 1
        log.add(ol.OP_ANNOTATE, client=1 + i % 3, seq=seq, ref_seq=seq - 1, min_seq=max(0, seq - 4),
                pos1=(5 * i) % 90, pos2=(5 * i) % 90 + 7, props={f"k{i % 12}": i})
    seq += 1
    log.add(ol.OP_ANNOTATE, client=2, seq=seq, ref_seq=seq - 1, min_seq=seq - 2, pos1=20, pos2=60,
            props={"s": 1}, combining=ol.COMBINE_INCR)
    return log
