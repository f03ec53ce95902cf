/*
 * mt_kernels.h — the CDNA4 (gfx950) kernels of the replay engine and their per-profile launchers.
 *
 * One 64-lane wavefront replays one document: control flow is wave-uniform, and the
 * data-parallel parts of every op — the perspective prefix scan that replaces the reference's
 * root-to-leaf walk (mergeTree.ts:2378-2507, nodeLength 1692-1732), range marking
 * (nodeMap 2936-2998), stable-id lookup and text copies — run across the 64 lanes with
 * DPP/permute shuffles and 64-bit ballots (mt_wave.h). Documents are independent, so the grid
 * is one workgroup per document and the machine is filled by documents.
 *
 * Each profile's kernels are instantiated in a translation unit of their own (prof_*.hip, and one
 * per k_replay occupancy variant), so the library builds in parallel; mt_replay.hip holds the C ABI
 * and dispatches through the engine's ProfOps table.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "../../include/mt_engine.h"
#include "mt_core.h"
#include "mt_store.h"
#include "mt_wave.h"

using namespace mt;

#define WG 64

template <class HT>
__global__ __launch_bounds__(WG) void k_init(Store<HT> st, int64_t ndocs) {
    int64_t d = blockIdx.x;
    if (d >= ndocs) return;
    Replica<WaveGPU, HT> r(st.doc(d), WaveGPU());
    r.init();
    r.commit();
}

template <class HT>
/* local[d] = doc d's local long id, local[ndocs + d] / local[2 ndocs + d] its minSeq / currentSeq */
__global__ __launch_bounds__(WG) void k_start_collab(Store<HT> st, int64_t ndocs, const int32_t* local) {
    int64_t d = blockIdx.x;
    if (d >= ndocs) return;
    Replica<WaveGPU, HT> r(st.doc(d), WaveGPU());
    r.start_collab(local[d], local[ndocs + d], local[2 * ndocs + d]);
    r.commit();
}

/* 16-byte vector copy of a hot image by the wave (HT is a multiple of 16 bytes) */
template <class HT>
__device__ inline void copy_image(HT* dst, const HT* src) {
    static_assert(sizeof(HT) % 16 == 0, "hot image must be 16-byte granular");
    const uint4* s = (const uint4*)src;
    uint4* d = (uint4*)dst;
    constexpr int n = sizeof(HT) / 16;
    for (int i = threadIdx.x; i < n; i += WG) d[i] = s[i];
}

/* The tree skeleton's per-node arrays and the zamboni heap of one document: staged into LDS by the
 * HBM-resident kernel (the rest of the hot image stays in HBM). */
template <class HT>
struct Skel {
    DocHdr zh; /* the image's header fields (the replica keeps the hot ones in registers) */
    int16_t lorder[HT::N], lpos[HT::N], nparent[HT::N];
    int8_t nchild[HT::N], nlevel[HT::N], nscour[HT::N];
    int32_t hseq[HT::H];
    int16_t hrid[HT::H];
    uint8_t hgen[HT::H];
    uint8_t l2s[HT::C];  /* long -> short client id */
    uint16_t s2l[HT::C]; /* short -> long */
};
/* The scan-critical subset of the skeleton (document order, child counts, parents): staged alone
 * where the whole Skel would cap residency through LDS (config-5 profile). */
template <class HT>
struct SkelLite {
    DocHdr zh; /* the image's header fields */
    int16_t lorder[HT::N], lpos[HT::N], nparent[HT::N];
    int8_t nchild[HT::N];
};
template <class T>
__device__ inline void wave_copy(T* dst, const T* src, int n) {
    for (int i = threadIdx.x; i < n; i += WG) dst[i] = src[i];
}
template <class HT>
__device__ inline void skel_move(Skel<HT>& k, HT& z, bool in) {
    constexpr int N = HT::N, H = HT::H;
    constexpr int C = HT::C, NH = (int)(sizeof(DocHdr) / 4);
    if (in) {
        wave_copy((int32_t*)&k.zh, (const int32_t*)&z.h, NH);
        wave_copy(k.lorder, z.lorder, N), wave_copy(k.lpos, z.lpos, N), wave_copy(k.nparent, z.nparent, N);
        wave_copy(k.nchild, z.nchild, N), wave_copy(k.nlevel, z.nlevel, N), wave_copy(k.nscour, z.nscour, N);
        wave_copy(k.hseq, z.hseq, H), wave_copy(k.hrid, z.hrid, H), wave_copy(k.hgen, z.hgen, H);
        wave_copy(k.l2s, z.l2s, C), wave_copy(k.s2l, z.s2l, C);
    } else {
        wave_copy((int32_t*)&z.h, (const int32_t*)&k.zh, NH);
        wave_copy(z.lorder, k.lorder, N), wave_copy(z.lpos, k.lpos, N), wave_copy(z.nparent, k.nparent, N);
        wave_copy(z.nchild, k.nchild, N), wave_copy(z.nlevel, k.nlevel, N), wave_copy(z.nscour, k.nscour, N);
        wave_copy(z.hseq, k.hseq, H), wave_copy(z.hrid, k.hrid, H), wave_copy(z.hgen, k.hgen, H);
        wave_copy(z.l2s, k.l2s, C), wave_copy(z.s2l, k.s2l, C);
    }
}

template <class HT>
__device__ inline void skel_lite_move(SkelLite<HT>& k, HT& z, bool in) {
    constexpr int N = HT::N, NH = (int)(sizeof(DocHdr) / 4);
    if (in) {
        wave_copy((int32_t*)&k.zh, (const int32_t*)&z.h, NH);
        wave_copy(k.lorder, z.lorder, N), wave_copy(k.lpos, z.lpos, N), wave_copy(k.nparent, z.nparent, N);
        wave_copy(k.nchild, z.nchild, N);
    } else {
        wave_copy((int32_t*)&z.h, (const int32_t*)&k.zh, NH);
        wave_copy(z.lorder, k.lorder, N), wave_copy(z.lpos, k.lpos, N), wave_copy(z.nparent, k.nparent, N);
        wave_copy(z.nchild, k.nchild, N);
    }
}

/* Per-launch extras of the replay kernels: the profiling build's per-document phase clocks, and the dispatch
 * order (workgroup b replays document order[b]; the hardware dispatches workgroups in index order as slots free
 * up, so a longest-first order is list scheduling by cost, mt_engine_set_order). */
struct ReplayAux {
    uint64_t* prof;
    const int32_t* order;
    int64_t doc0; /* a launch over documents [doc0, doc0 + grid): the chunked submit (mt_engine_submit_run) */
    int32_t compact; /* the staged pools are indexed by launch position, not by document (mt_engine_submit_docs:
                        `order` lists the documents with records) */
    const uint8_t* vkind; /* value kinds (mt_engine_set_value_kinds), nvk entries */
    int32_t nvk;
};
__device__ inline int64_t aux_doc(const ReplayAux& a) {
    const int64_t b = a.doc0 + (int64_t)blockIdx.x;
    return a.order ? a.order[b] : b;
}
/* the entry of the staged offset arrays that holds document d's pools */
__device__ inline int64_t aux_pool(const ReplayAux& a, int64_t d) {
    return a.compact ? a.doc0 + (int64_t)blockIdx.x : d;
}
/* the document's replay start / end on the constant-rate clock (s_memrealtime, 100 MHz), kept in its image header
 * (DocHdr.tStart / tEnd: no register stays live for it through the replay; mt_engine_doc_times) */
/* Stamped into the header copy the replay writes back (the LDS-staged DocHdr where one is staged): a direct HBM store
 * by lane 0 beside the other lanes' staging copies of the same header could be overwritten by the stale copy. */
__device__ inline void doc_stamp(DocHdr& h, int end) {
    if (threadIdx.x == 0) {
        int64_t now = (int64_t)__builtin_amdgcn_s_memrealtime();
        if (end)
            h.tEnd = now;
        else
            h.tStart = now;
    }
}

/* K1-K4 fused: the whole event stream of a document, one wave per document. LDS = true stages the
 * whole small-profile hot image in LDS; otherwise the image stays in HBM and only the skeleton and
 * the heap (Skel, 3.5 KB for the small profile) are staged. */
/* DL: the delta-event build (engines created with caps.dcap > 0) */
template <class HT, bool LDS, int MINW = 1, int SKM = 1, bool DL = false, bool LOAD = true> /* SKM: 1 Skel, 2 SkelLite, 0 none */
__global__ __launch_bounds__(WG, MINW) void k_replay(Store<HT> st, int64_t ndocs, const mt_op_rec* ops,
                                              const int64_t* op_off, const uint16_t* text, const int64_t* text_off,
                                              const mt_props_rec* props, const int64_t* props_off, const mt_kv* kv,
                                              const int64_t* kv_off, ReplayAux aux) {
    if ((int64_t)blockIdx.x >= ndocs) return;
    const int64_t d = aux_doc(aux);
    uint64_t* prof = aux.prof;
    (void)prof;
#ifdef MT_PROF
    __shared__ uint64_t sprof[PH_N]; /* the replica's phase clocks (LDS, not registers) */
    for (int i = threadIdx.x; i < PH_N; i += WG) sprof[i] = 0;
    __syncthreads();
#define MT_PROF_ATTACH(r) (r).prof = sprof
#else
#define MT_PROF_ATTACH(r) (void)0
#endif
    Pools p;
    const int64_t pi = aux_pool(aux, d);
    p.ops = ops + op_off[pi];
    p.nops = op_off[pi + 1] - op_off[pi];
    p.text = text + text_off[pi];
    p.props = props + props_off[pi];
    p.kv = kv + kv_off[pi];
    p.vkind = aux.vkind;
    p.nvk = aux.nvk;
    Doc<HT> v = st.doc(d);
    if constexpr (LDS) {
        __shared__ __attribute__((aligned(16))) HT hot;
        HT* g = v.t;
        copy_image(&hot, g);
        __syncthreads();
        doc_stamp(hot.h, 0);
        v.t = &hot;
        Replica<WaveGPU, HT, DL, LOAD> r(v, WaveGPU());
        MT_PROF_ATTACH(r);
        r.replay(p);
        r.commit();
#ifdef MT_PROF
        if (prof && threadIdx.x == 0)
            for (int i = 0; i < PH_N; i++) prof[d * PH_N + i] = r.prof[i];
#endif
        doc_stamp(hot.h, 1);
        __syncthreads();
        copy_image(g, &hot);
    } else if constexpr (SKM == 2) {
        __shared__ __attribute__((aligned(16))) SkelLite<HT> sk;
        skel_lite_move(sk, *v.t, true);
        __syncthreads();
        doc_stamp(sk.zh, 0);
        Replica<WaveGPU, HT, DL, LOAD> r(v, WaveGPU());
        MT_PROF_ATTACH(r);
        r.lo = sk.lorder, r.lp = sk.lpos, r.npar = sk.nparent, r.nch = sk.nchild;
        r.zh = &sk.zh;
        r.replay(p);
        r.commit();
        doc_stamp(sk.zh, 1);
        __syncthreads();
        skel_lite_move(sk, *v.t, false);
#ifdef MT_PROF
        if (prof && threadIdx.x == 0)
            for (int i = 0; i < PH_N; i++) prof[d * PH_N + i] = r.prof[i];
#endif
    } else if constexpr (SKM == 1 && sizeof(Skel<HT>) <= 12288) {
        static_assert(sizeof(DocHdr) % 4 == 0, "the header is copied in dwords");
        __shared__ __attribute__((aligned(16))) Skel<HT> sk;
        skel_move(sk, *v.t, true);
        __syncthreads();
        doc_stamp(sk.zh, 0);
        Replica<WaveGPU, HT, DL, LOAD> r(v, WaveGPU());
        MT_PROF_ATTACH(r);
        r.lo = sk.lorder, r.lp = sk.lpos, r.npar = sk.nparent, r.nch = sk.nchild, r.nlev = sk.nlevel;
        r.nsc = sk.nscour, r.hsq = sk.hseq, r.hrd = sk.hrid, r.hgn = sk.hgen;
        r.zh = &sk.zh, r.l2s = sk.l2s, r.s2l = sk.s2l;
        r.replay(p);
        r.commit();
        doc_stamp(sk.zh, 1);
        __syncthreads();
        skel_move(sk, *v.t, false);
#ifdef MT_PROF
        if (prof && threadIdx.x == 0)
            for (int i = 0; i < PH_N; i++) prof[d * PH_N + i] = r.prof[i];
#endif
    } else {
        doc_stamp(v.t->h, 0);
        Replica<WaveGPU, HT, DL, LOAD> r(v, WaveGPU());
        MT_PROF_ATTACH(r);
        r.replay(p);
        r.commit();
        doc_stamp(v.t->h, 1);
#ifdef MT_PROF
        if (prof && threadIdx.x == 0)
            for (int i = 0; i < PH_N; i++) prof[d * PH_N + i] = r.prof[i];
#endif
    }
}

/* Config 4 (large documents, the tiled profile): one workgroup per document, which has the CU's LDS to
 * itself (155 KB): the position-search scratch (per-chunk window deltas, all zero between searches, and each
 * window row's chunk position / leaf index / perspective length) and, for the duration of the replay, the
 * rope's chunk arrays and the window set (with each row's last-seen slot). The rows, the leaf summaries,
 * the per-leaf rope links and the zamboni heap stay in HBM (~0.2 GB per 1M-op document). An LDS copy of the
 * heap (~60 entries in use at lag 64) measured slower: a heap that can be in either memory is reached through
 * flat accesses, which wait for both counters (r04j A/B: 10.75 -> 10.33M ops/s at 256 x 300k). */
/* NARROW (the default config-4 kernel): the zamboni heap in LDS too (~60 entries in use at lag 64: every pop and
 * push an LDS pass instead of an HBM round trip), beside a window set of Replica::NARROW_W entries; a document whose
 * heap or window set would outgrow them latches E_CAPACITY and the engine replays it in the wide variant
 * (NARROW = false: the heap in HBM, the full window set) — capacity promotion (mt_replay.hip). */
template <class HT, bool DL = false, bool NARROW = false>
__global__ __launch_bounds__(WG * 2) void k_replay_tiled(Store<HT> st, int64_t ndocs, const mt_op_rec* ops,
                                                     const int64_t* op_off, const uint16_t* text,
                                                     const int64_t* text_off, const mt_props_rec* props,
                                                     const int64_t* props_off, const mt_kv* kv, const int64_t* kv_off,
                                                     ReplayAux aux) {
    static_assert(HT::TILED, "tiled profile only");
    typedef Replica<WaveGPU, HT, DL, true, NARROW> R;
    constexpr int NCH = HT::TL::NCH, WCAP = R::WCAPR, HL = NARROW ? R::HCAPR : 1;
    __shared__ int32_t cdel[NCH];
    __shared__ int32_t wcp[WCAP], wvs[WCAP];
    __shared__ uint8_t wlx[WCAP];
    __shared__ DocHdr zhs; /* the image's header fields, staged for the replay */
    /* the rope's chunk arrays and the window set, staged for the replay (written back at the end) */
    constexpr int NG = HT::TL::NG;
    __shared__ int32_t lcord[NCH], lcst[NCH], lcpos[NCH], lccnt[NCH], lwrid[WCAP];
    __shared__ int32_t lgst[NG], lgdel[NG]; /* chunk-group sums of lcst and of cdel */
    __shared__ uint16_t lkeys[HT::K];       /* the property key table */
    __shared__ __attribute__((aligned(16))) uint8_t lwgen[WCAP];
    __shared__ int32_t lwslot[WCAP];
    __shared__ int32_t lhseq[HL]; /* NARROW: the zamboni heap */
    __shared__ typename HT::IX lhrid[HL];
    __shared__ uint8_t lhgen[HL];
    __shared__ typename R::WinMail wmail; /* the window helper's mailbox */
#ifdef MT_PROF
    __shared__ uint64_t sprof[PH_N];
    for (int i = threadIdx.x; i < PH_N; i += blockDim.x) sprof[i] = 0;
#endif
    if ((int64_t)blockIdx.x >= ndocs) return;
    const int64_t d = aux_doc(aux);
    uint64_t* prof = aux.prof;
    (void)prof;
    Doc<HT> v = st.doc(d);
    auto& tl = v.t->tl;
    const bool replayer = threadIdx.x < WG;
    /* what the staged arrays cannot hold: nothing is staged, the replica latches E_CAPACITY */
    const bool fits = !NARROW || (tl.wN <= WCAP && v.t->h.heapN <= HL);
    const int32_t nheap = NARROW ? v.t->h.heapN : 0;
    if (replayer && fits) {
        for (int i = threadIdx.x; i < NCH; i += WG) cdel[i] = 0;
        for (int i = threadIdx.x; i < NG; i += WG) lgdel[i] = 0;
        wave_copy(lgst, tl.gst, NG);
        wave_copy(lkeys, v.t->keys, HT::K);
        wave_copy((int32_t*)&zhs, (const int32_t*)&v.t->h, (int)(sizeof(DocHdr) / 4));
        wave_copy(lcord, tl.cord, NCH);
        wave_copy(lcst, tl.cst, NCH);
        wave_copy(lcpos, tl.cpos, NCH);
        wave_copy(lccnt, tl.ccnt, NCH);
        wave_copy(lwrid, tl.wrid, WCAP);
        wave_copy((int32_t*)lwgen, (const int32_t*)tl.wgen, WCAP / 4);
        wave_copy(lwslot, tl.wslot, WCAP);
        if constexpr (NARROW) {
            wave_copy(lhseq, v.t->hseq, nheap);
            wave_copy(lhrid, v.t->hrid, nheap);
            wave_copy(lhgen, v.t->hgen, nheap);
        }
    }
    if (threadIdx.x == 0) wmail.quit = 0; /* every path: the helper reads it after its first barrier */
    __syncthreads();
    if (replayer && fits) doc_stamp(zhs, 0);
    Pools p;
    const int64_t pi = aux_pool(aux, d);
    p.ops = ops + op_off[pi];
    p.nops = op_off[pi + 1] - op_off[pi];
    p.text = text + text_off[pi];
    p.props = props + props_off[pi];
    p.kv = kv + kv_off[pi];
    p.vkind = aux.vkind;
    p.nvk = aux.nvk;
    if (!replayer) {
        if (threadIdx.x < 2 * WG) { /* the window helper: the replaying wave's LDS views of the set and the rope */
            R hr(v, WaveGPU());
            hr.tcpos = lcpos;
            hr.twrid = lwrid;
            hr.twgen = lwgen;
            hr.twslot = lwslot;
            hr.wm = &wmail;
            hr.win_helper();
        }
    } else if (!fits) {
        doc_stamp(v.t->h, 0);
        R r(v, WaveGPU());
        r.fail(E_CAPACITY);
        r.commit();
        doc_stamp(v.t->h, 1);
    } else {
        R r(v, WaveGPU());
        MT_PROF_ATTACH(r);
        r.cdel = cdel;
        r.wcp = wcp;
        r.wvs = wvs;
        r.wlx = wlx;
        r.zh = &zhs;
        r.tcord = lcord;
        r.tcst = lcst;
        r.tgst = lgst;
        r.gdel = lgdel;
        r.keys = lkeys;
        r.tcpos = lcpos;
        r.tccnt = lccnt;
        r.twrid = lwrid;
        r.twgen = lwgen;
        r.twslot = lwslot;
        if constexpr (NARROW) {
            r.hsq = lhseq;
            r.hrd = lhrid;
            r.hgn = lhgen;
        }
        r.wm = &wmail;
        r.replay(p);
        r.commit();
        doc_stamp(zhs, 1);
#ifdef MT_PROF
        if (prof && threadIdx.x == 0)
            for (int i = 0; i < PH_N; i++) prof[d * PH_N + i] = r.prof[i];
#endif
    }
    /* Barriers, reached by both waves in the same order: the one above (the staging done, quit cleared); per window
     * pass of more than 64 entries, win_pass's two, which pair with the two of win_helper's loop; then this one, on
     * every path of the replaying wave (the !fits one too), which pairs with the first barrier of the helper's loop,
     * where the helper reads quit and returns; and the last one, which both reach before the write-back. */
    if (replayer) {
        if (threadIdx.x == 0) wmail.quit = 1;
        __syncthreads();
    }
    __syncthreads();
    if (replayer && fits) {
        wave_copy((int32_t*)&v.t->h, (const int32_t*)&zhs, (int)(sizeof(DocHdr) / 4));
        wave_copy(tl.cord, lcord, NCH);
        wave_copy(tl.cst, lcst, NCH);
        wave_copy(tl.gst, lgst, NG);
        wave_copy(v.t->keys, lkeys, HT::K);
        wave_copy(tl.cpos, lcpos, NCH);
        wave_copy(tl.ccnt, lccnt, NCH);
        wave_copy(tl.wrid, lwrid, WCAP);
        wave_copy((int32_t*)tl.wgen, (const int32_t*)lwgen, WCAP / 4);
        wave_copy(tl.wslot, lwslot, WCAP);
        if constexpr (NARROW) {
            int32_t n = zhs.heapN <= HL ? zhs.heapN : HL;
            wave_copy(v.t->hseq, lhseq, n);
            wave_copy(v.t->hrid, lhrid, n);
            wave_copy(v.t->hgen, lhgen, n);
        }
    }
}

/* K5: per-doc digest of the canonical dump */
template <class HT>
__global__ __launch_bounds__(WG) void k_digest(Store<HT> st, int64_t ndocs, uint64_t* out) {
    int64_t d = blockIdx.x;
    if (d >= ndocs) return;
    /* The compiler reads the document here with scalar (SMEM) loads, including the
     * base + SGPR-offset + immediate form no other kernel uses. Round 1 put a compiler barrier here
     * after a digest mismatch; tools/smem_probe.hip shows that form (compiler- and asm-emitted)
     * returns what vector loads return, the round-1 failing case is clean without the barrier, and
     * tests/test_gpu_parity.py checks this digest against FNV-1a of k_dump for every document. */
    Replica<WaveGPU, HT> r(st.doc(d), WaveGPU());
    uint64_t h = r.digest();
    if (threadIdx.x == 0) out[d] = h;
}

template <class HT>
__global__ __launch_bounds__(WG) void k_dump(Store<HT> st, int64_t doc, uint8_t* out, int64_t cap, int64_t* n) {
    Replica<WaveGPU, HT> r(st.doc(doc), WaveGPU());
    int64_t m = r.dump(out, cap);
    if (threadIdx.x == 0) *n = m;
}

/* A read under a remote perspective (refSeq, client) is answered only where the reference's block
 * PartialSequenceLengths and the leaf visibility predicate the engine sums agree: refSeq >= minSeq (the
 * partials fold everything at or below the window into minLength, partialLengths.ts:489-518) and refSeq at
 * or past every refSeq that client has sent an op under (`floor`, tracked by the host from the records:
 * later entries of that client are added whole, getBranchPartialLength 456-486, which counts a removal of
 * a segment inserted after refSeq that the predicate does not — the "invalid combination" of
 * partialLengths.ts:672-681). The local client (cachedLength) and a non-collaborating replica are always
 * answered. Measured against the reference on 7,600 perspectives: every one this rule answers is equal
 * (tests/test_ref_persp.py). */
template <class R>
__device__ inline bool persp_refused(const R& r, int32_t ref_seq, int32_t long_client, int32_t floor) {
    if (long_client < 0 || !r.h.collaborating || long_client == r.h.localLong) return false;
    return ref_seq < r.h.minSeq || ref_seq < floor;
}

template <class HT>
__global__ __launch_bounds__(WG) void k_length(Store<HT> st, int64_t doc, int32_t ref_seq, int32_t long_client,
                                              int32_t floor, int32_t* out) {
    Replica<WaveGPU, HT> r(st.doc(doc), WaveGPU());
    int32_t v;
    if (persp_refused(r, ref_seq, long_client, floor)) {
        if (threadIdx.x == 0) out[0] = 0, out[1] = 1;
        return;
    }
    if (long_client < 0) {
        v = r.length_local();
    } else {
        int32_t sh = r.short_of(long_client);
        v = r.length(ref_seq, sh < 0 ? 0x7fff : sh);
    }
    if (threadIdx.x == 0) out[0] = v, out[1] = 0;
}

template <class HT>
__global__ __launch_bounds__(WG) void k_text(Store<HT> st, int64_t doc, int32_t ref_seq, int32_t long_client,
                                            int32_t floor, int32_t start, int32_t end, const uint16_t* ph,
                                            int32_t pl, uint16_t* out, int64_t cap, int64_t* n) {
    Replica<WaveGPU, HT> r(st.doc(doc), WaveGPU());
    if (persp_refused(r, ref_seq, long_client, floor)) {
        if (threadIdx.x == 0) *n = -E_UNSUPPORTED;
        return;
    }
    int32_t sh;
    if (long_client < 0) {
        sh = r.h.localShort;
        ref_seq = r.h.currentSeq;
    } else {
        sh = r.short_of(long_client);
        if (sh < 0) sh = 0x7fff;
    }
    /* pl < 0: SharedSequence.getItems(start, end) in the local view (the C ABI's mt_engine_get_items) */
    int64_t m = pl < 0 ? r.get_items(start, end, out, cap) : r.get_text_range(ref_seq, sh, start, end, ph, pl, out, cap);
    if (threadIdx.x == 0) *n = m;
}

/* Per-document segment queries (one workgroup); out[0] = status (1 found / 0 none / 2 several markers /
 * 3 refused perspective), then by mode:
 *   0 getContainingSegment(a = pos): mt_seg_ref fields {rid, gen, offset, length, seq, client, removedSeq,
 *     removedClient, ordinal} in out[1..9]
 *   1 getPosition(a = rid, b = gen): out[1]
 *   2 posFromRelativePos' marker (a = marker-id key, b = value): its position, out[1]
 *   3 HandleCache.getHandle(a = pos): out[1]
 *   4 a remote client's position a under (ref_seq, long_client) in the local view (resolveRemoteClientPosition,
 *     mergeTree.ts:2140-2160; PermutationVector.adjustPosition, permutationvector.ts:185-196): found: out[1] =
 *     getPosition(segment) + offset, out[2] = the segment's removal flag; none: out[3] = getLength under the
 *     remote perspective, out[4] = the local length
 *   5 getMarkerFromId (a = key, b = value): mt_seg_ref fields of the marker, as mode 0
 *   6 PermutationVector.handleToPosition (a = handle, b = localSeq; permutationvector.ts:198-253): the segment
 *     whose allocated handles hold a, findReconnectionPostition(segment, localSeq) + its offset, out[1] */
template <class R>
__device__ inline void seg_fields(R& r, int32_t s, int32_t off, int32_t* res) {
    int32_t rid = r.z.rid[s], rs = r.z.rseq(s);
    res[0] = 1;
    res[1] = rid;
    res[2] = r.z.rgen[rid];
    res[3] = off;
    res[4] = r.z.len(s);
    res[5] = r.z.seq(s);
    res[6] = r.long_of_cli(s);
    res[7] = rs;
    res[8] = rs == NOREM ? 0 : r.long_of_rcli(s);
    res[9] = r.ordinal_of(s);
}
#define MT_SEGQ_N 10
/* one query of the list above on a replica: res[0..MT_SEGQ_N) (k_seg: one document; k_segs: one per wave) */
template <class HT>
__device__ inline void seg_eval(Replica<WaveGPU, HT>& r, int32_t mode, int32_t a, int32_t b, int32_t ref_seq,
                                int32_t long_client, int32_t floor, int32_t* res) {
    res[0] = 0, res[1] = -1;
    for (int i = 2; i < MT_SEGQ_N; i++) res[i] = 0;
    if (persp_refused(r, ref_seq, long_client, floor)) { /* res[0] = 3: refused (MT_E_UNSUPPORTED) */
        res[0] = 3;
        return;
    }
    int32_t sh;
    if (long_client < 0) {
        sh = r.h.localShort;
        ref_seq = r.h.currentSeq;
    } else {
        sh = r.short_of(long_client);
        if (sh < 0) sh = 0x7fff; /* a client the replica has not seen: sequenced content only */
    }
    if (mode == 0) {
        int32_t off = 0;
        int32_t s = r.containing(a, ref_seq, sh, &off);
        if (s >= 0) seg_fields(r, s, off, res);
    } else if (mode == 1) {
        int32_t s = (a >= 0 && a < HT::S) ? r.slot_of(a, b) : -1;
        if (s >= 0) {
            res[0] = 1;
            res[1] = r.position_of(s, ref_seq, sh);
        }
    } else if (mode == 3) { /* HandleCache.getHandle(a): the PermutationSegment's start + offset, or unallocated */
        int32_t off = 0;
        int32_t s = r.containing(a, ref_seq, sh, &off);
        if (s >= 0) {
            uint32_t st = (r.z.flags(s) & RF_PERM) ? r.cold(s).toff : 0u;
            res[0] = 1;
            res[1] = st ? (int32_t)st + off : INT32_MIN;
        }
    } else if (mode == 4) {
        int32_t off = 0;
        int32_t s = r.containing(a, ref_seq, sh, &off);
        if (s >= 0) {
            res[0] = 1;
            res[1] = r.local_pos(s) + off;
            res[2] = r.z.rseq(s) != NOREM;
        } else {
            res[3] = r.length(ref_seq, sh);
            res[4] = r.length_local();
        }
    } else if (mode == 6) {
        int32_t s = -1, off = 0;
        /* assert(localSeq <= collabWindow.localSeq) (permutationvector.ts:199 -> client.ts:676): res[0] stays 0 */
        const bool inRange = b <= r.zh->localSeq;
        for (int32_t k = 0; inRange && s < 0 && r.kvalid(k); k = r.knext(k)) { /* walkAllSegments: the first match */
            int32_t n = r.leaf_at(k), c = r.nch[n];
            int32_t j = threadIdx.x;
            bool hit = false;
            int32_t q = n * MAXN + (j & (MAXN - 1));
            if (j < c && j < MAXN && (r.z.flags(q) & RF_PERM)) {
                int32_t h0 = (int32_t)r.cold(q).toff;
                hit = h0 != 0 && h0 <= a && a < h0 + r.z.len(q);
            }
            uint64_t m = r.w.ballot(hit);
            if (m) {
                s = n * MAXN + r.w.ffs(m);
                off = a - (int32_t)r.cold(s).toff;
            }
        }
        if (s >= 0) {
            res[0] = 1;
            res[1] = r.recon_pos(s, b) + off;
        }
    } else { /* modes 2 and 5: the marker whose property a (the marker-id key) is value b; res[0] = 2 if several */
        int32_t s = r.marker_by_id(a, b);
        if (s == -2) {
            res[0] = 2;
        } else if (s >= 0 && mode == 5) {
            seg_fields(r, s, 0, res);
        } else if (s >= 0) {
            res[0] = 1;
            res[1] = r.position_of(s, ref_seq, sh);
        }
    }
}
template <class HT>
__global__ __launch_bounds__(WG) void k_seg(Store<HT> st, int64_t doc, int32_t mode, int32_t a, int32_t b,
                                           int32_t ref_seq, int32_t long_client, int32_t floor, int32_t* out) {
    Replica<WaveGPU, HT> r(st.doc(doc), WaveGPU());
    int32_t res[MT_SEGQ_N];
    seg_eval<HT>(r, mode, a, b, ref_seq, long_client, floor, res);
    if (threadIdx.x == 0)
        for (int i = 0; i < MT_SEGQ_N; i++) out[i] = res[i];
}

/* ---- batched reads: one wave per query (mt_engine_get_lengths / _texts / _containing_segments / ..._positions) ----
 * A query names a document of this store, a perspective (ref_seq, long_client < 0 = the local view) with its floor
 * (persp_refused, filled by the host on the engine the caller holds, before routing), two arguments (a position,
 * or a text range) and `slot`, the caller's query index: every result lands there, so the queries of one call
 * can be split over the engines that hold their documents. The reads write nothing into a flat profile's
 * document block, so a document may be named by several queries of a launch; the tiled profile's position index
 * keeps scratch in the block (Replica: sdel, swcp, ...), so the host launches its queries of one document one
 * after the other (mt_replay.hip read_plan). */
struct ReadQ {
    int64_t doc;
    int32_t ref_seq, long_client, floor;
    int32_t a, b;
    int32_t slot;
};
/* the perspective set-up of k_text / k_seg */
template <class R>
__device__ inline int32_t persp_short(R& r, int32_t* ref_seq, int32_t long_client) {
    if (long_client < 0) {
        *ref_seq = r.h.currentSeq;
        return r.h.localShort;
    }
    int32_t sh = r.short_of(long_client);
    return sh < 0 ? 0x7fff : sh;
}
template <class HT>
__global__ __launch_bounds__(WG) void k_lengths(Store<HT> st, int64_t m, const ReadQ* qs, int32_t* len,
                                               int32_t* status) {
    if ((int64_t)blockIdx.x >= m) return;
    const ReadQ q = qs[blockIdx.x];
    Replica<WaveGPU, HT> r(st.doc(q.doc), WaveGPU());
    int32_t v = 0, rc = MT_OK;
    if (persp_refused(r, q.ref_seq, q.long_client, q.floor)) {
        rc = MT_E_UNSUPPORTED;
    } else if (q.long_client < 0) {
        v = r.length_local();
    } else {
        int32_t sh = r.short_of(q.long_client);
        v = r.length(q.ref_seq, sh < 0 ? 0x7fff : sh);
    }
    if (threadIdx.x == 0) len[q.slot] = v, status[q.slot] = rc;
}
/* the size of query i's text (size[slot]; 0 and status[slot] = MT_E_UNSUPPORTED for a refused one) */
template <class HT>
__global__ __launch_bounds__(WG) void k_text_sizes(Store<HT> st, int64_t m, const ReadQ* qs, int32_t pl,
                                                  int64_t* size, int32_t* status) {
    if ((int64_t)blockIdx.x >= m) return;
    const ReadQ q = qs[blockIdx.x];
    Replica<WaveGPU, HT> r(st.doc(q.doc), WaveGPU());
    int64_t n = -E_UNSUPPORTED;
    if (!persp_refused(r, q.ref_seq, q.long_client, q.floor)) {
        int32_t ref_seq = q.ref_seq;
        int32_t sh = persp_short(r, &ref_seq, q.long_client);
        n = r.get_text_range(ref_seq, sh, q.a, q.b, nullptr, pl, nullptr, 0);
    }
    if (threadIdx.x == 0) size[q.slot] = n < 0 ? 0 : n, status[q.slot] = n < 0 ? (int32_t)-n : MT_OK;
}
/* query i's text into out[off[slot], off[slot + 1]) (the host's prefix sum of k_text_sizes' sizes: a failed
 * query's window is empty); nothing is written outside the window */
template <class HT, bool PACKED>
__global__ __launch_bounds__(WG) void k_texts(Store<HT> st, int64_t m, const ReadQ* qs, const uint16_t* ph,
                                             int32_t pl, const int64_t* off, uint16_t* out) {
    if ((int64_t)blockIdx.x >= m) return;
    const ReadQ q = qs[blockIdx.x];
    const int64_t o = off[q.slot], cap = off[q.slot + 1] - o;
    if (cap <= 0) return;
    Replica<WaveGPU, HT> r(st.doc(q.doc), WaveGPU());
    if (persp_refused(r, q.ref_seq, q.long_client, q.floor)) return;
    int32_t ref_seq = q.ref_seq;
    int32_t sh = persp_short(r, &ref_seq, q.long_client);
    (void)r.template get_text_range<PACKED>(ref_seq, sh, q.a, q.b, ph, pl, out + o, cap);
}
/* k_seg's modes 0 and 4 per query (a = the position): res[slot * MT_SEGQ_N ..] */
template <class HT>
__global__ __launch_bounds__(WG) void k_segs(Store<HT> st, int64_t m, const ReadQ* qs, int32_t mode, int32_t* out) {
    if ((int64_t)blockIdx.x >= m) return;
    const ReadQ q = qs[blockIdx.x];
    Replica<WaveGPU, HT> r(st.doc(q.doc), WaveGPU());
    int32_t res[MT_SEGQ_N];
    seg_eval<HT>(r, mode, q.a, 0, q.ref_seq, q.long_client, q.floor, res);
    if (threadIdx.x == 0)
        for (int i = 0; i < MT_SEGQ_N; i++) out[(int64_t)q.slot * MT_SEGQ_N + i] = res[i];
}

/* ---- batched dumps (mt_engine_dumps): no perspective, so no status; only q.doc and q.slot are read ---- */
/* the byte size of query i's canonical dump (size[slot]): every lane sizes one row's record per pass, the wave
 * sums them (Replica::dump_wave without a buffer); what Replica::dump(nullptr, 0) returns */
template <class HT>
__global__ __launch_bounds__(WG) void k_dump_sizes(Store<HT> st, int64_t m, const ReadQ* qs, int64_t* size) {
    if ((int64_t)blockIdx.x >= m) return;
    const ReadQ q = qs[blockIdx.x];
    Replica<WaveGPU, HT> r(st.doc(q.doc), WaveGPU());
    int64_t n = r.dump_wave(nullptr, 0);
    if (threadIdx.x == 0) size[q.slot] = n;
}
/* query i's dump into out[off[slot], off[slot + 1]) (the host's prefix sum of k_dump_sizes' sizes) and nowhere
 * else. PAR: the whole wave writes (Replica::dump_wave); else lane 0 writes byte by byte (Replica::dump, what
 * k_dump runs): the same bytes either way. */
template <class HT, bool PAR>
__global__ __launch_bounds__(WG) void k_dumps(Store<HT> st, int64_t m, const ReadQ* qs, const int64_t* off,
                                             uint8_t* out) {
    if ((int64_t)blockIdx.x >= m) return;
    const ReadQ q = qs[blockIdx.x];
    const int64_t o = off[q.slot], cap = off[q.slot + 1] - o;
    if (cap <= 0) return;
    Replica<WaveGPU, HT> r(st.doc(q.doc), WaveGPU());
    if constexpr (PAR)
        (void)r.dump_wave(out + o, cap);
    else
        (void)r.dump(out + o, cap);
}

/* ---- batched summaries (mt_engine_summaries): the summary dump (mt_oplog.h) of each query's document; as the
 * batched dumps, only q.doc and q.slot are read ---- */
/* the byte size of query i's summary dump (size[slot]): Replica::summary_wave without a buffer, the decisions of
 * the fill */
template <class HT>
__global__ __launch_bounds__(WG) void k_summary_sizes(Store<HT> st, int64_t m, const ReadQ* qs, int32_t mode,
                                                     int64_t* size) {
    if ((int64_t)blockIdx.x >= m) return;
    const ReadQ q = qs[blockIdx.x];
    Replica<WaveGPU, HT> r(st.doc(q.doc), WaveGPU());
    int64_t n = r.summary_wave(nullptr, 0, mode);
    if (threadIdx.x == 0) size[q.slot] = n;
}
/* query i's summary dump into out[off[slot], off[slot + 1]) and nowhere else. PAR: the whole wave writes
 * (Replica::summary_wave); else lane 0 writes (Replica::summary): the same bytes either way. */
template <class HT, bool PAR>
__global__ __launch_bounds__(WG) void k_summaries(Store<HT> st, int64_t m, const ReadQ* qs, int32_t mode,
                                                 const int64_t* off, uint8_t* out) {
    if ((int64_t)blockIdx.x >= m) return;
    const ReadQ q = qs[blockIdx.x];
    const int64_t o = off[q.slot], cap = off[q.slot + 1] - o;
    if (cap <= 0) return;
    Replica<WaveGPU, HT> r(st.doc(q.doc), WaveGPU());
    if constexpr (PAR)
        (void)r.summary_wave(out + o, cap, mode);
    else
        (void)r.summary(out + o, cap, mode);
}

/* ---- batched marker queries (mt_engine_find_tiles / mt_engine_stack_contexts): the local view only, so no
 * perspective; q.a = the position (< 0: undefined), q.b = preceding (find_tiles). `key` is the label key's id and
 * `set` the call's one label as a bitmap over the host's value ids (Replica::label_in). The walks keep no scratch in
 * the document block. A refused query (the label key was annotated on a marker) has status MT_E_UNSUPPORTED. ---- */
static_assert(sizeof(mt_tile_ref) == 4 * MT_TILE_WORDS, "mt_tile_ref is Replica::tile_words' five words");
/* MergeTree.findTile per query: out[slot] (rid -1: none or refused), status[slot] */
template <class HT, bool PAR>
__global__ __launch_bounds__(WG) void k_find_tiles(Store<HT> st, int64_t m, const ReadQ* qs, int32_t key,
                                                  const uint32_t* set, int32_t* out, int32_t* status) {
    if ((int64_t)blockIdx.x >= m) return;
    const ReadQ q = qs[blockIdx.x];
    Replica<WaveGPU, HT> r(st.doc(q.doc), WaveGPU());
    int32_t res[MT_TILE_WORDS];
    int32_t rc;
    if constexpr (PAR)
        rc = r.find_tile_wave(q.a, q.b != 0, key, set, res);
    else
        rc = r.find_tile(q.a, q.b != 0, key, set, res);
    if (threadIdx.x == 0) {
        for (int i = 0; i < MT_TILE_WORDS; i++) out[(int64_t)q.slot * MT_TILE_WORDS + i] = res[i];
        status[q.slot] = rc == 2 ? MT_E_UNSUPPORTED : MT_OK;
    }
}
/* MergeTree.getStackContext per query, sized: count[slot] = the final depth, high[slot] = the deepest the walk gets
 * (the window k_stacks needs); both 0 for a refused query */
template <class HT>
__global__ __launch_bounds__(WG) void k_stack_sizes(Store<HT> st, int64_t m, const ReadQ* qs, int32_t key,
                                                   const uint32_t* set, int32_t* count, int64_t* high,
                                                   int32_t* status) {
    if ((int64_t)blockIdx.x >= m) return;
    const ReadQ q = qs[blockIdx.x];
    Replica<WaveGPU, HT> r(st.doc(q.doc), WaveGPU());
    int32_t d = 0, hw = 0;
    const int32_t rc = r.stack_context_wave(q.a, key, set, nullptr, 0, &d, &hw);
    if (threadIdx.x == 0) count[q.slot] = d, high[q.slot] = hw, status[q.slot] = rc == 2 ? MT_E_UNSUPPORTED : MT_OK;
}
/* query i's stack in its window out[off[slot], off[slot + 1]) (entries of MT_TILE_WORDS words; the host's prefix sum
 * of k_stack_sizes' high-water marks) and nowhere else: the first count[slot] entries are the answer, bottom first.
 * PAR: the wave form; else the serial walk, lane 0 writing: the same entries either way. */
template <class HT, bool PAR>
__global__ __launch_bounds__(WG) void k_stacks(Store<HT> st, int64_t m, const ReadQ* qs, int32_t key,
                                              const uint32_t* set, const int64_t* off, int32_t* out) {
    if ((int64_t)blockIdx.x >= m) return;
    const ReadQ q = qs[blockIdx.x];
    const int64_t o = off[q.slot], cap = off[q.slot + 1] - o;
    if (cap <= 0) return;
    Replica<WaveGPU, HT> r(st.doc(q.doc), WaveGPU());
    int32_t d, hw;
    const int32_t c = cap > 0x7fffffff ? 0x7fffffff : (int32_t)cap;
    if constexpr (PAR)
        (void)r.stack_context_wave(q.a, key, set, out + o * MT_TILE_WORDS, c, &d, &hw);
    else
        (void)r.stack_context(q.a, key, set, out + o * MT_TILE_WORDS, c, &d, &hw);
}

/* ---- batched matrix reads (mt_engine_get_handles / mt_engine_handles_to_positions / mt_engine_handle_tables): the
 * PermutationVector reads of a SharedMatrix host, in the local view only, so no perspective. The walks keep no scratch
 * in the document block. ---- */
/* a handle range query (q.a = start, q.b = end) is valid when 0 <= start <= end <= the local length (the assert of
 * getMaybeHandle, permutationvector.ts:158, and ensureRange's RangeError, handlecache.ts:102): size[slot] = end - start,
 * else 0 and status MT_E_ARG */
template <class HT>
__global__ __launch_bounds__(WG) void k_handle_sizes(Store<HT> st, int64_t m, const ReadQ* qs, int64_t* size,
                                                    int32_t* status) {
    if ((int64_t)blockIdx.x >= m) return;
    const ReadQ q = qs[blockIdx.x];
    Replica<WaveGPU, HT> r(st.doc(q.doc), WaveGPU());
    const bool ok = 0 <= q.a && q.a <= q.b && q.b <= r.length_local();
    if (threadIdx.x == 0) size[q.slot] = ok ? (int64_t)q.b - q.a : 0, status[q.slot] = ok ? MT_OK : MT_E_ARG;
}
/* query i's handles into out[off[slot], off[slot + 1]) (the host's prefix sum of k_handle_sizes' sizes: an invalid
 * query's window is empty) and nowhere else. PAR: the wave writes each pass's run together (Replica::get_handles);
 * else the serial row walk, lane 0 writing: the same words either way. */
template <class HT, bool PAR>
__global__ __launch_bounds__(WG) void k_handles(Store<HT> st, int64_t m, const ReadQ* qs, const int64_t* off,
                                               int32_t* out) {
    if ((int64_t)blockIdx.x >= m) return;
    const ReadQ q = qs[blockIdx.x];
    const int64_t o = off[q.slot], cap = off[q.slot + 1] - o;
    if (cap <= 0) return;
    Replica<WaveGPU, HT> r(st.doc(q.doc), WaveGPU());
    (void)r.template get_handles<PAR>(q.a, q.b, out + o, cap);
}
/* PermutationVector.handleToPosition per query (q.a = handle, q.b = localSeq, MT_LOCAL_SEQ_CURRENT: the replica's
 * own): out[slot] = the position, or -1 and status MT_E_ARG where the reference asserts. PAR: 64 rows per pass
 * (Replica::handle_to_position_wave); else k_seg's mode 6, a leaf per pass. */
template <class HT, bool PAR>
__global__ __launch_bounds__(WG) void k_handle_positions(Store<HT> st, int64_t m, const ReadQ* qs, int32_t* out,
                                                        int32_t* status) {
    if ((int64_t)blockIdx.x >= m) return;
    const ReadQ q = qs[blockIdx.x];
    Replica<WaveGPU, HT> r(st.doc(q.doc), WaveGPU());
    const int32_t lseq = q.b == MT_LOCAL_SEQ_CURRENT ? r.zh->localSeq : q.b;
    int32_t pos = -1;
    bool found;
    if constexpr (PAR) {
        found = r.handle_to_position_wave(q.a, lseq, &pos);
    } else {
        int32_t res[MT_SEGQ_N];
        seg_eval<HT>(r, 6, q.a, lseq, 0, -1, 0, res);
        found = res[0] == 1;
        pos = res[1];
    }
    if (threadIdx.x == 0) out[q.slot] = found ? pos : -1, status[q.slot] = found ? MT_OK : MT_E_ARG;
}
/* HandleTable.snapshot() per query: size[slot] = the length of the document's `handles` array (DState.hlen) */
template <class HT>
__global__ __launch_bounds__(WG) void k_handle_table_sizes(Store<HT> st, int64_t m, const ReadQ* qs, int64_t* size) {
    if ((int64_t)blockIdx.x >= m) return;
    const ReadQ q = qs[blockIdx.x];
    if (threadIdx.x == 0) size[q.slot] = st.doc(q.doc).dstate()->hlen;
}
/* the table's words into out[off[slot], off[slot + 1]) and nowhere else, copied by the wave */
template <class HT>
__global__ __launch_bounds__(WG) void k_handle_tables(Store<HT> st, int64_t m, const ReadQ* qs, const int64_t* off,
                                                     int32_t* out) {
    if ((int64_t)blockIdx.x >= m) return;
    const ReadQ q = qs[blockIdx.x];
    const int64_t o = off[q.slot], cap = off[q.slot + 1] - o;
    const Doc<HT> v = st.doc(q.doc);
    const int64_t n = v.dstate()->hlen;
    const int32_t* t = v.ht();
    for (int64_t i = threadIdx.x; i < n && i < cap; i += WG) out[o + i] = t[i];
}

/* ---- batched delta-event reads (mt_engine_deltas_batch): the MT_DELTA_* streams (mt_oplog.h) of many documents, one
 * wave per query; q.a = the cursor (a word index, < 0: invalid). The kernels read the DState and the logged words and
 * nothing else: no Replica is built, so they keep no scratch in the document block (checked against Doc::dstate /
 * Doc::dlog, which only add offsets), and a tiled document may be named by any number of queries of one launch;
 * read_plan's successive launches for tiled documents are harmless.
 *
 * Event boundaries are found structurally, not by looking for MT_DELTA_END among all words. mt_oplog.h promises only
 * that no position or length equals it, and the other words can: an ANNOTATE segment's property delta is
 * (key << 16 | previous value) (Replica::prop_deltas), mt_kv.key is a full uint16 and the host interners hand out key
 * ids up to 0xFFFE, so key 0x8000 with no previous value (0) is exactly 0x80000000; `seq` is the record's, which
 * mt_engine_submit does not bound either. (`nd` is a count >= -1 and a REGEN op type is 0..2: those two cannot.) So a
 * ballot on the terminator's value over every word would split such an event in two. What dhead / dseg / dtail and the
 * emitters do fix is the shape: op, seq, then segments of (pos, len, nd) with nd delta words after it only in an
 * ANNOTATE event with nd > 0, then MT_DELTA_END where the next `pos` would be, then nseg. Only `pos` slots are ever
 * compared with MT_DELTA_END. In every event but ANNOTATE the pos slots are 3 words apart, so the wave tests 64 of
 * them per pass (PAR); an ANNOTATE event chains through its nd counts. The serial form (!PAR) chains every event and
 * lane 0 copies: the same words either way. */
template <bool PAR>
__device__ inline int64_t delta_event_end(const int32_t* log, int64_t i, int64_t n) {
    /* the word after the nseg of the event at i, -1 when the n logged words cut it short */
    if (i + 2 > n) return -1;
    int64_t j = i + 2;
    if (PAR && log[i] != MT_DELTA_ANNOTATE) {
        for (;;) {
            const int64_t x = j + 3 * (int64_t)(threadIdx.x & 63);
            const uint64_t hit = __ballot(x < n && log[x] == MT_DELTA_END);
            if (hit) {
                const int64_t t = j + 3 * (int64_t)__builtin_ctzll(hit) + 2;
                return t <= n ? t : -1;
            }
            j += 3 * 64;
            if (j >= n) return -1;
        }
    }
    while (j < n) {
        if (log[j] == MT_DELTA_END) return j + 2 <= n ? j + 2 : -1;
        if (j + 3 > n) return -1;
        const int32_t nd = log[j + 2];
        j += 3 + (log[i] == MT_DELTA_ANNOTATE && nd > 0 ? nd : 0);
    }
    return -1;
}
/* one query's window: the number of words it holds (written to out[0, that) when out != nullptr; never more than cap),
 * *end = the next cursor, *rc = MT_E_ARG for an invalid cursor (an empty window, *end = from) */
template <bool PAR>
__device__ inline int64_t delta_window(const int32_t* log, int64_t n, int64_t from, int32_t kinds, int32_t* out,
                                       int64_t cap, int64_t* end, int32_t* rc) {
    const int lane = threadIdx.x & 63;
    *rc = MT_OK;
    *end = from;
    bool ok = 0 <= from && from <= n;
    if (ok && from != 0 && from != n) { /* an event boundary: the walk from word 0 lands on it */
        int64_t i = 0;
        while (i >= 0 && i < from) i = delta_event_end<PAR>(log, i, n);
        ok = i == from;
    }
    if (!ok) {
        *rc = MT_E_ARG;
        return 0;
    }
    auto copy = [&](int64_t src, int64_t len, int64_t dst) {
        if (!out) return;
        if (PAR) {
            for (int64_t k = lane; k < len && dst + k < cap; k += 64) out[dst + k] = log[src + k];
        } else if (lane == 0) {
            for (int64_t k = 0; k < len && dst + k < cap; k++) out[dst + k] = log[src + k];
        }
    };
    if (kinds == (MT_DELTA_KINDS_SEQUENCE | MT_DELTA_KINDS_MAINTENANCE)) {
        copy(from, n - from, 0);
        *end = n;
        return n - from;
    }
    /* whole events of one kind; neighbouring kept events are copied as one run */
    const bool want_seq = kinds == MT_DELTA_KINDS_SEQUENCE;
    int64_t i = from, total = 0, run = -1;
    while (i < n) {
        const int64_t t = delta_event_end<PAR>(log, i, n);
        if (t < 0) break; /* the trailing event dcap cut short: left out, the next cursor is its start */
        const bool keep = (log[i] >= 0) == want_seq;
        if (keep && run < 0) run = i;
        if (!keep && run >= 0) {
            copy(run, i - run, total);
            total += i - run;
            run = -1;
        }
        i = t;
    }
    if (run >= 0) {
        copy(run, i - run, total);
        total += i - run;
    }
    *end = i;
    return total;
}
/* the logged words of a document as the caller's engine counts them: min(n, dcap) with the caller's dcap, and never
 * past this store's own log */
template <class HT>
__device__ inline int64_t delta_logged(const Doc<HT>& v, int32_t dcap) {
    int64_t n = v.dstate()->n;
    if (n > dcap) n = dcap;
    if (n > v.caps.dcap) n = v.caps.dcap;
    return n < 0 ? 0 : n;
}
/* size[slot] = the words of query i's window, end[slot] = its next cursor, emit[slot] = DState.n, status[slot] */
template <class HT, bool PAR>
__global__ __launch_bounds__(WG) void k_delta_sizes(Store<HT> st, int64_t m, const ReadQ* qs, int32_t dcap,
                                                   int32_t kinds, int64_t* size, int64_t* end, int64_t* emit,
                                                   int32_t* status) {
    if ((int64_t)blockIdx.x >= m) return;
    const ReadQ q = qs[blockIdx.x];
    const Doc<HT> v = st.doc(q.doc);
    int64_t e;
    int32_t rc;
    const int64_t n = delta_window<PAR>(v.dlog(), delta_logged(v, dcap), q.a, kinds, nullptr, 0, &e, &rc);
    if (threadIdx.x == 0) size[q.slot] = n, end[q.slot] = e, emit[q.slot] = v.dstate()->n, status[q.slot] = rc;
}
/* query i's window into out[off[slot], off[slot + 1]) (the host's prefix sum of k_delta_sizes' sizes) and nowhere
 * else */
template <class HT, bool PAR>
__global__ __launch_bounds__(WG) void k_deltas(Store<HT> st, int64_t m, const ReadQ* qs, int32_t dcap, int32_t kinds,
                                              const int64_t* off, int32_t* out) {
    if ((int64_t)blockIdx.x >= m) return;
    const ReadQ q = qs[blockIdx.x];
    const int64_t o = off[q.slot], cap = off[q.slot + 1] - o;
    if (cap <= 0) return;
    const Doc<HT> v = st.doc(q.doc);
    int64_t e;
    int32_t rc;
    (void)delta_window<PAR>(v.dlog(), delta_logged(v, dcap), q.a, kinds, out + o, cap, &e, &rc);
}

/* every segment's handle in walkAllSegments order (the canonical dump's record order): out[2i] = row id,
 * out[2i+1] = its generation; *n = the segment count (writes at most cap pairs) */
template <class HT>
__global__ __launch_bounds__(WG) void k_segids(Store<HT> st, int64_t doc, int32_t* out, int64_t cap, int64_t* n) {
    Replica<WaveGPU, HT> r(st.doc(doc), WaveGPU());
    int64_t base = 0;
    for (int32_t k = 0; r.kvalid(k); k = r.knext(k)) {
        int32_t lf = r.leaf_at(k), c = r.nch[lf];
        int32_t j = threadIdx.x;
        if (j < c && j < MAXN && base + j < cap) {
            int32_t rid = r.z.rid[lf * MAXN + j];
            out[2 * (base + j)] = rid;
            out[2 * (base + j) + 1] = r.z.rgen[rid];
        }
        base += c;
    }
    if (threadIdx.x == 0) *n = base;
}

/* local references: per doc their count and LocalReference.toPosition() of each (-1 detached) */
template <class HT>
__global__ __launch_bounds__(WG) void k_refpos(Store<HT> st, int64_t ndocs, int32_t rcap, int32_t* nref, int32_t* pos) {
    int64_t d = blockIdx.x;
    if (d >= ndocs) return;
    Replica<WaveGPU, HT> r(st.doc(d), WaveGPU());
    int32_t n = r.d.dstate()->nref;
    for (int32_t i = 0; i < n; i++) {
        int32_t p = r.ref_position(i);
        if (threadIdx.x == 0) pos[d * rcap + i] = p;
    }
    if (threadIdx.x == 0) nref[d] = n;
}

/* per-doc header fields: errors, stats, roofline work counters */
template <class HT>
__global__ void k_hdr(Store<HT> st, int64_t ndocs, int32_t* err, int32_t* err_op, int32_t* stats4, int64_t* work3,
                      int64_t* times2) {
    int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= ndocs) return;
    const DocHdr& h = st.doc(d).t->h;
    if (times2) {
        times2[2 * d] = h.tStart;
        times2[2 * d + 1] = h.tEnd;
    }
    if (err) err[d] = h.err;
    if (err_op) err_op[d] = h.errOp;
    if (stats4) {
        stats4[4 * d + 0] = h.nleaf;
        stats4[4 * d + 1] = h.hwSlots;
        stats4[4 * d + 2] = h.hwHeap;
        stats4[4 * d + 3] = h.opsDone;
    }
    if (work3) {
        work3[3 * d + 0] = h.seqOps;
        work3[3 * d + 1] = h.sumR;
        work3[3 * d + 2] = h.sumW;
    }
}

/* ------------------------------------------------------------------------------------------
 * engine (host side)
 * ---------------------------------------------------------------------------------------- */
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

struct ProfOps;

struct mt_engine {
    const ProfOps* ops = nullptr; /* the profile's launchers (one translation unit per profile) */
    /* capacity promotion (mt_engine_sync): the documents a replay left with E_CAPACITY replay again, from
     * their staged logs, in an engine of the next profile (`over`); per-document queries route there */
    bool promote = true;
    bool ran = false;                 /* a replay was launched since the last sync */
    bool fresh = true;                /* no replay since create / reset: the staged log is each replica's whole history */
    bool ran_fresh = false;           /* the last launched replay started from such a state */
    bool forwarded = false;           /* the last replay also ran the promoted documents' records in `over` */
    mt_engine* over = nullptr;
    std::vector<int32_t> pro;         /* doc -> index in `over`, -1: not promoted */
    std::vector<int64_t> pro_docs;    /* index in `over` -> doc */
    std::vector<int64_t> h_op_off, h_text_off, h_props_off, h_kv_off; /* host copies of the staged offsets */
    std::vector<int32_t> h_local;     /* start_collab's local long ids, then per doc minSeq, then currentSeq */
    mt_caps caps0 = {};               /* creation capacities */
    bool borrowed = false;            /* text / props / kv point into the parent's staged pools */
    int device;
    int64_t ndocs;
    int32_t dcap = 0; /* delta event log words per document (0: off) */
    int32_t rcap = 0; /* local references per document (0: none) */
    int32_t pcap = 0; /* PermutationVector handles per document (0: none) */
    bool fx = false;  /* delta events or local references: the client-feature replay build */
    bool loads = false; /* the staged batch holds snapshot-load records (the config-2/3 kernel's full build) */
    Profile profile = P_SMALL;
    int waves = 8;    /* occupancy target of the HBM-resident small-profile kernel */
    bool wide = false; /* tiled profile: the variant with the heap in HBM and the full window set (promotion target) */
    AnyStore st = {};  /* the documents' blocks (st.base: device memory the engine owns) */
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_ms = 0.f;
    bool staged = false;
    DevBuf ops_buf, op_off, text, text_off, props, props_off, kv, kv_off, tmp, local_ids, prof;
    DevBuf order;    /* dispatch order of the replay kernel (empty: document order) */
    bool collab = false;
    std::string err;
    /* perspective floors (persp_refused): per document, the greatest refSeq each long client has sent a
     * sequenced op under (long id, refSeq pairs), and a floor for every client (a snapshot load's currentSeq:
     * the loaded window's ops are not in the log). `staged` is built by mt_engine_submit from the staged
     * records, `applied` covers every record replayed since create / reset. */
    struct Persp {
        int32_t all = INT32_MIN;
        int32_t segk = 0; /* segment kinds the document's records inserted: 1 TextSegment, 2 SubSequence (never both) */
        std::vector<std::pair<int32_t, int32_t>> ref;
        void note(int32_t c, int32_t r) {
            for (auto& x : ref)
                if (x.first == c) {
                    if (r > x.second) x.second = r;
                    return;
                }
            ref.emplace_back(c, r);
        }
        void merge(const Persp& o) {
            if (o.all > all) all = o.all;
            segk |= o.segk;
            for (auto& x : o.ref) note(x.first, x.second);
        }
        int32_t floor(int32_t c) const {
            int32_t f = all;
            for (auto& x : ref)
                if (x.first == c && x.second > f) f = x.second;
            return f;
        }
    };
    std::vector<Persp> persp_staged, persp_applied;
    /* the replay launch's document range and stream (mt_engine_run: all documents on `stream`; the chunked
     * mt_engine_submit_run: one range per chunk, alternating between `stream` and `stream2`) */
    int64_t run_d0 = 0, run_n = -1;
    int64_t chunk = 0; /* documents per chunk of mt_engine_submit_run (0: automatic) */
    /* a staged batch of some documents only (mt_engine_submit_docs): their ids (`sub`, increasing; nsub = -1: every
     * document); the staged offsets then hold one entry per listed document */
    int64_t nsub = -1;
    DevBuf sub;
    std::vector<int64_t> h_sub;
    /* the host's value kinds (mt_engine_set_value_kinds) */
    DevBuf vkind;
    int32_t nvk = 0;
    std::vector<uint8_t> h_vkind;
    bool texts_packed = true; /* k_texts' copy (MT_VAR_TEXTS_PACKED) */
    bool dumps_parallel = true; /* k_dumps' writer (MT_VAR_DUMPS_PARALLEL) */
    bool summaries_parallel = true; /* k_summaries' writer (MT_VAR_SUMMARIES_PARALLEL) */
    bool tiles_parallel = true; /* k_find_tiles' / k_stacks' walk (MT_VAR_TILES_PARALLEL) */
    bool handles_parallel = true; /* k_handles' / k_handle_positions' walk (MT_VAR_HANDLES_PARALLEL) */
    bool deltas_parallel = true; /* k_delta_sizes' / k_deltas' walk and copy (MT_VAR_DELTAS_PARALLEL) */
    DevBuf rq;                                   /* the batched reads' queries, results and text (mt_replay.hip) */
    hipStream_t run_stream = nullptr;
    /* mt_engine_submit_run: the copy stream, the second compute stream, and pinned staging buffers for pageable
     * sources (each with the event of the last copy out of it) */
    hipStream_t cstream = nullptr, stream2 = nullptr;
    hipEvent_t evs = nullptr, evc = nullptr, ev2 = nullptr;
    struct Pin {
        void* p = nullptr;
        hipEvent_t ev = nullptr;
    };
    static constexpr int NPIN = 3;
    Pin pin[NPIN];
    int pin_i = 0;
};

static inline int32_t hip_fail(mt_engine* e, hipError_t st, const char* what) {
    if (e) e->err = std::string(what) + ": " + hipGetErrorString(st);
    return MT_E_HIP;
}
#define HIPCHK(e, x)                                        \
    do {                                                    \
        hipError_t st_ = (x);                               \
        if (st_ != hipSuccess) return hip_fail(e, st_, #x); \
    } while (0)

static inline int32_t launch_check(mt_engine* e, const char* what) {
    hipError_t st = hipGetLastError();
    if (st != hipSuccess) return hip_fail(e, st, what);
    return MT_OK;
}

static inline dim3 docs_grid(int64_t n) { return dim3((unsigned)n); }
static inline dim3 flat_grid(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

/* The store-dependent launches of one profile. Device pointers come from the engine's buffers. */
struct ProfOps {
    int32_t (*init)(mt_engine* e);                                    /* k_init (+ k_start_collab) */
    int32_t (*start_collab)(mt_engine* e); /* k_start_collab from local_ids (ids, minSeq, currentSeq per doc) */
    int32_t (*replay)(mt_engine* e);                                  /* k_replay over the staged batch */
    int32_t (*hdr)(mt_engine* e, int32_t* de, int32_t* deo, int32_t* ds, int64_t* dw, int64_t* dt);
    int32_t (*digest)(mt_engine* e, uint64_t* dout);
    int32_t (*dump)(mt_engine* e, int64_t doc, uint8_t* dbuf, int64_t cap, int64_t* dn);
    /* the reads take the perspective floor of persp_refused (the host's per-client refSeq bound) */
    int32_t (*length)(mt_engine* e, int64_t doc, int32_t ref_seq, int32_t long_client, int32_t floor, int32_t* dout);
    int32_t (*text)(mt_engine* e, int64_t doc, int32_t ref_seq, int32_t long_client, int32_t floor, int32_t start,
                    int32_t end, const uint16_t* dph, int32_t pl, uint16_t* dbuf, int64_t cap, int64_t* dn);
    int32_t (*seg)(mt_engine* e, int64_t doc, int32_t mode, int32_t a, int32_t b, int32_t ref_seq,
                   int32_t long_client, int32_t floor, int32_t* dout);
    int32_t (*refpos)(mt_engine* e, int32_t* dn, int32_t* dpos);
    int32_t (*segids)(mt_engine* e, int64_t doc, int32_t* dout, int64_t cap, int64_t* dn);
    /* the batched reads: dq[0, m) queries of this engine's documents, launched on s (results by ReadQ.slot) */
    int32_t (*lengths)(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int32_t* dlen, int32_t* dstatus);
    int32_t (*text_sizes)(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int32_t pl, int64_t* dsize,
                          int32_t* dstatus);
    int32_t (*texts)(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, const uint16_t* dph, int32_t pl,
                     const int64_t* doff, uint16_t* dout, bool packed);
    int32_t (*segs)(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int32_t mode, int32_t* dres);
    int32_t (*dump_sizes)(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int64_t* dsize);
    int32_t (*dumps)(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, const int64_t* doff, uint8_t* dout,
                     bool par);
    int32_t (*summary_sizes)(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int32_t mode, int64_t* dsize);
    int32_t (*summaries)(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int32_t mode, const int64_t* doff,
                         uint8_t* dout, bool par);
    /* the marker queries: dset = the label's value bitmap (1,024 words) on the device */
    int32_t (*find_tiles)(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int32_t key, const uint32_t* dset,
                          int32_t* dout, int32_t* dstatus, bool par);
    int32_t (*stack_sizes)(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int32_t key, const uint32_t* dset,
                           int32_t* dcount, int64_t* dhigh, int32_t* dstatus);
    int32_t (*stacks)(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int32_t key, const uint32_t* dset,
                      const int64_t* doff, int32_t* dout, bool par);
    /* the matrix reads */
    int32_t (*handle_sizes)(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int64_t* dsize, int32_t* dstatus);
    int32_t (*handles)(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, const int64_t* doff, int32_t* dout,
                       bool par);
    int32_t (*handle_positions)(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int32_t* dout,
                                int32_t* dstatus, bool par);
    int32_t (*handle_table_sizes)(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int64_t* dsize);
    int32_t (*handle_tables)(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, const int64_t* doff,
                             int32_t* dout);
    /* the delta-event reads: dcap = the caller's engine's (a promoted document's engine logs more) */
    int32_t (*delta_sizes)(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int32_t dcap, int32_t kinds,
                           int64_t* dsize, int64_t* dend, int64_t* demit, int32_t* dstatus, bool par);
    int32_t (*deltas)(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int32_t dcap, int32_t kinds,
                      const int64_t* doff, int32_t* dout, bool par);
};
/* each profile's table (host functions, defined in its mt_prof_*.hip) */
const ProfOps* ops_small();
const ProfOps* ops_mat();
const ProfOps* ops_mid();
const ProfOps* ops_big();
const ProfOps* ops_huge();

/* the engine's store as the kernels of its profile take it */
template <class HT>
static inline Store<HT> store_of(const mt_engine* e) {
    return e->st.as<HT>();
}

/* one replay kernel over the staged batch (a document per workgroup) */
template <class HT, class K>
static inline int32_t launch_replay(mt_engine* e, K kern, int block = WG) {
    const int64_t n = e->run_n >= 0 ? e->run_n : e->nsub >= 0 ? e->nsub : e->ndocs;
    if (n <= 0) return MT_OK;
    const int32_t* order = e->nsub >= 0 ? (const int32_t*)e->sub.p : (const int32_t*)e->order.p;
    hipLaunchKernelGGL(kern, docs_grid(n), dim3(block), 0, e->run_stream ? e->run_stream : e->stream, store_of<HT>(e),
                       e->ndocs, (const mt_op_rec*)e->ops_buf.p, (const int64_t*)e->op_off.p, (const uint16_t*)e->text.p,
                       (const int64_t*)e->text_off.p, (const mt_props_rec*)e->props.p, (const int64_t*)e->props_off.p,
                       (const mt_kv*)e->kv.p, (const int64_t*)e->kv_off.p,
                       ReplayAux{(uint64_t*)e->prof.p, order, e->run_d0, e->nsub >= 0 ? 1 : 0,
                                 (const uint8_t*)e->vkind.p, e->nvk});
    return launch_check(e, "k_replay");
}

/* the launchers every profile shares (replay is the profile's own) */
template <class HT>
struct Launch {
    static int32_t init(mt_engine* e) {
        const Store<HT> st = store_of<HT>(e);
        hipLaunchKernelGGL((k_init<HT>), docs_grid(e->ndocs), dim3(WG), 0, e->stream, st, e->ndocs);
        int32_t rc = launch_check(e, "k_init");
        if (rc || !e->collab) return rc;
        hipLaunchKernelGGL((k_start_collab<HT>), docs_grid(e->ndocs), dim3(WG), 0, e->stream, st, e->ndocs,
                           (const int32_t*)e->local_ids.p);
        return launch_check(e, "k_start_collab");
    }
    static int32_t start_collab(mt_engine* e) {
        hipLaunchKernelGGL((k_start_collab<HT>), docs_grid(e->ndocs), dim3(WG), 0, e->stream, store_of<HT>(e),
                           e->ndocs, (const int32_t*)e->local_ids.p);
        return launch_check(e, "k_start_collab");
    }
    static int32_t hdr(mt_engine* e, int32_t* de, int32_t* deo, int32_t* ds, int64_t* dw, int64_t* dt) {
        hipLaunchKernelGGL((k_hdr<HT>), flat_grid(e->ndocs), dim3(256), 0, e->stream, store_of<HT>(e), e->ndocs, de,
                           deo, ds, dw, dt);
        return launch_check(e, "k_hdr");
    }
    static int32_t digest(mt_engine* e, uint64_t* dout) {
        hipLaunchKernelGGL((k_digest<HT>), docs_grid(e->ndocs), dim3(WG), 0, e->stream, store_of<HT>(e), e->ndocs,
                           dout);
        return launch_check(e, "k_digest");
    }
    static int32_t dump(mt_engine* e, int64_t doc, uint8_t* dbuf, int64_t cap, int64_t* dn) {
        hipLaunchKernelGGL((k_dump<HT>), dim3(1), dim3(WG), 0, e->stream, store_of<HT>(e), doc, dbuf, cap, dn);
        return launch_check(e, "k_dump");
    }
    static int32_t length(mt_engine* e, int64_t doc, int32_t ref_seq, int32_t long_client, int32_t floor,
                          int32_t* dout) {
        hipLaunchKernelGGL((k_length<HT>), dim3(1), dim3(WG), 0, e->stream, store_of<HT>(e), doc, ref_seq,
                           long_client, floor, dout);
        return launch_check(e, "k_length");
    }
    static int32_t text(mt_engine* e, int64_t doc, int32_t ref_seq, int32_t long_client, int32_t floor, int32_t start,
                        int32_t end, const uint16_t* dph, int32_t pl, uint16_t* dbuf, int64_t cap, int64_t* dn) {
        hipLaunchKernelGGL((k_text<HT>), dim3(1), dim3(WG), 0, e->stream, store_of<HT>(e), doc, ref_seq, long_client,
                           floor, start, end, dph, pl, dbuf, cap, dn);
        return launch_check(e, "k_text");
    }
    static int32_t seg(mt_engine* e, int64_t doc, int32_t mode, int32_t a, int32_t b, int32_t ref_seq,
                       int32_t long_client, int32_t floor, int32_t* dout) {
        hipLaunchKernelGGL((k_seg<HT>), dim3(1), dim3(WG), 0, e->stream, store_of<HT>(e), doc, mode, a, b, ref_seq,
                           long_client, floor, dout);
        return launch_check(e, "k_seg");
    }
    static int32_t refpos(mt_engine* e, int32_t* dn, int32_t* dpos) {
        hipLaunchKernelGGL((k_refpos<HT>), docs_grid(e->ndocs), dim3(WG), 0, e->stream, store_of<HT>(e), e->ndocs,
                           e->rcap, dn, dpos);
        return launch_check(e, "k_refpos");
    }
    static int32_t segids(mt_engine* e, int64_t doc, int32_t* dout, int64_t cap, int64_t* dn) {
        hipLaunchKernelGGL((k_segids<HT>), dim3(1), dim3(WG), 0, e->stream, store_of<HT>(e), doc, dout, cap, dn);
        return launch_check(e, "k_segids");
    }
    static int32_t lengths(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int32_t* dlen,
                           int32_t* dstatus) {
        hipLaunchKernelGGL((k_lengths<HT>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq, dlen, dstatus);
        return launch_check(e, "k_lengths");
    }
    static int32_t text_sizes(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int32_t pl, int64_t* dsize,
                              int32_t* dstatus) {
        hipLaunchKernelGGL((k_text_sizes<HT>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq, pl, dsize,
                           dstatus);
        return launch_check(e, "k_text_sizes");
    }
    static int32_t texts(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, const uint16_t* dph, int32_t pl,
                         const int64_t* doff, uint16_t* dout, bool packed) {
        if (packed)
            hipLaunchKernelGGL((k_texts<HT, true>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq, dph, pl,
                               doff, dout);
        else
            hipLaunchKernelGGL((k_texts<HT, false>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq, dph, pl,
                               doff, dout);
        return launch_check(e, "k_texts");
    }
    static int32_t segs(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int32_t mode, int32_t* dres) {
        hipLaunchKernelGGL((k_segs<HT>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq, mode, dres);
        return launch_check(e, "k_segs");
    }
    static int32_t dump_sizes(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int64_t* dsize) {
        hipLaunchKernelGGL((k_dump_sizes<HT>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq, dsize);
        return launch_check(e, "k_dump_sizes");
    }
    static int32_t dumps(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, const int64_t* doff, uint8_t* dout,
                         bool par) {
        if (par)
            hipLaunchKernelGGL((k_dumps<HT, true>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq, doff, dout);
        else
            hipLaunchKernelGGL((k_dumps<HT, false>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq, doff, dout);
        return launch_check(e, "k_dumps");
    }
    static int32_t summary_sizes(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int32_t mode,
                                 int64_t* dsize) {
        hipLaunchKernelGGL((k_summary_sizes<HT>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq, mode, dsize);
        return launch_check(e, "k_summary_sizes");
    }
    static int32_t summaries(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int32_t mode,
                             const int64_t* doff, uint8_t* dout, bool par) {
        if (par)
            hipLaunchKernelGGL((k_summaries<HT, true>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq, mode,
                               doff, dout);
        else
            hipLaunchKernelGGL((k_summaries<HT, false>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq, mode,
                               doff, dout);
        return launch_check(e, "k_summaries");
    }
    static int32_t find_tiles(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int32_t key,
                              const uint32_t* dset, int32_t* dout, int32_t* dstatus, bool par) {
        if (par)
            hipLaunchKernelGGL((k_find_tiles<HT, true>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq, key,
                               dset, dout, dstatus);
        else
            hipLaunchKernelGGL((k_find_tiles<HT, false>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq, key,
                               dset, dout, dstatus);
        return launch_check(e, "k_find_tiles");
    }
    static int32_t stack_sizes(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int32_t key,
                               const uint32_t* dset, int32_t* dcount, int64_t* dhigh, int32_t* dstatus) {
        hipLaunchKernelGGL((k_stack_sizes<HT>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq, key, dset,
                           dcount, dhigh, dstatus);
        return launch_check(e, "k_stack_sizes");
    }
    static int32_t stacks(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int32_t key, const uint32_t* dset,
                          const int64_t* doff, int32_t* dout, bool par) {
        if (par)
            hipLaunchKernelGGL((k_stacks<HT, true>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq, key, dset,
                               doff, dout);
        else
            hipLaunchKernelGGL((k_stacks<HT, false>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq, key, dset,
                               doff, dout);
        return launch_check(e, "k_stacks");
    }
    static int32_t handle_sizes(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int64_t* dsize,
                                int32_t* dstatus) {
        hipLaunchKernelGGL((k_handle_sizes<HT>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq, dsize, dstatus);
        return launch_check(e, "k_handle_sizes");
    }
    static int32_t handles(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, const int64_t* doff, int32_t* dout,
                           bool par) {
        if (par)
            hipLaunchKernelGGL((k_handles<HT, true>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq, doff, dout);
        else
            hipLaunchKernelGGL((k_handles<HT, false>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq, doff,
                               dout);
        return launch_check(e, "k_handles");
    }
    static int32_t handle_positions(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int32_t* dout,
                                    int32_t* dstatus, bool par) {
        if (par)
            hipLaunchKernelGGL((k_handle_positions<HT, true>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq,
                               dout, dstatus);
        else
            hipLaunchKernelGGL((k_handle_positions<HT, false>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq,
                               dout, dstatus);
        return launch_check(e, "k_handle_positions");
    }
    static int32_t handle_table_sizes(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int64_t* dsize) {
        hipLaunchKernelGGL((k_handle_table_sizes<HT>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq, dsize);
        return launch_check(e, "k_handle_table_sizes");
    }
    static int32_t handle_tables(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, const int64_t* doff,
                                 int32_t* dout) {
        hipLaunchKernelGGL((k_handle_tables<HT>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq, doff, dout);
        return launch_check(e, "k_handle_tables");
    }
    static int32_t delta_sizes(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int32_t dcap, int32_t kinds,
                               int64_t* dsize, int64_t* dend, int64_t* demit, int32_t* dstatus, bool par) {
        if (par)
            hipLaunchKernelGGL((k_delta_sizes<HT, true>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq, dcap,
                               kinds, dsize, dend, demit, dstatus);
        else
            hipLaunchKernelGGL((k_delta_sizes<HT, false>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq, dcap,
                               kinds, dsize, dend, demit, dstatus);
        return launch_check(e, "k_delta_sizes");
    }
    static int32_t deltas(mt_engine* e, hipStream_t s, int64_t m, const ReadQ* dq, int32_t dcap, int32_t kinds,
                          const int64_t* doff, int32_t* dout, bool par) {
        if (par)
            hipLaunchKernelGGL((k_deltas<HT, true>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq, dcap, kinds,
                               doff, dout);
        else
            hipLaunchKernelGGL((k_deltas<HT, false>), docs_grid(m), dim3(WG), 0, s, store_of<HT>(e), m, dq, dcap, kinds,
                               doff, dout);
        return launch_check(e, "k_deltas");
    }
    static ProfOps table(int32_t (*replay)(mt_engine*)) {
        return ProfOps{init,   start_collab, replay, hdr,     digest,     dump,  length, text,       seg,
                       refpos, segids,       lengths, text_sizes, texts, segs,   dump_sizes, dumps,
                       summary_sizes, summaries, find_tiles, stack_sizes, stacks,
                       handle_sizes, handles, handle_positions, handle_table_sizes, handle_tables,
                       delta_sizes, deltas};
    }
};
