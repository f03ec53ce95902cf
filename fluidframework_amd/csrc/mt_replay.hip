/*
 * mt_replay.hip — the C ABI of include/mt_engine.h over the replay kernels (mt_kernels.h).
 * Store-dependent launches go through the engine's ProfOps table; each profile's kernels live in
 * their own translation units (mt_prof_*.hip, mt_small_*.hip, mt_mat_*.hip).
 */
#include "mt_kernels.h"

#include <algorithm>
#include <thread>

static int32_t ensure(mt_engine* e, DevBuf& b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.cap >= bytes) return MT_OK;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
    hipError_t st = hipMalloc(&b.p, bytes);
    if (st != hipSuccess) return hip_fail(e, st, "hipMalloc(staging)");
    b.cap = bytes;
    return MT_OK;
}

/* each profile's launchers (mt_prof_*.hip) */
static const ProfOps* ops_for(Profile p) {
    switch (p) {
    case P_SMALL: return ops_small();
    case P_MAT: return ops_mat();
    case P_MID: return ops_mid();
    case P_BIG: return ops_big();
    case P_HUGE: return ops_huge();
    default: return nullptr;
    }
}

/* ---- staging the op logs ------------------------------------------------------------------------ */
struct SubmitArgs {
    const mt_op_rec* ops;
    const int64_t* op_off;
    const uint16_t* text;
    int64_t text_units;
    const int64_t* text_off;
    const mt_props_rec* props;
    int64_t nprops;
    const int64_t* props_off;
    const mt_kv* kv;
    int64_t nkv;
    const int64_t* kv_off;
};

/* host-side shape checks before the kernel trusts any offset */
static bool offsets_ok(const SubmitArgs& a, int64_t nd) {
    if (!a.op_off || !a.text_off || !a.props_off || !a.kv_off || a.text_units < 0 || a.nprops < 0 || a.nkv < 0)
        return false;
    if (a.op_off[0] < 0) return false;
    for (int64_t d = 0; d < nd; d++) {
        if (a.op_off[d] > a.op_off[d + 1] || a.text_off[d] < 0 || a.text_off[d] > a.text_units || a.props_off[d] < 0 ||
            a.props_off[d] > a.nprops || a.kv_off[d] < 0 || a.kv_off[d] > a.nkv)
            return false;
    }
    return !a.op_off[nd] || a.ops;
}

/* every pool reference of every event of documents [d0, d1) in bounds before the kernel dereferences it (in parallel
 * on the host: up to 16 threads, one contiguous range each); also each document's perspective floors
 * (mt_kernels.h persp_refused), whether it holds snapshot-load records, and (text_end) the end of the text the
 * documents reference */
static bool check_docs(const SubmitArgs& a, int64_t d0, int64_t d1, mt_engine::Persp* persp, char* loads,
                       int64_t* text_end) {
    int64_t te = 0;
    for (int64_t d = d0; d < d1; d++) {
        mt_engine::Persp& pp = persp[d];
        const int64_t to = a.text_off[d];
        for (int64_t i = a.op_off[d]; i < a.op_off[d + 1]; i++) {
            const mt_op_rec& o = a.ops[i];
            int kind = o.kind & MT_OP_KIND_MASK;
            if (!(o.kind & MT_OPF_LOCAL)) { /* perspective floors (mt_kernels.h persp_refused) */
                if (kind == MT_OP_RELOAD || kind == MT_OP_COLLAB || kind == MT_OP_APPEND) {
                    if (!(o.kind & MT_OPF_TREE)) loads[d] = 1; /* a snapshot load: the full build */
                    if (o.seq > pp.all) pp.all = o.seq;
                } else if (kind != MT_OP_NOOP && o.client != MT_CLIENT_LOCAL) {
                    pp.note(o.client, o.ref_seq);
                }
            }
            int64_t end = 0;
            if (kind == MT_OP_INSERT || kind == MT_OP_RELOAD || kind == MT_OP_APPEND) {
                /* a segment-bearing record: a known kind, and a document of TextSegments or of SubSequences, not both
                 * (mt_oplog.h MT_SEG_RUN; the kinds its earlier batches inserted are seeded by seed_segk) */
                const int sk = o.seg_kind & 0x7F;
                if (sk > MT_SEG_RUN) return false;
                const bool regen = (o.kind & (MT_OPF_LOCAL | MT_OPF_REGEN)) == (MT_OPF_LOCAL | MT_OPF_REGEN);
                const int32_t len = kind == MT_OP_INSERT ? o.text_len : o.pos2;
                if ((sk == MT_SEG_TEXT || sk == MT_SEG_RUN) && !regen && len > 0) pp.segk |= sk == MT_SEG_TEXT ? 1 : 2;
                if (pp.segk == 3) return false;
            }
            const bool units = (o.seg_kind & 0x7F) == MT_SEG_TEXT || (o.seg_kind & 0x7F) == MT_SEG_RUN;
            if (kind == MT_OP_INSERT && units) end = to + (int64_t)o.text_off + o.text_len;
            if (kind == MT_OP_NOOP && (o.kind & MT_OPF_LOCAL) && o.seg_kind == MT_NOOP_HTLOAD)
                end = to + (int64_t)o.text_off + o.text_len;
            if (o.seg_kind & MT_SEG_RELPOS) end = std::max(end, to + (int64_t)o.text_off + o.text_len + MT_RELPOS_UNITS);
            /* snapshot-load records carry the segment length in pos2 (mt_oplog.h) */
            if ((kind == MT_OP_RELOAD || kind == MT_OP_APPEND) && units) {
                if (o.pos2 < 0) return false;
                end = std::max(end, to + (int64_t)o.text_off + o.pos2);
            }
            if (end > a.text_units) return false;
            te = std::max(te, end);
            if (o.props) {
                if (a.props_off[d] + (int64_t)o.props > a.nprops) return false;
                const mt_props_rec& pr = a.props[a.props_off[d] + o.props - 1];
                if (a.kv_off[d] + (int64_t)pr.kv_off + pr.nkv > a.nkv) return false;
            }
        }
    }
    if (text_end) *text_end = te;
    return true;
}

static int host_threads() {
    unsigned hc = std::thread::hardware_concurrency();
    return (int)std::min<unsigned>(16, std::max<unsigned>(1, hc));
}

/* the segment kinds the staged documents' replicas already hold (an incremental batch; a reset clears them) */
static void seed_segk(const mt_engine* e, std::vector<mt_engine::Persp>& persp, const int64_t* docs) {
    for (size_t k = 0; k < persp.size(); k++) {
        size_t d = docs ? (size_t)docs[k] : k;
        persp[k].segk = !e->fresh && d < e->persp_applied.size() ? e->persp_applied[d].segk : 0;
    }
}

static bool check_range(const SubmitArgs& a, int64_t d0, int64_t d1, mt_engine::Persp* persp, char* loads,
                        int64_t* text_end) {
    int64_t nops = a.op_off[d1] - a.op_off[d0];
    int nth = nops > (1 << 20) ? host_threads() : 1;
    if (nth <= 1 || d1 - d0 < 2) return check_docs(a, d0, d1, persp, loads, text_end);
    nth = (int)std::min<int64_t>(nth, d1 - d0);
    std::vector<std::thread> th;
    std::vector<char> ok((size_t)nth, 1);
    std::vector<int64_t> te((size_t)nth, 0);
    for (int t = 0; t < nth; t++)
        th.emplace_back([&, t] {
            ok[(size_t)t] = check_docs(a, d0 + (d1 - d0) * t / nth, d0 + (d1 - d0) * (t + 1) / nth, persp, loads,
                                       &te[(size_t)t]);
        });
    for (auto& x : th) x.join();
    for (char c : ok)
        if (!c) return false;
    if (text_end) *text_end = *std::max_element(te.begin(), te.end());
    return true;
}

static int32_t ensure_staging(mt_engine* e, const SubmitArgs& a, int64_t nd = -1) {
    if (nd < 0) nd = e->ndocs; /* staged entries */
    int64_t nops = a.op_off[nd];
    int32_t rc;
    if ((rc = ensure(e, e->ops_buf, sizeof(mt_op_rec) * nops))) return rc;
    if ((rc = ensure(e, e->op_off, sizeof(int64_t) * (nd + 1)))) return rc;
    if ((rc = ensure(e, e->text, 2 * a.text_units))) return rc;
    if ((rc = ensure(e, e->text_off, sizeof(int64_t) * (nd + 1)))) return rc;
    if ((rc = ensure(e, e->props, sizeof(mt_props_rec) * a.nprops))) return rc;
    if ((rc = ensure(e, e->props_off, sizeof(int64_t) * (nd + 1)))) return rc;
    if ((rc = ensure(e, e->kv, sizeof(mt_kv) * a.nkv))) return rc;
    return ensure(e, e->kv_off, sizeof(int64_t) * (nd + 1));
}

/* the offsets and the property pools (small next to the records and the text) */
static int32_t copy_small(mt_engine* e, const SubmitArgs& a, hipStream_t s, int64_t nd = -1) {
    if (nd < 0) nd = e->ndocs; /* staged entries */
    HIPCHK(e, hipMemcpyAsync(e->op_off.p, a.op_off, sizeof(int64_t) * (nd + 1), hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(e->text_off.p, a.text_off, sizeof(int64_t) * nd, hipMemcpyHostToDevice, s));
    if (a.nprops) HIPCHK(e, hipMemcpyAsync(e->props.p, a.props, sizeof(mt_props_rec) * a.nprops, hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(e->props_off.p, a.props_off, sizeof(int64_t) * nd, hipMemcpyHostToDevice, s));
    if (a.nkv) HIPCHK(e, hipMemcpyAsync(e->kv.p, a.kv, sizeof(mt_kv) * a.nkv, hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(e->kv_off.p, a.kv_off, sizeof(int64_t) * nd, hipMemcpyHostToDevice, s));
    return MT_OK;
}

/* the host copies of a staged batch's offsets, floors and load flag */
static void keep_staged(mt_engine* e, const SubmitArgs& a, std::vector<mt_engine::Persp>& persp,
                        const std::vector<char>& loads) {
    int64_t nd = (int64_t)persp.size(); /* staged entries: every document, or the listed ones (mt_engine_submit_docs) */
    e->h_op_off.assign(a.op_off, a.op_off + nd + 1);
    e->h_text_off.assign(a.text_off, a.text_off + nd);
    e->h_props_off.assign(a.props_off, a.props_off + nd);
    e->h_kv_off.assign(a.kv_off, a.kv_off + nd);
    e->persp_staged.swap(persp);
    e->loads = std::find(loads.begin(), loads.end(), 1) != loads.end();
    e->staged = true;
}

static bool host_pinned(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t at;
    hipError_t st = hipPointerGetAttributes(&at, p);
    if (st != hipSuccess) {
        (void)hipGetLastError(); /* pageable memory is an error here, not a sticky one */
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

/* n bytes from host `src` to device `dst` on the copy stream: directly (pinned memory, or a single chunk), or through the engine's
 * pinned staging buffers (host threads fill one while the DMA engine drains the others) */
static constexpr size_t PIN_BYTES = (size_t)128 << 20;
static int32_t stage_h2d(mt_engine* e, void* dst, const void* src, size_t n, bool pinned) {
    if (!n) return MT_OK;
    if (pinned) {
        HIPCHK(e, hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, e->cstream));
        return MT_OK;
    }
    uint8_t* d = (uint8_t*)dst;
    const uint8_t* s = (const uint8_t*)src;
    while (n) {
        mt_engine::Pin& b = e->pin[e->pin_i];
        e->pin_i = (e->pin_i + 1) % mt_engine::NPIN;
        if (!b.p) {
            HIPCHK(e, hipHostMalloc(&b.p, PIN_BYTES, hipHostMallocDefault));
            HIPCHK(e, hipEventCreateWithFlags(&b.ev, hipEventDisableTiming));
        } else {
            HIPCHK(e, hipEventSynchronize(b.ev)); /* its previous copy has left it */
        }
        size_t m = std::min(n, PIN_BYTES);
        int nth = m >= ((size_t)8 << 20) ? std::min(8, host_threads()) : 1;
        if (nth <= 1) {
            memcpy(b.p, s, m);
        } else {
            std::vector<std::thread> th;
            for (int t = 0; t < nth; t++)
                th.emplace_back([&, t] {
                    size_t lo = (m * t / nth) & ~(size_t)63, hi = t + 1 == nth ? m : (m * (t + 1) / nth) & ~(size_t)63;
                    memcpy((uint8_t*)b.p + lo, s + lo, hi - lo);
                });
            for (auto& x : th) x.join();
        }
        HIPCHK(e, hipMemcpyAsync(d, b.p, m, hipMemcpyHostToDevice, e->cstream));
        HIPCHK(e, hipEventRecord(b.ev, e->cstream));
        d += m, s += m, n -= m;
    }
    return MT_OK;
}

/* stage a batch (mt_engine_submit: nsub = -1, an entry per document; mt_engine_submit_docs: an entry for each of the
 * nsub documents listed in `docs`) */
static int32_t submit(mt_engine* e, const SubmitArgs& a, int64_t nsub, const int64_t* docs) {
    const int64_t m = nsub < 0 ? e->ndocs : nsub; /* staged entries */
    if (!offsets_ok(a, m)) return MT_E_ARG;
    std::vector<mt_engine::Persp> persp((size_t)m);
    std::vector<char> loads((size_t)m, 0);
    seed_segk(e, persp, docs);
    if (!check_range(a, 0, m, persp.data(), loads.data(), nullptr)) return MT_E_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    int32_t rc;
    if ((rc = ensure_staging(e, a, m))) return rc;
    if (nsub >= 0 && (rc = ensure(e, e->sub, sizeof(int32_t) * (size_t)std::max<int64_t>(m, 1)))) return rc;
    e->nsub = nsub;
    e->h_sub.assign(docs, docs + std::max<int64_t>(nsub, 0));
    const std::vector<int32_t> ids(e->h_sub.begin(), e->h_sub.end());
    const int64_t nops = a.op_off[m];
    if (nops) HIPCHK(e, hipMemcpyAsync(e->ops_buf.p, a.ops, sizeof(mt_op_rec) * nops, hipMemcpyHostToDevice, e->stream));
    if (a.text_units) HIPCHK(e, hipMemcpyAsync(e->text.p, a.text, 2 * a.text_units, hipMemcpyHostToDevice, e->stream));
    if (!ids.empty())
        HIPCHK(e, hipMemcpyAsync(e->sub.p, ids.data(), sizeof(int32_t) * ids.size(), hipMemcpyHostToDevice, e->stream));
    if ((rc = copy_small(e, a, e->stream, m))) return rc;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    keep_staged(e, a, persp, loads);
    return MT_OK;
}

extern "C" {

int32_t mt_engine_create(int32_t device, int64_t ndocs, const mt_caps* caps, mt_engine** out) {
    if (!out || !caps || ndocs < 1 || ndocs > (int64_t)0x7fffffff) return MT_E_ARG;
    *out = nullptr;
    Caps k = {caps->acap, caps->mcap, caps->gcap, caps->dcap, caps->rcap, caps->pcap};
    Profile prof = profile_for(caps->ncap);
    if (!caps_valid(k) || prof == P_NONE || caps->ccap > 254 || caps->dcap < 0 || caps->rcap < 0 || caps->pcap < 0 ||
        caps->pcap > (1 << 24))
        return MT_E_ARG; /* short ids are bytes; 0xFF = LocalClientId */
    mt_engine* e = new mt_engine();
    e->device = device;
    e->ndocs = ndocs;
    e->dcap = caps->dcap;
    e->rcap = caps->rcap;
    e->pcap = caps->pcap;
    e->fx = caps->dcap > 0 || caps->rcap > 0 || caps->pcap > 0;
    const char* np = getenv("MT_NO_PROMOTE");
    e->promote = !(np && np[0] == '1');
    e->caps0 = *caps;
    e->pro.assign((size_t)ndocs, -1);
    e->profile = prof;
    e->ops = ops_for(prof);
    if (hipSetDevice(device) != hipSuccess) {
        delete e;
        return MT_E_HIP;
    }
    /* the small-profile kernel build (mt_prof_small.hip): the hot image in LDS when the batch's documents fit three
     * per CU (1: config 1 0.667 -> 0.691M ops/s, config 3 at 256 / 768 documents +3.0 / +1.5 %, profiles/r06l_ab/);
     * else HBM-resident, 4 waves per SIMD (no VGPR spills) when the documents, one wave each, fit 4 per SIMD (4 SIMDs
     * per CU), 8 otherwise; MT_SMALL_WAVES overrides */
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ncu < 1) ncu = 256;
    e->waves = ndocs <= (int64_t)ncu * 3 ? 1 : ndocs <= (int64_t)ncu * 4 * 4 ? 4 : 8;
    if (const char* sw = getenv("MT_SMALL_WAVES")) e->waves = atoi(sw) == 1 ? 1 : atoi(sw) == 4 ? 4 : 8;
    int64_t bytes = store_layout(e->st, prof, k, ndocs);
    if (hipMalloc((void**)&e->st.base, (size_t)bytes) != hipSuccess) {
        delete e;
        return MT_E_NOMEM;
    }
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&e->ev0) != hipSuccess || hipEventCreate(&e->ev1) != hipSuccess) {
        mt_engine_destroy(e);
        return MT_E_HIP;
    }
    /* The zero fill goes on the engine's own stream, ahead of k_init. A hipMemset on the null
     * stream is not ordered with a non-blocking stream: a large store's fill could still be running
     * when k_init wrote the last documents' headers, and zeroed them after it (round 2: the last
     * documents of a 3.2 GB tiled store failed at their first events, only in long test runs). */
    if (hipMemsetAsync(e->st.base, 0, (size_t)bytes, e->stream) != hipSuccess) {
        mt_engine_destroy(e);
        return MT_E_HIP;
    }
    if (e->ops->init(e) != MT_OK || hipStreamSynchronize(e->stream) != hipSuccess) {
        mt_engine_destroy(e);
        return MT_E_HIP;
    }
    *out = e;
    return MT_OK;
}

void mt_engine_destroy(mt_engine* e) {
    if (!e) return;
    mt_engine_destroy(e->over);
    (void)hipSetDevice(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->borrowed) e->text.p = e->props.p = e->kv.p = nullptr; /* the parent's */
    DevBuf* bufs[] = {&e->ops_buf, &e->op_off, &e->text, &e->text_off, &e->props,     &e->props_off,
                      &e->kv,     &e->kv_off, &e->tmp,  &e->local_ids, &e->prof, &e->order, &e->sub, &e->vkind,
                      &e->rq};
    for (DevBuf* b : bufs)
        if (b->p) (void)hipFree(b->p);
    if (e->st.base) (void)hipFree(e->st.base);
    if (e->ev0) (void)hipEventDestroy(e->ev0);
    if (e->ev1) (void)hipEventDestroy(e->ev1);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    if (e->cstream) {
        (void)hipStreamSynchronize(e->cstream);
        (void)hipStreamSynchronize(e->stream2);
        (void)hipStreamDestroy(e->cstream);
        (void)hipStreamDestroy(e->stream2);
        (void)hipEventDestroy(e->evs);
        (void)hipEventDestroy(e->evc);
        (void)hipEventDestroy(e->ev2);
    }
    for (auto& b : e->pin) {
        if (b.p) (void)hipHostFree(b.p);
        if (b.ev) (void)hipEventDestroy(b.ev);
    }
    delete e;
}

const char* mt_engine_last_error(const mt_engine* e) { return e ? e->err.c_str() : "null engine"; }
int64_t mt_engine_ndocs(const mt_engine* e) { return e ? e->ndocs : 0; }
void* mt_engine_stream(const mt_engine* e) { return e ? (void*)e->stream : nullptr; }
float mt_engine_last_run_ms(const mt_engine* e) { return e ? e->last_ms : 0.f; }

int32_t mt_engine_start_collab(mt_engine* e, const int32_t* local_long_ids, int32_t min_seq, int32_t cur_seq) {
    if (!e || !local_long_ids) return MT_E_ARG;
    std::vector<int32_t> mins((size_t)e->ndocs, min_seq), curs((size_t)e->ndocs, cur_seq);
    return mt_engine_start_collab_docs(e, local_long_ids, mins.data(), curs.data());
}

int32_t mt_engine_start_collab_docs(mt_engine* e, const int32_t* local_long_ids, const int32_t* min_seqs,
                                    const int32_t* cur_seqs) {
    if (!e || !local_long_ids || !min_seqs || !cur_seqs) return MT_E_ARG;
    int64_t nd = e->ndocs;
    HIPCHK(e, hipSetDevice(e->device));
    e->h_local.assign(local_long_ids, local_long_ids + nd);
    e->h_local.insert(e->h_local.end(), min_seqs, min_seqs + nd);
    e->h_local.insert(e->h_local.end(), cur_seqs, cur_seqs + nd);
    int32_t rc = ensure(e, e->local_ids, sizeof(int32_t) * 3 * nd);
    if (rc) return rc;
    HIPCHK(e, hipMemcpyAsync(e->local_ids.p, e->h_local.data(), sizeof(int32_t) * 3 * nd, hipMemcpyHostToDevice,
                             e->stream));
    e->collab = true;
    rc = e->ops->start_collab(e);
    if (rc) return rc;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (e->over && !e->pro_docs.empty()) { /* promoted documents live in `over` */
        size_t m = e->pro_docs.size();
        std::vector<int32_t> ids(m), mn(m), cu(m);
        for (size_t i = 0; i < m; i++) {
            int64_t d = e->pro_docs[i];
            ids[i] = local_long_ids[d];
            mn[i] = min_seqs[d];
            cu[i] = cur_seqs[d];
        }
        return mt_engine_start_collab_docs(e->over, ids.data(), mn.data(), cu.data());
    }
    return MT_OK;
}

int32_t mt_engine_submit(mt_engine* e, const mt_op_rec* ops, const int64_t* op_off, const uint16_t* text,
                         int64_t text_units, const int64_t* text_off, const mt_props_rec* props, int64_t nprops,
                         const int64_t* props_off, const mt_kv* kv, int64_t nkv, const int64_t* kv_off) {
    if (!e) return MT_E_ARG;
    return submit(e, {ops, op_off, text, text_units, text_off, props, nprops, props_off, kv, nkv, kv_off}, -1, nullptr);
}

int32_t mt_engine_submit_docs(mt_engine* e, int64_t m, const int64_t* docs, const mt_op_rec* ops, const int64_t* op_off,
                              const uint16_t* text, int64_t text_units, const int64_t* text_off,
                              const mt_props_rec* props, int64_t nprops, const int64_t* props_off, const mt_kv* kv,
                              int64_t nkv, const int64_t* kv_off) {
    if (!e || m < 0 || m > e->ndocs || (m && !docs)) return MT_E_ARG;
    for (int64_t k = 0; k < m; k++)
        if (docs[k] < 0 || docs[k] >= e->ndocs || (k && docs[k] <= docs[k - 1])) return MT_E_ARG; /* increasing ids */
    return submit(e, {ops, op_off, text, text_units, text_off, props, nprops, props_off, kv, nkv, kv_off}, m, docs);
}

int32_t mt_host_alloc(int64_t bytes, void** out) {
    if (!out || bytes < 0) return MT_E_ARG;
    *out = nullptr;
    if (hipHostMalloc(out, (size_t)std::max<int64_t>(bytes, 16), hipHostMallocDefault) != hipSuccess) {
        *out = nullptr;
        return MT_E_NOMEM;
    }
    return MT_OK;
}
void mt_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

int32_t mt_engine_reset(mt_engine* e) {
    if (!e) return MT_E_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    std::fill(e->pro.begin(), e->pro.end(), -1);
    e->pro_docs.clear();
    e->fresh = true;
    return e->ops->init(e);
}

static int32_t stage_subset(mt_engine* e, mt_engine* o);

static int32_t after_launch(mt_engine* e);

int32_t mt_engine_run(mt_engine* e) {
    if (!e || !e->staged) return MT_E_ARG;
    HIPCHK(e, hipSetDevice(e->device));
#ifdef MT_PROF
    if (ensure(e, e->prof, sizeof(uint64_t) * PH_N * e->ndocs)) return MT_E_NOMEM;
#endif
    HIPCHK(e, hipEventRecord(e->ev0, e->stream));
    int32_t rc = e->ops->replay(e);
    if (rc) return rc;
    HIPCHK(e, hipEventRecord(e->ev1, e->stream));
    return after_launch(e);
}

/* documents per chunk of mt_engine_submit_run: an eighth of the batch, but never fewer than the documents the GPU
 * holds at once (a chunk's launch must fill the machine by itself; config 4's 256 documents stay one launch) */
static int64_t chunk_docs(const mt_engine* e) {
    if (e->chunk > 0) return e->chunk;
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, e->device) != hipSuccess || ncu < 1) ncu = 256;
    int64_t resident = e->profile == P_HUGE                       ? ncu
                       : e->profile == P_SMALL && e->waves == 1 ? (int64_t)ncu * 3 /* the LDS-image build */
                                                                : (int64_t)ncu * 4 * (e->profile == P_SMALL ? e->waves : 7);
    return std::max<int64_t>(resident, (e->ndocs + 7) / 8);
}

int32_t mt_engine_submit_run(mt_engine* e, const mt_op_rec* ops, const int64_t* op_off, const uint16_t* text,
                             int64_t text_units, const int64_t* text_off, const mt_props_rec* props, int64_t nprops,
                             const int64_t* props_off, const mt_kv* kv, int64_t nkv, const int64_t* kv_off) {
    if (!e) return MT_E_ARG;
    const SubmitArgs a{ops, op_off, text, text_units, text_off, props, nprops, props_off, kv, nkv, kv_off};
    if (!offsets_ok(a, e->ndocs)) return MT_E_ARG;
    const int64_t nd = e->ndocs;
    HIPCHK(e, hipSetDevice(e->device));
    int32_t rc;
    if ((rc = ensure_staging(e, a))) return rc;
#ifdef MT_PROF
    if (ensure(e, e->prof, sizeof(uint64_t) * PH_N * e->ndocs)) return MT_E_NOMEM;
#endif
    if (!e->cstream) {
        HIPCHK(e, hipStreamCreateWithFlags(&e->cstream, hipStreamNonBlocking));
        HIPCHK(e, hipStreamCreateWithFlags(&e->stream2, hipStreamNonBlocking));
        HIPCHK(e, hipEventCreateWithFlags(&e->evs, hipEventDisableTiming));
        HIPCHK(e, hipEventCreateWithFlags(&e->evc, hipEventDisableTiming));
        HIPCHK(e, hipEventCreateWithFlags(&e->ev2, hipEventDisableTiming));
    }
    e->staged = false;
    e->nsub = -1;
    e->h_sub.clear();
    /* everything queued on the engine stream so far (a reset, the last replay reading the buffers about to be
     * overwritten) comes first, for the copies and both compute streams */
    HIPCHK(e, hipEventRecord(e->evs, e->stream));
    HIPCHK(e, hipStreamWaitEvent(e->cstream, e->evs, 0));
    HIPCHK(e, hipStreamWaitEvent(e->stream2, e->evs, 0));
    HIPCHK(e, hipEventRecord(e->ev0, e->stream));
    if ((rc = copy_small(e, a, e->cstream))) return rc;
    const int64_t step = e->order.p ? nd : chunk_docs(e); /* a dispatch order permutes across chunks: one launch */
    /* one chunk leaves nothing to overlap: the runtime's own pageable copy then beats the staging buffers (8,192
     * documents: 66 vs 105 ms, profiles/r06z_c3_share0of8_8192docs_bench.json) */
    const bool single = step >= nd;
    const bool pin_ops = single || host_pinned(ops), pin_text = single || host_pinned(text);
    std::vector<mt_engine::Persp> persp((size_t)nd);
    std::vector<char> loads((size_t)nd, 0);
    seed_segk(e, persp, nullptr);
    int64_t text_hi = 0; /* the text staged so far: a prefix of the pool */
    int k = 0;
    rc = MT_OK;
    /* the first chunks ramp up (a quarter, then half a chunk): the replay starts once a quarter of the first chunk is
     * copied instead of all of it, and the later, full chunks overlap the copies as before */
    static const int ramp_env = getenv("MT_SUBMIT_RAMP") ? atoi(getenv("MT_SUBMIT_RAMP")) : 1;
    const bool ramp = ramp_env != 0 && !single && e->chunk <= 0;
    int64_t len = step;
    for (int64_t d0 = 0; d0 < nd; d0 += len, k++) {
        len = ramp && k < 2 ? std::max<int64_t>(1, step >> (2 - k)) : step;
        const int64_t d1 = std::min(nd, d0 + len);
        int64_t te = 0;
        if (!check_range(a, d0, d1, persp.data(), loads.data(), &te)) {
            rc = MT_E_ARG;
            break;
        }
        if (te > text_hi) {
            if ((rc = stage_h2d(e, (uint16_t*)e->text.p + text_hi, text + text_hi, 2 * (size_t)(te - text_hi), pin_text)))
                break;
            text_hi = te;
        }
        if ((rc = stage_h2d(e, (mt_op_rec*)e->ops_buf.p + op_off[d0], ops + op_off[d0],
                            sizeof(mt_op_rec) * (size_t)(op_off[d1] - op_off[d0]), pin_ops)))
            break;
        HIPCHK(e, hipEventRecord(e->evc, e->cstream));
        hipStream_t s = (k & 1) ? e->stream2 : e->stream;
        HIPCHK(e, hipStreamWaitEvent(s, e->evc, 0));
        e->loads = std::find(loads.begin() + d0, loads.begin() + d1, 1) != loads.begin() + d1;
        e->run_d0 = d0, e->run_n = d1 - d0, e->run_stream = s;
        rc = e->ops->replay(e);
        e->run_d0 = 0, e->run_n = -1, e->run_stream = nullptr;
        if (rc) break;
    }
    /* the second compute stream joins the engine stream; the caller's buffers are free once the copies are done */
    HIPCHK(e, hipEventRecord(e->ev2, e->stream2));
    HIPCHK(e, hipStreamWaitEvent(e->stream, e->ev2, 0));
    HIPCHK(e, hipEventRecord(e->ev1, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->cstream));
    if (rc) {
        (void)hipStreamSynchronize(e->stream); /* the chunks launched before the failure have replayed */
        return rc;
    }
    keep_staged(e, a, persp, loads);
    return after_launch(e);
}

/* the bookkeeping after a replay launch (mt_engine_run, mt_engine_submit_run) */
static int32_t after_launch(mt_engine* e) {
    int32_t rc;
    e->ran = true;
    e->ran_fresh = e->fresh;
    if (e->fresh) e->persp_applied.assign((size_t)e->ndocs, mt_engine::Persp());
    for (size_t k = 0; k < e->persp_staged.size(); k++) {
        size_t d = e->nsub >= 0 ? (size_t)e->h_sub[k] : k;
        if (d < e->persp_applied.size()) e->persp_applied[d].merge(e->persp_staged[k]);
    }
    e->fresh = false;
    e->forwarded = false;
    /* documents promoted by an earlier replay of this replica history live on in `over`: their parent
     * replicas stay latched (E_CAPACITY, every later record a no-op), so this batch's records for them
     * replay there, on top of the state they already hold (no reset) */
    if (e->over && !e->pro_docs.empty()) {
        if ((rc = stage_subset(e, e->over))) return rc;
        if ((rc = mt_engine_run(e->over))) return rc;
        e->forwarded = true;
    }
    return MT_OK;
}

static int32_t promote(mt_engine* e);

int32_t mt_engine_sync(mt_engine* e) {
    if (!e) return MT_E_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e->ev0, e->ev1) == hipSuccess) e->last_ms = ms;
    if (e->ran) {
        e->ran = false;
        int32_t rc;
        if (e->forwarded) {
            e->forwarded = false;
            if ((rc = mt_engine_sync(e->over))) return rc;
            e->last_ms += e->over->last_ms;
        } else if (e->promote && e->ran_fresh) {
            /* only a replay that started from create / reset holds each replica's whole history in the staged
             * log; a document that overflows in a later incremental batch keeps E_CAPACITY visible */
            if ((rc = promote(e))) return rc;
            if (e->over && !e->pro_docs.empty()) e->last_ms += e->over->last_ms;
        }
    }
    return MT_OK;
}

static int32_t read_hdr(mt_engine* e, int32_t* err, int32_t* err_op, int32_t* stats4, int64_t* work3,
                        int64_t* times2 = nullptr) {
    HIPCHK(e, hipSetDevice(e->device));
    int64_t n = e->ndocs;
    int32_t rc = ensure(e, e->tmp, (size_t)n * (4 + 4 + 16 + 24 + 16));
    if (rc) return rc;
    int32_t* de = (int32_t*)e->tmp.p;
    int32_t* deo = de + n;
    int32_t* ds = deo + n;
    int64_t* dw = (int64_t*)(ds + 4 * n);
    int64_t* dt = dw + 3 * n;
    rc = e->ops->hdr(e, de, deo, ds, dw, times2 ? dt : nullptr);
    if (rc) return rc;
    if (err) HIPCHK(e, hipMemcpyAsync(err, de, 4 * n, hipMemcpyDeviceToHost, e->stream));
    if (err_op) HIPCHK(e, hipMemcpyAsync(err_op, deo, 4 * n, hipMemcpyDeviceToHost, e->stream));
    if (stats4) HIPCHK(e, hipMemcpyAsync(stats4, ds, 16 * n, hipMemcpyDeviceToHost, e->stream));
    if (work3) HIPCHK(e, hipMemcpyAsync(work3, dw, 24 * n, hipMemcpyDeviceToHost, e->stream));
    if (times2) HIPCHK(e, hipMemcpyAsync(times2, dt, 16 * n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return MT_OK;
}

/* ---- capacity promotion ------------------------------------------------------------------------
 * A document whose replay latched E_CAPACITY (row slots, nodes, heap, key slots, text arena, membership
 * log, pending groups) replays again from its staged log, from an empty replica, in an engine of the
 * next profile: small / config-5 -> HotMid (2,048 nodes, 24 key slots) -> HotBig (16,384) -> HotHuge
 * (262,144, tiled), with four times the arena, membership and pending-group capacities. The promoted
 * documents' records are gathered on the device; their text / props / kv pools stay the parent's. */
static int32_t next_ncap(const mt_engine* e) {
    switch (e->profile) {
    case P_SMALL: case P_MAT: return HotMid::N;
    case P_MID: return HotBig::N;
    case P_BIG: return HotHuge::N;
    case P_HUGE: return e->fx || e->wide ? -1 : HotHuge::N; /* the tiled kernel's LDS heap -> its wide variant */
    default: return -1;
    }
}
/* the staged entry holding document d's records (-1: none staged for it) */
static int64_t staged_entry(const mt_engine* e, int64_t d) {
    if (e->nsub < 0) return d;
    auto it = std::lower_bound(e->h_sub.begin(), e->h_sub.end(), d);
    return it != e->h_sub.end() && *it == d ? (int64_t)(it - e->h_sub.begin()) : -1;
}
/* stage, in `o`, the records `e` has staged for its promoted documents (e->pro_docs, in order), gathered
 * device to device; their text / props / kv pools stay the parent's */
static int32_t stage_subset(mt_engine* e, mt_engine* o) {
    int64_t m = (int64_t)e->pro_docs.size();
    int32_t rc;
    o->h_op_off.assign((size_t)m + 1, 0);
    o->h_text_off.resize((size_t)m);
    o->h_props_off.resize((size_t)m);
    o->h_kv_off.resize((size_t)m);
    o->nsub = -1;
    std::vector<int64_t> src((size_t)m);
    for (int64_t i = 0; i < m; i++) {
        int64_t k = staged_entry(e, e->pro_docs[(size_t)i]);
        src[(size_t)i] = k;
        int64_t n = k < 0 ? 0 : e->h_op_off[(size_t)k + 1] - e->h_op_off[(size_t)k];
        o->h_op_off[(size_t)i + 1] = o->h_op_off[(size_t)i] + n;
        o->h_text_off[(size_t)i] = k < 0 ? 0 : e->h_text_off[(size_t)k];
        o->h_props_off[(size_t)i] = k < 0 ? 0 : e->h_props_off[(size_t)k];
        o->h_kv_off[(size_t)i] = k < 0 ? 0 : e->h_kv_off[(size_t)k];
    }
    if ((rc = ensure(o, o->ops_buf, sizeof(mt_op_rec) * o->h_op_off[(size_t)m]))) return rc;
    if ((rc = ensure(o, o->op_off, sizeof(int64_t) * (m + 1)))) return rc;
    if ((rc = ensure(o, o->text_off, sizeof(int64_t) * m))) return rc;
    if ((rc = ensure(o, o->props_off, sizeof(int64_t) * m))) return rc;
    if ((rc = ensure(o, o->kv_off, sizeof(int64_t) * m))) return rc;
    for (int64_t i = 0; i < m; i++) {
        int64_t k = src[(size_t)i], n = o->h_op_off[(size_t)i + 1] - o->h_op_off[(size_t)i];
        if (n)
            HIPCHK(o, hipMemcpyAsync((mt_op_rec*)o->ops_buf.p + o->h_op_off[(size_t)i],
                                     (const mt_op_rec*)e->ops_buf.p + e->h_op_off[(size_t)k], sizeof(mt_op_rec) * n,
                                     hipMemcpyDeviceToDevice, o->stream));
    }
    HIPCHK(o, hipMemcpyAsync(o->op_off.p, o->h_op_off.data(), sizeof(int64_t) * (m + 1), hipMemcpyHostToDevice, o->stream));
    HIPCHK(o, hipMemcpyAsync(o->text_off.p, o->h_text_off.data(), sizeof(int64_t) * m, hipMemcpyHostToDevice, o->stream));
    HIPCHK(o, hipMemcpyAsync(o->props_off.p, o->h_props_off.data(), sizeof(int64_t) * m, hipMemcpyHostToDevice, o->stream));
    HIPCHK(o, hipMemcpyAsync(o->kv_off.p, o->h_kv_off.data(), sizeof(int64_t) * m, hipMemcpyHostToDevice, o->stream));
    o->borrowed = true;
    o->text = e->text;
    o->props = e->props;
    o->kv = e->kv;
    o->staged = true;
    return MT_OK;
}
static int32_t promote(mt_engine* e) {
    std::fill(e->pro.begin(), e->pro.end(), -1);
    e->pro_docs.clear();
    int32_t nc = next_ncap(e);
    if (nc < 0) return MT_OK;
    int64_t nd = e->ndocs;
    std::vector<int32_t> err((size_t)nd);
    int32_t rc = read_hdr(e, err.data(), nullptr, nullptr, nullptr);
    if (rc) return rc;
    for (int64_t d = 0; d < nd; d++)
        if (err[(size_t)d] == MT_E_CAPACITY) e->pro_docs.push_back(d);
    int64_t m = (int64_t)e->pro_docs.size();
    if (m == 0) return MT_OK;
    mt_caps c = e->caps0;
    c.ncap = nc;
    c.hcap = std::max(c.hcap, 2 * nc);
    c.acap = (int32_t)std::min<int64_t>(4 * (int64_t)c.acap, 1 << 23);
    c.mcap = (int32_t)std::min<int64_t>(4 * (int64_t)c.mcap, 1 << 18);
    c.gcap = (int32_t)std::min<int64_t>(4 * (int64_t)c.gcap, 1 << 16);
    /* the client-feature capacities grow too (delta-log words, references, PermutationVector handles),
     * so a document that overflowed one of them is not replayed again into the same limit */
    c.dcap = (int32_t)std::min<int64_t>(4 * (int64_t)c.dcap, 1 << 26);
    c.rcap = (int32_t)std::min<int64_t>(4 * (int64_t)c.rcap, 1 << 16);
    c.pcap = (int32_t)std::min<int64_t>(4 * (int64_t)c.pcap, 1 << 24);
    mt_engine* o = e->over;
    if (o && (o->ndocs != m || o->caps0.ncap != c.ncap)) {
        mt_engine_destroy(o);
        o = e->over = nullptr;
    }
    if (!o) {
        rc = mt_engine_create(e->device, m, &c, &o);
        if (rc) return rc;
        e->over = o;
    }
    o->promote = e->promote;
    o->wide = e->profile == P_HUGE; /* HotHuge -> HotHuge: the same layout, the wide kernel */
    if (e->nvk && (rc = mt_engine_set_value_kinds(o, e->h_vkind.data(), e->nvk))) return rc;
    if (e->collab) {
        std::vector<int32_t> loc((size_t)(3 * m)); /* the promoted documents' ids, minSeqs, currentSeqs */
        for (int64_t i = 0; i < m; i++)
            for (int64_t k = 0; k < 3; k++)
                loc[(size_t)(k * m + i)] = e->h_local[(size_t)(k * nd + e->pro_docs[(size_t)i])];
        HIPCHK(o, hipSetDevice(o->device));
        if ((rc = ensure(o, o->local_ids, sizeof(int32_t) * 3 * m))) return rc;
        HIPCHK(o, hipMemcpyAsync(o->local_ids.p, loc.data(), sizeof(int32_t) * 3 * m, hipMemcpyHostToDevice, o->stream));
        HIPCHK(o, hipStreamSynchronize(o->stream));
        o->h_local = loc;
        o->collab = true;
    }
    if ((rc = stage_subset(e, o))) return rc;
    /* an empty replica (create / reset state), the same local ids; then the replay, promoting further */
    if ((rc = mt_engine_reset(o))) return rc;
    if ((rc = mt_engine_run(o))) return rc;
    if ((rc = mt_engine_sync(o))) return rc;
    for (int64_t i = 0; i < m; i++) e->pro[(size_t)e->pro_docs[(size_t)i]] = (int32_t)i;
    return MT_OK;
}
/* the perspective floor of (doc, long client) for the reads (mt_kernels.h persp_refused) */
static int32_t persp_floor(const mt_engine* e, int64_t doc, int32_t long_client) {
    if (long_client < 0 || (size_t)doc >= e->persp_applied.size()) return INT32_MIN;
    return e->persp_applied[(size_t)doc].floor(long_client);
}
/* the engine and index that hold document `doc` (promoted documents live in `over`) */
static mt_engine* route(mt_engine* e, int64_t* doc) {
    while (e && e->over && *doc >= 0 && *doc < e->ndocs && e->pro[(size_t)*doc] >= 0) {
        *doc = e->pro[(size_t)*doc];
        e = e->over;
    }
    return e;
}
static bool promoted(const mt_engine* e) { return e->over && !e->pro_docs.empty(); }

/* The second half of every whole-batch read. `out` holds `row` entries per document, just read from e's own store;
 * the rows of e's promoted documents are read again from `over` (read_child(over, tmp): its rows are `crow` entries
 * long, and the call goes on through over's own promotions) and put back over them. A row keeps the first
 * min(row, crow) entries of its child row. out == nullptr (an output the caller did not ask for): the child is read
 * with nullptr. A read with two outputs nests two calls, so that one read of the child fills both temporaries. */
extern "C++" {
template <class T, class F>
static int32_t read_promoted(mt_engine* e, T* out, size_t row, size_t crow, F&& read_child) {
    if (!promoted(e)) return MT_OK;
    const size_t m = e->pro_docs.size();
    std::vector<T> tmp(out ? m * crow : 0);
    int32_t rc = read_child(e->over, out ? tmp.data() : nullptr);
    if (rc || !out) return rc;
    for (size_t i = 0; i < m; i++)
        std::copy_n(tmp.data() + i * crow, std::min(row, crow), out + (size_t)e->pro_docs[i] * row);
    return MT_OK;
}

/* The second half of every variable-length read of one document: fetch what the device holds at `dhdr`, wait, take
 * the count n = count(header), copy min(n, cap) elements of `unit` bytes from `dsrc` to `out` (`whole`: all n, or
 * none if they do not fit), wait. out == nullptr: the size query. Returns n, or the negated MT_E_* code. */
template <class H, class N>
static int64_t read_counted(mt_engine* e, const H* dhdr, N&& count, const void* dsrc, size_t unit, void* out,
                            int64_t cap, bool whole = false) {
    H hdr;
    if (hipMemcpyAsync(&hdr, dhdr, sizeof hdr, hipMemcpyDeviceToHost, e->stream) != hipSuccess) return -MT_E_HIP;
    if (hipStreamSynchronize(e->stream) != hipSuccess) return -MT_E_HIP;
    const int64_t n = count(hdr);
    const int64_t m = n <= cap ? n : whole ? 0 : cap;
    if (out && m > 0) {
        if (hipMemcpyAsync(out, dsrc, unit * (size_t)m, hipMemcpyDeviceToHost, e->stream) != hipSuccess)
            return -MT_E_HIP;
        if (hipStreamSynchronize(e->stream) != hipSuccess) return -MT_E_HIP;
    }
    return n;
}
}
static int64_t whole_count(int64_t n) { return n; } /* read_counted's `count` where the device wrote the count itself */

int32_t mt_engine_errors(mt_engine* e, int32_t* err, int32_t* err_op) {
    if (!e) return MT_E_ARG;
    int32_t rc = read_hdr(e, err, err_op, nullptr, nullptr);
    if (rc) return rc;
    return read_promoted(e, err, 1, 1, [&](mt_engine* o, int32_t* a) {
        return read_promoted(e, err_op, 1, 1, [&](mt_engine*, int32_t* b) { return mt_engine_errors(o, a, b); });
    });
}
int32_t mt_engine_stats(mt_engine* e, int32_t* out4) {
    if (!e || !out4) return MT_E_ARG;
    int32_t rc = read_hdr(e, nullptr, nullptr, out4, nullptr);
    return rc ? rc : read_promoted(e, out4, 4, 4, mt_engine_stats);
}
int32_t mt_engine_doc_times(mt_engine* e, int64_t* out2) {
    if (!e || !out2) return MT_E_ARG;
    int32_t rc = read_hdr(e, nullptr, nullptr, nullptr, nullptr, out2);
    return rc ? rc : read_promoted(e, out2, 2, 2, mt_engine_doc_times);
}

int32_t mt_engine_set_order(mt_engine* e, const int32_t* order) {
    if (!e) return MT_E_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    if (!order) {
        if (e->order.p) (void)hipFree(e->order.p);
        e->order = DevBuf();
        return MT_OK;
    }
    std::vector<char> seen((size_t)e->ndocs, 0);
    for (int64_t i = 0; i < e->ndocs; i++) {
        if (order[i] < 0 || order[i] >= e->ndocs || seen[(size_t)order[i]]) return MT_E_ARG; /* a permutation */
        seen[(size_t)order[i]] = 1;
    }
    if (ensure(e, e->order, sizeof(int32_t) * e->ndocs)) return MT_E_NOMEM;
    HIPCHK(e, hipMemcpyAsync(e->order.p, order, sizeof(int32_t) * e->ndocs, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return MT_OK;
}

int32_t mt_engine_set_value_kinds(mt_engine* e, const uint8_t* kinds, int32_t n) {
    if (!e || n < 0 || (n && !kinds) || n > MT_VALUE_DERIVED) return MT_E_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    int32_t rc = ensure(e, e->vkind, (size_t)std::max(n, 1));
    if (rc) return rc;
    e->h_vkind.assign(kinds, kinds + n);
    if (n) HIPCHK(e, hipMemcpyAsync(e->vkind.p, kinds, (size_t)n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->nvk = n;
    if (e->over) return mt_engine_set_value_kinds(e->over, kinds, n); /* promoted documents replay there */
    return MT_OK;
}

int32_t mt_engine_set_variant(mt_engine* e, int32_t key, int32_t value) {
    if (!e) return MT_E_ARG;
    switch (key) {
    case MT_VAR_SMALL_WAVES:
        if (value != 1 && value != 4 && value != 8) return MT_E_ARG;
        e->waves = value;
        return MT_OK;
    case MT_VAR_TILED_WIDE:
        if (value != 0 && value != 1) return MT_E_ARG;
        e->wide = value == 1;
        return MT_OK;
    case MT_VAR_CHUNK_DOCS:
        if (value < 0) return MT_E_ARG;
        e->chunk = value;
        return MT_OK;
    case MT_VAR_TEXTS_PACKED:
        if (value != 0 && value != 1) return MT_E_ARG;
        e->texts_packed = value == 1;
        return MT_OK;
    case MT_VAR_DUMPS_PARALLEL:
        if (value != 0 && value != 1) return MT_E_ARG;
        e->dumps_parallel = value == 1;
        return MT_OK;
    case MT_VAR_SUMMARIES_PARALLEL:
        if (value != 0 && value != 1) return MT_E_ARG;
        e->summaries_parallel = value == 1;
        return MT_OK;
    case MT_VAR_TILES_PARALLEL:
        if (value != 0 && value != 1) return MT_E_ARG;
        e->tiles_parallel = value == 1;
        return MT_OK;
    case MT_VAR_HANDLES_PARALLEL:
        if (value != 0 && value != 1) return MT_E_ARG;
        e->handles_parallel = value == 1;
        return MT_OK;
    case MT_VAR_DELTAS_PARALLEL:
        if (value != 0 && value != 1) return MT_E_ARG;
        e->deltas_parallel = value == 1;
        return MT_OK;
    default:
        return MT_E_ARG;
    }
}

int32_t mt_engine_work(mt_engine* e, int64_t* out3) {
    if (!e || !out3) return MT_E_ARG;
    int32_t rc = read_hdr(e, nullptr, nullptr, nullptr, out3);
    return rc ? rc : read_promoted(e, out3, 3, 3, mt_engine_work);
}
int64_t mt_engine_promoted(const mt_engine* e, int64_t* docs_out, int64_t cap) {
    if (!e) return -MT_E_ARG;
    int64_t m = promoted(e) ? (int64_t)e->pro_docs.size() : 0;
    for (int64_t i = 0; i < m && i < cap && docs_out; i++) docs_out[i] = e->pro_docs[(size_t)i];
    return m;
}

int32_t mt_engine_digests(mt_engine* e, uint64_t* out) {
    if (!e || !out) return MT_E_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    int32_t rc = ensure(e, e->tmp, sizeof(uint64_t) * e->ndocs);
    if (rc) return rc;
    rc = e->ops->digest(e, (uint64_t*)e->tmp.p);
    if (rc) return rc;
    HIPCHK(e, hipMemcpyAsync(out, e->tmp.p, sizeof(uint64_t) * e->ndocs, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return read_promoted(e, out, 1, 1, mt_engine_digests);
}

int64_t mt_engine_dump(mt_engine* e, int64_t doc, uint8_t* out, int64_t cap) {
    if (!e || doc < 0 || doc >= e->ndocs || cap < 0) return -MT_E_ARG;
    e = route(e, &doc);
    if (hipSetDevice(e->device) != hipSuccess) return -MT_E_HIP;
    size_t need = sizeof(int64_t) + (size_t)(out ? cap : 0) + 16;
    if (ensure(e, e->tmp, need)) return -MT_E_HIP;
    int64_t* dn = (int64_t*)e->tmp.p;
    uint8_t* dbuf = out ? (uint8_t*)e->tmp.p + 16 : nullptr;
    int32_t rc = e->ops->dump(e, doc, dbuf, out ? cap : 0, dn);
    if (rc) return -rc;
    return read_counted(e, dn, whole_count, dbuf, 1, out, cap, true); /* all n bytes or none */
}

int32_t mt_engine_get_length(mt_engine* e, int64_t doc, int32_t ref_seq, int32_t long_client, int32_t* out) {
    if (!e || !out || doc < 0 || doc >= e->ndocs) return MT_E_ARG;
    int32_t floor = persp_floor(e, doc, long_client);
    e = route(e, &doc);
    HIPCHK(e, hipSetDevice(e->device));
    int32_t rc = ensure(e, e->tmp, 16);
    if (rc) return rc;
    rc = e->ops->length(e, doc, ref_seq, long_client, floor, (int32_t*)e->tmp.p);
    if (rc) return rc;
    int32_t r2[2];
    HIPCHK(e, hipMemcpyAsync(r2, e->tmp.p, sizeof(r2), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (r2[1]) return MT_E_UNSUPPORTED; /* a perspective the reference's partial lengths answer differently */
    *out = r2[0];
    return MT_OK;
}

int64_t mt_engine_get_text(mt_engine* e, int64_t doc, int32_t ref_seq, int32_t long_client, uint16_t* out,
                           int64_t cap) {
    return mt_engine_get_text_range(e, doc, ref_seq, long_client, nullptr, 0, MT_TEXT_DEFAULT, MT_TEXT_DEFAULT, out,
                                    cap);
}

static int64_t text_read(mt_engine* e, int64_t doc, int32_t ref_seq, int32_t long_client, const uint16_t* placeholder,
                         int32_t placeholder_len, int32_t start, int32_t end, uint16_t* out, int64_t cap);

int64_t mt_engine_get_text_range(mt_engine* e, int64_t doc, int32_t ref_seq, int32_t long_client,
                                 const uint16_t* placeholder, int32_t placeholder_len, int32_t start, int32_t end,
                                 uint16_t* out, int64_t cap) {
    if (!e || doc < 0 || doc >= e->ndocs || cap < 0 || placeholder_len < 0 || placeholder_len > 4096 ||
        (placeholder_len > 0 && !placeholder))
        return -MT_E_ARG;
    if (placeholder_len == 1 && placeholder[0] == '*') return -MT_E_UNSUPPORTED; /* Marker.toString() */
    return text_read(e, doc, ref_seq, long_client, placeholder, placeholder_len, start, end, out, cap);
}

int64_t mt_engine_get_items(mt_engine* e, int64_t doc, int32_t start, int32_t end, uint16_t* out, int64_t cap) {
    if (!e || doc < 0 || doc >= e->ndocs || cap < 0 || start == MT_TEXT_DEFAULT) return -MT_E_ARG;
    return text_read(e, doc, 0, -1, nullptr, -1, start, end, out, cap); /* placeholder length -1: k_text's items mode */
}

static int64_t text_read(mt_engine* e, int64_t doc, int32_t ref_seq, int32_t long_client, const uint16_t* placeholder,
                         int32_t placeholder_len, int32_t start, int32_t end, uint16_t* out, int64_t cap) {
    int32_t floor = persp_floor(e, doc, long_client);
    e = route(e, &doc);
    if (hipSetDevice(e->device) != hipSuccess) return -MT_E_HIP;
    size_t phb = (2 * (size_t)(placeholder_len > 0 ? placeholder_len : 0) + 15) & ~(size_t)15;
    if (ensure(e, e->tmp, 16 + phb + 2 * (size_t)(out ? cap : 0) + 16)) return -MT_E_HIP;
    int64_t* dn = (int64_t*)e->tmp.p;
    uint16_t* dph = (uint16_t*)((uint8_t*)e->tmp.p + 16);
    uint16_t* dbuf = out ? (uint16_t*)((uint8_t*)e->tmp.p + 16 + phb) : nullptr;
    if (placeholder_len > 0 &&
        hipMemcpyAsync(dph, placeholder, 2 * (size_t)placeholder_len, hipMemcpyHostToDevice, e->stream) != hipSuccess)
        return -MT_E_HIP;
    int32_t rc = e->ops->text(e, doc, ref_seq, long_client, floor, start, end, dph, placeholder_len, dbuf,
                              out ? cap : 0, dn);
    if (rc) return -rc;
    return read_counted(e, dn, whole_count, dbuf, 2, out, cap);
}

static void seg_ref_of(const int32_t* r, mt_seg_ref* out) {
    out->rid = r[0] == 1 ? r[1] : -1;
    out->gen = r[2];
    out->offset = r[3];
    out->length = r[4];
    out->seq = r[5];
    out->client = r[6];
    out->removed_seq = r[7];
    out->removed_client = r[8];
    out->ordinal = r[9];
}
static int32_t seg_query(mt_engine* e, int64_t doc, int32_t mode, int32_t a, int32_t b, int32_t ref_seq,
                         int32_t long_client, int32_t* res7) { /* res7: MT_SEGQ_N words (mt_kernels.h k_seg) */
    if (!e || doc < 0 || doc >= e->ndocs) return MT_E_ARG;
    int32_t floor = persp_floor(e, doc, long_client);
    e = route(e, &doc);
    HIPCHK(e, hipSetDevice(e->device));
    int32_t rc = ensure(e, e->tmp, 64);
    if (rc) return rc;
    rc = e->ops->seg(e, doc, mode, a, b, ref_seq, long_client, floor, (int32_t*)e->tmp.p);
    if (rc) return rc;
    HIPCHK(e, hipMemcpyAsync(res7, e->tmp.p, MT_SEGQ_N * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (res7[0] == 3) return MT_E_UNSUPPORTED; /* a perspective the reference's partial lengths answer differently */
    return MT_OK;
}

int32_t mt_engine_get_containing_segment(mt_engine* e, int64_t doc, int32_t pos, int32_t ref_seq, int32_t long_client,
                                         mt_seg_ref* out) {
    if (!out) return MT_E_ARG;
    int32_t r[MT_SEGQ_N];
    int32_t rc = seg_query(e, doc, 0, pos, 0, ref_seq, long_client, r);
    if (rc) return rc;
    seg_ref_of(r, out);
    return MT_OK;
}

int32_t mt_engine_get_position(mt_engine* e, int64_t doc, int32_t rid, int32_t gen, int32_t ref_seq,
                               int32_t long_client, int32_t* out) {
    if (!out) return MT_E_ARG;
    int32_t r[MT_SEGQ_N];
    int32_t rc = seg_query(e, doc, 1, rid, gen, ref_seq, long_client, r);
    if (rc) return rc;
    if (!r[0]) return MT_E_ARG;
    *out = r[1];
    return MT_OK;
}

int32_t mt_engine_pos_from_relative_pos(mt_engine* e, int64_t doc, int32_t id_key, int32_t id_value, int32_t before,
                                        int32_t has_offset, int32_t offset, int32_t ref_seq, int32_t long_client,
                                        int32_t* out) {
    if (!out) return MT_E_ARG;
    int32_t r[MT_SEGQ_N];
    int32_t rc = seg_query(e, doc, 2, id_key, id_value, ref_seq, long_client, r);
    if (rc) return rc;
    if (r[0] == 2) return MT_E_UNSUPPORTED; /* several markers hold the id */
    int32_t pos = -1;
    if (r[0] == 1) { /* mergeTree.ts:1986-1996: a marker's cachedLength is 1 */
        pos = r[1];
        if (!before) pos += 1 + (has_offset ? offset : 0);
        else if (has_offset) pos -= offset;
    }
    *out = pos;
    return MT_OK;
}

/* what k_seg's mode 4 found for `pos` (r: its MT_SEGQ_N words), as resolveRemoteClientPosition (the segment's local
 * position + offset, the local length when pos is the remote client's length, else -1) or as adjustPosition (a
 * segment that exists and is not removed, else -1) */
static int32_t remote_pos(const int32_t* r, int32_t pos, bool adjust) {
    if (adjust) return r[0] == 1 && !r[2] ? r[1] : -1;
    return r[0] == 1 ? r[1] : (pos == r[3] ? r[4] : -1);
}

int32_t mt_engine_resolve_remote_client_position(mt_engine* e, int64_t doc, int32_t pos, int32_t ref_seq,
                                                 int32_t long_client, int32_t* out) {
    if (!out) return MT_E_ARG;
    int32_t r[MT_SEGQ_N];
    int32_t rc = seg_query(e, doc, 4, pos, 0, ref_seq, long_client, r);
    if (rc) return rc;
    *out = remote_pos(r, pos, false);
    return MT_OK;
}

int32_t mt_engine_adjust_position(mt_engine* e, int64_t doc, int32_t pos, int32_t from_seq, int32_t long_client,
                                  int32_t* out) {
    if (!out) return MT_E_ARG;
    int32_t r[MT_SEGQ_N];
    int32_t rc = seg_query(e, doc, 4, pos, 0, from_seq, long_client, r);
    if (rc) return rc;
    *out = remote_pos(r, pos, true);
    return MT_OK;
}

int32_t mt_engine_handle_to_position(mt_engine* e, int64_t doc, int32_t handle, int32_t local_seq, int32_t* out) {
    if (!out) return MT_E_ARG;
    int32_t r[MT_SEGQ_N];
    int32_t rc = seg_query(e, doc, 6, handle, local_seq, 0, -1, r);
    if (rc) return rc;
    /* assert(localSeq <= collabWindow.localSeq) (client.ts:676) and assert(isHandleValid(containingSegment.start)) */
    if (r[0] != 1) return MT_E_ARG;
    *out = r[1];
    return MT_OK;
}

int32_t mt_engine_get_marker_from_id(mt_engine* e, int64_t doc, int32_t id_key, int32_t id_value, mt_seg_ref* out) {
    if (!out) return MT_E_ARG;
    int32_t r[MT_SEGQ_N];
    int32_t rc = seg_query(e, doc, 5, id_key, id_value, 0, -1, r);
    if (rc) return rc;
    if (r[0] == 2) return MT_E_UNSUPPORTED; /* several markers hold the id, or an annotate changed it */
    seg_ref_of(r, out);
    return MT_OK;
}

int64_t mt_engine_segment_ids(mt_engine* e, int64_t doc, int32_t* out, int64_t cap) {
    if (!e || doc < 0 || doc >= e->ndocs || cap < 0) return -MT_E_ARG;
    e = route(e, &doc);
    if (hipSetDevice(e->device) != hipSuccess) return -MT_E_HIP;
    if (ensure(e, e->tmp, 16 + 8 * (size_t)(out ? cap : 0) + 16)) return -MT_E_HIP;
    int64_t* dn = (int64_t*)e->tmp.p;
    int32_t* dbuf = (int32_t*)((uint8_t*)e->tmp.p + 16);
    int32_t rc = e->ops->segids(e, doc, dbuf, out ? cap : 0, dn);
    if (rc) return -rc;
    return read_counted(e, dn, whole_count, dbuf, 8, out, cap);
}

/* ---- batched reads (mt_kernels.h k_lengths / k_text_sizes / k_texts / k_segs) ---------------------------------
 * The queries of one call, grouped by the engine that holds their document (route, through chains of promotions),
 * each group a contiguous run of `q` and one launch on its engine's stream. In a tiled engine the reads keep
 * scratch in the document block, so the k-th query that names a document goes into the k-th launch there
 * (launches on one stream run in order). All engines of a chain share the device: the queries and the results
 * live in the root engine's buffers, and every result lands at the caller's query index (ReadQ.slot). */
struct ReadPlan {
    struct Run {
        mt_engine* eng;
        int64_t q0, n;
    };
    std::vector<ReadQ> q;
    std::vector<Run> runs;
};
static int32_t read_plan(mt_engine* e, int64_t m, const int64_t* docs, const int32_t* a, const int32_t* b,
                         int32_t dflt, const int32_t* ref_seqs, const int32_t* long_clients, ReadPlan& p) {
    if (m > (int64_t)0x7fffffff || !ref_seqs != !long_clients || (!docs && m > e->ndocs)) return MT_E_ARG;
    std::vector<mt_engine*> chain;
    for (mt_engine* x = e; x; x = x->over) chain.push_back(x);
    std::vector<std::vector<ReadQ>> by(chain.size());
    for (int64_t i = 0; i < m; i++) {
        int64_t d = docs ? docs[i] : i;
        if (d < 0 || d >= e->ndocs) return MT_E_ARG;
        const int32_t lc = long_clients ? long_clients[i] : -1;
        const int32_t floor = persp_floor(e, d, lc); /* on the engine the caller holds, before routing */
        size_t depth = 0;
        for (mt_engine* x = e; x->over && x->pro[(size_t)d] >= 0; x = x->over, depth++) d = x->pro[(size_t)d];
        by[depth].push_back(ReadQ{d, ref_seqs ? ref_seqs[i] : 0, lc, floor, a ? a[i] : dflt, b ? b[i] : dflt, (int32_t)i});
    }
    p.q.reserve((size_t)m);
    for (size_t k = 0; k < chain.size(); k++) {
        std::vector<ReadQ>& g = by[k];
        if (g.empty()) continue;
        if (chain[k]->profile != P_HUGE) {
            p.runs.push_back({chain[k], (int64_t)p.q.size(), (int64_t)g.size()});
            p.q.insert(p.q.end(), g.begin(), g.end());
            continue;
        }
        std::vector<int32_t> seen((size_t)chain[k]->ndocs, 0), round(g.size());
        int32_t rounds = 0;
        for (size_t i = 0; i < g.size(); i++) rounds = std::max(rounds, (round[i] = seen[(size_t)g[i].doc]++) + 1);
        for (int32_t r = 0; r < rounds; r++) {
            const int64_t q0 = (int64_t)p.q.size();
            for (size_t i = 0; i < g.size(); i++)
                if (round[i] == r) p.q.push_back(g[i]);
            p.runs.push_back({chain[k], q0, (int64_t)p.q.size() - q0});
        }
    }
    return MT_OK;
}
extern "C++" {
/* one launch per run of the plan: launch(engine, stream, its queries on the device, their count). What the root
 * engine's stream has copied to the device is there before a child's stream reads it, and the root waits on each
 * child's stream before it copies anything back. */
template <class F>
static int32_t read_launch(mt_engine* e, const ReadPlan& p, const ReadQ* dq, F&& launch) {
    bool children = false;
    for (const ReadPlan::Run& r : p.runs) children |= r.eng != e;
    if (children) HIPCHK(e, hipStreamSynchronize(e->stream));
    for (const ReadPlan::Run& r : p.runs) {
        int32_t rc = launch(r.eng, r.eng->stream, dq + r.q0, r.n);
        if (rc) {
            if (r.eng != e) e->err = r.eng->err;
            return rc;
        }
    }
    for (size_t i = 0; children && i < p.runs.size(); i++)
        if (p.runs[i].eng != e && (i == 0 || p.runs[i].eng != p.runs[i - 1].eng))
            HIPCHK(e, hipStreamSynchronize(p.runs[i].eng->stream));
    return MT_OK;
}
}
static size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

int32_t mt_engine_get_lengths(mt_engine* e, int64_t m, const int64_t* docs, const int32_t* ref_seqs,
                              const int32_t* long_clients, int32_t* len_out, int32_t* status_out) {
    if (!e || m < 0) return MT_E_ARG;
    if (m == 0) return MT_OK;
    if (!len_out || (!status_out && long_clients)) return MT_E_ARG;
    ReadPlan p;
    int32_t rc = read_plan(e, m, docs, nullptr, nullptr, 0, ref_seqs, long_clients, p);
    if (rc) return rc;
    HIPCHK(e, hipSetDevice(e->device));
    const size_t qb = up16(sizeof(ReadQ) * (size_t)m);
    if ((rc = ensure(e, e->rq, qb + 8 * (size_t)m))) return rc;
    ReadQ* dq = (ReadQ*)e->rq.p;
    int32_t* dlen = (int32_t*)((uint8_t*)e->rq.p + qb);
    int32_t* dst = dlen + m;
    HIPCHK(e, hipMemcpyAsync(dq, p.q.data(), sizeof(ReadQ) * (size_t)m, hipMemcpyHostToDevice, e->stream));
    rc = read_launch(e, p, dq, [&](mt_engine* x, hipStream_t s, const ReadQ* q, int64_t n) {
        return x->ops->lengths(x, s, n, q, dlen, dst);
    });
    if (rc) return rc;
    HIPCHK(e, hipMemcpyAsync(len_out, dlen, 4 * (size_t)m, hipMemcpyDeviceToHost, e->stream));
    if (status_out) HIPCHK(e, hipMemcpyAsync(status_out, dst, 4 * (size_t)m, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return MT_OK;
}

int64_t mt_engine_get_texts(mt_engine* e, int64_t m, const int64_t* docs, const int32_t* ref_seqs,
                            const int32_t* long_clients, const int32_t* starts, const int32_t* ends,
                            const uint16_t* placeholder, int32_t placeholder_len, int64_t* off_out,
                            int32_t* status_out, uint16_t* out, int64_t cap) {
    if (!e || m < 0 || cap < 0 || placeholder_len < 0 || placeholder_len > 4096 || (placeholder_len > 0 && !placeholder))
        return -MT_E_ARG;
    if (placeholder_len == 1 && placeholder[0] == '*') return -MT_E_UNSUPPORTED; /* Marker.toString() */
    if (m == 0) return 0;
    if (!off_out || (!status_out && long_clients)) return -MT_E_ARG;
    ReadPlan p;
    int32_t rc = read_plan(e, m, docs, starts, ends, MT_TEXT_DEFAULT, ref_seqs, long_clients, p);
    if (rc) return -rc;
    if (hipSetDevice(e->device) != hipSuccess) return -MT_E_HIP;
    /* the queries, their sizes, the offsets, the statuses, the placeholder */
    const size_t qb = up16(sizeof(ReadQ) * (size_t)m), sb = up16(8 * (size_t)m), ob = up16(8 * ((size_t)m + 1)),
                 tb = up16(4 * (size_t)m), phb = up16(2 * (size_t)placeholder_len);
    if ((rc = ensure(e, e->rq, qb + sb + ob + tb + phb))) return -rc;
    uint8_t* base = (uint8_t*)e->rq.p;
    ReadQ* dq = (ReadQ*)base;
    int64_t* dsize = (int64_t*)(base + qb);
    int64_t* doff = (int64_t*)(base + qb + sb);
    int32_t* dst = (int32_t*)(base + qb + sb + ob);
    uint16_t* dph = (uint16_t*)(base + qb + sb + ob + tb);
    if (hipMemcpyAsync(dq, p.q.data(), sizeof(ReadQ) * (size_t)m, hipMemcpyHostToDevice, e->stream) != hipSuccess)
        return -MT_E_HIP;
    if (placeholder_len > 0 &&
        hipMemcpyAsync(dph, placeholder, 2 * (size_t)placeholder_len, hipMemcpyHostToDevice, e->stream) != hipSuccess)
        return -MT_E_HIP;
    rc = read_launch(e, p, dq, [&](mt_engine* x, hipStream_t s, const ReadQ* q, int64_t n) {
        return x->ops->text_sizes(x, s, n, q, placeholder_len, dsize, dst);
    });
    if (rc) return -rc;
    /* the exclusive prefix sum of the sizes, on the host: they come back in one copy */
    if (hipMemcpyAsync(off_out + 1, dsize, 8 * (size_t)m, hipMemcpyDeviceToHost, e->stream) != hipSuccess)
        return -MT_E_HIP;
    if (status_out && hipMemcpyAsync(status_out, dst, 4 * (size_t)m, hipMemcpyDeviceToHost, e->stream) != hipSuccess)
        return -MT_E_HIP;
    if (hipStreamSynchronize(e->stream) != hipSuccess) return -MT_E_HIP;
    off_out[0] = 0;
    for (int64_t i = 0; i < m; i++) off_out[i + 1] += off_out[i];
    const int64_t total = off_out[m];
    if (!out || total > cap || total == 0) return total; /* all or nothing */
    if (ensure(e, e->tmp, 2 * (size_t)total)) return -MT_E_NOMEM;
    uint16_t* dout = (uint16_t*)e->tmp.p;
    if (hipMemcpyAsync(doff, off_out, 8 * ((size_t)m + 1), hipMemcpyHostToDevice, e->stream) != hipSuccess)
        return -MT_E_HIP;
    const bool packed = e->texts_packed;
    rc = read_launch(e, p, dq, [&](mt_engine* x, hipStream_t s, const ReadQ* q, int64_t n) {
        return x->ops->texts(x, s, n, q, dph, placeholder_len, doff, dout, packed);
    });
    if (rc) return -rc;
    if (hipMemcpyAsync(out, dout, 2 * (size_t)total, hipMemcpyDeviceToHost, e->stream) != hipSuccess) return -MT_E_HIP;
    if (hipStreamSynchronize(e->stream) != hipSuccess) return -MT_E_HIP;
    return total;
}

extern "C++" {
/* The sizing contract of the batched dumps, summaries and handle tables, in one place: plan the queries, size(engine,
 * stream, queries, count, sizes) per run, the prefix sum on the host into off_out[0..m], then (when `out` is given and
 * the total fits cap: all or nothing) fill(engine, stream, queries, count, offsets, bytes) per run and one copy back.
 * Sizes, offsets and cap count elements of `unit` bytes. */
template <class FS, class FF>
static int64_t windows_read(mt_engine* e, int64_t m, const int64_t* docs, int64_t* off_out, uint8_t* out, int64_t cap,
                            FS&& size, FF&& fill, size_t unit = 1) {
    if (!e || m < 0 || cap < 0) return -MT_E_ARG;
    if (m == 0) return 0;
    if (!off_out) return -MT_E_ARG;
    ReadPlan p;
    int32_t rc = read_plan(e, m, docs, nullptr, nullptr, 0, nullptr, nullptr, p);
    if (rc) return -rc;
    if (hipSetDevice(e->device) != hipSuccess) return -MT_E_HIP;
    /* the queries, their sizes, the offsets */
    const size_t qb = up16(sizeof(ReadQ) * (size_t)m), sb = up16(8 * (size_t)m), ob = up16(8 * ((size_t)m + 1));
    if ((rc = ensure(e, e->rq, qb + sb + ob))) return -rc;
    uint8_t* base = (uint8_t*)e->rq.p;
    ReadQ* dq = (ReadQ*)base;
    int64_t* dsize = (int64_t*)(base + qb);
    int64_t* doff = (int64_t*)(base + qb + sb);
    if (hipMemcpyAsync(dq, p.q.data(), sizeof(ReadQ) * (size_t)m, hipMemcpyHostToDevice, e->stream) != hipSuccess)
        return -MT_E_HIP;
    rc = read_launch(e, p, dq, [&](mt_engine* x, hipStream_t s, const ReadQ* q, int64_t n) {
        return size(x, s, n, q, dsize);
    });
    if (rc) return -rc;
    if (hipMemcpyAsync(off_out + 1, dsize, 8 * (size_t)m, hipMemcpyDeviceToHost, e->stream) != hipSuccess)
        return -MT_E_HIP;
    if (hipStreamSynchronize(e->stream) != hipSuccess) return -MT_E_HIP;
    off_out[0] = 0;
    for (int64_t i = 0; i < m; i++) off_out[i + 1] += off_out[i];
    const int64_t total = off_out[m];
    if (!out || total > cap) return total; /* all or nothing */
    if (ensure(e, e->tmp, unit * (size_t)total)) return -MT_E_NOMEM;
    uint8_t* dout = (uint8_t*)e->tmp.p;
    if (hipMemcpyAsync(doff, off_out, 8 * ((size_t)m + 1), hipMemcpyHostToDevice, e->stream) != hipSuccess)
        return -MT_E_HIP;
    rc = read_launch(e, p, dq, [&](mt_engine* x, hipStream_t s, const ReadQ* q, int64_t n) {
        return fill(x, s, n, q, doff, dout);
    });
    if (rc) return -rc;
    if (hipMemcpyAsync(out, dout, unit * (size_t)total, hipMemcpyDeviceToHost, e->stream) != hipSuccess)
        return -MT_E_HIP;
    if (hipStreamSynchronize(e->stream) != hipSuccess) return -MT_E_HIP;
    return total;
}
}

int64_t mt_engine_dumps(mt_engine* e, int64_t m, const int64_t* docs, int64_t* off_out, uint8_t* out, int64_t cap) {
    const bool par = e && e->dumps_parallel;
    return windows_read(
        e, m, docs, off_out, out, cap,
        [&](mt_engine* x, hipStream_t s, int64_t n, const ReadQ* q, int64_t* dsize) {
            return x->ops->dump_sizes(x, s, n, q, dsize);
        },
        [&](mt_engine* x, hipStream_t s, int64_t n, const ReadQ* q, const int64_t* doff, uint8_t* dout) {
            return x->ops->dumps(x, s, n, q, doff, dout, par);
        });
}

int64_t mt_engine_summaries(mt_engine* e, int64_t m, const int64_t* docs, int32_t mode, int64_t* off_out, uint8_t* out,
                            int64_t cap) {
    if (mode != MT_SUMMARY_V1 && mode != MT_SUMMARY_LEGACY) return -MT_E_ARG;
    const bool par = e && e->summaries_parallel;
    return windows_read(
        e, m, docs, off_out, out, cap,
        [&](mt_engine* x, hipStream_t s, int64_t n, const ReadQ* q, int64_t* dsize) {
            return x->ops->summary_sizes(x, s, n, q, mode, dsize);
        },
        [&](mt_engine* x, hipStream_t s, int64_t n, const ReadQ* q, const int64_t* doff, uint8_t* dout) {
            return x->ops->summaries(x, s, n, q, mode, doff, dout, par);
        });
}

/* ---- batched marker queries (mt_kernels.h k_find_tiles / k_stack_sizes / k_stacks) ----
 * The label's value bitmap is copied once per call, into the root engine's read buffer (every engine of a chain is on
 * the root's device). */
int32_t mt_engine_find_tiles(mt_engine* e, int64_t m, const int64_t* docs, const int32_t* pos, const int32_t* preceding,
                             int32_t label_key, const uint32_t* value_set, mt_tile_ref* out, int32_t* status_out) {
    if (!e || m < 0) return MT_E_ARG;
    if (m == 0) return MT_OK;
    if (!out || !status_out || !value_set) return MT_E_ARG;
    ReadPlan p;
    /* a missing pos is undefined (-1) for every query; a missing preceding takes the same default, and any value
     * but 0 means preceding */
    int32_t rc = read_plan(e, m, docs, pos, preceding, -1, nullptr, nullptr, p);
    if (rc) return rc;
    HIPCHK(e, hipSetDevice(e->device));
    const size_t qb = up16(sizeof(ReadQ) * (size_t)m), vb = 4 * (size_t)MT_LABEL_SET_WORDS,
                 rb = up16(4 * (size_t)m * MT_TILE_WORDS);
    if ((rc = ensure(e, e->rq, qb + vb + rb + 4 * (size_t)m))) return rc;
    uint8_t* base = (uint8_t*)e->rq.p;
    ReadQ* dq = (ReadQ*)base;
    uint32_t* dset = (uint32_t*)(base + qb);
    int32_t* dres = (int32_t*)(base + qb + vb);
    int32_t* dst = (int32_t*)(base + qb + vb + rb);
    HIPCHK(e, hipMemcpyAsync(dq, p.q.data(), sizeof(ReadQ) * (size_t)m, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(dset, value_set, vb, hipMemcpyHostToDevice, e->stream));
    const bool par = e->tiles_parallel;
    rc = read_launch(e, p, dq, [&](mt_engine* x, hipStream_t s, const ReadQ* q, int64_t n) {
        return x->ops->find_tiles(x, s, n, q, label_key, dset, dres, dst, par);
    });
    if (rc) return rc;
    HIPCHK(e, hipMemcpyAsync(out, dres, 4 * (size_t)m * MT_TILE_WORDS, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(status_out, dst, 4 * (size_t)m, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return MT_OK;
}

int64_t mt_engine_stack_contexts(mt_engine* e, int64_t m, const int64_t* docs, const int32_t* pos, int32_t label_key,
                                 const uint32_t* value_set, int64_t* off_out, int32_t* count_out, int32_t* status_out,
                                 mt_tile_ref* out, int64_t cap) {
    if (!e || m < 0 || cap < 0) return -MT_E_ARG;
    if (m == 0) return 0;
    if (!off_out || !count_out || !status_out || !value_set) return -MT_E_ARG;
    ReadPlan p;
    int32_t rc = read_plan(e, m, docs, pos, nullptr, -1, nullptr, nullptr, p);
    if (rc) return -rc;
    if (hipSetDevice(e->device) != hipSuccess) return -MT_E_HIP;
    /* the queries, the label set, the high-water marks, the offsets, the counts, the statuses */
    const size_t qb = up16(sizeof(ReadQ) * (size_t)m), vb = 4 * (size_t)MT_LABEL_SET_WORDS, sb = up16(8 * (size_t)m),
                 ob = up16(8 * ((size_t)m + 1)), cb = up16(4 * (size_t)m);
    if ((rc = ensure(e, e->rq, qb + vb + sb + ob + 2 * cb))) return -rc;
    uint8_t* base = (uint8_t*)e->rq.p;
    ReadQ* dq = (ReadQ*)base;
    uint32_t* dset = (uint32_t*)(base + qb);
    int64_t* dhigh = (int64_t*)(base + qb + vb);
    int64_t* doff = (int64_t*)(base + qb + vb + sb);
    int32_t* dcount = (int32_t*)(base + qb + vb + sb + ob);
    int32_t* dst = (int32_t*)(base + qb + vb + sb + ob + cb);
    if (hipMemcpyAsync(dq, p.q.data(), sizeof(ReadQ) * (size_t)m, hipMemcpyHostToDevice, e->stream) != hipSuccess ||
        hipMemcpyAsync(dset, value_set, vb, hipMemcpyHostToDevice, e->stream) != hipSuccess)
        return -MT_E_HIP;
    rc = read_launch(e, p, dq, [&](mt_engine* x, hipStream_t s, const ReadQ* q, int64_t n) {
        return x->ops->stack_sizes(x, s, n, q, label_key, dset, dcount, dhigh, dst);
    });
    if (rc) return -rc;
    if (hipMemcpyAsync(off_out + 1, dhigh, 8 * (size_t)m, hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
        hipMemcpyAsync(count_out, dcount, 4 * (size_t)m, hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
        hipMemcpyAsync(status_out, dst, 4 * (size_t)m, hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
        hipStreamSynchronize(e->stream) != hipSuccess)
        return -MT_E_HIP;
    off_out[0] = 0;
    for (int64_t i = 0; i < m; i++) off_out[i + 1] += off_out[i];
    const int64_t total = off_out[m];
    if (!out || total > cap || total == 0) return total; /* all or nothing */
    const size_t eb = 4 * (size_t)MT_TILE_WORDS;
    if (ensure(e, e->tmp, eb * (size_t)total)) return -MT_E_NOMEM;
    int32_t* dout = (int32_t*)e->tmp.p;
    if (hipMemcpyAsync(doff, off_out, 8 * ((size_t)m + 1), hipMemcpyHostToDevice, e->stream) != hipSuccess)
        return -MT_E_HIP;
    const bool par = e->tiles_parallel;
    rc = read_launch(e, p, dq, [&](mt_engine* x, hipStream_t s, const ReadQ* q, int64_t n) {
        return x->ops->stacks(x, s, n, q, label_key, dset, doff, dout, par);
    });
    if (rc) return -rc;
    if (hipMemcpyAsync(out, dout, eb * (size_t)total, hipMemcpyDeviceToHost, e->stream) != hipSuccess) return -MT_E_HIP;
    if (hipStreamSynchronize(e->stream) != hipSuccess) return -MT_E_HIP;
    return total;
}

/* ---- batched matrix reads (mt_kernels.h k_handle_sizes / k_handles / k_handle_positions / k_handle_tables) ---- */
int64_t mt_engine_get_handles(mt_engine* e, int64_t m, const int64_t* docs, const int32_t* starts, const int32_t* ends,
                              int64_t* off_out, int32_t* status_out, int32_t* out, int64_t cap) {
    if (!e || e->pcap <= 0 || m < 0 || cap < 0) return -MT_E_ARG;
    if (m == 0) return 0;
    if (!off_out || !status_out || !starts || !ends) return -MT_E_ARG;
    ReadPlan p;
    int32_t rc = read_plan(e, m, docs, starts, ends, 0, nullptr, nullptr, p);
    if (rc) return -rc;
    if (hipSetDevice(e->device) != hipSuccess) return -MT_E_HIP;
    /* the queries, their sizes, the offsets, the statuses */
    const size_t qb = up16(sizeof(ReadQ) * (size_t)m), sb = up16(8 * (size_t)m), ob = up16(8 * ((size_t)m + 1));
    if ((rc = ensure(e, e->rq, qb + sb + ob + 4 * (size_t)m))) return -rc;
    uint8_t* base = (uint8_t*)e->rq.p;
    ReadQ* dq = (ReadQ*)base;
    int64_t* dsize = (int64_t*)(base + qb);
    int64_t* doff = (int64_t*)(base + qb + sb);
    int32_t* dst = (int32_t*)(base + qb + sb + ob);
    if (hipMemcpyAsync(dq, p.q.data(), sizeof(ReadQ) * (size_t)m, hipMemcpyHostToDevice, e->stream) != hipSuccess)
        return -MT_E_HIP;
    rc = read_launch(e, p, dq, [&](mt_engine* x, hipStream_t s, const ReadQ* q, int64_t n) {
        return x->ops->handle_sizes(x, s, n, q, dsize, dst);
    });
    if (rc) return -rc;
    if (hipMemcpyAsync(off_out + 1, dsize, 8 * (size_t)m, hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
        hipMemcpyAsync(status_out, dst, 4 * (size_t)m, hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
        hipStreamSynchronize(e->stream) != hipSuccess)
        return -MT_E_HIP;
    off_out[0] = 0;
    for (int64_t i = 0; i < m; i++) off_out[i + 1] += off_out[i];
    const int64_t total = off_out[m];
    if (!out || total > cap || total == 0) return total; /* all or nothing */
    if (ensure(e, e->tmp, 4 * (size_t)total)) return -MT_E_NOMEM;
    int32_t* dout = (int32_t*)e->tmp.p;
    if (hipMemcpyAsync(doff, off_out, 8 * ((size_t)m + 1), hipMemcpyHostToDevice, e->stream) != hipSuccess)
        return -MT_E_HIP;
    const bool par = e->handles_parallel;
    rc = read_launch(e, p, dq, [&](mt_engine* x, hipStream_t s, const ReadQ* q, int64_t n) {
        return x->ops->handles(x, s, n, q, doff, dout, par);
    });
    if (rc) return -rc;
    if (hipMemcpyAsync(out, dout, 4 * (size_t)total, hipMemcpyDeviceToHost, e->stream) != hipSuccess) return -MT_E_HIP;
    if (hipStreamSynchronize(e->stream) != hipSuccess) return -MT_E_HIP;
    return total;
}

int32_t mt_engine_handles_to_positions(mt_engine* e, int64_t m, const int64_t* docs, const int32_t* handles,
                                       const int32_t* local_seqs, int32_t* out, int32_t* status_out) {
    if (!e || e->pcap <= 0 || m < 0) return MT_E_ARG;
    if (m == 0) return MT_OK;
    if (!handles || !out || !status_out) return MT_E_ARG;
    ReadPlan p;
    int32_t rc = read_plan(e, m, docs, handles, local_seqs, MT_LOCAL_SEQ_CURRENT, nullptr, nullptr, p);
    if (rc) return rc;
    HIPCHK(e, hipSetDevice(e->device));
    const size_t qb = up16(sizeof(ReadQ) * (size_t)m), rb = up16(4 * (size_t)m);
    if ((rc = ensure(e, e->rq, qb + 2 * rb))) return rc;
    uint8_t* base = (uint8_t*)e->rq.p;
    ReadQ* dq = (ReadQ*)base;
    int32_t* dres = (int32_t*)(base + qb);
    int32_t* dst = (int32_t*)(base + qb + rb);
    HIPCHK(e, hipMemcpyAsync(dq, p.q.data(), sizeof(ReadQ) * (size_t)m, hipMemcpyHostToDevice, e->stream));
    const bool par = e->handles_parallel;
    rc = read_launch(e, p, dq, [&](mt_engine* x, hipStream_t s, const ReadQ* q, int64_t n) {
        return x->ops->handle_positions(x, s, n, q, dres, dst, par);
    });
    if (rc) return rc;
    HIPCHK(e, hipMemcpyAsync(out, dres, 4 * (size_t)m, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(status_out, dst, 4 * (size_t)m, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return MT_OK;
}

int64_t mt_engine_handle_tables(mt_engine* e, int64_t m, const int64_t* docs, int64_t* off_out, int32_t* out,
                                int64_t cap) {
    if (!e || e->pcap <= 0) return -MT_E_ARG;
    return windows_read(
        e, m, docs, off_out, (uint8_t*)out, cap,
        [&](mt_engine* x, hipStream_t s, int64_t n, const ReadQ* q, int64_t* dsize) {
            return x->ops->handle_table_sizes(x, s, n, q, dsize);
        },
        [&](mt_engine* x, hipStream_t s, int64_t n, const ReadQ* q, const int64_t* doff, uint8_t* dout) {
            return x->ops->handle_tables(x, s, n, q, doff, (int32_t*)dout);
        },
        4);
}

/* k_segs over m queries: res[i * MT_SEGQ_N ..] = query i's words; status_out[i] = MT_E_UNSUPPORTED for a refused one */
static int32_t segs_read(mt_engine* e, int64_t m, const int64_t* docs, const int32_t* pos, const int32_t* ref_seqs,
                         const int32_t* long_clients, int32_t mode, std::vector<int32_t>& res, int32_t* status_out) {
    if (!pos || (!status_out && long_clients)) return MT_E_ARG;
    ReadPlan p;
    int32_t rc = read_plan(e, m, docs, pos, nullptr, 0, ref_seqs, long_clients, p);
    if (rc) return rc;
    HIPCHK(e, hipSetDevice(e->device));
    const size_t qb = up16(sizeof(ReadQ) * (size_t)m), rb = 4 * (size_t)m * MT_SEGQ_N;
    if ((rc = ensure(e, e->rq, qb + rb))) return rc;
    ReadQ* dq = (ReadQ*)e->rq.p;
    int32_t* dres = (int32_t*)((uint8_t*)e->rq.p + qb);
    HIPCHK(e, hipMemcpyAsync(dq, p.q.data(), sizeof(ReadQ) * (size_t)m, hipMemcpyHostToDevice, e->stream));
    rc = read_launch(e, p, dq, [&](mt_engine* x, hipStream_t s, const ReadQ* q, int64_t n) {
        return x->ops->segs(x, s, n, q, mode, dres);
    });
    if (rc) return rc;
    res.resize((size_t)m * MT_SEGQ_N);
    HIPCHK(e, hipMemcpyAsync(res.data(), dres, rb, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    for (int64_t i = 0; status_out && i < m; i++)
        status_out[i] = res[(size_t)i * MT_SEGQ_N] == 3 ? MT_E_UNSUPPORTED : MT_OK;
    return MT_OK;
}

int32_t mt_engine_get_containing_segments(mt_engine* e, int64_t m, const int64_t* docs, const int32_t* pos,
                                          const int32_t* ref_seqs, const int32_t* long_clients, mt_seg_ref* out,
                                          int32_t* status_out) {
    if (!e || m < 0) return MT_E_ARG;
    if (m == 0) return MT_OK;
    if (!out) return MT_E_ARG;
    std::vector<int32_t> res;
    int32_t rc = segs_read(e, m, docs, pos, ref_seqs, long_clients, 0, res, status_out);
    if (rc) return rc;
    for (int64_t i = 0; i < m; i++) seg_ref_of(&res[(size_t)i * MT_SEGQ_N], &out[i]);
    return MT_OK;
}

static int32_t remote_positions(mt_engine* e, int64_t m, const int64_t* docs, const int32_t* pos, const int32_t* seqs,
                                const int32_t* long_clients, bool adjust, int32_t* out, int32_t* status_out) {
    if (!e || m < 0) return MT_E_ARG;
    if (m == 0) return MT_OK;
    if (!out) return MT_E_ARG;
    std::vector<int32_t> res;
    int32_t rc = segs_read(e, m, docs, pos, seqs, long_clients, 4, res, status_out);
    if (rc) return rc;
    for (int64_t i = 0; i < m; i++) {
        const int32_t* r = &res[(size_t)i * MT_SEGQ_N];
        out[i] = r[0] == 3 ? -1 : remote_pos(r, pos[i], adjust);
    }
    return MT_OK;
}
int32_t mt_engine_resolve_remote_client_positions(mt_engine* e, int64_t m, const int64_t* docs, const int32_t* pos,
                                                  const int32_t* ref_seqs, const int32_t* long_clients,
                                                  int32_t* out, int32_t* status_out) {
    return remote_positions(e, m, docs, pos, ref_seqs, long_clients, false, out, status_out);
}
int32_t mt_engine_adjust_positions(mt_engine* e, int64_t m, const int64_t* docs, const int32_t* pos,
                                   const int32_t* from_seqs, const int32_t* long_clients, int32_t* out,
                                   int32_t* status_out) {
    return remote_positions(e, m, docs, pos, from_seqs, long_clients, true, out, status_out);
}

/* where the host reads a document's block directly: the block (its header is at the start), the DState at the head
 * of its delta region (the logged words follow it) and its handle table */
struct DocBlock {
    const uint8_t* hdr;
    const DState* dstate;
    const int32_t* ht;
};
static DocBlock doc_block(const mt_engine* e, int64_t doc) {
    return with_profile(e->profile, [&](auto tag) {
        typedef Doc<typename decltype(tag)::Hot> D;
        const uint8_t* b = e->st.base + doc * e->st.stride;
        return DocBlock{b, (const DState*)(b + D::off_dl(e->st.caps)), (const int32_t*)(b + D::off_ht(e->st.caps))};
    });
}

int32_t mt_engine_delta_state(mt_engine* e, int64_t* n_out, uint64_t* hash_out) {
    if (!e || e->dcap <= 0) return MT_E_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    std::vector<DState> st((size_t)e->ndocs);
    /* one strided copy: the DState at the head of each document's delta region */
    HIPCHK(e, hipMemcpy2DAsync(st.data(), sizeof(DState), doc_block(e, 0).dstate, (size_t)e->st.stride, sizeof(DState),
                               (size_t)e->ndocs, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    for (int64_t d = 0; d < e->ndocs; d++) {
        if (n_out) n_out[d] = st[d].n;
        if (hash_out) hash_out[d] = st[d].h;
    }
    return read_promoted(e, n_out, 1, 1, [&](mt_engine* o, int64_t* a) {
        return read_promoted(e, hash_out, 1, 1, [&](mt_engine*, uint64_t* b) { return mt_engine_delta_state(o, a, b); });
    });
}

int64_t mt_engine_deltas(mt_engine* e, int64_t doc, int32_t* out, int64_t cap) {
    if (!e || e->dcap <= 0 || doc < 0 || doc >= e->ndocs || cap < 0) return -MT_E_ARG;
    const int64_t dcap = e->dcap; /* the caller's engine's: a promoted document's engine logs four times as many */
    e = route(e, &doc);
    if (hipSetDevice(e->device) != hipSuccess) return -MT_E_HIP;
    const DState* ds = doc_block(e, doc).dstate;
    return read_counted(e, ds, [&](const DState& st) { return std::min(st.n, dcap); }, ds + 1, 4, out, cap);
}

/* the batched form (mt_kernels.h k_delta_sizes / k_deltas): sizes, the prefix sum on the host, then the fill */
int64_t mt_engine_deltas_batch(mt_engine* e, int64_t m, const int64_t* docs, const int64_t* from_words, int32_t kinds,
                               int64_t* off_out, int64_t* end_out, int64_t* emitted_out, int32_t* status_out,
                               int32_t* out, int64_t cap) {
    if (!e || e->dcap <= 0 || m < 0 || cap < 0 || kinds <= 0 ||
        (kinds & ~(MT_DELTA_KINDS_SEQUENCE | MT_DELTA_KINDS_MAINTENANCE)))
        return -MT_E_ARG;
    if (m == 0) return 0;
    if (!off_out || !status_out) return -MT_E_ARG;
    /* a cursor is a word index below dcap, an int32: one that is not is invalid like any negative one */
    std::vector<int32_t> from;
    if (from_words) {
        from.resize((size_t)m);
        for (int64_t i = 0; i < m; i++)
            from[(size_t)i] = from_words[i] < 0 || from_words[i] > e->dcap ? -1 : (int32_t)from_words[i];
    }
    ReadPlan p;
    int32_t rc = read_plan(e, m, docs, from_words ? from.data() : nullptr, nullptr, 0, nullptr, nullptr, p);
    if (rc) return -rc;
    if (hipSetDevice(e->device) != hipSuccess) return -MT_E_HIP;
    /* the queries, their sizes, the offsets, the next cursors, the emitted counts, the statuses */
    const size_t qb = up16(sizeof(ReadQ) * (size_t)m), sb = up16(8 * (size_t)m), ob = up16(8 * ((size_t)m + 1));
    if ((rc = ensure(e, e->rq, qb + 3 * sb + ob + 4 * (size_t)m))) return -rc;
    uint8_t* base = (uint8_t*)e->rq.p;
    ReadQ* dq = (ReadQ*)base;
    int64_t* dsize = (int64_t*)(base + qb);
    int64_t* dend = (int64_t*)(base + qb + sb);
    int64_t* demit = (int64_t*)(base + qb + 2 * sb);
    int64_t* doff = (int64_t*)(base + qb + 3 * sb);
    int32_t* dst = (int32_t*)(base + qb + 3 * sb + ob);
    if (hipMemcpyAsync(dq, p.q.data(), sizeof(ReadQ) * (size_t)m, hipMemcpyHostToDevice, e->stream) != hipSuccess)
        return -MT_E_HIP;
    const int32_t dcap = e->dcap; /* the caller's engine's, as mt_engine_deltas */
    const bool par = e->deltas_parallel;
    rc = read_launch(e, p, dq, [&](mt_engine* x, hipStream_t s, const ReadQ* q, int64_t n) {
        return x->ops->delta_sizes(x, s, n, q, dcap, kinds, dsize, dend, demit, dst, par);
    });
    if (rc) return -rc;
    if (hipMemcpyAsync(off_out + 1, dsize, 8 * (size_t)m, hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
        hipMemcpyAsync(status_out, dst, 4 * (size_t)m, hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
        (end_out && hipMemcpyAsync(end_out, dend, 8 * (size_t)m, hipMemcpyDeviceToHost, e->stream) != hipSuccess) ||
        (emitted_out &&
         hipMemcpyAsync(emitted_out, demit, 8 * (size_t)m, hipMemcpyDeviceToHost, e->stream) != hipSuccess) ||
        hipStreamSynchronize(e->stream) != hipSuccess)
        return -MT_E_HIP;
    off_out[0] = 0;
    for (int64_t i = 0; i < m; i++) off_out[i + 1] += off_out[i];
    const int64_t total = off_out[m];
    if (!out || total > cap || total == 0) return total; /* all or nothing */
    if (ensure(e, e->tmp, 4 * (size_t)total)) return -MT_E_NOMEM;
    int32_t* dout = (int32_t*)e->tmp.p;
    if (hipMemcpyAsync(doff, off_out, 8 * ((size_t)m + 1), hipMemcpyHostToDevice, e->stream) != hipSuccess)
        return -MT_E_HIP;
    rc = read_launch(e, p, dq, [&](mt_engine* x, hipStream_t s, const ReadQ* q, int64_t n) {
        return x->ops->deltas(x, s, n, q, dcap, kinds, doff, dout, par);
    });
    if (rc) return -rc;
    if (hipMemcpyAsync(out, dout, 4 * (size_t)total, hipMemcpyDeviceToHost, e->stream) != hipSuccess) return -MT_E_HIP;
    if (hipStreamSynchronize(e->stream) != hipSuccess) return -MT_E_HIP;
    return total;
}

int32_t mt_engine_doc_error(mt_engine* e, int64_t doc, int32_t* err, int32_t* err_op) {
    if (!e || doc < 0 || doc >= e->ndocs) return MT_E_ARG;
    e = route(e, &doc);
    HIPCHK(e, hipSetDevice(e->device));
    int32_t v[2];
    const uint8_t* h = doc_block(e, doc).hdr + offsetof(DocHdr, err);
    static_assert(offsetof(DocHdr, errOp) == offsetof(DocHdr, err) + 4, "err, errOp adjacent");
    HIPCHK(e, hipMemcpyAsync(v, h, sizeof v, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (err) *err = v[0];
    if (err_op) *err_op = v[1];
    return MT_OK;
}

int32_t mt_engine_ref_capacity(const mt_engine* e) { return e ? e->rcap : 0; }

int64_t mt_engine_handle_table(mt_engine* e, int64_t doc, int32_t* out, int64_t cap) {
    if (!e || e->pcap <= 0 || doc < 0 || doc >= e->ndocs || cap < 0) return -MT_E_ARG;
    e = route(e, &doc);
    if (hipSetDevice(e->device) != hipSuccess) return -MT_E_HIP;
    const DocBlock b = doc_block(e, doc);
    return read_counted(e, b.dstate, [](const DState& st) { return (int64_t)st.hlen; }, b.ht, 4, out, cap);
}

int32_t mt_engine_get_handle(mt_engine* e, int64_t doc, int32_t pos, int32_t* out) {
    if (!out) return MT_E_ARG;
    int32_t r[MT_SEGQ_N];
    int32_t rc = seg_query(e, doc, 3, pos, 0, 0, -1, r);
    if (rc) return rc;
    if (!r[0]) return MT_E_ARG; /* RangeError: no segment at pos (ensureRange) */
    *out = r[1];
    return MT_OK;
}

int32_t mt_engine_ref_positions(mt_engine* e, int32_t* nref_out, int32_t* pos_out) {
    if (!e || e->rcap <= 0) return MT_E_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    int64_t n = e->ndocs;
    int32_t rc = ensure(e, e->tmp, 4 * (size_t)n * (1 + (size_t)e->rcap));
    if (rc) return rc;
    int32_t* dn = (int32_t*)e->tmp.p;
    int32_t* dpos = dn + n;
    rc = e->ops->refpos(e, dn, dpos);
    if (rc) return rc;
    if (nref_out) HIPCHK(e, hipMemcpyAsync(nref_out, dn, 4 * (size_t)n, hipMemcpyDeviceToHost, e->stream));
    if (pos_out)
        HIPCHK(e, hipMemcpyAsync(pos_out, dpos, 4 * (size_t)n * e->rcap, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    /* the promoted engine's rows have its own (larger) length; the caller's rows keep e->rcap entries, the first of
     * each child row. nref stays the true count (it may exceed e->rcap). */
    const size_t crow = promoted(e) ? (size_t)e->over->rcap : 0;
    return read_promoted(e, nref_out, 1, 1, [&](mt_engine* o, int32_t* a) {
        return read_promoted(e, pos_out, (size_t)e->rcap, crow,
                             [&](mt_engine*, int32_t* b) { return mt_engine_ref_positions(o, a, b); });
    });
}

#ifdef MT_PROF
/* profiling build only: per-doc phase cycles of the last run (PH_* order in mt_core.h) */
int32_t mt_engine_profile(mt_engine* e, uint64_t* out) {
    if (!e || !out || !e->prof.p) return MT_E_ARG;
    HIPCHK(e, hipMemcpyAsync(out, e->prof.p, sizeof(uint64_t) * PH_N * e->ndocs, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return MT_OK;
}
#endif

} /* extern "C" */
