/*
 * mt_store.h — per-document global-memory layout for a batch of documents.
 *
 * Each document owns one contiguous block: [hot image (HT) | cold rows | text arena (2 halves)
 * | membership log (gid, row id) | pending-group ring]. On the GPU the hot image is staged into
 * LDS for the duration of a replay (small profile) or used in place (larger profiles).
 */
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "mt_core.h"

namespace mt {

template <class HT>
struct Store {
    typedef HT Hot;
    uint8_t* base;
    int64_t stride; /* bytes per document (Doc<HT>::stride) */
    Caps caps;

    MT_HD Doc<HT> doc(int64_t d) const {
        Doc<HT> v;
        v.b = base + d * stride;
        v.t = (HT*)v.b;
        v.caps = caps;
        return v;
    }
};

inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

/* zeroed host block for a store (the hot image's leaf lines are 128-byte aligned); free() it */
inline uint8_t* host_store_alloc(int64_t bytes) {
    void* p = aligned_alloc(256, (size_t)align256(bytes));
    if (p) memset(p, 0, (size_t)align256(bytes));
    return (uint8_t*)p;
}

/* Fill the stride for capacities `caps` (the block layout is Doc<HT>'s); returns bytes for `ndocs`
 * documents. */
template <class HT>
inline int64_t store_layout(Store<HT>& st, const Caps& caps, int64_t ndocs) {
    st.stride = Doc<HT>::stride(caps);
    st.caps = caps;
    st.base = nullptr;
    return st.stride * ndocs;
}

inline bool caps_valid(const Caps& k) { return k.acap >= 16 && k.mcap >= 4 && k.gcap >= 1; }

/* profiles: the hot image type a store's documents use (P_HUGE: tiled, config 4) */
enum Profile : int { P_NONE = -1, P_SMALL = 0, P_MID = 1, P_BIG = 2, P_MAT = 3, P_HUGE = 4 };

inline Profile profile_for(int32_t ncap) {
    if (ncap <= HotSmall::N) return P_SMALL;
    if (ncap <= HotMat::N) return P_MAT;
    if (ncap <= HotMid::N) return P_MID;
    if (ncap <= HotBig::N) return P_BIG;
    if (ncap <= HotHuge::N) return P_HUGE;
    return P_NONE;
}

/* f(ProfTag<HT>()) for the profile's hot image type HT: the one place a profile number becomes a type.
 * A generic f names it with `typename decltype(tag)::Hot`. */
template <class HT>
struct ProfTag {
    typedef HT Hot;
};
template <class F>
inline auto with_profile(int prof, F&& f) {
    switch (prof) {
    case P_SMALL: return f(ProfTag<HotSmall>());
    case P_MAT: return f(ProfTag<HotMat>());
    case P_MID: return f(ProfTag<HotMid>());
    case P_HUGE: return f(ProfTag<HotHuge>());
    default: return f(ProfTag<HotBig>());
    }
}

/* A store whose profile is known at run time only (what an engine holds): Store<HT> without the type. */
struct AnyStore {
    uint8_t* base;
    int64_t stride;
    Caps caps;

    template <class HT>
    Store<HT> as() const {
        return Store<HT>{base, stride, caps};
    }
};

inline int64_t store_layout(AnyStore& st, int prof, const Caps& caps, int64_t ndocs) {
    st.stride = with_profile(prof, [&](auto tag) { return Doc<typename decltype(tag)::Hot>::stride(caps); });
    st.caps = caps;
    st.base = nullptr;
    return st.stride * ndocs;
}

} /* namespace mt */
