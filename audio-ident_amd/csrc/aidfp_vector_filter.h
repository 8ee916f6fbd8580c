// aidfp_vector_filter.h -- the host plan of the vector lane's filtered search (spec/FPSPEC.md 9.2, K9f): validation
// of a call's filters, the grouping of a batch's queries by identical filter, and the geometry of the allow-bitmaps
// that k_vec_allow (csrc/vector_filter.hip) writes and the selection kernels read. No HIP types: csrc/vector.hip and
// csrc/vector_filter.hip include it, and tests/test_vec_filter_plan_host.py compiles it alone.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/aidfp.h"

namespace aid {

constexpr int kVecFilterBatch = 64;  // queries per batch (kVecQueryBatch), hence distinct filters per batch at most

static_assert(sizeof(aid_vec_filter) == 64, "a filter is one 64-byte line on the device");

// ---- bitmap geometry. One bit per entry, bit (e & 63) of 64-bit word e >> 6; a filter's bitmap is
// vec_allow_words(n) words, a multiple of 8, so that every bitmap of the batch starts 64-byte aligned. Bits at and
// past n are 0. The readers test bit (e & 31) of the 32-bit word e >> 5 of the same bytes.
inline int64_t vec_allow_words(int64_t n) { return ((n + 63) / 64 + 7) / 8 * 8; }
inline int64_t vec_allow_word(int64_t e) { return e >> 6; }
inline int vec_allow_bit(int64_t e) { return (int)(e & 63); }

// ---- validation: 0, or the index (1-based) of the first filter that is out of range
inline int vec_filters_invalid(const aid_vec_filter *f, int nq) {
    for (int q = 0; q < nq; ++q)
        if (f[q].n_exclude > AID_VEC_MAX_EXCLUDE) return q + 1;
    return 0;
}

// The normal form of a filter: the excluded ids sorted ascending without duplicates (the reserved id
// AID_VEC_NO_TRACK, which no entry carries, dropped), the unused slots AID_VEC_NO_TRACK and the padding zero, so
// that two filters pass the same entries for every catalog exactly when their normal forms are equal bytes.
inline aid_vec_filter vec_filter_normal(const aid_vec_filter &f) {
    aid_vec_filter o;
    memset(&o, 0, sizeof o);
    o.any_of = f.any_of;
    o.all_of = f.all_of;
    o.none_of = f.none_of;
    uint32_t ids[AID_VEC_MAX_EXCLUDE];
    int m = 0;
    for (uint32_t i = 0; i < f.n_exclude && i < AID_VEC_MAX_EXCLUDE; ++i) {
        const uint32_t t = f.exclude[i];
        if (t == AID_VEC_NO_TRACK) continue;
        int at = 0;
        while (at < m && ids[at] < t) ++at;
        if (at < m && ids[at] == t) continue;
        for (int j = m; j > at; --j) ids[j] = ids[j - 1];
        ids[at] = t;
        ++m;
    }
    o.n_exclude = (uint32_t)m;
    for (int i = 0; i < AID_VEC_MAX_EXCLUDE; ++i) o.exclude[i] = i < m ? ids[i] : AID_VEC_NO_TRACK;
    return o;
}

// A filter in normal form that passes every live entry.
inline bool vec_filter_is_zero(const aid_vec_filter &f) {
    return f.any_of == 0 && f.all_of == 0 && f.none_of == 0 && f.n_exclude == 0;
}

// FPSPEC 9.2's rule for one entry (the host restatement of k_vec_allow's test; f in normal form or not).
inline bool vec_filter_passes(const aid_vec_filter &f, bool live, uint64_t tags, uint32_t track) {
    if (!live) return false;
    if (f.any_of != 0 && (tags & f.any_of) == 0) return false;
    if ((tags & f.all_of) != f.all_of) return false;
    if ((tags & f.none_of) != 0) return false;
    for (uint32_t i = 0; i < f.n_exclude && i < AID_VEC_MAX_EXCLUDE; ++i)
        if (f.exclude[i] == track) return false;
    return true;
}

// One batch of at most kVecFilterBatch queries: its D distinct filters in normal form, in order of first use, and
// fmap[q] = the one query q uses. `filtered` is false when every filter of the batch is zero: the caller then runs
// the unfiltered kernels on the unfiltered arguments.
struct VecFilterPlan {
    int n_distinct = 0;
    bool filtered = false;
    int32_t fmap[kVecFilterBatch];
    aid_vec_filter distinct[kVecFilterBatch];
};

inline void vec_filter_plan(const aid_vec_filter *f, int nb, VecFilterPlan &p) {
    p.n_distinct = 0;
    p.filtered = false;
    for (int q = 0; q < kVecFilterBatch; ++q) p.fmap[q] = 0;
    for (int q = 0; q < nb && q < kVecFilterBatch; ++q) {
        const aid_vec_filter nf = vec_filter_normal(f[q]);
        if (!vec_filter_is_zero(nf)) p.filtered = true;
        int d = 0;
        while (d < p.n_distinct && memcmp(&p.distinct[d], &nf, sizeof nf) != 0) ++d;
        if (d == p.n_distinct) p.distinct[p.n_distinct++] = nf;
        p.fmap[q] = d;
    }
}

}  // namespace aid
