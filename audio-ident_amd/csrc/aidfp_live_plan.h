// aidfp_live_plan.h -- the policy of the two-segment hash index (FPSPEC 7, DESIGN 4b "Live ingest"): which build an
// index in a given state needs before a query, whether an append keeps the main segment, and the rule by which a
// query's rows from the two segments become one list. index_host.cpp acts on the decisions, query.cpp and
// k_rows_merge (index.hip) share merge_rows. No HIP in here: tests/test_live_plan_host.py compiles it with plain g++.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define AID_LIVE_HD __host__ __device__
#else
#define AID_LIVE_HD
#endif

namespace aid {

constexpr int64_t kLiveDefaultCap = (int64_t)1 << 24;  // postings a delta holds before it is folded (service default)

// what ensure_index does before a query
enum LiveStep {
    kLiveKeep = 0,  // both segments answer for every stored posting
    kLiveDelta,     // (re)build the delta over the tail [n_main, n_post)
    kLiveFold,      // the tail passed the cap: one CSR over everything, the delta emptied
    kLiveFull,      // no valid main: today's full build (also the only build with the feature off)
};

// why a state that had a valid main fell back to the full build (aid_index_live_stats [6 ..])
enum LiveFallback {
    kFallOldTrack = 0,  // an append carried a track id below the track count at main's build
    kFallCompact,       // aid_index_compact moved the stored postings
    kFallReset,         // aid_index_reset
    kFallLoad,          // aid_index_load
    kFallSplice,        // aid_index_splice / aid_index_allgather replaced a range of postings
    kFallForce,         // aid_engine_force K4_BUILD
    kFallRemoved,       // aid_index_finalize with a track removed since main's build
    kLiveFallbacks
};
constexpr int kLiveStatsWords = 6 + kLiveFallbacks;

struct LiveState {
    int64_t cap;        // aid_index_live's max_delta_postings; 0 = the feature is off
    bool main_current;  // main is built and covers postings [0, n_main) as stored
    int64_t n_main;     // postings main covers
    int64_t n_post;     // postings stored
    int64_t n_delta;    // postings of the tail the delta segment covers (from n_main on)
};

AID_LIVE_HD inline LiveStep live_step(const LiveState &s) {
    if (!s.main_current) return kLiveFull;
    const int64_t tail = s.n_post - s.n_main;
    if (s.cap <= 0) return tail == 0 ? kLiveKeep : kLiveFull;  // off: an append never leaves main current
    if (tail == 0 || tail == s.n_delta) return kLiveKeep;
    return tail <= s.cap ? kLiveDelta : kLiveFold;
}

// The disjointness rule: an append keeps main only while the feature is on, main is current and every track id of the
// append is at or above the track count at main's build, so that no track has postings in both segments. K5's score is
// per (track, d) (FPSPEC 7): then a query's rows over all postings are the merge of its rows over each segment.
AID_LIVE_HD inline bool live_append_keeps_main(int64_t cap, bool main_current, uint32_t min_track, uint32_t tracks_at_main) {
    return cap > 0 && main_current && min_track >= tracks_at_main;
}

// One result row is five int32 words (aid_match_row): match_count, track, d, tq_min, tq_max. Rank order: match_count
// descending, then track id (unsigned) ascending.
constexpr int kRowWords = 5;
AID_LIVE_HD inline bool row_before(const int32_t *a, const int32_t *b) {
    return a[0] != b[0] ? a[0] > b[0] : (uint32_t)a[1] < (uint32_t)b[1];
}

// The rows of a two-segment query: lists a (na rows) and b (nb rows), each in rank order and of at most mr rows,
// merged in rank order and cut at mr; the result replaces a (which has room for mr rows) and its count is returned. In
// place: the first pass finds how many rows of each list make the cut, the second writes them from the back, where
// row k of the result never lands on a row of a that is still to be read (k >= its index in a).
AID_LIVE_HD inline int merge_rows(int32_t *a, int na, const int32_t *b, int nb, int mr) {
    na = na < 0 ? 0 : na > mr ? mr : na;
    nb = nb < 0 ? 0 : nb > mr ? mr : nb;
    const int total = na + nb < mr ? na + nb : mr;
    int ia = 0, ib = 0;
    while (ia + ib < total) {
        if (ib >= nb || (ia < na && !row_before(b + (int64_t)ib * kRowWords, a + (int64_t)ia * kRowWords))) ++ia;
        else ++ib;
    }
    for (int k = total - 1; k >= 0; --k) {
        // the later of the two candidates in rank order goes to slot k; on a tie (never between disjoint segments) b's
        const int32_t *pa = ia > 0 ? a + (int64_t)(ia - 1) * kRowWords : nullptr;
        const int32_t *pb = ib > 0 ? b + (int64_t)(ib - 1) * kRowWords : nullptr;
        const int32_t *src;
        if (!pa) src = pb, --ib;
        else if (!pb) src = pa, --ia;
        else if (row_before(pb, pa)) src = pa, --ia;  // b's row ranks first, so a's is the later one
        else src = pb, --ib;
        int32_t *dst = a + (int64_t)k * kRowWords;
        if (dst != src)
            for (int w = 0; w < kRowWords; ++w) dst[w] = src[w];
    }
    return total;
}

// ---- the fold without a sort: K4m csr_merge (index_merge.hip)
// Both CSRs share the key space and the bucket order, and the delta's postings arrived later: the folded CSR has
// off_new[k] = off_main[k] + off_delta[k] and each bucket is main's run followed by the delta's. The work is split by
// tiles of kMergeTileKeys consecutive keys (a tile's source ranges in both segments and its destination range are
// contiguous, and its offsets fit in LDS), and a tile into work items of at most `bound` destination postings: K4's
// buckets are heavily skewed, and one workgroup per tile would end with the hottest tile.
constexpr int kMergeTileKeys = 1024;
constexpr int kMergeItemPosts = 8192;  // destination postings of one work item (one workgroup)

struct MergeItem {
    uint32_t tile;   // keys [tile * kMergeTileKeys, (tile + 1) * kMergeTileKeys)
    uint32_t first;  // the item's first destination posting, counted from the tile's first
    uint32_t count;  // its postings: 1 .. bound
};

// the number of work items of n_tiles tiles with tile_total[t] destination postings each; with items != nullptr
// (capacity: a first call's result) also the items, in tile order. Empty tiles get none.
inline int64_t plan_merge(const uint32_t *tile_total, int64_t n_tiles, uint32_t bound, MergeItem *items) {
    int64_t n = 0;
    for (int64_t t = 0; t < n_tiles; ++t)
        for (uint32_t first = 0; first < tile_total[t];) {
            const uint32_t left = tile_total[t] - first, count = left < bound ? left : bound;
            if (items) items[n] = MergeItem{(uint32_t)t, first, count};
            ++n;
            first += count;
        }
    return n;
}

}  // namespace aid
