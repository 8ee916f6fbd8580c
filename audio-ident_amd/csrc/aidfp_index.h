// aidfp_index.h -- the hash index (spec/FPSPEC.md 7): its state (struct HashIndex, one per engine as aid_engine::idx),
// the read-only view the matcher gets of it, and the functions index_host.cpp defines for the other host files. They
// take the engine because they run on its streams; all of them are called with the engine lock held.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>
#include <vector>

#include "aidfp_buffers.h"
#include "aidfp_live_plan.h"

struct aid_engine;

namespace aid {

enum class K4Build { kRadix, kAtomic };  // index_sort.hip (the default) / the atomic counting sort of index.hip

// what K5 (query.cpp) reads of a built index: the CSR and the track table. Valid until the index changes
struct CsrView {
    const uint32_t *offsets;  // [2^26 + 1] bucket starts
    const uint64_t *post;     // track | t << 32 per posting, bucket by bucket in arrival order
    const uint16_t *sig;      // K5's 2-B vote signature per posting (aidfp_layout.h posting_sig)
    const uint8_t *tomb;      // per track id: 1 = removed
    uint32_t n_tracks;
    int check_tomb;  // tracks were removed after the build: the CSR still holds their postings
};

// One CSR over a contiguous range of the stored postings. The index has two (DESIGN 4b "Live ingest"): main over
// postings [0, n_main), and, only while aid_index_live is on, delta over the tail [n_main, n_main + covered). A segment
// is held through a shared_ptr: a ticket submitted with the feature on keeps the segments it was submitted under, and a
// build that finds one of them still held builds into a fresh set of buffers instead of overwriting it.
struct CsrSegment {
    DevBuf<uint32_t> cnt, off;
    DevBuf<uint64_t> post;
    DevBuf<uint16_t> sig;
    int64_t covered = 0;           // stored postings the build read
    int64_t n_indexed = 0;         // postings in the CSR (removed tracks' postings dropped)
    int64_t tomb_since_build = 0;  // removals after the build (queries must check tomb[])
};

struct HashIndex {
    // stored postings (SoA, the source of truth) and the in-flight append. aid_index_add_extracted appends without
    // waiting for its clips' counts: K_append scans them on the device and the new total comes back to pinned
    // h_npost behind add_ev; settle_postings() makes n_post exact again
    DevBuf<uint32_t> p_hash, p_track, p_t;
    int64_t n_post = 0;  // exact unless post_pend: then the last aid_index_add_extracted's count is in flight
    bool post_pend = false;
    Event add_ev;  // after the last append's staging copies (and, if post_pend, its count copy)
    DevBuf<int64_t> d_npost;
    HostBuf<int64_t> h_npost;
    HostBuf<int64_t> h_stage;        // pinned staging of the append: [counts n][src n][dst n][tracks n/2+1]
    DevBuf<int64_t> x_src, x_dst;    // the append's per-clip record starts and posting starts
    DevBuf<uint32_t> x_tracks;       // and track ids

    // track table
    std::vector<uint8_t> h_tomb;  // per track id: 1 = removed
    DevBuf<uint8_t> tomb;
    uint32_t n_tracks = 0;         // max track id + 1
    int64_t n_removed = 0;         // ones in h_tomb

    // CSR built from the postings: main, and the delta of the live index
    bool csr_current = false;  // main is built, and no posting it covers, no track of it and no K4 knob changed since
    std::shared_ptr<CsrSegment> main = std::make_shared<CsrSegment>();
    std::shared_ptr<CsrSegment> delta;  // exists only while live_cap > 0
    std::shared_ptr<CsrSegment> spare;  // the main a fold replaced: the next fold's destination (live_cap > 0 only)
    DevBuf<uint32_t> mrg_tot, mrg_items;  // K4m: the tiles' posting totals, the work items (MergeItem, 3 words each)
    // live index (aid_index_live; policy: aidfp_live_plan.h)
    int64_t live_cap = 0;         // max_delta_postings; 0 = off: every append clears csr_current, as ever
    uint32_t tracks_at_main = 0;  // n_tracks at main's build: an append with only ids >= this keeps main
    int64_t st_main_builds = 0, st_delta_builds = 0, st_folds = 0;
    int64_t st_fallback[kLiveFallbacks] = {};

    // K4 scratch and knobs (aid_engine_force K4_BUILD)
    DevBuf<uint32_t> scan_tmp;
    DevBuf<unsigned long long> nz;    // live keys of the last build
    DevBuf<unsigned long long> chk;   // aid_index_checksum result
    DevBuf<uint32_t> srt_k0, srt_k1;  // sort build: key double buffer
    DevBuf<uint64_t> srt_v;           // sort build: the value buffer idx_post pairs with
    DevBuf<uint32_t> srt_scratch;     // sort build: per-tile digit counts, their scan, scan temporary
    K4Build k4_build = K4Build::kRadix;
    int k4_rank = 0;  // radix sort's in-wave rank: 0 one LDS atomic per posting where the device serves
                      // same-address lanes in order (else ballots), 1 ballots (K4_BUILD 4)

    // exchange scratch (index_exchange.cpp)
    DevBuf<int64_t> g_meta;            // all-gather: (count, n_tracks) per rank
    DevBuf<uint32_t> g_send, g_recv;   // all-gather: [3][max] SoA planes per rank
    int inject_exchange_fail = 0;      // aid_engine_force EXCHANGE_FAIL: the next exchange's prepare step fails (tests)

    CsrView view(const CsrSegment &g) const {  // after ensure_index
        return {g.off.p, g.post.p, g.sig.p, tomb.p, n_tracks, g.tomb_since_build > 0};
    }
    CsrView view() const { return view(*main); }
    LiveState live_state() const {  // n_post settled
        return {live_cap, csr_current, main->covered, n_post, delta ? delta->covered : 0};
    }
    // a second K5 pass is due: the delta holds postings (after ensure_index)
    bool delta_live() const { return live_cap > 0 && csr_current && delta && delta->covered > 0 && delta->n_indexed > 0; }
    // an append of postings whose smallest track id is min_track: main stays current under the disjointness rule
    void note_append(uint32_t min_track) {
        if (live_append_keeps_main(live_cap, csr_current, min_track, tracks_at_main)) return;
        drop_main(kFallOldTrack);
    }
    // main no longer describes the stored postings: the next query runs the full build
    void drop_main(LiveFallback why) {
        if (live_cap > 0 && csr_current) ++st_fallback[why];
        csr_current = false;
    }
};

}  // namespace aid

#pragma GCC visibility push(hidden)
// the posting count of the last aid_index_add_extracted, if still in flight, made exact (the append's own kernels
// are ordered before the event; a reader of n_post or of the planes calls this first)
int settle_postings(aid_engine *e);
int ensure_index(aid_engine *e);  // (re)builds the CSR if it is not current
// the three posting planes grown to `want` postings, every stored posting kept
int grow_postings(aid_engine *e, size_t want, hipStream_t s);
// capacity of the track tables for max_track_plus1 ids, without changing the index
int reserve_tracks(aid_engine *e, uint32_t max_track_plus1, hipStream_t s);
// the track tables grown to max_track_plus1 ids (reserve first: nothing changes if that fails)
int ensure_tracks(aid_engine *e, uint32_t max_track_plus1, hipStream_t s);
#pragma GCC visibility pop
