// aidfp_index.h -- the hash index (spec/FPSPEC.md 7): its state (struct HashIndex, one per engine as aid_engine::idx),
// the read-only view the matcher gets of it, and the functions index_host.cpp defines for the other host files. They
// take the engine because they run on its streams; all of them are called with the engine lock held.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "aidfp_buffers.h"

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
    int64_t tomb_since_build = 0;  // removals after the last CSR build (queries must check tomb[])

    // CSR built from the postings
    bool csr_current = false;  // built, and no posting, track or K4 knob changed since
    int64_t n_indexed = 0;
    DevBuf<uint32_t> idx_cnt, idx_off;
    DevBuf<uint64_t> idx_post;
    DevBuf<uint16_t> idx_sig;

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

    CsrView view() const {  // after ensure_index
        return {idx_off.p, idx_post.p, idx_sig.p, tomb.p, n_tracks, tomb_since_build > 0};
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
