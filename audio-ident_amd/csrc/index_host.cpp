// index_host.cpp -- host side of the hash index (spec/FPSPEC.md 7; state: struct HashIndex, aidfp_index.h): the
// posting planes and their asynchronous append, the track table, K4's CSR build, and the aid_index_* entry points
// that store, remove, compact, build, read back, save and load, and the live index's two CSR segments (aid_index_live:
// main, the delta of the postings stored since, the fold K4m; policy in aidfp_live_plan.h). The exchange between ranks
// is index_exchange.cpp; K5 reads a built CSR segment through HashIndex::view() (query.cpp).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "engine_internal.h"

int grow_postings(aid_engine *e, size_t want, hipStream_t s) {
    HashIndex &ix = e->idx;
    HIP_TRY(ix.p_hash.grow_keep((size_t)ix.n_post, want, s));
    HIP_TRY(ix.p_track.grow_keep((size_t)ix.n_post, want, s));
    HIP_TRY(ix.p_t.grow_keep((size_t)ix.n_post, want, s));
    return AID_OK;
}

// wait for the engine's own streams (not the whole device: torch streams, other engines and ranks on the
// same GPU keep running) before a buffer that in-flight engine work may read is freed
static void sync_engine_streams(aid_engine *e, hipStream_t s) {
    if (e->last_stream && e->last_stream != s) (void)hipStreamSynchronize(e->last_stream);
    if (e->own_stream && e->own_stream != s) (void)hipStreamSynchronize(e->own_stream);
    (void)hipStreamSynchronize(s);
}

// the new tombstone buffer is allocated (and filled) before the old one goes, so a failed growth leaves the engine
// as it was
int reserve_tracks(aid_engine *e, uint32_t max_track_plus1, hipStream_t s) {
    HashIndex &ix = e->idx;
    const size_t want = std::max<size_t>(max_track_plus1, 1024);
    if (want <= ix.tomb.n) return AID_OK;
    DevBuf<uint8_t> nb;
    HIP_TRY(nb.reserve(std::max(want, 2 * ix.tomb.n)));
    if (ix.tomb.p) sync_engine_streams(e, s);  // in-flight queries may still read the old tombstones
    if (ix.n_tracks) {
        // synchronous: the engine's tombstones must be whole in the new buffer before it replaces the old one
        hipError_t he = hipMemcpyAsync(nb.p, ix.h_tomb.data(), ix.n_tracks, hipMemcpyHostToDevice, s);
        if (he == hipSuccess) he = hipStreamSynchronize(s);
        if (he != hipSuccess) return fail(AID_ERR_DEVICE, std::string("reserve_tracks: ") + hipGetErrorString(he));
    }
    std::swap(ix.tomb, nb);  // nb frees the old buffer
    return AID_OK;
}

int ensure_tracks(aid_engine *e, uint32_t max_track_plus1, hipStream_t s) {
    HashIndex &ix = e->idx;
    if (max_track_plus1 <= ix.n_tracks) return AID_OK;
    if (int rc = reserve_tracks(e, max_track_plus1, s)) return rc;
    ix.h_tomb.resize(max_track_plus1, 0);
    ix.n_tracks = max_track_plus1;
    HIP_TRY(hipMemcpyAsync(ix.tomb.p, ix.h_tomb.data(), ix.n_tracks, hipMemcpyHostToDevice, s));
    return AID_OK;
}

int settle_postings(aid_engine *e) {
    HashIndex &ix = e->idx;
    if (!ix.add_ev.live) return AID_OK;
    HIP_TRY(ix.add_ev.wait());
    if (ix.post_pend) ix.n_post = *ix.h_npost.p;
    ix.post_pend = false;
    return AID_OK;
}

extern "C" {

int aid_index_reset(aid_engine *e) {
    EngineCall call(e, nullptr, true);
    if (call.rc) return call.rc;
    HashIndex &ix = e->idx;
    ix.n_post = 0;
    ix.n_tracks = 0;
    ix.h_tomb.clear();
    ix.n_removed = 0;
    ix.drop_main(kFallReset);
    ix.main->n_indexed = 0;
    return AID_OK;
}

int aid_index_add_extracted(aid_engine *e, const uint32_t *track_ids) {
    if (!e) return fail(AID_ERR_INVALID, "aid_index_add_extracted: bad argument");
    EngineCall call(e);
    if (call.rc) return call.rc;
    if (!track_ids && e->ext.plan.n_clips > 0) return fail(AID_ERR_INVALID, "aid_index_add_extracted: bad argument");
    if (!e->ext.have_result) return fail(AID_ERR_STATE, "no extraction to index");
    // 0xFFFFFFFF is K5's empty-slot marker (and track + 1 would wrap to 0 below), as in aid_index_add_track
    for (int c = 0; c < e->ext.plan.n_clips; ++c)
        if (track_ids[c] == 0xFFFFFFFFu) return fail(AID_ERR_INVALID, "aid_index_add_extracted: bad track id");
    HashIndex &ix = e->idx;
    hipStream_t s = e->last_stream ? e->last_stream : call.s;  // behind the extraction, without waiting for it
    const int n = e->ext.plan.n_clips;
    if (n == 0) return AID_OK;
    // the previous call's count (normally long arrived: this batch's extraction was queued behind it) and its
    // pinned staging, whose H2D copies precede that call's event
    if (int rc = settle_postings(e)) return rc;
    // pinned staging [counts n][src n][dst n][tracks n/2+1] (int64 slots)
    HIP_TRY(ix.h_stage.reserve(3 * (size_t)n + (size_t)n / 2 + 1));
    int64_t *counts = ix.h_stage.p, *src = counts + n, *dst = src + n;
    uint32_t *trk = reinterpret_cast<uint32_t *>(dst + n);
    uint32_t mx = 0, mn = 0xFFFFFFFFu;
    for (int c = 0; c < n; ++c) {
        src[c] = e->ext.plan.hash_base[c];
        trk[c] = track_ids[c];
        mx = std::max(mx, track_ids[c] + 1);
        mn = std::min(mn, track_ids[c]);
    }
    if (int rc = ensure_tracks(e, mx, s)) return rc;
    HIP_TRY(ix.x_src.reserve(n));
    HIP_TRY(ix.x_dst.reserve(n));
    HIP_TRY(ix.x_tracks.reserve(n));
    // the batch's postings are at most its hash capacity: when the planes hold that much more, the append is
    // scanned on the device and nothing waits for it; otherwise the counts come back first and the planes grow
    // to the exact need plus one batch's hash capacity (1.5x the records buffer the extraction already holds),
    // so the following appends of such batches are asynchronous again (growth doubles: this path runs
    // O(log n) times), unless that headroom would take more than a quarter of the free device memory
    const int64_t bound = e->ext.plan.records;
    const int64_t cap = (int64_t)std::min({ix.p_hash.n, ix.p_track.n, ix.p_t.n});
    if (ix.n_post + bound <= cap) {
        HIP_TRY(ix.h_npost.reserve(1));
        HIP_TRY(ix.d_npost.reserve(1));
        HIP_TRY(hipMemcpyAsync(ix.x_src.p, src, n * sizeof(int64_t), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(ix.x_tracks.p, trk, n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        launch_append_offsets(e->ext.counts.p, n, ix.n_post, ix.x_dst.p, ix.d_npost.p, s);
        launch_records_to_postings(e->ext.records.p, ix.x_src.p, e->ext.counts.p, ix.x_dst.p, ix.x_tracks.p, n, ix.p_hash.p,
                                   ix.p_track.p, ix.p_t.p, s);
        HIP_TRY(hipMemcpyAsync(ix.h_npost.p, ix.d_npost.p, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(ix.add_ev.record(s));
        HIP_TRY(hipGetLastError());
        ix.post_pend = true;
    } else {
        HIP_TRY(hipMemcpyAsync(counts, e->ext.counts.p, n * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        int64_t tot = 0;
        for (int c = 0; c < n; ++c) {
            dst[c] = ix.n_post + tot;
            tot += counts[c];
        }
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        const bool room = (size_t)bound * 3 * sizeof(uint32_t) <= free_b / 4;
        if (int rc = grow_postings(e, (size_t)(ix.n_post + tot + (room ? bound : 0)), s)) return rc;
        HIP_TRY(hipMemcpyAsync(ix.x_src.p, src, n * sizeof(int64_t), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(ix.x_dst.p, dst, n * sizeof(int64_t), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(ix.x_tracks.p, trk, n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        launch_records_to_postings(e->ext.records.p, ix.x_src.p, e->ext.counts.p, ix.x_dst.p, ix.x_tracks.p, n, ix.p_hash.p,
                                   ix.p_track.p, ix.p_t.p, s);
        HIP_TRY(ix.add_ev.record(s));  // the staging's copies (the next call waits for them)
        HIP_TRY(hipGetLastError());  // no sync: every reader of the posting planes syncs last_stream first
        ix.n_post += tot;
    }
    ix.note_append(mn);
    return AID_OK;
}

int aid_index_add_postings(aid_engine *e, const uint32_t *hash, const uint32_t *track, const uint32_t *t, int64_t n,
                           int32_t location) {
    if (!e || n < 0 || (n > 0 && (!hash || !track || !t))) return fail(AID_ERR_INVALID, "aid_index_add_postings: bad argument");
    if (location != AID_PCM_HOST && location != AID_PCM_DEVICE) return fail(AID_ERR_INVALID, "bad location");
    if (n == 0) return AID_OK;
    EngineCall call(e, nullptr, true, kDrainLast);
    if (call.rc) return call.rc;
    HashIndex &ix = e->idx;
    hipStream_t s = call.s;
    // the largest track id; 0xFFFFFFFF is K5's empty-slot marker (with d = -1 also the empty (track, d) key), and
    // id + 1 would wrap to 0: rejected before anything is grown or copied, as in aid_index_add_track
    uint32_t top = 0, low = 0xFFFFFFFFu;  // low: the live index's disjointness rule (aidfp_live_plan.h)
    if (location == AID_PCM_HOST) {
        for (int64_t i = 0; i < n; ++i) {
            top = std::max(top, track[i]);
            low = std::min(low, track[i]);
        }
    } else {
        // device track ids: one max-reduction via a host copy of the track column
        std::vector<uint32_t> tr(n);
        HIP_TRY(hipMemcpy(tr.data(), track, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; ++i) {
            top = std::max(top, tr[i]);
            low = std::min(low, tr[i]);
        }
    }
    if (top == 0xFFFFFFFFu) return fail(AID_ERR_INVALID, "aid_index_add_postings: bad track id");
    const uint32_t mx = top + 1;
    if (int rc = grow_postings(e, (size_t)(ix.n_post + n), s)) return rc;
    if (int rc = ensure_tracks(e, mx, s)) return rc;
    const hipMemcpyKind k = location == AID_PCM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    HIP_TRY(hipMemcpyAsync(ix.p_hash.p + ix.n_post, hash, n * sizeof(uint32_t), k, s));
    HIP_TRY(hipMemcpyAsync(ix.p_track.p + ix.n_post, track, n * sizeof(uint32_t), k, s));
    HIP_TRY(hipMemcpyAsync(ix.p_t.p + ix.n_post, t, n * sizeof(uint32_t), k, s));
    HIP_TRY(hipStreamSynchronize(s));
    ix.n_post += n;
    ix.note_append(low);
    return AID_OK;
}

int aid_index_add_track(aid_engine *e, uint32_t track) {
    if (!e) return fail(AID_ERR_INVALID, "null engine");
    if (track == 0xFFFFFFFFu) return fail(AID_ERR_INVALID, "aid_index_add_track: bad track id");
    EngineCall call(e, nullptr, false, kDrainLast);
    if (call.rc) return call.rc;
    if (int rc = ensure_tracks(e, track + 1, call.s)) return rc;
    HIP_TRY(hipStreamSynchronize(call.s));
    return AID_OK;
}

int aid_index_remove(aid_engine *e, uint32_t track) {
    EngineCall call(e);  // no wait: a removal between the batches of an asynchronous ingest does not serialise it
    if (call.rc) return call.rc;
    HashIndex &ix = e->idx;
    if (track >= ix.n_tracks || ix.h_tomb[track]) return fail(AID_ERR_INVALID, "track not indexed");
    ix.h_tomb[track] = 1;
    ++ix.n_removed;
    ++ix.main->tomb_since_build;  // the CSRs still hold its postings until their next builds
    if (ix.delta) ++ix.delta->tomb_since_build;
    HIP_TRY(hipMemcpy(ix.tomb.p + track, &ix.h_tomb[track], 1, hipMemcpyHostToDevice));
    return AID_OK;
}

int aid_index_compact(aid_engine *e, int64_t *n_removed) {
    EngineCall call(e, nullptr, true);
    if (call.rc) return call.rc;
    HashIndex &ix = e->idx;
    hipStream_t s = call.s;
    if (n_removed) *n_removed = 0;
    if (ix.n_removed == 0 || ix.n_post == 0) return AID_OK;
    if (ix.n_post > 0xFFFFFFFFll) return fail(AID_ERR_INVALID, "index holds more than 2^32 postings");
    if (int rc = EngineCall::wait_last(e, s, kDrainLast)) return rc;
    const int64_t nb = (ix.n_post + 1023) / 1024;
    DevBuf<uint32_t> cnt, off, tmp, nh, ntr, nt;  // scratch: freed on every return path
    HIP_TRY(cnt.reserve((size_t)nb));
    HIP_TRY(off.reserve((size_t)nb));
    HIP_TRY(tmp.reserve(4 * ((size_t)nb / 1024 + 2) + 4096));
    HIP_TRY(nh.reserve((size_t)ix.n_post));
    HIP_TRY(ntr.reserve((size_t)ix.n_post));
    HIP_TRY(nt.reserve((size_t)ix.n_post));
    launch_compact(ix.p_hash.p, ix.p_track.p, ix.p_t.p, ix.n_post, ix.tomb.p, ix.n_tracks, cnt.p, off.p, tmp.p, nh.p,
                   ntr.p, nt.p, s);
    HIP_TRY(hipGetLastError());
    uint32_t last_off = 0, last_cnt = 0;
    HIP_TRY(hipMemcpyAsync(&last_off, off.p + (nb - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&last_cnt, cnt.p + (nb - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const int64_t live = (int64_t)last_off + last_cnt;
    if (n_removed) *n_removed = ix.n_post - live;
    std::swap(ix.p_hash, nh);
    std::swap(ix.p_track, ntr);
    std::swap(ix.p_t, nt);  // the old planes are released with the scratch buffers
    ix.n_post = live;  // tombstones stay: removed ids are never reused, and the CSR skips nothing new
    ix.drop_main(kFallCompact);
    return AID_OK;
}

// K4: the CSR (offsets, postings, signatures) of segment `seg` built from the stored postings [first, first + count).
// Engine lock held, the append settled and last_stream drained. A segment a ticket still holds is left to it and
// a fresh one built (aidfp.h, "Ingest while serving")
static int build_csr(aid_engine *e, std::shared_ptr<CsrSegment> &seg, int64_t first, int64_t count) {
    HashIndex &ix = e->idx;
    hipStream_t s = e->own_stream;
    if (ix.n_post > 0xFFFFFFFFll) return fail(AID_ERR_INVALID, "index holds more than 2^32 postings");
    if (seg.use_count() > 1) seg = std::make_shared<CsrSegment>();
    CsrSegment &g = *seg;
    const uint32_t *p_hash = ix.p_hash.p + first, *p_track = ix.p_track.p + first, *p_t = ix.p_t.p + first;
    const size_t K = (size_t)index_keys() + 1;
    HIP_TRY(g.cnt.reserve(K));
    HIP_TRY(g.off.reserve(K));
    HIP_TRY(ix.scan_tmp.reserve(4 * (K / 1024 + 2) + 4096));
    HIP_TRY(g.post.reserve((size_t)std::max<int64_t>(count, 1)));
    // + 8: K5's LDS path reads the signatures in aligned chunks of 4 or 8; a record's last chunk may reach past the end
    HIP_TRY(g.sig.reserve((size_t)std::max<int64_t>(count, 1) + 8));
    if (ix.n_tracks == 0) HIP_TRY(ix.tomb.reserve(1024));
    HIP_TRY(hipMemsetAsync(g.cnt.p, 0, K * sizeof(uint32_t), s));
    HIP_TRY(ix.nz.reserve(1));
    HIP_TRY(hipMemsetAsync(ix.nz.p, 0, sizeof(unsigned long long), s));
    if (ix.k4_build == K4Build::kRadix && count > 0) {
        // sort build (index_sort.hip): stable radix sort of (key27, track | t << 32) -> run ends -> max-scan
        const size_t np = (size_t)count;
        HIP_TRY(ix.srt_scratch.reserve(radix_scratch_u32(count)));
        HIP_TRY(ix.srt_k0.reserve(np));
        HIP_TRY(ix.srt_k1.reserve(np));
        HIP_TRY(ix.srt_v.reserve(np));
        uint64_t *sorted = nullptr;
        {
            ProfScope ps(e, AID_K_INDEX_BUILD, s);
            HIP_TRY(launch_index_sort_build(p_hash, p_track, p_t, count, ix.n_removed ? ix.tomb.p : nullptr, ix.n_tracks,
                                            ix.srt_k0.p, ix.srt_k1.p, ix.srt_v.p, g.post.p, ix.srt_scratch.p, g.cnt.p,
                                            g.off.p, ix.nz.p, &sorted, g.sig.p, ix.k4_rank, s));
            if (sorted == ix.srt_v.p) std::swap(ix.srt_v, g.post);  // the CSR's post array is where the sort ended
        }
    } else {
        launch_index_count(p_hash, p_track, count, ix.tomb.p, ix.n_tracks, g.cnt.p, s);
        launch_count_nonzero(g.cnt.p, (int64_t)K, ix.nz.p, s);
        launch_scan(g.cnt.p, g.off.p, (int64_t)K, ix.scan_tmp.p, s);
        HIP_TRY(hipMemcpyAsync(g.cnt.p, g.off.p, K * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        launch_index_scatter(p_hash, p_track, p_t, count, ix.tomb.p, ix.n_tracks, g.cnt.p, g.post.p, s);
        launch_make_sig(g.post.p, count, g.sig.p, s);  // (only the first n_indexed are read)
    }
    HIP_TRY(hipGetLastError());
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, g.off.p + (K - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    g.covered = count;
    g.n_indexed = total;
    g.tomb_since_build = 0;  // the build skipped every removed track's postings
    // the sort's double buffers are 16 B per posting (15 GB at the 100k-track catalog): kept for the next build
    // of a small index (a store + query cycle rebuilds it, or its delta), released above 1 GiB
    if ((ix.srt_k0.n + ix.srt_k1.n) * 4 + ix.srt_v.n * 8 + ix.srt_scratch.n * 4 > ((size_t)1 << 30)) {
        ix.srt_k0.release();
        ix.srt_k1.release();
        ix.srt_v.release();
        ix.srt_scratch.release();
    }
    return AID_OK;
}

static void empty_delta(HashIndex &ix) {
    if (!ix.delta) return;
    if (ix.delta.use_count() > 1) ix.delta = std::make_shared<CsrSegment>();  // a ticket keeps the old one
    ix.delta->covered = ix.delta->n_indexed = ix.delta->tomb_since_build = 0;
}

// The full build: main over every stored posting, the delta emptied
static int build_main(aid_engine *e) {
    HashIndex &ix = e->idx;
    if (int rc = build_csr(e, ix.main, 0, ix.n_post)) return rc;
    ix.csr_current = true;
    ix.tracks_at_main = ix.n_tracks;
    ++ix.st_main_builds;
    empty_delta(ix);
    return AID_OK;
}

// the delta over the tail [n_main, n_post): K4 unchanged, on the planes from n_main on
static int build_delta(aid_engine *e) {
    HashIndex &ix = e->idx;
    if (!ix.delta) ix.delta = std::make_shared<CsrSegment>();
    if (int rc = build_csr(e, ix.delta, ix.main->covered, ix.n_post - ix.main->covered)) return rc;
    ++ix.st_delta_builds;
    return AID_OK;
}

// The fold (K4m, index_merge.hip): the delta, built over the whole tail first, merged into main without a sort. The
// merged CSR goes into a second set of buffers (the main the last fold replaced, if no ticket holds it) and becomes
// main. With no track removed since main's build it equals the full build's CSR bit for bit; removed tracks' postings
// are carried along and check_tomb stays set for them
static int fold_delta(aid_engine *e) {
    HashIndex &ix = e->idx;
    hipStream_t s = e->own_stream;
    if (ix.n_post > 0xFFFFFFFFll) return fail(AID_ERR_INVALID, "index holds more than 2^32 postings");
    if (!ix.delta || ix.delta->covered != ix.n_post - ix.main->covered)
        if (int rc = build_delta(e)) return rc;
    std::shared_ptr<CsrSegment> out = ix.spare && ix.spare.use_count() == 1 ? std::move(ix.spare) : std::make_shared<CsrSegment>();
    ix.spare.reset();
    const CsrSegment &m = *ix.main, &d = *ix.delta;
    const int64_t n = m.n_indexed + d.n_indexed;
    const size_t K = (size_t)index_keys() + 1;
    const int n_tiles = (int)(index_keys() / kMergeTileKeys);
    HIP_TRY(out->off.reserve(K));
    HIP_TRY(out->post.reserve((size_t)std::max<int64_t>(n, 1)));
    HIP_TRY(out->sig.reserve((size_t)std::max<int64_t>(n, 1) + 8));  // + 8: as build_csr
    HIP_TRY(ix.mrg_tot.reserve((size_t)n_tiles));
    std::vector<uint32_t> tot((size_t)n_tiles);
    std::vector<MergeItem> items;
    {
        ProfScope ps(e, AID_K_INDEX_MERGE, s);
        launch_csr_merge_offsets(m.off.p, d.off.p, out->off.p, (int64_t)K, s);
        launch_csr_merge_totals(m.off.p, d.off.p, ix.mrg_tot.p, n_tiles, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(tot.data(), ix.mrg_tot.p, tot.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        items.resize((size_t)plan_merge(tot.data(), n_tiles, kMergeItemPosts, nullptr));
        plan_merge(tot.data(), n_tiles, kMergeItemPosts, items.data());
        if (!items.empty()) {
            static_assert(sizeof(MergeItem) == 3 * sizeof(uint32_t), "MergeItem is three words");
            HIP_TRY(ix.mrg_items.reserve(3 * items.size()));
            HIP_TRY(hipMemcpyAsync(ix.mrg_items.p, items.data(), items.size() * sizeof(MergeItem), hipMemcpyHostToDevice, s));
            launch_csr_merge(ix.mrg_items.p, (int64_t)items.size(), m.off.p, m.post.p, m.sig.p, d.off.p, d.post.p, d.sig.p,
                             out->post.p, out->sig.p, s);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipStreamSynchronize(s));  // (the items are pageable host memory)
    out->covered = ix.n_post;
    out->n_indexed = n;
    out->tomb_since_build = m.tomb_since_build + d.tomb_since_build;
    std::shared_ptr<CsrSegment> old = std::move(ix.main);
    ix.main = std::move(out);
    if (old.use_count() == 1) ix.spare = std::move(old);  // no ticket holds it: the next fold's destination
    empty_delta(ix);
    ix.csr_current = true;
    ix.tracks_at_main = ix.n_tracks;
    ++ix.st_folds;
    return AID_OK;
}

int aid_index_finalize(aid_engine *e) {
    EngineCall call(e, nullptr, true, kDrainLast);
    if (call.rc) return call.rc;
    HashIndex &ix = e->idx;
    // always one CSR over everything: a live delta is folded, or, with a track removed since main's build, rebuilt
    // with main (the full build drops that track's postings; a fold would carry them)
    if (ix.live_cap > 0 && ix.csr_current && ix.n_post > ix.main->covered) {
        if (ix.main->tomb_since_build == 0) return fold_delta(e);
        ++ix.st_fallback[kFallRemoved];
    }
    return build_main(e);
}

int aid_index_live(aid_engine *e, int64_t max_delta_postings) {
    if (max_delta_postings < 0) return fail(AID_ERR_INVALID, "aid_index_live: max_delta_postings must be >= 0");
    EngineCall call(e, nullptr, true, kDrainLast);
    if (call.rc) return call.rc;
    HashIndex &ix = e->idx;
    if (max_delta_postings == ix.live_cap) return AID_OK;
    if (ix.csr_current && ix.n_post > ix.main->covered)  // a change while a delta is live folds first
        if (int rc = fold_delta(e)) return rc;
    ix.live_cap = max_delta_postings;
    if (ix.live_cap == 0) {  // (a ticket that holds the delta keeps it until it is collected)
        ix.delta.reset();
        ix.spare.reset();
    }
    return AID_OK;
}

int aid_index_live_stats(aid_engine *e, int64_t *out, int32_t n) {
    if (n < 0 || (n > 0 && !out)) return fail(AID_ERR_INVALID, "aid_index_live_stats: bad argument");
    EngineCall call(e, nullptr, true);
    if (call.rc) return call.rc;
    const HashIndex &ix = e->idx;
    int64_t v[kLiveStatsWords] = {ix.st_main_builds,
                                  ix.st_delta_builds,
                                  ix.st_folds,
                                  ix.csr_current ? ix.main->covered : 0,
                                  ix.csr_current ? ix.n_post - ix.main->covered : 0,
                                  (int64_t)ix.tracks_at_main};
    for (int r = 0; r < kLiveFallbacks; ++r) v[6 + r] = ix.st_fallback[r];
    for (int i = 0; i < n && i < kLiveStatsWords; ++i) out[i] = v[i];
    return AID_OK;
}

int aid_index_stats(aid_engine *e, int64_t *n_postings, int64_t *n_live, uint32_t *n_tracks) {
    EngineCall call(e, nullptr, true);  // no wait: polled between the batches of an asynchronous ingest
    if (call.rc) return call.rc;
    const HashIndex &ix = e->idx;
    if (n_postings) *n_postings = ix.n_post;
    // both segments' postings; stale (-1) also while stored postings wait for their delta build
    const int64_t tail = ix.csr_current ? ix.n_post - ix.main->covered : 0;
    const bool stale = !ix.csr_current || (tail > 0 && (!ix.delta || ix.delta->covered != tail));
    if (n_live) *n_live = stale ? -1 : ix.main->n_indexed + (tail > 0 ? ix.delta->n_indexed : 0);
    if (n_tracks) *n_tracks = ix.n_tracks;
    return AID_OK;
}

int aid_index_export(aid_engine *e, uint32_t *hash, uint32_t *track, uint32_t *t, int64_t first, int64_t count,
                     int32_t location) {
    if (!e || first < 0 || count < 0) return fail(AID_ERR_INVALID, "aid_index_export: bad range");
    EngineCall call(e, nullptr, true);
    if (call.rc) return call.rc;
    const HashIndex &ix = e->idx;
    if (first + count > ix.n_post) return fail(AID_ERR_INVALID, "aid_index_export: bad range");
    if (count == 0) return AID_OK;
    // the posting append of aid_index_add_extracted runs asynchronously on the caller's stream
    if (int rc = EngineCall::wait_last(e, call.s, kDrainLast)) return rc;
    const hipMemcpyKind k = location == AID_PCM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    HIP_TRY(hipMemcpy(hash, ix.p_hash.p + first, count * sizeof(uint32_t), k));
    HIP_TRY(hipMemcpy(track, ix.p_track.p + first, count * sizeof(uint32_t), k));
    HIP_TRY(hipMemcpy(t, ix.p_t.p + first, count * sizeof(uint32_t), k));
    return AID_OK;
}

int aid_index_checksum(aid_engine *e, int64_t first, int64_t count, uint64_t *out) {
    if (!e || !out || first < 0 || count < 0) return fail(AID_ERR_INVALID, "aid_index_checksum: bad range");
    EngineCall call(e, nullptr, true);
    if (call.rc) return call.rc;
    HashIndex &ix = e->idx;
    hipStream_t s = call.s;
    if (first + count > ix.n_post) return fail(AID_ERR_INVALID, "aid_index_checksum: bad range");
    if (int rc = EngineCall::wait_last(e, s, kDrainLast)) return rc;
    HIP_TRY(ix.chk.reserve(1));
    HIP_TRY(hipMemsetAsync(ix.chk.p, 0, sizeof(unsigned long long), s));
    launch_index_checksum(ix.p_hash.p, ix.p_track.p, ix.p_t.p, first, count, ix.chk.p, s);
    HIP_TRY(hipGetLastError());
    unsigned long long v = 0;
    HIP_TRY(hipMemcpyAsync(&v, ix.chk.p, sizeof(v), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *out = (uint64_t)v;
    return AID_OK;
}

int aid_index_csr_export(aid_engine *e, uint32_t *offsets, int64_t n_offsets, uint64_t *posts, int64_t cap,
                         int64_t *n_out) {
    if (!e || !n_out || n_offsets < 0 || cap < 0 || (!offsets && n_offsets > 0) || (!posts && cap > 0))
        return fail(AID_ERR_INVALID, "aid_index_csr_export: bad argument");
    EngineCall call(e);
    if (call.rc) return call.rc;
    const HashIndex &ix = e->idx;
    if (!ix.csr_current) return fail(AID_ERR_STATE, "aid_index_csr_export: the index is not finalized");
    if (ix.n_post > ix.main->covered)
        return fail(AID_ERR_STATE, "aid_index_csr_export: postings stored since the last build are in the live delta "
                                   "segment (aid_index_live); call aid_index_finalize for one CSR over everything");
    if (int rc = EngineCall::wait_last(e, call.s, kDrainLast)) return rc;
    const int64_t K = (int64_t)index_keys() + 1;
    *n_out = ix.main->n_indexed;
    if (offsets && n_offsets > 0) {
        if (n_offsets < K) return fail(AID_ERR_INVALID, "aid_index_csr_export: offsets need 2^26 + 1 entries");
        HIP_TRY(hipMemcpy(offsets, ix.main->off.p, K * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    if (posts && cap > 0) {
        const int64_t n = std::min<int64_t>(cap, ix.main->n_indexed);
        if (n > 0) HIP_TRY(hipMemcpy(posts, ix.main->post.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    return AID_OK;
}

static const char kIdxMagic[8] = {'A', 'I', 'D', 'F', 'P', 'I', 'X', '1'};

int aid_index_save(aid_engine *e, const char *path) {
    if (!e || !path) return fail(AID_ERR_INVALID, "null argument");
    EngineCall call(e, nullptr, true, kDrainLast);
    if (call.rc) return call.rc;
    HashIndex &ix = e->idx;
    FILE *f = std::fopen(path, "wb");
    if (!f) return fail(AID_ERR_INVALID, std::string("cannot open ") + path);
    int64_t hdr[6] = {AID_ABI_VERSION, e->cfg.sample_rate, e->cfg.hop, ix.n_post, (int64_t)ix.n_tracks, 0};
    bool ok = std::fwrite(kIdxMagic, 1, 8, f) == 8 && std::fwrite(hdr, sizeof(hdr), 1, f) == 1;
    std::vector<uint32_t> buf((size_t)std::min<int64_t>(ix.n_post, 1 << 24));
    DevBuf<uint32_t> *cols[3] = {&ix.p_hash, &ix.p_track, &ix.p_t};
    for (int c = 0; c < 3 && ok; ++c)
        for (int64_t o = 0; o < ix.n_post && ok; o += (int64_t)buf.size()) {
            const int64_t m = std::min<int64_t>((int64_t)buf.size(), ix.n_post - o);
            if (hipMemcpy(buf.data(), cols[c]->p + o, m * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) ok = false;
            else ok = std::fwrite(buf.data(), sizeof(uint32_t), m, f) == (size_t)m;
        }
    if (ok && ix.n_tracks) ok = std::fwrite(ix.h_tomb.data(), 1, ix.n_tracks, f) == ix.n_tracks;
    ok = (std::fclose(f) == 0) && ok;
    if (!ok) return fail(AID_ERR_DEVICE, std::string("failed writing ") + path);
    return AID_OK;
}

int aid_index_load(aid_engine *e, const char *path) {
    if (!e || !path) return fail(AID_ERR_INVALID, "null argument");
    EngineCall call(e, nullptr, true);
    if (call.rc) return call.rc;
    HashIndex &ix = e->idx;
    // Everything is validated and read into scratch buffers first; the engine's index changes only
    // once the whole file has been read (a failed load leaves the previous index untouched).
    struct File {
        FILE *f;
        ~File() {
            if (f) std::fclose(f);
        }
    } file{std::fopen(path, "rb")};
    FILE *f = file.f;
    if (!f) return fail(AID_ERR_INVALID, std::string("cannot open ") + path);
    char magic[8];
    int64_t hdr[6];
    if (std::fread(magic, 1, 8, f) != 8 || std::memcmp(magic, kIdxMagic, 8) != 0 || std::fread(hdr, sizeof(hdr), 1, f) != 1)
        return fail(AID_ERR_INVALID, "not an aidfp index file");
    if (hdr[0] != AID_ABI_VERSION) return fail(AID_ERR_INVALID, "index file written by another ABI version");
    if (hdr[1] != e->cfg.sample_rate || hdr[2] != e->cfg.hop)
        return fail(AID_ERR_INVALID, "index sample_rate/hop differ from the engine's");
    const int64_t n = hdr[3];
    if (n < 0 || n > 0xFFFFFFFFll || hdr[4] < 0 || hdr[4] > 0xFFFFFFFFll || hdr[5] != 0)
        return fail(AID_ERR_INVALID, "corrupt index header");
    const uint32_t nt = (uint32_t)hdr[4];
    if (std::fseek(f, 0, SEEK_END) != 0) return fail(AID_ERR_INVALID, "cannot size index file");
    const long long fsize = (long long)ftello(f);
    const long long want = 8 + (long long)sizeof(hdr) + 12ll * n + (long long)nt;
    if (fsize != want) return fail(AID_ERR_INVALID, fsize < want ? "truncated index file" : "index file has trailing bytes");
    if (std::fseek(f, 8 + (long)sizeof(hdr), SEEK_SET) != 0) return fail(AID_ERR_INVALID, "cannot read index file");
    if (int rc = EngineCall::wait_last(e, call.s, kDrainLast)) return rc;
    DevBuf<uint32_t> cols[3];
    std::vector<uint32_t> buf((size_t)std::min<int64_t>(std::max<int64_t>(n, 1), 1 << 24));
    for (int c = 0; c < 3; ++c) {
        HIP_TRY(cols[c].reserve((size_t)std::max<int64_t>(n, 1)));
        for (int64_t o = 0; o < n; o += (int64_t)buf.size()) {
            const int64_t m = std::min<int64_t>((int64_t)buf.size(), n - o);
            if (std::fread(buf.data(), sizeof(uint32_t), m, f) != (size_t)m) return fail(AID_ERR_INVALID, "truncated index file");
            HIP_TRY(hipMemcpy(cols[c].p + o, buf.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
    }
    std::vector<uint8_t> tomb(nt);
    if (nt && std::fread(tomb.data(), 1, nt, f) != nt) return fail(AID_ERR_INVALID, "truncated index file");
    DevBuf<uint8_t> dtomb;
    HIP_TRY(dtomb.reserve(std::max<size_t>(nt, 1024)));
    if (nt) HIP_TRY(hipMemcpy(dtomb.p, tomb.data(), nt, hipMemcpyHostToDevice));
    // commit: swap the new planes in (the old ones are released with the scratch)
    std::swap(ix.tomb, dtomb);
    std::swap(ix.p_hash, cols[0]);
    std::swap(ix.p_track, cols[1]);
    std::swap(ix.p_t, cols[2]);
    ix.h_tomb = std::move(tomb);
    ix.n_removed = (int64_t)ix.h_tomb.size() - std::count(ix.h_tomb.begin(), ix.h_tomb.end(), 0);
    ix.n_tracks = nt;
    ix.n_post = n;
    ix.main->tomb_since_build = 0;
    ix.drop_main(kFallLoad);
    return AID_OK;
}

}  // extern "C"

int ensure_index(aid_engine *e) {
    HashIndex &ix = e->idx;
    if (ix.csr_current && ix.live_cap == 0) return AID_OK;
    if (int rc = settle_postings(e)) return rc;
    const LiveStep step = live_step(ix.live_state());
    if (step == kLiveKeep) return AID_OK;
    if (int rc = EngineCall::enter(e, e->own_stream, true, kDrainLast)) return rc;
    if (step == kLiveDelta) return build_delta(e);
    return step == kLiveFold ? fold_delta(e) : build_main(e);
}
