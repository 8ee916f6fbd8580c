// query.cpp -- the query half of libaidfp.so's host side: K5's orchestration, the query entry points (synchronous,
// and the submit / collect pair with its tickets) and the batched exact lane. Extraction lives in extract.cpp, the
// index in index_host.cpp (K5 reads it through HashIndex::view()); engine_internal.h is what the host files share.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "engine_internal.h"

// ---------------------------------------------------------------- K5, the matcher: host orchestration
//
// Every query is routed by its own exact vote count (k_query_votes). One LDS pass (k_match_lds) takes the whole
// batch in the same round trip as the vote counts: it answers the queries with <= kLdsMaxVotes votes (2^18 over the
// 2^16 4-bit counters of its filter, aidfp_layout.h) and hands the others back with nrows = -reason, reasons 1 to 5
// (index.hip): 1 too many votes (no LDS run), 2 its vote table, 3 its distinct set, 4 its candidate tracks or 5 its
// row staging overflowed. The handed-back queries run on the global-histogram path (K5a, K5h, K5b), whose histogram
// is sized for the votes that pass K5a's 2^20-bit seen filter (all but the distinct bits: v - m(1 - e^{-v/m})) at
// kForwardedPerBucket per bucket, where a chance bucket reaching min_match - 1 has probability ~1e-5. Measured on
// config 4: 16 bits 0.295 s against 0.383 s at 19 bits (sizing for all votes spreads K5a's atomics over HBM), and
// two key partitions once the filter saturates (> 2^18 votes: 46.6k -> 60.2k clips/s). A query that overflows the
// global path too is run again with 4x the buckets. History and the A/Bs: DESIGN.md 0d, 0e and 4b.
//
// The three phases below are the only K5 host code: run_queries (synchronous) runs them back to back, submit_locked
// runs the first and aid_query_windows_collect the other two.
constexpr double kForwardedPerBucket = 2.0;  // forwarded votes (1-bit filter estimate) per global histogram bucket

// Phase 1, no synchronisation: the vote counts of nq queries whose records are at device ranges (qstart_dev /
// qcount_dev), with `lds` the LDS pass, and the copies of starts, counts, votes and the pass's results into `h`.
// rec_cap: elements of `recs` (the CSR range cache the vote count writes for the LDS pass has one entry per record
// index). want_rows = false (device mode): the rows stay in sc.rows. have_starts: h.meta already holds the starts.
// The pass reads the CSR segment `ix` and works in the scratch `sc` (one per segment: engine_internal.h).
static int k5_enqueue(aid_engine *e, const CsrView &ix, K5Scratch &sc, const uint64_t *recs, const int64_t *qstart_dev,
                      const int64_t *qcount_dev, int nq, int64_t rec_cap, bool lds, bool want_rows, K5Host &h,
                      hipStream_t s, bool have_starts = false) {
    const int mr = e->cfg.max_results;
    HIP_TRY(sc.rows.reserve((size_t)std::max(nq, 1) * mr * 5));
    HIP_TRY(sc.nrows.reserve((size_t)std::max(nq, 1)));
    HIP_TRY(sc.votes.reserve((size_t)nq));
    if (lds) HIP_TRY(sc.ranges.reserve((size_t)std::max<int64_t>(rec_cap, 1)));
    HIP_TRY(h.meta.reserve((size_t)3 * nq));
    if (lds) HIP_TRY(h.nrows.reserve((size_t)nq));
    if (lds && want_rows) HIP_TRY(h.rows.reserve((size_t)nq * mr * 5));
    int64_t *p_start = h.meta.p, *p_count = p_start + nq, *p_votes = p_count + nq;
    if (!have_starts) HIP_TRY(hipMemcpyAsync(p_start, qstart_dev, nq * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(p_count, qcount_dev, nq * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    launch_query_votes(recs, qstart_dev, qcount_dev, nq, ix.offsets, sc.votes.p, lds ? sc.ranges.p : nullptr, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(p_votes, sc.votes.p, nq * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (!lds) return AID_OK;
    {
        ProfScope ps(e, AID_K_MATCH, s, true);
        launch_match_lds(recs, qstart_dev, qcount_dev, nq, ix.offsets, ix.post, ix.tomb, ix.n_tracks, e->cfg.min_match,
                         mr, sc.rows.p, sc.nrows.p, ix.check_tomb, sc.votes.p, ix.sig, sc.ranges.p, s);
    }
    HIP_TRY(hipGetLastError());
    if (want_rows)
        HIP_TRY(hipMemcpyAsync(h.rows.p, sc.rows.p, (size_t)nq * mr * sizeof(aid_match_row), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h.nrows.p, sc.nrows.p, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    return AID_OK;
}

// Phase 2, once the caller has waited for phase 1: the statistics of the nq queries (each counted here and nowhere
// else), nrows[q] of the queries the LDS pass answered, and in `todo` the ones it handed back (all, without `lds`).
// first_pass = false for the live index's delta pass: a query is counted once, its votes, records, reads and
// hand-backs in every pass.
static void k5_tally(aid_engine *e, const K5Host &h, int nq, bool lds, int32_t *nrows, std::vector<int> &todo,
                     bool first_pass = true) {
    const int64_t *counts = h.meta.p + nq, *votes = counts + nq;
    todo.clear();
    if (first_pass) e->st_queries += nq;
    for (int q = 0; q < nq; ++q) {
        e->st_votes += votes[q];
        e->st_records += counts[q];
        if (!lds) {
            todo.push_back(q);
            continue;
        }
        if (votes[q] <= kLdsMaxVotes) {  // the pass ran it: two enumerations (counting, then the exact inserts)
            e->st_sig_reads += 2 * votes[q];
            ++e->st_q_lds;
        }
        const int32_t n = h.nrows.p[q];
        if (n < 0) {
            todo.push_back(q);
            ++e->st_fb_reason[std::min(-n, 5) - 1];
        } else {
            nrows[q] = n;
        }
    }
}

// Phase 3: the global-histogram path, against the CSR segment `ix`, over the queries `todo` of a batch whose starts,
// counts and votes are on the host, until each has its rows (rows + q * max_results, or with rows == nullptr its slot
// of `dev_rows`, the pass's K5Scratch::rows) and
// nrows[q]. Ends with the stream drained. vmax sizes the histogram and the key partitions: run_queries passes the
// maximum over its whole batch, collect the maximum over the handed-back queries only (each as before the phases
// were shared; making them one changes a fallback pass's histogram size, so its speed).
static int k5_global(aid_engine *e, const CsrView &ix, int32_t *dev_rows, const uint64_t *recs, const int64_t *h_start,
                     const int64_t *h_count, const int64_t *h_votes, int64_t vmax, std::vector<int> todo,
                     aid_match_row *rows, int32_t *nrows, hipStream_t s) {
    const int mr = e->cfg.max_results;
    const double votes = (double)vmax;
    const int parts = e->k5_parts > 0 ? e->k5_parts : votes > (double)(1 << 18) ? 2 : 1;
    const double m_seen = (double)(1 << 20), vp = votes / parts;
    const double fwd = parts * (vp - m_seen * (1.0 - std::exp(-vp / m_seen)));
    int bits = 15;
    while (bits < 24 && (double)(1ull << bits) < fwd / kForwardedPerBucket) ++bits;
    for (int attempt = 1; !todo.empty(); ++attempt, bits += 2) {
        for (int q : todo) e->st_post_reads += h_votes[q] * (parts + 1);  // K5a once per key partition, K5b once
        e->st_q_global += (int64_t)todo.size();
        if (bits > 26) return fail(AID_ERR_STATE, "query vote table overflow (too many candidate votes)");
        const size_t H = (size_t)1 << bits;
        const int batch = (int)std::max<size_t>(1, std::min<size_t>(e->k5_batch, ((size_t)4 << 30) / (H * 4)));
        HIP_TRY(e->q_hist.reserve((size_t)std::min<int>((int)todo.size(), batch) * H));
        HIP_TRY(e->q_hot.reserve((size_t)std::min<int>((int)todo.size(), batch) * (H / 32)));
        if (e->hist_zero_cap != e->q_hist.n) {  // fresh allocation; K5h re-zeroes its rows afterwards
            HIP_TRY(hipMemsetAsync(e->q_hist.p, 0, e->q_hist.n * sizeof(uint32_t), s));
            e->hist_zero_cap = e->q_hist.n;
        }
        const std::vector<int> &order = todo;
        const int n = (int)order.size();
        // gather the queries' ranges into q_gsc; their rows and counts come out in q_grows
        HIP_TRY(e->q_gsc.reserve(2 * order.size()));
        std::vector<int64_t> st(order.size()), ct(order.size());
        for (size_t i = 0; i < order.size(); ++i) { st[i] = h_start[order[i]]; ct[i] = h_count[order[i]]; }
        HIP_TRY(hipMemcpyAsync(e->q_gsc.p, st.data(), st.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(e->q_gsc.p + order.size(), ct.data(), ct.size() * sizeof(int64_t),
                               hipMemcpyHostToDevice, s));
        const int64_t *qs = e->q_gsc.p, *qc = e->q_gsc.p + order.size();
        HIP_TRY(e->q_grows.reserve(order.size() * ((size_t)mr * 5 + 1)));
        int32_t *out_rows = e->q_grows.p, *out_n = out_rows + (size_t)order.size() * mr * 5;
        // from the second global attempt on, the distinct (slot, t_q) sets live in HBM (2^dbits entries per query,
        // 4x more per attempt): a query that overflowed k_vote_final's LDS set is a long one with a strong match
        // (FPSPEC v1 7), which more histogram buckets do not help
        const int dbits = attempt >= 2 ? std::min(12 + 2 * attempt, 26) : 0;
        int dbatch = batch;
        if (dbits) {
            dbatch = (int)std::max<size_t>(1, std::min<size_t>((size_t)batch, ((size_t)1 << 30) / ((size_t)4 << dbits)));
            HIP_TRY(e->q_dset.reserve((size_t)std::min(dbatch, n) << dbits));
        }
        for (int q0 = 0; q0 < n; q0 += dbatch) {
            const int nb = std::min(dbatch, n - q0);
            if (dbits) HIP_TRY(hipMemsetAsync(e->q_dset.p, 0xFF, ((size_t)nb << dbits) * sizeof(uint32_t), s));
            // K5a, K5h, K5b, each with its own dispatch-attached events when profiled
            for (int stage = 1; stage <= 3; ++stage) {
                ProfScope ps(e, stage == 1 ? AID_K_VOTE_HIST : stage == 2 ? AID_K_HOT_SCAN : AID_K_VOTE_FINAL, s, true);
                launch_query(recs, qs + q0, qc + q0, nb, ix.offsets, ix.post, ix.tomb, ix.n_tracks, e->cfg.min_match,
                             mr, e->q_hist.p, bits, e->q_hot.p, out_rows + (size_t)q0 * mr * 5, out_n + q0,
                             ix.check_tomb, parts, stage, dbits ? e->q_dset.p : nullptr, dbits, s);
            }
            HIP_TRY(hipGetLastError());
        }
        std::vector<int32_t> got_n(n);
        std::vector<aid_match_row> got;
        if (rows) {
            got.resize((size_t)n * mr);
            HIP_TRY(hipMemcpyAsync(got.data(), out_rows, (size_t)n * mr * sizeof(aid_match_row), hipMemcpyDeviceToHost, s));
        } else {  // device mode: the batch's rows go to their queries' slots of q_rows
            HIP_TRY(e->x_order.reserve(order.size()));
            HIP_TRY(hipMemcpyAsync(e->x_order.p, order.data(), order.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
            launch_rows_scatter(out_rows, e->x_order.p, n, mr, dev_rows, s);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(got_n.data(), out_n, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        std::vector<int> again;
        for (int i = 0; i < n; ++i) {
            const int q = order[i];
            if (got_n[i] < 0) {
                again.push_back(q);
                continue;
            }
            nrows[q] = got_n[i];
            if (rows) std::memcpy(rows + (size_t)q * mr, got.data() + (size_t)i * mr, (size_t)mr * sizeof(aid_match_row));
        }
        todo.swap(again);
    }
    return AID_OK;
}

// K5 over nq queries, synchronously. rows == nullptr: device mode, every query's rows end in e->q.rows
// ([nq][max_results][5] int32); nrows (host) is always filled. Over the live index (a delta that holds postings) both
// segments' LDS passes are queued before the one wait, each segment resolves its own hand-backs, and every query's
// two row lists are merged by merge_rows (aidfp_live_plan.h): on the host, or in device mode by k_rows_merge, so that
// K8b reads final rows from e->q.rows. A query is final only when both segments have answered it.
static int run_queries(aid_engine *e, const uint64_t *recs, const int64_t *qstart_dev, const int64_t *qcount_dev,
                       int nq, int64_t rec_cap, aid_match_row *rows_out, int32_t *nrows, hipStream_t s) {
    const bool lds = e->k5_path != 2, two = e->idx.delta_live();
    const int mr = e->cfg.max_results;
    // ROWS_MERGE force: a host-row call keeps its rows on the device as the lane does, and copies the merged rows out
    aid_match_row *rows = two && e->rows_merge_dev ? nullptr : rows_out;
    K5Host &h = e->k5h, &hd = e->k5h_d;
    const CsrView vm = e->idx.view();
    if (int rc = k5_enqueue(e, vm, e->q, recs, qstart_dev, qcount_dev, nq, rec_cap, lds, rows != nullptr, h, s)) return rc;
    if (two)
        if (int rc = k5_enqueue(e, e->idx.view(*e->idx.delta), e->qd, recs, qstart_dev, qcount_dev, nq, rec_cap, lds,
                                rows != nullptr, hd, s))
            return rc;
    HIP_TRY(hipStreamSynchronize(s));
    if (lds && rows) std::memcpy(rows, h.rows.p, (size_t)nq * mr * sizeof(aid_match_row));
    std::vector<int> todo;
    k5_tally(e, h, nq, lds, nrows, todo);
    const int64_t *h_start = h.meta.p, *h_count = h_start + nq, *h_votes = h_count + nq;
    int64_t vmax = 1;
    for (int q = 0; q < nq; ++q) vmax = std::max(vmax, h_votes[q]);
    if (int rc = k5_global(e, vm, e->q.rows.p, recs, h_start, h_count, h_votes, vmax, std::move(todo), rows, nrows, s))
        return rc;
    if (!two) return AID_OK;
    // the delta pass's hand-backs against the delta's own view, then the merge
    std::vector<aid_match_row> rows_d(rows ? (size_t)nq * mr : 0);
    std::vector<int32_t> nrows_d((size_t)nq, 0);
    if (lds && rows) std::memcpy(rows_d.data(), hd.rows.p, (size_t)nq * mr * sizeof(aid_match_row));
    k5_tally(e, hd, nq, lds, nrows_d.data(), todo, false);
    const int64_t *d_start = hd.meta.p, *d_count = d_start + nq, *d_votes = d_count + nq;
    vmax = 1;
    for (int q = 0; q < nq; ++q) vmax = std::max(vmax, d_votes[q]);
    if (int rc = k5_global(e, e->idx.view(*e->idx.delta), e->qd.rows.p, recs, d_start, d_count, d_votes, vmax,
                           std::move(todo), rows ? rows_d.data() : nullptr, nrows_d.data(), s))
        return rc;
    if (rows) {
        for (int q = 0; q < nq; ++q)
            nrows[q] = merge_rows(reinterpret_cast<int32_t *>(rows + (size_t)q * mr), nrows[q],
                                  reinterpret_cast<const int32_t *>(rows_d.data() + (size_t)q * mr), nrows_d[q], mr);
        return AID_OK;
    }
    // device mode: both passes' final counts go up (the LDS pass left -reason where it handed a query back)
    HIP_TRY(hipMemcpyAsync(e->q.nrows.p, nrows, (size_t)nq * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->qd.nrows.p, nrows_d.data(), (size_t)nq * sizeof(int32_t), hipMemcpyHostToDevice, s));
    {
        ProfScope ps(e, AID_K_ROWS_MERGE, s, true);
        launch_rows_merge(e->q.rows.p, e->q.nrows.p, e->qd.rows.p, e->qd.nrows.p, nq, mr, s);
    }
    HIP_TRY(hipGetLastError());
    if (rows_out)
        HIP_TRY(hipMemcpyAsync(rows_out, e->q.rows.p, (size_t)nq * mr * sizeof(aid_match_row), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));  // nrows and nrows_d are pageable: their copies must not outlive this call
    for (int q = 0; q < nq; ++q) nrows[q] = std::min(std::max(nrows[q], 0) + std::max(nrows_d[q], 0), mr);
    return AID_OK;
}

// K5 keys its distinct-frame sets by (table slot << 20 | t_q) (index.hip distinct_first): a query's anchor frames must
// stay below 2^20 - 1 (3.4 h of audio at 44.1 kHz, 4.6 h at 16 kHz)
constexpr int64_t kMaxQueryFrame = ((int64_t)1 << 20) - 2;
static int check_query_frames(const aid_engine *e) {
    for (int c = 0; c < e->ext.plan.n_clips; ++c)
        if (e->ext.plan.frames[c] > kMaxQueryFrame + 1)
            return fail(AID_ERR_INVALID, "query clip longer than 2^20 - 1 frames (FPSPEC v1 7)");
    return AID_OK;
}

extern "C" {

int aid_query(aid_engine *e, const aid_hash *recs, const int64_t *qoff, int32_t nq, aid_match_row *rows,
              int32_t *nrows) {
    if (!e || nq < 0 || !qoff || (nq > 0 && (!rows || !nrows))) return fail(AID_ERR_INVALID, "aid_query: bad argument");
    if (nq == 0) return AID_OK;
    for (int q = 0; q < nq; ++q)
        if (qoff[q + 1] < qoff[q]) return fail(AID_ERR_INVALID, "aid_query: offsets must be non-decreasing");
    for (int64_t i = qoff[0]; i < qoff[nq]; ++i)
        if ((int64_t)recs[i].t1 > kMaxQueryFrame)
            return fail(AID_ERR_INVALID, "aid_query: record anchor frame >= 2^20 - 1 (FPSPEC v1 7)");
    std::lock_guard<std::mutex> lk(e->mu);
    if (int rc = ensure_index(e)) return rc;
    hipStream_t s = e->own_stream;
    const int64_t n = qoff[nq] - qoff[0];
    HIP_TRY(e->q_recs.reserve((size_t)std::max<int64_t>(n, 1)));
    HIP_TRY(e->q_start.reserve(nq));
    HIP_TRY(e->q_count.reserve(nq));
    std::vector<int64_t> st(nq), ct(nq);
    for (int q = 0; q < nq; ++q) {
        st[q] = qoff[q] - qoff[0];
        ct[q] = qoff[q + 1] - qoff[q];
    }
    if (n > 0) HIP_TRY(hipMemcpyAsync(e->q_recs.p, recs + qoff[0], n * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->q_start.p, st.data(), nq * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->q_count.p, ct.data(), nq * sizeof(int64_t), hipMemcpyHostToDevice, s));
    return run_queries(e, e->q_recs.p, e->q_start.p, e->q_count.p, nq, std::max<int64_t>(n, 1), rows, nrows, s);
}

// q_start <- clip_base through page-locked staging: from the engine's std::vector (pageable) the copy could hold
// the host until the stream had drained the extraction queued before it. Every caller waits for its stream before
// returning, so the staging is free again at the next call.
static hipError_t upload_clip_base(aid_engine *e, int n, hipStream_t s) {
    hipError_t he = e->hq_start.reserve((size_t)n);
    if (he != hipSuccess) return he;
    std::memcpy(e->hq_start.p, e->ext.plan.hash_base.data(), (size_t)n * sizeof(int64_t));
    return hipMemcpyAsync(e->q_start.p, e->hq_start.p, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, s);
}

static int query_extracted_locked(aid_engine *e, aid_match_row *rows, int32_t *nrows) {
    if (int rc = check_query_frames(e)) return rc;
    if (int rc = ensure_index(e)) return rc;
    hipStream_t s = e->last_stream ? e->last_stream : e->own_stream;
    const int nq = e->ext.plan.n_clips;
    if (nq == 0) return AID_OK;
    if (!rows || !nrows) return fail(AID_ERR_INVALID, "null output");
    HIP_TRY(e->q_start.reserve(nq));
    HIP_TRY(upload_clip_base(e, nq, s));
    return run_queries(e, e->ext.records.p, e->q_start.p, e->ext.counts.p, nq, (int64_t)e->ext.records.n, rows, nrows, s);
}

int aid_query_extracted(aid_engine *e, aid_match_row *rows, int32_t *nrows) {
    if (!e) return fail(AID_ERR_INVALID, "null engine");
    if (!e->ext.have_result) return fail(AID_ERR_STATE, "no extraction to query with");
    std::lock_guard<std::mutex> lk(e->mu);
    return query_extracted_locked(e, rows, nrows);
}

static int query_pcm_entry(const char *fn, aid_engine *e, const void *pcm, PcmFmt fmt, const int64_t *offsets,
                           int32_t n_clips, int32_t loc, aid_match_row *rows, int32_t *nrows, void *stream) {
    if (int rc = check_clips(fn, e, pcm, offsets, n_clips, loc)) return rc;
    if (n_clips > 0 && (!rows || !nrows)) return fail(AID_ERR_INVALID, std::string(fn) + ": null output");
    if (n_clips == 0) return AID_OK;
    // one critical section: no other thread's extraction can land between this batch's K1-K3 and K5
    std::lock_guard<std::mutex> lk(e->mu);
    if (int rc = ensure_index(e)) return rc;
    if (int rc = extract_locked(e, pcm, fmt, offsets, n_clips, loc, stream)) return drain_host_copy(e, loc, stream, rc);
    return drain_host_copy(e, loc, stream, query_extracted_locked(e, rows, nrows));
}

int aid_query_pcm(aid_engine *e, const float *pcm, const int64_t *offsets, int32_t n_clips, int32_t loc,
                  aid_match_row *rows, int32_t *nrows, void *stream) {
    return query_pcm_entry("aid_query_pcm", e, pcm, kF32, offsets, n_clips, loc, rows, nrows, stream);
}

int aid_query_pcm_s16(aid_engine *e, const int16_t *pcm, const int64_t *offsets, int32_t n_clips, int32_t loc,
                      aid_match_row *rows, int32_t *nrows, void *stream) {
    return query_pcm_entry("aid_query_pcm_s16", e, pcm, kS16, offsets, n_clips, loc, rows, nrows, stream);
}

// ---- asynchronous windowed query: submit enqueues the extraction, K5's LDS path and the result
// copies and returns; collect waits for the ticket's event (struct aid_query_ticket: engine_internal.h).
static std::unique_ptr<aid_query_ticket> take_ticket(aid_engine *e) {
    // a pooled ticket keeps its page-locked and device buffers and its event: allocating them per call (pinned and
    // device blocks, and the free that synchronises the device on release) had cost more than the overlap gained
    if (e->ticket_pool.empty()) return std::unique_ptr<aid_query_ticket>(new aid_query_ticket());
    std::unique_ptr<aid_query_ticket> t = std::move(e->ticket_pool.back());
    e->ticket_pool.pop_back();
    return t;
}

// the body both submit entries share (engine lock held): the extraction of n clips, K5's LDS pass over the ticket's
// own copy of the records, the result copies into its page-locked buffers and its event
static int submit_locked(aid_engine *e, const void *pcm, PcmFmt fmt, const int64_t *offsets, const int64_t *ends,
                         int32_t n, int32_t loc, void *stream, aid_query_ticket *t) {
    t->nq = n;
    t->nrec = 0;
    t->two = false;
    t->seg_main.reset();  // (a pooled ticket that went back without a collect)
    t->seg_delta.reset();
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = ensure_index(e)) return rc;
    if (n == 0) return AID_OK;
    if (int rc = extract_locked(e, pcm, fmt, offsets, n, loc, stream, ends)) return rc;
    if (int rc = check_query_frames(e)) return rc;
    hipStream_t s = e->last_stream ? e->last_stream : e->own_stream;
    t->s = s;
    const int nq = n;
    t->nrec = e->ext.plan.records;
    HIP_TRY(t->host.meta.reserve((size_t)3 * nq));
    HIP_TRY(t->recs.reserve((size_t)std::max<int64_t>(t->nrec, 1)));
    HIP_TRY(t->qsc.reserve((size_t)2 * nq));
    std::memcpy(t->host.meta.p, e->ext.plan.hash_base.data(), (size_t)nq * sizeof(int64_t));
    // the ticket's own copies: record starts (from its page-locked meta), counts and records (device to device)
    HIP_TRY(hipMemcpyAsync(t->qsc.p, t->host.meta.p, (size_t)nq * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(t->qsc.p + nq, e->ext.counts.p, (size_t)nq * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(t->recs.p, e->ext.records.p, (size_t)t->nrec * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    // always the LDS pass: a ticket ignores the K5_PATH force (collect runs the global path for what it hands back)
    if (int rc = k5_enqueue(e, e->idx.view(), e->q, t->recs.p, t->qsc.p, t->qsc.p + nq, nq, t->nrec, true, true, t->host,
                            s, true))
        return rc;
    // live index: the delta's LDS pass behind main's, into the ticket's second result block; the ticket holds both
    // segments, so collect resolves each one's hand-backs against the views it was submitted under
    t->two = e->idx.delta_live();
    if (e->idx.live_cap > 0) {
        t->seg_main = e->idx.main;
        t->seg_delta = t->two ? e->idx.delta : nullptr;
    }
    if (t->two) {
        HIP_TRY(t->host_d.meta.reserve((size_t)3 * nq));
        std::memcpy(t->host_d.meta.p, t->host.meta.p, (size_t)nq * sizeof(int64_t));
        if (int rc = k5_enqueue(e, e->idx.view(*e->idx.delta), e->qd, t->recs.p, t->qsc.p, t->qsc.p + nq, nq, t->nrec, true,
                                true, t->host_d, s, true))
            return rc;
    }
    HIP_TRY(t->ev.record(s));
    return AID_OK;
}

static int windows_submit_entry(const char *fn, aid_engine *e, const void *pcm, PcmFmt fmt, const int64_t *starts,
                                const int64_t *ends, int32_t n_windows, void *stream, aid_query_ticket **out) {
    if (!e || n_windows < 0 || !out || (n_windows > 0 && (!starts || !ends || !pcm)))
        return fail(AID_ERR_INVALID, std::string(fn) + ": bad argument");
    *out = nullptr;
    for (int c = 0; c < n_windows; ++c)
        if (starts[c] < 0 || ends[c] < starts[c]) return fail(AID_ERR_INVALID, std::string(fn) + ": bad window");
    std::lock_guard<std::mutex> lk(e->mu);
    std::unique_ptr<aid_query_ticket> t = take_ticket(e);
    if (int rc = submit_locked(e, pcm, fmt, starts, ends, n_windows, AID_PCM_DEVICE, stream, t.get())) return rc;
    *out = t.release();
    return AID_OK;
}

extern "C" int aid_query_windows_submit(aid_engine *e, const float *pcm, const int64_t *starts, const int64_t *ends,
                                        int32_t n_windows, void *stream, aid_query_ticket **out) {
    return windows_submit_entry("aid_query_windows_submit", e, pcm, kF32, starts, ends, n_windows, stream, out);
}

extern "C" int aid_query_windows_submit_s16(aid_engine *e, const int16_t *pcm, const int64_t *starts,
                                            const int64_t *ends, int32_t n_windows, void *stream,
                                            aid_query_ticket **out) {
    return windows_submit_entry("aid_query_windows_submit_s16", e, pcm, kS16, starts, ends, n_windows, stream, out);
}

// aid_query_pcm in two halves (the query coalescer's pipelined batches): host PCM must stay unchanged until the ticket
// is collected (its one H2D copy is queued, not waited for)
static int pcm_submit_entry(const char *fn, aid_engine *e, const void *pcm, PcmFmt fmt, const int64_t *offsets,
                            int32_t n_clips, int32_t loc, void *stream, aid_query_ticket **out) {
    if (!out) return fail(AID_ERR_INVALID, std::string(fn) + ": bad argument");
    *out = nullptr;
    if (int rc = check_clips(fn, e, pcm, offsets, n_clips, loc)) return rc;
    std::lock_guard<std::mutex> lk(e->mu);
    std::unique_ptr<aid_query_ticket> t = take_ticket(e);
    if (int rc = submit_locked(e, pcm, fmt, offsets, nullptr, n_clips, loc, stream, t.get()))
        return drain_host_copy(e, loc, stream, rc);
    *out = t.release();
    return AID_OK;
}

extern "C" int aid_query_pcm_submit(aid_engine *e, const float *pcm, const int64_t *offsets, int32_t n_clips,
                                    int32_t loc, void *stream, aid_query_ticket **out) {
    return pcm_submit_entry("aid_query_pcm_submit", e, pcm, kF32, offsets, n_clips, loc, stream, out);
}

extern "C" int aid_query_pcm_submit_s16(aid_engine *e, const int16_t *pcm, const int64_t *offsets, int32_t n_clips,
                                        int32_t loc, void *stream, aid_query_ticket **out) {
    return pcm_submit_entry("aid_query_pcm_submit_s16", e, pcm, kS16, offsets, n_clips, loc, stream, out);
}

extern "C" int aid_query_windows_collect(aid_engine *e, aid_query_ticket *t, aid_match_row *rows, int32_t *nrows) {
    if (!e || !t) {
        delete t;
        return fail(AID_ERR_INVALID, "aid_query_windows_collect: bad argument");
    }
    if (t->nq > 0 && (!rows || !nrows)) {
        (void)t->ev.wait();
        std::lock_guard<std::mutex> lk(e->mu);
        e->ticket_pool.emplace_back(t);
        return fail(AID_ERR_INVALID, "aid_query_windows_collect: bad argument");
    }
    if (t->nq > 0) {
        const hipError_t we = t->ev.wait();
        if (we != hipSuccess) {
            delete t;
            return fail(AID_ERR_DEVICE, std::string("aid_query_windows_collect: ") + hipGetErrorString(we));
        }
    }
    std::lock_guard<std::mutex> lk(e->mu);
    struct Back {  // back to the pool on every return below (the ticket's work has completed)
        aid_engine *e;
        aid_query_ticket *t;
        ~Back() {
            t->seg_main.reset();  // the segments it held go back to the index (or, replaced meanwhile, are freed)
            t->seg_delta.reset();
            e->ticket_pool.emplace_back(t);
        }
    } back{e, t};
    if (t->nq == 0) return AID_OK;
    const int nq = t->nq, mr = e->cfg.max_results;
    std::memcpy(rows, t->host.rows.p, (size_t)nq * mr * sizeof(aid_match_row));
    // the views the ticket was submitted under where it holds its segments (live index), else the index's own. The
    // track table is the engine's current one either way; a held segment that a build has replaced meanwhile checks
    // it for every posting (removals since then were counted on its successor)
    const HashIndex &hx = e->idx;
    CsrView vm = t->seg_main ? hx.view(*t->seg_main) : hx.view();
    if (t->seg_main && t->seg_main != hx.main) vm.check_tomb = 1;
    std::vector<int> todo;
    k5_tally(e, t->host, nq, true, nrows, todo);
    if (todo.empty() && !t->two) return AID_OK;
    // the queries the LDS pass handed back: the global path over the ticket's own copy of their records. It uses
    // engine-wide scratch, which the K5 of a later submit on another stream may still be using
    HIP_TRY(hipSetDevice(e->device));
    if (e->last_stream && e->last_stream != t->s) HIP_TRY(hipStreamSynchronize(e->last_stream));
    const int64_t *starts = t->host.meta.p, *counts = starts + nq, *votes = counts + nq;
    int64_t vmax = 1;
    for (int q : todo) vmax = std::max(vmax, votes[q]);
    if (!todo.empty())
        if (int rc = k5_global(e, vm, nullptr, t->recs.p, starts, counts, votes, vmax, std::move(todo), rows, nrows, t->s))
            return rc;
    if (!t->two) return AID_OK;
    CsrView vd = hx.view(*t->seg_delta);
    if (t->seg_delta != hx.delta) vd.check_tomb = 1;
    std::vector<aid_match_row> rows_d((size_t)nq * mr);
    std::vector<int32_t> nrows_d((size_t)nq, 0);
    std::memcpy(rows_d.data(), t->host_d.rows.p, (size_t)nq * mr * sizeof(aid_match_row));
    k5_tally(e, t->host_d, nq, true, nrows_d.data(), todo, false);
    const int64_t *d_votes = t->host_d.meta.p + 2 * (size_t)nq;
    vmax = 1;
    for (int q : todo) vmax = std::max(vmax, d_votes[q]);
    if (!todo.empty())
        if (int rc = k5_global(e, vd, nullptr, t->recs.p, starts, counts, d_votes, vmax, std::move(todo), rows_d.data(),
                               nrows_d.data(), t->s))
            return rc;
    for (int q = 0; q < nq; ++q)
        nrows[q] = merge_rows(reinterpret_cast<int32_t *>(rows + (size_t)q * mr), nrows[q],
                              reinterpret_cast<const int32_t *>(rows_d.data() + (size_t)q * mr), nrows_d[q], mr);
    return AID_OK;
}

static int query_windows_entry(const char *fn, aid_engine *e, const void *pcm, PcmFmt fmt, const int64_t *starts,
                               const int64_t *ends, int32_t n_windows, aid_match_row *rows, int32_t *nrows,
                               void *stream) {
    if (!e || n_windows < 0 || (n_windows > 0 && (!starts || !ends || !rows || !nrows)))
        return fail(AID_ERR_INVALID, std::string(fn) + ": bad argument");
    for (int c = 0; c < n_windows; ++c)
        if (starts[c] < 0 || ends[c] < starts[c]) return fail(AID_ERR_INVALID, std::string(fn) + ": bad window");
    if (n_windows > 0 && !pcm) return fail(AID_ERR_INVALID, std::string(fn) + ": null pcm");
    if (n_windows == 0) return AID_OK;
    // one critical section, as aid_query_pcm: K1 reads every window in place (they may overlap), then K5
    std::lock_guard<std::mutex> lk(e->mu);
    if (int rc = ensure_index(e)) return rc;
    if (int rc = extract_locked(e, pcm, fmt, starts, n_windows, AID_PCM_DEVICE, stream, ends)) return rc;
    return query_extracted_locked(e, rows, nrows);
}

int aid_query_windows(aid_engine *e, const float *pcm, const int64_t *starts, const int64_t *ends, int32_t n_windows,
                      aid_match_row *rows, int32_t *nrows, void *stream) {
    return query_windows_entry("aid_query_windows", e, pcm, kF32, starts, ends, n_windows, rows, nrows, stream);
}

int aid_query_windows_s16(aid_engine *e, const int16_t *pcm, const int64_t *starts, const int64_t *ends,
                          int32_t n_windows, aid_match_row *rows, int32_t *nrows, void *stream) {
    return query_windows_entry("aid_query_windows_s16", e, pcm, kS16, starts, ends, n_windows, rows, nrows, stream);
}

}  // extern "C"

// ---------------------------------------------------------------- batched exact lane

extern "C" int aid_exact_windows(int64_t n, int32_t sample_rate, int64_t *lo, int64_t *len, int32_t *mode) {
    if (n < 0 || sample_rate <= 0 || !lo || !len || !mode) return fail(AID_ERR_INVALID, "aid_exact_windows: bad argument");
    // app/search/exact.py: duration = samples / SAMPLE_RATE (:389-390); <= 5.0 s -> SUB_WINDOWS
    // (:48-52, :103), stop = min(b, duration), piece = _extract_pcm_window(a, stop) if a < stop
    // (:150-160), whose byte bounds are int(t * SAMPLE_RATE) * 4 clamped to the data (:374-399)
    static const double kSub[3][2] = {{0.0, 3.5}, {0.75, 4.25}, {1.5, 5.0}};
    const double sr = (double)sample_rate, dur = (double)n / sr;
    if (!(dur <= 5.0)) {
        *mode = 0;
        lo[0] = 0;
        len[0] = n;
        return 1;
    }
    *mode = 1;
    for (int w = 0; w < 3; ++w) {
        const double a = kSub[w][0], stop = std::min(kSub[w][1], dur);
        int64_t l = 0, h = 0;
        if (a < stop) {
            l = std::min(std::max<int64_t>((int64_t)(a * sr), 0), n);
            h = std::max(l, std::min<int64_t>((int64_t)(stop * sr), n));
        }
        lo[w] = l;
        len[w] = h - l;  // 0: the reference sends no query for this window
    }
    return 3;
}

static int exact_lane_locked(aid_engine *e, const void *pcm, PcmFmt fmt, const int64_t *offsets, int32_t n_clips,
                             int32_t loc, int32_t max_out, aid_exact_row *out, int32_t *n_out, void *stream);

static int exact_lane_entry(const char *fn, aid_engine *e, const void *pcm, PcmFmt fmt, const int64_t *offsets,
                            int32_t n_clips, int32_t loc, int32_t max_out, aid_exact_row *out, int32_t *n_out,
                            void *stream) {
    if (!e || !offsets || n_clips < 0 || max_out <= 0 || (n_clips > 0 && (!out || !n_out)))
        return fail(AID_ERR_INVALID, std::string(fn) + ": bad argument");
    if (int rc = check_clips(fn, e, pcm, offsets, n_clips, loc)) return rc;
    if (e->cfg.max_results > 256) return fail(AID_ERR_INVALID, std::string(fn) + ": engine max_results must be <= 256");
    if (n_clips == 0) return AID_OK;
    std::lock_guard<std::mutex> lk(e->mu);
    return drain_host_copy(e, loc, stream,
                           exact_lane_locked(e, pcm, fmt, offsets, n_clips, loc, max_out, out, n_out, stream));
}

extern "C" int aid_exact_lane(aid_engine *e, const float *pcm, const int64_t *offsets, int32_t n_clips, int32_t loc,
                              int32_t max_out, aid_exact_row *out, int32_t *n_out, void *stream) {
    return exact_lane_entry("aid_exact_lane", e, pcm, kF32, offsets, n_clips, loc, max_out, out, n_out, stream);
}

extern "C" int aid_exact_lane_s16(aid_engine *e, const int16_t *pcm, const int64_t *offsets, int32_t n_clips,
                                  int32_t loc, int32_t max_out, aid_exact_row *out, int32_t *n_out, void *stream) {
    return exact_lane_entry("aid_exact_lane_s16", e, pcm, kS16, offsets, n_clips, loc, max_out, out, n_out, stream);
}

// The lane up to K8b, engine lock held: the rows of clip c end in e->x_out[c * max_out ..] and their count in
// e->x_nout[c], on the device, complete in stream order (exact_lane_locked copies them out; the speed lane, speed.cpp,
// selects among them first)
int exact_lane_device(aid_engine *e, const void *pcm, PcmFmt fmt, const int64_t *offsets, int32_t n_clips, int32_t loc,
                      int32_t max_out, void *stream) {
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = ensure_index(e)) return rc;
    hipStream_t s = pick_stream(e, stream);
    if (e->last_stream && e->last_stream != s) HIP_TRY(hipStreamSynchronize(e->last_stream));
    // fan-out plan (host): clip_win = (first window, windows, mode). A window of odd length n is
    // extracted as n - 1 samples: with an even hop, frames(n) = frames(n - 1) for odd n and no
    // frame reaches the last sample, so the records are the same. K1 reads the windows in place
    // (wstart / wend into the clips' PCM; at 44.1 kHz the 0.75 s window starts at an odd sample);
    // the LANE_GATHER A/B copies them to even offsets of a staging buffer first (xoff)
    std::vector<int64_t> wdesc, xoff(1, 0), wstart, wend;
    std::vector<int32_t> clipwin(3 * (size_t)n_clips);
    int64_t staged = 0, max_len = 0;
    for (int c = 0; c < n_clips; ++c) {
        int64_t lo[3], len[3];
        int32_t mode = 0;
        const int nw = aid_exact_windows(offsets[c + 1] - offsets[c], e->cfg.sample_rate, lo, len, &mode);
        clipwin[3 * c] = (int32_t)(xoff.size() - 1);
        int used = 0;
        for (int w = 0; w < nw; ++w) {
            if (len[w] <= 0) continue;  // the reference sends no query for an empty piece
            const int64_t m = len[w] & ~(int64_t)1;
            wdesc.push_back(offsets[c] - offsets[0] + lo[w]);
            wdesc.push_back(m);
            wdesc.push_back(staged);
            wstart.push_back(offsets[c] - offsets[0] + lo[w]);
            wend.push_back(offsets[c] - offsets[0] + lo[w] + m);
            staged += m;
            xoff.push_back(staged);
            max_len = std::max(max_len, m);
            ++used;
        }
        clipwin[3 * c + 1] = used;
        clipwin[3 * c + 2] = mode;
    }
    const int n_win = (int)(xoff.size() - 1);
    const void *src = pcm_at(pcm, fmt, offsets[0]);
    if (loc == AID_PCM_HOST) {
        const int64_t n_all = offsets[n_clips] - offsets[0];
        const size_t nbytes = (size_t)n_all * pcm_size(fmt);  // x_in is raw bytes to both formats
        HIP_TRY(e->x_in.reserve(std::max<size_t>((nbytes + sizeof(float) - 1) / sizeof(float), 1)));
        if (n_all > 0) HIP_TRY(hipMemcpyAsync(e->x_in.p, src, nbytes, hipMemcpyHostToDevice, s));
        src = e->x_in.p;
    }
    HIP_TRY(e->x_clipwin.reserve(clipwin.size()));
    HIP_TRY(hipMemcpyAsync(e->x_clipwin.p, clipwin.data(), clipwin.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(e->x_nout.reserve((size_t)n_clips));
    HIP_TRY(e->x_out.reserve((size_t)n_clips * max_out * 3));
    std::vector<int32_t> nrows(std::max(n_win, 1), 0);
    const int mr = e->cfg.max_results;
    if (n_win > 0) {
        if (e->lane_gather) {
            HIP_TRY(e->x_wdesc.reserve(wdesc.size()));
            HIP_TRY(hipMemcpyAsync(e->x_wdesc.p, wdesc.data(), wdesc.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
            HIP_TRY(e->x_win.reserve((size_t)std::max<int64_t>(staged, 2)));
            // the gather converts s16 windows on the way: the staged windows are float to either format
            launch_window_gather(src, fmt == kS16, e->x_wdesc.p, n_win, max_len, e->x_win.p, s);
            HIP_TRY(hipGetLastError());
            if (int rc = extract_locked(e, e->x_win.p, kF32, xoff.data(), n_win, AID_PCM_DEVICE, s)) return rc;
        } else {
            if (int rc = extract_locked(e, src, fmt, wstart.data(), n_win, AID_PCM_DEVICE, s, wend.data())) return rc;
        }
        if (int rc = check_query_frames(e)) return rc;
        HIP_TRY(e->q_start.reserve(n_win));
        HIP_TRY(upload_clip_base(e, n_win, s));
        if (int rc = run_queries(e, e->ext.records.p, e->q_start.p, e->ext.counts.p, n_win,
                                 (int64_t)e->ext.records.n, nullptr, nrows.data(), s))
            return rc;
        HIP_TRY(e->q.nrows.reserve((size_t)n_win));
        HIP_TRY(hipMemcpyAsync(e->q.nrows.p, nrows.data(), n_win * sizeof(int32_t), hipMemcpyHostToDevice, s));
    } else {
        HIP_TRY(e->q.nrows.reserve(1));
        HIP_TRY(e->q.rows.reserve((size_t)mr * 5));
        HIP_TRY(hipMemsetAsync(e->q.nrows.p, 0, sizeof(int32_t), s));
    }
    const double sec = (double)e->cfg.hop / (double)e->cfg.sample_rate;
    launch_exact_consensus(e->q.rows.p, e->q.nrows.p, mr, e->x_clipwin.p, n_clips, sec, max_out, e->x_out.p, e->x_nout.p,
                           s);
    HIP_TRY(hipGetLastError());
    return AID_OK;
}

static int exact_lane_locked(aid_engine *e, const void *pcm, PcmFmt fmt, const int64_t *offsets, int32_t n_clips,
                             int32_t loc, int32_t max_out, aid_exact_row *out, int32_t *n_out, void *stream) {
    if (int rc = exact_lane_device(e, pcm, fmt, offsets, n_clips, loc, max_out, stream)) return rc;
    hipStream_t s = pick_stream(e, stream);
    HIP_TRY(hipMemcpyAsync(n_out, e->x_nout.p, (size_t)n_clips * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out, e->x_out.p, (size_t)n_clips * max_out * sizeof(aid_exact_row), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    e->last_stream = s;
    return AID_OK;
}

