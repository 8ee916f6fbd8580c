// engine_internal.h -- what the host files of libaidfp.so share: the engine's state (struct aid_engine), its buffer
// and profiling helpers, the prologue of its entry points (EngineCall), and the few functions the host files call
// across their boundaries. engine.cpp: the engine itself, synth, resampling, dedup, the vector lane's wrappers,
// profiling. extract.cpp: extraction and its results (aidfp_extract.h). index_host.cpp: the hash index
// (aidfp_index.h). index_exchange.cpp: aid_comm and the index exchange (the only file that includes RCCL).
// query.cpp: K5, the query entry points, the exact lane. speed.cpp: the speed fan-out and the speed lane
// (aidfp_speed_plan.h). mel.cpp: the CLAP log-mel front end (aidfp_mel_plan.h, aidfp_mel.h). chroma.cpp: the content fingerprint
// (aidfp_chroma_plan.h, aidfp_chroma.h). Nothing here is part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/aidfp.h"
#include "aidfp_buffers.h"
#include "aidfp_chroma.h"
#include "aidfp_device.h"
#include "aidfp_extract.h"
#include "aidfp_index.h"
#include "aidfp_launch.h"
#include "aidfp_layout.h"
#include "aidfp_mel.h"
#include "aidfp_speed_plan.h"
#include "aidfp_vector.h"

#pragma GCC visibility push(hidden)  // shared between the host files, not exported

using namespace aid;

int fail(int code, const std::string &msg);  // engine.cpp: keeps msg for aid_last_error, returns code
const std::string &last_error_text();        // engine.cpp: the calling thread's last fail() message

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return fail(_e == hipErrorOutOfMemory ? AID_ERR_NOMEM : AID_ERR_DEVICE,                \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                        \
    } while (0)

// K5's page-locked result block: a call queues the copies into it behind its kernels and waits once. The engine
// owns one (the synchronous calls), every aid_query_ticket its own
struct K5Host {
    HostBuf<int64_t> meta;   // [0, nq) record starts, [nq, 2nq) record counts, [2nq, 3nq) exact votes
    HostBuf<int32_t> rows;   // the LDS pass's rows, [nq][max_results][5]
    HostBuf<int32_t> nrows;  // the LDS pass's row counts; -r: handed back for reason r (index.hip)
};

// K5's device scratch of one pass over one CSR segment: the queries' exact votes, the CSR range of every query record
// (k_query_votes -> k_match_lds), and the pass's rows and row counts. The engine owns one per segment: the two passes
// of a query over the live index are queued back to back, and a set shared between them would be overwritten by the
// second before the first one's results were copied out
struct K5Scratch {
    DevBuf<int64_t> votes;    // exact votes per query (LDS-histogram eligibility)
    DevBuf<uint64_t> ranges;  // per query record its CSR range
    DevBuf<int32_t> rows, nrows;  // [nq][max_results][5], [nq]
};

struct ProfEvent {
    int kernel;
    hipEvent_t a, b;
};

// the engine's own stream. Declared ahead of every buffer and event of aid_engine, so it is destroyed after them
struct OwnStream {
    hipStream_t s = nullptr;
    OwnStream() = default;
    OwnStream(const OwnStream &) = delete;
    OwnStream &operator=(const OwnStream &) = delete;
    ~OwnStream() {
        if (s) (void)hipStreamDestroy(s);
    }
    operator hipStream_t() const { return s; }
};

// asynchronous windowed query (query.cpp): the ticket owns page-locked result buffers and a device
// copy of its records (the next submit reuses the engine's extraction buffers in stream order), so a query the LDS
// path hands back can still be answered on the global path at collect time
struct aid_query_ticket {
    int nq = 0;
    int64_t nrec = 0;
    hipStream_t s = nullptr;
    Event ev;
    K5Host host;  // the LDS pass's results, complete behind ev
    // live index (aid_index_live on at submit): the delta pass's results, and the segments the ticket was submitted
    // under, held until it is collected (a build meanwhile leaves them alone, aidfp_index.h CsrSegment)
    K5Host host_d;
    bool two = false;  // a delta pass was queued
    std::shared_ptr<CsrSegment> seg_main, seg_delta;
    DevBuf<uint64_t> recs;
    DevBuf<int64_t> qsc;  // device record starts and counts of the ticket's queries ([0, nq), [nq, 2nq))
};

struct aid_engine {
    aid_config cfg{};
    int device = 0;
    OwnStream own_stream;
    Extractor ext;  // extraction (FPSPEC 1-6): K1..K3's buffers, K2's policy, the last call's plan (aidfp_extract.h)
    DevBuf<Tables> d_tab;
    DevBuf<int16_t> d_sin;
    DevBuf<uint32_t> synth_tracks;
    DevBuf<int64_t> synth_starts;
    HostBuf<uint8_t> h_synth;  // pinned staging of aid_synth_rate's tracks + starts (AID_SYNTH_ASYNC returns early)
    Event synth_ev;

    HashIndex idx;  // hash index (FPSPEC 7): postings, track table, CSR, K4 and exchange scratch (aidfp_index.h)
    // query workspaces
    DevBuf<uint64_t> q_recs;
    DevBuf<int64_t> q_start, q_count;
    DevBuf<uint32_t> q_hist;
    K5Scratch q, qd;  // K5 scratch of the main pass and of the live index's delta pass
    DevBuf<uint32_t> q_hot;  // K5h hot-bucket bitmaps, [batch][2^bits / 32]
    DevBuf<uint32_t> q_dset;  // K5b retries: HBM distinct (slot, t_q) sets, [batch][2^dbits]
    K5Host k5h, k5h_d;          // run_queries: the synchronous calls' result blocks (main pass, delta pass)
    HostBuf<int64_t> hq_start;  // the queries' record starts (clip_base) staged page-locked for their upload
    // collected tickets, reused: their buffers and event stay allocated
    std::vector<std::unique_ptr<aid_query_ticket>> ticket_pool;
    DevBuf<int64_t> q_gsc;    // K5 global pass: record starts and counts of the queries it runs ([0, n), [n, 2n))
    DevBuf<int32_t> q_grows;  // K5 global pass: their rows [n][max_results][5], then their n row counts
    // batched exact lane (aid_exact_lane): PCM staging, window descriptors, consensus output
    DevBuf<float> x_in, x_win;
    DevBuf<int64_t> x_wdesc;
    DevBuf<int32_t> x_order, x_clipwin, x_nout;
    DevBuf<double> x_out;  // aid_exact_row, 3 x 8 bytes each
    std::map<std::pair<int32_t, int32_t>, DevBuf<float>> rs_taps;  // (up, down) -> device [up][J] taps
    // speed fan-out (speed.cpp; FPSPEC 8.2, 7.1): the call's plan, its device tables ([clip_off | dst_off | blk_first]
    // int64, the speeds' SpeedVarDev rows, the speeds), staged host PCM, a clip group's variant PCM, the winners
    SpeedPlan sp_plan;
    HostBuf<int64_t> sp_hidx;
    HostBuf<uint8_t> sp_hvar;
    DevBuf<int64_t> sp_idx;
    DevBuf<uint8_t> sp_var;
    DevBuf<int32_t> sp_seln;  // the winners' row counts [n_clips], then their speeds [n_clips]
    DevBuf<float> sp_in, sp_pcm;
    DevBuf<double> sp_sel;  // aid_exact_row, 3 x 8 bytes each
    Event sp_ev;            // the last K6s launch: its tables and staging are free again behind it
    int64_t speed_group = 0;  // aid_engine_force SPEED_GROUP: variant samples per clip group (0 = 1 GiB of them)
    // Chromaprint dedup catalog (insertion order) + scan scratch
    DevBuf<uint32_t> dd_words;
    DevBuf<int64_t> dd_off;
    DevBuf<double> dd_dur;
    int64_t dd_n = 0, dd_nw = 0;
    DevBuf<uint32_t> dq_words, dq_words2;
    DevBuf<int64_t> dq_off, dq_off2, dq_idx, dq_pidx;
    DevBuf<double> dq_lo, dq_hi, dq_sim, dq_psim;
    ChromaState chroma;  // content fingerprint (FPSPEC 11): tables, block lists, staging, rows (chroma.cpp)
    MelState mel;    // CLAP log-mel front end (FPSPEC 10): tables, filter bank, chunk table, staging (mel.cpp)
    VecCatalog vec;  // vector lane (FPSPEC 9): chunk-embedding catalog + its scratch (csrc/vector.hip)
    size_t hist_zero_cap = 0;  // q_hist capacity known to be all-zero

    // aid_engine_force K5_PATH (tests): 0 the LDS pass, then the global path for the queries it hands back; 1 as 0
    // (kept for callers that pin the LDS path); 2 global path only. The submit/collect pair ignores it
    int k5_path = 0;
    int k5_parts = 0;      // aid_engine_force K5_PARTS: K5a key partitions per query (0 = by vote count)
    int lane_gather = 0;           // aid_engine_force LANE_GATHER: stage the exact lane's sub-windows (A/B)
    int rows_merge_dev = 0;        // aid_engine_force ROWS_MERGE: host-row calls merge two-segment rows on the device
    // aid_match_stats: queries, exact votes, and the postings K5 read (a vote = one 8-B posting per pass)
    int64_t st_queries = 0, st_votes = 0, st_post_reads = 0, st_q_global = 0, st_q_lds = 0, st_records = 0;
    int64_t st_sig_reads = 0;  // 2-B posting signatures the LDS path read (two per vote: counting and insert passes)
    int64_t st_fb_reason[5] = {0, 0, 0, 0, 0};  // LDS-path fallbacks (speculative pass) by reason (index.hip)
    size_t k5_batch = 2048;        // global-path queries per launch
    hipStream_t last_stream = nullptr;

    bool profiling = false;
    uint32_t prof_mask = 0xFFFFFFFFu;  // bit k: kernel id k gets events (aid_profile_select)
    std::vector<ProfEvent> pending;
    std::vector<hipEvent_t> pool;
    double prof_ms[AID_K_COUNT] = {};
    int64_t prof_n[AID_K_COUNT] = {};
    std::mutex mu;

    ~aid_engine() {  // the profiling events; every other resource is a member that frees itself
        for (auto &p : pending) {
            event_destroy(p.a);
            event_destroy(p.b);
        }
        for (hipEvent_t ev : pool) event_destroy(ev);
    }
};

static inline hipEvent_t take_event(aid_engine *e) {
    if (!e->pool.empty()) {
        hipEvent_t ev = e->pool.back();
        e->pool.pop_back();
        return ev;
    }
    hipEvent_t ev = nullptr;
    if (event_create(&ev, hipEventDefault) != hipSuccess) return nullptr;
    return ev;
}

// attached = the scope wraps exactly one timed_launch: its events are stamped by the dispatch itself
// (aidfp_device.h LaunchTiming); otherwise two hipEventRecord markers bracket the scope.
struct ProfScope {
    aid_engine *e;
    int k;
    hipStream_t s;
    bool attached;
    hipEvent_t a = nullptr, b = nullptr;
    ProfScope(aid_engine *e_, int k_, hipStream_t s_, bool attached_ = false) : e(e_), k(k_), s(s_), attached(attached_) {
        if (!e->profiling || !((e->prof_mask >> k) & 1u) || !(a = take_event(e))) return;
        if (!attached) {
            (void)hipEventRecord(a, s);
            return;
        }
        if (!(b = take_event(e))) {
            e->pool.push_back(a);
            a = nullptr;
            return;
        }
        launch_timing().start = a;
        launch_timing().stop = b;
    }
    ~ProfScope() {
        if (!a) return;
        if (attached) {
            LaunchTiming &t = launch_timing();
            if (t.start) {  // nothing was launched: the events were never stamped
                t.start = t.stop = nullptr;
                e->pool.push_back(a);
                e->pool.push_back(b);
                return;
            }
        } else {
            if (!(b = take_event(e))) return;
            (void)hipEventRecord(b, s);
        }
        e->pending.push_back({k, a, b});
    }
};

static inline hipStream_t pick_stream(aid_engine *e, void *stream) {
    return stream ? (hipStream_t)stream : e->own_stream;
}

// A host-PCM call copies the caller's samples with ONE hipMemcpyAsync on the call's stream; from page-locked
// memory that copy is a real DMA that can still be running when the call returns. On success the caller syncs
// before reusing its buffer (include/aidfp.h); on an error return the engine drains the stream itself, so a
// caller that reuses or frees its buffer after a failed call cannot race the copy. Returns rc.
static inline int drain_host_copy(aid_engine *e, int32_t loc, void *stream, int rc) {
    if (rc != AID_OK && loc == AID_PCM_HOST && e) (void)hipStreamSynchronize(pick_stream(e, stream));
    return rc;
}

// PCM sample format of an entry point (FPSPEC 8). The float functions and their _s16 twins funnel into one
// implementation each, which takes the samples as const void * plus the format; offsets count samples either way
enum PcmFmt : int { kF32 = 0, kS16 = 1 };
static inline size_t pcm_size(PcmFmt f) { return f == kS16 ? sizeof(int16_t) : sizeof(float); }
static inline const void *pcm_at(const void *p, PcmFmt f, int64_t i) {
    return static_cast<const char *>(p) + i * (int64_t)pcm_size(f);
}

// the argument checks every clip-batch entry point shares (fn = its name, for the message)
static inline int check_clips(const char *fn, aid_engine *e, const void *pcm, const int64_t *offsets, int32_t n_clips,
                              int32_t loc) {
    const std::string f(fn);
    if (!e || !offsets || n_clips < 0) return fail(AID_ERR_INVALID, f + ": bad argument");
    if (loc != AID_PCM_HOST && loc != AID_PCM_DEVICE) return fail(AID_ERR_INVALID, f + ": bad pcm_location");
    for (int c = 0; c < n_clips; ++c)
        if (offsets[c + 1] < offsets[c] || offsets[c] < 0)
            return fail(AID_ERR_INVALID, f + ": offsets must be non-decreasing and >= 0");
    if (n_clips > 0 && !pcm && offsets[n_clips] > offsets[0]) return fail(AID_ERR_INVALID, f + ": null pcm");
    return AID_OK;
}

// The prologue of an entry point that works on the engine's state: null check, the engine lock (held while the
// object lives), the engine's device made current, then on request the in-flight append settled and one wait for
// the stream of the last extraction. `s` is the call's stream. Usage: EngineCall call(e, ...); if (call.rc) return
// call.rc;
enum LastWait {
    kNoWait,     // none: the call reads host state only, or queues behind last_stream itself
    kDrainLast,  // last_stream drained: the call reads what the last extraction or append wrote
    kOrderLast,  // last_stream drained only if it is not the call's own stream
};
struct EngineCall {
    std::unique_lock<std::mutex> lk;
    hipStream_t s = nullptr;
    int rc = AID_OK;
    EngineCall(aid_engine *e, void *stream = nullptr, bool settle = false, LastWait w = kNoWait) {
        if (!e) {
            rc = fail(AID_ERR_INVALID, "null engine");
            return;
        }
        lk = std::unique_lock<std::mutex>(e->mu);
        s = pick_stream(e, stream);
        rc = enter(e, s, settle, w);
    }
    // the same steps for code that already holds the lock (ensure_index's build)
    static int enter(aid_engine *e, hipStream_t s, bool settle, LastWait w) {
        HIP_TRY(hipSetDevice(e->device));
        if (settle)
            if (int r = settle_postings(e)) return r;
        return wait_last(e, s, w);
    }
    // the wait alone, for a call whose argument checks against engine state come before it
    static int wait_last(aid_engine *e, hipStream_t s, LastWait w) {
        if (w != kNoWait && e->last_stream && !(w == kOrderLast && e->last_stream == s))
            HIP_TRY(hipStreamSynchronize(e->last_stream));
        return AID_OK;
    }
};

// extract.cpp; engine lock held
int extract_locked(aid_engine *e, const void *pcm, PcmFmt fmt, const int64_t *offsets, int32_t n_clips, int32_t loc,
                   void *stream, const int64_t *ends = nullptr);
// query.cpp; engine lock held: the exact lane up to K8b, rows and counts left in e->x_out / e->x_nout
int exact_lane_device(aid_engine *e, const void *pcm, PcmFmt fmt, const int64_t *offsets, int32_t n_clips, int32_t loc,
                      int32_t max_out, void *stream);
// engine.cpp; engine lock held: the device [up][J] tap table of a plan from the engine's cache (impulse: the unit
// impulse at the filter's centre, cached under -down)
int resample_taps_dev(aid_engine *e, const ResamplePlan &p, bool impulse, float **out);

#pragma GCC visibility pop
