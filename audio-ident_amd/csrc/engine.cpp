// engine.cpp -- host side of libaidfp.so, the C ABI of include/aidfp.h, which replaces the `olaf_c` process boundary
// of the reference (audio-ident-service/app/audio/fingerprint.py:87-270): the engine itself (one GPU's tables and
// workspaces; create, destroy, force knobs, profiling, stats) and the synth, resample, dedup and vector entry points.
// Extraction is extract.cpp, the hash index index_host.cpp, its exchange between ranks index_exchange.cpp, the query
// half (K5, the query entry points, the exact lane) query.cpp; engine_internal.h holds what the host files share.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>

#include "aidfp_resample_plan.h"
#include "engine_internal.h"
#include "resample_design.h"

#if defined(AID_K2_STAMPS)
namespace aid {
int k2_stamps_read(unsigned long long *out, bool reset);
}
extern "C" int aid_diag_k2_stamps(unsigned long long *out, int reset) {  // diagnostic build only
    return aid::k2_stamps_read(out, reset != 0);
}
#endif

#if defined(AID_K1_STAMPS)
namespace aid {
int k1_stamps_read(unsigned long long *out, int waves);
}
extern "C" int aid_diag_k1_stamps(unsigned long long *out, int waves) {  // diagnostic build only
    return aid::k1_stamps_read(out, waves);
}
#endif

static thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

const std::string &last_error_text() { return g_err; }

static void build_tables(Tables &t) {
    auto tw = [](int j, int L) {
        return make_float2((float)cos(2.0 * M_PI * (double)j / (double)L),
                           (float)(-sin(2.0 * M_PI * (double)j / (double)L)));
    };
    for (int m = 0; m < 1024; ++m)
        t.win2[m] = make_float2((float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)(2 * m) / 2048.0)),
                                (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)(2 * m + 1) / 2048.0)));
    for (int j = 0; j < 16; ++j) t.t16[j] = tw(j, 16);
    for (int j = 0; j < 64; ++j) t.t64[j] = tw(j, 64);
    for (int j = 0; j < 1024; ++j) t.t1k[j] = tw(j, 1024);
    for (int j = 0; j < 1024; ++j) t.t2k[j] = tw(j, 2048);
}

extern "C" {

int32_t aid_abi_version(void) { return AID_ABI_VERSION; }

const char *aid_last_error(void) { return g_err.c_str(); }

int aid_config_default(int32_t sample_rate, aid_config *out) {
    if (!out || sample_rate <= 0) return fail(AID_ERR_INVALID, "aid_config_default: bad argument");
    std::memset(out, 0, sizeof(*out));
    out->sample_rate = sample_rate;
    out->hop = sample_rate >= 32000 ? 512 : 256;
    out->peak_threshold = 4.0f;
    out->device = -1;
    out->min_match = 10;
    out->max_results = 50;
    return AID_OK;
}

int aid_engine_create(const aid_config *cfg, aid_engine **out) {
    if (!cfg || !out) return fail(AID_ERR_INVALID, "aid_engine_create: null argument");
    *out = nullptr;
    aid_config c = *cfg;
    if (c.sample_rate <= 0) return fail(AID_ERR_INVALID, "sample_rate must be > 0");
    if (c.hop == 0) c.hop = c.sample_rate >= 32000 ? 512 : 256;
    if (c.hop != 128 && c.hop != 256 && c.hop != 512 && c.hop != 1024 && c.hop != 2048)
        return fail(AID_ERR_INVALID, "hop must be one of 128, 256, 512, 1024, 2048");
    if (c.peak_threshold == 0.0f) c.peak_threshold = 4.0f;
    // [2^-124, 2^100]: K1/K2 compare the plane's Q = 4P against 4 thr. In that range 4 thr is exact and
    // any Q of a candidate (Q > 4 thr) is normal, so Q-order and P-order decide every comparison alike
    if (!(c.peak_threshold >= 0x1p-124f) || c.peak_threshold > 0x1p100f)
        return fail(AID_ERR_INVALID, "peak_threshold must be in [2^-124, 2^100]");
    // FPSPEC 5.1: 0 = off; else the clip's threshold is max(peak_threshold, peak_rel * max P). Below 1 (at 1 and
    // above no bin can exceed the threshold); from 2^-60 (the product with any P that matters stays normal)
    if (c.peak_rel != 0.0f && !(c.peak_rel >= 0x1p-60f && c.peak_rel < 1.0f))
        return fail(AID_ERR_INVALID, "peak_rel must be 0 or in [2^-60, 1)");
    if (c.min_match <= 0) c.min_match = 10;
    if (c.max_results <= 0) c.max_results = 50;
    if (c.flags & ~AID_FLAG_KEEP_POWER) return fail(AID_ERR_INVALID, "unknown aid_config.flags bits");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail(AID_ERR_DEVICE, "no HIP device visible");
    int dev = c.device;
    if (dev < 0) HIP_TRY(hipGetDevice(&dev));
    if (dev >= ndev) return fail(AID_ERR_INVALID, "device ordinal out of range");
    HIP_TRY(hipSetDevice(dev));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(AID_ERR_DEVICE, std::string("libaidfp is built for gfx950, device is ") + prop.gcnArchName);
    c.device = dev;

    std::unique_ptr<aid_engine> e(new aid_engine());  // every early return below frees what was built so far
    e->cfg = c;
    e->device = dev;
    for (int w = 0; w < 2; ++w) e->ext.k2_slots[w] = (int64_t)prop.multiProcessorCount * peak_pick_blocks_per_cu(2 + 2 * w);
    e->ext.k1_slots = (int64_t)prop.multiProcessorCount * kStftWaves;
    // blocking stream: ordered against the legacy default stream (torch's default), so device
    // buffers the caller filled there without a stream handle are complete before NULL-stream calls
    hipError_t he = hipStreamCreateWithFlags(&e->own_stream.s, hipStreamDefault);
    if (he != hipSuccess) return fail(AID_ERR_DEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(he));
    std::unique_ptr<Tables> h(new Tables());
    build_tables(*h);
    // K1 derives the real split's mirror twiddle T2K[1024-k] as (-re, im) of T2K[k]
    for (int k = 1; k < 512; ++k)
        if (!(h->t2k[1024 - k].x == -h->t2k[k].x && h->t2k[1024 - k].y == h->t2k[k].y))
            return fail(AID_ERR_DEVICE, "twiddle table lacks the mirror symmetry K1 relies on");
    // K1's DFT16 (aidfp_device.h) shares one product in the cmuls by T16[2], T16[4], T16[6]
    {
        const float2 w2 = h->t16[2], w4 = h->t16[4], w6 = h->t16[6];
        if (!(w2.y == -w2.x && w6.x == w6.y && w6.x == -w2.x && w4.y == -1.0f))
            return fail(AID_ERR_DEVICE, "DFT16 twiddle table lacks the symmetry K1 relies on");
    }
    std::vector<int16_t> sin_tab(4096);
    for (int k = 0; k < 4096; ++k) sin_tab[k] = (int16_t)nearbyint(32767.0 * sin(2.0 * M_PI * (double)k / 4096.0));
    he = e->d_tab.reserve(1);
    if (he == hipSuccess) he = hipMemcpy(e->d_tab.p, h.get(), sizeof(Tables), hipMemcpyHostToDevice);
    if (he == hipSuccess) he = e->d_sin.reserve(4096);
    if (he == hipSuccess) he = hipMemcpy(e->d_sin.p, sin_tab.data(), 4096 * sizeof(int16_t), hipMemcpyHostToDevice);
    if (he != hipSuccess) return fail(AID_ERR_DEVICE, std::string("table upload: ") + hipGetErrorString(he));
    *out = e.release();
    return AID_OK;
}

void aid_engine_destroy(aid_engine *e) {
    if (!e) return;
    // a call still running on another thread (ctypes releases the GIL) holds e->mu: it finishes before anything
    // is freed; the lock is released before the engine itself is deleted below
    std::unique_lock<std::mutex> destroy_lk(e->mu);
    (void)hipSetDevice(e->device);
    if (e->own_stream) (void)hipStreamSynchronize(e->own_stream);
    (void)hipDeviceSynchronize();
    e->ticket_pool.clear();
    destroy_lk.unlock();
    delete e;
}

int aid_live_allocations(int64_t *device, int64_t *pinned, int64_t *events) {
    if (device) *device = g_live.device.load();
    if (pinned) *pinned = g_live.pinned.load();
    if (events) *events = g_live.events.load();
    return AID_OK;
}

int aid_engine_config(const aid_engine *e, aid_config *out) {
    if (!e || !out) return fail(AID_ERR_INVALID, "null argument");
    *out = e->cfg;
    return AID_OK;
}

int aid_engine_force(aid_engine *e, int32_t what, int32_t value) {
    if (!e) return fail(AID_ERR_INVALID, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    switch (what) {
        case AID_FORCE_K5_PATH:
            if (value < 0 || value > 2) return fail(AID_ERR_INVALID, "K5_PATH: 0 auto, 1 as 0, 2 global");
            e->k5_path = value;
            return AID_OK;
        case AID_FORCE_K5_PARTS:
            if (value != 0 && value != 1 && value != 2 && value != 4) return fail(AID_ERR_INVALID, "K5_PARTS: 0, 1, 2 or 4");
            e->k5_parts = value;
            return AID_OK;
        case AID_FORCE_K5_BATCH:
            if (value < 0) return fail(AID_ERR_INVALID, "K5_BATCH must be >= 0");
            e->k5_batch = value ? (size_t)value : 2048;
            return AID_OK;
        case AID_FORCE_K2_STRIPS_X100:
            if (value < 0) return fail(AID_ERR_INVALID, "K2_STRIPS_X100 must be >= 0");
            e->ext.k2.force_slots_x = value / 100.0;
            return AID_OK;
        case AID_FORCE_K2_WIDTH:
            if (value != 0 && value != 2 && value != 4) return fail(AID_ERR_INVALID, "K2_WIDTH: 0 adaptive, 2 or 4");
            e->ext.k2.force_width = value;
            return AID_OK;
        case AID_FORCE_K4_BUILD:
            if (value < 0 || value > 4 || value == 3)  // 3 was a library sort kept for A/B; the number stays retired
                return fail(AID_ERR_INVALID, "K4_BUILD: 0 default, 1 radix, 2 atomic, 4 radix with ballot ranks");
            e->idx.k4_build = value == 2 ? K4Build::kAtomic : K4Build::kRadix;
            e->idx.k4_rank = value == 4 ? 1 : 0;
            e->idx.drop_main(kFallForce);
            return AID_OK;
        case AID_FORCE_EXCHANGE_FAIL:
            if (value != 0 && value != 1) return fail(AID_ERR_INVALID, "EXCHANGE_FAIL: 0 or 1");
            e->idx.inject_exchange_fail = value;
            return AID_OK;
        case AID_FORCE_LANE_GATHER:
            if (value != 0 && value != 1) return fail(AID_ERR_INVALID, "LANE_GATHER: 0 or 1");
            e->lane_gather = value;
            return AID_OK;
        case AID_FORCE_PLANE_ROWS:
            if (value < 0) return fail(AID_ERR_INVALID, "PLANE_ROWS must be >= 0");
            e->ext.plane_rows = value;
            return AID_OK;
        case AID_FORCE_VEC_PATH:
            if (value < 0 || value > 2) return fail(AID_ERR_INVALID, "VEC_PATH: 0 auto, 1 MFMA, 2 VALU");
            e->vec.force_path = value;
            return AID_OK;
        case AID_FORCE_VEC_CHUNK:
            if (value != 0 && (value < 32 || value > 4096 || value % 32))
                return fail(AID_ERR_INVALID, "VEC_CHUNK: 0 default, else a multiple of 32 in [32, 4096]");
            e->vec.force_chunk = value;
            return AID_OK;
        case AID_FORCE_VEC_CAND:
            if (value < 0 || value > kVecCandCap) return fail(AID_ERR_INVALID, "VEC_CAND: 0 default, else in [1, 4096]");
            e->vec.force_cand = value;
            return AID_OK;
        case AID_FORCE_SPEED_GROUP:
            if (value < 0) return fail(AID_ERR_INVALID, "SPEED_GROUP must be >= 0");
            e->speed_group = value;
            return AID_OK;
        case AID_FORCE_K1_WAVES:
            if (value < 0) return fail(AID_ERR_INVALID, "K1_WAVES must be >= 0");
            e->ext.k1_waves = value;
            return AID_OK;
        case AID_FORCE_ROWS_MERGE:
            if (value != 0 && value != 1) return fail(AID_ERR_INVALID, "ROWS_MERGE: 0 or 1");
            e->rows_merge_dev = value;
            return AID_OK;
        default:
            return fail(AID_ERR_INVALID, "aid_engine_force: unknown path id");
    }
}

int aid_synth_rate(aid_engine *e, float *dst, const uint32_t *tracks, const int64_t *starts, int32_t n_clips,
                   int64_t n, int32_t sample_rate, int32_t noise_a, uint32_t salt, int32_t fmax_hz, int32_t flags,
                   void *stream) {
    if (!e || !dst || !tracks || !starts || n_clips < 0 || n < 0 || noise_a < 0 || sample_rate <= 0)
        return fail(AID_ERR_INVALID, "aid_synth: bad argument");
    if (flags & ~(AID_SYNTH_STATIONARY | AID_SYNTH_ASYNC)) return fail(AID_ERR_INVALID, "aid_synth: unknown flags");
    if (sample_rate > 384000) return fail(AID_ERR_INVALID, "aid_synth: sample_rate above 384 kHz");
    if (fmax_hz <= 100 || 2 * (int64_t)fmax_hz > sample_rate)
        return fail(AID_ERR_INVALID, "aid_synth: fmax_hz must be in (100, sample_rate / 2]");
    if (n_clips == 0 || n == 0) return AID_OK;
    std::lock_guard<std::mutex> lk(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = pick_stream(e, stream);
    const bool async = (flags & AID_SYNTH_ASYNC) != 0;
    // the engine's last work on another stream may still read dst; on the same stream it is ordered already
    if (e->last_stream && (!async || e->last_stream != s)) HIP_TRY(hipStreamSynchronize(e->last_stream));
    // the previous call's copies and kernel must have left the pinned staging and the device arrays before a
    // reserve may reallocate them or the copies below overwrite them
    HIP_TRY(e->synth_ev.wait());
    HIP_TRY(e->synth_tracks.reserve(n_clips));
    HIP_TRY(e->synth_starts.reserve(n_clips));
    // tracks + starts go up from pinned staging (the caller's arrays may be gone when an async copy runs)
    const size_t tb = ((size_t)n_clips * sizeof(uint32_t) + 7) & ~(size_t)7, need = tb + (size_t)n_clips * sizeof(int64_t);
    HIP_TRY(e->h_synth.reserve(need));
    std::memcpy(e->h_synth.p, tracks, (size_t)n_clips * sizeof(uint32_t));
    std::memcpy(e->h_synth.p + tb, starts, (size_t)n_clips * sizeof(int64_t));
    HIP_TRY(hipMemcpyAsync(e->synth_tracks.p, e->h_synth.p, n_clips * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->synth_starts.p, e->h_synth.p + tb, n_clips * sizeof(int64_t), hipMemcpyHostToDevice, s));
    {
        ProfScope ps(e, AID_K_SYNTH, s);
        launch_synth(dst, e->synth_tracks.p, e->synth_starts.p, n_clips, n, sample_rate, noise_a, salt, fmax_hz,
                     !(flags & AID_SYNTH_STATIONARY), e->d_sin.p, s);
    }
    HIP_TRY(hipGetLastError());
    // the event covers the kernel's reads of synth_tracks / synth_starts as well as the copies into them, so the
    // next call (any stream) waits for both before it reuses the pinned staging or the device arrays; last_stream
    // makes every later call on another stream wait for this one too
    HIP_TRY(e->synth_ev.record(s));
    e->last_stream = s;
    if (!async) HIP_TRY(hipStreamSynchronize(s));
    return AID_OK;
}

int aid_synth_band(aid_engine *e, float *dst, const uint32_t *tracks, const int64_t *starts, int32_t n_clips,
                   int64_t n, int32_t noise_a, uint32_t salt, int32_t fmax_hz, void *stream) {
    if (!e) return fail(AID_ERR_INVALID, "aid_synth: null engine");
    return aid_synth_rate(e, dst, tracks, starts, n_clips, n, e->cfg.sample_rate, noise_a, salt, fmax_hz, 0, stream);
}

int aid_synth(aid_engine *e, float *dst, const uint32_t *tracks, const int64_t *starts, int32_t n_clips, int64_t n,
              int32_t noise_a, uint32_t salt, void *stream) {
    return aid_synth_band(e, dst, tracks, starts, n_clips, n, noise_a, salt, 8000, stream);
}

int aid_resample_plan(int32_t sr_in, int32_t sr_out, int32_t *up, int32_t *down, int32_t *hl, int32_t *J) {
    ResamplePlan p;
    if (!resample_plan(sr_in, sr_out, p)) return 0;
    if (up) *up = p.up;
    if (down) *down = p.down;
    if (hl) *hl = p.hl;
    if (J) *J = p.J;
    return 1;
}

int64_t aid_resample_len(int64_t n, int32_t sr_in, int32_t sr_out) {
    ResamplePlan p;
    if (n <= 0 || !resample_plan(sr_in, sr_out, p)) return 0;
    return (n * p.up + p.down - 1) / p.down;
}

}  // extern "C"

// impulse: the unit impulse at the filter's centre instead of the designed taps (cached under -down); shared with
// speed.cpp (engine_internal.h)
int resample_taps_dev(aid_engine *e, const ResamplePlan &p, bool impulse, float **out) {
    const std::pair<int32_t, int32_t> key{p.up, impulse ? -p.down : p.down};
    auto it = e->rs_taps.find(key);
    if (it != e->rs_taps.end()) {
        *out = it->second.p;
        return AID_OK;
    }
    std::vector<float> h = resample_phase_taps(p);
    if (impulse) {
        std::fill(h.begin(), h.end(), 0.0f);
        h[(size_t)(p.hl % p.up) * p.J + p.hl / p.up] = 1.0f;  // taps[k], k = phase + j * up = hl
    }
    DevBuf<float> taps;
    HIP_TRY(taps.reserve(h.size()));
    hipError_t he = hipMemcpy(taps.p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice);
    if (he != hipSuccess) return fail(AID_ERR_DEVICE, std::string("aid_resample: ") + hipGetErrorString(he));
    *out = taps.p;
    e->rs_taps[key] = std::move(taps);
    return AID_OK;
}

extern "C" {

int aid_resample_range(aid_engine *e, const float *src, int64_t in_base, int64_t n, int32_t channels, int32_t sr_in,
                       int32_t sr_out, int64_t m_first, int64_t count, float *dst, void *stream) {
    return aid_resample_batch(e, src, 0, 1, in_base, n, channels, sr_in, sr_out, m_first, count, dst, 0, stream);
}

// src / hist are samples of `fmt` and the strides count them; a stereo frame must be aligned to its own size
// (8 bytes of float, 4 of s16: the kernels read it as one word)
static int resample_batch(aid_engine *e, const void *src, PcmFmt fmt, int64_t src_stride, int32_t n_streams,
                          int64_t in_base, int64_t n, int32_t channels, int32_t sr_in, int32_t sr_out, int64_t m_first,
                          int64_t count, float *dst, int64_t dst_stride, void *stream, const void *hist, int64_t hist_n,
                          int64_t hist_stride) {
    const uintptr_t frame_mask = 2 * pcm_size(fmt) - 1;
    if (!e || n < 0 || in_base < 0 || m_first < 0 || count < 0 || (channels != 1 && channels != 2) || n_streams < 0 ||
        n_streams > 65535 || src_stride < 0 || dst_stride < 0 || hist_n < 0 || hist_n > in_base || hist_stride < 0)
        return fail(AID_ERR_INVALID, "aid_resample: bad argument");
    if (n_streams > 1 && (src_stride < n * channels || dst_stride < count || (channels == 2 && (src_stride & 1))))
        return fail(AID_ERR_INVALID, "aid_resample_batch: strides must cover one stream (stereo: even)");
    if (hist_n > 0 && (!hist || (n_streams > 1 && hist_stride < hist_n * channels) ||
                       (channels == 2 && ((hist_stride & 1) || (reinterpret_cast<uintptr_t>(hist) & frame_mask)))))
        return fail(AID_ERR_INVALID, "aid_resample_batch_split: bad history (null, stride, or stereo alignment)");
    if (n_streams == 0) return AID_OK;
    ResamplePlan p;
    if (!resample_plan(sr_in, sr_out, p)) return fail(AID_ERR_INVALID, "aid_resample: sample rates must be > 0");
    if (count == 0) return AID_OK;
    if (!dst || (n > 0 && !src)) return fail(AID_ERR_INVALID, "aid_resample: null buffer");
    if (channels == 2 && (reinterpret_cast<uintptr_t>(src) & frame_mask))
        return fail(AID_ERR_INVALID, fmt == kS16 ? "aid_resample: stereo s16 src must be 4-byte aligned"
                                                 : "aid_resample: stereo src must be 8-byte aligned");
    if (channels == 1 && fmt == kS16 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(hist)) & 1))
        return fail(AID_ERR_INVALID, "aid_resample: s16 src must be 2-byte aligned");
    if (const ResLaunch pl = resample_launch_plan(p.up, p.down, p.J); pl.path == kResReject)
        return fail(AID_ERR_INVALID, std::string("aid_resample: ") + resample_status_text(pl.status));
    std::lock_guard<std::mutex> lk(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = pick_stream(e, stream);
    float *taps = nullptr;
    // up == down copies (FPSPEC 8). Integer PCM gets exactly the copy from the same kernels through a unit-impulse
    // table: fma(1, x, +0) = x and every other tap adds +0, and an s16 sample is never -0. The float path keeps the
    // designed taps it has always used there (off-centre ~1e-17, not 0)
    if (int rc = resample_taps_dev(e, p, fmt == kS16 && p.up == p.down, &taps)) return rc;
    {
        ProfScope ps(e, AID_K_RESAMPLE, s);
        launch_resample(src, fmt == kS16, in_base, n, channels, p.up, p.down, p.hl, p.J, taps, dst, m_first, count, s, n_streams,
                        src_stride, dst_stride, hist, hist_n, hist_stride);
    }
    HIP_TRY(hipGetLastError());
    return AID_OK;
}

int aid_resample_batch(aid_engine *e, const float *src, int64_t src_stride, int32_t n_streams, int64_t in_base, int64_t n,
                       int32_t channels, int32_t sr_in, int32_t sr_out, int64_t m_first, int64_t count, float *dst,
                       int64_t dst_stride, void *stream) {
    return resample_batch(e, src, kF32, src_stride, n_streams, in_base, n, channels, sr_in, sr_out, m_first, count, dst,
                          dst_stride, stream, nullptr, 0, 0);
}

int aid_resample_batch_split(aid_engine *e, const float *hist, int64_t hist_stride, int64_t hist_n, const float *src,
                             int64_t src_stride, int32_t n_streams, int64_t in_base, int64_t n, int32_t channels,
                             int32_t sr_in, int32_t sr_out, int64_t m_first, int64_t count, float *dst,
                             int64_t dst_stride, void *stream) {
    return resample_batch(e, src, kF32, src_stride, n_streams, in_base, n, channels, sr_in, sr_out, m_first, count, dst,
                          dst_stride, stream, hist, hist_n, hist_stride);
}

int aid_resample_batch_split_s16(aid_engine *e, const int16_t *hist, int64_t hist_stride, int64_t hist_n,
                                 const int16_t *src, int64_t src_stride, int32_t n_streams, int64_t in_base, int64_t n,
                                 int32_t channels, int32_t sr_in, int32_t sr_out, int64_t m_first, int64_t count,
                                 float *dst, int64_t dst_stride, void *stream) {
    return resample_batch(e, src, kS16, src_stride, n_streams, in_base, n, channels, sr_in, sr_out, m_first, count, dst,
                          dst_stride, stream, hist, hist_n, hist_stride);
}

static int resample_whole(aid_engine *e, const void *src, PcmFmt fmt, int64_t n, int32_t channels, int32_t sr_in,
                          int32_t sr_out, float *dst, int64_t cap, int64_t *n_out, void *stream) {
    if (!e || n < 0 || (channels != 1 && channels != 2)) return fail(AID_ERR_INVALID, "aid_resample: bad argument");
    const int64_t m = aid_resample_len(n, sr_in, sr_out);
    if (n > 0 && m == 0) return fail(AID_ERR_INVALID, "aid_resample: sample rates must be > 0");
    if (n_out) *n_out = m;
    if (m > cap) return fail(AID_ERR_INVALID, "aid_resample: output capacity too small");
    if (m == 0) return AID_OK;
    if (sr_in == sr_out && channels == 1) {  // same rate, mono: a copy
        if (!src || !dst) return fail(AID_ERR_INVALID, "aid_resample: null buffer");
        std::lock_guard<std::mutex> lk(e->mu);
        HIP_TRY(hipSetDevice(e->device));
        if (fmt == kS16) {  // the copy converts
            if (reinterpret_cast<uintptr_t>(src) & 1) return fail(AID_ERR_INVALID, "aid_resample: s16 src must be 2-byte aligned");
            launch_s16_to_f32(static_cast<const int16_t *>(src), n, dst, pick_stream(e, stream));
            HIP_TRY(hipGetLastError());
            return AID_OK;
        }
        HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, pick_stream(e, stream)));
        return AID_OK;
    }
    return resample_batch(e, src, fmt, 0, 1, 0, n, channels, sr_in, sr_out, 0, m, dst, 0, stream, nullptr, 0, 0);
}

int aid_resample(aid_engine *e, const float *src, int64_t n, int32_t channels, int32_t sr_in, int32_t sr_out,
                 float *dst, int64_t cap, int64_t *n_out, void *stream) {
    return resample_whole(e, src, kF32, n, channels, sr_in, sr_out, dst, cap, n_out, stream);
}

int aid_resample_s16(aid_engine *e, const int16_t *src, int64_t n, int32_t channels, int32_t sr_in, int32_t sr_out,
                     float *dst, int64_t cap, int64_t *n_out, void *stream) {
    return resample_whole(e, src, kS16, n, channels, sr_in, sr_out, dst, cap, n_out, stream);
}

int aid_dedup_reset(aid_engine *e) {
    if (!e) return fail(AID_ERR_INVALID, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    e->dd_n = 0;
    e->dd_nw = 0;
    return AID_OK;
}

int aid_dedup_count(aid_engine *e, int64_t *n_entries, int64_t *n_words) {
    if (!e) return fail(AID_ERR_INVALID, "null engine");
    if (n_entries) *n_entries = e->dd_n;
    if (n_words) *n_words = e->dd_nw;
    return AID_OK;
}

static int check_offsets(const int64_t *off, int32_t n, const char *what) {
    if (off[0] != 0) return fail(AID_ERR_INVALID, std::string(what) + ": offsets[0] must be 0");
    for (int32_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return fail(AID_ERR_INVALID, std::string(what) + ": offsets must be non-decreasing");
    return AID_OK;
}

// words: host or device (loc); a device array is copied in stream order on the engine's own stream
static int dedup_add(aid_engine *e, const uint32_t *words, const int64_t *offsets, const double *durations, int32_t n,
                     int32_t loc) {
    if (!e || n < 0 || (n > 0 && (!offsets || !durations)) || (loc != AID_PCM_HOST && loc != AID_PCM_DEVICE))
        return fail(AID_ERR_INVALID, "aid_dedup_add: bad argument");
    if (n == 0) return AID_OK;
    if (int rc = check_offsets(offsets, n, "aid_dedup_add")) return rc;
    const int64_t nw = offsets[n];
    if (nw > 0 && !words) return fail(AID_ERR_INVALID, "aid_dedup_add: null words");
    EngineCall call(e, nullptr, false, kDrainLast);
    if (call.rc) return call.rc;
    hipStream_t s = call.s;
    HIP_TRY(e->dd_words.grow_keep((size_t)e->dd_nw, (size_t)(e->dd_nw + nw + 1), s));
    HIP_TRY(e->dd_off.grow_keep((size_t)e->dd_n + 1, (size_t)(e->dd_n + n + 1), s));
    HIP_TRY(e->dd_dur.grow_keep((size_t)e->dd_n, (size_t)(e->dd_n + n), s));
    std::vector<int64_t> off(n + 1);
    for (int32_t i = 0; i <= n; ++i) off[i] = e->dd_nw + offsets[i];
    if (nw > 0)
        HIP_TRY(hipMemcpyAsync(e->dd_words.p + e->dd_nw, words, nw * sizeof(uint32_t),
                               loc == AID_PCM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->dd_off.p + e->dd_n, off.data(), (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->dd_dur.p + e->dd_n, durations, n * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    e->dd_n += n;
    e->dd_nw += nw;
    return AID_OK;
}

int aid_dedup_add(aid_engine *e, const uint32_t *words, const int64_t *offsets, const double *durations, int32_t n) {
    return dedup_add(e, words, offsets, durations, n, AID_PCM_HOST);
}

int aid_dedup_add_at(aid_engine *e, const uint32_t *words, const int64_t *offsets, const double *durations, int32_t n,
                     int32_t location) {
    return dedup_add(e, words, offsets, durations, n, location);
}

// words: host (copied to the scan's scratch) or device (K7 reads them in place)
static int dedup_scan(aid_engine *e, const uint32_t *words, const int64_t *offsets, const double *durations, int32_t nq,
                      int32_t loc, int64_t *best_idx, double *best_sim) {
    if (!e || nq < 0 || (nq > 0 && (!offsets || !durations || !best_idx || !best_sim)) ||
        (loc != AID_PCM_HOST && loc != AID_PCM_DEVICE))
        return fail(AID_ERR_INVALID, "aid_dedup_scan: bad argument");
    if (nq == 0) return AID_OK;
    if (int rc = check_offsets(offsets, nq, "aid_dedup_scan")) return rc;
    const int64_t nw = offsets[nq];
    if (nw > 0 && !words) return fail(AID_ERR_INVALID, "aid_dedup_scan: null words");
    EngineCall call(e, nullptr, false, kDrainLast);
    if (call.rc) return call.rc;
    hipStream_t s = call.s;
    const int nc = std::max(1, dedup_chunks(e->dd_n));
    std::vector<double> lo(nq), hi(nq);
    for (int32_t q = 0; q < nq; ++q) {  // the reference's SQL bounds (dedup.py:193-194)
        lo[q] = durations[q] * 0.9;
        hi[q] = durations[q] * 1.1;
    }
    HIP_TRY(e->dq_words.reserve((size_t)nw + 1));
    HIP_TRY(e->dq_off.reserve((size_t)nq + 1));
    HIP_TRY(e->dq_lo.reserve((size_t)nq));
    HIP_TRY(e->dq_hi.reserve((size_t)nq));
    HIP_TRY(e->dq_sim.reserve((size_t)nq));
    HIP_TRY(e->dq_idx.reserve((size_t)nq));
    HIP_TRY(e->dq_psim.reserve((size_t)nq * nc));
    HIP_TRY(e->dq_pidx.reserve((size_t)nq * nc));
    const uint32_t *qw = e->dq_words.p;
    if (loc == AID_PCM_DEVICE && nw > 0)
        qw = words;
    else if (nw > 0)
        HIP_TRY(hipMemcpyAsync(e->dq_words.p, words, nw * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->dq_off.p, offsets, (nq + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->dq_lo.p, lo.data(), nq * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->dq_hi.p, hi.data(), nq * sizeof(double), hipMemcpyHostToDevice, s));
    {
        ProfScope ps(e, AID_K_DEDUP, s);
        launch_dedup_scan(e->dd_words.p, e->dd_off.p, e->dd_dur.p, e->dd_n, qw, e->dq_off.p, e->dq_lo.p,
                          e->dq_hi.p, nq, e->dq_psim.p, e->dq_pidx.p, e->dq_sim.p, e->dq_idx.p, s);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(best_idx, e->dq_idx.p, nq * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(best_sim, e->dq_sim.p, nq * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return AID_OK;
}

int aid_dedup_scan(aid_engine *e, const uint32_t *words, const int64_t *offsets, const double *durations, int32_t nq,
                   int64_t *best_idx, double *best_sim) {
    return dedup_scan(e, words, offsets, durations, nq, AID_PCM_HOST, best_idx, best_sim);
}

int aid_dedup_scan_at(aid_engine *e, const uint32_t *words, const int64_t *offsets, const double *durations,
                      int32_t nq, int32_t location, int64_t *best_idx, double *best_sim) {
    return dedup_scan(e, words, offsets, durations, nq, location, best_idx, best_sim);
}

int aid_dedup_pairs(aid_engine *e, const uint32_t *a, const int64_t *a_off, const uint32_t *b, const int64_t *b_off,
                    int32_t n, double *sim) {
    if (!e || n < 0 || (n > 0 && (!a_off || !b_off || !sim))) return fail(AID_ERR_INVALID, "aid_dedup_pairs: bad argument");
    if (n == 0) return AID_OK;
    if (int rc = check_offsets(a_off, n, "aid_dedup_pairs")) return rc;
    if (int rc = check_offsets(b_off, n, "aid_dedup_pairs")) return rc;
    const int64_t na = a_off[n], nb = b_off[n];
    if ((na > 0 && !a) || (nb > 0 && !b)) return fail(AID_ERR_INVALID, "aid_dedup_pairs: null words");
    EngineCall call(e);
    if (call.rc) return call.rc;
    hipStream_t s = call.s;
    HIP_TRY(e->dq_words.reserve((size_t)na + 1));
    HIP_TRY(e->dq_words2.reserve((size_t)nb + 1));
    HIP_TRY(e->dq_off.reserve((size_t)n + 1));
    HIP_TRY(e->dq_off2.reserve((size_t)n + 1));
    HIP_TRY(e->dq_sim.reserve((size_t)n));
    if (na > 0) HIP_TRY(hipMemcpyAsync(e->dq_words.p, a, na * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if (nb > 0) HIP_TRY(hipMemcpyAsync(e->dq_words2.p, b, nb * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->dq_off.p, a_off, (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->dq_off2.p, b_off, (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    launch_dedup_pairs(e->dq_words.p, e->dq_off.p, e->dq_words2.p, e->dq_off2.p, n, e->dq_sim.p, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(sim, e->dq_sim.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return AID_OK;
}

// ---- vector lane (FPSPEC 9): thin wrappers over csrc/vector.hip, one critical section per call
#define VEC_CALL(e, stream, call)                      \
    do {                                               \
        EngineCall ec(e, stream, false, kDrainLast);   \
        if (ec.rc) return ec.rc;                       \
        hipStream_t s = ec.s;                          \
        (void)s;                                       \
        const int rc = (call);                         \
        return rc ? fail(rc, (e)->vec.err) : AID_OK;   \
    } while (0)

int aid_vec_reset(aid_engine *e, int32_t dim) { VEC_CALL(e, nullptr, vec_reset(e->vec, dim)); }

int aid_vec_add(aid_engine *e, const float *vecs, const uint32_t *tracks, const int32_t *chunk_index,
                const double *offset_sec, int64_t n, int32_t location) {
    VEC_CALL(e, nullptr, vec_add(e->vec, vecs, tracks, chunk_index, offset_sec, nullptr, n, location, s));
}

int aid_vec_add_tagged(aid_engine *e, const float *vecs, const uint32_t *tracks, const int32_t *chunk_index,
                       const double *offset_sec, const uint64_t *tags, int64_t n, int32_t location) {
    VEC_CALL(e, nullptr, vec_add(e->vec, vecs, tracks, chunk_index, offset_sec, tags, n, location, s));
}

int aid_vec_retag(aid_engine *e, uint32_t track, uint64_t tags) { VEC_CALL(e, nullptr, vec_retag(e->vec, track, tags)); }

int aid_vec_tags(aid_engine *e, uint64_t *out, int64_t cap) { VEC_CALL(e, nullptr, vec_tags(e->vec, out, cap)); }

int aid_vec_remove(aid_engine *e, uint32_t track) { VEC_CALL(e, nullptr, vec_remove(e->vec, track, s)); }

int aid_vec_compact(aid_engine *e, int64_t *n_removed) { VEC_CALL(e, nullptr, vec_compact(e->vec, n_removed, s)); }

int aid_vec_count(aid_engine *e, int64_t *n_entries, int64_t *n_live, int32_t *dim) {
    if (!e) return fail(AID_ERR_INVALID, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    if (n_entries) *n_entries = e->vec.n;
    if (n_live) *n_live = e->vec.n_live;
    if (dim) *dim = e->vec.dim;
    return AID_OK;
}

int aid_vec_search(aid_engine *e, const float *queries, int32_t nq, int32_t location, int32_t limit,
                   aid_vec_hit *hits, int32_t *n_hits, void *stream) {
    VEC_CALL(e, stream, vec_search(e->vec, queries, nq, location, limit, nullptr, hits, n_hits, s));
}

int aid_vec_search_filtered(aid_engine *e, const float *queries, int32_t nq, int32_t location, int32_t limit,
                            const aid_vec_filter *filters, aid_vec_hit *hits, int32_t *n_hits, void *stream) {
    VEC_CALL(e, stream, vec_search(e->vec, queries, nq, location, limit, filters, hits, n_hits, s));
}

int aid_vec_scores(aid_engine *e, const float *queries, int32_t nq, int32_t location, float *out, int64_t cap) {
    VEC_CALL(e, nullptr, vec_scores(e->vec, queries, nq, location, out, cap, s));
}

int aid_vec_aggregate(aid_engine *e, const aid_vec_hit *hits, const int64_t *hoff, int32_t nq, int32_t top_k_per_track,
                      double diversity_weight, const uint32_t *exclude, double threshold, int32_t max_out,
                      aid_vibe_row *out, int32_t *n_out) {
    VEC_CALL(e, nullptr, vec_aggregate(e->vec, hits, hoff, nq, top_k_per_track, diversity_weight, exclude, threshold,
                                       max_out, out, n_out, s));
}

int aid_vibe_lane(aid_engine *e, const float *queries, int32_t nq, int32_t location, int32_t limit,
                  int32_t top_k_per_track, double diversity_weight, const uint32_t *exclude, double threshold,
                  int32_t max_out, aid_vibe_row *out, int32_t *n_out, void *stream) {
    VEC_CALL(e, stream, vec_lane(e->vec, queries, nq, location, limit, top_k_per_track, diversity_weight, nullptr, exclude,
                                 threshold, max_out, out, n_out, s));
}

int aid_vibe_lane_filtered(aid_engine *e, const float *queries, int32_t nq, int32_t location, int32_t limit,
                           int32_t top_k_per_track, double diversity_weight, const aid_vec_filter *filters,
                           const uint32_t *exclude, double threshold, int32_t max_out, aid_vibe_row *out,
                           int32_t *n_out, void *stream) {
    VEC_CALL(e, stream, vec_lane(e->vec, queries, nq, location, limit, top_k_per_track, diversity_weight, filters, exclude,
                                 threshold, max_out, out, n_out, s));
}

int aid_vec_save(aid_engine *e, const char *path) { VEC_CALL(e, nullptr, vec_save(e->vec, path, s)); }

int aid_vec_load(aid_engine *e, const char *path) { VEC_CALL(e, nullptr, vec_load(e->vec, path, s)); }

int aid_vec_stats(aid_engine *e, int64_t *out, int32_t n, int32_t reset) {
    if (!e || (n > 0 && !out)) return fail(AID_ERR_INVALID, "aid_vec_stats: bad argument");
    std::lock_guard<std::mutex> lk(e->mu);
    for (int i = 0; i < n && i < kVecStats; ++i) out[i] = e->vec.st[i];
    if (reset)
        for (auto &v : e->vec.st) v = 0;
    return AID_OK;
}

int aid_vec_prefilter(aid_engine *e, int32_t mode, int32_t oversample) {
    VEC_CALL(e, nullptr, vec_prefilter(e->vec, mode, oversample, s));
}

int aid_vec_scores_i8(aid_engine *e, const float *queries, int32_t nq, int32_t location, float *approx_out,
                      double *eps_out, int64_t cap) {
    VEC_CALL(e, nullptr, vec_scores_i8(e->vec, queries, nq, location, approx_out, eps_out, cap, s));
}

int aid_vec_prefilter_stats(aid_engine *e, int64_t *out, int32_t n, int32_t reset) {
    if (!e || (n > 0 && !out)) return fail(AID_ERR_INVALID, "aid_vec_prefilter_stats: bad argument");
    std::lock_guard<std::mutex> lk(e->mu);
    for (int i = 0; i < n && i < kVecQ8Stats; ++i) out[i] = e->vec.q8st[i];
    if (reset)
        for (auto &v : e->vec.q8st) v = 0;
    return AID_OK;
}

int aid_profile_enable(aid_engine *e, int32_t on) {
    if (!e) return fail(AID_ERR_INVALID, "null engine");
    e->profiling = on != 0;
    return AID_OK;
}

int aid_profile_select(aid_engine *e, uint32_t kernel_mask) {
    if (!e) return fail(AID_ERR_INVALID, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    e->prof_mask = kernel_mask;
    return AID_OK;
}

int aid_profile_read(aid_engine *e, double *ms, int64_t *launches, int32_t reset) {
    if (!e) return fail(AID_ERR_INVALID, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    for (auto &p : e->pending) {
        HIP_TRY(hipEventSynchronize(p.b));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, p.a, p.b));
        e->prof_ms[p.kernel] += t;
        e->prof_n[p.kernel] += 1;
        e->pool.push_back(p.a);
        e->pool.push_back(p.b);
    }
    e->pending.clear();
    for (int k = 0; k < AID_K_COUNT; ++k) {
        if (ms) ms[k] = e->prof_ms[k];
        if (launches) launches[k] = e->prof_n[k];
    }
    if (reset)
        for (int k = 0; k < AID_K_COUNT; ++k) {
            e->prof_ms[k] = 0;
            e->prof_n[k] = 0;
        }
    return AID_OK;
}

int aid_match_stats(aid_engine *e, int64_t *out, int32_t n, int32_t reset) {
    if (!e || (n > 0 && !out)) return fail(AID_ERR_INVALID, "aid_match_stats: bad argument");
    std::lock_guard<std::mutex> lk(e->mu);
    const int64_t v[15] = {e->st_queries,     e->st_votes,   e->st_post_reads, e->st_q_lds,
                           e->st_q_global,    e->st_records, e->st_sig_reads,  (int64_t)match_lds_blocks_per_cu(),
                           e->st_fb_reason[0], e->st_fb_reason[1], e->st_fb_reason[2], e->st_fb_reason[3],
                           e->st_fb_reason[4], e->ext.k2.width, e->ext.plan.strips};
    for (int i = 0; i < n && i < 15; ++i) out[i] = v[i];
    if (reset) {
        e->st_queries = e->st_votes = e->st_post_reads = e->st_q_lds = e->st_q_global = e->st_records = e->st_sig_reads = 0;
        for (auto &r : e->st_fb_reason) r = 0;
    }
    return AID_OK;
}

}  // extern "C"

extern "C" int aid_downmix(aid_engine *e, const float *stereo, int64_t n_frames, float *mono, void *stream) {
    if (!e || n_frames < 0 || (n_frames > 0 && (!stereo || !mono))) return fail(AID_ERR_INVALID, "aid_downmix: bad argument");
    if (((uintptr_t)stereo & 15) || ((uintptr_t)mono & 7)) return fail(AID_ERR_INVALID, "aid_downmix: misaligned buffers");
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = pick_stream(e, stream);
    launch_downmix(stereo, n_frames, mono, s);
    HIP_TRY(hipGetLastError());
    return AID_OK;
}
