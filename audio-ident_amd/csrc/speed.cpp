// speed.cpp -- the speed-tolerant exact lane (FPSPEC 8.2, 7.1): aid_speed_plan / aid_speed_len, aid_resample_speeds
// (K6s: every speed variant of every clip in one launch) and aid_exact_lane_speeds (per clip group: K6s into an
// engine-owned buffer, the exact lane over the group's (clip, speed) pairs read in place, K8c speed selection; only
// the winners' rows, counts and speeds leave the device). The plan is aidfp_speed_plan.h's; the lane is query.cpp's.
#include <cstring>

#include "engine_internal.h"

namespace {

int speed_fail(const char *fn, int st) { return fail(AID_ERR_INVALID, std::string(fn) + ": " + speed_status_text(st)); }

// what both entry points check before they plan: the clips' frames and the samples' alignment
int check_speed_args(const char *fn, aid_engine *e, const void *pcm, PcmFmt fmt, const int64_t *offsets, int32_t n_clips,
                     int32_t channels, const int32_t *speeds_pm, int32_t loc) {
    const std::string f(fn);
    if (!e || !offsets || n_clips < 0 || (channels != 1 && channels != 2) || !speeds_pm)
        return fail(AID_ERR_INVALID, f + ": bad argument");
    for (int c = 0; c < n_clips; ++c)
        if (offsets[c + 1] < offsets[c] || offsets[c] < 0)
            return fail(AID_ERR_INVALID, f + ": offsets must be non-decreasing and >= 0");
    if (n_clips > 0 && !pcm && offsets[n_clips] > offsets[0]) return fail(AID_ERR_INVALID, f + ": null pcm");
    // device PCM is read in place: a stereo frame is one word (8 bytes of float, 4 of s16), an s16 sample 2 bytes
    const uintptr_t mask = loc == AID_PCM_DEVICE ? (channels == 2 ? 2 * pcm_size(fmt) - 1 : pcm_size(fmt) - 1) : 0;
    if (reinterpret_cast<uintptr_t>(pcm) & mask) return fail(AID_ERR_INVALID, f + ": pcm must be aligned to one frame");
    return AID_OK;
}

// the call's tables to the device, behind the last K6s launch that read them: [clip_off | dst_off | blk_first] and
// [SpeedVarDev per speed | the speeds]. Engine lock held, e->sp_plan planned
int upload_speed_tables(aid_engine *e, const int32_t *speeds_pm, hipStream_t s) {
    const SpeedPlan &p = e->sp_plan;
    HIP_TRY(e->sp_ev.wait());
    const size_t n_pairs = (size_t)p.n_clips * p.n_speeds, n_idx = (size_t)p.n_clips + 1 + 2 * (n_pairs + 1);
    const size_t var_bytes = (size_t)p.n_speeds * (sizeof(SpeedVarDev) + sizeof(int32_t));
    HIP_TRY(e->sp_hidx.reserve(n_idx));
    HIP_TRY(e->sp_hvar.reserve(var_bytes));
    HIP_TRY(e->sp_idx.reserve(n_idx));
    HIP_TRY(e->sp_var.reserve(var_bytes));
    int64_t *h = e->sp_hidx.p;
    std::memcpy(h, p.clip_off.data(), ((size_t)p.n_clips + 1) * sizeof(int64_t));
    std::memcpy(h + p.n_clips + 1, p.dst_off.data(), (n_pairs + 1) * sizeof(int64_t));
    std::memcpy(h + p.n_clips + 1 + n_pairs + 1, p.blk_first.data(), (n_pairs + 1) * sizeof(int64_t));
    SpeedVarDev *hv = reinterpret_cast<SpeedVarDev *>(e->sp_hvar.p);
    for (int v = 0; v < p.n_speeds; ++v) {
        const ResamplePlan &r = p.var[v];
        float *taps = nullptr;
        // up == down copies (FPSPEC 8): no table is read
        if (r.up != r.down)
            if (int rc = resample_taps_dev(e, r, false, &taps)) return rc;
        hv[v] = SpeedVarDev{r.up, r.down, r.hl, r.J, taps, r.up == r.down ? 1 : 0, 0};
    }
    std::memcpy(hv + p.n_speeds, speeds_pm, (size_t)p.n_speeds * sizeof(int32_t));
    HIP_TRY(hipMemcpyAsync(e->sp_idx.p, h, n_idx * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->sp_var.p, hv, var_bytes, hipMemcpyHostToDevice, s));
    return AID_OK;
}

// K6s over the pairs of clips [first, first + n): their variants packed from dst[0] on
int launch_group(aid_engine *e, const void *src, PcmFmt fmt, int channels, int first, int n, float *dst, hipStream_t s) {
    const SpeedPlan &p = e->sp_plan;
    const size_t n_pairs = (size_t)p.n_clips * p.n_speeds, a = (size_t)first * p.n_speeds, b = a + (size_t)n * p.n_speeds;
    const int64_t *clip_off = e->sp_idx.p, *dst_off = clip_off + p.n_clips + 1, *blk_first = dst_off + n_pairs + 1;
    {
        ProfScope ps(e, AID_K_RESAMPLE_SPEEDS, s);
        launch_resample_speeds(src, fmt == kS16, channels, clip_off, reinterpret_cast<const SpeedVarDev *>(e->sp_var.p),
                               p.n_speeds, blk_first, dst_off, (int)a, (int)(b - a), p.blk_first[b] - p.blk_first[a],
                               p.lds_floats, dst, s);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(e->sp_ev.record(s));
    return AID_OK;
}

int resample_speeds_entry(const char *fn, aid_engine *e, const void *src, PcmFmt fmt, const int64_t *offsets,
                          int32_t n_clips, int32_t channels, int32_t sr_in, const int32_t *speeds_pm, int32_t n_speeds,
                          float *dst, int64_t cap, int64_t *dst_offsets, void *stream) {
    if (int rc = check_speed_args(fn, e, src, fmt, offsets, n_clips, channels, speeds_pm, AID_PCM_DEVICE)) return rc;
    if (!dst_offsets || cap < 0) return fail(AID_ERR_INVALID, std::string(fn) + ": bad argument");
    std::lock_guard<std::mutex> lk(e->mu);
    SpeedPlan &p = e->sp_plan;
    if (int st = plan_speeds(p, offsets, n_clips, sr_in, e->cfg.sample_rate, speeds_pm, n_speeds, INT64_MAX))
        return speed_fail(fn, st);
    std::memcpy(dst_offsets, p.dst_off.data(), p.dst_off.size() * sizeof(int64_t));
    if (p.total() > cap) return fail(AID_ERR_INVALID, std::string(fn) + ": output capacity too small");
    if (p.total() == 0) return AID_OK;
    if (!dst) return fail(AID_ERR_INVALID, std::string(fn) + ": null buffer");
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = pick_stream(e, stream);
    if (int rc = upload_speed_tables(e, speeds_pm, s)) return rc;
    return launch_group(e, pcm_at(src, fmt, offsets[0] * channels), fmt, channels, 0, n_clips, dst, s);
}

int lane_speeds_locked(const char *fn, aid_engine *e, const void *pcm, PcmFmt fmt, const int64_t *offsets,
                       int32_t n_clips, int32_t loc, int32_t channels, int32_t sr_in, const int32_t *speeds_pm,
                       int32_t n_speeds, int32_t max_out, aid_exact_row *out, int32_t *n_out, int32_t *speed_pm_out,
                       void *stream) {
    SpeedPlan &p = e->sp_plan;
    if (int st = plan_speeds(p, offsets, n_clips, sr_in, e->cfg.sample_rate, speeds_pm, n_speeds, e->speed_group))
        return speed_fail(fn, st);
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = ensure_index(e)) return rc;
    hipStream_t s = pick_stream(e, stream);
    if (e->last_stream && e->last_stream != s) HIP_TRY(hipStreamSynchronize(e->last_stream));
    if (int rc = upload_speed_tables(e, speeds_pm, s)) return rc;
    const void *src = pcm_at(pcm, fmt, offsets[0] * channels);
    if (loc == AID_PCM_HOST) {  // one copy of the clips' span, as aid_extract stages host PCM
        const size_t nbytes = (size_t)(offsets[n_clips] - offsets[0]) * channels * pcm_size(fmt);
        HIP_TRY(e->sp_in.reserve(std::max<size_t>((nbytes + sizeof(float) - 1) / sizeof(float), 1)));
        if (nbytes > 0) HIP_TRY(hipMemcpyAsync(e->sp_in.p, src, nbytes, hipMemcpyHostToDevice, s));
        src = e->sp_in.p;
    }
    int64_t group_floats = 2;
    size_t group_pairs = 0;
    for (const SpeedGroup &g : p.groups) {
        group_floats = std::max(group_floats, g.floats);
        group_pairs = std::max(group_pairs, (size_t)g.n * n_speeds);
    }
    HIP_TRY(e->sp_pcm.reserve((size_t)group_floats));
    HIP_TRY(e->sp_sel.reserve((size_t)n_clips * max_out * 3));
    HIP_TRY(e->sp_seln.reserve((size_t)2 * n_clips));
    int32_t *sel_n = e->sp_seln.p, *sel_pm = sel_n + n_clips;
    const int32_t *pm_dev = reinterpret_cast<const int32_t *>(e->sp_var.p + (size_t)n_speeds * sizeof(SpeedVarDev));
    std::vector<int64_t> goff(group_pairs + 1);
    for (const SpeedGroup &g : p.groups) {
        const size_t a = (size_t)g.first * n_speeds, np = (size_t)g.n * n_speeds;
        if (int rc = launch_group(e, src, fmt, channels, g.first, g.n, e->sp_pcm.p, s)) return rc;
        for (size_t k = 0; k <= np; ++k) goff[k] = p.dst_off[a + k] - p.dst_off[a];
        // every variant is a clip in its own right at the engine's rate: its own window plan, K1-K5, K8b
        if (int rc = exact_lane_device(e, e->sp_pcm.p, kF32, goff.data(), (int32_t)np, AID_PCM_DEVICE, max_out, s))
            return rc;
        {
            ProfScope ps(e, AID_K_SPEED_SELECT, s);
            launch_speed_select(e->x_out.p, e->x_nout.p, max_out, pm_dev, n_speeds, g.n,
                                e->sp_sel.p + (size_t)g.first * max_out * 3, sel_n + g.first, sel_pm + g.first, s);
        }
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(n_out, sel_n, (size_t)n_clips * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(speed_pm_out, sel_pm, (size_t)n_clips * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out, e->sp_sel.p, (size_t)n_clips * max_out * sizeof(aid_exact_row), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    e->last_stream = s;
    return AID_OK;
}

int lane_speeds_entry(const char *fn, aid_engine *e, const void *pcm, PcmFmt fmt, const int64_t *offsets,
                      int32_t n_clips, int32_t loc, int32_t channels, int32_t sr_in, const int32_t *speeds_pm,
                      int32_t n_speeds, int32_t max_out, aid_exact_row *out, int32_t *n_out, int32_t *speed_pm_out,
                      void *stream) {
    if (loc != AID_PCM_HOST && loc != AID_PCM_DEVICE) return fail(AID_ERR_INVALID, std::string(fn) + ": bad pcm_location");
    if (int rc = check_speed_args(fn, e, pcm, fmt, offsets, n_clips, channels, speeds_pm, loc)) return rc;
    if (max_out <= 0 || (n_clips > 0 && (!out || !n_out || !speed_pm_out)))
        return fail(AID_ERR_INVALID, std::string(fn) + ": bad argument");
    if (e->cfg.max_results > 256) return fail(AID_ERR_INVALID, std::string(fn) + ": engine max_results must be <= 256");
    std::lock_guard<std::mutex> lk(e->mu);
    if (n_clips == 0) {  // nothing to run, but the speeds are still checked
        const int st = plan_speeds(e->sp_plan, offsets, 0, sr_in, e->cfg.sample_rate, speeds_pm, n_speeds, 0);
        return st ? speed_fail(fn, st) : AID_OK;
    }
    return drain_host_copy(e, loc, stream,
                           lane_speeds_locked(fn, e, pcm, fmt, offsets, n_clips, loc, channels, sr_in, speeds_pm,
                                              n_speeds, max_out, out, n_out, speed_pm_out, stream));
}

}  // namespace

extern "C" {

int aid_speed_plan(int32_t sr_in, int32_t sr_out, int32_t speed_pm, int32_t *up, int32_t *down, int32_t *hl, int32_t *J) {
    ResamplePlan p;
    if (speed_variant(sr_in, sr_out, speed_pm, p) != kSpeedOk) return 0;
    if (up) *up = p.up;
    if (down) *down = p.down;
    if (hl) *hl = p.hl;
    if (J) *J = p.J;
    return 1;
}

int64_t aid_speed_len(int64_t n, int32_t sr_in, int32_t sr_out, int32_t speed_pm) {
    ResamplePlan p;
    if (n <= 0 || n > ((int64_t)1 << 31) || speed_variant(sr_in, sr_out, speed_pm, p) != kSpeedOk) return 0;
    return speed_len(n, p);
}

int aid_resample_speeds(aid_engine *e, const float *src, const int64_t *offsets, int32_t n_clips, int32_t channels,
                        int32_t sr_in, const int32_t *speeds_pm, int32_t n_speeds, float *dst, int64_t cap,
                        int64_t *dst_offsets, void *stream) {
    return resample_speeds_entry("aid_resample_speeds", e, src, kF32, offsets, n_clips, channels, sr_in, speeds_pm,
                                 n_speeds, dst, cap, dst_offsets, stream);
}

int aid_resample_s16_speeds(aid_engine *e, const int16_t *src, const int64_t *offsets, int32_t n_clips, int32_t channels,
                            int32_t sr_in, const int32_t *speeds_pm, int32_t n_speeds, float *dst, int64_t cap,
                            int64_t *dst_offsets, void *stream) {
    return resample_speeds_entry("aid_resample_s16_speeds", e, src, kS16, offsets, n_clips, channels, sr_in, speeds_pm,
                                 n_speeds, dst, cap, dst_offsets, stream);
}

int aid_exact_lane_speeds(aid_engine *e, const float *pcm, const int64_t *offsets, int32_t n_clips, int32_t loc,
                          int32_t channels, int32_t sr_in, const int32_t *speeds_pm, int32_t n_speeds, int32_t max_out,
                          aid_exact_row *out, int32_t *n_out, int32_t *speed_pm_out, void *stream) {
    return lane_speeds_entry("aid_exact_lane_speeds", e, pcm, kF32, offsets, n_clips, loc, channels, sr_in, speeds_pm,
                             n_speeds, max_out, out, n_out, speed_pm_out, stream);
}

int aid_exact_lane_s16_speeds(aid_engine *e, const int16_t *pcm, const int64_t *offsets, int32_t n_clips, int32_t loc,
                              int32_t channels, int32_t sr_in, const int32_t *speeds_pm, int32_t n_speeds,
                              int32_t max_out, aid_exact_row *out, int32_t *n_out, int32_t *speed_pm_out, void *stream) {
    return lane_speeds_entry("aid_exact_lane_s16_speeds", e, pcm, kS16, offsets, n_clips, loc, channels, sr_in,
                             speeds_pm, n_speeds, max_out, out, n_out, speed_pm_out, stream);
}

}  // extern "C"
