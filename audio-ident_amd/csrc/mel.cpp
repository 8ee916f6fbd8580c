// mel.cpp -- the CLAP log-mel front end (FPSPEC 10): aid_mel_configure / aid_mel_filters (the filter bank and K10's
// tables), aid_mel_plan (host only) and aid_logmel (K10 over every chunk of a batch of clips). The plan and the banks
// are aidfp_mel_plan.h's; the kernel is mel.hip's.
#include <cmath>
#include <cstring>

#include "engine_internal.h"

namespace {

static_assert(AID_MEL_FRAMES == kMelFrames && AID_MEL_BANDS == kMelBands && AID_MEL_BINS == kMelBins &&
                  AID_MEL_WINDOW == kMelWindow && AID_MEL_ZERO == kMelZero && AID_MEL_REPEATPAD == kMelRepeatPad &&
                  AID_MEL_BANK_SLANEY == kMelSlaney && AID_MEL_BANK_HTK == kMelHtk && AID_MEL_BANK_CUSTOM == kMelCustom,
              "include/aidfp.h and aidfp_mel_plan.h disagree");

int mel_fail(const char *fn, int st) { return fail(AID_ERR_INVALID, std::string(fn) + ": " + mel_status_text(st)); }

float2 twiddle(int j, int n) {
    const double a = 2.0 * M_PI * (double)j / (double)n;
    return make_float2((float)std::cos(a), (float)(-std::sin(a)));
}

void fill_tables(MelTables &t, const MelSupport &s) {
    for (int m = 0; m < 512; ++m) {
        const double w0 = 0.5 - 0.5 * std::cos(2.0 * M_PI * (double)(2 * m) / 1024.0);
        const double w1 = 0.5 - 0.5 * std::cos(2.0 * M_PI * (double)(2 * m + 1) / 1024.0);
        t.win2[m] = make_float2((float)w0, (float)w1);
        t.t512[m] = twiddle(m, 512);
        t.t1k[m] = twiddle(m, 1024);
    }
    for (int j = 0; j < 8; ++j) t.t8[j] = twiddle(j, 8);
    for (int j = 0; j < 64; ++j) t.t64[j] = twiddle(j, 64);
    for (int m = 0; m < kMelBands; ++m) {
        t.lo[m] = s.lo[m];
        t.len[m] = s.hi[m] - s.lo[m];
    }
    t.K = s.K;
    t.max_len = s.max_len;
}

void to_abi(const MelChunk &c, aid_mel_chunk &o) {
    o.clip = c.clip;
    o.chunk_index = c.chunk_index;
    o.start = c.start;
    o.r = c.r;
    o.rep = c.rep;
    o.offset_sec = c.offset_sec;
    o.duration_sec = c.duration_sec;
}

int logmel_locked(const char *fn, aid_engine *e, const void *pcm, PcmFmt fmt, const int64_t *clip_off,
                  const int64_t *clip_len, int32_t n_clips, int32_t loc, int32_t mode, int64_t start, float *out,
                  int64_t cap, int32_t out_loc, aid_mel_chunk *meta, int64_t *n_chunks, hipStream_t s) {
    const std::string f(fn);
    MelState &ms = e->mel;
    if (!ms.ready) return fail(AID_ERR_STATE, f + ": aid_mel_configure first");
    for (int c = 0; c < n_clips; ++c)
        if (clip_off[c] < 0 || clip_len[c] < 0 || clip_off[c] > INT64_MAX - clip_len[c])
            return fail(AID_ERR_INVALID, f + ": clip offsets and lengths must be >= 0");
    if (int st = mel_plan(clip_len, n_clips, mode, start, ms.plan)) return mel_fail(fn, st);
    const int64_t n = (int64_t)ms.plan.size();
    *n_chunks = n;
    if (!mel_fits(n, cap)) return fail(AID_ERR_INVALID, f + ": output capacity too small");
    for (int64_t i = 0; meta && i < n; ++i) to_abi(ms.plan[i], meta[i]);
    if (n == 0) return AID_OK;
    if (!pcm || !out) return fail(AID_ERR_INVALID, f + ": null buffer");
    if (loc == AID_PCM_DEVICE && (reinterpret_cast<uintptr_t>(pcm) & (pcm_size(fmt) - 1)))
        return fail(AID_ERR_INVALID, f + ": pcm must be aligned to one sample");
    if (out_loc == AID_PCM_DEVICE && (reinterpret_cast<uintptr_t>(out) & 3u))
        return fail(AID_ERR_INVALID, f + ": out must be aligned to one float");

    HIP_TRY(ms.ev.wait());  // the last launch still reads the chunk table and the staging
    // host PCM: one copy of the span the chunks' clips cover; chunk sources then count from the span's first sample
    int64_t lo = INT64_MAX, hi = 0;
    for (const MelChunk &c : ms.plan) {
        lo = std::min(lo, clip_off[c.clip]);
        hi = std::max(hi, clip_off[c.clip] + clip_len[c.clip]);
    }
    const void *src = pcm;
    int64_t base = 0;
    if (loc == AID_PCM_HOST) {
        const size_t nbytes = (size_t)(hi - lo) * pcm_size(fmt);
        HIP_TRY(ms.d_in.reserve((nbytes + sizeof(float) - 1) / sizeof(float)));
        HIP_TRY(hipMemcpyAsync(ms.d_in.p, pcm_at(pcm, fmt, lo), nbytes, hipMemcpyHostToDevice, s));
        src = ms.d_in.p;
        base = lo;
    }
    HIP_TRY(ms.h_chunks.reserve((size_t)n));
    HIP_TRY(ms.d_chunks.reserve((size_t)n));
    for (int64_t i = 0; i < n; ++i) {
        const MelChunk &c = ms.plan[i];
        ms.h_chunks.p[i] = MelChunkDev{clip_off[c.clip] - base + c.start, c.r, (int32_t)c.fill()};
    }
    HIP_TRY(hipMemcpyAsync(ms.d_chunks.p, ms.h_chunks.p, (size_t)n * sizeof(MelChunkDev), hipMemcpyHostToDevice, s));
    float *dst = out;
    if (out_loc == AID_PCM_HOST) {
        HIP_TRY(ms.d_out.reserve((size_t)mel_out_floats(n)));
        dst = ms.d_out.p;
    }
    // a launch's grid stays far below 2^31 workgroups: slices of 2^18 chunks
    constexpr int64_t kSlice = (int64_t)1 << 18;
    for (int64_t c0 = 0; c0 < n; c0 += kSlice) {
        launch_logmel(src, fmt == kS16, ms.d_chunks.p, c0, std::min(kSlice, n - c0), ms.d_tab.p, ms.d_wc.p,
                      dst + mel_out_floats(c0), s);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(ms.ev.record(s));
    if (out_loc == AID_PCM_HOST) {
        HIP_TRY(hipMemcpyAsync(out, dst, (size_t)mel_out_floats(n) * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return AID_OK;
}

int logmel_entry(const char *fn, aid_engine *e, const void *pcm, PcmFmt fmt, const int64_t *clip_off,
                 const int64_t *clip_len, int32_t n_clips, int32_t loc, int32_t mode, int64_t start, float *out,
                 int64_t cap, int32_t out_loc, aid_mel_chunk *meta, int64_t *n_chunks, void *stream) {
    const std::string f(fn);
    if (!e || n_clips < 0 || !n_chunks || cap < 0 || (n_clips > 0 && (!clip_off || !clip_len)))
        return fail(AID_ERR_INVALID, f + ": bad argument");
    if ((loc != AID_PCM_HOST && loc != AID_PCM_DEVICE) || (out_loc != AID_PCM_HOST && out_loc != AID_PCM_DEVICE))
        return fail(AID_ERR_INVALID, f + ": bad location");
    EngineCall call(e, stream);
    if (call.rc) return call.rc;
    return drain_host_copy(e, loc, stream,
                           logmel_locked(fn, e, pcm, fmt, clip_off, clip_len, n_clips, loc, mode, start, out, cap,
                                         out_loc, meta, n_chunks, call.s));
}

}  // namespace

extern "C" {

int aid_mel_configure(aid_engine *e, int32_t bank, double fmin, double fmax, const float *filters) {
    if (bank != kMelSlaney && bank != kMelHtk && bank != kMelCustom)
        return fail(AID_ERR_INVALID, "aid_mel_configure: bad bank");
    if ((bank == kMelCustom) != (filters != nullptr))
        return fail(AID_ERR_INVALID, "aid_mel_configure: filters go with AID_MEL_BANK_CUSTOM and only with it");
    EngineCall call(e);
    if (call.rc) return call.rc;
    std::vector<float> W;
    if (bank == kMelCustom)
        W.assign(filters, filters + (size_t)kMelBins * kMelBands);
    else if (int st = mel_build_bank(bank, fmin, fmax, W))
        return mel_fail("aid_mel_configure", st);
    MelSupport sup;
    if (int st = mel_supports(W.data(), sup)) return mel_fail("aid_mel_configure", st);
    MelState &ms = e->mel;
    HIP_TRY(ms.ev.wait());
    ms.ready = false;
    std::vector<MelTables> tab(1);
    fill_tables(tab[0], sup);
    std::vector<float> wc((size_t)sup.max_len * kMelBands, 0.f);
    for (int m = 0; m < kMelBands; ++m)
        for (int j = 0; j < sup.hi[m] - sup.lo[m]; ++j)
            wc[(size_t)j * kMelBands + m] = W[(size_t)(sup.lo[m] + j) * kMelBands + m];
    HIP_TRY(ms.d_tab.reserve(1));
    HIP_TRY(ms.d_wc.reserve(wc.size()));
    HIP_TRY(hipMemcpy(ms.d_tab.p, tab.data(), sizeof(MelTables), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ms.d_wc.p, wc.data(), wc.size() * sizeof(float), hipMemcpyHostToDevice));
    ms.W = std::move(W);
    ms.sup = sup;
    ms.bank = bank;
    ms.ready = true;
    return AID_OK;
}

int aid_mel_filters(aid_engine *e, float *out) {
    if (!out) return fail(AID_ERR_INVALID, "aid_mel_filters: bad argument");
    EngineCall call(e);
    if (call.rc) return call.rc;
    if (!e->mel.ready) return fail(AID_ERR_STATE, "aid_mel_filters: aid_mel_configure first");
    std::memcpy(out, e->mel.W.data(), e->mel.W.size() * sizeof(float));
    return AID_OK;
}

int aid_mel_plan(const int64_t *lengths, int32_t n_clips, int32_t mode, int64_t start, int64_t *n_chunks,
                 aid_mel_chunk *meta_out, int64_t meta_cap) {
    if (n_clips < 0 || !n_chunks || (n_clips > 0 && !lengths) || meta_cap < 0)
        return fail(AID_ERR_INVALID, "aid_mel_plan: bad argument");
    std::vector<MelChunk> plan;
    if (int st = mel_plan(lengths, n_clips, mode, start, plan)) return mel_fail("aid_mel_plan", st);
    *n_chunks = (int64_t)plan.size();
    for (int64_t i = 0; meta_out && i < std::min<int64_t>(*n_chunks, meta_cap); ++i) to_abi(plan[i], meta_out[i]);
    return AID_OK;
}

int aid_logmel(aid_engine *e, const float *pcm, const int64_t *clip_off, const int64_t *clip_len, int32_t n_clips,
               int32_t location, int32_t mode, int64_t start, float *out, int64_t out_cap_chunks, int32_t out_location,
               aid_mel_chunk *meta, int64_t *n_chunks, void *stream) {
    return logmel_entry("aid_logmel", e, pcm, kF32, clip_off, clip_len, n_clips, location, mode, start, out,
                        out_cap_chunks, out_location, meta, n_chunks, stream);
}

int aid_logmel_pcm16(aid_engine *e, const int16_t *pcm, const int64_t *clip_off, const int64_t *clip_len,
                        int32_t n_clips, int32_t location, int32_t mode, int64_t start, float *out,
                        int64_t out_cap_chunks, int32_t out_location, aid_mel_chunk *meta, int64_t *n_chunks,
                        void *stream) {
    return logmel_entry("aid_logmel_pcm16", e, pcm, kS16, clip_off, clip_len, n_clips, location, mode, start, out,
                        out_cap_chunks, out_location, meta, n_chunks, stream);
}

}  // extern "C"
