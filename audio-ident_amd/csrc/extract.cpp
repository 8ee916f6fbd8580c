// extract.cpp -- host side of extraction (K1 -> K2 -> K3): extract_locked (state: aidfp_extract.h, planning:
// aidfp_extract_plan.h), the extraction entry points and the readers of the last call's results.
#include <cstring>

#include "engine_internal.h"

// Clip c is pcm[offsets[c], offsets[c + 1]); with `ends` (device PCM only) it is pcm[offsets[c], ends[c]), so clips
// may overlap (the exact lane's sub-windows are read in place). Plan, reserve, stage, upload, launch.
int extract_locked(aid_engine *e, const void *pcm, PcmFmt fmt, const int64_t *offsets, int32_t n_clips, int32_t loc,
                   void *stream, const int64_t *ends) {
    if (ends && loc != AID_PCM_DEVICE) return fail(AID_ERR_INVALID, "extract: clip ends need device PCM");
    HIP_TRY(hipSetDevice(e->device));
    Extractor &x = e->ext;
    ExtractPlan &p = x.plan;
    hipStream_t s = pick_stream(e, stream);
    const bool keep_power = (e->cfg.flags & AID_FLAG_KEEP_POWER) != 0, rel = e->cfg.peak_rel > 0.0f;
    // a different stream than the previous call's: order against it the simple way
    if (e->last_stream && e->last_stream != s) HIP_TRY(hipStreamSynchronize(e->last_stream));
    // plan: K2's width and strips per slot from the words K3 left, then descriptors, groups and totals
    x.have_result = false;  // the plan is also the result state: none until this call has queued all of its work
    const uint64_t cw = x.h_cold.p ? *reinterpret_cast<volatile uint64_t *>(x.h_cold.p) : 0;
    const uint64_t sw = x.h_cold.p ? *reinterpret_cast<volatile uint64_t *>(x.h_cold.p + 1) : 0;
    const K2Choice k2 = x.k2.choose(cw, sw);
    plan_extract(p, offsets, ends, n_clips, loc, e->cfg.hop, x.plane_rows, keep_power,
                 x.k2_slots[k2.width == 2 ? 0 : 1], k2.slots_x, k2.width);
    // reserve
    int64_t plane = 1;
    for (const ClipGroup &g : p.groups) plane = std::max(plane, g.frames);
    HIP_TRY(x.desc.reserve((size_t)n_clips + 1));
    HIP_TRY(x.power.reserve((size_t)plane * kBins));
    HIP_TRY(x.mask.reserve((size_t)p.total_frames * kMaskWords));
    HIP_TRY(x.rowflags.reserve((size_t)p.flag_words + 4));
    HIP_TRY(x.hotw.reserve((size_t)p.total_frames + 1));
    // relative mode: the clips' maxima start at +0 on this call's stream, ahead of the first group's K1
    if (rel) {
        HIP_TRY(x.clip_qmax.reserve((size_t)n_clips + 1));
        if (n_clips > 0) HIP_TRY(hipMemsetAsync(x.clip_qmax.p, 0, sizeof(uint32_t) * (size_t)n_clips, s));
    }
    if (!x.h_cold.p) {  // the first call: K2's counters and the pinned words K3 sums them into
        HIP_TRY(x.k2_cold.reserve(128));
        HIP_TRY(hipMemsetAsync(x.k2_cold.p, 0, 128 * sizeof(uint32_t), s));
        HIP_TRY(x.h_cold.reserve(2, hipHostMallocMapped));
        x.h_cold.p[0] = x.h_cold.p[1] = 0;
        HIP_TRY(hipHostGetDevicePointer((void **)&x.h_cold_dev, x.h_cold.p, 0));
    }
    HIP_TRY(x.chunk_counts.reserve((size_t)p.chunks + 1));
    HIP_TRY(x.records.reserve((size_t)p.records + 1));
    HIP_TRY(x.counts.reserve((size_t)n_clips + 1));
    // stage host PCM: one copy of the clips' whole span (a copy per clip cost ~10-20 us of call overhead each: 64
    // coalesced service queries ~1 ms), raw bytes to both formats (s16: half the copy)
    const void *dpcm = pcm;
    if (p.staged > 0) {
        // an earlier K1 may still read it: ordered on the same stream (a pipelined submit must not wait), else wait
        if (x.stage_stream != s) HIP_TRY(x.stage_ev.wait());
        x.stage_ev.live = false;
        const size_t nbytes = (size_t)p.staged * pcm_size(fmt);
        HIP_TRY(x.pcm_stage.reserve((nbytes + sizeof(float) - 1) / sizeof(float)));
        HIP_TRY(hipMemcpyAsync(x.pcm_stage.p, pcm_at(pcm, fmt, offsets[0]), nbytes, hipMemcpyHostToDevice, s));
        dpcm = x.pcm_stage.p;
    }
    // upload, unless the device holds these very bytes. Only this branch writes h_desc: the last upload must have left it
    if (n_clips > 0 && (x.desc_dev != x.desc.p || desc_differ(p.desc.data(), (size_t)n_clips, x.h_desc.p, x.desc_n))) {
        x.desc_dev = nullptr;  // until the copy below is queued, nothing is known to be on the device
        HIP_TRY(x.desc_ev.wait());
        HIP_TRY(x.h_desc.reserve((size_t)n_clips + 1));
        std::memcpy(x.h_desc.p, p.desc.data(), sizeof(ClipDesc) * n_clips);
        HIP_TRY(hipMemcpyAsync(x.desc.p, x.h_desc.p, sizeof(ClipDesc) * n_clips, hipMemcpyHostToDevice, s));
        HIP_TRY(x.desc_ev.record(s));
        x.desc_n = (size_t)n_clips;
        x.desc_dev = x.desc.p;
    }
    if (p.empty_clip || p.total_frames == 0)
        HIP_TRY(hipMemsetAsync(x.counts.p, 0, sizeof(int64_t) * ((size_t)n_clips + 1), s));
    // launch: K1 -> K2 per clip group on one power buffer, then K3 over the call
    if (p.total_frames > 0) {
        for (const ClipGroup &g : p.groups) {
            if (g.frames == 0) continue;
            uint32_t *qmax = rel ? x.clip_qmax.p + g.first : nullptr;
            {
                ProfScope ps(e, AID_K_STFT, s, true);
                launch_stft_power(dpcm, fmt == kS16, x.desc.p + g.first, g.n, g.frame0, g.frames, g.k1_strips,
                                  x.k1_waves > 0 ? x.k1_waves : x.k1_slots, e->cfg.hop, e->d_tab.p, x.power.p, false,
                                  x.hotw.p, e->cfg.peak_threshold, keep_power, qmax, s);
            }
            if (loc == AID_PCM_HOST && &g == &p.groups.back()) {
                HIP_TRY(x.stage_ev.record(s));
                x.stage_stream = s;
            }
            {
                ProfScope ps(e, AID_K_PEAKS, s, true);
                launch_peak_pick(p.width, x.power.p, x.desc.p + g.first, g.n, g.frame0, g.strips, g.strip_len,
                                 e->cfg.peak_threshold, x.hotw.p, x.mask.p, x.k2_cold.p, qmax, e->cfg.peak_rel,
                                 x.rowflags.p, s);
            }
        }
        if (p.multi_chunk) {  // some clip spans several K3 chunks: their bases need the COUNT pass
            ProfScope ps(e, AID_K_LANDMARK_COUNT, s, true);
            launch_landmarks(x.mask.p, x.rowflags.p, x.desc.p, n_clips, p.chunks, x.chunk_counts.p, x.records.p,
                             x.counts.p, false, nullptr, nullptr, 0u, 0u, p.one_chunk_each, s);
        }
        {
            ProfScope ps(e, AID_K_LANDMARK_WRITE, s, true);
            launch_landmarks(x.mask.p, x.rowflags.p, x.desc.p, n_clips, p.chunks, x.chunk_counts.p, x.records.p,
                             x.counts.p, true, x.h_cold_dev ? x.k2_cold.p : nullptr, x.h_cold_dev,
                             (uint32_t)(p.width * p.strips), (uint32_t)p.strips, p.one_chunk_each, s);
        }
    }
    HIP_TRY(hipGetLastError());
    e->last_stream = s;
    x.have_result = true;
    return AID_OK;
}

// the checks the result readers share (clip: null for a reader of every clip), then on request the wait for the call
static int result_ready(aid_engine *e, const int32_t *clip, bool wait = true) {
    if (!e) return fail(AID_ERR_INVALID, "null engine");
    if (!e->ext.have_result) return fail(AID_ERR_STATE, "no extraction yet");
    if (clip && (*clip < 0 || *clip >= e->ext.plan.n_clips)) return fail(AID_ERR_INVALID, "clip index out of range");
    return wait ? aid_sync(e) : AID_OK;
}

template <typename T>  // rows [frame_base, + frames) of a clip in a plane of `per` elements a row
static int read_rows(aid_engine *e, int32_t clip, const T *plane, int per, T *out, int64_t cap) {
    const ClipDesc &d = e->ext.plan.desc[clip];
    if (d.frames * per > cap) return fail(AID_ERR_INVALID, "output capacity too small");
    if (d.frames > 0)
        HIP_TRY(hipMemcpy(out, plane + d.frame_base * per, d.frames * per * sizeof(T), hipMemcpyDeviceToHost));
    return AID_OK;
}

extern "C" {

int64_t aid_num_frames(const aid_engine *e, int64_t n) { return e ? num_frames(n, e->cfg.hop) : 0; }
int64_t aid_hash_capacity(const aid_engine *e, int64_t n) { return e ? hash_capacity(num_frames(n, e->cfg.hop)) : 0; }

static int extract_entry(const char *fn, aid_engine *e, const void *pcm, PcmFmt fmt, const int64_t *offsets,
                         int32_t n_clips, int32_t loc, void *stream) {
    if (int rc = check_clips(fn, e, pcm, offsets, n_clips, loc)) return rc;
    std::lock_guard<std::mutex> lk(e->mu);
    return drain_host_copy(e, loc, stream, extract_locked(e, pcm, fmt, offsets, n_clips, loc, stream));
}

int aid_extract(aid_engine *e, const float *pcm, const int64_t *offsets, int32_t n_clips, int32_t loc, void *stream) {
    return extract_entry("aid_extract", e, pcm, kF32, offsets, n_clips, loc, stream);
}

int aid_extract_s16(aid_engine *e, const int16_t *pcm, const int64_t *offsets, int32_t n_clips, int32_t loc,
                    void *stream) {
    return extract_entry("aid_extract_s16", e, pcm, kS16, offsets, n_clips, loc, stream);
}

int aid_sync(aid_engine *e) {
    if (!e) return fail(AID_ERR_INVALID, "null engine");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->last_stream ? e->last_stream : e->own_stream));
    return AID_OK;
}

int aid_result_counts(aid_engine *e, int64_t *counts) {
    if (int rc = result_ready(e, nullptr)) return rc;
    const int n = e->ext.plan.n_clips;
    if (n > 0 && !counts) return fail(AID_ERR_INVALID, "null argument");
    if (n > 0) HIP_TRY(hipMemcpy(counts, e->ext.counts.p, sizeof(int64_t) * n, hipMemcpyDeviceToHost));
    return AID_OK;
}

int aid_result_hashes(aid_engine *e, int32_t clip, aid_hash *out, int64_t cap, int64_t *n_out) {
    if (!n_out) return fail(AID_ERR_INVALID, "null argument");
    if (int rc = result_ready(e, &clip)) return rc;
    int64_t n = 0;
    HIP_TRY(hipMemcpy(&n, e->ext.counts.p + clip, sizeof(int64_t), hipMemcpyDeviceToHost));
    *n_out = n;
    if (n > cap) return fail(AID_ERR_INVALID, "output capacity too small");
    if (n > 0 && !out) return fail(AID_ERR_INVALID, "null output");
    const uint64_t *src = e->ext.records.p + e->ext.plan.hash_base[clip];
    if (n > 0) HIP_TRY(hipMemcpy(out, src, n * sizeof(aid_hash), hipMemcpyDeviceToHost));
    return AID_OK;
}

int aid_result_device(aid_engine *e, const aid_hash **records, const int64_t **counts_dev,
                      const int64_t **clip_base_host, int32_t *n_clips) {
    if (int rc = result_ready(e, nullptr, false)) return rc;  // hands out pointers and does not wait
    if (records) *records = reinterpret_cast<const aid_hash *>(e->ext.records.p);
    if (counts_dev) *counts_dev = e->ext.counts.p;
    if (clip_base_host) *clip_base_host = e->ext.plan.hash_base.data();
    if (n_clips) *n_clips = e->ext.plan.n_clips;
    return AID_OK;
}

int aid_result_power(aid_engine *e, int32_t clip, float *out, int64_t cap) {
    if (int rc = result_ready(e, &clip)) return rc;
    if (!(e->cfg.flags & AID_FLAG_KEEP_POWER))
        return fail(AID_ERR_STATE, "aid_result_power: engine created without AID_FLAG_KEEP_POWER (cold blocks not stored)");
    if (int rc = read_rows(e, clip, e->ext.power.p, kBins, out, cap)) return rc;
    // K1 stores Q = fma(Xr, Xr, Xi*Xi) = 4P; FPSPEC 4's P is Q * 0.25f, the same binary32 op
    for (int64_t i = 0; i < e->ext.plan.frames[clip] * kBins; ++i) out[i] = out[i] * 0.25f;
    return AID_OK;
}

int aid_result_thresholds(aid_engine *e, float *out) {
    if (int rc = result_ready(e, nullptr)) return rc;
    const int n = e->ext.plan.n_clips;
    if (n > 0 && !out) return fail(AID_ERR_INVALID, "null argument");
    const float thr = e->cfg.peak_threshold, r = e->cfg.peak_rel;
    std::vector<uint32_t> q((size_t)n, 0u);  // relative mode off: +0 for every clip, so the floor below
    if (r > 0.0f && n > 0) HIP_TRY(hipMemcpy(q.data(), e->ext.clip_qmax.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    for (int c = 0; c < n; ++c) {
        // FPSPEC 5.1 in the spec's own terms: Pmax = Qmax * 0.25f (the readout scaling of aid_result_power; the
        // maximum commutes with it), one binary32 multiply by r, then the maximum with the floor
        float qm;
        std::memcpy(&qm, &q[c], sizeof(qm));
        const float t = r * (qm * 0.25f);
        out[c] = t > thr ? t : thr;
    }
    return AID_OK;
}

int aid_result_peakmask(aid_engine *e, int32_t clip, uint64_t *out, int64_t cap) {
    if (int rc = result_ready(e, &clip)) return rc;
    if (int rc = read_rows(e, clip, e->ext.mask.p, kMaskWords, out, cap)) return rc;
    // K2 stores a row's 4 words of a 256-bin quarter only when they hold a peak (aidfp_layout.h, row flags): the
    // complete mask has zeros wherever the quarter's flag is clear
    const ClipDesc &d = e->ext.plan.desc[clip];
    if (d.frames == 0) return AID_OK;
    const int64_t L = d.strip_len, per = flag_words_per_strip((int)L);
    std::vector<uint32_t> fl((size_t)(((d.frames + L - 1) / L) * per));
    HIP_TRY(hipMemcpy(fl.data(), e->ext.rowflags.p + d.flag_base, fl.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int64_t r = 0; r < d.frames; ++r) {
        const int64_t o = r % L;
        const uint32_t *unit = fl.data() + (r / L) * per + 4 * (o >> 5);
        for (int q = 0; q < 4; ++q)
            if (!((unit[q] >> (o & 31)) & 1u)) std::memset(out + r * kMaskWords + 4 * q, 0, 4 * sizeof(uint64_t));
    }
    return AID_OK;
}

int aid_spectrogram(aid_engine *e, const float *pcm, int64_t n, float *out, int64_t cap) {
    if (!e || (n > 0 && !pcm) || n < 0) return fail(AID_ERR_INVALID, "aid_spectrogram: bad argument");
    const int64_t F = num_frames(n, e->cfg.hop);
    if (F * kBins > cap) return fail(AID_ERR_INVALID, "output capacity too small");
    if (F == 0) return AID_OK;
    EngineCall call(e, nullptr, false, kDrainLast);
    if (call.rc) return call.rc;
    hipStream_t s = call.s;
    DevBuf<float> d_pcm, d_out;
    DevBuf<ClipDesc> d_desc;
    ClipDesc d{};
    d.frames = F;
    HIP_TRY(d_pcm.reserve((size_t)n));
    // from here every failure is AID_ERR_DEVICE under the function's name
    hipError_t he = d_out.reserve((size_t)(F * kBins));
    if (he == hipSuccess) he = d_desc.reserve(1);
    if (he == hipSuccess) he = hipMemcpy(d_pcm.p, pcm, n * sizeof(float), hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(d_desc.p, &d, sizeof(ClipDesc), hipMemcpyHostToDevice);
    if (he == hipSuccess)
        launch_stft_power(d_pcm.p, false, d_desc.p, 1, 0, F, (F + kStftStrip - 1) / kStftStrip, e->ext.k1_slots,
                          e->cfg.hop, e->d_tab.p, d_out.p, true, nullptr, e->cfg.peak_threshold, true, nullptr, s);
    if (he == hipSuccess) he = hipGetLastError();
    if (he == hipSuccess) he = hipStreamSynchronize(s);
    if (he == hipSuccess) he = hipMemcpy(out, d_out.p, F * kBins * sizeof(float), hipMemcpyDeviceToHost);
    return he == hipSuccess ? AID_OK : fail(AID_ERR_DEVICE, std::string("aid_spectrogram: ") + hipGetErrorString(he));
}

}  // extern "C"
