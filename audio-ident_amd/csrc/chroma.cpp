// chroma.cpp -- the content fingerprint (FPSPEC 11): aid_chroma_len / aid_chroma_plan (host only), aid_chroma
// (K11a + K11b over a batch of clips), aid_chroma_rows (K11a alone) and aid_chroma_words (K11b on the caller's
// rows). The plan and the tables' contents are aidfp_chroma_plan.h's; the kernels are chroma.hip's.
#include <cmath>
#include <cstring>

#include "engine_internal.h"

namespace {

static_assert(AID_CHROMA_RATE == kChromaRate && AID_CHROMA_BANDS == kChromaBands && AID_CHROMA_RUN == kChromaRun,
              "include/aidfp.h and aidfp_chroma_plan.h disagree");

int chroma_fail(const char *fn, int st) { return fail(AID_ERR_INVALID, std::string(fn) + ": " + chroma_status_text(st)); }

float2 twiddle(int j, int n) {
    const double a = 2.0 * M_PI * (double)j / (double)n;
    return make_float2((float)std::cos(a), (float)(-std::sin(a)));
}

// the device tables, built on first use
int chroma_tables(aid_engine *e) {
    ChromaState &cs = e->chroma;
    if (cs.ready) return AID_OK;
    std::vector<ChromaTables> tab(1);
    ChromaTables &t = tab[0];
    std::memset(&t, 0, sizeof(t));
    auto win = [](int j) { return (float)(0.54 - 0.46 * std::cos(2.0 * M_PI * (double)j / 4095.0)); };
    for (int m = 0; m < kChromaN / 2; ++m) t.win2[m] = make_float2(win(2 * m), win(2 * m + 1));
    for (int j = 0; j < 8; ++j) t.t8[j] = twiddle(j, 8);
    for (int j = 0; j < 16; ++j) t.t16[j] = twiddle(j, 16);
    for (int j = 0; j < 128; ++j) t.t128[j] = twiddle(j, 128);
    for (int j = 0; j < 2048; ++j) {
        t.t2048[j] = twiddle(j, 2048);
        t.t4096[j] = twiddle(j, 4096);
    }
    const std::vector<ChromaBinRun> runs = chroma_runs();
    if (runs.size() > (size_t)kChromaMaxRuns) return fail(AID_ERR_STATE, "chroma: note table has too many runs");
    t.n_runs = (int32_t)runs.size();
    for (size_t r = 0; r < runs.size(); ++r) {
        t.run_lo[r] = runs[r].lo;
        t.run_len[r] = runs[r].len;
        t.run_note[r] = runs[r].note;
    }
    for (int j = 0; j < kChromaClassifiers; ++j) t.cls[j] = chroma_classifier(j);
    HIP_TRY(cs.d_tab.reserve(1));
    HIP_TRY(hipMemcpy(cs.d_tab.p, tab.data(), sizeof(ChromaTables), hipMemcpyHostToDevice));
    cs.ready = true;
    return AID_OK;
}

// a launch's grid stays far below 2^31 workgroups
constexpr int64_t kSlice = (int64_t)1 << 20;

// K11a over the batch: cs.frame_off / cs.word_off filled, C of every frame left in cs.d_rows. Engine lock held
int rows_locked(const char *fn, aid_engine *e, const void *pcm, PcmFmt fmt, const int64_t *clip_off, int32_t n_clips,
                int32_t loc, hipStream_t s) {
    const std::string f(fn);
    ChromaState &cs = e->chroma;
    if (int rc = chroma_tables(e)) return rc;
    const int64_t T = cs.frame_off[n_clips];
    if (T == 0) return AID_OK;
    if (loc == AID_PCM_DEVICE && (reinterpret_cast<uintptr_t>(pcm) & (pcm_size(fmt) - 1)))
        return fail(AID_ERR_INVALID, f + ": pcm must be aligned to one sample");
    HIP_TRY(cs.ev.wait());  // the last launch still reads the block lists and the staging
    const void *src = pcm;
    int64_t base = 0;
    if (loc == AID_PCM_HOST) {  // one copy of the span the clips cover; block sources then count from its first sample
        base = clip_off[0];
        const size_t nbytes = (size_t)(clip_off[n_clips] - base) * pcm_size(fmt);
        HIP_TRY(cs.d_in.reserve((nbytes + sizeof(float) - 1) / sizeof(float)));
        HIP_TRY(hipMemcpyAsync(cs.d_in.p, pcm_at(pcm, fmt, base), nbytes, hipMemcpyHostToDevice, s));
        src = cs.d_in.p;
    }
    chroma_row_blocks(clip_off, cs.frame_off.data(), n_clips, base, cs.row_blocks);
    const int64_t nb = (int64_t)cs.row_blocks.size();
    HIP_TRY(cs.h_rb.reserve((size_t)nb));
    HIP_TRY(cs.d_rb.reserve((size_t)nb));
    std::memcpy(cs.h_rb.p, cs.row_blocks.data(), (size_t)nb * sizeof(ChromaRowBlock));
    HIP_TRY(hipMemcpyAsync(cs.d_rb.p, cs.h_rb.p, (size_t)nb * sizeof(ChromaRowBlock), hipMemcpyHostToDevice, s));
    HIP_TRY(cs.d_rows.reserve((size_t)T * kChromaBands));
    for (int64_t b0 = 0; b0 < nb; b0 += kSlice) {
        launch_chroma_rows(src, fmt == kS16, cs.d_rb.p, b0, std::min(kSlice, nb - b0), cs.d_tab.p, cs.d_rows.p, s);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(cs.ev.record(s));
    return AID_OK;
}

// K11b over rows [row_off[c], row_off[c + 1]) of cs.d_rows per clip, words packed at word_off into `dst` (device)
int words_locked(aid_engine *e, const int64_t *row_off, const int64_t *word_off, int32_t n_clips, bool raw,
                 uint32_t *dst, hipStream_t s) {
    ChromaState &cs = e->chroma;
    chroma_item_blocks(row_off, word_off, n_clips, cs.item_blocks);
    const int64_t nb = (int64_t)cs.item_blocks.size();
    if (nb == 0) return AID_OK;
    HIP_TRY(cs.h_ib.reserve((size_t)nb));
    HIP_TRY(cs.d_ib.reserve((size_t)nb));
    std::memcpy(cs.h_ib.p, cs.item_blocks.data(), (size_t)nb * sizeof(ChromaItemBlock));
    HIP_TRY(hipMemcpyAsync(cs.d_ib.p, cs.h_ib.p, (size_t)nb * sizeof(ChromaItemBlock), hipMemcpyHostToDevice, s));
    for (int64_t b0 = 0; b0 < nb; b0 += kSlice) {
        launch_chroma_words(cs.d_rows.p, cs.d_ib.p, b0, std::min(kSlice, nb - b0), cs.d_tab.p, raw, dst, s);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(cs.ev.record(s));
    return AID_OK;
}

// the clip lengths of a batch into the engine's offsets
int plan_clips(const char *fn, aid_engine *e, const int64_t *clip_off, int32_t n_clips) {
    ChromaState &cs = e->chroma;
    std::vector<int64_t> len((size_t)n_clips);
    for (int32_t c = 0; c < n_clips; ++c) len[c] = clip_off[c + 1] - clip_off[c];
    cs.frame_off.assign((size_t)n_clips + 1, 0);
    cs.word_off.assign((size_t)n_clips + 1, 0);
    if (int st = chroma_offsets(len.data(), n_clips, cs.frame_off.data(), cs.word_off.data())) return chroma_fail(fn, st);
    return AID_OK;
}

int chroma_locked(const char *fn, aid_engine *e, const void *pcm, PcmFmt fmt, const int64_t *clip_off, int32_t n_clips,
                  int32_t loc, uint32_t *words_out, int64_t *word_off_out, int64_t cap, int32_t out_loc,
                  int64_t *n_words, hipStream_t s) {
    const std::string f(fn);
    ChromaState &cs = e->chroma;
    if (int rc = plan_clips(fn, e, clip_off, n_clips)) return rc;
    const int64_t W = cs.word_off[n_clips];
    *n_words = W;
    if (W > cap) return fail(AID_ERR_INVALID, f + ": output capacity too small");
    if (word_off_out) std::memcpy(word_off_out, cs.word_off.data(), ((size_t)n_clips + 1) * sizeof(int64_t));
    if (W == 0) return AID_OK;
    if (!words_out) return fail(AID_ERR_INVALID, f + ": null buffer");
    if (out_loc == AID_PCM_DEVICE && (reinterpret_cast<uintptr_t>(words_out) & 3u))
        return fail(AID_ERR_INVALID, f + ": words_out must be aligned to one word");
    if (int rc = rows_locked(fn, e, pcm, fmt, clip_off, n_clips, loc, s)) return rc;
    uint32_t *dst = words_out;
    if (out_loc == AID_PCM_HOST) {
        HIP_TRY(cs.d_words.reserve((size_t)W));
        dst = cs.d_words.p;
    }
    if (int rc = words_locked(e, cs.frame_off.data(), cs.word_off.data(), n_clips, false, dst, s)) return rc;
    if (out_loc == AID_PCM_HOST) {
        HIP_TRY(hipMemcpyAsync(words_out, dst, (size_t)W * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return AID_OK;
}

int chroma_entry(const char *fn, aid_engine *e, const void *pcm, PcmFmt fmt, const int64_t *clip_off, int32_t n_clips,
                 int32_t loc, uint32_t *words_out, int64_t *word_off_out, int64_t cap, int32_t out_loc,
                 int64_t *n_words, void *stream) {
    if (int rc = check_clips(fn, e, pcm, clip_off, n_clips, loc)) return rc;
    if (!n_words || cap < 0 || (out_loc != AID_PCM_HOST && out_loc != AID_PCM_DEVICE))
        return fail(AID_ERR_INVALID, std::string(fn) + ": bad argument");
    EngineCall call(e, stream);
    if (call.rc) return call.rc;
    return drain_host_copy(e, loc, stream,
                           chroma_locked(fn, e, pcm, fmt, clip_off, n_clips, loc, words_out, word_off_out, cap, out_loc,
                                         n_words, call.s));
}

int rows_entry(const char *fn, aid_engine *e, const void *pcm, PcmFmt fmt, const int64_t *clip_off, int32_t n_clips,
               int32_t loc, float *rows_out, int64_t *row_off_out, int64_t cap, int64_t *n_rows, void *stream) {
    if (int rc = check_clips(fn, e, pcm, clip_off, n_clips, loc)) return rc;
    if (!n_rows || cap < 0) return fail(AID_ERR_INVALID, std::string(fn) + ": bad argument");
    EngineCall call(e, stream);
    if (call.rc) return call.rc;
    ChromaState &cs = e->chroma;
    if (int rc = plan_clips(fn, e, clip_off, n_clips)) return rc;
    const int64_t T = cs.frame_off[n_clips];
    *n_rows = T;
    if (T > cap) return fail(AID_ERR_INVALID, std::string(fn) + ": output capacity too small");
    if (row_off_out) std::memcpy(row_off_out, cs.frame_off.data(), ((size_t)n_clips + 1) * sizeof(int64_t));
    if (T == 0) return AID_OK;
    if (!rows_out) return fail(AID_ERR_INVALID, std::string(fn) + ": null buffer");
    int rc = rows_locked(fn, e, pcm, fmt, clip_off, n_clips, loc, call.s);
    if (rc == AID_OK) {
        HIP_TRY(hipMemcpyAsync(rows_out, cs.d_rows.p, (size_t)T * kChromaBands * sizeof(float), hipMemcpyDeviceToHost, call.s));
        HIP_TRY(hipStreamSynchronize(call.s));
    }
    return drain_host_copy(e, loc, stream, rc);
}

}  // namespace

extern "C" {

int64_t aid_chroma_len(int64_t n) { return n < 0 ? 0 : chroma_words(n); }

int aid_chroma_plan(const int64_t *lengths, int32_t n_clips, int64_t *word_off_out, int64_t *n_frames, int64_t *n_words) {
    if (n_clips < 0 || (n_clips > 0 && !lengths)) return fail(AID_ERR_INVALID, "aid_chroma_plan: bad argument");
    std::vector<int64_t> fo((size_t)n_clips + 1), wo((size_t)n_clips + 1);
    if (int st = chroma_offsets(lengths, n_clips, fo.data(), wo.data())) return chroma_fail("aid_chroma_plan", st);
    if (word_off_out) std::memcpy(word_off_out, wo.data(), wo.size() * sizeof(int64_t));
    if (n_frames) *n_frames = fo[n_clips];
    if (n_words) *n_words = wo[n_clips];
    return AID_OK;
}

int aid_chroma(aid_engine *e, const float *pcm, const int64_t *clip_off, int32_t n_clips, int32_t location,
               uint32_t *words_out, int64_t *word_off_out, int64_t cap_words, int32_t out_location, int64_t *n_words,
               void *stream) {
    return chroma_entry("aid_chroma", e, pcm, kF32, clip_off, n_clips, location, words_out, word_off_out, cap_words,
                        out_location, n_words, stream);
}

int aid_chroma_pcm16(aid_engine *e, const int16_t *pcm, const int64_t *clip_off, int32_t n_clips, int32_t location,
                   uint32_t *words_out, int64_t *word_off_out, int64_t cap_words, int32_t out_location,
                   int64_t *n_words, void *stream) {
    return chroma_entry("aid_chroma_pcm16", e, pcm, kS16, clip_off, n_clips, location, words_out, word_off_out,
                        cap_words, out_location, n_words, stream);
}

int aid_chroma_rows(aid_engine *e, const float *pcm, const int64_t *clip_off, int32_t n_clips, int32_t location,
                    float *rows_out, int64_t *row_off_out, int64_t cap_rows, int64_t *n_rows, void *stream) {
    return rows_entry("aid_chroma_rows", e, pcm, kF32, clip_off, n_clips, location, rows_out, row_off_out, cap_rows,
                      n_rows, stream);
}

int aid_chroma_rows_pcm16(aid_engine *e, const int16_t *pcm, const int64_t *clip_off, int32_t n_clips, int32_t location,
                        float *rows_out, int64_t *row_off_out, int64_t cap_rows, int64_t *n_rows, void *stream) {
    return rows_entry("aid_chroma_rows_pcm16", e, pcm, kS16, clip_off, n_clips, location, rows_out, row_off_out,
                      cap_rows, n_rows, stream);
}

int aid_chroma_words(aid_engine *e, const float *rows, const int64_t *row_off, int32_t n_clips, int32_t raw_features,
                     uint32_t *words_out, int64_t *word_off_out, int64_t cap_words, int64_t *n_words) {
    if (!e || n_clips < 0 || !n_words || cap_words < 0 || (n_clips > 0 && !row_off))
        return fail(AID_ERR_INVALID, "aid_chroma_words: bad argument");
    std::vector<int64_t> wo((size_t)n_clips + 1, 0);
    for (int32_t c = 0; c < n_clips; ++c) {
        const int64_t R = row_off[c + 1] - row_off[c];
        if (R < 0 || row_off[c] < 0) return chroma_fail("aid_chroma_words", kChromaBadLength);
        wo[c + 1] = wo[c] + (raw_features ? chroma_words_of_features(R) : chroma_words_of_frames(R));
    }
    const int64_t W = wo[n_clips];
    *n_words = W;
    if (W > cap_words) return fail(AID_ERR_INVALID, "aid_chroma_words: output capacity too small");
    if (word_off_out) std::memcpy(word_off_out, wo.data(), wo.size() * sizeof(int64_t));
    if (W == 0) return AID_OK;
    if (!rows || !words_out) return fail(AID_ERR_INVALID, "aid_chroma_words: null buffer");
    EngineCall call(e);
    if (call.rc) return call.rc;
    ChromaState &cs = e->chroma;
    if (int rc = chroma_tables(e)) return rc;
    HIP_TRY(cs.ev.wait());
    const int64_t lo = row_off[0], hi = row_off[n_clips];
    std::vector<int64_t> ro((size_t)n_clips + 1);
    for (int32_t c = 0; c <= n_clips; ++c) ro[c] = row_off[c] - lo;
    HIP_TRY(cs.d_rows.reserve((size_t)(hi - lo) * kChromaBands));
    HIP_TRY(cs.d_words.reserve((size_t)W));
    HIP_TRY(hipMemcpyAsync(cs.d_rows.p, rows + lo * kChromaBands, (size_t)(hi - lo) * kChromaBands * sizeof(float),
                           hipMemcpyHostToDevice, call.s));
    int rc = words_locked(e, ro.data(), wo.data(), n_clips, raw_features != 0, cs.d_words.p, call.s);
    if (rc == AID_OK) {
        HIP_TRY(hipMemcpyAsync(words_out, cs.d_words.p, (size_t)W * sizeof(uint32_t), hipMemcpyDeviceToHost, call.s));
    }
    HIP_TRY(hipStreamSynchronize(call.s));
    return rc;
}

}  // extern "C"
