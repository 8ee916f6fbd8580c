// aidfp_mel_plan.h -- the host-only half of the CLAP log-mel front end (spec/FPSPEC.md 10): the chunk plan of a list
// of clip lengths in either mode, K10's workgroup grid, the two shipped filter banks built in binary64, the per-band
// supports and K of a filter table, and the output capacity in int64. No HIP in here: tests/test_mel_plan_host.py
// compiles it with g++ (plain and sanitized) into a stand-alone program, the engine (mel.cpp) calls the same code.
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

namespace aid {

constexpr int kMelRate = 48000;
constexpr int kMelN = 1024;            // frame length
constexpr int kMelHop = 480;           // frame hop
constexpr int kMelWindow = 480000;     // L: samples of one chunk (10 s)
constexpr int kMelChunkHop = 240000;   // chunk hop (5 s)
constexpr int kMelMinChunk = 48000;    // ingest: the plan stops at the first chunk shorter than this (1 s)
constexpr int kMelFrames = 1001;       // T = 1 + L / hop (centred frames)
constexpr int kMelBands = 64;
constexpr int kMelBins = 513;          // rows of a filter table
constexpr int kMelMaxK = 512;          // the Nyquist bin is never computed: a table that weights it is rejected
#ifndef AID_MEL_RUN  // diagnostic builds (build_ext.build(variant=..., defines=...)) try other run lengths
#define AID_MEL_RUN 4
#endif
constexpr int kMelRun = AID_MEL_RUN;   // R: frames of one K10 workgroup
constexpr int kMelRuns = (kMelFrames + kMelRun - 1) / kMelRun;  // workgroups per chunk (the last run is short)
constexpr int kMelStage = (kMelRun - 1) * kMelHop + kMelN;      // samples a workgroup stages

enum MelMode : int { kMelZero = 0, kMelRepeatPad = 1 };
enum MelBank : int { kMelSlaney = 0, kMelHtk = 1, kMelCustom = 2 };
enum MelStatus : int {
    kMelOk = 0,
    kMelBadMode,     // mode is neither zero nor repeatpad
    kMelBadLength,   // a negative clip length
    kMelBadStart,    // repeatpad: start < 0 or start + L past the end of a clip longer than L
    kMelTooMany,     // more chunks than an int32 counts
    kMelEmptyBand,   // a band without a non-zero weight (or a negative / non-finite weight table entry)
    kMelGapBand,     // a band whose non-zero weights are not contiguous
    kMelNyquist,     // a band that weights bin 512
    kMelBadRange,    // fmin / fmax outside 0 <= fmin < fmax <= 24000
};

inline const char *mel_status_text(int st) {
    switch (st) {
        case kMelOk: return "ok";
        case kMelBadMode: return "mode must be 0 (zero fill) or 1 (repeatpad)";
        case kMelBadLength: return "clip lengths must be >= 0";
        case kMelBadStart: return "start must lie in [0, n - 480000] for every clip longer than 480000 samples";
        case kMelTooMany: return "too many chunks";
        case kMelEmptyBand: return "filter table has a band without a positive finite weight";
        case kMelGapBand: return "filter table has a band whose non-zero weights are not contiguous";
        case kMelNyquist: return "filter table weights the Nyquist bin";
        case kMelBadRange: return "need 0 <= fmin < fmax <= 24000";
    }
    return "unknown";
}

// one chunk: clip `clip`, chunk_index-th of it, real samples x[start .. start + r) of the clip; fill = the samples
// of v[0..L) that come from the clip (r in zero mode, rep * r in repeatpad), the rest is zero
struct MelChunk {
    int32_t clip, chunk_index;
    int64_t start;
    int32_t r, rep;
    double offset_sec, duration_sec;  // start / 48000, r / 48000 (binary64, as the reference's tuples)
    int64_t fill() const { return (int64_t)rep * r; }
};

// The chunk plan. zero mode: chunk_audio's loop per clip. repeatpad: one chunk per non-empty clip; a clip longer
// than L is cropped to [start, start + L)
inline int mel_plan(const int64_t *lengths, int32_t n_clips, int mode, int64_t start, std::vector<MelChunk> &out) {
    out.clear();
    if (mode != kMelZero && mode != kMelRepeatPad) return kMelBadMode;
    for (int32_t c = 0; c < n_clips; ++c) {
        const int64_t n = lengths[c];
        if (n < 0) return kMelBadLength;
        if (mode == kMelZero) {
            int32_t idx = 0;
            for (int64_t s = 0; s < n; s += kMelChunkHop, ++idx) {
                const int64_t r = n - s < kMelWindow ? n - s : kMelWindow;
                if (r < kMelMinChunk) break;
                if (out.size() >= (size_t)INT32_MAX) return kMelTooMany;
                out.push_back(MelChunk{c, idx, s, (int32_t)r, 1, (double)s / kMelRate, (double)r / kMelRate});
            }
        } else if (n > 0) {
            if (out.size() >= (size_t)INT32_MAX) return kMelTooMany;
            if (n > kMelWindow) {
                if (start < 0 || start > n - kMelWindow) return kMelBadStart;
                out.push_back(MelChunk{c, 0, start, kMelWindow, 1, (double)start / kMelRate, (double)kMelWindow / kMelRate});
            } else {
                out.push_back(MelChunk{c, 0, 0, (int32_t)n, (int32_t)(kMelWindow / n), 0.0, (double)n / kMelRate});
            }
        }
    }
    return kMelOk;
}

// K10's grid and the output it fills, in int64: floats of `chunks` chunks, and whether a capacity in chunks holds them
inline int64_t mel_grid(int64_t chunks) { return chunks * kMelRuns; }
inline int64_t mel_out_floats(int64_t chunks) { return chunks * kMelFrames * kMelBands; }
inline bool mel_fits(int64_t chunks, int64_t cap_chunks) { return chunks >= 0 && chunks <= cap_chunks; }

// ---- filter banks (binary64, rounded once to binary32) ----
inline double mel_hz_to_mel(double f, bool slaney) {
    if (!slaney) return 2595.0 * std::log10(1.0 + f / 700.0);
    if (f >= 1000.0) return 15.0 + std::log(f / 1000.0) * (27.0 / std::log(6.4));
    return 3.0 * f / 200.0;
}
inline double mel_mel_to_hz(double m, bool slaney) {
    if (!slaney) return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0);
    if (m >= 15.0) return 1000.0 * std::exp((std::log(6.4) / 27.0) * (m - 15.0));
    return 200.0 * m / 3.0;
}

// W[k][m], k < 513, m < 64: triangles over 66 points equally spaced on the mel scale between fmin and fmax;
// slaney bank: slaney scale, each band scaled by 2 / (f[m+2] - f[m]); htk bank: htk scale, no scaling
inline int mel_build_bank(int bank, double fmin, double fmax, std::vector<float> &W) {
    if (!(fmin >= 0.0) || !(fmax > fmin) || !(fmax <= kMelRate / 2.0)) return kMelBadRange;
    const bool slaney = bank == kMelSlaney;
    const double m0 = mel_hz_to_mel(fmin, slaney), m1 = mel_hz_to_mel(fmax, slaney);
    const int np = kMelBands + 2;
    double ff[kMelBands + 2];
    const double step = (m1 - m0) / (np - 1);
    for (int i = 0; i < np; ++i) ff[i] = mel_mel_to_hz(i == np - 1 ? m1 : (double)i * step + m0, slaney);
    W.assign((size_t)kMelBins * kMelBands, 0.f);
    for (int k = 0; k < kMelBins; ++k) {
        const double fk = (double)k * ((kMelRate / 2.0) / (kMelBins - 1));
        for (int m = 0; m < kMelBands; ++m) {
            const double down = -(ff[m] - fk) / (ff[m + 1] - ff[m]);
            const double up = (ff[m + 2] - fk) / (ff[m + 2] - ff[m + 1]);
            double w = down < up ? down : up;
            if (!(w > 0.0)) w = 0.0;
            if (slaney) w *= 2.0 / (ff[m + 2] - ff[m]);
            W[(size_t)k * kMelBands + m] = (float)w;
        }
    }
    return kMelOk;
}

// per band the support [lo, hi) of its non-zero weights, and K = 1 + the highest bin any band weights
struct MelSupport {
    int32_t lo[kMelBands], hi[kMelBands];
    int32_t K = 0, max_len = 0;
};
inline int mel_supports(const float *W, MelSupport &s) {
    s.K = s.max_len = 0;
    for (int m = 0; m < kMelBands; ++m) {
        int lo = -1, hi = -1, nz = 0;
        for (int k = 0; k < kMelBins; ++k) {
            const float w = W[(size_t)k * kMelBands + m];
            if (!(w >= 0.f) || !std::isfinite(w)) return kMelEmptyBand;
            if (w != 0.f) {
                if (lo < 0) lo = k;
                hi = k + 1;
                ++nz;
            }
        }
        if (nz == 0) return kMelEmptyBand;
        if (nz != hi - lo) return kMelGapBand;
        if (hi > kMelMaxK) return kMelNyquist;
        s.lo[m] = lo;
        s.hi[m] = hi;
        if (hi > s.K) s.K = hi;
        if (hi - lo > s.max_len) s.max_len = hi - lo;
    }
    return kMelOk;
}

}  // namespace aid
