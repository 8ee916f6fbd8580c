// aidfp_chroma_plan.h -- the host-only half of the content fingerprint (spec/FPSPEC.md 11): the constants, the frame
// and word counts of a clip, the per-clip frame and word offsets of a batch in int64, K11a's and K11b's workgroup
// lists, the note table and its runs, and the 16 classifiers with their thresholds and rectangles. No HIP in here:
// tests/test_chroma_plan_host.py compiles it with g++ (plain and sanitized) into a stand-alone program, the engine
// (chroma.cpp) calls the same code and the kernels (chroma.hip) read the tables it builds.
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

namespace aid {

constexpr int kChromaRate = 11025;
constexpr int kChromaN = 4096;       // frame length
constexpr int kChromaHop = 1365;     // frame hop (odd)
constexpr int kChromaBinLo = 10;     // round(4096 * 28 / 11025)
constexpr int kChromaBinHi = 1308;   // round(4096 * 3520 / 11025): bins [10, 1308) are computed
constexpr int kChromaBins = kChromaBinHi - kChromaBinLo;  // 1298
constexpr int kChromaBands = 12;
constexpr int kChromaTaps = 5;       // smoothing: rows t .. t + 4
constexpr int kChromaItem = 16;      // rows of F one word reads
constexpr int kChromaItemRows = kChromaItem + kChromaTaps - 1;  // 20 rows of C one word reads
constexpr int kChromaClassifiers = 16;
constexpr int kChromaMaxRuns = 96;   // device table size; the table has 83
#ifndef AID_CHROMA_RUN  // diagnostic builds (build_ext.build(variant=..., defines=...)) try other run lengths
#define AID_CHROMA_RUN 4
#endif
constexpr int kChromaRun = AID_CHROMA_RUN;  // R: frames of one K11a workgroup
constexpr int kChromaStage = (kChromaRun - 1) * kChromaHop + kChromaN;  // samples a workgroup stages
constexpr int kChromaItems = 240;    // words of one K11b workgroup (it holds 240 + 19 rows of C)
constexpr uint32_t kChromaZeroWord = 0x256DF977u;  // every word of an all-zero input (627964279)

enum ChromaStatus : int {
    kChromaOk = 0,
    kChromaBadLength,  // a negative clip length (or row count)
    kChromaOverflow,   // the batch's rows do not fit an int64 byte count
};

inline const char *chroma_status_text(int st) {
    switch (st) {
        case kChromaOk: return "ok";
        case kChromaBadLength: return "clip lengths must be >= 0";
        case kChromaOverflow: return "too many frames";
    }
    return "unknown";
}

// frames T and words Wn of a clip of n samples at 11025 Hz
inline int64_t chroma_frames(int64_t n) { return n >= kChromaN ? 1 + (n - kChromaN) / kChromaHop : 0; }
inline int64_t chroma_words_of_frames(int64_t T) { return T > kChromaItemRows - 1 ? T - (kChromaItemRows - 1) : 0; }
inline int64_t chroma_words(int64_t n) { return chroma_words_of_frames(chroma_frames(n)); }
// words of `rows` rows of F handed in directly (aid_chroma_words with raw_features)
inline int64_t chroma_words_of_features(int64_t rows) { return rows > kChromaItem - 1 ? rows - (kChromaItem - 1) : 0; }

// frame_off[c], word_off[c] (n_clips + 1 entries each; either may be null): where clip c's rows and words start
inline int chroma_offsets(const int64_t *lengths, int32_t n_clips, int64_t *frame_off, int64_t *word_off) {
    int64_t f = 0, w = 0;
    constexpr int64_t kMaxFrames = INT64_MAX / (kChromaBands * (int64_t)sizeof(float));
    for (int32_t c = 0; c < n_clips; ++c) {
        if (lengths[c] < 0) return kChromaBadLength;
        if (frame_off) frame_off[c] = f;
        if (word_off) word_off[c] = w;
        const int64_t T = chroma_frames(lengths[c]);
        if (T > kMaxFrames - f) return kChromaOverflow;
        f += T;
        w += chroma_words_of_frames(T);
    }
    if (frame_off) frame_off[n_clips] = f;
    if (word_off) word_off[n_clips] = w;
    return kChromaOk;
}

// one K11a workgroup: frames [row, row + nfr) of the batch, the first of which starts at sample `src` (counted from
// the call's PCM pointer); it reads samples [src, src + (nfr - 1) * 1365 + 4096), all inside its clip
struct ChromaRowBlock {
    int64_t src, row;
    int32_t nfr, pad;
};
inline int64_t chroma_row_grid(int64_t T) { return (T + kChromaRun - 1) / kChromaRun; }
inline void chroma_row_blocks(const int64_t *clip_off, const int64_t *frame_off, int32_t n_clips, int64_t base,
                              std::vector<ChromaRowBlock> &out) {
    out.clear();
    for (int32_t c = 0; c < n_clips; ++c) {
        const int64_t T = frame_off[c + 1] - frame_off[c];
        for (int64_t t = 0; t < T; t += kChromaRun)
            out.push_back(ChromaRowBlock{clip_off[c] - base + t * kChromaHop, frame_off[c] + t,
                                         (int32_t)(T - t < kChromaRun ? T - t : kChromaRun), 0});
    }
}

// one K11b workgroup: words [word, word + n) of one clip; word i of it reads rows [row + i, row + i + 20) of C
// (16 rows of F with raw features), none of them another clip's
struct ChromaItemBlock {
    int64_t row, word;
    int32_t n, pad;
};
inline void chroma_item_blocks(const int64_t *row_off, const int64_t *word_off, int32_t n_clips,
                               std::vector<ChromaItemBlock> &out) {
    out.clear();
    for (int32_t c = 0; c < n_clips; ++c) {
        const int64_t W = word_off[c + 1] - word_off[c];
        for (int64_t i = 0; i < W; i += kChromaItems)
            out.push_back(ChromaItemBlock{row_off[c] + i, word_off[c] + i, (int32_t)(W - i < kChromaItems ? W - i : kChromaItems), 0});
    }
}

// ---- notes and runs ----
inline int chroma_note(int k) {
    const double o = std::log2(((double)k * 11025.0 / 4096.0) / 27.5);
    return (int)(12.0 * (o - std::floor(o)));
}
// consecutive bins with the same note: bins [lo, lo + len)
struct ChromaBinRun {
    int32_t lo, len, note;
};
inline std::vector<ChromaBinRun> chroma_runs() {
    std::vector<ChromaBinRun> r;
    for (int k = kChromaBinLo; k < kChromaBinHi; ++k) {
        const int n = chroma_note(k);
        if (!r.empty() && r.back().note == n)
            ++r.back().len;
        else
            r.push_back(ChromaBinRun{k, 1, n});
    }
    return r;
}

// ---- classifiers ----
// a rectangle of an item's 16 x 12 image: rows [x0, x1) counted from the item's first row, bands [y0, y1)
struct ChromaRect {
    int32_t x0, x1, y0, y1;
};
// q = #{ i : 1 + a >= E[i] * (1 + b) }, a and b the sums of the areas of na and nb rectangles in their order
struct ChromaClassifier {
    int32_t type, y, h, w;
    float t[3], E[3];
    int32_t na, nb;
    ChromaRect a[2], b[2];
};
struct ChromaClassifierSpec {
    int type, y, h, w;
    float t0, t1, t2;
};
constexpr ChromaClassifierSpec kChromaSpecs[kChromaClassifiers] = {
    {0, 4, 3, 15, 1.98215f, 2.35817f, 2.63523f},        {4, 4, 6, 15, -1.03809f, -0.651211f, -0.282167f},
    {1, 0, 4, 16, -0.298702f, 0.119262f, 0.558497f},    {3, 8, 2, 12, -0.105439f, 0.0153946f, 0.135898f},
    {3, 4, 4, 8, -0.142891f, 0.0258736f, 0.200632f},    {4, 0, 3, 5, -0.826319f, -0.590612f, -0.368214f},
    {1, 2, 2, 9, -0.557409f, -0.233035f, 0.0534525f},   {2, 7, 3, 4, -0.0646826f, 0.00620476f, 0.0784847f},
    {2, 6, 2, 16, -0.192387f, -0.029699f, 0.215855f},   {2, 1, 3, 2, -0.0397818f, -0.00568076f, 0.0292026f},
    {5, 10, 1, 15, -0.53823f, -0.369934f, -0.190235f},  {3, 6, 2, 10, -0.124877f, 0.0296483f, 0.139239f},
    {2, 1, 1, 14, -0.101475f, 0.0225617f, 0.231971f},   {3, 5, 6, 4, -0.0799915f, -0.00729616f, 0.063262f},
    {1, 9, 2, 12, -0.272556f, 0.019424f, 0.302559f},    {3, 4, 2, 14, -0.164292f, -0.0321188f, 0.0846339f},
};
constexpr uint32_t kChromaGray[4] = {0, 1, 3, 2};

inline ChromaClassifier chroma_classifier(int j) {
    const ChromaClassifierSpec &s = kChromaSpecs[j];
    ChromaClassifier c{};
    c.type = s.type;
    c.y = s.y;
    c.h = s.h;
    c.w = s.w;
    c.t[0] = s.t0;
    c.t[1] = s.t1;
    c.t[2] = s.t2;
    for (int i = 0; i < 3; ++i) c.E[i] = (float)std::exp((double)c.t[i]);
    const int y = s.y, h = s.h, w = s.w, h2 = h / 2, w2 = w / 2, h3 = h / 3, w3 = w / 3, h23 = 2 * h / 3, w23 = 2 * w / 3;
    switch (s.type) {
        case 0:
            c.na = 1;
            c.a[0] = {0, w, y, y + h};
            break;
        case 1:
            c.na = c.nb = 1;
            c.a[0] = {0, w, y + h2, y + h};
            c.b[0] = {0, w, y, y + h2};
            break;
        case 2:
            c.na = c.nb = 1;
            c.a[0] = {w2, w, y, y + h};
            c.b[0] = {0, w2, y, y + h};
            break;
        case 3:
            c.na = c.nb = 2;
            c.a[0] = {0, w2, y + h2, y + h};
            c.a[1] = {w2, w, y, y + h2};
            c.b[0] = {0, w2, y, y + h2};
            c.b[1] = {w2, w, y + h2, y + h};
            break;
        case 4:
            c.na = 1;
            c.nb = 2;
            c.a[0] = {0, w, y + h3, y + h23};
            c.b[0] = {0, w, y, y + h3};
            c.b[1] = {0, w, y + h23, y + h};
            break;
        default:
            c.na = 1;
            c.nb = 2;
            c.a[0] = {w3, w23, y, y + h};
            c.b[0] = {0, w3, y, y + h};
            c.b[1] = {w23, w, y, y + h};
            break;
    }
    return c;
}

}  // namespace aid
