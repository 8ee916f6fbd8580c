// aidfp_speed_plan.h -- the planning half of the speed fan-out (FPSPEC 8.2; speed.cpp acts on it, K6s in resample.hip
// reads what it lays out): the rate pair and ResamplePlan of every speed, the length and packed offset of every
// (clip, speed) pair, the flattened block list of one launch, and the clip groups under a scratch budget. No HIP in
// here: tests/test_speed_plan_host.py compiles it with plain g++.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "resample_design.h"

#ifdef __HIPCC__
#define AID_SPEED_HD __host__ __device__
#else
#define AID_SPEED_HD
#endif

namespace aid {

constexpr int kSpeedMin = -500, kSpeedMax = 1000;        // per mille (FPSPEC 8.2)
constexpr int kSpeedMaxVariants = 256;                   // speeds of one call
constexpr int kSpeedBlock = 1024;                        // outputs of one K6s workgroup
constexpr int64_t kSpeedGroupFloats = (int64_t)1 << 28;  // variant PCM of one clip group: 1 GiB
constexpr int64_t kSpeedMaxLds = 65536;                  // bytes of LDS a K6s workgroup may stage
constexpr int64_t kSpeedMaxTaps = (int64_t)1 << 24;      // floats of one [up][J] tap table (as aid_resample)

enum SpeedStatus {
    kSpeedOk = 0,
    kSpeedBadRates,   // a rate <= 0, or a factor of the rate pair beyond int32
    kSpeedBadCount,   // n_speeds outside [1, 256]
    kSpeedBadSpeed,   // a speed outside [-500, +1000]
    kSpeedBadWindow,  // a workgroup's input window above 64 KB of LDS
    kSpeedBadTaps,    // up * J above 2^24
    kSpeedBadClips,   // offsets decrease, or more blocks than one launch holds
};

inline const char *speed_status_text(int st) {
    switch (st) {
        case kSpeedOk: return "ok";
        case kSpeedBadRates: return "sample rates must be > 0 and sr * (1000 + speed) must fit int32";
        case kSpeedBadCount: return "n_speeds must be in [1, 256]";
        case kSpeedBadSpeed: return "speed out of [-500, +1000] per mille";
        case kSpeedBadWindow: return "down/up ratio too large (LDS window > 64 KB)";
        case kSpeedBadTaps: return "tap table too large";
        default: return "bad clip offsets";
    }
}

// the rate pair of speed pm (FPSPEC 8.2): (sr_in * 1000, sr_e * (1000 + pm)), both within int32
inline int speed_rates(int32_t sr_in, int32_t sr_e, int32_t pm, int32_t *a, int32_t *b) {
    if (pm < kSpeedMin || pm > kSpeedMax) return kSpeedBadSpeed;
    if (sr_in <= 0 || sr_e <= 0) return kSpeedBadRates;
    const int64_t ra = (int64_t)sr_in * 1000, rb = (int64_t)sr_e * (1000 + pm);
    if (ra > INT32_MAX || rb > INT32_MAX) return kSpeedBadRates;
    *a = (int32_t)ra;
    *b = (int32_t)rb;
    return kSpeedOk;
}

// floats of input a K6s workgroup stages for kSpeedBlock consecutive outputs
inline int64_t speed_window_floats(int64_t up, int64_t down, int64_t J) { return (kSpeedBlock - 1) * down / up + J + 2; }

// ResamplePlan of one speed, with what aid_resample rejects for a rate pair rejected here
inline int speed_variant(int32_t sr_in, int32_t sr_e, int32_t pm, ResamplePlan &p) {
    int32_t a = 0, b = 0;
    if (int st = speed_rates(sr_in, sr_e, pm, &a, &b)) return st;
    const int64_t g = std::gcd((int64_t)a, (int64_t)b);
    const int64_t R = std::max(a / g, b / g);
    if (20 * R + 1 > kSpeedMaxTaps) return kSpeedBadTaps;  // up * J >= 2 * hl + 1, and hl = 10 * R stays in int32
    if (!resample_plan(a, b, p)) return kSpeedBadRates;
    if ((int64_t)p.up * p.J > kSpeedMaxTaps) return kSpeedBadTaps;
    if (speed_window_floats(p.up, p.down, p.J) * 4 > kSpeedMaxLds) return kSpeedBadWindow;
    return kSpeedOk;
}

inline int64_t speed_len(int64_t n, const ResamplePlan &p) { return n <= 0 ? 0 : (n * p.up + p.down - 1) / p.down; }

// what K6s reads per speed (device table); taps = the [up][J] table of the engine's cache
struct SpeedVarDev {
    int32_t up, down, hl, J;
    const float *taps;
    int32_t copy, pad;  // up == down: the output is the (downmixed) input sample, as FPSPEC 8 copies there
};

// the pair of block b: the last p in [0, n_pairs) with blk_first[p] <= b (pairs without outputs own no block)
AID_SPEED_HD inline int speed_find_pair(const int64_t *blk_first, int n_pairs, int64_t b) {
    int lo = 0, hi = n_pairs;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (blk_first[mid] <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct SpeedGroup {
    int first = 0, n = 0;  // its clips
    int64_t floats = 0;    // variant PCM of all their pairs
};

struct SpeedPlan {
    int n_clips = 0, n_speeds = 0;
    std::vector<ResamplePlan> var;                 // per speed
    std::vector<int64_t> clip_off;                 // [n_clips + 1]: the clips' frames, from the first clip's start
    std::vector<int64_t> dst_off, blk_first;       // [n_pairs + 1], pair = clip * n_speeds + v: packed, prefix sums
    std::vector<SpeedGroup> groups;                // whole clips; at least one group
    int64_t lds_floats = 0;                        // the widest window of the speeds
    int64_t total() const { return dst_off.back(); }
    int64_t blocks() const { return blk_first.back(); }
};

// Clip c = frames [offsets[c], offsets[c + 1]). budget: variant floats per clip group (0 = kSpeedGroupFloats). p's
// vectors are reused: no allocation in steady state. Returns a SpeedStatus; p is valid only for kSpeedOk
inline int plan_speeds(SpeedPlan &p, const int64_t *offsets, int n_clips, int32_t sr_in, int32_t sr_e,
                       const int32_t *speeds_pm, int n_speeds, int64_t budget) {
    if (n_speeds < 1 || n_speeds > kSpeedMaxVariants || !speeds_pm) return kSpeedBadCount;
    if (n_clips < 0 || (n_clips > 0 && !offsets)) return kSpeedBadClips;
    p.n_clips = n_clips;
    p.n_speeds = n_speeds;
    p.var.resize(n_speeds);
    p.lds_floats = 0;
    for (int v = 0; v < n_speeds; ++v) {
        if (int st = speed_variant(sr_in, sr_e, speeds_pm[v], p.var[v])) return st;
        p.lds_floats = std::max(p.lds_floats, speed_window_floats(p.var[v].up, p.var[v].down, p.var[v].J));
    }
    const size_t n_pairs = (size_t)n_clips * n_speeds;
    p.clip_off.resize((size_t)n_clips + 1);
    p.dst_off.resize(n_pairs + 1);
    p.blk_first.resize(n_pairs + 1);
    p.groups.clear();
    p.clip_off[0] = p.dst_off[0] = p.blk_first[0] = 0;
    const int64_t cap = budget > 0 ? budget : kSpeedGroupFloats;
    SpeedGroup g;
    for (int c = 0; c < n_clips; ++c) {
        const int64_t n = offsets[c + 1] - offsets[c];
        if (n < 0 || n > ((int64_t)1 << 31)) return kSpeedBadClips;  // n * up stays below 2^63
        p.clip_off[c + 1] = p.clip_off[c] + n;
        int64_t floats = 0;
        for (int v = 0; v < n_speeds; ++v) {
            const size_t k = (size_t)c * n_speeds + v;
            const int64_t m = speed_len(n, p.var[v]);
            p.dst_off[k + 1] = p.dst_off[k] + m;
            p.blk_first[k + 1] = p.blk_first[k] + (m + kSpeedBlock - 1) / kSpeedBlock;
            floats += m;
        }
        if (g.n > 0 && g.floats + floats > cap) {
            p.groups.push_back(g);
            g = SpeedGroup{c, 0, 0};
        }
        ++g.n;
        g.floats += floats;
    }
    p.groups.push_back(g);
    for (const SpeedGroup &q : p.groups) {  // one launch per group: grid.x is 31 bits
        const size_t a = (size_t)q.first * n_speeds, b = (size_t)(q.first + q.n) * n_speeds;
        if (p.blk_first[b] - p.blk_first[a] > INT32_MAX) return kSpeedBadClips;
    }
    return kSpeedOk;
}

}  // namespace aid
