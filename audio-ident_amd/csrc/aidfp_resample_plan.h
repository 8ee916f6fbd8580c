// aidfp_resample_plan.h -- the host-only half of K6 `resample` (spec/FPSPEC.md 8; the kernels are in resample.hip): which
// kernel form a reduced rate pair (up, down, J) runs, the outputs and threads of one workgroup, the floats of LDS it
// stages, and what aid_resample refuses. No HIP in here: tests/test_resample_plan_host.py compiles it with g++ (plain
// and sanitized) into a stand-alone program, resample.hip launches by it and engine.cpp rejects by it.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace aid {

constexpr int kResThreads = 256;
constexpr int kResPerThread = 4;
constexpr int kResBlock = kResThreads * kResPerThread;  // outputs of a k_resample workgroup

constexpr int kResR = 16;  // k_resample_phase: outputs per thread (one phase); a workgroup holds up * kResR outputs
constexpr int kResMaxPhaseUp = 1024;         // phase-major form: 1 < up <= this ...
constexpr int64_t kResMaxPhaseWindow = 12288;  // ... while the window of up * kResR outputs stays within 48 KB

#ifndef AID_K6_DECR
#define AID_K6_DECR 4
#endif
constexpr int kDecR = AID_K6_DECR;  // k_decimate: consecutive outputs per thread
constexpr int kDecThreads = 256;
constexpr int kDecBlock = kDecR * kDecThreads;

constexpr int64_t kResMaxLds = 65536;               // bytes of LDS a K6 workgroup may stage
constexpr int64_t kResMaxTaps = (int64_t)1 << 24;   // floats of one [up][J] tap table

enum ResPath : int {
    kResReject = 0,
    kResDecimate3,   // k_decimate<., 3, 61>: 48 kHz -> 16 kHz
    kResPhase,       // k_resample_phase: a thread owns one phase
    kResUniform,     // k_resample MODE 2: integer decimation, wave-uniform taps
    kResGlobalTaps,  // k_resample MODE 0: per-lane phase rows read from L1/L2
};

enum ResStatus : int {
    kResOk = 0,
    kResBadWindow,  // a workgroup's input window above 64 KB of LDS
    kResBadTaps,    // up * J above 2^24
};

inline const char *resample_status_text(int st) {
    switch (st) {
        case kResOk: return "ok";
        case kResBadWindow: return "down/up ratio too large (LDS window > 64 KB)";
        default: return "tap table too large";
    }
}

// phase-major blocks hold up * kResR outputs: used while that window stays small (common rate
// pairs: up = 147, 160, 441); very large up (near-coprime rates) keep the 1024-output blocks
inline bool use_phase(int up, int down, int J) {
    return up > 1 && up <= kResMaxPhaseUp && ((int64_t)up * kResR - 1) * down / up + J + 2 <= kResMaxPhaseWindow;
}

// floats of input one workgroup stages: the window of its up * kResR (phase form) or kResBlock consecutive outputs, + 2
inline int64_t window_floats(int up, int down, int J) {
    if (use_phase(up, down, J)) return ((int64_t)up * kResR - 1) * down / up + J + 2;
    return (int64_t)(kResBlock - 1) * down / up + J + 2;
}

inline int64_t resample_lds_floats(int up, int down, int J) { return window_floats(up, down, J); }

// k_decimate's window of kDecBlock outputs; it stages 4 floats more (the last thread's 16-B over-read)
constexpr int64_t dec_window(int down, int J) { return (int64_t)(kDecBlock - 1) * down + J; }

struct ResLaunch {
    int path = kResReject;
    int status = kResOk;     // why, when path is kResReject
    int64_t block = 0;       // outputs of one workgroup: grid.x = ceil(count / block)
    int threads = 0;         // of one workgroup
    int64_t lds_floats = 0;  // dynamic LDS of the launch
};

// The form (up, down, J) runs and its launch shape. The window test comes first, as aid_resample reports it first
inline ResLaunch resample_launch_plan(int up, int down, int J) {
    ResLaunch r;
    if (resample_lds_floats(up, down, J) * 4 > kResMaxLds) {
        r.status = kResBadWindow;
        return r;
    }
    if ((int64_t)up * J > kResMaxTaps) {
        r.status = kResBadTaps;
        return r;
    }
    if (use_phase(up, down, J)) {
        r.path = kResPhase;
        r.block = (int64_t)up * kResR;
        r.threads = std::min(256, (up + 63) / 64 * 64);
        r.lds_floats = resample_lds_floats(up, down, J);
        return r;
    }
#ifndef AID_K6_NO_DEC  // diagnostic builds: MODE 2 for every decimation (A/B)
    if (up == 1 && down == 3 && J == 61) {  // 48 kHz -> 16 kHz (browser capture -> the index rate)
        r.path = kResDecimate3;
        r.block = kDecBlock;
        r.threads = kDecThreads;
        r.lds_floats = dec_window(3, 61) + 4;
        return r;
    }
#endif
    r.path = up == 1 ? kResUniform : kResGlobalTaps;
    r.block = kResBlock;
    r.threads = kResThreads;
    r.lds_floats = resample_lds_floats(up, down, J);
    return r;
}

}  // namespace aid
