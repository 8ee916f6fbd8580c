// aidfp_mel.h -- what K10 (mel.hip) and its host side (mel.cpp) share: the device tables of spec/FPSPEC.md 10 and a
// chunk as the kernel sees it. The planning half is aidfp_mel_plan.h (no HIP).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aidfp_buffers.h"
#include "aidfp_mel_plan.h"

namespace aid {

struct MelTables {
    float2 win2[512];  // (w[2m], w[2m+1]), periodic Hann of 1024
    float2 t8[8];
    float2 t64[64];
    float2 t512[512];
    float2 t1k[512];  // exp(-2 pi i k / 1024), k < 512 (the real split)
    int32_t lo[kMelBands], len[kMelBands];  // band supports [lo, lo + len)
    int32_t K, max_len;
};

// x[src .. src + r) are the chunk's real samples (src counts samples from the call's PCM pointer); v[j] takes
// x[src + j mod r] for j < fill and 0 from there on (fill = r: zero mode; rep * r: repeatpad)
struct MelChunkDev {
    int64_t src;
    int32_t r, fill;
};

// the state an engine keeps for aid_mel_configure / aid_logmel (mel.cpp)
struct MelState {
    bool ready = false;
    int bank = kMelSlaney;
    std::vector<float> W;  // [513][64], what aid_mel_filters returns
    MelSupport sup;
    DevBuf<MelTables> d_tab;
    DevBuf<float> d_wc;  // [max_len][64]: W[lo_m + j][m], +0 past a band's support
    std::vector<MelChunk> plan;  // the last call's chunks
    HostBuf<MelChunkDev> h_chunks;
    DevBuf<MelChunkDev> d_chunks;
    DevBuf<float> d_in;   // staged host PCM
    DevBuf<float> d_out;  // the rows of a call whose `out` is host memory
    Event ev;             // the last K10 launch: the chunk table and the staging are free again behind it
};

}  // namespace aid
