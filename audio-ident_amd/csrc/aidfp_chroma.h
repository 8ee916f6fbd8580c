// aidfp_chroma.h -- what K11 (chroma.hip) and its host side (chroma.cpp) share: the device tables of
// spec/FPSPEC.md 11 and the engine's state for the content fingerprint. The planning half is aidfp_chroma_plan.h
// (no HIP).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "aidfp_buffers.h"
#include "aidfp_chroma_plan.h"

namespace aid {

struct ChromaTables {
    float2 win2[kChromaN / 2];  // (w[2m], w[2m+1]), symmetric Hamming of 4096
    float2 t8[8];
    float2 t16[16];
    float2 t128[128];
    float2 t2048[2048];
    float2 t4096[2048];  // exp(-2 pi i k / 4096), k < 2048 (the real split)
    int32_t n_runs;
    int32_t run_lo[kChromaMaxRuns], run_len[kChromaMaxRuns], run_note[kChromaMaxRuns];
    ChromaClassifier cls[kChromaClassifiers];
};

// the state an engine keeps for aid_chroma* (chroma.cpp)
struct ChromaState {
    bool ready = false;
    DevBuf<ChromaTables> d_tab;
    std::vector<int64_t> frame_off, word_off;  // the last call's offsets
    std::vector<ChromaRowBlock> row_blocks;
    std::vector<ChromaItemBlock> item_blocks;
    HostBuf<ChromaRowBlock> h_rb;
    DevBuf<ChromaRowBlock> d_rb;
    HostBuf<ChromaItemBlock> h_ib;
    DevBuf<ChromaItemBlock> d_ib;
    DevBuf<float> d_in;        // staged host PCM
    DevBuf<float> d_rows;      // C[frames][12] of a call (or the caller's host rows)
    DevBuf<uint32_t> d_words;  // the words of a call whose output is host memory
    Event ev;                  // the last K11 launch: the block lists and the staging are free again behind it
};

}  // namespace aid
