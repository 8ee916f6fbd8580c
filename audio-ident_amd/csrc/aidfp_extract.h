// aidfp_extract.h -- extraction's state (K1 -> K2 -> K3; spec/FPSPEC.md 1-6), one per engine as aid_engine::ext.
// extract.cpp plans a call (aidfp_extract_plan.h), reserves, stages, uploads and launches; others read the results.
#pragma once
#include "aidfp_buffers.h"
#include "aidfp_extract_plan.h"

namespace aid {

struct Extractor {
    DevBuf<float> pcm_stage, power;  // host PCM staged as one copy (raw bytes to both formats); one clip group's plane
    DevBuf<uint64_t> mask, hotw;     // the call's peak bits; K1 -> K2: per power row, bit hot_bit(c) = chunk c is > thr
    // K2 -> K3 (aidfp_layout.h): per K2 strip, 32 rows and quarter one word; a mask quarter without its bit is stale
    DevBuf<uint32_t> rowflags;
    // FPSPEC 5.1 (peak_rel > 0): per clip the bits of max Q over its plane: zeroed ahead of K1, raised by it, read by K2
    DevBuf<uint32_t> clip_qmax;
    DevBuf<uint32_t> k2_cold;  // K2: strip-cold wave counters (64) and twice-walked strip counters (64), summed and reset by K3
    // pinned, host-mapped: K3 stores (cold waves | waves << 32) and (twice-walked strips | strips << 32) of the last K2
    HostBuf<uint64_t> h_cold;
    uint64_t *h_cold_dev = nullptr;  // its device address
    DevBuf<int64_t> chunk_counts, counts;
    DevBuf<uint64_t> records;
    // descriptor cache: h_desc (pinned) holds the desc_n descriptors last uploaded, to device address desc_dev
    DevBuf<ClipDesc> desc;
    HostBuf<ClipDesc> h_desc;
    size_t desc_n = 0;
    ClipDesc *desc_dev = nullptr;
    Event desc_ev, stage_ev;  // reuse hazards (no stream sync per call): an async H2D copy reads h_desc, K1 pcm_stage
    hipStream_t stage_stream = nullptr;  // the stream whose K1 read pcm_stage last
    K2Policy k2;
    int64_t k2_slots[2] = {1, 1};  // resident K2 workgroups on the device (CUs x blocks per CU) at width 2, 4
    int64_t k1_slots = 1;          // resident K1 waves (CUs x kStftWaves: one K1 workgroup per CU)
    int64_t k1_waves = 0;          // aid_engine_force K1_WAVES: the wave count K1 splits over (0 = k1_slots)
    int64_t plane_rows = 0;        // aid_engine_force PLANE_ROWS: power rows per clip group (0 = kPlaneRows)
    ExtractPlan plan;  // of the last call: what the result readers, the queries and the index append go by
    bool have_result = false;  // false while a call that failed leaves the plan and the buffers out of step
};

}  // namespace aid
