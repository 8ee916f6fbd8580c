// aidfp_extract_plan.h -- the planning half of extraction (K1 -> K2 -> K3; extract.cpp acts on it): K2Policy,
// plan_extract and desc_differ. No HIP in here: tests/test_extract_plan_host.py compiles it with plain g++.
#pragma once
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/aidfp.h"
#include "aidfp_layout.h"

namespace aid {

constexpr int64_t kPlaneRows = (int64_t)3 << 18;  // power rows per K1 -> K2 clip group of a call (3 GB of plane)
constexpr int kK2Hold = 64;                       // calls at width 4 after a fall-back from width 2

struct K2Choice {  // of one call: quarter waves per K2 workgroup (2 or 4), K2 strips per resident workgroup slot
    int width;
    double slots_x;
};

// K2 strips per resident workgroup slot. Strip-cold K2 waves exit (peaks.hip) and their registers admit more
// workgroups per CU (LDS allows 7 instead of the 4 of an all-hot CU): with the fraction c of cold waves counted in
// earlier calls (K3 stores it in pinned memory; read without a sync, so it lags a few calls), the strips are made
// shorter and more numerous, 0.75 / (1 - c) per slot, quantised to 1, 1.25, 1.5 (few distinct descriptor arrays, so
// the cached ones keep matching)
// K2 width (peaks.hip): 2-wave workgroups over bins 0..511 fit 8 to a CU, all of their waves working, where band-
// limited audio leaves a CU 4 four-wave workgroups with two cold waves each; but they walk a strip a second time
// for bins 512..1023 when its upper half is hot, and K2 ends with its slowest workgroup: with 2 full-band clips
// among 256 (0.8 % of the strips walked twice) width 2 already took 0.196 ms against 0.118 at width 4, against
// 0.092 / 0.117 with none (profiles/k2_width_ab.txt). So width 2 is for calls in which no strip is walked twice.
// K2 counts those strips at width 2, K3 stores the count beside the cold one. From width 4 (the start) the choice
// goes to 2 when the cold count of a width-4 call says that there would be none: a strip needs no second walk
// exactly when its two upper quarter waves are strip-cold, so none does when half of all waves or more were
// cold (cold waves of the lower quarters can overstate this; the count at width 2 then corrects it). From width
// 2 it goes back to 4 as soon as a strip was walked twice, and stays there for kK2Hold calls, so a mixed workload
// does not flap: one slow call in 64. Counts of a launch at another width than the one in use are not applied
// (the words lag a few calls). Results never depend on the width or the strip length. At width 2 nothing exits on
// the audio it is chosen for: 1 strip per slot (1.25: K2 0.111 against 0.093 ms).
struct K2Policy {
    int width = 4;               // the adaptive choice; also the width of the last call
    int hold = 0;                // calls left at width 4 after a fall-back from width 2 (hysteresis)
    int force_width = 0;         // aid_engine_force K2_WIDTH: 2 or 4; 0 = adaptive
    double force_slots_x = 0.0;  // aid_engine_force K2_STRIPS_X100: fixed strips per slot; 0 = adaptive

    // cw = cold waves | waves << 32, sw = twice-walked strips | strips << 32 of the last K2 that K3 counted (waves /
    // strips: its width), as the caller read them from the two pinned words
    K2Choice choose(uint64_t cw, uint64_t sw) {
        const int seen_width = (sw >> 32) ? (int)((cw >> 32) / (sw >> 32)) : 0;
        if (force_width) {
            width = force_width;
        } else if (width == 4) {
            if (hold > 0) --hold;
            else if (seen_width == 4 && 2 * (uint64_t)(uint32_t)cw >= (cw >> 32)) width = 2;
        } else if (seen_width == 2 && (uint32_t)sw > 0) {
            width = 4;
            hold = kK2Hold;
        }
        if (force_slots_x > 0.0) return {width, force_slots_x};
        if (width != 4 || seen_width != 4) return {width, 1.0};
        const double c = std::min(1.0, (double)(uint32_t)cw / (double)(cw >> 32));
        return {width, c >= 0.45 ? 1.5 : c >= 0.3 ? 1.25 : 1.0};
    }
};

// clip groups: consecutive clips whose frames fit the plane-row cap each run K1 -> K2 on one power buffer (DESIGN.md,
// "bounded power planes"); K3 runs once over the call's mask. AID_FLAG_KEEP_POWER keeps every row: one group.
struct ClipGroup {
    int first = 0, n = 0;               // its clips
    int64_t frame0 = 0, frames = 0;     // its rows of the call's power and mask planes
    int64_t strips = 0, k1_strips = 0;  // K2 strips at strip_len (strip_base restarts per group); K1 wave-strips
    int strip_len = 0;
    int64_t flag_base = 0;  // its first row-flag word (aidfp_layout.h: strips x flag_words_per_strip(strip_len) words)
};

struct ExtractPlan {
    std::vector<ClipDesc> desc;              // what the device gets
    std::vector<int64_t> frames, hash_base;  // per clip, as in desc (hash_base is what aid_result_device hands out)
    std::vector<ClipGroup> groups;           // at least one, also for a call without clips
    int n_clips = 0, width = 4;
    int64_t total_frames = 0, strips = 0, chunks = 0, records = 0, flag_words = 0;
    int64_t staged = 0;       // samples of host PCM to stage: the clips' span as one copy (0 for device PCM)
    bool empty_clip = false;  // a clip without frames gets no count from K3: zero the counts first
    // K3 (landmarks.hip): a clip of several chunks needs the COUNT pass; when every clip is exactly one chunk, a
    // workgroup's clip is its chunk index. Not the totals' business: [frameless, two-chunk] has as many chunks as clips
    bool multi_chunk = false, one_chunk_each = false;
};

// Clip c is pcm[offsets[c], offsets[c + 1]), or with `ends` pcm[offsets[c], ends[c]). plane_rows: the cap of a group
// (0 = kPlaneRows); slots: resident K2 workgroups at `width`. p's vectors are reused: no allocation in steady state
inline void plan_extract(ExtractPlan &p, const int64_t *offsets, const int64_t *ends, int n_clips, int loc, int hop,
                         int64_t plane_rows, bool keep_power, int64_t slots, double slots_x, int width) {
    auto clip_end = [&](int c) { return ends ? ends[c] : offsets[c + 1]; };
    p.n_clips = n_clips;
    p.width = width;
    p.desc.resize(n_clips);
    p.frames.resize(n_clips);
    p.hash_base.resize(n_clips);
    p.groups.clear();
    const int64_t cap = plane_rows > 0 ? plane_rows : kPlaneRows;
    int first = 0;
    int64_t acc = 0;
    for (int c = 0; c < n_clips; ++c) {
        p.frames[c] = num_frames(clip_end(c) - offsets[c], hop);
        if (!keep_power && acc > 0 && acc + p.frames[c] > cap) {
            p.groups.push_back({first, c - first});
            first = c;
            acc = 0;
        }
        acc += p.frames[c];
    }
    p.groups.push_back({first, n_clips - first});
    p.total_frames = p.strips = p.chunks = p.records = p.flag_words = 0;
    p.staged = loc == AID_PCM_HOST && n_clips > 0 ? clip_end(n_clips - 1) - offsets[0] : 0;
    p.empty_clip = p.multi_chunk = false;
    p.one_chunk_each = n_clips > 0;
    int64_t k1_strips = 0;
    for (ClipGroup &g : p.groups) {
        g.strip_len = peak_strip_len(p.frames.data() + g.first, g.n, std::max<int64_t>(1, (int64_t)(slots * slots_x)));
        g.frame0 = p.total_frames;
        g.flag_base = p.flag_words;
        for (int c = g.first; c < g.first + g.n; ++c) {
            const int64_t F = p.frames[c], nck = (F + kHashChunk - 1) / kHashChunk;
            // pcm_off: device PCM is read in place (odd offsets: K1's float2 loads need dword alignment only), host PCM
            // from its staged span. strip_base counts within the group (K2 runs per group), other bases over the call
            p.desc[c] = {loc == AID_PCM_DEVICE ? offsets[c] : offsets[c] - offsets[0], F, p.total_frames, g.strips,
                         p.chunks, p.records, hash_capacity(F), k1_strips,
                         g.flag_base + g.strips * flag_words_per_strip(g.strip_len), g.strip_len};
            p.hash_base[c] = p.records;
            p.empty_clip |= F == 0;
            p.multi_chunk |= nck > 1;
            p.one_chunk_each &= nck == 1;
            p.total_frames += F;
            g.frames += F;
            g.strips += (F + g.strip_len - 1) / g.strip_len;
            g.k1_strips += (F + kStftStrip - 1) / kStftStrip;
            k1_strips += (F + kStftStrip - 1) / kStftStrip;
            p.chunks += nck;
            p.records += hash_capacity(F);
        }
        p.strips += g.strips;
        p.flag_words += g.strips * flag_words_per_strip(g.strip_len);
    }
}

// the descriptor cache's criterion: kernels take all but the group bounds and the PCM pointer from these bytes
inline bool desc_differ(const ClipDesc *a, size_t na, const ClipDesc *b, size_t nb) {
    return na != nb || (na > 0 && memcmp(a, b, na * sizeof(ClipDesc)) != 0);
}

}  // namespace aid
