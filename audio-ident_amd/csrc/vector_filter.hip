// vector_filter.hip -- K9f, the allow-bitmaps of the vector lane's filtered search (spec/FPSPEC.md 9.2).
//
// A filtered batch evaluates its D <= 64 distinct filters once per entry, in one pass over the tombstones, the track
// column and the tags column (13 bytes an entry), and leaves D bitmaps of one bit per entry. The selection kernels of
// csrc/vector.hip and csrc/vector_q8.hip, which walk all n entries per query, then test one bit where the unfiltered
// kernels test dead[e]: 1 bit per (query, entry) instead of the 13 payload bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aidfp_vector.h"
#include "aidfp_vector_filter.h"

namespace aid {

// One wave per 64-bit word: lane l owns entry 64 * word + l. The wave reads its 64 tombstones, tracks and tags
// coalesced, evaluates filter d (read uniformly: the same address in every lane) and packs the 64 verdicts with a
// ballot; lane d keeps the word of filter d and stores it once the loop is over. Entries at and past n fail every
// filter, so the last word's upper bits and the words that pad a bitmap to `words` are 0. Grid: words / 4 workgroups
// of four waves (words is a multiple of 8).
__global__ __launch_bounds__(256) void k_vec_allow(const uint8_t *__restrict__ dead, const uint32_t *__restrict__ track,
                                                   const uint64_t *__restrict__ tags, int64_t n,
                                                   const aid_vec_filter *__restrict__ filters, int n_filters,
                                                   unsigned long long *__restrict__ allow, int64_t words) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= words) return;
    const int64_t e = w * 64 + lane;
    bool live = false;
    uint32_t tr = AID_VEC_NO_TRACK;
    uint64_t tg = 0;
    if (e < n) {
        live = dead[e] == 0;
        tr = track[e];
        tg = tags[e];
    }
    unsigned long long mine = 0;
    for (int d = 0; d < n_filters; ++d) {
        const aid_vec_filter f = filters[d];
        bool ok = live && (f.any_of == 0 || (tg & f.any_of) != 0) && (tg & f.all_of) == f.all_of && (tg & f.none_of) == 0;
#pragma unroll
        for (int j = 0; j < AID_VEC_MAX_EXCLUDE; ++j) ok = ok && tr != f.exclude[j];  // unused slots: the reserved id
        const unsigned long long m = __ballot(ok);
        if (lane == d) mine = m;
    }
    if (lane < n_filters) allow[(size_t)lane * words + w] = mine;
}

void vec_allow(const uint8_t *dead, const uint32_t *track, const uint64_t *tags, int64_t n, const aid_vec_filter *filters,
               int n_filters, unsigned long long *allow, hipStream_t s) {
    const int64_t words = vec_allow_words(n);
    hipLaunchKernelGGL(k_vec_allow, dim3((unsigned)(words / 4)), dim3(256), 0, s, dead, track, tags, n, filters, n_filters,
                       allow, words);
}

}  // namespace aid
