// aidfp_vector_q8.h -- the pure arithmetic of the vector lane's int8 prefilter (spec/FPSPEC.md 9.1, K9q): the int8
// tile layout, the candidate count R and the error bound eps. No HIP types: the host code and the kernels of
// csrc/vector.hip / csrc/vector_q8.hip include it, and tests/test_vec_q8_plan_host.py compiles it alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define AID_Q8_HD __host__ __device__
#else
#define AID_Q8_HD
#endif

namespace aid {

constexpr int kVecQ8MaxR = 1024;          // first-stage candidates per query, at most
constexpr int kVecQ8MaxOversample = 64;   // aid_vec_prefilter's oversample is in [1, 64]
constexpr int kVecQ8Stats = 6;            // counters of aid_vec_prefilter_stats
constexpr int kVecQ8CntStride = 32;       // int32 per query in the prefilter's candidate counters: one 128-byte line

// Stored layout of a [rows][dim] int8 matrix (catalog and query tiles alike): rows in tiles of 32, a tile in
// k-steps of 32 (one v_mfma_i32_32x32x32_i8 each), and within a k-step the byte at (row i, k) sits at
// ((k >> 4) & 1) * 512 + i * 16 + (k & 15). Lane (i, h) of a wave fetches its 16 operand bytes of one MFMA with one
// aligned 16-byte load, and the 64 lanes of a wave read 1 KB contiguous. Queries and catalog use the same map, and
// an integer sum does not depend on the order of its terms, so the result needs only that the MFMA pairs byte j of
// lane (i, h) of A with byte j of lane (i', h) of B, whichever k the hardware calls it.
AID_Q8_HD inline size_t vec_q8_layout_index(int64_t row, int k, int dim) {
    return (size_t)(row >> 5) * 32 * (size_t)dim +
           (size_t)((k >> 5) * 1024 + ((k >> 4) & 1) * 512 + (int)(row & 31) * 16 + (k & 15));
}

// R = min(1024, max(limit, oversample * limit))
AID_Q8_HD inline int vec_q8_candidates(int limit, int oversample) {
    const int64_t r = (int64_t)limit * oversample;
    return (int)(r > kVecQ8MaxR ? kVecQ8MaxR : (r < limit ? limit : r));
}

// eps(q) = (e_q + (1 + e_q) * E) * (1 + 2^-10) + dim * 2^-21, binary64, left to right
AID_Q8_HD inline double vec_q8_eps(float e_q, float E, int dim) {
    const double eq = (double)e_q;
    const double a = 1.0 + eq;
    const double b = a * (double)E;
    const double c = eq + b;
    const double d = c * (1.0 + 0x1p-10);
    return d + (double)dim * 0x1p-21;
}

}  // namespace aid
