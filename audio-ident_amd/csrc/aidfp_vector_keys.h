// aidfp_vector_keys.h -- device helpers shared by the vector lane's translation units (csrc/vector.hip and
// csrc/vector_q8.hip): the selection keys and the bitonic sort over them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace aid {

// Selection keys: larger = better. vec_score_key maps a score's bits so that unsigned order is numeric order
// (-0 counts as +0; never 0 for a number). The 64-bit key has it in the high word and ~entry in the low word, so
// the lower entry wins a tie. 0 = no entry.
__device__ __forceinline__ uint32_t vec_score_key(float score) {
    uint32_t b = __float_as_uint(score);
    if (b == 0x80000000u) b = 0;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ unsigned long long vec_key(float score, uint32_t entry) {
    return ((unsigned long long)vec_score_key(score) << 32) | (0xFFFFFFFFu - entry);
}
__device__ __forceinline__ float vec_key_score(unsigned long long key) {
    const uint32_t m = (uint32_t)(key >> 32);
    return __uint_as_float((m & 0x80000000u) ? (m & 0x7FFFFFFFu) : ~m);
}
__device__ __forceinline__ uint32_t vec_key_entry(unsigned long long key) { return 0xFFFFFFFFu - (uint32_t)key; }

// Bitonic sort, descending, of sp (a power of two) keys in LDS by a 256-thread workgroup.
template <typename T>
__device__ __forceinline__ void vec_sort_desc(T *keys, int sp) {
    for (int k = 2; k <= sp; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (sp >> 1); t += 256) {
                const int i = 2 * t - (t & (j - 1));
                const T a = keys[i], b = keys[i + j];
                const bool desc = (i & k) == 0;
                if ((a < b) == desc && a != b) {
                    keys[i] = b;
                    keys[i + j] = a;
                }
            }
            __syncthreads();
        }
    }
}

}  // namespace aid
