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

// Which entries a selection kernel may pick for query q: the compile-time parameter of k_vec_select,
// k_vec_slice_max, k_vec_filter and k_vec_filter_q8. VecLive is FPSPEC 9's "live" (the tombstone column; one pointer,
// so the kernels' arguments are what they were); VecAllowed is FPSPEC 9.2's "passes": bit e of the allow-bitmap
// fmap[q] that k_vec_allow wrote. A lane reads the 32-bit word e >> 5, so the 64 consecutive entries of a wave
// come from two or three adjacent words, one coalesced load, wherever the slice starts.
struct VecLive {
    const uint8_t *dead;
    __device__ __forceinline__ const uint8_t *row(int) const { return dead; }
    static __device__ __forceinline__ bool test(const uint8_t *r, int64_t e) { return !r[e]; }
};
struct VecAllowed {
    const uint32_t *bm;   // [bitmaps][words32]
    const int32_t *fmap;  // query of the launch -> bitmap
    int64_t words32;
    __device__ __forceinline__ const uint32_t *row(int q) const { return bm + (size_t)fmap[q] * words32; }
    static __device__ __forceinline__ bool test(const uint32_t *r, int64_t e) { return (r[e >> 5] >> (e & 31)) & 1u; }
};

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
