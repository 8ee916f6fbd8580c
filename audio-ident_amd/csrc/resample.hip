// resample.hip -- K6 `resample`: stereo downmix + rational polyphase resampling (FPSPEC 8),
// the GPU replacement of ffmpeg's `-ac 1 -ar <rate>` in the reference
// (audio-ident-service/app/audio/decode.py:41-60).
//
// A workgroup produces kResBlock consecutive outputs (4 per thread, strided by 256 so each
// store instruction writes 1 KB contiguous). It stages the input window those outputs touch
// ONCE into LDS, downmixed to mono at staging time (float2 loads for stereo), zero outside the
// clip; every output then runs its J-tap dot product from LDS with the phase row of the
// [up][J] tap table, read from L1/L2 (no rate pair that aid_resample accepts has a table small enough
// to stage beside its window: tests/test_resample_plan_host.py scans them all). HBM traffic is the algorithmic
// minimum: input once (+ the J-sample window overlap per block) and output once.
// Which form a rate pair runs, and its launch shape, is decided in aidfp_resample_plan.h (host only).
#include "aidfp_device.h"
#include "aidfp_launch.h"
#include "aidfp_resample_plan.h"
#include "aidfp_speed_plan.h"

namespace aid {

// The input of one launch: stream frames [b_base, b_base + b_n) at b + y * b_stride and, optionally, the frames
// [a_base, a_base + a_n) just before them at a + y * a_stride (y = stream of a batch), so a live stream's chunk is read
// where its caller left it and only the last few frames of the previous chunk are kept (StreamBank); 0 elsewhere
// T = the input's sample type: float, or int16_t (integer PCM, FPSPEC 8: x = float(q) * 2^-15, exact); strides count T
template <typename T>
struct ResInT {
    const T *a;
    int64_t a_base, a_n, a_stride;
    const T *b;
    int64_t b_base, b_n, b_stride;
};
typedef ResInT<float> ResIn;

// s16 -> FPSPEC sample value; the stereo downmix is (xL + xR) * 0.5f on the converted values, as for float input
__device__ __forceinline__ float s16_val(int16_t q) { return (float)q * 0x1p-15f; }
__device__ __forceinline__ float s16_lo(uint32_t w) { return s16_val((int16_t)(w & 0xFFFFu)); }
__device__ __forceinline__ float s16_hi(uint32_t w) { return (float)((int32_t)w >> 16) * 0x1p-15f; }

// Stage input samples lo .. lo + cnt - 1 (stream indices) into sx[0 .. cnt), downmixed at load time. The loads go out
// kStageBatch at a time before their LDS stores: a plain strided loop waits for each load before the next (its trip
// count is not known at compile time), so a block staging ~12 samples per thread paid ~12 serial memory latencies
#ifndef AID_K6_STAGE_BATCH
#define AID_K6_STAGE_BATCH 8
#endif
constexpr int kStageBatch = AID_K6_STAGE_BATCH;
template <bool STEREO, typename T>
__device__ __forceinline__ void stage_window(const ResInT<T> &in, int64_t lo, int cnt, float *sx, int tid, int nthreads) {
    constexpr bool S16 = sizeof(T) == 2;
    const int64_t y = blockIdx.y;
    const T *A = in.a + y * in.a_stride, *B = in.b + y * in.b_stride;
    // a window wholly inside part B whose 16-B words are all in it (B 16-B aligned): 16-B loads, two stereo frames or
    // four mono samples each. The hardware moved ~3.3 TB/s on 8-B lane loads of the 256-stream push (77 % of K6's
    // wave cycles waiting, every fetched byte needed) and 22 % more on 16-B ones (profiles/r06yz_k6_v4_ab.txt)
    // (s16: four stereo frames or eight mono samples per word, converted and downmixed here: LDS holds f32 mono)
    constexpr int kPer = (STEREO ? 2 : 4) * (S16 ? 2 : 1);  // stream samples per 16-B word
    const int64_t k0 = lo - in.b_base;
#if defined(AID_K6_NO_V4)  // diagnostic A/B build: 8-B / 4-B loads only
    if (false) {
#else
    if (k0 >= 0 && (k0 + cnt + kPer - 1) / kPer * kPer <= in.b_n && (reinterpret_cast<uintptr_t>(B) & 15) == 0) {
#endif
        const int64_t p0 = k0 / kPer;
        const int np = (int)((k0 + cnt - 1) / kPer - p0 + 1);
        if constexpr (S16) {
            const uint4 *B4 = reinterpret_cast<const uint4 *>(B);
            for (int i0 = tid; i0 < np; i0 += kStageBatch * nthreads) {
                uint4 v[kStageBatch];
#pragma unroll
                for (int u = 0; u < kStageBatch; ++u) {
                    const int i = i0 + u * nthreads;
                    v[u] = i < np ? B4[p0 + i] : make_uint4(0u, 0u, 0u, 0u);
                }
#pragma unroll
                for (int u = 0; u < kStageBatch; ++u) {
                    const int i = i0 + u * nthreads;
                    if (i >= np) continue;
                    const int f = (int)(kPer * (p0 + i) - k0);  // window index of the word's first sample
                    const uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if constexpr (STEREO) {
                            if (f + j >= 0 && f + j < cnt) sx[f + j] = (s16_lo(w[j]) + s16_hi(w[j])) * 0.5f;
                        } else {
                            if (f + 2 * j >= 0 && f + 2 * j < cnt) sx[f + 2 * j] = s16_lo(w[j]);
                            if (f + 2 * j + 1 >= 0 && f + 2 * j + 1 < cnt) sx[f + 2 * j + 1] = s16_hi(w[j]);
                        }
                    }
                }
            }
            return;
        }
        const float4 *B4 = reinterpret_cast<const float4 *>(B);
        for (int i0 = tid; i0 < np; i0 += kStageBatch * nthreads) {
            float4 v[kStageBatch];
#pragma unroll
            for (int u = 0; u < kStageBatch; ++u) {
                const int i = i0 + u * nthreads;
                v[u] = i < np ? B4[p0 + i] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < kStageBatch; ++u) {
                const int i = i0 + u * nthreads;
                if (i >= np) continue;
                const int f = (int)(kPer * (p0 + i) - k0);  // window index of the word's first sample
                if constexpr (STEREO) {
                    if (f >= 0) sx[f] = (v[u].x + v[u].y) * 0.5f;
                    if (f + 1 < cnt) sx[f + 1] = (v[u].z + v[u].w) * 0.5f;
                } else {
                    if (f >= 0) sx[f] = v[u].x;
                    if (f + 1 >= 0 && f + 1 < cnt) sx[f + 1] = v[u].y;
                    if (f + 2 >= 0 && f + 2 < cnt) sx[f + 2] = v[u].z;
                    if (f + 3 < cnt) sx[f + 3] = v[u].w;
                }
            }
        }
        return;
    }
    for (int i0 = tid; i0 < cnt; i0 += kStageBatch * nthreads) {
        float v[kStageBatch];
#pragma unroll
        for (int u = 0; u < kStageBatch; ++u) {
            const int i = i0 + u * nthreads;
            const int64_t g = lo + i;
            const T *p = nullptr;
            int64_t k = 0;
            if (i < cnt) {
                if (g >= in.b_base && g - in.b_base < in.b_n) {
                    p = B;
                    k = g - in.b_base;
                } else if (g >= in.a_base && g - in.a_base < in.a_n) {
                    p = A;
                    k = g - in.a_base;
                }
            }
            v[u] = 0.0f;
            if (p) {
                if constexpr (S16 && STEREO) {  // one frame = one dword (the engine checks the 4-byte alignment)
                    const uint32_t w = reinterpret_cast<const uint32_t *>(p)[k];
                    v[u] = (s16_lo(w) + s16_hi(w)) * 0.5f;
                } else if constexpr (S16) {
                    v[u] = s16_val(p[k]);
                } else if constexpr (STEREO) {
                    const float2 s = reinterpret_cast<const float2 *>(p)[k];
                    v[u] = (s.x + s.y) * 0.5f;
                } else {
                    v[u] = p[k];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kStageBatch; ++u)
            if (i0 + u * nthreads < cnt) sx[i0 + u * nthreads] = v[u];
    }
}

// MODE 0: per-lane phase rows, taps from L1/L2; 2: integer decimation (up == 1): one phase,
// the taps are wave-uniform and read as scalar loads (no LDS traffic for them)
template <bool STEREO, int MODE, typename T = float>
__global__ __launch_bounds__(kResThreads) void k_resample(ResInT<T> in, int up, int down, int hl, int J,
                                                         const float *__restrict__ taps, float *__restrict__ dst,
                                                         int64_t m_first, int64_t m_end, int64_t dst_stride) {
    // Outputs m_first .. m_end-1 (stream indices) go to dst[m - m_first].
    // blockIdx.y = stream of a batch: its input as ResIn says, its output at dst + y * dst_stride (floats)
    dst += (int64_t)blockIdx.y * dst_stride;
    static_assert(MODE == 0 || MODE == 2, "k_resample: MODE 0 (rational) or 2 (integer decimation)");
    extern __shared__ float sx[];  // the input window
    const int tid = threadIdx.x;
    const int64_t m0 = m_first + (int64_t)blockIdx.x * kResBlock;
    const int64_t mlast = min(m0 + kResBlock - 1, m_end - 1);
    const int64_t lo = (m0 * down + hl) / up - (J - 1);
    const int64_t hi = (mlast * down + hl) / up;  // inclusive
    const int cnt = (int)(hi - lo + 1);
    stage_window<STEREO>(in, lo, cnt, sx, tid, kResThreads);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kResPerThread; ++r) {
        const int64_t m = m0 + tid + r * kResThreads;
        if (m >= m_end) break;
        const int64_t c = m * down + hl;
        float acc = 0.0f;
        if constexpr (MODE == 2) {
            const float *xp = sx + (c - lo);
            for (int j = 0; j < J; ++j) acc = __builtin_fmaf(taps[j], xp[-j], acc);  // taps[j]: uniform
        } else {
            const int p = (int)(c % up);
            const float *tp = taps + (int64_t)p * J;
            const float *xp = sx + (c / up - lo);
            for (int j = 0; j < J; ++j) acc = __builtin_fmaf(tp[j], xp[-j], acc);
        }
        dst[m - m_first] = acc;
    }
}

// Integer decimation (up == 1) with compile-time DOWN and J (48 kHz -> 16 kHz: 3, 61), register-blocked: a thread
// owns kDecR consecutive outputs, whose windows are one run of (kDecR - 1) * DOWN + J staged inputs; it reads that run
// from LDS once with 16-B loads into registers and runs the kDecR dot products from there: ~19 LDS dwords per output
// instead of J single-dword reads (MODE 2). Same fma chain per output (taps j = 0..J-1 in order), so the outputs are
// MODE 2's bit for bit. kDecR 4 (80 VGPRs, 6 waves per SIMD): 98 us per 256-stream push against MODE 2's 105 and
// kDecR 8's 155 (164 VGPRs, 3 waves per SIMD; profiles/r06p_k6_decimate_ab.txt): K6 is not bound by its LDS reads.
// (kDecR and kDecThreads: aidfp_resample_plan.h)
template <bool STEREO, int DOWN, int J, typename T = float>
__global__ __launch_bounds__(kDecThreads) void k_decimate(ResInT<T> in, int hl, const float *__restrict__ taps,
                                                          float *__restrict__ dst, int64_t m_first, int64_t m_end,
                                                          int64_t dst_stride) {
    static_assert((kDecR * DOWN) % 4 == 0, "a thread's run must start 16-B aligned in LDS");
    constexpr int NX = (kDecR - 1) * DOWN + J;  // inputs of one thread's outputs
    constexpr int NX4 = (NX + 3) / 4;
    dst += (int64_t)blockIdx.y * dst_stride;
    extern __shared__ float sx[];  // dec_window(DOWN, J) + 4 floats (the last run's 16-B over-read)
    const int tid = threadIdx.x;
    const int64_t m0 = m_first + (int64_t)blockIdx.x * (kDecThreads * kDecR);
    const int64_t mlast = min(m0 + kDecThreads * kDecR - 1, m_end - 1);
    const int64_t lo = m0 * DOWN + hl - (J - 1);
    const int cnt = (int)(mlast * DOWN + hl - lo + 1);
    stage_window<STEREO>(in, lo, cnt, sx, tid, kDecThreads);
    __syncthreads();
    const int64_t mb = m0 + (int64_t)tid * kDecR;
    if (mb >= m_end) return;
    // output mb + r reads sx[tid * kDecR * DOWN + r * DOWN + J - 1 - j]; words past cnt only feed outputs >= m_end
    float x[NX4 * 4];
    const float4 *p = reinterpret_cast<const float4 *>(sx + tid * kDecR * DOWN);
#pragma unroll
    for (int i = 0; i < NX4; ++i) {
        const float4 v = p[i];
        x[4 * i] = v.x;
        x[4 * i + 1] = v.y;
        x[4 * i + 2] = v.z;
        x[4 * i + 3] = v.w;
    }
    float acc[kDecR];
#pragma unroll
    for (int r = 0; r < kDecR; ++r) acc[r] = 0.0f;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const float t = taps[j];  // uniform
#pragma unroll
        for (int r = 0; r < kDecR; ++r) acc[r] = __builtin_fmaf(t, x[r * DOWN + J - 1 - j], acc[r]);
    }
    float *o = dst + (mb - m_first);
    if (mb + kDecR <= m_end && ((reinterpret_cast<uintptr_t>(o) & 15) == 0)) {
#pragma unroll
        for (int r = 0; r < kDecR; r += 4)
            *reinterpret_cast<float4 *>(o + r) = make_float4(acc[r], acc[r + 1], acc[r + 2], acc[r + 3]);
    } else {
#pragma unroll
        for (int r = 0; r < kDecR; ++r)
            if (mb + r < m_end) o[r] = acc[r];
    }
}

// MODE 3 (up > 1, the default): phase-major. Outputs m and m + up share a phase, so a thread
// owns one phase of the block and kResR outputs up apart: it loads its phase's taps once per
// 8-tap chunk (L1-resident table) and runs kResR dot products with them. Per output that is
// J input reads from LDS (+ J / kResR tap loads) instead of 2J LDS reads with per-lane phase
// rows (which also bank-conflicted). Same fma chain per output (taps j = 0..J-1 in order).
// (kResR outputs per thread: aidfp_resample_plan.h)
template <bool STEREO, typename T = float>
__global__ __launch_bounds__(256) void k_resample_phase(ResInT<T> in, int up, int down, int hl, int J,
                                                       const float *__restrict__ taps, float *__restrict__ dst,
                                                       int64_t m_first, int64_t m_end, int64_t dst_stride) {
    dst += (int64_t)blockIdx.y * dst_stride;  // stream of a batch (k_resample)
    extern __shared__ float sx[];
    const int tid = threadIdx.x;
    const int64_t m0 = m_first + (int64_t)blockIdx.x * up * kResR;
    const int64_t mlast = min(m0 + (int64_t)up * kResR - 1, m_end - 1);
    const int64_t lo = (m0 * down + hl) / up - (J - 1);
    const int64_t hi = (mlast * down + hl) / up;  // inclusive
    const int cnt = (int)(hi - lo + 1);
    stage_window<STEREO>(in, lo, cnt, sx, tid, (int)blockDim.x);
    __syncthreads();
    for (int t = tid; t < up; t += blockDim.x) {
        const int64_t c0 = (m0 + t) * down + hl;  // output r: c = c0 + r * up * down
        const int p = (int)(c0 % up);
        const int b0 = (int)(c0 / up - lo);       // its input index: b0 + r * down - j
        const float *tp = taps + (int64_t)p * J;
        float acc[kResR];
#pragma unroll
        for (int r = 0; r < kResR; ++r) acc[r] = 0.0f;
        for (int jb = 0; jb < J; jb += 8) {
            float tv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) tv[u] = jb + u < J ? tp[jb + u] : 0.0f;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (jb + u >= J) break;  // uniform
#pragma unroll
                for (int r = 0; r < kResR; ++r) acc[r] = __builtin_fmaf(tv[u], sx[b0 + r * down - (jb + u)], acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < kResR; ++r) {
            const int64_t m = m0 + t + (int64_t)r * up;
            if (m < m_end) dst[m - m_first] = acc[r];
        }
    }
}

// n_streams > 1: the same output range of n_streams streams in one launch (grid.y = stream), each stream's input
// src_stride samples (of T) after the previous one's and its output dst_stride floats after; bit for bit the outputs of
// n_streams single launches (same staging, same fma chain per output). With hist_n > 0 the input is two parts:
// stream frames [in_base - hist_n, in_base) from hist (hist_stride per stream), then [in_base, in_base + n) from src.
template <typename T>
static void launch_resample_t(const T *src, int64_t in_base, int64_t n, int channels, int up, int down, int hl, int J,
                              const float *taps, float *dst, int64_t m_first, int64_t count, hipStream_t s, int n_streams,
                              int64_t src_stride, int64_t dst_stride, const T *hist, int64_t hist_n, int64_t hist_stride) {
    if (count <= 0 || n_streams <= 0) return;
    const ResInT<T> in{hist_n > 0 ? hist : src, in_base - hist_n, hist_n, hist_stride, src, in_base, n, src_stride};
    const ResLaunch pl = resample_launch_plan(up, down, J);
    if (pl.path == kResReject) return;  // not from the engine: aid_resample refuses those with AID_ERR_INVALID
    const int64_t m_end = m_first + count;
    const dim3 g((unsigned)((count + pl.block - 1) / pl.block), (unsigned)n_streams), b((unsigned)pl.threads);
    const size_t lds = (size_t)pl.lds_floats * sizeof(float);
    const bool st = channels == 2;
#define AID_RS_LAUNCH(KERNEL, ...) \
    hipLaunchKernelGGL((KERNEL), g, b, lds, s, in, __VA_ARGS__, taps, dst, m_first, m_end, dst_stride)
    switch (pl.path) {
        case kResPhase:
            if (st) AID_RS_LAUNCH((k_resample_phase<true, T>), up, down, hl, J);
            else AID_RS_LAUNCH((k_resample_phase<false, T>), up, down, hl, J);
            break;
        case kResDecimate3:
            if (st) AID_RS_LAUNCH((k_decimate<true, 3, 61, T>), hl);
            else AID_RS_LAUNCH((k_decimate<false, 3, 61, T>), hl);
            break;
        case kResUniform:
            if (st) AID_RS_LAUNCH((k_resample<true, 2, T>), up, down, hl, J);
            else AID_RS_LAUNCH((k_resample<false, 2, T>), up, down, hl, J);
            break;
        case kResGlobalTaps:
            if (st) AID_RS_LAUNCH((k_resample<true, 0, T>), up, down, hl, J);
            else AID_RS_LAUNCH((k_resample<false, 0, T>), up, down, hl, J);
            break;
        default: break;
    }
#undef AID_RS_LAUNCH
}

// src / hist: float samples, or int16 with s16 (strides then count int16)
void launch_resample(const void *src, bool s16, int64_t in_base, int64_t n, int channels, int up, int down, int hl, int J,
                     const float *taps, float *dst, int64_t m_first, int64_t count, hipStream_t s, int n_streams,
                     int64_t src_stride, int64_t dst_stride, const void *hist, int64_t hist_n, int64_t hist_stride) {
    if (s16)
        launch_resample_t(static_cast<const int16_t *>(src), in_base, n, channels, up, down, hl, J, taps, dst, m_first,
                          count, s, n_streams, src_stride, dst_stride, static_cast<const int16_t *>(hist), hist_n,
                          hist_stride);
    else
        launch_resample_t(static_cast<const float *>(src), in_base, n, channels, up, down, hl, J, taps, dst, m_first,
                          count, s, n_streams, src_stride, dst_stride, static_cast<const float *>(hist), hist_n,
                          hist_stride);
}

// n mono s16 samples -> float (aid_resample_s16 at equal rates, mono: the float sibling's copy)
__global__ __launch_bounds__(256) void k_s16_to_f32(const int16_t *__restrict__ src, int64_t n, float *__restrict__ dst) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = s16_val(src[i]);
}

void launch_s16_to_f32(const int16_t *src, int64_t n, float *dst, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_s16_to_f32, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 65535)), dim3(256), 0, s, src, n,
                       dst);
}

// K6s `resample_speeds` (FPSPEC 8.2): every (clip, speed, output block) of a clip group in ONE launch. A workgroup
// finds its pair (clip * n_speeds + v) in the block-id prefix sums (uniform: scalar loads and a scalar search), reads
// that speed's (up, down, hl, J, taps) from the device table, stages its input window once (stage_window: float or
// s16, mono or stereo, the clip at any sample offset) and runs k_resample's fma chain, taps j = 0 .. J-1 in order, so
// an output equals the single-pair kernels' bit for bit. Blocks are kSpeedBlock consecutive outputs of one pair, the
// taps read from L1/L2 (the 41 tables of a 2 per mille grid are ~40 KB each; neighbouring workgroups share a speed).
static_assert(kSpeedBlock == kResBlock, "K6s blocks are k_resample's");

template <bool STEREO, typename T>
__global__ __launch_bounds__(kResThreads) void k_resample_speeds(const T *__restrict__ src,
                                                                 const int64_t *__restrict__ clip_off,
                                                                 const SpeedVarDev *__restrict__ vars, int n_speeds,
                                                                 const int64_t *__restrict__ blk_first,
                                                                 const int64_t *__restrict__ dst_off, int pair0,
                                                                 int n_pairs, float *__restrict__ dst) {
    // pairs [pair0, pair0 + n_pairs) (whole clips); block blockIdx.x of them; dst[0] = the first output of pair0
    extern __shared__ float sx[];
    const int tid = threadIdx.x;
    const int64_t b = blk_first[pair0] + blockIdx.x;
    const int pair = pair0 + speed_find_pair(blk_first + pair0, n_pairs, b);
    const int clip = pair / n_speeds;
    const SpeedVarDev v = vars[pair - clip * n_speeds];
    const T *x = src + clip_off[clip] * (STEREO ? 2 : 1);
    const ResInT<T> in{x, 0, 0, 0, x, 0, clip_off[clip + 1] - clip_off[clip], 0};
    const int64_t m_end = dst_off[pair + 1] - dst_off[pair];
    float *__restrict__ out = dst + (dst_off[pair] - dst_off[pair0]);
    const int up = v.up, down = v.down, hl = v.hl, J = v.J;
    const int64_t m0 = (b - blk_first[pair]) * kResBlock;
    const int64_t mlast = min(m0 + kResBlock - 1, m_end - 1);
    const int64_t c0 = m0 * down + hl, q0 = c0 / up;
    const int r0 = (int)(c0 - q0 * up);
    const int64_t lo = q0 - (J - 1);
    const int cnt = (int)((mlast * down + hl) / up - lo + 1);
    stage_window<STEREO>(in, lo, cnt, sx, tid, kResThreads);
    __syncthreads();
    // output m0 + i: c = c0 + i * down; in 32 bits when r0 + 1023 * down fits (every rate pair but the extreme ones)
    const bool small = (int64_t)kResBlock * down + up < 0x7FFFFFFF;
#pragma unroll
    for (int r = 0; r < kResPerThread; ++r) {
        const int i = tid + r * kResThreads;
        if (m0 + i >= m_end) break;
        int p, q;  // phase, input index - q0
        if (small) {
            const uint32_t t = (uint32_t)r0 + (uint32_t)i * (uint32_t)down;
            q = (int)(t / (uint32_t)up);
            p = (int)(t - (uint32_t)q * (uint32_t)up);
        } else {
            const int64_t t = r0 + (int64_t)i * down;
            q = (int)(t / up);
            p = (int)(t - (int64_t)q * up);
        }
        const float *xp = sx + (q + J - 1);  // the input at c / up (window index c / up - lo)
        float acc;
        if (v.copy) {
            acc = xp[-hl];  // up == down == 1: c = m + hl
        } else {
            acc = 0.0f;
            const float *tp = v.taps + (int64_t)p * J;
            for (int j = 0; j < J; ++j) acc = __builtin_fmaf(tp[j], xp[-j], acc);
        }
        out[m0 + i] = acc;
    }
}

void launch_resample_speeds(const void *src, bool s16, int channels, const int64_t *clip_off, const SpeedVarDev *vars,
                            int n_speeds, const int64_t *blk_first, const int64_t *dst_off, int pair0, int n_pairs,
                            int64_t blocks, int64_t lds_floats, float *dst, hipStream_t s) {
    if (blocks <= 0 || n_pairs <= 0) return;
    const dim3 g((unsigned)blocks), b(kResThreads);
    const size_t lds = (size_t)lds_floats * sizeof(float);
#define AID_RS_SPEEDS(ST, T) \
    hipLaunchKernelGGL((k_resample_speeds<ST, T>), g, b, lds, s, static_cast<const T *>(src), clip_off, vars, n_speeds, \
                       blk_first, dst_off, pair0, n_pairs, dst)
    if (s16) {
        if (channels == 2) AID_RS_SPEEDS(true, int16_t); else AID_RS_SPEEDS(false, int16_t);
    } else {
        if (channels == 2) AID_RS_SPEEDS(true, float); else AID_RS_SPEEDS(false, float);
    }
#undef AID_RS_SPEEDS
}

}  // namespace aid
