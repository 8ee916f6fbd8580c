// mel.hip -- K10 `k_logmel`: the CLAP log-mel front end (spec/FPSPEC.md 10). Per 10 s chunk of 48 kHz PCM the
// [1001][64] log-mel image the reference gets from ClapFeatureExtractor (transformers.audio_utils.spectrogram, one
// float64 rfft per frame on the host), written where a device model reads it.
//
// Work mapping (gfx950, wave64):
//   * one workgroup (4 waves) takes a run of kMelRun = 4 consecutive frames of one chunk, one frame per wave. It
//     stages the run's 3 * 480 + 1024 samples into LDS once; centre reflection, repetition and zero fill are index arithmetic at
//     staging, and the only global loads are x[src + j], j < r, of the chunk's own clip;
//   * each wave transforms whole frames (frame f of the run goes to wave f & 3). Lane l holds 8 complex values:
//     window on the way out of LDS, then 512 = 8 * 8 * 8 as three DFT8 passes in registers with two transposes
//     through the wave's own LDS buffer (rows padded to 72 and 9 float2 against bank conflicts); the window and
//     the stage twiddles depend on the lane only and stay in registers for all of the wave's frames;
//   * the real split runs for bins < K only and leaves the power row in LDS; lane m then owns band m: the fma chain
//     over its support (weights band-compact [j][m], one coalesced row per step, read through L1), floor, dB;
//   * the wave stores the frame's 64 floats as one 256-byte row. No atomics, nothing crosses a workgroup.
// The exchanges are wave-private, so the only workgroup barrier is the one after staging.
// Run length and workgroup size were swept on the card (profiles/logmel_ab.txt): 4 waves x 4 frames is the fastest of
// 4 x {16, 8, 4}, 2 x {4, 2} and 1 x {2, 1}; longer runs stage less per frame but keep the waves idle at the barrier.
// Unlike K1, this file is faster with hipcc's SLP vectorizer left on (+1.3 % without it).
#include "aidfp_device.h"
#include "aidfp_launch.h"
#include "aidfp_mel.h"

namespace aid {

namespace {

#ifndef AID_MEL_WAVES  // diagnostic builds try other workgroup sizes
#define AID_MEL_WAVES 4
#endif
constexpr int kMelWaves = AID_MEL_WAVES;
constexpr int kMelExRow = 72;                // float2 per row of the exchange buffer (64 + 8 of padding)
constexpr int kMelEx = 8 * kMelExRow;        // 576 float2 per wave
static_assert(7 * kMelExRow + 7 * 9 + 7 < kMelEx, "E2 layout exceeds the wave's exchange buffer");
static_assert(kMelRun % kMelWaves == 0, "a run splits evenly over the waves");
static_assert(kMelHop % 2 == 0, "a frame's first sample pair must be 8-byte aligned in LDS");

__device__ __forceinline__ float mel_load(const float *p) { return *p; }
__device__ __forceinline__ float mel_load(const int16_t *p) { return (float)*p * 0x1p-15f; }  // FPSPEC 8.1

// FPSPEC 10 "dB": 10 log10(M) of a normal positive M
__device__ __forceinline__ float mel_db10(float M) {
    const uint32_t b = __float_as_uint(M);
    int e = (int)(b >> 23) - 127;
    float m = __uint_as_float((b & 0x7FFFFFu) | 0x3F800000u);
    if (m >= 0x1.6a09e6p+0f) {
        m *= 0.5f;
        e += 1;
    }
    const float f = m - 1.0f, ef = (float)e;
    float q = 0x1.24486ep-2f;
    q = __builtin_fmaf(q, f, -0x1.026534p-1f);
    q = __builtin_fmaf(q, f, 0x1.09a088p-1f);
    q = __builtin_fmaf(q, f, -0x1.143018p-1f);
    q = __builtin_fmaf(q, f, 0x1.3c05d4p-1f);
    q = __builtin_fmaf(q, f, -0x1.729872p-1f);
    q = __builtin_fmaf(q, f, 0x1.bcc62p-1f);
    q = __builtin_fmaf(q, f, -0x1.15f2fcp+0f);
    q = __builtin_fmaf(q, f, 0x1.7298fep+0f);
    q = __builtin_fmaf(q, f, -0x1.15f2cep+1f);
    q = __builtin_fmaf(q, f, 0x1.15f2cep+2f);
    float t = f * q;
    t = __builtin_fmaf(ef, -0x1.f6ce2ap-17f, t);
    return __builtin_fmaf(ef, 0x1.8152p+1f, t);
}

// slot of Z[k] in the wave's buffer after stage C: rows of 64 padded to kMelExRow
__device__ __forceinline__ int zslot(int k) { return k + (kMelExRow - 64) * (k >> 6); }

template <typename T>
__global__ __launch_bounds__(kMelWaves * 64) void k_logmel(const T *__restrict__ pcm, const MelChunkDev *__restrict__ chunks,
                                                         int64_t chunk0, const MelTables *__restrict__ tab,
                                                         const float *__restrict__ wc, float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) float s_x[kMelStage];
    __shared__ __attribute__((aligned(16))) float2 s_ex[kMelWaves][kMelEx];
    __shared__ float s_p[kMelWaves][kMelMaxK];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t chunk = chunk0 + blockIdx.x / kMelRuns;
    const int run = blockIdx.x % kMelRuns;
    const int t0 = run * kMelRun;
    const int nfr = min(kMelRun, kMelFrames - t0);
    const MelChunkDev c = chunks[chunk];
    const T *x = pcm + c.src;

    // staging: sample i of the run is u[480 t0 - 512 + i]; every load is x[j], 0 <= j < r
    const int n_stage = (nfr - 1) * kMelHop + kMelN;
    for (int i = threadIdx.x; i < n_stage; i += kMelWaves * 64) {
        int p = kMelHop * t0 - kMelN / 2 + i;
        p = p < 0 ? -p : p;
        p = p >= kMelWindow ? 2 * (kMelWindow - 1) - p : p;
        float v = 0.f;
        if (p < c.fill) {
            const int j = p < c.r ? p : p % c.r;
            v = mel_load(x + j);
        }
        s_x[i] = v;
    }

    // per-lane constants of all frames: window pairs, stage-A twiddles T512[n2 k1] (n2 = lane), stage-B twiddles
    // T64[m2 j1] (m2 = lane & 7)
    const int kq = lane >> 3, lq = lane & 7;
    float2 wv[8], ta[8], tb[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        wv[i] = tab->win2[64 * i + lane];
        ta[i] = tab->t512[lane * i];
        tb[i] = tab->t64[lq * i];
    }
    const float2 w1 = tab->t8[1], w3 = tab->t8[3];
    const int K = tab->K, max_len = tab->max_len;
    const int lo = tab->lo[lane], len = tab->len[lane];
    float2 *buf = s_ex[wave];
    float *prow = s_p[wave];
    __syncthreads();

    for (int f = wave; f < nfr; f += kMelWaves) {  // wave-uniform
        float2 v[8];
        const float2 *xs = reinterpret_cast<const float2 *>(s_x + kMelHop * f);
        // stage A: lane = n2, register = n1
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float2 s = xs[64 * i + lane];
            v[i] = make_float2(s.x * wv[i].x, s.y * wv[i].y);
        }
        dft8(v, w1, w3);
        // lane 0 multiplies by T512[0] = (1, -0): value-identical up to the sign of a zero (FPSPEC 4 note)
#pragma unroll
        for (int i = 1; i < 8; ++i) v[i] = cmul(v[i], ta[i]);
        // E1: A[k1][n2] -> lane (kq = k1, lq = m2) gets A[k1][8 m1 + m2] in register m1
#pragma unroll
        for (int i = 0; i < 8; ++i) buf[kMelExRow * i + lane] = v[i];
        wave_lds_sync();
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = buf[kMelExRow * kq + 8 * i + lq];
        wave_lds_sync();
        // stage B: register = j1
        dft8(v, w1, w3);
#pragma unroll
        for (int i = 1; i < 8; ++i) v[i] = cmul(v[i], tb[i]);
        // E2: B[k1][m2][j1] -> lane (kq = k1, lq = j1) gets it in register m2
#pragma unroll
        for (int i = 0; i < 8; ++i) buf[kMelExRow * kq + 9 * i + lq] = v[i];
        wave_lds_sync();
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = buf[kMelExRow * kq + 9 * lq + i];
        wave_lds_sync();
        // stage C: register j2 = Z[k1 + 8 j1 + 64 j2]
        dft8(v, w1, w3);
#pragma unroll
        for (int i = 0; i < 8; ++i) buf[kMelExRow * i + kq + 8 * lq] = v[i];
        wave_lds_sync();
        // real split, bins < K only
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = lane + 64 * i;
            if (64 * i < K) {  // wave-uniform
                if (k < K) {
                    const float2 a = buf[zslot(k)], b = buf[zslot((512 - k) & 511)];
                    const float er = a.x + b.x, ei = a.y - b.y, orr = a.y + b.y, oi = b.x - a.x;
                    const float2 tw = cmul(make_float2(orr, oi), tab->t1k[k]);
                    const float xr = er + tw.x, xi = ei + tw.y;
                    prow[k] = __builtin_fmaf(xr, xr, xi * xi) * 0.25f;
                }
            }
        }
        wave_lds_sync();
        // band = lane: the ascending chain over its support
        float acc = 0.f;
        for (int j = 0; j < max_len; ++j) {
            if (j < len) acc = __builtin_fmaf(wc[(size_t)j * kMelBands + lane], prow[lo + j], acc);
        }
        const float M = fmaxf(acc, 1e-10f);
        out[((chunk - chunk0) * kMelFrames + t0 + f) * kMelBands + lane] = mel_db10(M);
        wave_lds_sync();
    }
}

}  // namespace

// chunks [chunk0, chunk0 + n) of the device chunk table; out = the row of chunk chunk0
void launch_logmel(const void *pcm, bool s16, const MelChunkDev *chunks, int64_t chunk0, int64_t n, const MelTables *tab,
                   const float *wc, float *out, hipStream_t s) {
    if (n <= 0) return;
    const dim3 g((unsigned)mel_grid(n)), b(kMelWaves * 64);
    if (s16)
        timed_launch(k_logmel<int16_t>, g, b, 0, s, static_cast<const int16_t *>(pcm), chunks, chunk0, tab, wc, out);
    else
        timed_launch(k_logmel<float>, g, b, 0, s, static_cast<const float *>(pcm), chunks, chunk0, tab, wc, out);
}

}  // namespace aid
