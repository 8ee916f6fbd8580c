// chroma.hip -- K11: the content fingerprint (spec/FPSPEC.md 11), the engine's counterpart of the reference's
// `fpcalc -raw` subprocess (app/audio/dedup.py:53-124) in the raw-Chromaprint form K7 scans: 32-bit words from
// 11025 Hz mono PCM. Parity with fpcalc itself is unpinned (FPSPEC 11); the spec is the engine's own.
//
// K11a `k_chroma_rows`, PCM -> C[frames][12] (gfx950, wave64):
//   * one workgroup takes a run of kChromaRun consecutive frames of one clip (aidfp_chroma_plan.h ChromaRowBlock),
//     one frame per wave at a time. It stages the run's (R - 1) * 1365 + 4096 samples into LDS once (frames overlap
//     3x), sample by sample: the hop is odd and s16 clips start at any 2-byte offset, so neither the global reads
//     nor a frame's start in LDS are ever assumed wider than one sample;
//   * a wave transforms a whole frame: 2048 = 16 * 16 * 8 as two DFT16 passes and one DFT8 pass with two exchanges
//     through the wave's own LDS buffer. Stage A and B run in two halves of 64 columns each (16 complex values in
//     registers), stage B in place (a half rewrites only the rows it has read); stage C reads all of its 32 values
//     before it writes Z, which lands all over the buffer. Rows are padded (136 for 128, 17 for 16) against bank
//     conflicts;
//   * the real split runs for bins 10..1307 only; run r of the note table goes to lane r mod 64 (the 19 long runs
//     at the top share a lane with the 19 shortest), then lane c < 12 adds the runs of note c in bin order and
//     stores its float: 48 bytes per frame. No atomics, nothing crosses a workgroup.
// The exchanges are wave-private, so the only workgroup barrier is the one after staging.
// Run length and workgroup size were swept on the card (profiles/chroma_ab.txt): 2 waves x 4 frames is the fastest of
// 4 x {8, 4, 2}, 3 x {6, 3}, 2 x {8, 6, 4, 2} and 1 x {2, 1}. A wave's exchange buffer and power row cost 22.6 KB of
// LDS, so no shape has more than one wave per SIMD; two 2-wave workgroups fit a CU.
//
// K11b `k_chroma_words`, C -> words: a workgroup takes up to 240 consecutive words of one clip
// (ChromaItemBlock), stages their 259 rows of C, thread i smooths and normalises row i into LDS (F, rows padded to
// 13), then thread i evaluates the 16 classifiers of word i over F[i .. i + 16). With raw features the staged rows
// are F themselves. A block never reads a row of another clip: the host cuts blocks per clip.
#include "aidfp_chroma.h"
#include "aidfp_device.h"
#include "aidfp_launch.h"

namespace aid {

namespace {

#ifndef AID_CHROMA_WAVES  // diagnostic builds try other workgroup sizes
#define AID_CHROMA_WAVES 2
#endif
constexpr int kChromaWaves = AID_CHROMA_WAVES;
constexpr int kChromaExRow = 136;              // float2 per row of the exchange buffer (128 + 8 of padding)
constexpr int kChromaEx = 16 * kChromaExRow;   // 2176 float2 per wave
constexpr int kChromaFRow = kChromaBands + 1;  // floats per row of F in LDS
static_assert(7 * 17 + 15 < kChromaExRow, "stage B's layout exceeds a row of the exchange buffer");
static_assert(2047 + (2047 >> 4) < kChromaEx, "Z's layout exceeds the wave's exchange buffer");
static_assert(kChromaItems + kChromaItem - 1 <= 256, "one thread per row of F");

__device__ __forceinline__ float chroma_load(const float *p) { return *p; }
__device__ __forceinline__ float chroma_load(const int16_t *p) { return (float)*p * 0x1p-15f; }  // FPSPEC 8.1

// slot of Z[k] in the wave's buffer after stage C: 16 values, then one slot of padding
__device__ __forceinline__ int zslot(int k) { return k + (k >> 4); }

template <typename T>
__global__ __launch_bounds__(kChromaWaves * 64) void k_chroma_rows(const T *__restrict__ pcm,
                                                                   const ChromaRowBlock *__restrict__ blocks,
                                                                   int64_t block0, const ChromaTables *__restrict__ tab,
                                                                   float *__restrict__ rows) {
    __shared__ float s_x[kChromaStage];
    __shared__ __attribute__((aligned(16))) float2 s_ex[kChromaWaves][kChromaEx];
    __shared__ float s_p[kChromaWaves][kChromaBins];
    __shared__ float s_run[kChromaWaves][kChromaMaxRuns];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const ChromaRowBlock blk = blocks[block0 + blockIdx.x];
    const T *x = pcm + blk.src;

    // staging: sample i of the run is x[i]; the last one is the last sample of the run's last frame
    const int n_stage = (blk.nfr - 1) * kChromaHop + kChromaN;
    for (int i = threadIdx.x; i < n_stage; i += kChromaWaves * 64) s_x[i] = chroma_load(x + i);

    float2 t16[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) t16[i] = tab->t16[i];
    const float2 w1 = tab->t8[1], w3 = tab->t8[3];
    const int n_runs = tab->n_runs;
    float2 *buf = s_ex[wave];
    float *prow = s_p[wave];
    float *srun = s_run[wave];
    __syncthreads();

    for (int f = wave; f < blk.nfr; f += kChromaWaves) {  // wave-uniform
        const float *xs = s_x + kChromaHop * f;
        // stage A: column n2 = lane + 64 h, register = n1 -> k1
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
            const int n2 = lane + 64 * h;
            float2 v[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int m = 128 * i + n2;
                const float2 w = tab->win2[m];
                v[i] = make_float2(xs[2 * m] * w.x, xs[2 * m + 1] * w.y);
            }
            dft16(v, t16);
            // column 0 multiplies by T2048[0] = (1, -0): value-identical up to the sign of a zero (FPSPEC 4 note)
#pragma unroll
            for (int i = 1; i < 16; ++i) v[i] = cmul(v[i], tab->t2048[n2 * i]);
#pragma unroll
            for (int i = 0; i < 16; ++i) buf[kChromaExRow * i + n2] = v[i];
        }
        wave_lds_sync();
        // stage B: pair (k1, m2) = lane + 64 h, register = m1 -> j1; rows [8 h, 8 h + 8) are rewritten in place
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
            const int k1 = (lane >> 3) + 8 * h, m2 = lane & 7;
            float2 v[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) v[i] = buf[kChromaExRow * k1 + 8 * i + m2];
            wave_lds_sync();
            dft16(v, t16);
#pragma unroll
            for (int i = 1; i < 16; ++i) v[i] = cmul(v[i], tab->t128[m2 * i]);
#pragma unroll
            for (int i = 0; i < 16; ++i) buf[kChromaExRow * k1 + 17 * m2 + i] = v[i];
            wave_lds_sync();
        }
        // stage C: pair (k1, j1) = lane + 64 g, register = m2 -> j2 = Z[k1 + 16 j1 + 256 j2]
        float2 c[4][8];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int k1 = (lane >> 4) + 4 * g, j1 = lane & 15;
#pragma unroll
            for (int i = 0; i < 8; ++i) c[g][i] = buf[kChromaExRow * k1 + 17 * i + j1];
        }
        wave_lds_sync();
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int k1 = (lane >> 4) + 4 * g, j1 = lane & 15;
            dft8(c[g], w1, w3);
#pragma unroll
            for (int i = 0; i < 8; ++i) buf[zslot(k1 + 16 * j1 + 256 * i)] = c[g][i];
        }
        wave_lds_sync();
        // real split, bins [10, 1308) only
        for (int k = kChromaBinLo + lane; k < kChromaBinHi; k += 64) {
            const float2 a = buf[zslot(k)], b = buf[zslot(2048 - k)];
            const float er = a.x + b.x, ei = a.y - b.y, orr = a.y + b.y, oi = b.x - a.x;
            const float2 tw = cmul(make_float2(orr, oi), tab->t4096[k]);
            const float xr = er + tw.x, xi = ei + tw.y;
            prow[k - kChromaBinLo] = __builtin_fmaf(xr, xr, xi * xi) * 0.25f;
        }
        wave_lds_sync();
        // run sums in ascending bin order, then lane c adds the runs of note c in bin order
        for (int r = lane; r < n_runs; r += 64) {
            const int lo = tab->run_lo[r] - kChromaBinLo, len = tab->run_len[r];
            float s = 0.f;
            for (int j = 0; j < len; ++j) s = s + prow[lo + j];
            srun[r] = s;
        }
        wave_lds_sync();
        if (lane < kChromaBands) {
            float acc = 0.f;
            for (int r = 0; r < n_runs; ++r)
                if (tab->run_note[r] == lane) acc = acc + srun[r];
            rows[(blk.row + f) * kChromaBands + lane] = acc;
        }
        wave_lds_sync();
    }
}

__device__ __forceinline__ float chroma_area(const float *F, const ChromaRect &r) {
    float s = 0.f;
    for (int x = r.x0; x < r.x1; ++x)
        for (int y = r.y0; y < r.y1; ++y) s = s + F[x * kChromaFRow + y];
    return s;
}

__global__ __launch_bounds__(256) void k_chroma_words(const float *__restrict__ rows,
                                                      const ChromaItemBlock *__restrict__ blocks, int64_t block0,
                                                      const ChromaTables *__restrict__ tab, int raw,
                                                      uint32_t *__restrict__ words) {
    __shared__ float s_c[(kChromaItems + kChromaItemRows - 1) * kChromaBands];
    __shared__ float s_f[(kChromaItems + kChromaItem - 1) * kChromaFRow];
    const ChromaItemBlock blk = blocks[block0 + blockIdx.x];
    const int tid = threadIdx.x;
    const int n_f = blk.n + kChromaItem - 1;                    // rows of F the block's words read
    const int n_c = raw ? n_f : blk.n + kChromaItemRows - 1;    // rows it stages
    const float *src = rows + blk.row * kChromaBands;
    for (int i = tid; i < n_c * kChromaBands; i += 256) s_c[i] = src[i];
    __syncthreads();
    if (tid < n_f) {
        const float *C = s_c + tid * kChromaBands;
        float g[kChromaBands];
        if (raw) {
#pragma unroll
            for (int c = 0; c < kChromaBands; ++c) g[c] = C[c];
        } else {
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < kChromaBands; ++c) {
                float v = 0.25f * C[c];
                v = __builtin_fmaf(0.75f, C[kChromaBands + c], v);
                v = __builtin_fmaf(1.0f, C[2 * kChromaBands + c], v);
                v = __builtin_fmaf(0.75f, C[3 * kChromaBands + c], v);
                v = __builtin_fmaf(0.25f, C[4 * kChromaBands + c], v);
                g[c] = v;
            }
#pragma unroll
            for (int c = 0; c < kChromaBands; ++c) s = __builtin_fmaf(g[c], g[c], s);
            const float r = __builtin_sqrtf(s);
#pragma unroll
            for (int c = 0; c < kChromaBands; ++c) g[c] = r < 0.01f ? 0.f : g[c] / r;
        }
#pragma unroll
        for (int c = 0; c < kChromaBands; ++c) s_f[tid * kChromaFRow + c] = g[c];
    }
    __syncthreads();
    if (tid < blk.n) {
        const float *F = s_f + tid * kChromaFRow;
        uint32_t v = 0;
        for (int j = 0; j < kChromaClassifiers; ++j) {  // uniform: the table is read through the scalar cache
            const ChromaClassifier &cl = tab->cls[j];
            float a = chroma_area(F, cl.a[0]);
            if (cl.na == 2) a = a + chroma_area(F, cl.a[1]);
            float b = 0.f;
            if (cl.nb >= 1) b = chroma_area(F, cl.b[0]);
            if (cl.nb == 2) b = b + chroma_area(F, cl.b[1]);
            const float A = 1.0f + a, B = 1.0f + b;
            const int q = (A >= cl.E[0] * B) + (A >= cl.E[1] * B) + (A >= cl.E[2] * B);
            v = (v << 2) | (uint32_t)(q ^ (q >> 1));  // GRAY = {0, 1, 3, 2}
        }
        words[blk.word + tid] = v;
    }
}

}  // namespace

// blocks [block0, block0 + n) of the device block list
void launch_chroma_rows(const void *pcm, bool s16, const ChromaRowBlock *blocks, int64_t block0, int64_t n,
                        const ChromaTables *tab, float *rows, hipStream_t s) {
    if (n <= 0) return;
    const dim3 g((unsigned)n), b(kChromaWaves * 64);
    if (s16)
        hipLaunchKernelGGL(k_chroma_rows<int16_t>, g, b, 0, s, static_cast<const int16_t *>(pcm), blocks, block0, tab, rows);
    else
        hipLaunchKernelGGL(k_chroma_rows<float>, g, b, 0, s, static_cast<const float *>(pcm), blocks, block0, tab, rows);
}

void launch_chroma_words(const float *rows, const ChromaItemBlock *blocks, int64_t block0, int64_t n,
                         const ChromaTables *tab, bool raw, uint32_t *words, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_chroma_words, dim3((unsigned)n), dim3(256), 0, s, rows, blocks, block0, tab, raw ? 1 : 0, words);
}

}  // namespace aid
