// vector_q8.hip -- K9q, the int8 prefilter of the vector lane (spec/FPSPEC.md 9.1). The catalog keeps an int8 copy
// of its unit vectors (a quarter of the bytes), a query batch is scored against that copy on
// v_mfma_i32_32x32x32_i8, and the few entries that the proven bound eps cannot rule out are rescored with FPSPEC 9's
// binary32 chain. The hit lists stay FPSPEC 9's, bit for bit; the host side of the route is in csrc/vector.hip.
//
//   k_vec_quantize   rows of the tiled f32 layout -> int8 rows (aidfp_vector_q8.h), scale s and residual e
//   k_vec_scan_i8    approximate scores of a 32-query tile against the int8 catalog, k_vec_scan_mfma's shape
//   k_vec_rescore    FPSPEC 9 scores of listed (query, entry) pairs, the chain of k_vec_scan_valu out of LDS
//   k_vec_tau        tau of the rescored first-stage candidates and the per-query threshold key of the filter
//   k_vec_filter_q8  k_vec_filter with one counter line per query
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aidfp_vector.h"
#include "aidfp_vector_keys.h"

namespace aid {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

// FPSPEC 9.1 quantisation of row row0 + blockIdx.x, one wave per row. Lane u quantises the 16 values of k-step
// u >> 1, half u & 1 and stores them with one 16-byte store; the squared residuals go through LDS to lane 0, which
// adds them in k order (the chain is the spec's; only its terms are computed in parallel).
__global__ __launch_bounds__(64) void k_vec_quantize(const float *__restrict__ src, int64_t row0, int dim,
                                                     int8_t *__restrict__ dst, float *__restrict__ s_out,
                                                     float *__restrict__ e_out) {
    __shared__ float sy[1024];
    __shared__ double sd[1024];
    const int64_t row = row0 + blockIdx.x;
    const int lane = threadIdx.x;
    const float *tile = src + (size_t)(row >> 5) * 32 * dim + (size_t)(row & 31) * 4;
    float m = 0.0f;
    for (int k = lane; k < dim; k += 64) {
        const float y = tile[(size_t)((k >> 3) * 2 + (k & 1)) * 128 + ((k & 7) >> 1)];
        sy[k] = y;
        m = fmaxf(m, fabsf(y));
    }
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    __syncthreads();
    const float s = m / 127.0f;
    if (lane < (dim >> 4)) {
        const int k0 = lane * 16;
        int w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float y = sy[k0 + j];
            int i = 0;
            if (m > 0.0f) i = min(127, max(-127, (int)rintf(y / s)));
            const double d = (double)y - (double)s * (double)i;
            sd[k0 + j] = d * d;
            w[j >> 2] |= (i & 0xFF) << (8 * (j & 3));
        }
        i32x4 v;
        v.x = w[0];
        v.y = w[1];
        v.z = w[2];
        v.w = w[3];
        *reinterpret_cast<i32x4 *>(dst + vec_q8_layout_index(row, k0, dim)) = v;
    }
    __syncthreads();
    if (lane == 0) {
        double r2 = 0.0;
        for (int k = 0; k < dim; ++k) r2 += sd[k];
        s_out[row] = s;
        e_out[row] = (float)sqrt(r2);
    }
}

// One workgroup: `tiles_per_wg` int8 catalog tiles against one tile of 32 int8 queries staged in LDS; wave w takes
// tiles w, w + NT / 64, ... of the chunk, as in k_vec_scan_mfma. A = queries (rows), B = catalog (columns). One
// k-step is one 16-byte load per lane (1 KB per wave) and one MFMA; a wave walks its (tile, k-step) sequence with
// four loads in flight, each issued before the MFMA of the step whose register it takes over. The integer sums are
// exact, so the accumulation order is free; the epilogue applies t = s_q * s_c and approx = (float)idot * t.
template <int NT>
__global__ __launch_bounds__(NT) void k_vec_scan_i8(const int8_t *__restrict__ cat, const float *__restrict__ cat_s,
                                                    int64_t n_tiles, int tiles_per_wg, const int8_t *__restrict__ q,
                                                    const float *__restrict__ q_s, int dim,
                                                    float *__restrict__ scores, int64_t ns) {
    extern __shared__ i32x4 sq[];  // [dim / 32][64], then the 32 query scales
    const int S = dim >> 5;        // k-steps per tile
    float *sqs = reinterpret_cast<float *>(sq + S * 64);
    const int qt0 = blockIdx.y;
    const i32x4 *qsrc = reinterpret_cast<const i32x4 *>(q) + (size_t)qt0 * S * 64;
    for (int i = threadIdx.x; i < S * 64; i += NT) sq[i] = qsrc[i];
    if (threadIdx.x < 32) sqs[threadIdx.x] = q_s[qt0 * 32 + threadIdx.x];
    __syncthreads();
    constexpr int NW = NT / 64;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t t1 = min((int64_t)(blockIdx.x + 1) * tiles_per_wg, n_tiles);
    int64_t t = (int64_t)blockIdx.x * tiles_per_wg + wave;
    if (t >= t1) return;
    const int64_t total = (t1 - t + NW - 1) / NW * S;  // k-steps of this wave
    const i32x4 *cat4 = reinterpret_cast<const i32x4 *>(cat) + lane;
    int64_t lt = t, issued = 0;  // the load cursor: tile, k-step, count
    int lst = 0;
    i32x4 buf[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        buf[u] = i32x4{0, 0, 0, 0};
        if (issued < total) {
            buf[u] = cat4[((size_t)lt * S + lst) * 64];
            ++issued;
            if (++lst == S) {
                lst = 0;
                lt += NW;
            }
        }
    }
    i32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0;
    int st = 0;
    for (int64_t base = 0; base < total; base += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (base + u >= total) break;
            const i32x4 cur = buf[u];
            if (issued < total) {
                buf[u] = cat4[((size_t)lt * S + lst) * 64];
                ++issued;
                if (++lst == S) {
                    lst = 0;
                    lt += NW;
                }
            }
            const i32x4 qv = sq[st * 64 + lane];
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(qv, cur, acc, 0, 0, 0);
            if (++st == S) {  // the tile's sums are complete
                const float sc = cat_s[t * 32 + (lane & 31)];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int qr = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    const float tt = sqs[qr] * sc;
                    scores[(size_t)(qt0 * 32 + qr) * ns + t * 32 + (lane & 31)] = (float)acc[r] * tt;
                    acc[r] = 0;
                }
                st = 0;
                t += NW;
            }
        }
    }
}

// The FPSPEC 9 score of every listed pair: keys[q][i] (0 = none) names an entry, and the key comes back with the
// score in place of whatever ordered the list before. Only lists whose count (cnt[q * kVecQ8CntStride]) is at most
// cnt_cap are touched, their first `count` keys; without cnt, the first n_max keys of every list.
// A workgroup takes kVecRescorePairs pairs of one query. An entry's row is 16-byte pieces 512 bytes apart inside one
// 64 KB tile, and the listed entries lie anywhere in the catalog, so the rows are fetched one per half wave-load
// (64 lanes, 64 pieces of one row: one page) with all of a thread's loads in flight together, and transposed
// through LDS ([k][pair], padded to 33: the chain's reads are conflict-free). Lane p of the first wave then runs pair
// p's chain: k ascending into one accumulator from +0, the chain of k_vec_scan_valu and so its bits.
constexpr int kVecRescorePairs = 32;
__global__ __launch_bounds__(256) void k_vec_rescore(const float *__restrict__ cat, const float *__restrict__ q, int dim,
                                                     unsigned long long *__restrict__ keys, int64_t stride, int n_max,
                                                     const int32_t *__restrict__ cnt, int cnt_cap) {
    extern __shared__ float sc[];  // [dim][kVecRescorePairs + 1], then the query [dim] in k order
    __shared__ uint32_t s_e[kVecRescorePairs];
    constexpr int P = kVecRescorePairs, PS = kVecRescorePairs + 1;
    const int qi = blockIdx.y;
    const int i0 = blockIdx.x * P;
    int have = n_max;
    if (cnt) {
        const int c = cnt[(size_t)qi * kVecQ8CntStride];
        if (c > cnt_cap) return;
        have = min(have, c);
    }
    if (i0 >= have) return;
    if (threadIdx.x < P) {
        const int i = i0 + threadIdx.x;
        const unsigned long long key = i < have ? keys[(size_t)qi * stride + i] : 0ull;
        s_e[threadIdx.x] = key ? vec_key_entry(key) : 0xFFFFFFFFu;
    }
    __syncthreads();
    const int F = dim >> 2;           // 16-byte pieces per row: 8 .. 256, so a wave's 64 pieces are of one row or of whole rows
    const int iters = P * F / 256;    // = dim / 32
    const float4 *cat4 = reinterpret_cast<const float4 *>(cat);
    float *sqv = sc + (size_t)dim * PS;
    for (int f = threadIdx.x; f < F; f += 256) {
        const float4 v = reinterpret_cast<const float4 *>(q)[((size_t)(qi >> 5) * F + f) * 32 + (qi & 31)];
        const int k0 = 8 * (f >> 1) + (f & 1);
        sqv[k0 + 0] = v.x;
        sqv[k0 + 2] = v.y;
        sqv[k0 + 4] = v.z;
        sqv[k0 + 6] = v.w;
    }
    for (int b = 0; b < iters; b += 4) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            v[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (b + u < iters) {
                const int idx = (b + u) * 256 + threadIdx.x;
                const uint32_t e = s_e[idx / F];
                if (e != 0xFFFFFFFFu) v[u] = cat4[((size_t)(e >> 5) * F + (idx % F)) * 32 + (e & 31)];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (b + u < iters) {
                const int idx = (b + u) * 256 + threadIdx.x;
                const int pr = idx / F, f = idx % F;
                const int k0 = 8 * (f >> 1) + (f & 1);  // the piece holds k0, k0 + 2, k0 + 4, k0 + 6
                sc[(k0 + 0) * PS + pr] = v[u].x;
                sc[(k0 + 2) * PS + pr] = v[u].y;
                sc[(k0 + 4) * PS + pr] = v[u].z;
                sc[(k0 + 6) * PS + pr] = v[u].w;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x >= P) return;
    const int pr = threadIdx.x;
    const uint32_t e = s_e[pr];
    if (e == 0xFFFFFFFFu) return;
    const float *c = sc + pr;
    float acc = 0.0f;
#pragma unroll 16
    for (int k = 0; k < dim; ++k) acc = __builtin_fmaf(sqv[k], c[k * PS], acc);
    keys[(size_t)qi * stride + i0 + pr] = vec_key(acc, e);
}

// k_vec_filter for the prefilter's two candidate lists, which are longer than the f32 route's (R and |W| against
// `limit`): the same test and the same keys, but query q counts in cnt[q * kVecQ8CntStride], a 128-byte line of its
// own, so the appends of different queries do not queue behind one another in one L2 line.
// M: which entries count, as in k_vec_filter (VecLive, or VecAllowed under a filter, FPSPEC 9.2).
template <typename M>
__global__ __launch_bounds__(256) void k_vec_filter_q8(const float *__restrict__ scores, int64_t ns, const M member,
                                                       int64_t n, const uint32_t *__restrict__ thr,
                                                       unsigned long long *__restrict__ cand, int cap,
                                                       int32_t *__restrict__ cnt) {
    const int q = blockIdx.y;
    const uint32_t t = thr[q];
    const auto mrow = member.row(q);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int64_t e = (int64_t)blockIdx.x * 2048 + j * 256 + threadIdx.x;
        if (e < n && M::test(mrow, e)) {
            const float s = scores[(size_t)q * ns + e];
            if (vec_score_key(s) >= t) {
                const int pos = atomicAdd(&cnt[(size_t)q * kVecQ8CntStride], 1);
                if (pos < cap) cand[(size_t)q * cap + pos] = vec_key(s, (uint32_t)e);
            }
        }
    }
}

// Query blockIdx.x: tau = the limit-th largest score of its R rescored keys, and the threshold of k_vec_filter.
// FPSPEC 9.1 admits an entry when (double)approx >= (double)tau - eps. approx is a binary32 number, so that holds
// exactly when approx >= the difference rounded toward +inf to binary32; k_vec_filter compares keys, which order
// as the numbers do, so the key of that float decides as the binary64 rule does. Fewer than `limit` keys: key 0,
// which every live entry reaches.
__global__ __launch_bounds__(256) void k_vec_tau(const unsigned long long *__restrict__ keys, int64_t stride, int R, int sp,
                                                 int limit, const float *__restrict__ q_e, float E, int dim,
                                                 uint32_t *__restrict__ thr, int32_t *__restrict__ cnt) {
    extern __shared__ unsigned long long sk[];  // [sp], sp = R rounded up to a power of two
    const int q = blockIdx.x;
    for (int i = threadIdx.x; i < sp; i += 256) sk[i] = i < R ? keys[(size_t)q * stride + i] : 0ull;
    __syncthreads();
    vec_sort_desc(sk, sp);
    if (threadIdx.x == 0) {
        const unsigned long long key = sk[limit - 1];  // limit <= R
        uint32_t t = 0;
        if (key != 0) {
            const double d = (double)vec_key_score(key) - vec_q8_eps(q_e[q], E, dim);
            t = vec_score_key(__double2float_ru(d));
        }
        thr[q] = t;
        cnt[(size_t)q * kVecQ8CntStride] = 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// launches (the callers check hipGetLastError)

void vec_q8_quantize(const float *tiled, int64_t row0, int64_t n, int dim, int8_t *dst, float *s_out, float *e_out,
                     hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_vec_quantize, dim3((unsigned)n), dim3(64), 0, s, tiled, row0, dim, dst, s_out, e_out);
}

void vec_q8_scan(const int8_t *cat, const float *cat_s, int64_t n_tiles, int tiles_per_wg, const int8_t *q,
                 const float *q_s, int nqt, int dim, float *scores, int64_t ns, hipStream_t s) {
    const unsigned gx = (unsigned)((n_tiles + tiles_per_wg - 1) / tiles_per_wg);
    const size_t lds = (size_t)32 * dim + 32 * sizeof(float);  // 16.1 KB at dim 512, 32.1 KB at 1024
    hipLaunchKernelGGL(k_vec_scan_i8<512>, dim3(gx, (unsigned)nqt), dim3(512), lds, s, cat, cat_s, n_tiles, tiles_per_wg, q,
                       q_s, dim, scores, ns);
}

hipError_t vec_q8_rescore(const float *cat, const float *q, int dim, unsigned long long *keys, int64_t stride, int n_max,
                          const int32_t *cnt, int cnt_cap, int nb, hipStream_t s) {
    if (n_max <= 0) return hipSuccess;
    const size_t lds = (size_t)dim * (kVecRescorePairs + 2) * sizeof(float);  // 68 KB at dim 512, 136 KB at 1024
    if (lds > 65536) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_vec_rescore),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_vec_rescore, dim3((unsigned)((n_max + kVecRescorePairs - 1) / kVecRescorePairs), (unsigned)nb),
                       dim3(256), lds, s, cat, q, dim, keys, stride, n_max, cnt, cnt_cap);
    return hipGetLastError();
}

void vec_q8_filter(const float *scores, int64_t ns, const uint8_t *dead, int64_t n, const uint32_t *thr,
                   unsigned long long *cand, int cap, int32_t *cnt, int nb, hipStream_t s) {
    hipLaunchKernelGGL(k_vec_filter_q8<VecLive>, dim3((unsigned)((n + 2047) / 2048), (unsigned)nb), dim3(256), 0, s, scores, ns,
                       VecLive{dead}, n, thr, cand, cap, cnt);
}

void vec_q8_filter_allowed(const float *scores, int64_t ns, const VecAllow &al, int64_t n, const uint32_t *thr,
                           unsigned long long *cand, int cap, int32_t *cnt, int nb, hipStream_t s) {
    hipLaunchKernelGGL(k_vec_filter_q8<VecAllowed>, dim3((unsigned)((n + 2047) / 2048), (unsigned)nb), dim3(256), 0, s, scores,
                       ns, VecAllowed{reinterpret_cast<const uint32_t *>(al.bm), al.fmap, al.words * 2}, n, thr, cand, cap,
                       cnt);
}

void vec_q8_tau(const unsigned long long *keys, int64_t stride, int R, int limit, const float *q_e, float E, int dim,
                uint32_t *thr, int32_t *cnt, int nb, hipStream_t s) {
    int sp = 2;
    while (sp < R) sp <<= 1;
    hipLaunchKernelGGL(k_vec_tau, dim3((unsigned)nb), dim3(256), (size_t)sp * 8, s, keys, stride, R, sp, limit, q_e, E, dim,
                       thr, cnt);
}

}  // namespace aid
