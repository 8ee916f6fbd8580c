// vector.hip -- K9, the vector ("vibe") lane of spec/FPSPEC.md 9: an exact brute-force cosine top-K over a
// device-resident catalog of chunk embeddings, and the chunk -> track aggregation.
//
// Replaces the reference's Qdrant round trip (audio-ident-service/app/search/vibe.py:164-218, an approximate HNSW
// search over int8-quantised vectors) and aggregate_chunk_hits (app/search/aggregation.py:63-138).
//
//   k_vec_normalize   raw vectors -> unit vectors in the tiled layout (aidfp_vector.h), one wave per vector
//   k_vec_scan_mfma   scores of a 32-query tile against the catalog on v_mfma_f32_32x32x2_f32: k ascending into
//                     one accumulator per (query, entry), which is bit for bit the spec's fmaf chain
//   k_vec_scan_valu   the same chain with explicit fmaf, one pair per lane (A/B and second witness)
//   k_vec_slice_max, k_vec_threshold, k_vec_filter
//                     selection by threshold: the limit-th largest slice maximum bounds the hit list from below;
//                     the few entries at or above it become 64-bit keys (score, ~entry)
//   k_vec_select      a bitonic sort of such keys in LDS, best first; also the whole selection, slice by slice,
//                     where the threshold route does not apply (fewer slices than `limit`, or too many ties)
//   k_vec_hits        final keys -> hit columns
//   k_vec_aggregate   one wave per query, binary64, in LDS
//
// The opt-in int8 prefilter (FPSPEC 9.1, aid_vec_prefilter) answers the same searches from an int8 copy of the
// catalog plus exact rescoring; its kernels are in csrc/vector_q8.hip, its host route (vec_search_q8) is here.
// The opt-in filtered search (FPSPEC 9.2) narrows "live" to "passes this query's filter" on every route: K9f
// (csrc/vector_filter.hip) writes a batch's allow-bitmaps, and the selection kernels read them through VecAllowed.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "aidfp_vector.h"
#include "aidfp_vector_keys.h"

namespace aid {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------------------------
// kernels

// FPSPEC 9 normalisation, one wave per vector. src: [n][dim] row-major; dst: tiled layout, vector v lands at row
// row0 + v. The wave stages the vector in LDS with coalesced loads, every lane runs the same serial ss chain over
// it (the chain is the spec's; only its operands are fetched in parallel), then each lane divides and stores its
// own elements.
__global__ __launch_bounds__(64) void k_vec_normalize(const float *__restrict__ src, int64_t n, int dim,
                                                      float *__restrict__ dst, int64_t row0) {
    __shared__ float4 sx4[256];
    float *sx = reinterpret_cast<float *>(sx4);
    const int64_t v = blockIdx.x;
    const int lane = threadIdx.x;
    const float *x = src + (size_t)v * dim;
    for (int k = lane; k < dim; k += 64) sx[k] = x[k];
    __syncthreads();
    float ss = 0.0f;
    for (int k4 = 0; k4 < (dim >> 2); ++k4) {
        const float4 a = sx4[k4];
        ss = __builtin_fmaf(a.x, a.x, ss);
        ss = __builtin_fmaf(a.y, a.y, ss);
        ss = __builtin_fmaf(a.z, a.z, ss);
        ss = __builtin_fmaf(a.w, a.w, ss);
    }
    const bool ok = ss > 0.0f && ss < __builtin_inff();  // not 0, not inf, not NaN
    const float d = sqrtf(ss);
    const int64_t row = row0 + v;
    float *tile = dst + (size_t)(row >> 5) * 32 * dim + (size_t)(row & 31) * 4;
    for (int k = lane; k < dim; k += 64) {
        const float y = ok ? sx[k] / d : 0.0f;
        tile[(size_t)((k >> 3) * 2 + (k & 1)) * 128 + ((k & 7) >> 1)] = y;
    }
}

// One workgroup: `tiles_per_wg` catalog tiles against one tile of 32 queries staged in LDS; wave w takes tiles
// w, w + NT / 64, ... of the chunk. A = queries (rows), B = catalog (columns): C has the entry on the lane, so the
// 32 lanes of a half wave store 128 contiguous bytes of one query's score row. A stage is four k-groups (32 values
// of k, 4 KB per wave, 16 MFMAs); the next stage's loads, of this tile or of the wave's next one,
// are issued before the current stage's MFMAs, so every wave always has 4 KB in flight.
template <int NT>
__global__ __launch_bounds__(NT) void k_vec_scan_mfma(const float *__restrict__ cat, int64_t n_tiles, int tiles_per_wg,
                                                      const float *__restrict__ q, int dim,
                                                      float *__restrict__ scores, int64_t ns) {
    extern __shared__ float4 sq[];  // [dim / 8][64]
    const int G = dim >> 3;
    const int qt0 = blockIdx.y;
    const float4 *qsrc = reinterpret_cast<const float4 *>(q) + (size_t)qt0 * G * 64;
    for (int i = threadIdx.x; i < G * 64; i += NT) sq[i] = qsrc[i];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t t1 = min((int64_t)(blockIdx.x + 1) * tiles_per_wg, n_tiles);
    int64_t t = (int64_t)blockIdx.x * tiles_per_wg + wave;
    if (t >= t1) return;
    const int n_stages = G >> 2;  // dim is a multiple of 32
    const float4 *cat4 = reinterpret_cast<const float4 *>(cat) + lane;
    float4 cv[4], nx[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) cv[u] = cat4[(size_t)t * G * 64 + u * 64];
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    int st = 0;
    for (;;) {
        int st_next = st + 1;
        int64_t t_next = t;
        if (st_next == n_stages) {
            st_next = 0;
            t_next = t + NT / 64;
        }
        const bool more = t_next < t1;
        if (more) {
            const float4 *cn = cat4 + (size_t)t_next * G * 64 + (size_t)st_next * 256;
#pragma unroll
            for (int u = 0; u < 4; ++u) nx[u] = cn[u * 64];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float4 qv = sq[(st * 4 + u) * 64 + lane];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qv.x, cv[u].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qv.y, cv[u].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qv.z, cv[u].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qv.w, cv[u].w, acc, 0, 0, 0);
        }
        if (st_next == 0) {  // the tile's chain is complete
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qrow = qt0 * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                scores[(size_t)qrow * ns + t * 32 + (lane & 31)] = acc[r];
                acc[r] = 0.0f;
            }
        }
        if (!more) break;
        cv[0] = nx[0];
        cv[1] = nx[1];
        cv[2] = nx[2];
        cv[3] = nx[3];
        st = st_next;
        t = t_next;
    }
}

// One (query, entry) pair per lane: the spec's chain written out. Rows [n, ns) are the zero padding of the last tile.
__global__ __launch_bounds__(256) void k_vec_scan_valu(const float *__restrict__ cat, int64_t ns, const float *__restrict__ q,
                                                       int dim, float *__restrict__ scores) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int qi = blockIdx.y;
    if (e >= ns) return;
    const int G = dim >> 3;
    const float4 *c = reinterpret_cast<const float4 *>(cat) + (size_t)(e >> 5) * G * 64 + (e & 31);
    const float4 *v = reinterpret_cast<const float4 *>(q) + (size_t)(qi >> 5) * G * 64 + (qi & 31);
    float acc = 0.0f;
    for (int g = 0; g < G; ++g) {
        const float4 c0 = c[g * 64], c1 = c[g * 64 + 32], q0 = v[g * 64], q1 = v[g * 64 + 32];
        acc = __builtin_fmaf(q0.x, c0.x, acc);
        acc = __builtin_fmaf(q1.x, c1.x, acc);
        acc = __builtin_fmaf(q0.y, c0.y, acc);
        acc = __builtin_fmaf(q1.y, c1.y, acc);
        acc = __builtin_fmaf(q0.z, c0.z, acc);
        acc = __builtin_fmaf(q1.z, c1.z, acc);
        acc = __builtin_fmaf(q0.w, c0.w, acc);
        acc = __builtin_fmaf(q1.w, c1.w, acc);
    }
    scores[(size_t)qi * ns + e] = acc;
}

// Slice blockIdx.x of query blockIdx.y: keys of `slice` inputs (scores of live entries on the first pass, the
// previous pass's keys after it) sorted descending in LDS; the first `keep` go to out[q][slice_index][keep].
// M (aidfp_vector_keys.h) says which entries count, here and in k_vec_slice_max and k_vec_filter: VecLive by
// default, VecAllowed under a filter (FPSPEC 9.2).
template <typename M>
__global__ __launch_bounds__(256) void k_vec_select(const float *__restrict__ scores, int64_t ns, const M member,
                                                    const unsigned long long *__restrict__ in, int64_t in_stride,
                                                    int64_t n_in, int slice, int keep,
                                                    unsigned long long *__restrict__ out, int64_t out_stride) {
    extern __shared__ unsigned long long keys[];  // [slice rounded up to a power of two]
    const int q = blockIdx.y;
    const int64_t base = (int64_t)blockIdx.x * slice;
    const int cnt = (int)min((int64_t)slice, n_in - base);
    int sp = 2;  // this slice's own padded size: a ragged last slice sorts less
    while (sp < cnt) sp <<= 1;
    const auto mrow = member.row(q);
    for (int i = threadIdx.x; i < sp; i += 256) {
        unsigned long long key = 0;
        if (i < cnt) {
            if (scores) {
                const int64_t e = base + i;
                if (M::test(mrow, e)) key = vec_key(scores[(size_t)q * ns + e], (uint32_t)e);
            } else {
                key = in[(size_t)q * in_stride + base + i];
            }
        }
        keys[i] = key;
    }
    __syncthreads();
    vec_sort_desc(keys, sp);
    for (int i = threadIdx.x; i < keep; i += 256)
        out[(size_t)q * out_stride + (size_t)blockIdx.x * keep + i] = i < sp ? keys[i] : 0ull;
}

// ---- the threshold route of the selection (exact, and a small fraction of the sorting work). With the live
// entries of a query cut into slices, the limit-th largest of the slice maxima is a score that at least `limit`
// entries reach, so no entry below it is in the hit list. k_vec_slice_max and k_vec_threshold find it, and
// k_vec_filter appends the keys of the entries at or above it to the query's candidate list, which one
// k_vec_select sorts. Candidates arrive in any order; their keys are distinct, so the sorted list is the same on
// every run. A list that would overflow (many equal scores) sends the batch down the slice-by-slice route instead.
template <typename M>
__global__ __launch_bounds__(256) void k_vec_slice_max(const float *__restrict__ scores, int64_t ns, const M member,
                                                       int64_t n, int slice, int n_slices,
                                                       uint32_t *__restrict__ out) {
    __shared__ uint32_t part[4];
    const int q = blockIdx.y;
    const int64_t base = (int64_t)blockIdx.x * slice;
    const int64_t end = min(base + (int64_t)slice, n);
    const auto mrow = member.row(q);
    uint32_t m = 0;
    for (int64_t e = base + threadIdx.x; e < end; e += 256)
        if (M::test(mrow, e)) m = max(m, vec_score_key(scores[(size_t)q * ns + e]));
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) out[(size_t)q * n_slices + blockIdx.x] = max(max(part[0], part[1]), max(part[2], part[3]));
}

__global__ __launch_bounds__(256) void k_vec_threshold(const uint32_t *__restrict__ maxs, int n_slices, int sp, int limit,
                                                       uint32_t *__restrict__ thr, int32_t *__restrict__ cnt) {
    extern __shared__ uint32_t smax[];  // [sp], sp = n_slices rounded up to a power of two
    const int q = blockIdx.x;
    for (int i = threadIdx.x; i < sp; i += 256) smax[i] = i < n_slices ? maxs[(size_t)q * n_slices + i] : 0u;
    __syncthreads();
    vec_sort_desc(smax, sp);
    if (threadIdx.x == 0) {
        thr[q] = smax[limit - 1];  // limit <= n_slices
        cnt[q] = 0;
    }
}

template <typename M>
__global__ __launch_bounds__(256) void k_vec_filter(const float *__restrict__ scores, int64_t ns, const M member,
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
                const int pos = atomicAdd(&cnt[q], 1);
                if (pos < cap) cand[(size_t)q * cap + pos] = vec_key(s, (uint32_t)e);
            }
        }
    }
}

// Final keys of query blockIdx.x (a sorted prefix of non-zero keys among `have`) -> hit columns [q][limit]. With
// qmap the columns of query blockIdx.x are those of qmap[blockIdx.x] (the prefilter's fallback queries, which are
// scanned as a tile of their own).
__global__ __launch_bounds__(256) void k_vec_hits(const unsigned long long *__restrict__ keys, int64_t stride, int have,
                                                  int limit, const uint32_t *__restrict__ track,
                                                  const double *__restrict__ off, const int32_t *__restrict__ qmap,
                                                  uint32_t *__restrict__ h_entry, uint32_t *__restrict__ h_track,
                                                  float *__restrict__ h_score, double *__restrict__ h_off,
                                                  int32_t *__restrict__ n_hits) {
    const unsigned long long *k = keys + (size_t)blockIdx.x * stride;
    const int q = qmap ? qmap[blockIdx.x] : (int)blockIdx.x;
    if (threadIdx.x == 0 && (have == 0 || k[0] == 0)) n_hits[q] = 0;
    for (int i = threadIdx.x; i < have; i += 256) {
        const unsigned long long key = k[i];
        if (key == 0) continue;
        const uint32_t e = 0xFFFFFFFFu - (uint32_t)key;
        const size_t o = (size_t)q * limit + i;
        h_entry[o] = e;
        h_track[o] = track[e];
        h_score[o] = vec_key_score(key);
        h_off[o] = off[e];
        if (i + 1 == have || k[i + 1] == 0) n_hits[q] = i + 1;
    }
}

// FPSPEC 9 aggregation of one query's hit list (at most kVecMaxLimit hits), one wave, binary64.
__global__ __launch_bounds__(64) void k_vec_aggregate(const uint32_t *__restrict__ track, const float *__restrict__ score,
                                                      const double *__restrict__ off, const int64_t *__restrict__ start,
                                                      const int32_t *__restrict__ count, int64_t stride, int top_k,
                                                      double weight, const uint32_t *__restrict__ exclude,
                                                      double threshold, int max_out, aid_vibe_row *__restrict__ out,
                                                      int32_t *__restrict__ n_out) {
    __shared__ uint32_t s_track[kVecMaxLimit];
    __shared__ uint16_t s_lead[kVecMaxLimit];   // first hit of the same track
    __shared__ uint16_t s_glist[kVecMaxLimit];  // leaders, in order of first appearance
    __shared__ double s_final[kVecMaxLimit], s_base[kVecMaxLimit], s_bonus[kVecMaxLimit];
    __shared__ int32_t s_cnt[kVecMaxLimit];
    __shared__ uint8_t s_ex[kVecMaxLimit];
    __shared__ int s_kept;
    const int q = blockIdx.x, lane = threadIdx.x;
    const int64_t s0 = start ? start[q] : (int64_t)q * stride;
    const int n = min(count[q], kVecMaxLimit);
    if (lane == 0) s_kept = 0;
    for (int i = lane; i < n; i += 64) s_track[i] = track[s0 + i];
    __syncthreads();
    for (int i = lane; i < n; i += 64) {
        const uint32_t t = s_track[i];
        int l = i;
        for (int j = 0; j < i; ++j)
            if (s_track[j] == t) {
                l = j;
                break;
            }
        s_lead[i] = (uint16_t)l;
    }
    __syncthreads();
    int ng = 0;
    for (int b = 0; b < n; b += 64) {
        const int i = b + lane;
        const bool f = i < n && s_lead[i] == i;
        const unsigned long long m = __ballot(f);
        if (f) s_glist[ng + __popcll(m & ((1ull << lane) - 1))] = (uint16_t)i;
        ng += __popcll(m);
    }
    __syncthreads();
    const uint32_t ex = exclude ? exclude[q] : AID_VEC_NO_TRACK;
    for (int g = lane; g < ng; g += 64) {
        const int lead = s_glist[g];
        int cnt = 0, uniq = 0;
        double sum = 0.0, u0 = 0.0, u1 = 0.0, u2 = 0.0, u3 = 0.0;  // the fifth distinct offset need not be kept
        for (int i = lead; i < n; ++i) {
            if (s_lead[i] != lead) continue;
            if (cnt < top_k) sum += (double)score[s0 + i];
            ++cnt;
            if (uniq < 5) {  // min(unique / 5.0, 1.0) saturates at five distinct offsets
                const double o = off[s0 + i];
                const bool seen = (uniq > 0 && u0 == o) || (uniq > 1 && u1 == o) || (uniq > 2 && u2 == o) ||
                                  (uniq > 3 && u3 == o);
                if (!seen) {
                    if (uniq == 0) u0 = o;
                    if (uniq == 1) u1 = o;
                    if (uniq == 2) u2 = o;
                    if (uniq == 3) u3 = o;
                    ++uniq;
                }
            }
        }
        const double base = sum / (double)min(top_k, cnt);
        const double bonus = fmin((double)uniq / 5.0, 1.0) * weight;
        s_base[g] = base;
        s_bonus[g] = bonus;
        s_final[g] = base + bonus;
        s_cnt[g] = cnt;
        s_ex[g] = s_track[lead] == ex && ex != AID_VEC_NO_TRACK;
    }
    __syncthreads();
    for (int g = lane; g < ng; g += 64) {
        if (s_ex[g]) continue;
        const double f = s_final[g];
        if (!(f >= threshold)) continue;
        int rank = 0;
        for (int h = 0; h < ng; ++h)
            if (!s_ex[h] && (s_final[h] > f || (s_final[h] == f && h < g))) ++rank;
        if (rank < max_out) {
            aid_vibe_row r;
            r.track = s_track[s_glist[g]];
            r.chunk_count = s_cnt[g];
            r.final_score = f;
            r.base_score = s_base[g];
            r.diversity_bonus = s_bonus[g];
            out[(size_t)q * max_out + rank] = r;
            atomicAdd(&s_kept, 1);
        }
    }
    __syncthreads();
    if (lane == 0) n_out[q] = s_kept;
}

// Compaction: new row r takes old row map[r]; rows [n_new, rows_pad) become +0. One thread per float4.
__global__ __launch_bounds__(256) void k_vec_gather(const float4 *__restrict__ src, const uint32_t *__restrict__ map,
                                                    int64_t n_new, int64_t rows_pad, int dim, float4 *__restrict__ dst) {
    const int G2 = dim >> 2;  // float4 per row
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows_pad * G2) return;
    const int64_t t = idx / (32 * G2);
    const int rem = (int)(idx % (32 * G2));
    const int gh = rem >> 5, i = rem & 31;
    const int64_t r = t * 32 + i;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (r < n_new) {
        const int64_t o = map[r];
        v = src[(size_t)(o >> 5) * 32 * G2 + (size_t)gh * 32 + (o & 31)];
    }
    dst[idx] = v;
}

// ---------------------------------------------------------------------------------------------------------------
// host side

static int vfail(VecCatalog &c, int code, const std::string &msg) {
    c.err = msg;
    return code;
}

#define VEC_TRY(expr)                                                                                    \
    do {                                                                                                 \
        hipError_t _e = (expr);                                                                          \
        if (_e != hipSuccess)                                                                            \
            return vfail(c, _e == hipErrorOutOfMemory ? AID_ERR_NOMEM : AID_ERR_DEVICE,                  \
                         std::string(#expr) + ": " + hipGetErrorString(_e));                             \
    } while (0)

static bool vec_dim_ok(int dim) { return dim >= 32 && dim <= 1024 && dim % 32 == 0; }

// ---- the int8 planes of the prefilter (FPSPEC 9.1): a pure function of the stored f32 rows
static void vec_q8_release(VecCatalog &c) {
    c.d_v8.release();
    c.d_s8.release();
    c.d_e8.release();
    c.h_s8.clear();
    c.h_e8.clear();
    c.q8_rows = 0;
    c.q8_E = 0.0f;
}

// Quantise rows [row0, row0 + n) of d_vecs into the planes, bring their s and e to the host mirror (whose size is
// row0 on entry) and fold them into E.
static int vec_q8_append(VecCatalog &c, int64_t row0, int64_t n, hipStream_t s) {
    if (n <= 0) return AID_OK;
    vec_q8_quantize(c.d_vecs.p, row0, n, c.dim, c.d_v8.p, c.d_s8.p, c.d_e8.p, s);
    VEC_TRY(hipGetLastError());
    c.h_s8.resize((size_t)(row0 + n));
    c.h_e8.resize((size_t)(row0 + n));
    VEC_TRY(hipMemcpyAsync(c.h_s8.data() + row0, c.d_s8.p + row0, n * sizeof(float), hipMemcpyDeviceToHost, s));
    VEC_TRY(hipMemcpyAsync(c.h_e8.data() + row0, c.d_e8.p + row0, n * sizeof(float), hipMemcpyDeviceToHost, s));
    VEC_TRY(hipStreamSynchronize(s));
    for (int64_t i = row0; i < row0 + n; ++i) c.q8_E = std::max(c.q8_E, c.h_e8[i]);
    return AID_OK;
}

// Build the planes for the catalog as it stands (cap_rows rows, the first n quantised, the rest zero): on enabling,
// after a load, and when the f32 block has grown.
static int vec_q8_rebuild(VecCatalog &c, hipStream_t s) {
    c.h_s8.clear();
    c.h_e8.clear();
    c.q8_E = 0.0f;
    c.q8_rows = 0;
    if (!c.cap_rows) return AID_OK;
    const size_t rows = (size_t)c.cap_rows;
    VEC_TRY(c.d_v8.reserve(rows * c.dim));
    VEC_TRY(c.d_s8.reserve(rows));
    VEC_TRY(c.d_e8.reserve(rows));
    VEC_TRY(hipMemsetAsync(c.d_v8.p, 0, rows * c.dim, s));
    VEC_TRY(hipMemsetAsync(c.d_s8.p, 0, rows * sizeof(float), s));
    VEC_TRY(hipMemsetAsync(c.d_e8.p, 0, rows * sizeof(float), s));
    c.q8_rows = c.cap_rows;
    return vec_q8_append(c, 0, c.n, s);
}

int vec_prefilter(VecCatalog &c, int mode, int oversample, hipStream_t s) {
    if ((mode != 0 && mode != 1) || oversample < 1 || oversample > kVecQ8MaxOversample)
        return vfail(c, AID_ERR_INVALID, "aid_vec_prefilter: mode is 0 (off) or 1 (int8), oversample in [1, 64]");
    c.q8_over = oversample;
    if (mode == 0) {
        if (c.q8_mode) (void)hipDeviceSynchronize();
        c.q8_mode = 0;
        vec_q8_release(c);
        return AID_OK;
    }
    if (c.q8_mode == 1) return AID_OK;
    c.q8_mode = 1;
    if (int rc = vec_q8_rebuild(c, s)) {
        c.q8_mode = 0;
        vec_q8_release(c);
        return rc;
    }
    return AID_OK;
}

int vec_reset(VecCatalog &c, int dim) {
    if (!vec_dim_ok(dim)) return vfail(c, AID_ERR_INVALID, "aid_vec_reset: dim must be a multiple of 32 in [32, 1024]");
    if (dim != c.dim && c.d_vecs.p) {  // another row size: the stored tiles are of no use
        (void)hipDeviceSynchronize();
        c.d_vecs.release();
        c.cap_rows = 0;
        vec_q8_release(c);
    }
    if (c.d_vecs.p) VEC_TRY(hipMemset(c.d_vecs.p, 0, (size_t)c.cap_rows * dim * sizeof(float)));
    if (c.q8_rows) {  // the int8 planes of an empty catalog: zero, as the f32 rows are
        VEC_TRY(hipMemset(c.d_v8.p, 0, (size_t)c.q8_rows * dim));
        VEC_TRY(hipMemset(c.d_s8.p, 0, (size_t)c.q8_rows * sizeof(float)));
        VEC_TRY(hipMemset(c.d_e8.p, 0, (size_t)c.q8_rows * sizeof(float)));
    }
    c.h_s8.clear();
    c.h_e8.clear();
    c.q8_E = 0.0f;
    c.dim = dim;
    c.n = c.n_live = 0;
    c.h_track.clear();
    c.h_chunk.clear();
    c.h_off.clear();
    c.h_dead.clear();
    c.h_tags.clear();
    c.tags_on_dev = 0;
    return AID_OK;
}

// Grow the catalog to hold `rows` rows (tiles, payload columns); stored rows are kept, new rows are +0.
static int vec_grow(VecCatalog &c, int64_t rows, hipStream_t s) {
    if (rows > c.cap_rows) {
        int64_t cap = std::max<int64_t>(rows, c.cap_rows * 2);
        cap = (cap + 1023) / 1024 * 1024;
        // the new block is whole (stored tiles copied, the rest +0) before it replaces the old one: a failure on
        // the way leaves the catalog as it was (DevBuf::grow_keep would commit ahead of the memset)
        DevBuf<float> nb;
        VEC_TRY(nb.reserve((size_t)cap * c.dim));
        const size_t keep = (size_t)((c.n + 31) / 32) * 32 * c.dim;
        if (keep) VEC_TRY(hipMemcpyAsync(nb.p, c.d_vecs.p, keep * sizeof(float), hipMemcpyDeviceToDevice, s));
        VEC_TRY(hipMemsetAsync(nb.p + keep, 0, ((size_t)cap * c.dim - keep) * sizeof(float), s));
        VEC_TRY(hipStreamSynchronize(s));
        if (c.d_vecs.p) (void)hipDeviceSynchronize();
        std::swap(c.d_vecs, nb);  // nb frees the old block
        c.cap_rows = cap;
        if (keep) ++c.st[5];
    }
    if ((size_t)rows > c.d_track.n) {  // payload columns: rebuilt from the host mirror
        const size_t cap = (size_t)c.cap_rows;
        VEC_TRY(c.d_track.reserve(cap));
        VEC_TRY(c.d_off.reserve(cap));
        VEC_TRY(c.d_dead.reserve(cap));
        if (c.n) {
            VEC_TRY(hipMemcpyAsync(c.d_track.p, c.h_track.data(), c.n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            VEC_TRY(hipMemcpyAsync(c.d_off.p, c.h_off.data(), c.n * sizeof(double), hipMemcpyHostToDevice, s));
            VEC_TRY(hipMemcpyAsync(c.d_dead.p, c.h_dead.data(), c.n, hipMemcpyHostToDevice, s));
            VEC_TRY(hipStreamSynchronize(s));
        }
    }
    return AID_OK;
}

int vec_add(VecCatalog &c, const float *vecs, const uint32_t *tracks, const int32_t *chunk_index, const double *offset_sec,
            const uint64_t *tags, int64_t n, int location, hipStream_t s) {
    if (n < 0 || (location != AID_PCM_HOST && location != AID_PCM_DEVICE) || (n > 0 && (!vecs || !tracks || !offset_sec)))
        return vfail(c, AID_ERR_INVALID, "aid_vec_add: bad argument");
    if (!c.dim) return vfail(c, AID_ERR_STATE, "aid_vec_add: call aid_vec_reset first");
    if (n == 0) return AID_OK;
    if (c.n + n >= 0xFFFFFFFFll) return vfail(c, AID_ERR_INVALID, "aid_vec_add: more than 2^32 - 2 entries");
    if (int rc = vec_grow(c, c.n + n, s)) return rc;
    if (c.q8_mode && c.q8_rows != c.cap_rows)  // the f32 block is new or has grown: so do the int8 planes
        if (int rc = vec_q8_rebuild(c, s)) return rc;
    // payload to the host mirror first (a device caller's columns come back once; they are 16 bytes an entry)
    std::vector<uint32_t> tr(n);
    std::vector<int32_t> ch(n);
    std::vector<double> of(n);
    std::vector<uint64_t> tg(n, 0);  // FPSPEC 9.2: 0 unless given
    if (location == AID_PCM_DEVICE) {
        if (tags) VEC_TRY(hipMemcpyAsync(tg.data(), tags, n * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        VEC_TRY(hipMemcpyAsync(tr.data(), tracks, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        VEC_TRY(hipMemcpyAsync(of.data(), offset_sec, n * sizeof(double), hipMemcpyDeviceToHost, s));
        if (chunk_index) VEC_TRY(hipMemcpyAsync(ch.data(), chunk_index, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        VEC_TRY(hipStreamSynchronize(s));
    } else {
        memcpy(tr.data(), tracks, n * sizeof(uint32_t));
        memcpy(of.data(), offset_sec, n * sizeof(double));
        if (chunk_index) memcpy(ch.data(), chunk_index, n * sizeof(int32_t));
        if (tags) memcpy(tg.data(), tags, n * sizeof(uint64_t));
    }
    if (!chunk_index)
        for (int64_t i = 0; i < n; ++i) ch[i] = (int32_t)i;
    for (int64_t i = 0; i < n; ++i)
        if (tr[i] == AID_VEC_NO_TRACK) return vfail(c, AID_ERR_INVALID, "aid_vec_add: track id 0xFFFFFFFF is reserved");
    const float *src = vecs;
    if (location == AID_PCM_HOST) {
        VEC_TRY(c.d_raw.reserve((size_t)n * c.dim));
        VEC_TRY(hipMemcpyAsync(c.d_raw.p, vecs, (size_t)n * c.dim * sizeof(float), hipMemcpyHostToDevice, s));
        src = c.d_raw.p;
    }
    hipLaunchKernelGGL(k_vec_normalize, dim3((unsigned)n), dim3(64), 0, s, src, n, c.dim, c.d_vecs.p, c.n);
    VEC_TRY(hipGetLastError());
    VEC_TRY(hipMemcpyAsync(c.d_track.p + c.n, tr.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    VEC_TRY(hipMemcpyAsync(c.d_off.p + c.n, of.data(), n * sizeof(double), hipMemcpyHostToDevice, s));
    VEC_TRY(hipMemsetAsync(c.d_dead.p + c.n, 0, n, s));
    VEC_TRY(hipStreamSynchronize(s));
    if (c.q8_mode)
        if (int rc = vec_q8_append(c, c.n, n, s)) return rc;
    c.h_track.insert(c.h_track.end(), tr.begin(), tr.end());
    c.h_chunk.insert(c.h_chunk.end(), ch.begin(), ch.end());
    c.h_off.insert(c.h_off.end(), of.begin(), of.end());
    c.h_dead.insert(c.h_dead.end(), (size_t)n, (uint8_t)0);
    c.h_tags.insert(c.h_tags.end(), tg.begin(), tg.end());  // the device column follows at the next filtered call
    c.n += n;
    c.n_live += n;
    return AID_OK;
}

int vec_remove(VecCatalog &c, uint32_t track, hipStream_t s) {
    int64_t hit = 0;
    for (int64_t i = 0; i < c.n; ++i)
        if (c.h_track[i] == track && !c.h_dead[i]) {
            c.h_dead[i] = 1;
            ++hit;
        }
    if (!hit) return vfail(c, AID_ERR_INVALID, "aid_vec_remove: unknown or already removed track");
    c.n_live -= hit;
    VEC_TRY(hipMemcpyAsync(c.d_dead.p, c.h_dead.data(), c.n, hipMemcpyHostToDevice, s));
    VEC_TRY(hipStreamSynchronize(s));
    return AID_OK;
}

int vec_retag(VecCatalog &c, uint32_t track, uint64_t tags) {
    int64_t hit = 0;
    for (int64_t i = 0; i < c.n; ++i)
        if (c.h_track[i] == track && !c.h_dead[i]) {
            c.h_tags[i] = tags;
            ++hit;
        }
    if (!hit) return vfail(c, AID_ERR_INVALID, "aid_vec_retag: unknown or removed track");
    c.tags_on_dev = 0;
    return AID_OK;
}

int vec_tags(VecCatalog &c, uint64_t *out, int64_t cap) {
    if (cap < c.n || (c.n > 0 && !out)) return vfail(c, AID_ERR_INVALID, "aid_vec_tags: out holds fewer than n_entries words");
    if (c.n) memcpy(out, c.h_tags.data(), (size_t)c.n * sizeof(uint64_t));
    return AID_OK;
}

int vec_compact(VecCatalog &c, int64_t *n_removed, hipStream_t s) {
    const int64_t gone = c.n - c.n_live;
    if (n_removed) *n_removed = gone;
    if (!gone) return AID_OK;
    std::vector<uint32_t> map;
    map.reserve(c.n_live);
    for (int64_t i = 0; i < c.n; ++i)
        if (!c.h_dead[i]) map.push_back((uint32_t)i);
    const int64_t m = (int64_t)map.size();
    {
        DevBuf<float> nb;  // the live rows gathered into a new block, which then replaces the old one
        VEC_TRY(nb.reserve((size_t)c.cap_rows * c.dim));
        VEC_TRY(c.d_hentry.reserve((size_t)std::max<int64_t>(m, 1)));
        if (m) VEC_TRY(hipMemcpyAsync(c.d_hentry.p, map.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        const int64_t f4 = c.cap_rows * (c.dim / 4);
        hipLaunchKernelGGL(k_vec_gather, dim3((unsigned)((f4 + 255) / 256)), dim3(256), 0, s,
                           reinterpret_cast<const float4 *>(c.d_vecs.p), c.d_hentry.p, m, c.cap_rows, c.dim,
                           reinterpret_cast<float4 *>(nb.p));
        VEC_TRY(hipGetLastError());
        VEC_TRY(hipStreamSynchronize(s));
        std::swap(c.d_vecs, nb);
    }
    if (c.q8_mode && c.q8_rows) {
        // the int8 rows move as the f32 rows do: a tile is [dim / 16][32] 16-byte units, which k_vec_gather copies
        // bit for bit as the float4 units of a catalog of dim / 4
        DevBuf<int8_t, 64> nb;
        VEC_TRY(nb.reserve((size_t)c.q8_rows * c.dim));
        const int64_t u16 = c.q8_rows * (c.dim / 16);
        hipLaunchKernelGGL(k_vec_gather, dim3((unsigned)((u16 + 255) / 256)), dim3(256), 0, s,
                           reinterpret_cast<const float4 *>(c.d_v8.p), c.d_hentry.p, m, c.q8_rows, c.dim / 4,
                           reinterpret_cast<float4 *>(nb.p));
        VEC_TRY(hipGetLastError());
        VEC_TRY(hipStreamSynchronize(s));
        std::swap(c.d_v8, nb);
        c.q8_E = 0.0f;
        for (int64_t r = 0; r < m; ++r) {
            c.h_s8[r] = c.h_s8[map[r]];
            c.h_e8[r] = c.h_e8[map[r]];
            c.q8_E = std::max(c.q8_E, c.h_e8[r]);
        }
        c.h_s8.resize(m);
        c.h_e8.resize(m);
        VEC_TRY(hipMemsetAsync(c.d_s8.p, 0, (size_t)c.q8_rows * sizeof(float), s));
        VEC_TRY(hipMemsetAsync(c.d_e8.p, 0, (size_t)c.q8_rows * sizeof(float), s));
        if (m) {
            VEC_TRY(hipMemcpyAsync(c.d_s8.p, c.h_s8.data(), m * sizeof(float), hipMemcpyHostToDevice, s));
            VEC_TRY(hipMemcpyAsync(c.d_e8.p, c.h_e8.data(), m * sizeof(float), hipMemcpyHostToDevice, s));
        }
        VEC_TRY(hipStreamSynchronize(s));
    }
    for (int64_t r = 0; r < m; ++r) {
        c.h_track[r] = c.h_track[map[r]];
        c.h_chunk[r] = c.h_chunk[map[r]];
        c.h_off[r] = c.h_off[map[r]];
        c.h_tags[r] = c.h_tags[map[r]];
    }
    c.h_tags.resize(m);
    c.tags_on_dev = 0;
    c.h_track.resize(m);
    c.h_chunk.resize(m);
    c.h_off.resize(m);
    c.h_dead.assign(m, 0);
    c.n = c.n_live = m;
    if (m) {
        VEC_TRY(hipMemcpyAsync(c.d_track.p, c.h_track.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        VEC_TRY(hipMemcpyAsync(c.d_off.p, c.h_off.data(), m * sizeof(double), hipMemcpyHostToDevice, s));
        VEC_TRY(hipMemsetAsync(c.d_dead.p, 0, m, s));
        VEC_TRY(hipStreamSynchronize(s));
    }
    return AID_OK;
}

static int pow2_ceil(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

// Normalise queries [q0, q0 + nb) into c.d_q (tiled, zero padded to a whole tile) and score them against the
// catalog into c.d_scores [nb rounded up to 32][ns], ns = n rounded up to 32.
static int vec_scan_batch(VecCatalog &c, const float *dq, int nb, hipStream_t s) {
    const int dim = c.dim;
    const int nqt = (nb + 31) / 32;
    const int64_t n_tiles = (c.n + 31) / 32, ns = n_tiles * 32;
    VEC_TRY(hipMemsetAsync(c.d_q.p, 0, (size_t)nqt * 32 * dim * sizeof(float), s));
    hipLaunchKernelGGL(k_vec_normalize, dim3((unsigned)nb), dim3(64), 0, s, dq, (int64_t)nb, dim, c.d_q.p,
                       (int64_t)0);
    if (c.force_path == 2) {
        hipLaunchKernelGGL(k_vec_scan_valu, dim3((unsigned)((ns + 255) / 256), (unsigned)nb), dim3(256), 0, s, c.d_vecs.p, ns,
                           c.d_q.p, dim, c.d_scores.p);
        ++c.st[7];
    } else {
        const int chunk = c.force_chunk ? c.force_chunk : kVecScanChunk;
        const int tiles_per_wg = std::max(1, chunk / 32);
        const unsigned gx = (unsigned)((n_tiles + tiles_per_wg - 1) / tiles_per_wg);
        const size_t lds = (size_t)32 * dim * sizeof(float);  // 64 KB at dim 512: two workgroups, 16 waves, per CU
        if (lds > 65536)
            VEC_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_vec_scan_mfma<512>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_vec_scan_mfma<512>, dim3(gx, (unsigned)nqt), dim3(512), lds, s, c.d_vecs.p, n_tiles, tiles_per_wg,
                           c.d_q.p, dim, c.d_scores.p, ns);
        ++c.st[6];
    }
    VEC_TRY(hipGetLastError());
    return AID_OK;
}

static int vec_query_args(VecCatalog &c, const char *what, const float *queries, int nq, int location) {
    if (nq < 0 || (nq > 0 && !queries) || (location != AID_PCM_HOST && location != AID_PCM_DEVICE))
        return vfail(c, AID_ERR_INVALID, std::string(what) + ": bad argument");
    if (!c.dim) return vfail(c, AID_ERR_STATE, std::string(what) + ": call aid_vec_reset first");
    return AID_OK;
}

// The queries on the device (staged through d_raw when they are host memory).
static int vec_stage_queries(VecCatalog &c, const float *queries, int nq, int location, hipStream_t s, const float **dq) {
    *dq = queries;
    if (location == AID_PCM_HOST) {
        VEC_TRY(c.d_raw.reserve((size_t)nq * c.dim));
        VEC_TRY(hipMemcpyAsync(c.d_raw.p, queries, (size_t)nq * c.dim * sizeof(float), hipMemcpyHostToDevice, s));
        *dq = c.d_raw.p;
    }
    const int64_t ns = (c.n + 31) / 32 * 32;
    VEC_TRY(c.d_q.reserve((size_t)kVecQueryBatch * c.dim));
    VEC_TRY(c.d_scores.reserve((size_t)kVecQueryBatch * std::max<int64_t>(ns, 32)));
    return AID_OK;
}

// How one batch's hit lists are selected from its score matrix, for one `limit`.
struct VecSelPlan {
    int limit, slice, keep, mslice;
    int64_t msl;
    bool by_threshold;
    bool q8 = false;  // the prefilter's selection over approx: candidate counts in lines of their own (k_vec_filter_q8)
};

// The plan for `limit`, with the scratch it needs.
static int vec_sel_plan(VecCatalog &c, int limit, VecSelPlan &p) {
    p.limit = limit;
    // slice-by-slice route: a slice holds at least 2 * limit keys, so every pass shrinks the candidate set
    p.slice = std::max(c.force_chunk ? c.force_chunk : kVecSelectSlice, 2 * pow2_ceil(limit));
    p.keep = std::min(limit, p.slice);
    const int64_t nsl0 = (c.n + p.slice - 1) / p.slice;
    VEC_TRY(c.d_keys0.reserve((size_t)kVecQueryBatch * nsl0 * p.keep));
    VEC_TRY(c.d_keys1.reserve((size_t)kVecQueryBatch * ((nsl0 * p.keep + p.slice - 1) / p.slice) * p.keep));
    // threshold route: needs at least `limit` slices, and few enough of them for one sort of their maxima
    p.mslice = c.force_chunk ? c.force_chunk
                             : std::max(kVecMaxSlice, pow2_ceil((int)((c.n + kVecCandCap - 1) / kVecCandCap)));
    p.msl = (c.n + p.mslice - 1) / p.mslice;
    p.by_threshold = p.msl >= limit && p.msl <= kVecCandCap;
    if (p.by_threshold) {
        VEC_TRY(c.d_smax.reserve((size_t)kVecQueryBatch * p.msl));
        VEC_TRY(c.d_thr.reserve((size_t)kVecQueryBatch));
        VEC_TRY(c.d_ccnt.reserve((size_t)kVecQueryBatch));
        VEC_TRY(c.d_cand.reserve((size_t)kVecQueryBatch * kVecCandCap));
    }
    return AID_OK;
}

static VecAllowed vec_allowed(const VecAllow &al) {
    return VecAllowed{reinterpret_cast<const uint32_t *>(al.bm), al.fmap, al.words * 2};
}

// The best p.limit keys of each of the batch's nb rows of d_scores, sorted, at (*in)[q * *in_stride ..]. With
// al.bm the entries that count are the ones the batch's allow-bitmaps pass (FPSPEC 9.2), not the live ones.
static int vec_select_batch(VecCatalog &c, int nb, const VecSelPlan &p, const VecAllow &al, hipStream_t s,
                            unsigned long long **in_out, int64_t *in_stride_out) {
    const int64_t ns = (c.n + 31) / 32 * 32;
    const int limit = p.limit, slice = p.slice, keep = p.keep, mslice = p.mslice;
    const int64_t msl = p.msl;
    unsigned long long *in = nullptr;
    int64_t in_stride = 0;
    if (p.by_threshold) {
        int32_t cnt[kVecQueryBatch];
        std::vector<int32_t> cnt_lines(p.q8 ? (size_t)nb * kVecQ8CntStride : 0);
        if (al.bm)
            hipLaunchKernelGGL(k_vec_slice_max<VecAllowed>, dim3((unsigned)msl, (unsigned)nb), dim3(256), 0, s, c.d_scores.p,
                               ns, vec_allowed(al), c.n, mslice, (int)msl, c.d_smax.p);
        else
            hipLaunchKernelGGL(k_vec_slice_max<VecLive>, dim3((unsigned)msl, (unsigned)nb), dim3(256), 0, s, c.d_scores.p, ns,
                               VecLive{c.d_dead.p}, c.n, mslice, (int)msl, c.d_smax.p);
        const int msp = std::max(2, pow2_ceil((int)msl));
        hipLaunchKernelGGL(k_vec_threshold, dim3((unsigned)nb), dim3(256), (size_t)msp * 4, s, c.d_smax.p, (int)msl, msp,
                           limit, c.d_thr.p, c.d_ccnt.p);
        VEC_TRY(hipMemsetAsync(c.d_cand.p, 0, (size_t)nb * kVecCandCap * 8, s));
        if (p.q8) {
            VEC_TRY(hipMemsetAsync(c.d_ccnt.p, 0, (size_t)nb * kVecQ8CntStride * sizeof(int32_t), s));
            if (al.bm)
                vec_q8_filter_allowed(c.d_scores.p, ns, al, c.n, c.d_thr.p, c.d_cand.p, kVecCandCap, c.d_ccnt.p, nb, s);
            else
                vec_q8_filter(c.d_scores.p, ns, c.d_dead.p, c.n, c.d_thr.p, c.d_cand.p, kVecCandCap, c.d_ccnt.p, nb, s);
            VEC_TRY(hipGetLastError());
            VEC_TRY(hipMemcpyAsync(cnt_lines.data(), c.d_ccnt.p, (size_t)nb * kVecQ8CntStride * sizeof(int32_t),
                                   hipMemcpyDeviceToHost, s));
        } else {
            if (al.bm)
                hipLaunchKernelGGL(k_vec_filter<VecAllowed>, dim3((unsigned)((c.n + 2047) / 2048), (unsigned)nb), dim3(256), 0,
                                   s, c.d_scores.p, ns, vec_allowed(al), c.n, c.d_thr.p, c.d_cand.p, kVecCandCap,
                                   c.d_ccnt.p);
            else
                hipLaunchKernelGGL(k_vec_filter<VecLive>, dim3((unsigned)((c.n + 2047) / 2048), (unsigned)nb), dim3(256), 0, s,
                                   c.d_scores.p, ns, VecLive{c.d_dead.p}, c.n, c.d_thr.p, c.d_cand.p, kVecCandCap,
                                   c.d_ccnt.p);
            VEC_TRY(hipGetLastError());
            VEC_TRY(hipMemcpyAsync(cnt, c.d_ccnt.p, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        }
        VEC_TRY(hipStreamSynchronize(s));
        if (p.q8)
            for (int i = 0; i < nb; ++i) cnt[i] = cnt_lines[(size_t)i * kVecQ8CntStride];
        const int most = *std::max_element(cnt, cnt + nb);
        c.st[4] = std::max<int64_t>(c.st[4], most);
        ++c.st[most <= kVecCandCap ? 0 : 2];
        if (most <= kVecCandCap) {  // every list fits: one sort each
            const int one = std::max(2 * pow2_ceil(limit), pow2_ceil(most));  // <= kVecCandCap
            hipLaunchKernelGGL(k_vec_select<VecLive>, dim3(1, (unsigned)nb), dim3(256), (size_t)one * 8, s,
                               (const float *)nullptr, ns, VecLive{c.d_dead.p}, c.d_cand.p, (int64_t)kVecCandCap,
                               (int64_t)one, one, keep, c.d_keys0.p, (int64_t)keep);
            VEC_TRY(hipGetLastError());
            in = c.d_keys0.p;
            in_stride = keep;
        }
    } else {
        ++c.st[1];
    }
    if (!in) {
        int64_t n_in = c.n;
        unsigned long long *out = c.d_keys0.p, *other = c.d_keys1.p;
        for (bool first = true;; first = false) {
            const int64_t nsl = (n_in + slice - 1) / slice;
            const int64_t out_stride = nsl * keep;
            if (first && al.bm)  // only the first pass asks which entries count: the later ones sort its keys
                hipLaunchKernelGGL(k_vec_select<VecAllowed>, dim3((unsigned)nsl, (unsigned)nb), dim3(256),
                                   (size_t)pow2_ceil(slice) * 8, s, c.d_scores.p, ns, vec_allowed(al), in, in_stride, n_in,
                                   slice, keep, out, out_stride);
            else
                hipLaunchKernelGGL(k_vec_select<VecLive>, dim3((unsigned)nsl, (unsigned)nb), dim3(256),
                                   (size_t)pow2_ceil(slice) * 8, s, first ? c.d_scores.p : nullptr, ns, VecLive{c.d_dead.p}, in,
                                   in_stride, n_in, slice, keep, out, out_stride);
            VEC_TRY(hipGetLastError());
            ++c.st[3];
            in = out;
            in_stride = out_stride;
            n_in = out_stride;
            std::swap(out, other);
            if (nsl == 1) break;
        }
    }
    *in_out = in;
    *in_stride_out = in_stride;
    return AID_OK;
}

// Sorted keys of the batch's queries -> the hit columns of queries q0 + i (q0 + qmap[i] with a map).
static int vec_hits_batch(VecCatalog &c, const unsigned long long *in, int64_t in_stride, int keep, int limit, int nb,
                          int q0, const int32_t *qmap, hipStream_t s) {
    hipLaunchKernelGGL(k_vec_hits, dim3((unsigned)nb), dim3(256), 0, s, in, in_stride, keep, limit, c.d_track.p, c.d_off.p,
                       qmap, c.d_hentry.p + (size_t)q0 * limit, c.d_htrack.p + (size_t)q0 * limit,
                       c.d_hscore.p + (size_t)q0 * limit, c.d_hoff.p + (size_t)q0 * limit, c.d_nhits.p + q0);
    VEC_TRY(hipGetLastError());
    return AID_OK;
}

// FPSPEC 9 for one batch: the f32 scan, the selection, the hit columns.
static int vec_f32_batch(VecCatalog &c, const float *dq, int nb, const VecSelPlan &p, int q0, const int32_t *qmap,
                         const VecAllow &al, hipStream_t s) {
    if (int rc = vec_scan_batch(c, dq, nb, s)) return rc;
    unsigned long long *in = nullptr;
    int64_t in_stride = 0;
    if (int rc = vec_select_batch(c, nb, p, al, s, &in, &in_stride)) return rc;
    return vec_hits_batch(c, in, in_stride, p.keep, p.limit, nb, q0, qmap, s);
}

// ---- filtered search (FPSPEC 9.2). A call with filters plans all its batches first (c.h_fplans, empty for an
// unfiltered call), brings the tags column up to date and reserves the scratch; each filtered batch then stages its
// distinct filters and runs K9f before its selection.
static int vec_filters_begin(VecCatalog &c, const aid_vec_filter *filters, int nq, hipStream_t s) {
    c.h_fplans.clear();
    if (!filters || c.n == 0) return AID_OK;
    bool any = false;
    for (int q0 = 0; q0 < nq; q0 += kVecQueryBatch) {
        c.h_fplans.emplace_back();
        vec_filter_plan(filters + q0, std::min(kVecQueryBatch, nq - q0), c.h_fplans.back());
        any = any || c.h_fplans.back().filtered;
    }
    if (!any) {
        c.h_fplans.clear();
        return AID_OK;
    }
    if (c.d_tags.n < (size_t)c.n) {
        VEC_TRY(c.d_tags.reserve((size_t)c.cap_rows));
        c.tags_on_dev = 0;
    }
    if (c.tags_on_dev < c.n) {
        VEC_TRY(hipMemcpyAsync(c.d_tags.p + c.tags_on_dev, c.h_tags.data() + c.tags_on_dev,
                               (size_t)(c.n - c.tags_on_dev) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        VEC_TRY(hipStreamSynchronize(s));
        c.tags_on_dev = c.n;
    }
    VEC_TRY(c.d_filters.reserve((size_t)kVecQueryBatch));
    VEC_TRY(c.d_fmap.reserve((size_t)kVecQueryBatch));
    VEC_TRY(c.d_fmap_fb.reserve((size_t)kVecQueryBatch));
    VEC_TRY(c.d_allow.reserve((size_t)kVecQueryBatch * vec_allow_words(c.n)));
    return AID_OK;
}

// The allow-bitmaps of batch b of the call; `al` stays empty for an unfiltered batch, which then takes FPSPEC 9's
// kernels on their arguments.
static int vec_allow_batch(VecCatalog &c, size_t b, hipStream_t s, VecAllow &al) {
    al = VecAllow{};
    if (b >= c.h_fplans.size() || !c.h_fplans[b].filtered) return AID_OK;
    const VecFilterPlan &p = c.h_fplans[b];
    VEC_TRY(hipMemcpyAsync(c.d_filters.p, p.distinct, (size_t)p.n_distinct * sizeof(aid_vec_filter), hipMemcpyHostToDevice, s));
    VEC_TRY(hipMemcpyAsync(c.d_fmap.p, p.fmap, sizeof p.fmap, hipMemcpyHostToDevice, s));
    vec_allow(c.d_dead.p, c.d_track.p, c.d_tags.p, c.n, c.d_filters.p, p.n_distinct, c.d_allow.p, s);
    VEC_TRY(hipGetLastError());
    al.bm = c.d_allow.p;
    al.fmap = c.d_fmap.p;
    al.words = vec_allow_words(c.n);
    return AID_OK;
}

// Normalise queries [q0, q0 + nb) into c.d_q, quantise the tiles (FPSPEC 9.1) into d_q8 / d_qs / d_qe and score
// them against the int8 catalog: approx into c.d_scores [nb rounded up to 32][ns].
static int vec_q8_scan_batch(VecCatalog &c, const float *dq, int nb, hipStream_t s) {
    const int dim = c.dim;
    const int nqt = (nb + 31) / 32;
    const int64_t n_tiles = (c.n + 31) / 32, ns = n_tiles * 32;
    VEC_TRY(c.d_q8.reserve((size_t)kVecQueryBatch * dim));
    VEC_TRY(c.d_qs.reserve((size_t)kVecQueryBatch));
    VEC_TRY(c.d_qe.reserve((size_t)kVecQueryBatch));
    VEC_TRY(hipMemsetAsync(c.d_q.p, 0, (size_t)nqt * 32 * dim * sizeof(float), s));
    hipLaunchKernelGGL(k_vec_normalize, dim3((unsigned)nb), dim3(64), 0, s, dq, (int64_t)nb, dim, c.d_q.p,
                       (int64_t)0);
    vec_q8_quantize(c.d_q.p, 0, (int64_t)nqt * 32, dim, c.d_q8.p, c.d_qs.p, c.d_qe.p, s);  // the zero rows too
    const int chunk = c.force_chunk ? c.force_chunk : kVecScanChunk;
    vec_q8_scan(c.d_v8.p, c.d_s8.p, n_tiles, std::max(1, chunk / 32), c.d_q8.p, c.d_qs.p, nqt, dim, c.d_scores.p, ns, s);
    ++c.q8st[5];
    VEC_TRY(hipGetLastError());
    return AID_OK;
}

// FPSPEC 9.1 for all nq queries: per batch the int8 scan, the R best by approx rescored, tau and the threshold, W,
// W rescored and sorted; the queries whose W is over the cap go through vec_f32_batch as a tile of their own.
static int vec_search_q8(VecCatalog &c, const float *dq, int nq, const VecSelPlan &pl, hipStream_t s) {
    const int limit = pl.limit, dim = c.dim;
    const int64_t ns = (c.n + 31) / 32 * 32;
    const int R = vec_q8_candidates(limit, c.q8_over);
    const int wcap = c.force_cand ? c.force_cand : kVecCandCap;
    VecSelPlan pr;
    if (int rc = vec_sel_plan(c, R, pr)) return rc;
    pr.q8 = true;
    VEC_TRY(c.d_thr.reserve((size_t)kVecQueryBatch));
    VEC_TRY(c.d_ccnt.reserve((size_t)kVecQueryBatch * kVecQ8CntStride));
    VEC_TRY(c.d_cand.reserve((size_t)kVecQueryBatch * kVecCandCap));
    const int64_t r_live = std::min<int64_t>(R, c.n_live);
    for (int q0 = 0; q0 < nq; q0 += kVecQueryBatch) {
        const int nb = std::min(kVecQueryBatch, nq - q0);
        const float *dqb = dq + (size_t)q0 * dim;
        VecAllow al;  // FPSPEC 9.2: "live" reads "passes" in the first stage, in W and in the fallback
        if (int rc = vec_allow_batch(c, (size_t)(q0 / kVecQueryBatch), s, al)) return rc;
        if (int rc = vec_q8_scan_batch(c, dqb, nb, s)) return rc;
        unsigned long long *in = nullptr;
        int64_t in_stride = 0;
        if (int rc = vec_select_batch(c, nb, pr, al, s, &in, &in_stride)) return rc;  // the R best by approx
        VEC_TRY(vec_q8_rescore(c.d_vecs.p, c.d_q.p, dim, in, in_stride, R, nullptr, 0, nb, s));
        vec_q8_tau(in, in_stride, R, limit, c.d_qe.p, c.q8_E, dim, c.d_thr.p, c.d_ccnt.p, nb, s);
        VEC_TRY(hipMemsetAsync(c.d_cand.p, 0, (size_t)nb * kVecCandCap * 8, s));
        if (al.bm)
            vec_q8_filter_allowed(c.d_scores.p, ns, al, c.n, c.d_thr.p, c.d_cand.p, kVecCandCap, c.d_ccnt.p, nb, s);
        else
            vec_q8_filter(c.d_scores.p, ns, c.d_dead.p, c.n, c.d_thr.p, c.d_cand.p, kVecCandCap, c.d_ccnt.p, nb, s);
        VEC_TRY(hipGetLastError());
        int32_t cnt[kVecQueryBatch], fb[kVecQueryBatch];
        std::vector<int32_t> cnt_lines((size_t)nb * kVecQ8CntStride);
        VEC_TRY(hipMemcpyAsync(cnt_lines.data(), c.d_ccnt.p, cnt_lines.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        VEC_TRY(hipStreamSynchronize(s));
        for (int i = 0; i < nb; ++i) cnt[i] = cnt_lines[(size_t)i * kVecQ8CntStride];
        int nfb = 0, most = 0;
        c.q8st[4] += r_live * nb;
        for (int i = 0; i < nb; ++i) {  // cnt[i] = |W| of query q0 + i
            c.q8st[2] += cnt[i];
            c.q8st[3] = std::max<int64_t>(c.q8st[3], cnt[i]);
            if (cnt[i] > wcap) {
                fb[nfb++] = i;
            } else {
                most = std::max(most, cnt[i]);
                c.q8st[4] += cnt[i];
            }
        }
        c.q8st[0] += nb - nfb;
        c.q8st[1] += nfb;
        if (nfb < nb) {
            VEC_TRY(vec_q8_rescore(c.d_vecs.p, c.d_q.p, dim, c.d_cand.p, kVecCandCap, most, c.d_ccnt.p, wcap, nb, s));
            const int one = std::max(2 * pow2_ceil(limit), pow2_ceil(most));  // <= kVecCandCap
            hipLaunchKernelGGL(k_vec_select<VecLive>, dim3(1, (unsigned)nb), dim3(256), (size_t)one * 8, s,
                               (const float *)nullptr, ns, VecLive{c.d_dead.p}, c.d_cand.p, (int64_t)kVecCandCap,
                               (int64_t)one, one, pl.keep, c.d_keys0.p, (int64_t)pl.keep);
            VEC_TRY(hipGetLastError());
            // the columns of a query that fell back hold an unfinished list until the f32 route rewrites them below
            if (int rc = vec_hits_batch(c, c.d_keys0.p, pl.keep, pl.keep, limit, nb, q0, nullptr, s)) return rc;
        }
        if (nfb) {
            VEC_TRY(c.d_fbq.reserve((size_t)kVecQueryBatch * dim));
            VEC_TRY(c.d_qmap.reserve((size_t)kVecQueryBatch));
            for (int j = 0; j < nfb; ++j)
                VEC_TRY(hipMemcpyAsync(c.d_fbq.p + (size_t)j * dim, dqb + (size_t)fb[j] * dim, (size_t)dim * sizeof(float),
                                       hipMemcpyDeviceToDevice, s));
            VEC_TRY(hipMemcpyAsync(c.d_qmap.p, fb, (size_t)nfb * sizeof(int32_t), hipMemcpyHostToDevice, s));
            VecAllow al_fb = al;
            if (al.bm) {  // query j of the tile is query fb[j] of the batch: it keeps that query's bitmap
                const VecFilterPlan &fp = c.h_fplans[(size_t)(q0 / kVecQueryBatch)];
                for (int j = 0; j < nfb; ++j) c.h_fmap_fb[j] = fp.fmap[fb[j]];
                VEC_TRY(hipMemcpyAsync(c.d_fmap_fb.p, c.h_fmap_fb, (size_t)nfb * sizeof(int32_t), hipMemcpyHostToDevice, s));
                al_fb.fmap = c.d_fmap_fb.p;
            }
            VEC_TRY(hipStreamSynchronize(s));
            if (int rc = vec_f32_batch(c, c.d_fbq.p, nfb, pl, q0, c.d_qmap.p, al_fb, s)) return rc;
        }
    }
    return AID_OK;
}

// Hit columns of all nq queries on the device: d_hentry / d_htrack / d_hscore / d_hoff [nq][limit], d_nhits [nq].
static int vec_search_dev(VecCatalog &c, const float *queries, int nq, int location, int limit,
                          const aid_vec_filter *filters, hipStream_t s) {
    const size_t nh = (size_t)nq * limit;
    VEC_TRY(c.d_hentry.reserve(nh));
    VEC_TRY(c.d_htrack.reserve(nh));
    VEC_TRY(c.d_hscore.reserve(nh));
    VEC_TRY(c.d_hoff.reserve(nh));
    VEC_TRY(c.d_nhits.reserve((size_t)nq));
    VEC_TRY(hipMemsetAsync(c.d_nhits.p, 0, (size_t)nq * sizeof(int32_t), s));
    if (c.n == 0) return AID_OK;
    const float *dq = nullptr;
    if (int rc = vec_stage_queries(c, queries, nq, location, s, &dq)) return rc;
    VecSelPlan pl;
    if (int rc = vec_sel_plan(c, limit, pl)) return rc;
    if (int rc = vec_filters_begin(c, filters, nq, s)) return rc;
    if (c.q8_mode) return vec_search_q8(c, dq, nq, pl, s);
    for (int q0 = 0; q0 < nq; q0 += kVecQueryBatch) {
        const int nb = std::min(kVecQueryBatch, nq - q0);
        VecAllow al;
        if (int rc = vec_allow_batch(c, (size_t)(q0 / kVecQueryBatch), s, al)) return rc;
        if (int rc = vec_f32_batch(c, dq + (size_t)q0 * c.dim, nb, pl, q0, nullptr, al, s)) return rc;
    }
    return AID_OK;
}

static int vec_filter_args(VecCatalog &c, const char *what, const aid_vec_filter *filters, int nq) {
    if (filters && nq > 0)
        if (const int bad = vec_filters_invalid(filters, nq))
            return vfail(c, AID_ERR_INVALID, std::string(what) + ": filter " + std::to_string(bad - 1) +
                                                 " excludes more than 8 tracks");
    return AID_OK;
}

int vec_search(VecCatalog &c, const float *queries, int nq, int location, int limit, const aid_vec_filter *filters,
               aid_vec_hit *hits, int32_t *n_hits, hipStream_t s) {
    if (int rc = vec_query_args(c, "aid_vec_search", queries, nq, location)) return rc;
    if (limit < 1 || limit > kVecMaxLimit || (nq > 0 && (!hits || !n_hits)))
        return vfail(c, AID_ERR_INVALID, "aid_vec_search: limit must be in [1, 1024] and hits, n_hits non-null");
    if (int rc = vec_filter_args(c, "aid_vec_search_filtered", filters, nq)) return rc;
    if (nq == 0) return AID_OK;
    if (int rc = vec_search_dev(c, queries, nq, location, limit, filters, s)) return rc;
    const size_t nh = (size_t)nq * limit;
    std::vector<uint32_t> he(nh);
    std::vector<float> hs(nh);
    VEC_TRY(hipMemcpyAsync(he.data(), c.d_hentry.p, nh * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    VEC_TRY(hipMemcpyAsync(hs.data(), c.d_hscore.p, nh * sizeof(float), hipMemcpyDeviceToHost, s));
    VEC_TRY(hipMemcpyAsync(n_hits, c.d_nhits.p, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    VEC_TRY(hipStreamSynchronize(s));
    for (int q = 0; q < nq; ++q)
        for (int i = 0; i < n_hits[q]; ++i) {
            const size_t o = (size_t)q * limit + i;
            const uint32_t e = he[o];
            aid_vec_hit h;
            h.entry = e;
            h.track = c.h_track[e];
            h.chunk_index = c.h_chunk[e];
            h.score = hs[o];
            h.offset_sec = c.h_off[e];
            hits[o] = h;
        }
    return AID_OK;
}

int vec_scores(VecCatalog &c, const float *queries, int nq, int location, float *out, int64_t cap, hipStream_t s) {
    if (int rc = vec_query_args(c, "aid_vec_scores", queries, nq, location)) return rc;
    if (cap < (int64_t)nq * c.n || (nq > 0 && c.n > 0 && !out))
        return vfail(c, AID_ERR_INVALID, "aid_vec_scores: out holds fewer than nq * n_entries floats");
    if (nq == 0 || c.n == 0) return AID_OK;
    const float *dq = nullptr;
    if (int rc = vec_stage_queries(c, queries, nq, location, s, &dq)) return rc;
    const int64_t ns = (c.n + 31) / 32 * 32;
    for (int q0 = 0; q0 < nq; q0 += kVecQueryBatch) {
        const int nb = std::min(kVecQueryBatch, nq - q0);
        if (int rc = vec_scan_batch(c, dq + (size_t)q0 * c.dim, nb, s)) return rc;
        VEC_TRY(hipMemcpy2DAsync(out + (size_t)q0 * c.n, c.n * sizeof(float), c.d_scores.p, ns * sizeof(float),
                                 c.n * sizeof(float), nb, hipMemcpyDeviceToHost, s));
        VEC_TRY(hipStreamSynchronize(s));
    }
    return AID_OK;
}

int vec_scores_i8(VecCatalog &c, const float *queries, int nq, int location, float *approx_out, double *eps_out,
                  int64_t cap, hipStream_t s) {
    if (int rc = vec_query_args(c, "aid_vec_scores_i8", queries, nq, location)) return rc;
    if (!c.q8_mode) return vfail(c, AID_ERR_STATE, "aid_vec_scores_i8: the prefilter is off (aid_vec_prefilter)");
    if (cap < (int64_t)nq * c.n || (nq > 0 && c.n > 0 && !approx_out) || (nq > 0 && !eps_out))
        return vfail(c, AID_ERR_INVALID, "aid_vec_scores_i8: approx_out holds fewer than nq * n_entries floats, or null eps_out");
    if (nq == 0) return AID_OK;
    const float *dq = nullptr;
    if (int rc = vec_stage_queries(c, queries, nq, location, s, &dq)) return rc;
    if (c.n == 0) {  // no int8 planes yet: normalise and quantise the queries alone
        VEC_TRY(c.d_q8.reserve((size_t)kVecQueryBatch * c.dim));
        VEC_TRY(c.d_qs.reserve((size_t)kVecQueryBatch));
        VEC_TRY(c.d_qe.reserve((size_t)kVecQueryBatch));
    }
    const int64_t ns = (c.n + 31) / 32 * 32;
    for (int q0 = 0; q0 < nq; q0 += kVecQueryBatch) {
        const int nb = std::min(kVecQueryBatch, nq - q0);
        float qe[kVecQueryBatch];
        if (c.n) {
            if (int rc = vec_q8_scan_batch(c, dq + (size_t)q0 * c.dim, nb, s)) return rc;
            VEC_TRY(hipMemcpy2DAsync(approx_out + (size_t)q0 * c.n, c.n * sizeof(float), c.d_scores.p, ns * sizeof(float),
                                     c.n * sizeof(float), nb, hipMemcpyDeviceToHost, s));
        } else {
            const int nqt = (nb + 31) / 32;
            VEC_TRY(hipMemsetAsync(c.d_q.p, 0, (size_t)nqt * 32 * c.dim * sizeof(float), s));
            hipLaunchKernelGGL(k_vec_normalize, dim3((unsigned)nb), dim3(64), 0, s, dq + (size_t)q0 * c.dim, (int64_t)nb,
                               c.dim, c.d_q.p, (int64_t)0);
            vec_q8_quantize(c.d_q.p, 0, (int64_t)nqt * 32, c.dim, c.d_q8.p, c.d_qs.p, c.d_qe.p, s);
            VEC_TRY(hipGetLastError());
        }
        VEC_TRY(hipMemcpyAsync(qe, c.d_qe.p, (size_t)nb * sizeof(float), hipMemcpyDeviceToHost, s));
        VEC_TRY(hipStreamSynchronize(s));
        for (int i = 0; i < nb; ++i) eps_out[q0 + i] = vec_q8_eps(qe[i], c.q8_E, c.dim);
    }
    return AID_OK;
}

static int vec_agg_args(VecCatalog &c, const char *what, int top_k, int max_out, int nq, const void *out, const void *n_out) {
    if (top_k < 1 || max_out < 1 || (nq > 0 && (!out || !n_out)))
        return vfail(c, AID_ERR_INVALID, std::string(what) + ": top_k_per_track and max_out must be >= 1, out and n_out non-null");
    return AID_OK;
}

// Run the aggregation over device hit columns and copy the rows out.
static int vec_agg_run(VecCatalog &c, const uint32_t *track, const float *score, const double *off, const int64_t *start,
                       const int32_t *count, int64_t stride, int nq, int top_k, double weight, const uint32_t *exclude,
                       double threshold, int max_out, aid_vibe_row *out, int32_t *n_out, hipStream_t s) {
    const uint32_t *dex = nullptr;
    if (exclude) {
        VEC_TRY(c.d_excl.reserve((size_t)nq));
        VEC_TRY(hipMemcpyAsync(c.d_excl.p, exclude, (size_t)nq * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        dex = c.d_excl.p;
    }
    VEC_TRY(c.d_rows.reserve((size_t)nq * max_out));
    VEC_TRY(c.d_nout.reserve((size_t)nq));
    hipLaunchKernelGGL(k_vec_aggregate, dim3((unsigned)nq), dim3(64), 0, s, track, score, off, start, count, stride, top_k,
                       weight, dex, threshold, max_out, c.d_rows.p, c.d_nout.p);
    VEC_TRY(hipGetLastError());
    VEC_TRY(hipMemcpyAsync(n_out, c.d_nout.p, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    VEC_TRY(hipStreamSynchronize(s));
    for (int q = 0; q < nq; ++q)
        if (n_out[q] > 0)
            VEC_TRY(hipMemcpyAsync(out + (size_t)q * max_out, c.d_rows.p + (size_t)q * max_out,
                                   (size_t)n_out[q] * sizeof(aid_vibe_row), hipMemcpyDeviceToHost, s));
    VEC_TRY(hipStreamSynchronize(s));
    return AID_OK;
}

int vec_aggregate(VecCatalog &c, const aid_vec_hit *hits, const int64_t *hoff, int nq, int top_k, double weight,
                  const uint32_t *exclude, double threshold, int max_out, aid_vibe_row *out, int32_t *n_out,
                  hipStream_t s) {
    if (nq < 0 || (nq > 0 && !hoff)) return vfail(c, AID_ERR_INVALID, "aid_vec_aggregate: bad argument");
    if (int rc = vec_agg_args(c, "aid_vec_aggregate", top_k, max_out, nq, out, n_out)) return rc;
    if (nq == 0) return AID_OK;
    if (hoff[0] != 0) return vfail(c, AID_ERR_INVALID, "aid_vec_aggregate: hoff[0] must be 0");
    std::vector<int32_t> cnt(nq);
    for (int q = 0; q < nq; ++q) {
        const int64_t m = hoff[q + 1] - hoff[q];
        if (m < 0 || m > kVecMaxLimit)
            return vfail(c, AID_ERR_INVALID, "aid_vec_aggregate: a hit list holds 0 to 1024 hits, hoff non-decreasing");
        cnt[q] = (int32_t)m;
    }
    const int64_t nh = hoff[nq];
    if (nh > 0 && !hits) return vfail(c, AID_ERR_INVALID, "aid_vec_aggregate: null hits");
    std::vector<uint32_t> tr((size_t)nh);
    std::vector<float> sc((size_t)nh);
    std::vector<double> of((size_t)nh);
    for (int64_t i = 0; i < nh; ++i) {
        tr[i] = hits[i].track;
        sc[i] = hits[i].score;
        of[i] = hits[i].offset_sec;
    }
    const size_t cap = (size_t)std::max<int64_t>(nh, 1);
    VEC_TRY(c.d_htrack.reserve(cap));
    VEC_TRY(c.d_hscore.reserve(cap));
    VEC_TRY(c.d_hoff.reserve(cap));
    VEC_TRY(c.d_start.reserve((size_t)nq + 1));
    VEC_TRY(c.d_cnt.reserve((size_t)nq));
    if (nh) {
        VEC_TRY(hipMemcpyAsync(c.d_htrack.p, tr.data(), nh * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        VEC_TRY(hipMemcpyAsync(c.d_hscore.p, sc.data(), nh * sizeof(float), hipMemcpyHostToDevice, s));
        VEC_TRY(hipMemcpyAsync(c.d_hoff.p, of.data(), nh * sizeof(double), hipMemcpyHostToDevice, s));
    }
    VEC_TRY(hipMemcpyAsync(c.d_start.p, hoff, ((size_t)nq + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    VEC_TRY(hipMemcpyAsync(c.d_cnt.p, cnt.data(), (size_t)nq * sizeof(int32_t), hipMemcpyHostToDevice, s));
    return vec_agg_run(c, c.d_htrack.p, c.d_hscore.p, c.d_hoff.p, c.d_start.p, c.d_cnt.p, 0, nq, top_k, weight, exclude,
                       threshold, max_out, out, n_out, s);
}

int vec_lane(VecCatalog &c, const float *queries, int nq, int location, int limit, int top_k, double weight,
             const aid_vec_filter *filters, const uint32_t *exclude, double threshold, int max_out, aid_vibe_row *out,
             int32_t *n_out, hipStream_t s) {
    if (int rc = vec_query_args(c, "aid_vibe_lane", queries, nq, location)) return rc;
    if (limit < 1 || limit > kVecMaxLimit) return vfail(c, AID_ERR_INVALID, "aid_vibe_lane: limit must be in [1, 1024]");
    if (int rc = vec_agg_args(c, "aid_vibe_lane", top_k, max_out, nq, out, n_out)) return rc;
    if (int rc = vec_filter_args(c, "aid_vibe_lane_filtered", filters, nq)) return rc;
    if (nq == 0) return AID_OK;
    if (int rc = vec_search_dev(c, queries, nq, location, limit, filters, s)) return rc;
    return vec_agg_run(c, c.d_htrack.p, c.d_hscore.p, c.d_hoff.p, nullptr, c.d_nhits.p, limit, nq, top_k, weight, exclude,
                       threshold, max_out, out, n_out, s);
}

// ---- persistence: magic, version, dim, n, then the tiles of ceil(n / 32) * 32 rows as stored, tracks, chunk
// indices, offsets, tombstones, and in version 2 the tags (FPSPEC 9.2)
namespace {
struct VecFileHeader {
    char magic[8];
    uint32_t version;
    int32_t dim;
    int64_t n;
};
const char kVecMagic[8] = {'A', 'I', 'D', 'F', 'P', 'V', 'C', '1'};
}  // namespace

int vec_save(VecCatalog &c, const char *path, hipStream_t s) {
    if (!path) return vfail(c, AID_ERR_INVALID, "aid_vec_save: null path");
    if (!c.dim) return vfail(c, AID_ERR_STATE, "aid_vec_save: call aid_vec_reset first");
    const size_t nf = (size_t)((c.n + 31) / 32) * 32 * c.dim;
    std::vector<float> v(nf);
    if (nf) {
        VEC_TRY(hipMemcpyAsync(v.data(), c.d_vecs.p, nf * sizeof(float), hipMemcpyDeviceToHost, s));
        VEC_TRY(hipStreamSynchronize(s));
    }
    FILE *f = fopen(path, "wb");
    if (!f) return vfail(c, AID_ERR_INVALID, std::string("aid_vec_save: cannot open ") + path);
    VecFileHeader h;
    memcpy(h.magic, kVecMagic, 8);
    // version 2 = version 1 with the tags column (FPSPEC 9.2) after the tombstones; a catalog without a tag saves
    // the file it always saved
    const bool tagged = std::any_of(c.h_tags.begin(), c.h_tags.end(), [](uint64_t t) { return t != 0; });
    h.version = tagged ? 2 : 1;
    h.dim = c.dim;
    h.n = c.n;
    const size_t n = (size_t)c.n;
    bool ok = fwrite(&h, sizeof h, 1, f) == 1;
    ok = ok && (!nf || fwrite(v.data(), sizeof(float), nf, f) == nf);
    ok = ok && (!n || (fwrite(c.h_track.data(), 4, n, f) == n && fwrite(c.h_chunk.data(), 4, n, f) == n &&
                       fwrite(c.h_off.data(), 8, n, f) == n && fwrite(c.h_dead.data(), 1, n, f) == n));
    ok = ok && (!tagged || fwrite(c.h_tags.data(), 8, n, f) == n);
    ok = (fclose(f) == 0) && ok;
    if (!ok) return vfail(c, AID_ERR_INVALID, std::string("aid_vec_save: write failed: ") + path);
    return AID_OK;
}

int vec_load(VecCatalog &c, const char *path, hipStream_t s) {
    if (!path) return vfail(c, AID_ERR_INVALID, "aid_vec_load: null path");
    FILE *f = fopen(path, "rb");
    if (!f) return vfail(c, AID_ERR_INVALID, std::string("aid_vec_load: cannot open ") + path);
    VecFileHeader h;
    bool ok = fread(&h, sizeof h, 1, f) == 1 && memcmp(h.magic, kVecMagic, 8) == 0 && (h.version == 1 || h.version == 2) &&
              vec_dim_ok(h.dim) && h.n >= 0 && h.n < 0xFFFFFFFFll;
    std::vector<uint64_t> tg;
    std::vector<float> v;
    std::vector<uint32_t> tr;
    std::vector<int32_t> ch;
    std::vector<double> of;
    std::vector<uint8_t> dead;
    if (ok) {
        const size_t n = (size_t)h.n, nf = (size_t)((h.n + 31) / 32) * 32 * h.dim;
        const long want = (long)(sizeof h + nf * 4 + n * (h.version == 2 ? 25 : 17));
        ok = fseek(f, 0, SEEK_END) == 0 && ftell(f) == want && fseek(f, (long)sizeof h, SEEK_SET) == 0;
        if (ok) {
            v.resize(nf);
            tr.resize(n);
            ch.resize(n);
            of.resize(n);
            dead.resize(n);
            ok = (!nf || fread(v.data(), 4, nf, f) == nf) &&
                 (!n || (fread(tr.data(), 4, n, f) == n && fread(ch.data(), 4, n, f) == n &&
                         fread(of.data(), 8, n, f) == n && fread(dead.data(), 1, n, f) == n));
            tg.assign(n, 0);  // version 1: no entry is tagged
            ok = ok && (h.version != 2 || !n || fread(tg.data(), 8, n, f) == n);
        }
    }
    fclose(f);
    if (!ok) return vfail(c, AID_ERR_INVALID, std::string("aid_vec_load: not an AIDFPVC1 file, or truncated: ") + path);
    // the file is whole: replace the catalog
    if (int rc = vec_reset(c, h.dim)) return rc;
    if (h.n == 0) return AID_OK;
    if (int rc = vec_grow(c, h.n, s)) return rc;
    VEC_TRY(hipMemcpyAsync(c.d_vecs.p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice, s));
    VEC_TRY(hipMemcpyAsync(c.d_track.p, tr.data(), tr.size() * 4, hipMemcpyHostToDevice, s));
    VEC_TRY(hipMemcpyAsync(c.d_off.p, of.data(), of.size() * 8, hipMemcpyHostToDevice, s));
    VEC_TRY(hipMemcpyAsync(c.d_dead.p, dead.data(), dead.size(), hipMemcpyHostToDevice, s));
    VEC_TRY(hipStreamSynchronize(s));
    c.n = h.n;
    c.n_live = 0;
    for (uint8_t &d : dead) {
        d = d ? 1 : 0;
        c.n_live += !d;
    }
    c.h_track.swap(tr);
    c.h_chunk.swap(ch);
    c.h_off.swap(of);
    c.h_dead.swap(dead);
    c.h_tags.swap(tg);
    if (c.q8_mode) return vec_q8_rebuild(c, s);  // the file holds no int8 form: it follows from the f32 rows
    return AID_OK;
}

}  // namespace aid
