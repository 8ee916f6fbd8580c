// aidfp_vector.h -- the vector lane's catalog (spec/FPSPEC.md 9, K9): host state and entry points of
// csrc/vector.hip. struct aid_engine (engine_internal.h) owns one VecCatalog; engine.cpp calls these under the
// engine lock with the engine's device current; every function returns AID_OK or an AID_ERR_* code and leaves its
// message in `err`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/aidfp.h"
#include "aidfp_buffers.h"
#include "aidfp_vector_filter.h"
#include "aidfp_vector_q8.h"

namespace aid {

constexpr int kVecMaxLimit = 1024;      // hits per query, and hits per list of aid_vec_aggregate
constexpr int kVecQueryBatch = 64;      // queries per scan + selection pass: bounds the score and key scratch
constexpr int kVecScanChunk = 1024;     // default catalog rows per scan workgroup (8 waves, 4 tiles each)
constexpr int kVecMaxSlice = 1024;      // default entries per slice maximum of the threshold route
constexpr int kVecCandCap = 4096;       // candidates per query of the threshold route (one sort in LDS)
constexpr int kVecSelectSlice = 4096;   // default keys per selection workgroup (one bitonic sort in LDS)
constexpr int kVecStats = 8;            // counters of aid_vec_stats

// Stored layout of a [rows][dim] matrix (catalog and query tiles alike): rows in tiles of 32, and within a tile
// the float at (row i, k) sits at ((k >> 3) * 2 + (k & 1)) * 128 + i * 4 + ((k & 7) >> 1). Lane (i, h) of a wave
// fetches the operands of four consecutive 32x32x2 MFMA steps (k = 8g + h + {0, 2, 4, 6}) with one aligned 16-byte
// load, and the 64 lanes of a wave read 1 KB contiguous.
inline size_t vec_layout_index(int64_t row, int k, int dim) {
    return (size_t)(row >> 5) * 32 * dim + (size_t)(((k >> 3) * 2 + (k & 1)) * 128 + (int)(row & 31) * 4 + ((k & 7) >> 1));
}

// The allow-bitmaps of one filtered batch on the device (FPSPEC 9.2): bitmap d is words [d * words, (d + 1) * words)
// of bm, and query q of the batch (or of a fallback tile) uses bitmap fmap[q]. bm == nullptr: the batch is unfiltered.
struct VecAllow {
    const unsigned long long *bm = nullptr;
    const int32_t *fmap = nullptr;
    int64_t words = 0;
};

struct VecCatalog {
    int dim = 0;  // 0 until aid_vec_reset
    int64_t n = 0, n_live = 0;
    int64_t cap_rows = 0;  // multiple of 32; rows [n, cap_rows) of d_vecs are +0
    DevBuf<float> d_vecs;
    DevBuf<uint32_t, 64> d_track;
    DevBuf<double, 64> d_off;
    DevBuf<uint8_t, 64> d_dead;
    std::vector<uint32_t> h_track;  // host mirror of the payload columns (hits are filled from it)
    std::vector<int32_t> h_chunk;
    std::vector<double> h_off;
    std::vector<uint8_t> h_dead;
    // FPSPEC 9.2: the tags column. The host mirror is the truth; rows [0, tags_on_dev) of d_tags are current, and a
    // filtered call brings the rest up before it runs k_vec_allow, so an unfiltered catalog never holds the column
    std::vector<uint64_t> h_tags;
    DevBuf<uint64_t, 64> d_tags;
    int64_t tags_on_dev = 0;
    // a filtered call: the plans of its batches (the sources of the staging copies, so they live as long as the
    // call), the batch's distinct filters, allow-bitmaps and query -> bitmap maps (the second for a fallback tile)
    std::vector<VecFilterPlan> h_fplans;
    DevBuf<aid_vec_filter, 64> d_filters;
    DevBuf<unsigned long long, 64> d_allow;
    DevBuf<int32_t, 64> d_fmap, d_fmap_fb;
    int32_t h_fmap_fb[kVecQueryBatch] = {};
    int force_path = 0;   // AID_FORCE_VEC_PATH
    int force_chunk = 0;  // AID_FORCE_VEC_CHUNK
    // aid_vec_stats, in its order: batches by threshold, not eligible, overflowed; slice-route select launches;
    // largest candidate count; reallocations that copied rows; MFMA and VALU scan launches
    int64_t st[kVecStats] = {};
    // int8 prefilter (FPSPEC 9.1), off by default. While it is on, the planes below mirror rows [0, n) of d_vecs:
    // int8 rows in the layout of aidfp_vector_q8.h, their scales s and residuals e (both also on the host), and E =
    // the largest e. q8_rows = the rows the planes were built for (cap_rows, or 0 = not built)
    int q8_mode = 0;      // aid_vec_prefilter: 0 off, 1 int8
    int q8_over = 4;      // oversample
    int force_cand = 0;   // AID_FORCE_VEC_CAND
    int64_t q8_rows = 0;
    float q8_E = 0.0f;
    DevBuf<int8_t, 64> d_v8;
    DevBuf<float, 64> d_s8, d_e8;
    std::vector<float> h_s8, h_e8;
    // aid_vec_prefilter_stats, in its order: queries answered by the prefilter, queries that fell back to the f32
    // scan, total |W|, largest |W|, rescored pairs, int8 scan launches
    int64_t q8st[kVecQ8Stats] = {};
    DevBuf<int8_t, 64> d_q8;
    DevBuf<float, 64> d_qs, d_qe, d_fbq;
    DevBuf<int32_t, 64> d_qmap;
    // scratch
    DevBuf<float, 64> d_raw, d_q, d_scores;
    DevBuf<unsigned long long, 64> d_keys0, d_keys1, d_cand;
    DevBuf<uint32_t, 64> d_smax, d_thr;
    DevBuf<int32_t, 64> d_ccnt;
    DevBuf<uint32_t, 64> d_hentry, d_htrack, d_excl;
    DevBuf<float, 64> d_hscore;
    DevBuf<double, 64> d_hoff;
    DevBuf<int32_t, 64> d_nhits, d_cnt, d_nout;
    DevBuf<int64_t, 64> d_start;
    DevBuf<aid_vibe_row, 64> d_rows;
    std::string err;
};

int vec_reset(VecCatalog &c, int dim);
int vec_add(VecCatalog &c, const float *vecs, const uint32_t *tracks, const int32_t *chunk_index, const double *offset_sec,
            const uint64_t *tags, int64_t n, int location, hipStream_t s);
int vec_retag(VecCatalog &c, uint32_t track, uint64_t tags);
int vec_tags(VecCatalog &c, uint64_t *out, int64_t cap);
int vec_remove(VecCatalog &c, uint32_t track, hipStream_t s);
int vec_compact(VecCatalog &c, int64_t *n_removed, hipStream_t s);
// filters: host [nq] or null (FPSPEC 9.2), here and in vec_lane
int vec_search(VecCatalog &c, const float *queries, int nq, int location, int limit, const aid_vec_filter *filters,
               aid_vec_hit *hits, int32_t *n_hits, hipStream_t s);
int vec_scores(VecCatalog &c, const float *queries, int nq, int location, float *out, int64_t cap, hipStream_t s);
int vec_aggregate(VecCatalog &c, const aid_vec_hit *hits, const int64_t *hoff, int nq, int top_k, double weight,
                  const uint32_t *exclude, double threshold, int max_out, aid_vibe_row *out, int32_t *n_out,
                  hipStream_t s);
int vec_lane(VecCatalog &c, const float *queries, int nq, int location, int limit, int top_k, double weight,
             const aid_vec_filter *filters, const uint32_t *exclude, double threshold, int max_out, aid_vibe_row *out,
             int32_t *n_out, hipStream_t s);
int vec_prefilter(VecCatalog &c, int mode, int oversample, hipStream_t s);
int vec_scores_i8(VecCatalog &c, const float *queries, int nq, int location, float *approx_out, double *eps_out,
                  int64_t cap, hipStream_t s);
int vec_save(VecCatalog &c, const char *path, hipStream_t s);
int vec_load(VecCatalog &c, const char *path, hipStream_t s);

// launch of csrc/vector_filter.hip (K9f): n_filters bitmaps of vec_allow_words(n) words each
void vec_allow(const uint8_t *dead, const uint32_t *track, const uint64_t *tags, int64_t n, const aid_vec_filter *filters,
               int n_filters, unsigned long long *allow, hipStream_t s);

// launches of csrc/vector_q8.hip (K9q); the caller checks hipGetLastError (vec_q8_rescore returns it)
void vec_q8_quantize(const float *tiled, int64_t row0, int64_t n, int dim, int8_t *dst, float *s_out, float *e_out,
                     hipStream_t s);
void vec_q8_scan(const int8_t *cat, const float *cat_s, int64_t n_tiles, int tiles_per_wg, const int8_t *q,
                 const float *q_s, int nqt, int dim, float *scores, int64_t ns, hipStream_t s);
hipError_t vec_q8_rescore(const float *cat, const float *q, int dim, unsigned long long *keys, int64_t stride, int n_max,
                          const int32_t *cnt, int cnt_cap, int nb, hipStream_t s);
void vec_q8_filter(const float *scores, int64_t ns, const uint8_t *dead, int64_t n, const uint32_t *thr,
                   unsigned long long *cand, int cap, int32_t *cnt, int nb, hipStream_t s);
// the same under a batch's allow-bitmaps (FPSPEC 9.2): query q tests bit e of bitmap fmap[q]
void vec_q8_filter_allowed(const float *scores, int64_t ns, const VecAllow &al, int64_t n, const uint32_t *thr,
                           unsigned long long *cand, int cap, int32_t *cnt, int nb, hipStream_t s);
void vec_q8_tau(const unsigned long long *keys, int64_t stride, int R, int limit, const float *q_e, float E, int dim,
                uint32_t *thr, int32_t *cnt, int nb, hipStream_t s);

}  // namespace aid
