// aidfp_launch.h -- the host-callable launchers the .hip files define, declared once: the host files call them
// through this header and every defining .hip file includes it, so a signature that drifts fails to compile there.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aidfp_device.h"

namespace aid {
void launch_stft_power(const void *pcm, bool s16, const ClipDesc *clips, int n_clips, int64_t f0, int64_t total_frames,
                       int64_t total_strips, int64_t slots, int hop, const Tables *tab, float *out, bool logmag,
                       uint64_t *hot, float thr, bool keep_power, uint32_t *qmax, hipStream_t s);
int peak_pick_blocks_per_cu(int width);
void launch_peak_pick(int width, const float *power, const ClipDesc *clips, int n_clips, int64_t f0, int64_t total_strips,
                      int strip_len, float thr, const uint64_t *hot, uint64_t *mask, uint32_t *cold_cnt,
                      const uint32_t *clip_qmax, float rel, uint32_t *rowflags, hipStream_t s);
void launch_landmarks(const uint64_t *mask, const uint32_t *rowflags, const ClipDesc *clips, int n_clips,
                      int64_t total_chunks, int64_t *chunk_counts, uint64_t *records, int64_t *clip_counts, bool write,
                      uint32_t *k2_cold, uint64_t *k2_cold_host, uint32_t k2_waves, uint32_t k2_strips,
                      bool one_chunk_each, hipStream_t s);
void launch_synth(float *out, const uint32_t *tracks, const int64_t *starts, int n_clips, int64_t n, int sr,
                  int noise_a, uint32_t salt, int fmax_hz, bool envelope, const int16_t *sin_tab, hipStream_t s);
// (the launch shape and what is refused: aidfp_resample_plan.h)
void launch_resample(const void *src, bool s16, int64_t in_base, int64_t n, int channels, int up, int down, int hl,
                     int J, const float *taps, float *dst, int64_t m_first, int64_t count, hipStream_t s,
                     int n_streams = 1, int64_t src_stride = 0, int64_t dst_stride = 0, const void *hist = nullptr,
                     int64_t hist_n = 0, int64_t hist_stride = 0);
struct SpeedVarDev;  // aidfp_speed_plan.h
void launch_resample_speeds(const void *src, bool s16, int channels, const int64_t *clip_off, const SpeedVarDev *vars,
                            int n_speeds, const int64_t *blk_first, const int64_t *dst_off, int pair0, int n_pairs,
                            int64_t blocks, int64_t lds_floats, float *dst, hipStream_t s);
void launch_s16_to_f32(const int16_t *src, int64_t n, float *dst, hipStream_t s);
int dedup_chunks(int64_t n_cat);
void launch_dedup_scan(const uint32_t *cw, const int64_t *coff, const double *cdur, int64_t n_cat, const uint32_t *qw,
                       const int64_t *qoff, const double *qlo, const double *qhi, int nq, double *part_sim,
                       int64_t *part_idx, double *best_sim, int64_t *best_idx, hipStream_t s);
void launch_dedup_pairs(const uint32_t *aw, const int64_t *aoff, const uint32_t *bw, const int64_t *boff, int n,
                        double *sim, hipStream_t s);
void launch_index_count(const uint32_t *ph, const uint32_t *ptrack, int64_t n, const uint8_t *tomb, uint32_t n_tracks,
                        uint32_t *cnt, hipStream_t s);
void launch_index_scatter(const uint32_t *ph, const uint32_t *ptrack, const uint32_t *pt, int64_t n,
                          const uint8_t *tomb, uint32_t n_tracks, uint32_t *cursor, uint64_t *post, hipStream_t s);
void launch_scan(const uint32_t *in, uint32_t *out, int64_t n, uint32_t *tmp, hipStream_t s);
int match_lds_blocks_per_cu();
size_t radix_scratch_u32(int64_t n);
hipError_t launch_index_sort_build(const uint32_t *ph, const uint32_t *ptrack, const uint32_t *pt, int64_t n,
                                   const uint8_t *tomb, uint32_t n_tracks, uint32_t *keys0, uint32_t *keys1,
                                   uint64_t *vals0, uint64_t *vals1, uint32_t *scratch, uint32_t *E, uint32_t *offsets,
                                   unsigned long long *nz, uint64_t **vals_out, uint16_t *sig, int rank_mode,
                                   hipStream_t s);
void launch_make_sig(const uint64_t *post, int64_t n, uint16_t *sig, hipStream_t s);
void launch_compact(const uint32_t *ph, const uint32_t *ptrack, const uint32_t *pt, int64_t n, const uint8_t *tomb,
                    uint32_t n_tracks, uint32_t *cnt, uint32_t *off, uint32_t *tmp, uint32_t *oh, uint32_t *otrack,
                    uint32_t *ot, hipStream_t s);
void launch_records_to_postings(const uint64_t *recs, const int64_t *src_off, const int64_t *counts,
                                const int64_t *dst_off, const uint32_t *track_ids, int n_clips, uint32_t *ph,
                                uint32_t *ptrack, uint32_t *pt, hipStream_t s);
void launch_append_offsets(const int64_t *counts, int n_clips, int64_t base, int64_t *dst_off, int64_t *total,
                           hipStream_t s);
void launch_query_votes(const uint64_t *recs, const int64_t *qstart, const int64_t *qcount, int nq,
                        const uint32_t *offsets, int64_t *votes, uint64_t *ranges, hipStream_t s);
void launch_query(const uint64_t *recs, const int64_t *qstart, const int64_t *qcount, int nq, const uint32_t *offsets,
                  const uint64_t *post, const uint8_t *tomb, uint32_t n_tracks, int min_match, int max_rows,
                  uint32_t *hist, int hist_bits, uint32_t *hot, int32_t *rows, int32_t *nrows, int tomb_live,
                  int parts, int stage, uint32_t *dset, int dset_bits, hipStream_t s);
void launch_count_nonzero(const uint32_t *cnt, int64_t n, unsigned long long *out, hipStream_t s);
void launch_index_checksum(const uint32_t *ph, const uint32_t *ptr, const uint32_t *pt, int64_t first, int64_t n,
                           unsigned long long *out, hipStream_t s);
void launch_match_lds(const uint64_t *recs, const int64_t *qstart, const int64_t *qcount, int nq,
                      const uint32_t *offsets, const uint64_t *post, const uint8_t *tomb, uint32_t n_tracks,
                      int min_match, int max_rows, int32_t *rows, int32_t *nrows, int tomb_live, const int64_t *votes,
                      const uint16_t *sig, const uint64_t *ranges, hipStream_t s);
uint32_t index_keys();
void launch_downmix(const float *in, int64_t n, float *out, hipStream_t s);
void launch_window_gather(const void *src, bool s16, const int64_t *win, int n_win, int64_t max_len, float *dst, hipStream_t s);
void launch_exact_consensus(const int32_t *rows, const int32_t *nrows, int mr, const int32_t *clip_win, int n_clips,
                            double sec, int max_out, void *out, int32_t *n_out, hipStream_t s);
void launch_speed_select(const void *rows, const int32_t *nrows, int max_out, const int32_t *speeds_pm, int n_speeds,
                         int n_clips, void *out, int32_t *n_out, int32_t *speed_out, hipStream_t s);
struct MelChunkDev;  // aidfp_mel.h
struct MelTables;
void launch_logmel(const void *pcm, bool s16, const MelChunkDev *chunks, int64_t chunk0, int64_t n, const MelTables *tab,
                   const float *wc, float *out, hipStream_t s);
struct ChromaRowBlock;  // aidfp_chroma_plan.h
struct ChromaItemBlock;
struct ChromaTables;  // aidfp_chroma.h
void launch_chroma_rows(const void *pcm, bool s16, const ChromaRowBlock *blocks, int64_t block0, int64_t n,
                        const ChromaTables *tab, float *rows, hipStream_t s);
void launch_chroma_words(const float *rows, const ChromaItemBlock *blocks, int64_t block0, int64_t n,
                         const ChromaTables *tab, bool raw, uint32_t *words, hipStream_t s);
void launch_rows_scatter(const int32_t *src, const int32_t *order, int n, int mr, int32_t *dst, hipStream_t s);
// the two row lists of each of nq queries over the live index merged into the first (index.hip k_rows_merge)
void launch_rows_merge(int32_t *a, int32_t *na, const int32_t *b, const int32_t *nb, int nq, int mr, hipStream_t s);
// K4m csr_merge (index_merge.hip): the folded CSR's offsets, the tiles' posting totals, and the merge over the work
// items of aidfp_live_plan.h plan_merge (items: device MergeItem[n_items])
void launch_csr_merge_offsets(const uint32_t *om, const uint32_t *od, uint32_t *on, int64_t n, hipStream_t s);
void launch_csr_merge_totals(const uint32_t *om, const uint32_t *od, uint32_t *total, int n_tiles, hipStream_t s);
void launch_csr_merge(const void *items, int64_t n_items, const uint32_t *om, const uint64_t *pm, const uint16_t *sm,
                      const uint32_t *od, const uint64_t *pd, const uint16_t *sd, uint64_t *pn, uint16_t *sn,
                      hipStream_t s);
}  // namespace aid
