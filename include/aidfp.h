/*
 * aidfp.h -- C ABI of the MI355X fingerprint engine (libaidfp.so, gfx950).
 *
 * This is the drop-in boundary that replaces the process boundary of the
 * reference: audio-ident-service/app/audio/fingerprint.py spawns `olaf_c`
 * (store :117-125, query :185-193, del :239-246) with env OLAF_DB (:71-84) and
 * parses its stdout CSV (:273-350). Here the same three operations are plain C
 * calls on caller-owned buffers; the Python adapter
 * (audio-ident_amd/aidfp/fingerprint.py) keeps the reference's async API on top.
 *
 * Conventions: every function returns AID_OK (0) or a negative AID_ERR_*;
 * aid_last_error() returns a thread-local message for the last failure. Pointers
 * are plain host or device pointers as documented per call; `stream` is a
 * hipStream_t passed as void* (NULL = the engine's own stream, a blocking stream:
 * it is ordered after work the caller queued on the legacy default stream, so
 * buffers produced there are complete before the engine reads them). An engine is
 * bound to one GPU and takes an internal lock per call, so calls from several
 * threads never corrupt it; but a SEQUENCE of calls that shares state (aid_extract
 * then aid_result_* / aid_index_add_extracted / aid_query_extracted) must not be
 * interleaved with another thread's extraction. The single-call readers aid_query_pcm
 * and aid_exact_lane have no such window. The Python adapter takes a reader/writer
 * lock: index writers exclusive (the reference's single LMDB writer,
 * fingerprint.py:7-8), concurrent readers shared.
 */
#ifndef AIDFP_H
#define AIDFP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AID_ABI_VERSION 1

#define AID_OK 0
#define AID_ERR_INVALID (-1)  /* bad argument */
#define AID_ERR_DEVICE (-2)   /* HIP runtime / device failure: engine unusable */
#define AID_ERR_NOMEM (-3)    /* device or host allocation failed */
#define AID_ERR_STATE (-4)    /* call out of order (e.g. no extraction yet) */

#define AID_PCM_HOST 0
#define AID_PCM_DEVICE 1

/* kernel ids for aid_profile_read */
#define AID_K_STFT 0
#define AID_K_PEAKS 1
#define AID_K_LANDMARK_COUNT 2
#define AID_K_LANDMARK_WRITE 3
#define AID_K_SYNTH 4
#define AID_K_MATCH 5
#define AID_K_RESAMPLE 6
#define AID_K_DEDUP 7
#define AID_K_INDEX_BUILD 8 /* the K4 sort build (sort + bucket lengths + offsets) */
#define AID_K_VOTE_HIST 9    /* K5a: seen filter + global vote histogram (global match path) */
#define AID_K_HOT_SCAN 10    /* K5h: histogram rows -> hot-bucket bitmaps */
#define AID_K_VOTE_FINAL 11  /* K5b: exact (track, d) table of the hot votes, best d per track, rows */
#define AID_K_RESAMPLE_SPEEDS 12 /* K6s: every speed variant of a clip group, one launch */
#define AID_K_SPEED_SELECT 13    /* K8c: per-clip speed selection over the lane's rows */
#define AID_K_ROWS_MERGE 14      /* live index: a query's rows from the two CSR segments merged (device-row callers) */
#define AID_K_INDEX_MERGE 15     /* K4m: the live index's delta folded into main (offsets, tile totals, merge) */
#define AID_K_COUNT 16       /* AID_K_MATCH (5) is the LDS match path (k_match_lds) */

typedef struct aid_engine aid_engine;

typedef struct aid_config {
    int32_t sample_rate;   /* Hz; per-index property */
    int32_t hop;           /* 0 = FPSPEC default: 512 at sr >= 32 kHz, else 256 */
    float peak_threshold;  /* 0 = FPSPEC default 4.0; otherwise in [2^-124, 2^100] */
    int32_t device;        /* HIP device ordinal; -1 = current device */
    int32_t min_match;     /* query: 0 = FPSPEC default 10 (distinct query anchor frames, FPSPEC v1 7) */
    int32_t max_results;   /* query: 0 = FPSPEC default 50 */
    int32_t flags;         /* AID_FLAG_* (0 = default) */
    float peak_rel;        /* FPSPEC 5.1: 0 = off (default); else r in [2^-60, 1): per clip of an extraction call the peak
                              threshold is thr_c = max(peak_threshold, r * Pmax_c), Pmax_c = the clip's largest power
                              over all frames and bins (a NaN never raises it; +0 for a clip without frames), and
                              peak_threshold is the absolute floor. r = 10^(-top_db / 10) for "top_db below the
                              loudest bin". Took the first reserved word: the struct stays 64 bytes, ABI version 1 */
    int32_t reserved[8];
} aid_config;

/* aid_config.flags: keep the whole power plane of an extraction for aid_result_power. Without it
   K1 skips the stores of 64-bin blocks whose every power is <= peak_threshold (K2 never reads
   them) and aid_result_power fails with AID_ERR_STATE. */
#define AID_FLAG_KEEP_POWER 1

/* one landmark record (FPSPEC 6): hash in the low word, anchor frame in the high word */
typedef struct aid_hash {
    uint32_t hash;
    uint32_t t1;
} aid_hash;

int32_t aid_abi_version(void);
const char *aid_last_error(void);

/* Fill *out with the FPSPEC defaults for `sample_rate`. */
int aid_config_default(int32_t sample_rate, aid_config *out);

/* Create / destroy an engine (allocates device tables; workspaces grow on demand). */
int aid_engine_create(const aid_config *cfg, aid_engine **out);
void aid_engine_destroy(aid_engine *e);
int aid_engine_config(const aid_engine *e, aid_config *out);

/* Test hook: force one of the engine's own code paths, which it otherwise chooses itself per call
   (the parity tests run every path against the oracle). Never needed in production. */
#define AID_FORCE_K5_PATH 1        /* 0 auto, 1: as 0; kept for callers that pin the LDS path, 2 global histogram only */
#define AID_FORCE_K5_PARTS 2       /* 0 by vote count, else 1, 2 or 4 key partitions per query (K5a) */
#define AID_FORCE_K5_BATCH 3       /* 0 default (2048), else global-path queries per launch */
#define AID_FORCE_K2_STRIPS_X100 4 /* 0 adaptive, else 100 x K2 strips per resident workgroup slot */
#define AID_FORCE_K4_BUILD 5       /* 0 default, 1 radix sort (the default), 2 atomic counting sort (A/B), 3 retired
                                      (a library sort once kept for A/B: AID_ERR_INVALID),
                                      4 radix sort with the ballot-matched in-wave rank (A/B of the one-atomic rank) */
#define AID_FORCE_EXCHANGE_FAIL 6  /* 1: the next index exchange's pack (aid_index_pack, or the prepare step of
                                      aid_index_allgather) fails with AID_ERR_NOMEM, once (rank-failure tests) */
#define AID_FORCE_LANE_GATHER 7    /* 1: aid_exact_lane copies its sub-windows to a staging buffer before K1 instead
                                      of extracting them in place (A/B) */
#define AID_FORCE_PLANE_ROWS 8     /* 0 default (786,432), else power rows per K1 -> K2 clip group of one extraction
                                      call (tests: small calls split into several groups) */
#define AID_FORCE_K2_WIDTH 9       /* 0 adaptive, else 2 or 4 quarter waves per K2 workgroup (width 2: bins 0..511 per
                                      walk, a second walk over a strip whose upper half is hot) */
#define AID_FORCE_VEC_PATH 10      /* K9 scan: 0 auto (MFMA), 1 MFMA, 2 VALU (explicit fmaf, one pair per lane) */
#define AID_FORCE_VEC_CHUNK 11     /* 0 default, else a multiple of 32 in [32, 4096]: catalog rows per K9 scan workgroup
                                      and keys per selection slice (tests: a small catalog spans several chunks) */
#define AID_FORCE_SPEED_GROUP 12   /* 0 default (2^28: 1 GiB), else variant samples per clip group of one
                                      aid_exact_lane_speeds call (tests: a small call split into several groups) */
#define AID_FORCE_ROWS_MERGE 13    /* live index: 0 default (the host-row query calls merge a query's two row lists on the
                                      host), 1: they merge on the device (k_rows_merge, as aid_exact_lane always
                                      does) and copy the merged rows out (tests: constructed lists through the kernel) */
#define AID_FORCE_VEC_CAND 14      /* int8 prefilter: 0 default (4096), else the cap on |W| in [1, 4096] above which a
                                      query falls back to the f32 scan (tests: fallbacks on a small catalog) */
#define AID_FORCE_K1_WAVES 15      /* 0 default (CUs x 16, the resident K1 waves), else the wave count K1 splits a call's
                                      frames over (tests: small calls whose waves cross clip edges, or get few frames) */
int aid_engine_force(aid_engine *e, int32_t what, int32_t value);

/* Frames and worst-case record count of a clip of n samples (FPSPEC 1, 5). */
int64_t aid_num_frames(const aid_engine *e, int64_t n_samples);
int64_t aid_hash_capacity(const aid_engine *e, int64_t n_samples);

/*
 * Fingerprint extraction (K1 stft_power -> K2 peak_pick -> K3 landmark_hash).
 * Clip c is pcm[offsets[c] .. offsets[c+1]); `offsets` is a HOST array of
 * n_clips+1 non-decreasing sample indices. With AID_PCM_DEVICE, `pcm` is a device
 * pointer read in place (a clip at an odd offset reads its frames with 4-byte aligned
 * float2 loads); with AID_PCM_HOST the engine stages the samples itself, by ONE
 * asynchronous copy on `stream`: from page-locked memory that copy is a DMA, so
 * host PCM must stay unchanged until the call's stream completes (aid_sync, or
 * any aid_result_* call). An error return has already drained the stream.
 * Asynchronous on `stream`; results stay on the device until fetched below.
 * Replaces the FFT/peak/hash work of `olaf_c store|query` (fingerprint.py:117,185).
 */
int aid_extract(aid_engine *e, const float *pcm, const int64_t *offsets, int32_t n_clips, int32_t pcm_location,
                void *stream);
/*
 * Integer PCM (spec/FPSPEC.md 8): every PCM entry point has an _s16 twin that takes native-endian (little-endian)
 * int16 samples where its sibling takes floats. A sample's value is x = float(q) * 2^-15, exact in binary32 and
 * equal to q / 32768, so an _s16 call computes bit for bit what its float sibling computes on the widened samples;
 * the conversion happens in the kernels' loads (K1's ring, K6's staging), and a host batch is staged by a copy of
 * half the bytes. Offsets, starts, ends and strides count samples (frames for stereo) exactly as in the sibling;
 * an s16 clip may start at any sample (2-byte alignment), a stereo s16 frame is 4-byte aligned. WAV data, capture
 * devices and the reference's decode test vector are all s16: no host widening is needed.
 */
int aid_extract_s16(aid_engine *e, const int16_t *pcm, const int64_t *offsets, int32_t n_clips, int32_t pcm_location,
                    void *stream);

/* Block until the last extraction finished. */
int aid_sync(aid_engine *e);

/* Per-clip record counts of the last extraction (host array of n_clips). Synchronises. */
int aid_result_counts(aid_engine *e, int64_t *counts);
/* Copy clip `clip`'s records to host `out` (capacity `cap`); *n_out = count. Synchronises. */
int aid_result_hashes(aid_engine *e, int32_t clip, aid_hash *out, int64_t cap, int64_t *n_out);
/* Zero-copy device view of the last extraction: records (clip c starts at clip_base[c]),
   per-clip counts (device int64[n_clips]); clip_base is a HOST array owned by the engine. */
int aid_result_device(aid_engine *e, const aid_hash **records, const int64_t **counts_dev,
                      const int64_t **clip_base_host, int32_t *n_clips);

/* Debug/parity views of the last extraction (host copies, synchronise):
   power rows [F][1024] fp32 of clip `clip` (needs AID_FLAG_KEEP_POWER); peak bitmask [F][16] uint64. */
int aid_result_power(aid_engine *e, int32_t clip, float *out, int64_t cap_floats);
int aid_result_peakmask(aid_engine *e, int32_t clip, uint64_t *out, int64_t cap_words);
/* Effective peak threshold thr_c of every clip of the last extraction (host array of n_clips floats; FPSPEC 5.1).
   With peak_rel = 0 it is peak_threshold for every clip. Synchronises. Every route that extracts (aid_extract*,
   aid_query_pcm*, aid_query_windows*, aid_exact_lane*, the stream bank's windows) applies the engine's rule; a
   clip is one extraction unit: a track, a query clip, one sub-window or one stream window. */
int aid_result_thresholds(aid_engine *e, float *out);

/* Log-magnitude spectrogram 10*log10(P + 1e-10) of one host clip: out[F][1024] (host). */
int aid_spectrogram(aid_engine *e, const float *pcm, int64_t n, float *out, int64_t cap_floats);

/* Deterministic synthetic PCM (aidfp/synth.py semantics) written to DEVICE `dst`
   [n_clips][n]: tracks/starts are HOST arrays; noise_a = query-noise half-width (0 = none). */
int aid_synth(aid_engine *e, float *dst, const uint32_t *tracks, const int64_t *starts, int32_t n_clips, int64_t n,
              int32_t noise_a, uint32_t salt, void *stream);
/* Same with the partials' band [100, fmax_hz) Hz instead of [100, 8000) (fmax_hz <= sample_rate / 2): the
   bench's full-band workload, whose spectrum has no cold upper blocks. aid_synth = fmax_hz 8000. */
int aid_synth_band(aid_engine *e, float *dst, const uint32_t *tracks, const int64_t *starts, int32_t n_clips,
                   int64_t n, int32_t noise_a, uint32_t salt, int32_t fmax_hz, void *stream);
/* Same audio at an explicit sample rate (the engine's own rate above): the same partials and notes sampled
   at `sample_rate`, e.g. a 44.1 kHz catalog or a 48 kHz capture for an engine that indexes at 16 kHz.
   flags: AID_SYNTH_STATIONARY = the v0 generator (constant amplitude within a note); default = v2 (every
   note decays linearly to half amplitude, as a struck or plucked note: landmark times lock to the onsets). */
#define AID_SYNTH_STATIONARY 1
/* flags: AID_SYNTH_ASYNC = return once the generation is enqueued on `stream` (ordered after the engine's
   earlier work on that stream; the caller orders its own reads of dst). Default: the call waits for it. */
#define AID_SYNTH_ASYNC 2
int aid_synth_rate(aid_engine *e, float *dst, const uint32_t *tracks, const int64_t *starts, int32_t n_clips,
                   int64_t n, int32_t sample_rate, int32_t noise_a, uint32_t salt, int32_t fmax_hz, int32_t flags,
                   void *stream);

/* ---- index + match (FPSPEC 7) ----
 * Replaces `olaf_c store` + LMDB (fingerprint.py:117-125), `olaf_c del` (:239-246) and
 * `olaf_c query` (:185-202). Postings accumulate on the device; the CSR is (re)built by
 * aid_index_finalize, which aid_query* call implicitly when the index changed. Single
 * writer: calls that mutate the index must be serialised by the caller (fingerprint.py:7-8). */

/* one query result row (FPSPEC 7): d = t_ref - t_q of the best offset bin, in frames */
typedef struct aid_match_row {
    int32_t match_count;
    uint32_t track;
    int32_t d;
    int32_t tq_min;
    int32_t tq_max;
} aid_match_row;

int aid_index_reset(aid_engine *e);
/* Add every clip of the last aid_extract as track track_ids[c] (host array of n_clips). Asynchronous: the
   clips' posting counts are scanned on the device and the call does not wait for them (only for the previous
   call's); every reader of the postings (stats, finalize, export, ...) waits for the count first.
   Track id 0xFFFFFFFF is reserved (the matcher's empty-slot marker): AID_ERR_INVALID, nothing is added. */
int aid_index_add_extracted(aid_engine *e, const uint32_t *track_ids);
/* Add n postings (hash, track, t) from host (AID_PCM_HOST) or device (AID_PCM_DEVICE) arrays. A posting whose
   track id is 0xFFFFFFFF (reserved, as for aid_index_add_track) fails the whole call with AID_ERR_INVALID before
   anything is stored. */
int aid_index_add_postings(aid_engine *e, const uint32_t *hash, const uint32_t *track, const uint32_t *t, int64_t n,
                           int32_t location);
/* Register track id `track` without postings (a clip too short or too quiet to give a hash), so a
 * later aid_index_remove of it succeeds like `olaf_c del` of any stored name (fingerprint.py:239-262).
 * Idempotent. */
int aid_index_add_track(aid_engine *e, uint32_t track);
/* Tombstone a track: its postings stop voting; AID_ERR_INVALID if unknown or already removed. */
int aid_index_remove(aid_engine *e, uint32_t track);
/* Drop the stored postings of every removed track (order of the others kept; the LMDB delete of
 * `olaf_c del` frees its entries). *n_removed = postings dropped. The CSR is rebuilt lazily. */
int aid_index_compact(aid_engine *e, int64_t *n_removed);
/* One CSR over every stored posting, built now. With the live index on (below) it folds the delta segment into main,
   or runs the full build if a track was removed since main's build; aid_index_csr_export then sees everything. */
int aid_index_finalize(aid_engine *e);
/* ---- ingest while serving: the live index (two CSR segments) ----
 * Off (the default), any stored posting makes the next query rebuild the whole CSR. On, the CSR built last stays as
 * the MAIN segment and the postings stored since go into a second, small CSR, the DELTA, which alone is rebuilt
 * (O(delta + 2^26)); every query votes over both segments and its rows are merged: match_count descending, then
 * track id ascending, cut at max_results. When the delta would pass max_delta_postings it is FOLDED into main: the
 * two CSRs share the bucket order, so K4m merges them in one streaming pass, without a sort. A fold carries the
 * postings of tracks removed since main's build along (queries keep skipping them); the next full build drops them. Results do not depend on the segmentation (FPSPEC 7): a row's score is per (track, d), and
 * the rule below keeps every track's postings in one segment.
 * Rules:
 *  - Disjointness: an append keeps main only if every track id it carries is >= the track count (max id + 1) at
 *    main's build. An append with an older id, and aid_index_compact, _reset, _load, _splice / _allgather and a
 *    K4_BUILD force, fall back to the full build at the next query and empty the delta (counted by reason).
 *  - aid_index_remove works as ever: both segments skip the track's postings from then on.
 *  - aid_index_save / _load / _export / _checksum and the exchange read the stored postings and do not see segments.
 *    aid_index_csr_export fails with AID_ERR_STATE while postings sit in the delta; aid_index_finalize first.
 *  - aid_index_stats' n_live is the sum over both segments (-1 while stored postings wait for their build).
 *  - Tickets: a ticket submitted with the feature on holds the CSR segments it was submitted under until it is
 *    collected, and collect answers its handed-back queries against those. A store, delta rebuild or fold between
 *    submit and collect therefore never frees or overwrites what the ticket reads: the build that finds a segment held
 *    builds into new buffers, and the held ones are freed at collect. An uncollected ticket can so keep one extra copy
 *    of a segment alive (8 + 2 B per posting and the 256 MB offset array): collect tickets promptly. Its rows are those
 *    of the index as it was at submit, except that tracks removed since may be missing from handed-back queries.
 * aid_index_live: max_delta_postings = 0 turns the feature off, > 0 on with that cap. A change while a delta holds
 * postings folds first. */
int aid_index_live(aid_engine *e, int64_t max_delta_postings);
/* The first n of 13 counters since the engine was created: out[0] full (K4) builds of main, [1] delta builds (a fold
   first builds the delta over the whole tail, and counts here), [2] folds (K4m merges of the delta into main),
   [3] postings in main, [4] postings stored since (the delta's), [5] the
   track count at main's last build, [6..12] fall-backs from a valid main to the full build while the feature was on,
   by reason: an append with an older track id, aid_index_compact, _reset, _load, a splice / all-gather, a K4_BUILD
   force, aid_index_finalize with a track removed since main's build. */
int aid_index_live_stats(aid_engine *e, int64_t *out, int32_t n);
/* Cumulative match counters since the last reset (the first n of 7): out[0] queries, [1] exact votes (postings whose
   hash a query record hits), [2] 8-B postings K5's global path read (once per key partition in K5a + once in K5b),
   [3] queries answered on the LDS path, [4] on the global path, [5] query records, [6] 2-B posting signatures the
   LDS path read (twice per vote: its counting and insert passes; the insert pass also reads the 8-B posting of a
   vote whose bucket is hot), [7] resident LDS-path workgroups per CU (an occupancy query, not a counter),
   [8..12] queries the LDS path handed to the global path, by reason: above 2^18 votes, (track, d) table full,
   distinct-frame set full, track table full, more rows than its staging holds. Not counters either: [13] the K2
   width (AID_FORCE_K2_WIDTH) and [14] the K2 strips of the engine's last extraction call. Over the live index
   (aid_index_live) a query runs one pass per CSR segment: it is counted once in [0], while votes, records, reads,
   the LDS / global path counts [3] [4] and the hand-backs are summed over its passes. */
int aid_match_stats(aid_engine *e, int64_t *out, int32_t n, int32_t reset);
/* n_postings = stored postings, n_live = postings in the built CSR (-1 if stale), n_tracks = max id + 1 */
int aid_index_stats(aid_engine *e, int64_t *n_postings, int64_t *n_live, uint32_t *n_tracks);
/* Copy stored postings [first, first+count) to host or device columns (RCCL all-gather export). */
int aid_index_export(aid_engine *e, uint32_t *hash, uint32_t *track, uint32_t *t, int64_t first, int64_t count,
                     int32_t location);
/* Order-sensitive 64-bit checksum of stored postings [first, first+count), computed on the device:
   sum mod 2^64 over i of splitmix64-finalizer((hash << 32 | t) ^ track * 0x9E3779B97F4A7C15 ^ i * 0xD6E8FEB86659FD93),
   i counted from `first`. After the catalog exchange every rank compares its replica's checksum with the others'
   (the sequential ingest it replaces, app/ingest/pipeline.py:294-310, had one LMDB and nothing to compare). */
int aid_index_checksum(aid_engine *e, int64_t first, int64_t count, uint64_t *out);
/* The built CSR to host memory (tests and tools; the index must be finalized): offsets (n_offsets >= 2^26 + 1, or
   NULL) = the start of each bucket key's postings (offsets[k]..offsets[k+1]), posts (up to cap, or NULL) = the
   postings (track | t << 32) in bucket-key order, each bucket in arrival order (K4 is a stable sort); *n_out = the
   postings in the CSR (removed tracks' postings dropped). Replaces reading the LMDB that `olaf_c store` writes
   (audio-ident-service/app/audio/fingerprint.py:117-125). */
int aid_index_csr_export(aid_engine *e, uint32_t *offsets, int64_t n_offsets, uint64_t *posts, int64_t cap,
                         int64_t *n_out);
/* ---- PCM front-end (spec/FPSPEC.md 8) ----
 * Replaces ffmpeg `-ac 1 -ar <rate>` (audio-ident-service/app/audio/decode.py:41-60): optional
 * stereo downmix ((L+R)*0.5f) + rational polyphase resampling sr_in -> sr_out (scipy
 * resample_poly's Kaiser(5) filter, binary32, pinned order). src/dst are device pointers; src
 * holds n frames of `channels` (1, or 2 interleaved) floats, dst receives
 * aid_resample_len(n, sr_in, sr_out) mono samples. Asynchronous on `stream` (NULL = engine). */
int64_t aid_resample_len(int64_t n, int32_t sr_in, int32_t sr_out);
int aid_resample(aid_engine *e, const float *src, int64_t n, int32_t channels, int32_t sr_in, int32_t sr_out,
                 float *dst, int64_t cap, int64_t *n_out, void *stream);
/* src = n frames of `channels` int16 (stereo: interleaved, downmixed as (xL + xR) * 0.5f on the converted values);
   dst is float as above. */
int aid_resample_s16(aid_engine *e, const int16_t *src, int64_t n, int32_t channels, int32_t sr_in, int32_t sr_out,
                     float *dst, int64_t cap, int64_t *n_out, void *stream);
/* Streaming form: src[0] is stream sample in_base (samples outside [in_base, in_base+n) read as 0);
 * computes stream outputs [m_first, m_first+count) into dst[0..count). Output m needs inputs up to
 * floor((m*down + hl)/up) and J-1 before it, so a caller that keeps that history gets exactly the
 * whole-signal result chunk by chunk (aidfp.stream). */
int aid_resample_range(aid_engine *e, const float *src, int64_t in_base, int64_t n, int32_t channels, int32_t sr_in,
                       int32_t sr_out, int64_t m_first, int64_t count, float *dst, void *stream);
/* aid_resample_range for n_streams streams in lockstep, ONE launch (config 5: every stream of a bank pushes
 * the same chunk length): stream i's input starts src_stride floats after stream i-1's, its outputs
 * dst_stride floats after. Each stream's outputs are bit for bit those of its own aid_resample_range.
 * Replaces one ffmpeg `-ac 1 -ar` process per upload (decode.py:41-60) for a whole batch of live streams. */
int aid_resample_batch(aid_engine *e, const float *src, int64_t src_stride, int32_t n_streams, int64_t in_base, int64_t n,
                       int32_t channels, int32_t sr_in, int32_t sr_out, int64_t m_first, int64_t count, float *dst,
                       int64_t dst_stride, void *stream);
/* aid_resample_batch over a two-part input: stream frames [in_base - hist_n, in_base) from hist (hist_stride floats
 * per stream), then [in_base, in_base + n) from src. A live stream's chunk is read where the caller holds it and only
 * the previous chunk's last few frames are kept, instead of appending every chunk to a long history first (a
 * 256-stream 2.5 s push is 246 MB of stereo: its append cost ~80 us of GPU per push). Outputs bit for bit those of
 * aid_resample_batch over the concatenated input. */
int aid_resample_batch_split(aid_engine *e, const float *hist, int64_t hist_stride, int64_t hist_n, const float *src,
                             int64_t src_stride, int32_t n_streams, int64_t in_base, int64_t n, int32_t channels,
                             int32_t sr_in, int32_t sr_out, int64_t m_first, int64_t count, float *dst,
                             int64_t dst_stride, void *stream);
/* The same over int16 input: hist and src are both s16, hist_stride and src_stride count int16 (dst_stride floats);
 * hist_n = 0 is the batch form, n_streams = 1 the range form (a 256-stream 2.5 s push is 123 MB of s16 stereo). */
int aid_resample_batch_split_s16(aid_engine *e, const int16_t *hist, int64_t hist_stride, int64_t hist_n,
                                 const int16_t *src, int64_t src_stride, int32_t n_streams, int64_t in_base, int64_t n,
                                 int32_t channels, int32_t sr_in, int32_t sr_out, int64_t m_first, int64_t count,
                                 float *dst, int64_t dst_stride, void *stream);
/* (up, down, hl, J) of a rate pair (FPSPEC 8); returns 0 on bad rates */
int aid_resample_plan(int32_t sr_in, int32_t sr_out, int32_t *up, int32_t *down, int32_t *hl, int32_t *J);

/* ---- Chromaprint content dedup ----
 * Replaces app/audio/dedup.py:127-222 (`_fingerprint_similarity`, `check_content_duplicate`):
 * a device-resident catalog of raw Chromaprint fingerprints (u32 words) with durations; a scan
 * scores every entry whose duration d satisfies lo <= d <= hi (lo = duration*0.9,
 * hi = duration*1.1 in binary64, as the reference's SQL bounds) by
 * (matching_bits / (min_len*32)) * (min_len / max_len) in binary64 and returns the best entry
 * (earliest on ties, only scores > 0; -1 if none) and its score. Entry index = insertion order.
 * All arrays are host arrays; offsets are int64[n+1] word offsets. */
int aid_dedup_reset(aid_engine *e);
int aid_dedup_add(aid_engine *e, const uint32_t *words, const int64_t *offsets, const double *durations, int32_t n);
int aid_dedup_count(aid_engine *e, int64_t *n_entries, int64_t *n_words);
int aid_dedup_scan(aid_engine *e, const uint32_t *words, const int64_t *offsets, const double *durations, int32_t nq,
                   int64_t *best_idx, double *best_sim);
/* score of n (a_i, b_i) pairs, same formula (the reference's `_fingerprint_similarity`) */
int aid_dedup_pairs(aid_engine *e, const uint32_t *a, const int64_t *a_off, const uint32_t *b, const int64_t *b_off,
                    int32_t n, double *sim);

/* ---- vector ("vibe") lane (spec/FPSPEC.md 9) ----
 * Replaces the Qdrant collection of app/audio/qdrant_setup.py:50-64 and its search (app/search/vibe.py:164-218,
 * HNSW over int8-quantised vectors) by an exact brute-force scan of a device-resident catalog of chunk embeddings
 * (K9, csrc/vector.hip), and app/search/aggregation.py:63-138 by a kernel. The embedding model stays with the
 * caller: vectors arrive as floats, [n][dim] row-major, and are normalised on the way in (cosine distance).
 * Scores, hit lists and aggregated rows are the pinned arithmetic of FPSPEC 9, bit for bit.
 * An entry is one chunk of a track; entry index = insertion order. `tracks` are caller-chosen ids
 * (AID_VEC_NO_TRACK is reserved). Arrays are host (AID_PCM_HOST) or device (AID_PCM_DEVICE) where a `location`
 * is given, host otherwise. `stream` as everywhere; every call has finished when it returns. */
/* Empty the catalog and set its dimension: a multiple of 32 in [32, 1024] (the reference's is 512). */
int aid_vec_reset(aid_engine *e, int32_t dim);
/* Append n entries (replaces upsert_track_embeddings' points). chunk_index NULL = 0 .. n-1. The catalog grows on
   demand. */
int aid_vec_add(aid_engine *e, const float *vecs, const uint32_t *tracks, const int32_t *chunk_index,
                const double *offset_sec, int64_t n, int32_t location);
/* Tombstone every entry of a track (delete_track_embeddings); AID_ERR_INVALID if it has no live entry. */
int aid_vec_remove(aid_engine *e, uint32_t track);
/* Drop the tombstoned entries; the others keep their order and are renumbered. *n_removed = entries dropped. */
int aid_vec_compact(aid_engine *e, int64_t *n_removed);
int aid_vec_count(aid_engine *e, int64_t *n_entries, int64_t *n_live, int32_t *dim);

typedef struct aid_vec_hit {
    uint32_t entry;
    uint32_t track;
    int32_t chunk_index;
    float score;
    double offset_sec;
} aid_vec_hit;
/* The `limit` (1..1024) live entries of the largest score per query, score descending then entry ascending
   (replaces _query_qdrant). hits: host [nq][limit]; n_hits: host [nq]. */
int aid_vec_search(aid_engine *e, const float *queries, int32_t nq, int32_t location, int32_t limit,
                   aid_vec_hit *hits, int32_t *n_hits, void *stream);
/* Debug and parity view: the whole score matrix [nq][n_entries] to host `out` (capacity `cap` floats); removed
   entries are included. */
int aid_vec_scores(aid_engine *e, const float *queries, int32_t nq, int32_t location, float *out, int64_t cap);

typedef struct aid_vibe_row {
    uint32_t track;
    int32_t chunk_count; /* hits of the track in the list */
    double final_score, base_score, diversity_bonus;
} aid_vibe_row;
#define AID_VEC_NO_TRACK 0xFFFFFFFFu
/* aggregate_chunk_hits over nq host hit lists (list q = hits[hoff[q] .. hoff[q+1]), at most 1024 hits each; only
   track, score and offset_sec are read), then final_score >= threshold and the first max_out. exclude: NULL, or
   per query a track to drop (AID_VEC_NO_TRACK = none). out: host [nq][max_out]; n_out: host [nq]. */
int aid_vec_aggregate(aid_engine *e, const aid_vec_hit *hits, const int64_t *hoff, int32_t nq, int32_t top_k_per_track,
                      double diversity_weight, const uint32_t *exclude, double threshold, int32_t max_out,
                      aid_vibe_row *out, int32_t *n_out);
/* Search, aggregation, threshold and limit of a batch of queries in one critical section (run_vibe_lane's steps 2
   and 3, vibe.py:36-161, without the metadata lookup): safe to call from several threads, like aid_exact_lane. */
int aid_vibe_lane(aid_engine *e, const float *queries, int32_t nq, int32_t location, int32_t limit,
                  int32_t top_k_per_track, double diversity_weight, const uint32_t *exclude, double threshold,
                  int32_t max_out, aid_vibe_row *out, int32_t *n_out, void *stream);
/* Flat versioned file (magic AIDFPVC1, u32 version, i32 dim, i64 n, then the normalised vectors as stored, tracks,
   chunk indices, offsets, tombstones): replaces Qdrant's own persistence. A truncated or foreign file gives
   AID_ERR_INVALID and leaves the catalog as it was. A catalog with a non-zero tags word (FPSPEC 9.2) saves version
   2, the same file with the u64 tags column appended; one without saves version 1 as before. Load reads both. */
int aid_vec_save(aid_engine *e, const char *path);
int aid_vec_load(aid_engine *e, const char *path);
/* Cumulative vector-lane counters since the last reset (the first n of 8), counted on the host. A batch is one scan +
   selection pass of at most 64 queries of aid_vec_search / aid_vibe_lane: out[0] batches whose hit lists came from
   the threshold route, [1] batches not eligible for it (fewer slices than `limit`, or more than 4096 of them),
   [2] batches that tried it and overflowed a candidate list (answered slice by slice, like [1]), [3] k_vec_select
   launches of the slice-by-slice route (one per pass), [4] the largest candidate count read back (a maximum, not a
   sum; it may exceed 4096, which is what [2] counts), [5] catalog reallocations that copied stored rows, [6] MFMA
   scan launches and [7] VALU scan launches (aid_vec_scores counts in these two as well). */
int aid_vec_stats(aid_engine *e, int64_t *out, int32_t n, int32_t reset);
/* int8 prefilter (spec/FPSPEC.md 9.1; K9q, csrc/vector_q8.hip), off by default. mode 1 keeps an int8 copy of the
   catalog (dim + 8 bytes per entry beside the f32 rows, which stay: rescoring reads them), and aid_vec_search /
   aid_vibe_lane then scan that copy, rescore the entries that a proven error bound cannot rule out with FPSPEC 9's
   chain, and fall back to the f32 scan for a query with more than 4096 such entries. Hit lists, score bits and rows
   are the same with it on and off; only the work differs. oversample in [1, 64]: the first-stage candidates are
   R = min(1024, oversample * limit). Entries already stored are quantised by the call; mode 0 frees the copy. The
   save file does not change: the int8 form follows from the stored rows and is rebuilt by aid_vec_load. */
int aid_vec_prefilter(aid_engine *e, int32_t mode, int32_t oversample);
/* Debug and parity view of the prefilter, as aid_vec_scores is of the scan: approx [nq][n_entries] to host
   `approx_out` (capacity `cap` floats) and eps [nq] to host `eps_out`. AID_ERR_STATE while the prefilter is off. */
int aid_vec_scores_i8(aid_engine *e, const float *queries, int32_t nq, int32_t location, float *approx_out,
                      double *eps_out, int64_t cap);
/* Cumulative prefilter counters since the last reset (the first n of 6): out[0] queries answered by the prefilter,
   [1] queries that fell back to the f32 scan, [2] the sum and [3] the largest of |W| over both kinds, [4] pairs
   rescored with the FPSPEC 9 chain (first-stage candidates and the W of the answered queries), [5] int8 scan
   launches (aid_vec_scores_i8 counts here as well). The selection over approx also counts in aid_vec_stats. */
int aid_vec_prefilter_stats(aid_engine *e, int64_t *out, int32_t n, int32_t reset);
/* Filtered search (spec/FPSPEC.md 9.2; K9f, csrc/vector_filter.hip), opt-in: the calls above do what they did.
   Every entry carries a 64-bit `tags` word, 0 unless given here. A filter belongs to one query; entry e passes it
   iff e is live, (any_of == 0 or tags_e & any_of != 0), tags_e & all_of == all_of, tags_e & none_of == 0, and
   track_e is not among the first n_exclude ids of `exclude` (an id that no entry carries is not an error). The hit
   list of a filtered query is FPSPEC 9's with "live" read as "passes": the filter acts before the selection, so
   an excluded track takes no slot. The all-zero filter passes exactly the live entries. */
#define AID_VEC_MAX_EXCLUDE 8
typedef struct aid_vec_filter {
    uint64_t any_of, all_of, none_of;
    uint32_t n_exclude;
    uint32_t exclude[AID_VEC_MAX_EXCLUDE];
} aid_vec_filter;
/* aid_vec_add with a tags column [n] (NULL = all 0; host or device, as the other payload columns). aid_vec_add is
   this call with NULL. */
int aid_vec_add_tagged(aid_engine *e, const float *vecs, const uint32_t *tracks, const int32_t *chunk_index,
                       const double *offset_sec, const uint64_t *tags, int64_t n, int32_t location);
/* Set the tags word of every live entry of a track; AID_ERR_INVALID if it has no live entry. */
int aid_vec_retag(aid_engine *e, uint32_t track, uint64_t tags);
/* The tags column [n_entries] to host `out` (capacity `cap` words). */
int aid_vec_tags(aid_engine *e, uint64_t *out, int64_t cap);
/* aid_vec_search under per-query filters: `filters` is host [nq], or NULL, which is aid_vec_search itself. A query
   with fewer than `limit` passing entries gets a shorter list, with none n_hits = 0. n_exclude > 8 gives
   AID_ERR_INVALID before anything runs. A batch of 64 queries whose filters are all zero runs the unfiltered
   kernels. Filtered batches count in aid_vec_stats and aid_vec_prefilter_stats as the others do; the prefilter's
   rescored pairs ([4]) are counted on the host from the live count, so a filtered query adds min(R, n_live) for its
   first stage even where fewer entries pass. */
int aid_vec_search_filtered(aid_engine *e, const float *queries, int32_t nq, int32_t location, int32_t limit,
                            const aid_vec_filter *filters, aid_vec_hit *hits, int32_t *n_hits, void *stream);
/* aid_vibe_lane under per-query filters (host [nq], or NULL), in one critical section. `exclude` keeps its meaning
   (dropped in the aggregation, after the track has taken its hit slots) and may be combined with a filter. */
int aid_vibe_lane_filtered(aid_engine *e, const float *queries, int32_t nq, int32_t location, int32_t limit,
                           int32_t top_k_per_track, double diversity_weight, const aid_vec_filter *filters,
                           const uint32_t *exclude, double threshold, int32_t max_out, aid_vibe_row *out,
                           int32_t *n_out, void *stream);

/* ---- CLAP log-mel front end (spec/FPSPEC.md 10; K10, csrc/mel.hip) ----
 * What the reference computes on the host before its CLAP model sees a sample: chunk_audio (10 s chunks, 5 s hop,
 * app/audio/embedding.py:101-152) and ClapFeatureExtractor's [1001][64] log-mel image per chunk. The input is mono
 * 48 kHz PCM (aid_resample gives it on the device), the output a [chunks][1001][64] float plane a device model
 * reads in place. The model itself stays with the caller. */
#define AID_MEL_FRAMES 1001
#define AID_MEL_BANDS 64
#define AID_MEL_BINS 513
#define AID_MEL_WINDOW 480000
#define AID_MEL_ZERO 0      /* ingest: chunk_audio's plan, a short last chunk is zero-filled */
#define AID_MEL_REPEATPAD 1 /* query: one chunk per clip; shorter than 10 s: repeated floor(480000 / n) times, then
                               zero-filled; longer: the 10 s from `start` on */
#define AID_MEL_BANK_SLANEY 0 /* slaney scale and norm (the extractor's mel_filters_slaney: truncation != "fusion") */
#define AID_MEL_BANK_HTK 1    /* htk scale, no norm (mel_filters: truncation == "fusion") */
#define AID_MEL_BANK_CUSTOM 2 /* the caller's own table */

/* one chunk of a plan: samples [start, start + r) of clip `clip`; rep = repetitions (1 in zero mode) */
typedef struct aid_mel_chunk {
    int32_t clip;
    int32_t chunk_index;
    int64_t start;
    int32_t r;
    int32_t rep;
    double offset_sec;   /* start / 48000 */
    double duration_sec; /* r / 48000 */
} aid_mel_chunk;

/* Chooses the filter bank; required once before aid_logmel. SLANEY / HTK: built on the host in binary64 from fmin and
   fmax (Hz, 0 <= fmin < fmax <= 24000), rounded once; `filters` must be NULL. CUSTOM: `filters` is a host
   [513][64] table (fmin, fmax ignored): every band's non-zero weights must be contiguous, non-negative and finite,
   no band may be empty, none may weight bin 512. Synchronous. */
int aid_mel_configure(aid_engine *e, int32_t bank, double fmin, double fmax, const float *filters);
/* The configured table, host out[513][64]. */
int aid_mel_filters(aid_engine *e, float *out);
/* Host only, no engine: the chunk plan of n_clips clip lengths (samples). *n_chunks receives the chunk count;
   meta_out (may be NULL) receives the first min(count, meta_cap) chunks. `start` matters in REPEATPAD mode for clips
   longer than 480000 samples and must lie in [0, n - 480000] for each of them. */
int aid_mel_plan(const int64_t *lengths, int32_t n_clips, int32_t mode, int64_t start, int64_t *n_chunks,
                 aid_mel_chunk *meta_out, int64_t meta_cap);
/* K10 over every chunk of the clips pcm[clip_off[c] .. clip_off[c] + clip_len[c]) (offsets in samples from `pcm`;
   location AID_PCM_HOST or AID_PCM_DEVICE). out[chunk][1001][64] floats, in device memory (out_location
   AID_PCM_DEVICE, the normal case: the call returns with the kernel queued on `stream`) or host memory (the call
   waits). *n_chunks receives the chunk count, `meta` (host, may be NULL) one entry per chunk. More chunks than
   out_cap_chunks: AID_ERR_INVALID with *n_chunks set and nothing written. No sample outside a clip is read. */
int aid_logmel(aid_engine *e, const float *pcm, const int64_t *clip_off, const int64_t *clip_len, int32_t n_clips,
               int32_t location, int32_t mode, int64_t start, float *out, int64_t out_cap_chunks, int32_t out_location,
               aid_mel_chunk *meta, int64_t *n_chunks, void *stream);
/* The same over int16 PCM (FPSPEC 8.1: x = q / 32768), offsets and lengths in int16 samples. */
int aid_logmel_pcm16(aid_engine *e, const int16_t *pcm, const int64_t *clip_off, const int64_t *clip_len,
                        int32_t n_clips, int32_t location, int32_t mode, int64_t start, float *out,
                        int64_t out_cap_chunks, int32_t out_location, aid_mel_chunk *meta, int64_t *n_chunks,
                        void *stream);

/* ---- content fingerprint (spec/FPSPEC.md 11) ----
 * Replaces the `fpcalc -raw` subprocess of app/audio/dedup.py:53-124 (`generate_chromaprint`) by K11: mono PCM at
 * 11025 Hz (resample first: aid_resample) -> 32-bit words in the raw-Chromaprint form aid_dedup_* takes. The spec is
 * the engine's own; PARITY WITH fpcalc IS UNPINNED (no fpcalc was at hand to compare with), so do not mix these
 * words with a database filled by fpcalc. Clip c = pcm[clip_off[c] .. clip_off[c+1]) (HOST offsets, n_clips + 1,
 * non-decreasing); a clip of n samples has 1 + (n - 4096) / 1365 frames and max(0, frames - 19) words, the first
 * at n = 30031. No sample outside a clip is read. */
#define AID_CHROMA_RATE 11025
#define AID_CHROMA_BANDS 12
#ifndef AID_CHROMA_RUN /* frames of one K11a workgroup (tests aim at its edges); diagnostic builds set others */
#define AID_CHROMA_RUN 4
#endif
/* words of a clip of n samples. No device. */
int64_t aid_chroma_len(int64_t n);
/* word offsets (word_off_out: int64[n_clips + 1] or NULL), frames and words of a batch of clip lengths. No device. */
int aid_chroma_plan(const int64_t *lengths, int32_t n_clips, int64_t *word_off_out, int64_t *n_frames,
                    int64_t *n_words);
/* The words of every clip, packed in clip order. pcm: host or device (`location`, AID_PCM_*; host PCM is staged by
   one copy). words_out: host or device (`out_location`), capacity cap_words; word_off_out: HOST int64[n_clips + 1]
   or NULL. *n_words is always set; more words than cap_words: AID_ERR_INVALID and nothing else written. Device
   output is asynchronous on `stream` (NULL: the engine's own stream, which aid_dedup_*_at run on too). */
int aid_chroma(aid_engine *e, const float *pcm, const int64_t *clip_off, int32_t n_clips, int32_t location,
               uint32_t *words_out, int64_t *word_off_out, int64_t cap_words, int32_t out_location, int64_t *n_words,
               void *stream);
/* The same over int16 PCM (FPSPEC 8.1: x = q / 32768), offsets in int16 samples. */
int aid_chroma_pcm16(aid_engine *e, const int16_t *pcm, const int64_t *clip_off, int32_t n_clips, int32_t location,
                   uint32_t *words_out, int64_t *word_off_out, int64_t cap_words, int32_t out_location,
                   int64_t *n_words, void *stream);
/* K11a alone, for tests and diagnosis: the chroma rows C[frames][12] of every clip (rows_out: HOST floats, capacity
   cap_rows rows; row_off_out: HOST int64[n_clips + 1] or NULL). Synchronous. */
int aid_chroma_rows(aid_engine *e, const float *pcm, const int64_t *clip_off, int32_t n_clips, int32_t location,
                    float *rows_out, int64_t *row_off_out, int64_t cap_rows, int64_t *n_rows, void *stream);
int aid_chroma_rows_pcm16(aid_engine *e, const int16_t *pcm, const int64_t *clip_off, int32_t n_clips, int32_t location,
                        float *rows_out, int64_t *row_off_out, int64_t cap_rows, int64_t *n_rows, void *stream);
/* K11b alone on the caller's HOST rows: clip c = rows [row_off[c], row_off[c+1]) of 12 floats. raw_features = 0:
   the rows are C (a word reads 20 of them); != 0: they are F, smoothing and normalisation skipped (a word reads 16).
   A word never reads another clip's rows. All arrays host; synchronous. */
int aid_chroma_words(aid_engine *e, const float *rows, const int64_t *row_off, int32_t n_clips, int32_t raw_features,
                     uint32_t *words_out, int64_t *word_off_out, int64_t cap_words, int64_t *n_words);
/* aid_dedup_add / aid_dedup_scan with the word array on the host or the device (`location`; offsets and durations
   stay host arrays): fingerprints made by aid_chroma on the device reach K7 without a round trip. Device words must
   be complete on the engine's own stream (aid_chroma with stream NULL) or before the call. */
int aid_dedup_add_at(aid_engine *e, const uint32_t *words, const int64_t *offsets, const double *durations, int32_t n,
                     int32_t location);
int aid_dedup_scan_at(aid_engine *e, const uint32_t *words, const int64_t *offsets, const double *durations,
                      int32_t nq, int32_t location, int64_t *best_idx, double *best_sim);

/* ---- native multi-GPU exchange (SURVEY.md 8b "aid_allgather_index", 8e) ----
 * One process per GPU. Rank 0 calls aid_comm_id, the host hands the 128 id bytes to every
 * rank (any side channel: torch.distributed store, MPI, a file), then every rank calls
 * aid_comm_create with its own engine. aid_comm wraps an RCCL communicator over xGMI.
 * Replaces the reference's single LMDB writer (pipeline.py:294-310, fingerprint.py:7-8):
 * ingest is sharded, the index is replicated by ONE all-gather. */
#define AID_COMM_ID_BYTES 128
typedef struct aid_comm aid_comm;
int aid_comm_id(uint8_t id[AID_COMM_ID_BYTES]);
int aid_comm_create(aid_engine *e, const uint8_t id[AID_COMM_ID_BYTES], int32_t world, int32_t rank, aid_comm **out);
void aid_comm_destroy(aid_comm *c);
/* Collective over all ranks of c: every rank's postings [first, n) (its shard) are all-gathered
 * (counts and track-id ranges first, then one padded SoA all-gather) and replace [first, n) by
 * the union in rank order; postings before `first` stay. The index is left dirty (finalize
 * next). *n_total = postings now held. Every rank must call it with the same comm.
 * Failure agreement: after the counts, every rank reserves the exchange buffers and the grown
 * index and packs its shard, then all ranks all-gather one ok flag; the payload all-gather runs
 * only if every rank is ready. A rank-local failure therefore makes EVERY rank return an error
 * (AID_ERR_STATE on the others) with its index unchanged, instead of leaving peers blocked in RCCL. */
int aid_index_allgather(aid_engine *e, aid_comm *c, int64_t first, int64_t *n_total);
/* The communicator's RCCL view: ranks (ncclCommCount) and this rank (ncclCommUserRank). */
int aid_comm_size(const aid_comm *c, int32_t *world, int32_t *rank);
/* aid_index_allgather in three steps, for an exchange the host runs itself (e.g. torch.distributed,
 * gloo on host copies). Every rank: aid_index_shard_info -> all-gather (count, n_tracks) -> stride = max
 * count -> aid_index_pack its shard into DEVICE planes [3][stride] (hash, track, t; zero padding) ->
 * all-gather the planes into DEVICE recv [world][3][stride] -> aid_index_splice with the host counts
 * [world] and max n_tracks. Splice is failure-atomic: on error the index is unchanged. */
int aid_index_shard_info(aid_engine *e, int64_t first, int64_t *count, uint32_t *n_tracks);
/* Everything a splice of `total` postings at `first` with n_tracks ids can fail on (growth of the posting
 * planes and the track tables), done ahead of the payload collective; the index itself does not change.
 * A host-driven exchange calls it with aid_index_pack before it agrees on every rank's readiness. */
int aid_index_reserve(aid_engine *e, int64_t first, int64_t total, uint32_t n_tracks, void *stream);
int aid_index_pack(aid_engine *e, int64_t first, uint32_t *planes, int64_t stride, void *stream);
int aid_index_splice(aid_engine *e, int64_t first, const uint32_t *recv, int32_t world, int64_t stride,
                     const int64_t *counts, uint32_t n_tracks, void *stream);

/* Flat versioned file (magic AIDFPIX1 + header + posting columns + tombstones): replaces the OLAF_DB dir. */
int aid_index_save(aid_engine *e, const char *path);
int aid_index_load(aid_engine *e, const char *path);
/* nq queries from host records: query q = recs[qoff[q] .. qoff[q+1]) (host qoff, nq+1 entries).
   rows: host [nq][max_results]; nrows: host [nq]. */
int aid_query(aid_engine *e, const aid_hash *recs, const int64_t *qoff, int32_t nq, aid_match_row *rows,
              int32_t *nrows);
/* Query with every clip of the last aid_extract (records stay on the device). */
int aid_query_extracted(aid_engine *e, aid_match_row *rows, int32_t *nrows);
/* Extraction + query of a batch of clips as ONE call (offsets/pcm as aid_extract; rows [n_clips][max_results],
   nrows [n_clips], host): safe to call from several threads at once -- the engine serialises the calls and no
   other call's extraction can interleave. The reader entry point of the Python service, which coalesces
   concurrent olaf_query requests into one call (replaces one `olaf_c query` process per request,
   fingerprint.py:185-193). Synchronous. */
int aid_query_pcm(aid_engine *e, const float *pcm, const int64_t *offsets, int32_t n_clips, int32_t pcm_location,
                  aid_match_row *rows, int32_t *nrows, void *stream);
int aid_query_pcm_s16(aid_engine *e, const int16_t *pcm, const int64_t *offsets, int32_t n_clips, int32_t pcm_location,
                      aid_match_row *rows, int32_t *nrows, void *stream);
/* aid_query_pcm over windows of DEVICE PCM given as [starts[c], ends[c]) sample ranges, which may overlap
 * (50 %-overlap stream windows, sub-windows of one clip): K1-K3 read them in place, then K5, in one critical
 * section. Rows as aid_query. Replaces one `olaf_c query` per window (fingerprint.py:185-193). */
int aid_query_windows(aid_engine *e, const float *pcm, const int64_t *starts, const int64_t *ends, int32_t n_windows,
                      aid_match_row *rows, int32_t *nrows, void *stream);
int aid_query_windows_s16(aid_engine *e, const int16_t *pcm, const int64_t *starts, const int64_t *ends,
                          int32_t n_windows, aid_match_row *rows, int32_t *nrows, void *stream);
/* The same query in two halves (a caller overlaps its next batch's host work with this batch's
 * kernels). _submit enqueues the extraction, K5 and the result copies on `stream` and returns a ticket at once;
 * _collect waits for that ticket's work, answers any query the fast match path handed back, writes the rows exactly
 * as aid_query_windows would and hands the ticket back to the engine's pool (also on error). Tickets may be collected
 * in any order; the windows' PCM must stay unchanged until the ticket's work has run (it is read in stream order).
 * Collect every ticket before aid_engine_destroy (the engine frees its pooled tickets, not the outstanding ones). */
typedef struct aid_query_ticket aid_query_ticket;
int aid_query_windows_submit(aid_engine *e, const float *pcm, const int64_t *starts, const int64_t *ends,
                             int32_t n_windows, void *stream, aid_query_ticket **ticket);
/* (an _s16 ticket is collected with aid_query_windows_collect like any other) */
int aid_query_windows_submit_s16(aid_engine *e, const int16_t *pcm, const int64_t *starts, const int64_t *ends,
                                 int32_t n_windows, void *stream, aid_query_ticket **ticket);
int aid_query_windows_collect(aid_engine *e, aid_query_ticket *ticket, aid_match_row *rows, int32_t *nrows);
/* aid_query_pcm in the same two halves (the query coalescer's pipelined batches, replacing the per-request
 * `olaf_c query` processes of fingerprint.py:185-193): HOST PCM is copied to the device in stream order, so the
 * caller keeps it unchanged until it has collected the ticket (with aid_query_windows_collect). */
int aid_query_pcm_submit(aid_engine *e, const float *pcm, const int64_t *offsets, int32_t n_clips,
                         int32_t pcm_location, void *stream, aid_query_ticket **ticket);
int aid_query_pcm_submit_s16(aid_engine *e, const int16_t *pcm, const int64_t *offsets, int32_t n_clips,
                             int32_t pcm_location, void *stream, aid_query_ticket **ticket);

/* Batched exact lane: replaces app/search/exact.py run_exact_lane's
   sub-window fan-out, the olaf_query calls and the consensus (exact.py:70-124, :132-353) for a
   batch of clips in one call. Clip c = pcm[offsets[c] .. offsets[c+1]) at the engine's sample
   rate (the reference's SAMPLE_RATE, exact.py:58). Clips of <= 5 s are queried as the three
   SUB_WINDOWS (:48-52) and merged by consensus (:220-293), longer clips whole (:296-332);
   candidates below MIN_ALIGNED_HASHES = 8 are dropped and the rest ranked by confidence
   min(h/20, 1), stable, descending (:109-121, :340-353). out: host [n_clips][max_out] rows,
   n_out: host [n_clips]. The metadata lookup (:447-496) stays with the caller. Synchronous. */
typedef struct aid_exact_row {
    uint32_t track;          /* engine track id */
    int32_t aligned_hashes;  /* consensus score */
    double offset_seconds;   /* median reference_start of the track's rows (binary64, as Python) */
    double confidence;       /* min(aligned_hashes / 20, 1) */
} aid_exact_row;
int aid_exact_lane(aid_engine *e, const float *pcm, const int64_t *offsets, int32_t n_clips, int32_t pcm_location,
                   int32_t max_out, aid_exact_row *out, int32_t *n_out, void *stream);
/* s16 clips: the sub-windows are read in place as above (under AID_FORCE_LANE_GATHER the gather converts them) */
int aid_exact_lane_s16(aid_engine *e, const int16_t *pcm, const int64_t *offsets, int32_t n_clips,
                       int32_t pcm_location, int32_t max_out, aid_exact_row *out, int32_t *n_out, void *stream);
/* The lane's window plan for a clip of n samples (host only, no device): returns the number of
   windows (3 for clips <= 5 s, mode 1; else 1 whole-clip window, mode 0) with sample bounds
   lo[w], len[w] (len 0 = no query, as the reference's empty piece, exact.py:150-160, :374-399). */
int aid_exact_windows(int64_t n, int32_t sample_rate, int64_t *lo, int64_t *len, int32_t *mode);

/* ---- speed-tolerant exact lane (spec/FPSPEC.md 8.2, 7.1) ----
 * A recording played fast or slow (tempo and pitch together: radio, a turntable, a "sped-up" rip) shares almost no
 * hash with its track. A speed is an integer pm in per mille, s = (1000 + pm) / 1000, pm in [-500, +1000]; the
 * speed-pm variant of a clip captured at sr_in, for an engine at rate sr_e, is the FPSPEC 8 resampling of the clip
 * for the rate pair (sr_in * 1000, sr_e * (1000 + pm)): what aid_resample returns for those two rates. Both factors
 * must fit int32. */
/* (up, down, hl, J) of a speed's rate pair; returns 0 on bad rates or speed, or a pair aid_resample rejects. No device. */
int aid_speed_plan(int32_t sr_in, int32_t sr_out, int32_t speed_pm, int32_t *up, int32_t *down, int32_t *hl, int32_t *J);
/* Samples of the variant of a clip of n frames (0 on bad input). No device. */
int64_t aid_speed_len(int64_t n, int32_t sr_in, int32_t sr_out, int32_t speed_pm);
/* Every speed variant of every clip in ONE launch (K6s). src: device, clip c = frames [offsets[c], offsets[c+1]) of
   `channels` (HOST offsets, n_clips + 1); sr_out is the engine's rate. dst: device floats, capacity cap; the variant
   of (clip c, speed v) lands at dst[dst_offsets[c * n_speeds + v] ..), packed in that order. dst_offsets: HOST
   int64[n_clips * n_speeds + 1], written by the call (also when cap is too small: its last entry is the capacity
   needed). Each variant equals aid_resample's output bit for bit. n_speeds in [1, 256]. Asynchronous on `stream`. */
int aid_resample_speeds(aid_engine *e, const float *src, const int64_t *offsets, int32_t n_clips, int32_t channels,
                        int32_t sr_in, const int32_t *speeds_pm, int32_t n_speeds, float *dst, int64_t cap,
                        int64_t *dst_offsets, void *stream);
/* int16 clips (FPSPEC 8.1), the rest the same. The int16 forms of the two speed entry points carry the infix of the
   s16 call they extend (aid_resample_s16, aid_exact_lane_s16) */
int aid_resample_s16_speeds(aid_engine *e, const int16_t *src, const int64_t *offsets, int32_t n_clips,
                            int32_t channels, int32_t sr_in, const int32_t *speeds_pm, int32_t n_speeds, float *dst,
                            int64_t cap, int64_t *dst_offsets, void *stream);
/* aid_exact_lane over every speed variant of every clip, and per clip the best speed (FPSPEC 7.1). Clips as above
   (frames of `channels` at sr_in; host PCM is staged by one copy, as in aid_extract). Each variant is a clip in its
   own right at the engine's rate: its own aid_exact_windows plan, K1-K5 and the consensus. A variant's key is the
   largest aligned_hashes among the rows the lane returns for it at max_out (0 without rows); the winner has the
   largest key, then the smaller |pm|, then the smaller pm, then the lower position in speeds_pm. out: host
   [n_clips][max_out], the winner's rows unchanged; n_out: host [n_clips]; speed_pm_out: host [n_clips], the winner's
   speed (0 for a clip without rows). Variant PCM lives in an engine buffer, 1 GiB per clip group (whole clips);
   only the winners' rows leave the device. Synchronous; safe to call from several threads, like aid_exact_lane. */
int aid_exact_lane_speeds(aid_engine *e, const float *pcm, const int64_t *offsets, int32_t n_clips,
                          int32_t pcm_location, int32_t channels, int32_t sr_in, const int32_t *speeds_pm,
                          int32_t n_speeds, int32_t max_out, aid_exact_row *out, int32_t *n_out,
                          int32_t *speed_pm_out, void *stream);
int aid_exact_lane_s16_speeds(aid_engine *e, const int16_t *pcm, const int64_t *offsets, int32_t n_clips,
                              int32_t pcm_location, int32_t channels, int32_t sr_in, const int32_t *speeds_pm,
                              int32_t n_speeds, int32_t max_out, aid_exact_row *out, int32_t *n_out,
                              int32_t *speed_pm_out, void *stream);

/* Streaming front end (config 5): interleaved f32 stereo [n_frames][2] -> mono [n_frames] on the
   device, m = (L + R) * 0.5f (the ffmpeg -ac 1 role, decode.py:50-51). Device pointers, stereo
   16-byte and mono 8-byte aligned; asynchronous on `stream`. */
int aid_downmix(aid_engine *e, const float *stereo, int64_t n_frames, float *mono, void *stream);

/* Per-kernel timing with HIP events recorded on the launch stream. */
int aid_profile_enable(aid_engine *e, int32_t on);
/* Which kernels get events while profiling is on: bit k = kernel id k (AID_K_*); default all.
   Each timed launch carries two dispatch-attached events (~5 us of end-of-kernel work per launch on
   MI355X), so a bench can time only the kernels it reports. */
int aid_profile_select(aid_engine *e, uint32_t kernel_mask);
/* ms[AID_K_COUNT] summed device time, launches[AID_K_COUNT]; synchronises; reset != 0 clears. */
int aid_profile_read(aid_engine *e, double *ms, int64_t *launches, int32_t reset);
/* Diagnostic: how many device blocks, page-locked host blocks and events the library's engines (their tickets
   included) hold in this process right now; any pointer may be NULL. A destroyed engine leaves all three as they
   were before it was created. */
int aid_live_allocations(int64_t *device, int64_t *pinned, int64_t *events);

#ifdef __cplusplus
}
#endif

#endif /* AIDFP_H */
