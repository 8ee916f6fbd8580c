"""K5 at its limits, on constructed postings (k5_fixtures.py; their preconditions: test_k5_fixtures_host.py): every
hand-back reason of the LDS path alone, the global path's retry levels, the documented 1024-track limit, one mixed
batch with sub-batching, min_match above the LDS filter's counter width, the record-group and chunk edges, ties and
the frame bound, and the reserved track id. Every row comparison is against the CPU oracle (oracle/fp_match.c,
FPSPEC 7) on the engine's exported postings, never against another engine path. The expected counters follow from
the constants of csrc/index.hip and csrc/query.cpp named beside each literal, not from a run."""

import numpy as np
import pytest

import k5_fixtures as F
import oracle as O
from aidfp._lib import AID_ERR_INVALID, AID_ERR_STATE, EngineError
from aidfp.engine import Engine

pytestmark = pytest.mark.gpu
SR = 44100
REASONS = ("fallback_heavy", "fallback_table", "fallback_distinct", "fallback_tracks", "fallback_rows")  # reasons 1..5


def add(eng, *posts):
    for p in posts:
        h, tr, t = F.columns(p)
        eng.index_add_postings(h.ctypes.data, tr.ctypes.data, t.ctypes.data, len(p), device=False)
    eng.index_finalize()


def ref(eng, post, rec):
    return O.query(post, rec, min_match=eng.min_match, max_rows=eng.max_results)


def run_one(eng, rec):
    eng.match_stats(reset=True)
    got = eng.query([rec])[0]
    return got, eng.match_stats()


def reasons(st):
    return {k: st[k] for k in REASONS if st[k]}


# ---- a. every hand-back reason on its own (path 0: the engine's own choice) ----
# 204 = sizeof(FastLds::hot) / (5 * 4) rows of k_match_lds's staging; 256 = kFastTrackCap; 1024 = kFastVoteCap;
# 2048 = kFastDistinctCap; 2^18 = kLdsMaxVotes. On the global path 205..257 tracks, 1,100 keys and 2,100 frames are
# far below kTrackCap 1024, kVoteCap 4096 and kDistinctCap 8192: one attempt.
ISOLATED = {
    "tracks204": (lambda: F.tracks(204, 5), None, 1, 0),
    "tracks205": (lambda: F.tracks(205, 5), "fallback_rows", 1, 1),
    "tracks256": (lambda: F.tracks(256, 5), "fallback_rows", 1, 1),
    "tracks257": (lambda: F.tracks(257, 5), "fallback_tracks", 1, 1),
    "offsets1100": (lambda: F.many_offsets(100, 11), "fallback_table", 1, 1),
    "offsets600": (lambda: F.many_offsets(100, 6), None, 1, 0),
    "run2100": (lambda: F.long_run(2100), "fallback_distinct", 1, 1),
    "heavy": (F.heavy, "fallback_heavy", 0, None),  # above kLdsMaxVotes the LDS pass does not run the query
}


@pytest.mark.parametrize("name", list(ISOLATED))
def test_reason_in_isolation(name):
    build, reason, q_lds, q_global = ISOLATED[name]
    post, rec, mm = build()
    with Engine(SR, min_match=mm) as eng:
        add(eng, post)
        want = ref(eng, eng.index_export(), rec)
        got, st = run_one(eng, rec)
        print(name, "path 0", reasons(st), "queries_lds", st["queries_lds"], "queries_global", st["queries_global"])
        assert np.array_equal(got, want), (got[:4], want[:4])
        assert len(want) > 0
        assert st["queries"] == 1
        assert reasons(st) == ({reason: 1} if reason else {}), st
        assert st["queries_lds"] == q_lds, st
        if q_global is None:
            assert st["queries_global"] >= 1, st
        else:
            assert st["queries_global"] == q_global, st


# ---- b. retry levels of the global path ----
@pytest.mark.parametrize("path", [0, 2])
@pytest.mark.parametrize("n,attempts", [(9000, 2), (70000, 3)])
def test_global_retry_levels(n, attempts, path):
    """k5_global adds todo.size() to queries_global on every attempt: for one query the counter is the attempt count.
    9000 frames overflow k_vote_final's LDS set (kDistinctCap 8192), so attempt 2 keeps the sets in HBM at
    2^(12 + 2 * 2) = 2^16 entries; 70000 overflow those too: attempt 3, 2^18 entries, and hist_bits 15 + 2 + 2 = 19 is
    above kHotLdsBits 17, so the hot bitmap is read from global memory."""
    post, rec, mm = F.long_run(n)
    with Engine(SR, min_match=mm) as eng:
        eng.force("k5_path", path)
        add(eng, post)
        got, st = run_one(eng, rec)
        print(f"run{n} path {path}", reasons(st), "queries_lds", st["queries_lds"], "queries_global", st["queries_global"])
        assert np.array_equal(got, ref(eng, eng.index_export(), rec)), got
        assert np.array_equal(got, [[n, 42, 17, 0, n - 1]])
        assert st["queries_global"] == attempts, st
        assert reasons(st) == ({"fallback_distinct": 1} if path == 0 else {}), st  # kFastDistinctCap 2048 < n


# ---- c. the documented limit: kTrackCap = 1024 matching tracks on the global path ----
def test_track_limit_of_the_global_path():
    """1024 matching tracks fill k_vote_final's track table exactly and are answered; 1025 overflow it on every
    attempt (more histogram buckets do not help) until hist_bits passes 26: AID_ERR_STATE. The engine then answers
    an LDS query and a global-path query as before: no histogram row, bitmap or distinct set was left dirty."""
    t1024, r1024, _ = F.tracks(1024, 5)
    t1025, r1025, _ = F.tracks(1025, 5, hbase=100, tbase=2000)
    t204, r204, _ = F.tracks(204, 5, hbase=200, tbase=4000)
    run, rrun, _ = F.long_run(2100, track=9000, hbase=1000)
    with Engine(SR, min_match=5) as eng:
        add(eng, t1024, t1025, t204, run)
        post = eng.index_export()
        got = eng.query([r1024])[0]
        want = ref(eng, post, r1024)
        assert np.array_equal(got, want)
        assert len(got) == 50 and np.array_equal(got[:, 1], np.arange(50)) and np.all(got[:, 0] == 5)
        with pytest.raises(EngineError) as ei:
            eng.query([r1025])
        assert ei.value.code == AID_ERR_STATE
        for rec, q_lds_only in ((r204, True), (rrun, False), (r1024, False)):
            got, st = run_one(eng, rec)
            assert np.array_equal(got, ref(eng, post, rec))
            assert len(got) and (st["queries_global"] == 0) == q_lds_only, st


# ---- d. one mixed batch, then the same batch in sub-batches of the global path ----
def test_mixed_batch_and_sub_batches():
    """Seven fixtures in one index (disjoint hashes and track ids, min_match 5), queried interleaved in one call with
    two light queries between every two handed-back ones. Each query equals the oracle, and the counters are the
    fixtures' sum: rows 1 (205 tracks), tracks 1 (257), distinct 3 (2100 frames, and the 9000 frames in both record
    orders), heavy 1, table 0; six queries on the first global attempt and the two 9000-frame ones on a second. The
    light queries stay in LDS: each has at most 204 rows, 256 tracks and 2,048 (track, d, t_q) in all, and the
    64-record fixture's fillers are single votes, of which the filter lets only buckets with five through. K5_BATCH
    2 and 1 then split the global pass (the q0 += dbatch loop: its offsets into out_rows / out_n, and the refill of
    the HBM sets per pass: at K5_BATCH 1 the second 9000-frame query reuses the set the first one filled with the
    same (slot, t_q) keys, so a set left as it was would count none of its frames)."""
    fx = {
        "t204": F.tracks(204, 5),
        "t205": F.tracks(205, 5, hbase=100, tbase=2000),
        "t257": F.tracks(257, 5, hbase=200, tbase=4000),
        "run2100": F.long_run(2100, track=50000, hbase=1000),
        "run9000": F.long_run(9000, track=50001, hbase=10000),
        "heavy": F.heavy(hbase=30000, tbase=20000),
        "ge64": F.group_edges(64, 5, hbase=40000, tbase=40000),
    }
    rec = {k: v[1] for k, v in fx.items()}
    light = [rec["t204"], rec["ge64"], rec["run2100"][:100], rec["run9000"][:500], rec["t205"][:4], rec["ge64"][::-1].copy(),
             rec["run2100"][50:90], rec["t204"][::-1].copy(), rec["run9000"][8000:], rec["t257"][1:],
             rec["run9000"][3000:4000], rec["run2100"][1000:1900]]
    handed = [rec["t205"], rec["t257"], rec["run2100"], rec["run9000"], rec["run9000"][::-1].copy(), rec["heavy"]]
    qs = []
    for i, q in enumerate(handed):
        qs += [q, light[2 * i], light[2 * i + 1]]
    with Engine(SR, min_match=5) as eng:
        add(eng, *(v[0] for v in fx.values()))
        post = eng.index_export()
        want = [ref(eng, post, q) for q in qs]
        assert sum(len(w) > 0 for w in want) == len(qs) - 2  # four of five records: no row
        try:
            for batch in (0, 2, 1):
                eng.force("k5_batch", batch)
                eng.match_stats(reset=True)
                got = eng.query(qs)
                st = eng.match_stats()
                print("mixed batch, k5_batch", batch, reasons(st), "queries_lds", st["queries_lds"], "queries_global",
                      st["queries_global"])
                for i, (g, w) in enumerate(zip(got, want)):
                    assert np.array_equal(g, w), (batch, i, g[:3], w[:3])
                assert st["queries"] == len(qs)
                assert reasons(st) == {"fallback_heavy": 1, "fallback_distinct": 3, "fallback_tracks": 1,
                                       "fallback_rows": 1}, (batch, st)
                assert st["queries_lds"] == len(qs) - 1 and st["queries_global"] == 6 + 2, (batch, st)
        finally:
            eng.force("k5_batch", 0)


# ---- e. min_match above the 4-bit counters of the LDS filter (kLdsCtrBits) ----
@pytest.mark.parametrize("path", [0, 2])
@pytest.mark.parametrize("mm", [15, 16, 17, 40])
def test_min_match_above_counter_width(mm, path):
    """From min_match 16 on no 4-bit counter can reach it: a bucket is hot only through the wrap marking of phase 1."""
    post, rec, _ = F.high_min_match(mm)
    with Engine(SR, min_match=mm) as eng:
        eng.force("k5_path", path)
        add(eng, post)
        got, st = run_one(eng, rec)
        assert np.array_equal(got, ref(eng, eng.index_export(), rec)), got
        assert np.array_equal(got[:, :2], [[mm + 1, 3], [mm, 2]])
        if path == 0:
            assert st["queries_lds"] == 1 and st["queries_global"] == 0 and not reasons(st), st


# ---- f. record groups of for_each_window / walk_group, chunk edges of maskc ----
@pytest.mark.parametrize("path", [0, 2])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025])
def test_record_group_and_chunk_edges(n, path):
    """n records around the group sizes: 64 per wave, 8 x 64 = 512 for k_match_lds's one_group, 16 x 64 = 1024 for
    the global path's workgroup; buckets of every length class, so CSR ranges begin and end at every residue of the
    8-signature chunk. Then the same with three records whose buckets are empty, and once more with a filler track
    removed after index_finalize(): ensure_index rebuilds only when csr_current is false, which a removal does not
    clear, so the query runs on the old CSR with tomb_live set (the queued insert, and from 639 hot votes on --
    kHotQueue 638 -- the direct one)."""
    mm = 1 if n <= 65 else 3
    with Engine(SR, min_match=mm, max_results=1024) as eng:
        eng.force("k5_path", path)
        for absent in (0, 3):
            post, rec, _ = F.group_edges(n, mm, absent=absent)
            eng.index_reset()
            add(eng, post)
            exported = eng.index_export()
            got, st = run_one(eng, rec)
            print(f"group_edges({n}, absent={absent}) path {path}", reasons(st), "queries_global", st["queries_global"])
            assert np.array_equal(got, ref(eng, exported, rec)), (absent, got[:3])
            assert got[got[:, 1] == 5][0, 0] == n
            if path == 0 and n <= 65:  # the whole query fits k_match_lds's tables (test_k5_fixtures_host.py)
                assert st["queries_lds"] == 1 and st["queries_global"] == 0, st
        live = eng.index_stats()["live"]
        ids, cnt = np.unique(exported[exported[:, 1] >= 1000, 1], return_counts=True)
        gone = int(ids[np.argmax(cnt)])
        eng.index_remove(gone)
        assert eng.index_stats()["live"] == live  # no rebuild: the CSR still holds the removed track's postings
        got = eng.query([rec])[0]
        want = ref(eng, exported[exported[:, 1] != gone], rec)
        assert np.array_equal(got, want), got[:3]
        assert got[got[:, 1] == 5][0, 0] == n and gone not in got[:, 1]


# ---- g. ties and bounds ----
@pytest.mark.parametrize("path", [0, 2])
def test_ties_at_the_cut_and_smallest_d(path):
    post, rec, mm = F.cut_ties()
    with Engine(SR, min_match=mm, max_results=50) as eng:
        eng.force("k5_path", path)
        add(eng, post)
        got = eng.query([rec])[0]
        assert np.array_equal(got, ref(eng, eng.index_export(), rec))
        eleven = sorted(t for t, c in F.best_counts(post, rec).items() if c == 11)
        assert np.array_equal(got[45:, 1], eleven[:5]) and np.all(got[:45, 0] == 12)  # track ascending at the cut
        post, rec, mm = F.many_offsets(100, 6)
    with Engine(SR, min_match=mm, max_results=128) as eng:
        eng.force("k5_path", path)
        add(eng, post)
        got = eng.query([rec])[0]
        assert np.array_equal(got, ref(eng, eng.index_export(), rec))
        tr, d, _ = F.vote_list(post, rec)
        assert np.array_equal(got[:, 2], [d[tr == t].min() for t in range(100)]) and np.sum(got[:, 2] < 0) == 50


@pytest.mark.parametrize("path", [0, 2])
def test_query_frame_bound(path):
    """t_q = kMaxQueryFrame = 2^20 - 2 is the last frame a distinct-set key (slot << 20 | t_q) can carry without
    meeting the empty marker; 2^20 - 1 is refused, and the engine goes on."""
    post, rec, mm = F.frame_bound()
    with Engine(SR, min_match=mm) as eng:
        eng.force("k5_path", path)
        add(eng, post)
        want = ref(eng, eng.index_export(), rec)
        got = eng.query([rec])[0]
        assert np.array_equal(got, want) and got[0, 4] == (1 << 20) - 2
        bad = rec.copy()
        bad[1] += np.uint64(1 << 32)
        with pytest.raises(EngineError) as ei:
            eng.query([bad])
        assert ei.value.code == AID_ERR_INVALID
        assert np.array_equal(eng.query([rec])[0], want)


# ---- h. track id 0xFFFFFFFF is K5's empty marker: no call may store it ----
def test_reserved_track_id_is_rejected_everywhere():
    import torch

    post, rec, mm = F.tracks(7, 5)
    bad = post.copy()
    bad[3, 1] = 0xFFFFFFFF
    with Engine(SR, min_match=mm) as eng:
        add(eng, post)
        stats, exported = eng.index_stats(), eng.index_export()
        want = ref(eng, exported, rec)
        h, tr, t = F.columns(bad)
        with pytest.raises(EngineError) as ei:
            eng.index_add_postings(h.ctypes.data, tr.ctypes.data, t.ctypes.data, len(bad), device=False)
        assert ei.value.code == AID_ERR_INVALID
        dev = [torch.from_numpy(c.view(np.int32)).cuda() for c in (h, tr, t)]
        with pytest.raises(EngineError) as ei:
            eng.index_add_postings(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), len(bad), device=True)
        assert ei.value.code == AID_ERR_INVALID
        with pytest.raises(EngineError) as ei:
            eng.index_add_records(0xFFFFFFFF, rec)
        assert ei.value.code == AID_ERR_INVALID
        assert eng.index_stats() == stats and np.array_equal(eng.index_export(), exported)
        assert np.array_equal(eng.query([rec])[0], want) and len(want) == 7
