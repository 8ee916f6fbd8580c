"""The preconditions of test_gpu_match_edges.py, on the CPU oracle alone (oracle/fp_match.c, FPSPEC 7): every fixture
of k5_fixtures.py reaches the count its GPU test needs -- rows, distinct (track, d) keys, distinct (track, d, t_q)
triples, votes -- so a fixture can never quietly stop meeting the limit it was built for. The limits are the
constants of csrc/index.hip and csrc/aidfp_layout.h, named beside each literal."""

import numpy as np
import pytest

import k5_fixtures as F
import oracle as O

BIG = 4096  # max_rows above every fixture's row count
LDS_MAX_VOTES = 1 << 18  # kLdsMaxVotes


def stats(post, rec):
    tr, d, tq = F.vote_list(post, rec)
    keys = np.unique(np.stack([tr, d], axis=1), axis=0)
    triples = np.unique(np.stack([tr, d, tq], axis=1), axis=0)
    return len(tr), len(keys), len(triples)


def fast_slots(post, rec):
    """Home slots of the query's distinct (track, d) keys in k_match_lds's exact table (kFastVoteCap = 1024)."""
    tr, d, _ = F.vote_list(post, rec)
    keys = np.unique(np.stack([tr, d], axis=1), axis=0)
    return (F.mix_td(keys[:, 0], keys[:, 1]) >> np.uint32(20)) & np.uint32(1023)


def test_hashes_are_distinct_buckets_with_clear_spare_bits():
    h = F.hashes((1 << 26) - 5000, 5000)
    assert len(np.unique(h)) == 5000 and not np.any(h & np.uint32(0xFC0))  # bits 6..11: no hash sets them
    assert len(np.unique(F.bucket_key(h))) == 5000 and F.bucket_key(h).max() < (1 << 26)
    assert F.mix_td(np.array([0]), np.array([0]))[0] == 0
    assert F.mix_td(np.array([7]), np.array([-1]))[0] == F.mix_td(np.array([7]), np.array([0xFFFFFFFF]))[0]


def test_builders_are_deterministic():
    for build in (lambda: F.tracks(205), lambda: F.many_offsets(), lambda: F.high_min_match(16),
                  lambda: F.group_edges(65, 1, absent=3), F.cut_ties):
        a, b = build(), build()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


# 204: rows of k_match_lds's staging (sizeof(FastLds::hot) / 20); 256: kFastTrackCap; 1024: kTrackCap
@pytest.mark.parametrize("k", [204, 205, 256, 257, 1024, 1025])
def test_tracks_rows_keys_triples(k):
    post, rec, mm = F.tracks(k, 5)
    assert mm == 5 and len(rec) == 5
    rows = O.query(post, rec, mm, BIG)
    assert len(rows) == k and np.all(rows[:, 0] == 5) and np.array_equal(rows[:, 1], np.arange(k))
    assert np.any(rows[:, 2] < 0)
    votes, keys, triples = stats(post, rec)
    assert (votes, keys, triples) == (5 * k, k, 5 * k)
    # below the other LDS limits, so the reason is the rows' (from 205) or the tracks' (from 257) alone
    if k <= 257:
        assert keys <= 1024 // 2 and triples <= 2048  # kFastVoteCap (no 512-probe run at <= half load asserted below), kFastDistinctCap
        assert F.longest_probe_run(fast_slots(post, rec), 1024) < 512  # kFastVoteCap, kProbeMax
    assert triples <= 8192  # kDistinctCap: the global path's first attempt holds the set in LDS


def test_tracks_at_default_min_match_would_overflow_the_distinct_set():
    """Why tracks() uses min_match 5: at 10, 205 tracks are 2,050 keys for the 2,048-key set (reason 3, not 5)."""
    assert stats(*F.tracks(205, 10)[:2])[2] > 2048  # kFastDistinctCap


@pytest.mark.parametrize("per_track,keys_want", [(11, 1100), (6, 600)])
def test_many_offsets(per_track, keys_want):
    post, rec, mm = F.many_offsets(100, per_track)
    assert mm == 1
    rows = O.query(post, rec, mm, BIG)
    votes, keys, triples = stats(post, rec)
    assert (votes, keys, triples) == (keys_want, keys_want, keys_want)
    assert len(rows) == 100 and np.all(rows[:, 0] == 1) and np.array_equal(rows[:, 1], np.arange(100))
    tr, d, _ = F.vote_list(post, rec)
    smallest = np.array([d[tr == t].min() for t in range(100)])
    assert np.array_equal(rows[:, 2], smallest) and np.sum(smallest < 0) == 50
    assert np.all(rows[:, 3] == rows[:, 4])
    if keys_want > 1024:  # kFastVoteCap: more keys than slots, the table must overflow
        return
    # 600 keys in 1,024 slots: no run of occupied slots reaches kProbeMax = 512, so no insert gives up
    assert F.longest_probe_run(fast_slots(post, rec), 1024) < 512
    assert len(rows) <= 204 and triples <= 2048  # row staging, kFastDistinctCap


@pytest.mark.parametrize("n", [2100, 9000, 70000])
def test_long_run(n):
    post, rec, mm = F.long_run(n)
    rows = O.query(post, rec, mm, BIG)
    assert np.array_equal(rows, [[n, 42, 17, 0, n - 1]])
    assert stats(post, rec) == (n, 1, n)
    # 2100 > kFastDistinctCap 2048; 9000 > kDistinctCap 8192; 70000 > 2^16, the second global attempt's set
    assert n <= LDS_MAX_VOTES and n - 1 <= (1 << 20) - 2  # kMaxQueryFrame


def test_heavy_is_above_the_lds_vote_bound():
    post, rec, mm = F.heavy()
    votes, _, _ = stats(post, rec)
    assert votes == 300 * 901 and votes > LDS_MAX_VOTES
    rows = O.query(post, rec, mm, BIG)
    assert np.array_equal(rows[0], [300, 7, 100, 0, 598])
    assert len(rows) <= 204  # not handed back for any other reason once on the global path


@pytest.mark.parametrize("mm", [15, 16, 17, 40])
def test_high_min_match(mm):
    post, rec, got_mm = F.high_min_match(mm)
    assert got_mm == mm
    best = F.best_counts(post, rec)
    assert (best[1], best[2], best[3], best[4]) == (mm - 1, mm, mm + 1, mm - 1)
    tr, d, tq = F.vote_list(post, rec)
    assert np.sum(tr == 4) >= 2 * mm and len(np.unique(tq[tr == 4])) == mm - 1  # raw votes against distinct frames
    qt = (rec >> np.uint64(32)).astype(np.int64)
    assert len(np.unique(qt)) == len(rec) - 2  # two records share their t_q with another
    rows = O.query(post, rec, mm, BIG)
    assert np.array_equal(rows[:, 1], [3, 2]) and np.array_equal(rows[:, 0], [mm + 1, mm])
    votes, keys, triples = stats(post, rec)
    assert votes <= LDS_MAX_VOTES and keys <= 1024 // 2 and triples <= 2048  # answered in LDS


@pytest.mark.parametrize("absent", [0, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025])
def test_group_edges(n, absent):
    mm = 1 if n <= 65 else 3
    post, rec, got_mm = F.group_edges(n, mm, absent=absent)
    assert got_mm == mm and len(rec) == n + absent
    rows = O.query(post, rec, mm, BIG)
    tr, _, tq = F.vote_list(post, rec)
    true_row = [n, 5, 33, tq[tr == 5].min(), tq[tr == 5].max()]
    assert np.array_equal(rows[0] if n > 1 else rows[rows[:, 1] == 5][0], true_row)
    assert F.best_counts(post, rec)[5] == n
    votes, keys, triples = stats(post, rec)
    assert votes == len(post) and votes <= LDS_MAX_VOTES and len(post) > n  # at least one filler posting
    if n <= 65:  # min_match 1: every vote enters k_match_lds's tables, and they hold the whole query
        assert keys <= 1024 and F.longest_probe_run(fast_slots(post, rec), 1024) < 512  # kFastVoteCap, kProbeMax
        assert triples <= 2048 and len(rows) <= 204  # kFastDistinctCap, row staging (and so kFastTrackCap)
    h, cnt = np.unique(post[:, 0], return_counts=True)
    assert set(cnt.tolist()) <= set(F.GROUP_EDGE_LENGTHS)
    if n >= 12:
        assert set(cnt.tolist()) == set(F.GROUP_EDGE_LENGTHS)
    qh = (rec & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    assert len(np.unique(qh)) == len(qh) and np.sum(~np.isin(qh, h)) == absent
    if n >= 63:  # CSR ranges (cumulative bucket lengths in bucket order) begin and end at every residue mod 8
        cnt = cnt[np.argsort(F.bucket_key(h))]
        starts = np.cumsum(cnt) - cnt
        assert set((starts % 8).tolist()) == set(range(8)) and set(((starts + cnt) % 8).tolist()) == set(range(8))
    # the true posting arrives first, in the middle and last in its bucket
    where = set()
    for hh in h[:30]:
        b = post[post[:, 0] == hh]
        i = int(np.flatnonzero(b[:, 1] == 5)[0])
        where.add("first" if i == 0 else "last" if i == len(b) - 1 else "middle")
    assert where >= ({"first"} if n == 1 else {"first", "middle", "last"})


def test_frame_bound():
    post, rec, mm = F.frame_bound()
    assert mm == 2
    assert np.array_equal(O.query(post, rec, mm, BIG), [[2, 9, 5, 0, (1 << 20) - 2]])  # kMaxQueryFrame


def test_cut_ties():
    post, rec, mm = F.cut_ties()
    best = F.best_counts(post, rec)
    twelve = sorted(t for t, c in best.items() if c == 12)
    eleven = sorted(t for t, c in best.items() if c == 11)
    assert len(best) == 60 and len(twelve) == 45 and len(eleven) == 15 and mm <= 11
    assert twelve != list(range(twelve[0], twelve[0] + 45)) and min(eleven) < max(twelve)  # ids shuffled
    rows = O.query(post, rec, mm, 50)
    assert len(rows) == 50
    assert np.array_equal(rows[:45, 1], twelve) and np.array_equal(rows[45:, 1], eleven[:5])
    assert len(O.query(post, rec, mm, BIG)) == 60
