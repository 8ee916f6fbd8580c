"""The preconditions of test_gpu_consensus_edges.py, on the all-oracle lane alone (consensus_fixtures.expected:
oracle/fp_match.c rows, then aidfp.exact's consensus and ranking): every decision edge that the constructed index is
meant to hold is there -- the totals at 7 and 8 aligned hashes, halved and not, the medians in every window order,
confidence ties cut by max_out, a clip that fills the kernel's 768 staged rows with one window cut at max_results --
so the builder can never quietly stop producing an edge. What each candidate should be is worked out here from the
specs and the rows (sums, sorted middles, first appearances), not taken from aidfp.exact, which is what is checked."""

import numpy as np
import pytest

import consensus_fixtures as F
from aidfp.engine import exact_windows


@pytest.fixture(scope="module")
def B():
    return F.batch()


def by_tag(clip):
    out = {}
    for s in clip.specs:
        out.setdefault(s.tag, []).append(s)
    return out


def cand(clip):
    return {c.track_uuid.int: c for c in F.candidates(clip)}


def kept(clip):
    return F.expected(clip, F.MAX_STAGED)


def starts_of(clip, track):
    """The track's reference starts, per sent window in window order, from the oracle's K5 rows."""
    out = []
    for rows in clip.rows:
        for c, t, d, q0, _ in rows.tolist():
            if t == track:
                out.append((q0 + d) * F.SEC)
    return out


def test_batch_is_deterministic_and_small(B):
    F._BATCH.clear()
    again = F.batch()
    assert np.array_equal(again.postings, B.postings)
    assert [c.name for c in again.clips] == list(F.CLIPS)
    assert sum(len(c.pcm) for c in B.clips) <= 18 * F.SR and len(B.clips) <= 6
    assert B.postings[:, 1].max() < (1 << 20)


def test_windows_are_the_lanes_own(B):
    """The builder slices with aidfp.exact; aid_exact_windows (host-only C) gives the same plan. Window lengths are
    even, so the lane extracts every sample of them."""
    for c in B.clips:
        mode, wins = exact_windows(len(c.pcm), F.SR)
        assert mode == c.mode or len(c.pcm) == 0
        assert [(lo, ln) for lo, ln in wins if ln > 0] == c.windows, c.name
        assert all(ln % 2 == 0 for _, ln in c.windows)
    assert [len(c.windows) for c in B.clips] == [3, 0, 3, 1, 1, 2]
    assert [c.mode for c in B.clips][2:] == [1, 0, 1, 1]
    assert B.clips[1].name == "empty" and len(B.clips[0].pcm) and len(B.clips[2].pcm)  # an empty clip between two full


def test_pools_are_unique_hashes_at_distinct_frames(B):
    every = np.concatenate([r & np.uint64(0xFFFFFFFF) for c in B.clips for r in c.records])
    for c in B.clips:
        for pool, rec in zip(c.pools, c.records):
            h = pool & np.uint64(0xFFFFFFFF)
            assert all((every == x).sum() == 1 for x in h.tolist())
            assert len(np.unique(pool >> np.uint64(32))) == len(pool)
            assert np.isin(pool, rec).all()
    sizes = {c.name: [len(p) for p in c.pools] for c in B.clips}
    assert min(sizes["cases"]) >= 37 and max(sizes["cases"]) >= 40, sizes
    assert sizes["whole"][0] >= 40 and sizes["one_window"][0] >= 18 and min(sizes["two_windows"]) >= 10, sizes


def test_rows_are_what_the_specs_say(B):
    """K5's row of a track in a window carries the spec's count and offset (unless max_results cut the row)."""
    for c in B.clips:
        for w, rows in enumerate(c.rows):
            got = {t: (n, d, q0) for n, t, d, q0, _ in rows.tolist()}
            want = {s.track: (s.c[w], s.d[w], F.tq_min(c.pools[w], s.c[w])) for s in c.specs if s.c[w]}
            assert set(got) <= set(want)
            assert all(got[t] == want[t] for t in got), (c.name, w)
            assert len(got) == min(len(want), F.MAX_RESULTS)


def _check_totals(clip, halve_single: bool):
    """Every candidate's aligned_hashes from the specs' counts of the rows that reached the consensus."""
    cs = cand(clip)
    seen = {}
    for w, rows in enumerate(clip.rows):
        for n, t, *_ in rows.tolist():
            seen.setdefault(t, []).append(n)
    assert set(cs) == set(seen)
    for t, counts in seen.items():
        total = sum(counts)
        want = max(total // 2, 1) if halve_single and len(counts) == 1 else total
        assert cs[t].aligned_hashes == want, (clip.name, t, counts)
        st = sorted(starts_of(clip, t))
        med = st[0] if len(st) == 1 else (st[0] + st[1]) / 2 if len(st) == 2 else st[1]
        assert cs[t].offset_seconds == med, (clip.name, t, st)


@pytest.mark.parametrize("name", ["cases", "bulk", "whole", "one_window", "two_windows"])
def test_every_candidate_is_sum_halving_and_median(B, name):
    clip = B.clip(name)
    _check_totals(clip, halve_single=clip.mode == 1)
    k = kept(clip)
    cs = cand(clip)
    assert set(k["track"].tolist()) == {t for t, c in cs.items() if c.aligned_hashes >= 8}  # the threshold at 8
    assert np.array_equal(k["confidence"], np.minimum(k["aligned_hashes"] / 20.0, 1.0))
    # stable ranking: confidence descending, first appearance (window 0's rows, then 1, then 2) among equals
    first = {}
    for rows in clip.rows:
        for _, t, *_ in rows.tolist():
            first.setdefault(t, len(first))
    order = sorted(k["track"].tolist(), key=lambda t: (-min(cs[t].aligned_hashes / 20.0, 1.0), first[t]))
    assert k["track"].tolist() == order


def test_single_window_totals(B):
    clip = B.clip("cases")
    tags, cs, k = by_tag(clip), cand(clip), set(kept(clip)["track"].tolist())
    for total, aligned in ((15, 7), (16, 8), (17, 8), (2, 1), (40, 20)):
        ss = tags[f"single{total}"]
        assert ss and all(sum(x > 0 for x in s.c) == 1 and sum(s.c) == total for s in ss)
        for s in ss:
            assert cs[s.track].aligned_hashes == aligned
            assert (s.track in k) == (aligned >= 8)
    assert cs[tags["single40"][0].track].aligned_hashes / 20.0 == 1.0
    assert {s.c.index(15) for s in tags["single15"]} == {0, 1, 2}  # one in each window


def test_two_and_three_window_totals(B):
    clip = B.clip("cases")
    tags, cs, k = by_tag(clip), cand(clip), set(kept(clip)["track"].tolist())
    for tag, aligned in (("pair4+4", 8), ("pair3+4", 7), ("pair10+9", 19), ("triple3+3+2", 8)):
        ss = tags[tag]
        assert len(ss) == (1 if tag.startswith("triple") else 3)  # every pair of windows
        for s in ss:
            assert sum(x > 0 for x in s.c) >= 2 and cs[s.track].aligned_hashes == aligned  # kept whole, not halved
            assert (s.track in k) == (aligned >= 8)


def test_medians(B):
    clip = B.clip("cases")
    tags, cs = by_tag(clip), cand(clip)
    orders, medians, not_first = set(), [], 0
    for tag in ("median012", "median021", "median102", "median120", "median201", "median210"):
        (s,) = tags[tag]
        st = starts_of(clip, s.track)
        assert len(st) == 3 and len(set(st)) == 3
        orders.add(tuple(np.argsort(st).tolist()))
        assert cs[s.track].offset_seconds == sorted(st)[1]
        not_first += cs[s.track].offset_seconds != st[0]
        medians.append(cs[s.track].offset_seconds)
    assert len(orders) == 6 and len(set(medians)) == 6
    assert not_first == 4  # the median is window 1's or window 2's start in four of the six orders
    (s,) = tags["median_two_equal"]
    st = starts_of(clip, s.track)
    assert st[0] == st[1] != st[2] and cs[s.track].offset_seconds == st[0]
    for s in tags["pair4+4"]:  # two rows: the mean of two different starts
        a, b = starts_of(clip, s.track)
        assert a != b and cs[s.track].offset_seconds == (a + b) / 2 and cs[s.track].offset_seconds not in (a, b)


def test_confidence_ties_and_cuts(B):
    clip = B.clip("cases")
    k = kept(clip)
    strong = k[k["confidence"] == 1.0]
    counts = strong["aligned_hashes"].tolist()
    assert len(strong) >= 3 and len(set(counts)) >= 3
    assert counts != sorted(counts) and counts != sorted(counts, reverse=True)  # listed in no count order
    assert np.all(k["confidence"][:len(strong)] == 1.0)
    vals, n = np.unique(k["aligned_hashes"][k["aligned_hashes"] < 20], return_counts=True)
    assert n.max() >= 4  # four or more candidates share one aligned_hashes below 20
    # the cuts the GPU test makes fall inside tie groups: after rank 1, 3 and kept - 1 the next row has the same confidence
    for cut in (1, 3, len(k) - 1):
        assert k["confidence"][cut - 1] == k["confidence"][cut], cut
        assert np.array_equal(F.expected(clip, cut), k[:cut])
    assert len(F.expected(clip, len(k) + 1)) == len(k)


def test_staged_rows(B):
    cases, blk = B.clip("cases"), B.clip("bulk")
    staged = sum(len(r) for r in blk.rows)
    assert 760 <= staged <= F.MAX_STAGED and len(kept(blk)) > 64  # kExactMaxRows nearly (here: exactly) full
    assert sum(1 for s in blk.specs if all(s.c)) >= 254
    assert len(set.intersection(*[set(r[:, 1].tolist()) for r in blk.rows])) >= 249  # three rows each
    # window 0 is cut by max_results: tracks with postings there reach the consensus without that row
    want0 = {s.track for s in blk.specs if s.c[0]}
    got0 = set(blk.rows[0][:, 1].tolist())
    assert len(want0) > F.MAX_RESULTS == len(got0)
    cut = want0 - got0
    later = set(blk.rows[1][:, 1].tolist()) & set(blk.rows[2][:, 1].tolist())
    assert cut and cut <= later
    cs = cand(blk)
    spec = {s.track: s for s in blk.specs}
    for t in cut:
        assert cs[t].aligned_hashes == spec[t].c[1] + spec[t].c[2] < sum(spec[t].c)
    k = kept(blk)
    assert (k["aligned_hashes"] == 8).sum() >= 10 and sum(c.aligned_hashes == 7 for c in cs.values()) >= 10
    assert sum(len(r) for r in cases.rows) > 64  # a lane of the wave handles several rows there too


def test_clip_shapes(B):
    whole, one, two = B.clip("whole"), B.clip("one_window"), B.clip("two_windows")
    # whole clip: one row per track, nothing halved: 15 is kept as 15, 2 is dropped
    tags, cs = by_tag(whole), cand(whole)
    assert whole.mode == 0 and len(whole.rows) == 1
    assert {t: cs[tags[t][0].track].aligned_hashes for t in ("single15", "single16", "single2", "single40", "single7",
                                                             "single8")} \
        == {"single15": 15, "single16": 16, "single2": 2, "single40": 40, "single7": 7, "single8": 8}
    assert len(kept(whole)) == len(whole.specs) - 2  # all but 2 and 7
    # 0.7 s: window 0 only, every candidate halved
    tags, cs = by_tag(one), cand(one)
    assert one.mode == 1 and len(one.rows) == 1
    assert {t: cs[tags[t][0].track].aligned_hashes for t in ("single15", "single16", "single17", "single18", "single2")} \
        == {"single15": 7, "single16": 8, "single17": 8, "single18": 9, "single2": 1}
    assert sorted(kept(one)["aligned_hashes"].tolist()) == [8, 8, 9]
    # 1.4 s: two windows
    tags, cs = by_tag(two), cand(two)
    assert two.mode == 1 and len(two.rows) == 2
    assert {t: cs[tags[t][0].track].aligned_hashes for t in ("pair4+4", "pair3+4", "pair10+9", "single15", "single16")} \
        == {"pair4+4": 8, "pair3+4": 7, "pair10+9": 19, "single15": 7, "single16": 8}
    a, b = starts_of(two, tags["pair4+4"][0].track)
    assert a != b and cs[tags["pair4+4"][0].track].offset_seconds == (a + b) / 2
    e = B.clip("empty")
    assert e.windows == [] and e.rows == [] and len(F.expected(e, 10)) == 0
