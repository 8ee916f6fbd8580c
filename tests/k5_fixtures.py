"""Constructed postings and queries for the K5 matcher tests (spec/FPSPEC.md 7): each builder chooses which of the
matcher's limits its query meets -- a hand-back reason of the LDS path, a retry level of the global path, a
record-group or chunk edge, a tie -- where queries made from synthesised audio only meet them by chance.

Plain numpy, no GPU. Every builder returns (postings uint32 [n, 3] (hash, track, t), query records uint64
(hash | t_q << 32), min_match) and is deterministic from its seed. `hbase` and `tbase` shift a fixture's hashes and
track ids, so several fixtures can share one index without meeting. Query hashes within one query are distinct
(high_min_match says where two records share a t_q); track ids stay below 2^20 and t below 2^31.

test_k5_fixtures_host.py runs every fixture through the CPU oracle and asserts the counts (rows, (track, d) keys,
(track, d, t_q) triples, votes) that the GPU tests' expectations rest on."""

import numpy as np

U32 = np.uint32
U64 = np.uint64

GROUP_EDGE_LENGTHS = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 200)  # every residue of a CSR range's ends mod 8


def hashes(base: int, n: int) -> np.ndarray:
    """n distinct landmark hashes, numbers base .. base + n - 1 of the 2^26 a hash can be (FPSPEC 6: k1 = h >> 22,
    k2 = (h >> 12) & 1023, dt = h & 63; bits 6..11 stay clear), so distinct hashes are distinct index buckets."""
    c = base + np.arange(n, dtype=np.int64)
    assert n == 0 or (base >= 0 and int(c[-1]) < (1 << 26))
    return ((((c >> 16) & 0x3FF) << 22) | (((c >> 6) & 0x3FF) << 12) | (c & 0x3F)).astype(U32)


def bucket_key(h: np.ndarray) -> np.ndarray:
    """aidfp_layout.h bucket_key: the CSR bucket of a hash (the order in which the buckets' postings lie)."""
    h = np.asarray(h).astype(np.int64)
    return (((h >> 22) & 0xFF) << 18) | ((h >> 30) << 16) | (((h >> 12) & 0x7F) << 9) | (((h >> 19) & 0x7) << 6) | (h & 0x3F)


def records(h: np.ndarray, tq: np.ndarray) -> np.ndarray:
    return np.asarray(h).astype(U64) | (np.asarray(tq).astype(U64) << U64(32))


def _postings(h, track, t) -> np.ndarray:
    t = np.asarray(t, dtype=np.int64)
    track = np.broadcast_to(np.asarray(track, dtype=np.int64), t.shape)
    assert t.size == 0 or (t.min() >= 0 and t.max() < (1 << 31) and track.min() >= 0 and track.max() < (1 << 20))
    return np.stack([np.asarray(h, dtype=U32), track.astype(U32), t.astype(U32)], axis=1)


def columns(postings: np.ndarray):
    """The three contiguous uint32 columns Engine.index_add_postings takes."""
    return tuple(np.ascontiguousarray(postings[:, c]) for c in range(3))


def vote_list(postings: np.ndarray, rec: np.ndarray):
    """Every vote of the query as (track, d, t_q) int64 arrays: FPSPEC 7's join of the records and the postings on
    the hash, written independently of the oracle (sort + searchsorted)."""
    p = postings[np.argsort(postings[:, 0], kind="stable")]
    qh = (rec & U64(0xFFFFFFFF)).astype(U32)
    qt = (rec >> U64(32)).astype(np.int64)
    lo = np.searchsorted(p[:, 0], qh, "left")
    hi = np.searchsorted(p[:, 0], qh, "right")
    n = hi - lo
    which = np.repeat(np.arange(len(rec)), n)
    idx = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n) + np.repeat(lo, n)
    tq = qt[which]
    return p[idx, 1].astype(np.int64), p[idx, 2].astype(np.int64) - tq, tq


def best_counts(postings: np.ndarray, rec: np.ndarray) -> dict:
    """track -> its best (track, d) score, the distinct t_q among that key's votes (FPSPEC v1 7), from vote_list."""
    tr, d, tq = vote_list(postings, rec)
    keys, cnt = np.unique(np.unique(np.stack([tr, d, tq], axis=1), axis=0)[:, :2], axis=0, return_counts=True)
    best: dict = {}
    for (t, _), c in zip(keys.tolist(), cnt.tolist()):
        best[t] = max(best.get(t, 0), c)
    return best


def mix_td(track, d) -> np.ndarray:
    """index.hip mix_td in uint32 arithmetic: the hash that places a (track, d) in K5's exact tables."""
    with np.errstate(over="ignore"):
        x = (np.asarray(track).astype(U32) * U32(0x9E3779B1)) ^ (np.asarray(d).astype(np.int64).astype(U32) * U32(0x85EBCA77))
        x ^= x >> U32(15)
        x *= U32(0x2C1B3C6D)
        x ^= x >> U32(12)
    return x


def longest_probe_run(slots: np.ndarray, cap: int) -> int:
    """Longest cyclic run of occupied slots once every key of `slots` (home slots, one per distinct key) sits in a
    linear-probed table of `cap` slots. The occupied set does not depend on the insertion order, and no insert or
    lookup probes further than the run it lands in plus one."""
    occ = np.zeros(cap, dtype=bool)
    for s in np.sort(np.asarray(slots, dtype=np.int64)):
        while occ[s]:
            s = (s + 1) % cap
        occ[s] = True
    if occ.all():
        return cap
    z = int(np.argmin(occ))
    best = run = 0
    for v in np.roll(occ, -z):
        run = run + 1 if v else 0
        best = max(best, run)
    return best


def tracks(k: int, mm: int = 5, seed: int = 0, hbase: int = 0, tbase: int = 0):
    """k tracks (ids tbase .. tbase + k - 1), each sharing the query's mm records at one offset d_j in [-4, 400):
    k rows of count mm, k (track, d) keys, k * mm distinct (track, d, t_q)."""
    rng = np.random.default_rng([seed, k, mm])
    tq = 4 + 3 * np.arange(mm)
    h = hashes(hbase, mm)
    d = rng.integers(-4, 400, k)
    d[: min(k, 3)] = (-4, -1, 0)[: min(k, 3)]
    tr = tbase + np.arange(k)
    post = _postings(np.tile(h, k), np.repeat(tr, mm), (d[:, None] + tq[None, :]).ravel())
    return post[rng.permutation(len(post))], records(h, tq), mm


def many_offsets(tracks: int = 100, per_track: int = 11, seed: int = 0, hbase: int = 0, tbase: int = 0):
    """min_match 1: every track has one vote at each of per_track distinct offsets (every second track's first one
    negative, none shared by two of a track's records): tracks * per_track (track, d) keys, one count-1 row per
    track, which must carry the track's smallest d."""
    rng = np.random.default_rng([seed, tracks, per_track])
    tq = 10 + 7 * np.arange(per_track)
    h = hashes(hbase, per_track)
    d = np.stack([rng.choice(np.arange(0, 300), per_track, replace=False) for _ in range(tracks)])
    d[::2, 0] = -rng.integers(1, 9, len(d[::2]))
    d = np.stack([row[rng.permutation(per_track)] for row in d])  # the smallest d at any of the records
    tr = tbase + np.arange(tracks)
    post = _postings(np.tile(h, tracks), np.repeat(tr, per_track), (d + tq[None, :]).ravel())
    return post[rng.permutation(len(post))], records(h, tq), 1


def long_run(n: int, track: int = 42, d: int = 17, mm: int = 5, hbase: int = 0):
    """One track, one d, n records at t_q = 0 .. n - 1: the row [n, track, d, 0, n - 1], n distinct (track, d, t_q)."""
    tq = np.arange(n)
    h = hashes(hbase, n)
    return _postings(h, track, tq + d), records(h, tq), mm


def heavy(seed: int = 0, hbase: int = 0, tbase: int = 0, mm: int = 5):
    """300 records x 900 filler postings per hash (random tracks and times, as test_gpu_match_load.py) plus the true
    track tbase + 7 on every record at d = 100: 300 * 901 votes, above kLdsMaxVotes = 2^18."""
    rng = np.random.default_rng([seed, 300])
    n, per_hash = 300, 900
    tq = 2 * np.arange(n)
    h = hashes(hbase, n)
    fill = _postings(np.repeat(h, per_hash), tbase + rng.integers(1000, 9000, n * per_hash),
                     rng.integers(0, 3000, n * per_hash))
    post = np.concatenate([_postings(h, tbase + 7, tq + 100), fill])
    return post, records(h, tq), mm


def high_min_match(mm: int, seed: int = 0, hbase: int = 0, tbase: int = 0):
    """Tracks tbase + 1, + 2, + 3 with exactly mm - 1, mm and mm + 1 distinct frames at one offset each, and track
    tbase + 4 with 2 * mm + 2 raw votes on mm - 1 distinct t_q: its postings are stored twice, and two further
    records (own hashes) repeat the t_q of records 0 and 1. Only + 2 and + 3 are rows. A few hundred filler postings."""
    rng = np.random.default_rng([seed, mm])
    n = mm + 1
    tq = 3 + 3 * np.arange(n)
    h = hashes(hbase, n + 2)
    qh, qt = h, np.concatenate([tq, tq[:2]])  # records n and n + 1 share t_q with records 0 and 1
    parts = [_postings(h[: mm - 1], tbase + 1, tq[: mm - 1] + 20),
             _postings(h[:mm], tbase + 2, tq[:mm] - 3),
             _postings(h[:n], tbase + 3, tq + 150)]
    four = np.concatenate([_postings(h[: mm - 1], tbase + 4, tq[: mm - 1] + 61), _postings(h[n:], tbase + 4, tq[:2] + 61)])
    parts += [four, four]
    nf = 300
    parts.append(_postings(rng.choice(h, nf), tbase + rng.integers(100, 5000, nf), rng.integers(0, 3000, nf)))
    post = np.concatenate(parts)
    order = rng.permutation(len(qh))
    return post[rng.permutation(len(post))], records(qh[order], qt[order]), mm


def group_edges(n: int, mm: int, absent: int = 0, seed: int = 0, hbase: int = 0, tbase: int = 0):
    """The true track tbase + 5 matches n records (distinct t_q, in no order) at d = 33; every record's bucket is
    padded to a length drawn from GROUP_EDGE_LENGTHS (each at least once from n = 12 on, short ones more often) with
    filler postings of tracks tbase + 1000 .., the true posting arriving first, in the middle or last. `absent`
    further records, spread among the others, have hashes the index does not hold (empty buckets between full
    ones): the query then has n + absent records, and the true row still counts n."""
    rng = np.random.default_rng([seed, n, mm, absent])
    m = n + absent
    h = hashes(hbase, m)
    is_abs = np.zeros(m, dtype=bool)
    is_abs[rng.choice(m, absent, replace=False)] = True
    tq_all = 5 + rng.permutation(m)
    L = np.array(GROUP_EDGE_LENGTHS)
    # up to 65 records the short lengths are drawn far more often: the whole query stays below kFastVoteCap keys, so
    # at min_match 1 (every vote a candidate) the LDS path itself answers it
    w = np.array([14, 14, 3, 3, 3, 1, 1, 1, 0.3, 0.3, 0.3, 0.1] if n <= 65 else [6, 6, 4, 4, 4, 3, 3, 3, 1, 1, 1, 0.5])
    lens = rng.choice(L, n, p=w / w.sum())
    lens[: min(n, len(L))] = rng.permutation(L)[: min(n, len(L))]
    lens = lens[rng.permutation(n)]
    parts = []
    for i, (hi, tqi) in enumerate(zip(h[~is_abs], tq_all[~is_abs])):
        k = int(lens[i]) - 1
        fill = _postings(np.full(k, hi), tbase + 1000 + rng.integers(0, 150, k), rng.integers(0, 4000, k))
        true = _postings([hi], tbase + 5, [tqi + 33])
        at = (0, k // 2, k)[i % 3]
        parts += [fill[:at], true, fill[at:]]
    order = rng.permutation(m)
    return np.concatenate(parts), records(h[order], tq_all[order]), mm


def frame_bound(hbase: int = 0, track: int = 9):
    """min_match 2: records at t_q = 0 and at kMaxQueryFrame = 2^20 - 2, one track at d = 5."""
    tq = np.array([0, (1 << 20) - 2])
    h = hashes(hbase, 2)
    return _postings(h, track, tq + 5), records(h, tq), 2


def cut_ties(seed: int = 0, hbase: int = 0, tbase: int = 0, mm: int = 10):
    """60 tracks with shuffled ids: 45 match all 12 records, 15 match 11 of them. With max_results = 50 the last five
    rows are the five smallest ids among the count-11 tracks (best_counts tells the two groups apart)."""
    rng = np.random.default_rng([seed, 60])
    ids = tbase + rng.permutation(np.arange(100, 1000))[:60]
    tq = 6 + 5 * np.arange(12)
    h = hashes(hbase, 12)
    parts = []
    for j, tr in enumerate(ids):
        keep = np.ones(12, dtype=bool)
        if j >= 45:
            keep[rng.integers(0, 12)] = False
        parts.append(_postings(h[keep], tr, tq[keep] + int(rng.integers(-6, 500))))
    post = np.concatenate(parts)
    return post[rng.permutation(len(post))], records(h, tq), mm
