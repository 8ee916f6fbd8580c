"""tests/store_ref.py on the CPU: the model against per-posting Python loops, the checksum's sensitivity to order and
position, and the preconditions of every constructed case the GPU tests (test_gpu_store_edges.py,
test_gpu_store_model.py) rest on, so that a case which no longer crosses its edge fails here and not silently there."""

import numpy as np
import pytest

import k5_fixtures as F
import oracle as O
import store_ref as S
from aidfp import synth
from aidfp.catalog import checksum_np

M64 = (1 << 64) - 1


# ---------------------------------------------------------------- the model against brute force
def small_model(seed, n=300):
    rng = np.random.default_rng(seed)
    m = S.StoreModel()
    post = np.stack([S.valid_hash(rng.integers(0, 40, n) * 1_600_000 + 5), rng.integers(0, 9, n), rng.integers(0, 500, n)],
                    axis=1).astype(np.uint32)
    m.add(post[:200])
    m.add_track(11)
    for t in (2, 7, 11):
        m.remove(t)
    m.add(post[200:])  # tracks 2 and 7 again: dead on arrival
    return m


def brute_live(m):
    return [row for row in m.post.tolist() if not m.tomb[row[1]]]


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def brute_checksum(rows):
    acc = 0
    for i, (h, tr, t) in enumerate(rows):
        acc += mix64(((h << 32) | t) ^ ((tr * 0x9E3779B97F4A7C15) & M64) ^ ((i * 0xD6E8FEB86659FD93) & M64))
    return acc & M64


def test_bucket_key_equals_the_k5_fixture_one():
    rng = np.random.default_rng(0)
    h = np.concatenate([rng.integers(0, 1 << 32, 100000, dtype=np.uint64), [0, 0xFFFFFFFF, 0xFFC00000, 0x003FFFFF]]).astype(np.uint32)
    assert np.array_equal(S.bucket_key(h), F.bucket_key(h))
    c = rng.integers(0, S.KEYS, 100000)
    assert np.array_equal(S.valid_hash(c), np.concatenate([F.hashes(int(x), 1) for x in c[:200]] + [S.valid_hash(c[200:])]))
    assert len(np.unique(S.bucket_key(S.valid_hash(np.arange(1 << 16) * 1024 + 3)))) == 1 << 16  # distinct hashes, distinct buckets
    assert not (S.valid_hash(c) & 0xFC0).any()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_equals_brute_force(seed):
    m = small_model(seed)
    live = brute_live(m)
    assert 0 < len(live) < len(m.post) and m.dead()[200:].any()
    assert m.live().tolist() == live
    # csr: per key the live postings in arrival order; offsets from a histogram counted one posting at a time
    buckets, cnt = {}, np.zeros(S.KEYS, np.int64)
    for h, tr, t in live:
        k = int(F.bucket_key(np.uint32(h)))
        buckets.setdefault(k, []).append(tr | (t << 32))
        cnt[k] += 1
    offs, posts = m.csr()
    assert posts.tolist() == [p for k in sorted(buckets) for p in buckets[k]]
    assert offs.dtype == np.uint32 and len(offs) == S.KEYS + 1 and offs[0] == 0
    assert np.array_equal(offs[1:], np.cumsum(cnt))
    keys, posts2 = m.csr_sorted()
    assert np.array_equal(posts2, posts) and S.offsets_equal(offs, keys)
    # checksum, whole and in ranges
    rows = m.post.tolist()
    assert m.checksum() == brute_checksum(rows)
    for first, count in ((0, 0), (0, 1), (1, 1), (17, 100), (299, 1), (300, 0)):
        assert m.checksum(first, count) == brute_checksum(rows[first:first + count]), (first, count)
    for bad in ((-1, 1), (0, -1), (0, 301), (300, 1)):
        with pytest.raises(ValueError):
            m.checksum(*bad)
    # compact
    tomb = m.tomb.copy()
    assert m.compact() == len(rows) - len(live)
    assert m.post.tolist() == live and np.array_equal(m.tomb, tomb) and m.n_tracks == 12
    assert m.compact() == 0


def test_remove_raises_and_changes_nothing():
    m = small_model(4)
    before = (m.post.copy(), m.tomb.copy(), m.n_tracks)
    for bad in (2, 11, 12, 5000, -1):  # removed twice, removed empty, unknown
        with pytest.raises(ValueError):
            m.remove(bad)
    assert np.array_equal(m.post, before[0]) and np.array_equal(m.tomb, before[1]) and m.n_tracks == before[2]
    m.remove(10)  # a slot no posting names can be removed
    m.reset()
    assert len(m.post) == 0 and m.n_tracks == 0 and len(m.tomb) == 0 and m.checksum() == 0


def test_checksum_sees_order_and_position():
    m = small_model(5)
    p = m.post.copy()
    i, j = 10, 200
    assert not np.array_equal(p[i], p[j])
    q = p.copy()
    q[[i, j]] = q[[j, i]]
    assert checksum_np(q) != checksum_np(p)
    # the same rows with the position term counted from 1 and not from 0: what the kernel would sum if it numbered
    # the rows of a range [first, first + count) from `first` and not from 0
    rows = p[1:101]
    assert m.checksum(1, 100) == checksum_np(rows) == checksum_np(rows, first_index=0)
    assert checksum_np(rows, first_index=1) != checksum_np(rows)
    assert checksum_np(rows, first_index=333) != checksum_np(rows)


def test_offsets_equal_is_exact():
    keys = np.sort(np.random.default_rng(6).integers(0, S.KEYS, 500))
    keys[100:140] = keys[100]
    keys = np.sort(keys)
    offs = S.csr_offsets(keys)
    assert S.offsets_equal(offs, keys)
    uk = np.unique(keys)
    gap = int(uk[50] + (uk[51] - uk[50]) // 2)
    for where, delta in ((gap, 1), (int(uk[50]), 1), (int(uk[50]) + 1, -1), (S.KEYS, 1), (0, 1), (1, 1)):
        bad = offs.copy()
        bad[where] = int(bad[where]) + delta
        assert not np.array_equal(bad, offs) and not S.offsets_equal(bad, keys), where
    assert not S.offsets_equal(offs[:-1], keys)
    assert S.offsets_equal(np.zeros(S.KEYS + 1, np.uint32), keys[:0])


def test_bucket_multisets_ignore_order_inside_a_bucket_only():
    m = small_model(7)
    keys, posts = m.csr_sorted()
    uk, start, cnt = np.unique(keys, return_index=True, return_counts=True)
    b = int(np.argmax(cnt))
    assert cnt[b] >= 3
    shuffled = posts.copy()
    shuffled[start[b]:start[b] + cnt[b]] = shuffled[start[b]:start[b] + cnt[b]][::-1]
    assert not np.array_equal(shuffled, posts)
    assert np.array_equal(S.bucket_multisets(shuffled, keys), S.bucket_multisets(posts, keys))
    moved = posts.copy()
    other = start[b] + cnt[b] if b + 1 < len(uk) else start[b] - 1
    moved[[start[b], other]] = moved[[other, start[b]]]
    assert not np.array_equal(S.bucket_multisets(moved, keys), S.bucket_multisets(posts, keys))


def test_snapshot_layout_and_round_trip():
    m = small_model(8)
    blob = m.snapshot_bytes(7, 16000, 256)
    n = len(m.post)
    assert blob[:8] == b"AIDFPIX1" and len(blob) == 8 + 48 + 12 * n + m.n_tracks
    assert np.frombuffer(blob, "<i8", 6, 8).tolist() == [7, 16000, 256, n, m.n_tracks, 0]
    for c in range(3):
        assert np.frombuffer(blob, "<u4", n, 56 + 4 * n * c).tolist() == m.post[:, c].tolist()
    assert blob[56 + 12 * n:] == bytes(m.tomb.tolist())
    back = S.StoreModel.from_snapshot(blob)
    assert back.header == (7, 16000, 256) and back.n_tracks == m.n_tracks
    assert np.array_equal(back.post, m.post) and np.array_equal(back.tomb, m.tomb)
    empty = S.StoreModel().snapshot_bytes(7, 16000, 256)
    assert len(empty) == 56 and S.StoreModel.from_snapshot(empty).n_tracks == 0
    for bad in (blob[:-1], blob + b"\0", b"X" + blob[1:]):
        with pytest.raises(ValueError):
            S.StoreModel.from_snapshot(bad)


# ---------------------------------------------------------------- the compaction patterns
def test_compaction_patterns_cut_waves_and_blocks():
    assert S.COMPACT_SIZES == (1, 63, 64, 65, 1023, 1024, 1025, 4097, 5 * 1024 + 17) and len(S.COMPACT_PATTERNS) == 12
    for n in S.COMPACT_SIZES:
        for pat in S.COMPACT_PATTERNS:
            post, victim = S.compact_case(pat, n)
            mask = S.compact_mask(pat, n)
            assert len(np.unique(post[:, 0])) == n and np.array_equal(post[:, 2], np.arange(n))  # every posting names its place
            assert np.array_equal(post[:, 1], mask.astype(np.uint32))
            assert victim == (5 if pat == "none_with_removed_track" else 1)
            m = S.StoreModel()
            m.add(post)
            m.add_track(victim)
            m.remove(victim)
            assert m.compact() == int(mask.sum())
            assert np.array_equal(m.post[:, 2], np.flatnonzero(~mask))
        waves, blocks = -(-n // 64), -(-n // 1024)
        lanes = lambda pat: [int(S.compact_mask(pat, n)[w * 64:(w + 1) * 64].sum()) for w in range(waves)]
        last = n - 64 * (waves - 1)
        assert S.compact_mask("first", n).sum() == 1 == S.compact_mask("last", n).sum()
        assert S.compact_mask("first", n)[0] and S.compact_mask("last", n)[n - 1]
        assert lanes("lane0") == [1] * waves
        assert lanes("lane63") == [1] * (waves - 1) + [1 if last == 64 else 0]
        assert lanes("all_but_lane63") == [63] * (waves - 1) + [min(last, 63)]
        assert lanes("alt_waves") == [(64 if w < waves - 1 else last) * (w % 2 == 0) for w in range(waves)]
        per_block = lambda pat: [int(S.compact_mask(pat, n)[b * 1024:(b + 1) * 1024].sum()) for b in range(blocks)]
        sizes = [min(1024, n - 1024 * b) for b in range(blocks)]
        assert per_block("alt_blocks") == [s * (b % 2 == 0) for b, s in enumerate(sizes)]
        assert per_block("block0") == [sizes[0]] + [0] * (blocks - 1)
        assert per_block("all_but_last_block") == sizes[:-1] + [0]
        assert per_block("every") == sizes and per_block("none_with_removed_track") == [0] * blocks
        r = S.compact_mask("random", n)
        assert n < 63 or (0.3 * n < r.sum() < 0.7 * n)
    assert {n % 1024 for n in S.COMPACT_SIZES} >= {0, 1, 1023} and max(S.COMPACT_SIZES) > 5 * 1024  # partial last blocks


# ---------------------------------------------------------------- the large stores
def test_scan_level_cases_cross_their_edges():
    assert [-(-n // S.SCAN_BLOCK) for n in S.LEVEL_SIZES] == [1024, 1025, 2050]
    n = S.LEVEL_SIZES[-1]
    post, gone = S.big_postings(n), S.big_removed(0.3)
    assert len(gone) == 900 and len(np.unique(gone)) == 900
    for k in S.LEVEL_SIZES:
        assert np.array_equal(S.big_postings(k), post[:k])  # a prefix: one generator for every size
    assert len(np.unique(post[:, 0])) <= S.BIG_POOL < n // 10  # hash collisions
    assert not (post[:, 0] & 0xFC0).any() and int(post[:, 1].max()) == S.BIG_TRACKS - 1 and int(post[:, 2].max()) < 1 << 13
    live = ~np.isin(post[:, 1], gone)
    per_block = np.add.reduceat(live.astype(np.int64), np.arange(0, n, S.SCAN_BLOCK))
    # the blocks' live counts vary, and every group of 1024 blocks (one block of the second scan level) carries a sum
    # of its own into the next, so a wrong level-2 offset moves whole groups of postings
    assert len(np.unique(per_block)) > 50
    groups = np.add.reduceat(per_block, np.arange(0, len(per_block), 1024))
    assert len(groups) == 3 and len(set(groups.tolist())) == 3 and groups.min() > 0
    assert 0.25 * n < n - live.sum() < 0.35 * n
    # the checksum cases: counts on both sides of one grid of k_index_checksum, from three starts
    assert n > 333 + S.CHECKSUM_GRID + 1


@pytest.fixture(scope="module")
def atomic():
    post, gone, rec = S.atomic_case()
    m = S.StoreModel()
    m.add(post)
    for t in gone.tolist():
        m.remove(t)
    return m, rec


def test_atomic_case_plants_buckets_in_both_trips(atomic):
    m, rec = atomic
    n = len(m.post)
    assert n > 2 * S.BUILD_GRID and n > S.SIG_GRID  # second trips of k_index_count / k_index_scatter
    offs, posts = m.csr()
    assert len(posts) == len(m.live()) > S.SIG_GRID + 2 * S.PLANT_PER_SIDE  # ... and of k_make_sig
    h = (rec & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    keys = S.bucket_key(h)
    assert len(np.unique(keys)) == 2 * S.PLANT_PER_SIDE
    top, low = keys[:S.PLANT_PER_SIDE], keys[S.PLANT_PER_SIDE:]
    assert (h[:S.PLANT_PER_SIDE] >= 0xFFC00000).all() and top.min() >= S.KEYS - (1 << 16) and low.max() < 1 << 16
    assert int((offs[top] >= S.SIG_GRID).sum()) >= 64
    assert int((offs[low + 1] <= S.BUILD_GRID).sum()) >= 64
    # every planted bucket holds the planted posting
    for k, r in zip(keys.tolist(), rec.tolist()):
        want = S.PLANT_TRACK | ((r >> 32) << 32)
        assert want in posts[offs[k]:offs[k + 1]].tolist()
    rows = O.query(m.live(), rec, min_match=5, max_rows=20)
    assert rows[0].tolist() == [2 * S.PLANT_PER_SIDE, S.PLANT_TRACK, 0, 100, 100 + 3 * (2 * S.PLANT_PER_SIDE - 1)]
    assert int(posts.max() >> np.uint64(32)) < 1 << 20 and S.PLANT_TRACK < 1 << 18  # bucket_multisets' packing


# ---------------------------------------------------------------- the appends
def test_append_clips_cross_the_trip_edges():
    clips = S.append_clips(synth.synth)
    assert len(clips) == S.APPEND_CLIPS > S.APPEND_TRIP and S.APPEND_PREFIXES == (1024, 1025, 1100)
    assert [len(clips[c]) for c in sorted(S.APPEND_EMPTY)] == [0, 100, 16000, 2047]
    full = [c for c in range(S.APPEND_CLIPS) if c not in S.APPEND_EMPTY]
    recs = O.fingerprint_batch(np.stack([clips[c] for c in full]), S.APPEND_HOP, threads=16)
    assert min(len(r) for r in recs) >= 48
    for c in S.APPEND_EMPTY:
        assert len(O.fingerprint(clips[c], S.APPEND_HOP)) == 0
    assert {0, S.APPEND_TRIP - 1, S.APPEND_TRIP, S.APPEND_CLIPS - 1} == set(S.APPEND_EMPTY)  # zero counts at both sides of the edge
    long = S.long_clips(synth.synth)
    counts = [len(O.fingerprint(x, S.APPEND_HOP)) for x in long]
    assert counts[0] >= 48 and counts[1] > S.RECORD_TRIP and counts[2] == 0
    m = S.appended_twice([np.arange(3, dtype=np.uint64), np.zeros(0, np.uint64)], [4, 9])
    assert m.n_tracks == S.APPEND_SHIFT + 10 and m.post[:, 1].tolist() == [4] * 3 + [4 + S.APPEND_SHIFT] * 3


# ---------------------------------------------------------------- the operation traces
@pytest.fixture(scope="module")
def clip_records():
    cache = {}

    def records(t):
        if t not in cache:
            cache[t] = O.fingerprint(synth.synth(t, 0, S.APPEND_SR, S.APPEND_SR, salt=t), S.APPEND_HOP)
        return cache[t]

    return records


@pytest.mark.parametrize("seed", S.TRACE_SEEDS)
def test_trace_meets_its_coverage_conditions(seed, clip_records):
    ops = S.make_trace(seed, clip_records)
    again = S.make_trace(seed, clip_records)
    assert len(ops) == S.TRACE_OPS == 40
    assert all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(ops, again))  # a function of the seed
    rp = S.Replay(clip_records)
    planted_hits = 0
    for i, (kind, arg) in enumerate(ops):
        if kind in ("add_host", "add_device", "add_dead"):
            assert 1 <= len(arg) <= 3000 and set(arg[:, 1].tolist()) <= set(S.TRACE_IDS) and not (arg[:, 0] & 0xFC0).any()
            dead = rp.model.n_tracks > int(arg[:, 1].max()) and rp.model.tomb[arg[:, 1]].all()
            assert dead == (kind == "add_dead") and (kind == "add_dead" or not rp.model.tomb[arg[:, 1][arg[:, 1] < rp.model.n_tracks]].any())
        if kind == "add_extracted":
            assert len(set(arg)) == 2 and set(arg) <= set(S.TRACE_IDS)
        rp.apply(kind, arg)
        if i % 3 == 2:
            live, dead = rp.queries()
            if live:
                rows = O.query(rp.model.live(), live[1], min_match=5, max_rows=20)
                planted_hits += int(live[0] in rows[:, 1].tolist())
            if dead:
                assert dead[0] not in O.query(rp.model.live(), dead[1], min_match=5, max_rows=20)[:, 1].tolist()
    c = S.trace_conditions(rp.facts)
    assert c["least_kind_count"] >= 3, c
    assert c["compactions_that_drop"] >= 2 and c["compactions_that_drop_after_a_load"] >= 1, c
    assert c["growths_after_a_removal"] >= 1, c
    assert c["dead_adds_before_a_finalize"] >= 1, c
    assert c["bad_removals_that_raise"] == sum(1 for k, _ in ops if k == "remove_bad"), c
    assert planted_hits >= 5, planted_hits


def test_traces_grow_the_tombstone_buffer_both_ways(clip_records):
    """Past 1024 ids (a doubling) and past twice the capacity (id 70000), each at least once after a removal."""
    kinds = set()
    for seed in S.TRACE_SEEDS:
        rp = S.Replay(clip_records)
        for kind, arg in S.make_trace(seed, clip_records):
            rp.apply(kind, arg)
        kinds |= set(S.trace_conditions(rp.facts)["growth_kinds_after_a_removal"])
    assert kinds == {"double", "jump"}
