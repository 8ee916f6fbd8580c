"""The posting store's own kernels (csrc/index.hip k_append_offsets, k_records_to_postings, k_compact_count,
k_compact_scatter, launch_scan, k_index_checksum, and the atomic build k_index_count / k_index_scatter / k_make_sig)
and its snapshot (csrc/index_host.cpp), at the sizes where a loop takes a second trip, a scan a second level, and a
removal pattern cuts waves and blocks. Every expected value comes from the numpy model (tests/store_ref.py) or from
oracle/; none from another engine call. test_store_ref_host.py checks on the CPU that each constructed case crosses the
edge it is named for.

Out of scope, on purpose: a third scan level of the compaction needs more than 2^30 stored postings, and the
2^24-posting chunk loop of aid_index_save / aid_index_load a 200 MB file per run."""

import numpy as np
import pytest

import oracle as O
import store_ref as S
from aidfp import _lib, synth
from aidfp.engine import Engine

pytestmark = pytest.mark.gpu
SR, HOP = S.APPEND_SR, S.APPEND_HOP


def add(eng, post):
    if len(post):
        h, tr, t = S.columns(post)
        eng.index_add_postings(h.ctypes.data, tr.ctypes.data, t.ctypes.data, len(post), device=False)


def check_store(eng, m):
    """The stored postings, their count, the track slots and the checksum equal the model's."""
    st = eng.index_stats()
    assert (st["postings"], st["tracks"]) == (len(m.post), m.n_tracks)
    got = eng.index_export()
    bad = np.flatnonzero((got != m.post).any(axis=1))
    assert len(bad) == 0, f"{len(bad)} stored postings differ, first at {bad[:5]}: {got[bad[:3]]} for {m.post[bad[:3]]}"
    assert eng.index_checksum() == m.checksum()


def check_csr(eng, m):
    """index_finalize, then the CSR equals model.csr(): the postings position for position, the offsets by
    store_ref.offsets_equal (the same equality in one pass over the 2^26 + 1 entries, proved there and pinned to the
    plain comparison by test_store_ref_host.py)."""
    eng.index_finalize()
    assert eng.index_stats()["live"] == len(m.live())
    offs, posts = eng.index_csr()
    keys, ref_posts = m.csr_sorted()
    assert len(posts) == len(ref_posts)
    bad = np.flatnonzero(posts != ref_posts)
    assert len(bad) == 0, f"{len(bad)} CSR postings out of place, first at {bad[:5]}"
    assert S.offsets_equal(offs, keys)


def check_compaction(eng, m):
    dropped = m.compact()
    assert eng.index_compact() == dropped
    check_store(eng, m)
    check_csr(eng, m)
    assert eng.index_compact() == 0
    check_store(eng, m)


# ---------------------------------------------------------------- compaction patterns (small)
@pytest.fixture(scope="module")
def small_engine():
    with Engine(SR) as eng:
        yield eng


@pytest.mark.parametrize("pattern", S.COMPACT_PATTERNS)
@pytest.mark.parametrize("n", S.COMPACT_SIZES)
def test_compaction_patterns(small_engine, n, pattern):
    """Removed postings that cut waves (the ballot and lane mask of k_compact_scatter) and 1024-blocks (the block
    offsets), at sizes around one wave, one block and a partial last block. A misplaced posting names its origin: t is
    its position before the compaction."""
    eng = small_engine
    eng.index_reset()
    post, victim = S.compact_case(pattern, n)
    m = S.StoreModel()
    add(eng, post)
    m.add(post)
    eng.index_add_records(victim, np.zeros(0, np.uint64))  # the slot alone
    m.add_track(victim)
    eng.index_remove(victim)
    m.remove(victim)
    check_store(eng, m)
    check_compaction(eng, m)
    if pattern == "every":  # the store is empty now; it still takes postings
        assert len(m.post) == 0
        more = S.compact_case("random", 777)[0]
        add(eng, more)
        m.add(more)
        check_store(eng, m)
        check_csr(eng, m)
        assert eng.index_stats()["live"] == int((more[:, 1] == 0).sum())


# ---------------------------------------------------------------- compaction across scan levels, checksum ranges
@pytest.fixture(scope="module")
def big():
    """The 2.1 M postings of the largest scan-level case (the smaller cases are its prefixes) and the removed ids."""
    return S.big_postings(S.LEVEL_SIZES[-1]), S.big_removed(0.3).tolist()


@pytest.mark.parametrize("n", S.LEVEL_SIZES)
def test_compaction_across_scan_levels(big, n):
    """1024, 1025 and 2050 blocks of 1024 postings: launch_scan with one block of counts (no second level), with two
    (a second level over two block sums, the second block nearly empty: n is no multiple of 1024 at either level) and
    with three. 30 % of 3000 tracks removed at random: the blocks keep varying numbers of postings, and a wrong
    second-level offset moves a thousand blocks at once."""
    post, gone = big
    m = S.StoreModel()
    m.add(post[:n])
    with Engine(SR) as eng:
        add(eng, post[:n])
        for t in gone:
            eng.index_remove(t)
            m.remove(t)
        check_compaction(eng, m)


CHECKSUM_COUNTS = (0, 1, 255, 256, 257, S.CHECKSUM_GRID - 1, S.CHECKSUM_GRID, S.CHECKSUM_GRID + 1, None)


@pytest.fixture(scope="module")
def big_store(big):
    """The 2.1 M postings stored and not compacted, ten tracks removed; the model of it."""
    post, gone = big
    m = S.StoreModel()
    m.add(post)
    with Engine(SR) as eng:
        add(eng, post)
        for t in gone[:10]:
            eng.index_remove(t)
            m.remove(t)
        yield eng, m


@pytest.mark.parametrize("first", [0, 1, 333])
def test_checksum_ranges(big_store, first):
    """k_index_checksum below, at and past one grid (4096 x 256 threads): the position term counts from `first`, the
    planes are read at first + i."""
    eng, m = big_store
    n = len(m.post)
    for count in CHECKSUM_COUNTS:
        count = n - first if count is None else count
        assert first + count <= n
        assert eng.index_checksum(first, count) == m.checksum(first, count), (first, count)


def test_checksum_bad_ranges_raise(big_store):
    """One posting past the end, from any start, and negative values: refused, and the index is as it was."""
    eng, m = big_store
    n = len(m.post)
    for first, count in ((0, n + 1), (1, n), (333, n - 332), (n + 1, 0), (-1, 5), (0, -1), (-1, -1)):
        assert first < 0 or count < 0 or first + count == n + 1
        with pytest.raises(_lib.EngineError):
            eng.index_checksum(first, count)
    assert eng.index_checksum(n, 0) == 0
    check_store(eng, m)


# ---------------------------------------------------------------- the atomic build past one grid
@pytest.fixture(scope="module")
def atomic():
    """The 4.3 M-posting store in an engine, and every expected value of it, once: the model, the mirror CSR, its
    buckets as sorted multisets, the planted query and the oracle's rows for it."""
    post, gone, rec = S.atomic_case()
    m = S.StoreModel()
    m.add(post)
    for t in gone.tolist():
        m.remove(t)
    keys, posts = m.csr_sorted()
    ref = {"model": m, "rec": rec, "keys": keys, "posts": posts, "offs": S.csr_offsets(keys),
           "multisets": S.bucket_multisets(posts, keys)}
    with Engine(SR, min_match=5) as eng:
        ref["rows"] = O.query(m.live(), rec, min_match=eng.min_match, max_rows=eng.max_results)
        add(eng, post)
        for t in gone.tolist():
            eng.index_remove(t)
        yield eng, ref


def build(eng, k4_build):
    eng.force("k4_build", k4_build)
    eng.force("k5_path", 0)
    eng.index_finalize()


def test_atomic_build_equals_the_mirror(atomic):
    """k_index_count / k_index_scatter (8192 x 256 threads) and k_make_sig (16384 x 256) on their second grid-stride
    trips, pinned to the mirror and not only to the radix build: offsets exact, every bucket's postings as a sorted
    multiset (the atomic build keeps no arrival order inside a bucket)."""
    eng, ref = atomic
    build(eng, 2)
    m = ref["model"]
    assert eng.index_stats() == {"postings": len(m.post), "live": len(ref["posts"]), "tracks": m.n_tracks}
    offs, posts = eng.index_csr()
    assert np.array_equal(offs, ref["offs"])
    assert np.array_equal(S.bucket_multisets(posts, ref["keys"]), ref["multisets"])


@pytest.mark.parametrize("k4_build", [2, 1], ids=["atomic", "radix"])
def test_planted_rows_past_one_grid(atomic, k4_build):
    """The planted query, half of whose buckets lie past CSR position 4,194,304 (k_make_sig's second trip) and half
    before 2,097,152, on the LDS path (1, which reads the signatures) and the global path (2): the oracle's rows, from
    the atomic build and from the radix build of the same store."""
    eng, ref = atomic
    want = ref["rows"]
    assert want[0, 1] == S.PLANT_TRACK and want[0, 0] == len(ref["rec"])
    build(eng, k4_build)
    for path in (1, 2):
        eng.force("k5_path", path)
        eng.match_stats(reset=True)
        assert np.array_equal(eng.query([ref["rec"]])[0], want), path
        st = eng.match_stats()
        if path == 1:  # answered from the signatures alone, no hand-back to the global path
            assert st["queries_lds"] == 1 and st["queries_global"] == 0 and st["sig_reads"] >= len(ref["rec"]), st
        else:
            assert st["queries_lds"] == 0 and st["queries_global"] >= 1, st
    eng.force("k5_path", 0)


def test_radix_build_of_the_same_store(atomic):
    """The default build of the store the atomic build was checked on: the mirror, position for position."""
    eng, ref = atomic
    build(eng, 1)
    offs, posts = eng.index_csr()
    assert np.array_equal(offs, ref["offs"])
    bad = np.flatnonzero(posts != ref["posts"])
    assert len(posts) == len(ref["posts"]) and len(bad) == 0, f"{len(bad)} CSR postings out of place, first at {bad[:5]}"


# ---------------------------------------------------------------- the appends
@pytest.fixture(scope="module")
def many_clips():
    """The 1100 clips and the oracle's records of each, once."""
    clips = S.append_clips(synth.synth)
    full = [c for c in range(len(clips)) if c not in S.APPEND_EMPTY]
    batch = O.fingerprint_batch(np.stack([clips[c] for c in full]), HOP, threads=16)
    recs = [np.zeros(0, np.uint64)] * len(clips)
    for c, r in zip(full, batch):
        recs[c] = r
    return clips, recs


def append_twice(clips, recs):
    """Extract and append the batch, check every clip's records against the oracle, then extract and append it again
    under ids shifted by 5000: the store equals the model's, in clip order, both times."""
    tracks = np.arange(len(clips), dtype=np.uint32)
    m = S.appended_twice(recs, tracks)
    with Engine(SR) as eng:
        for shift in (0, S.APPEND_SHIFT):
            got = eng.extract_host(clips)
            for c, (g, r) in enumerate(zip(got, recs)):
                assert np.array_equal(g, r), f"clip {c}: records differ from the oracle ({len(g)} for {len(r)})"
            eng.index_add_extracted(tracks + shift)
        check_store(eng, m)
        check_csr(eng, m)


@pytest.mark.parametrize("k", S.APPEND_PREFIXES)
def test_append_many_clips(many_clips, k):
    """k_append_offsets with 1024 clips (one trip), 1025 and 1100 (the carry into a second trip), record-less clips on
    both sides of the trip edge and at both ends. The first append of a fresh engine grows the planes (the counts come
    back to the host first) by its need plus one batch's hash capacity, so the second fits and takes the
    device-scanned asynchronous path, the one that runs k_append_offsets. Which path an append took cannot be observed
    through the API; the growth rule holds unless under a quarter of the device memory is free."""
    clips, recs = many_clips
    assert k > 1024 or k == S.APPEND_TRIP
    append_twice(clips[:k], recs[:k])


def test_append_long_clip():
    """A clip of more than 4096 records (the grid-stride trip of k_records_to_postings: 16 blocks x 256 threads per
    clip) between a one-second clip and an empty one, appended twice as above."""
    clips = S.long_clips(synth.synth)
    recs = [O.fingerprint(x, HOP) for x in clips]
    assert len(recs[1]) > S.RECORD_TRIP and len(recs[2]) == 0
    append_twice(clips, recs)


# ---------------------------------------------------------------- the snapshot
def snapshot_model():
    m = S.StoreModel()
    m.add(S.big_postings(5000))
    m.add_track(S.BIG_TRACKS + 40)  # trailing slots without postings
    return m


def test_snapshot_bytes_equal_the_model(tmp_path):
    """aid_index_save writes exactly the model's AIDFPIX1 bytes: without and with removed tracks, after a compaction,
    and for the empty store."""
    abi = _lib.load().aid_abi_version()
    path = tmp_path / "s.aidfp"
    with Engine(SR) as eng:
        def same(m, what):
            eng.index_save(str(path))
            assert path.read_bytes() == m.snapshot_bytes(abi, SR, HOP), what

        same(S.StoreModel(), "empty")
        m = snapshot_model()
        add(eng, m.post)
        eng.index_add_records(S.BIG_TRACKS + 40, np.zeros(0, np.uint64))
        same(m, "no removal")
        for t in (0, 17, S.BIG_TRACKS + 40):
            eng.index_remove(t)
            m.remove(t)
        same(m, "removed")
        assert eng.index_compact() == m.compact() > 0
        same(m, "compacted")
        eng.index_reset()
        same(S.StoreModel(), "reset")


def test_snapshot_written_by_the_model_loads(tmp_path):
    """A file the engine never wrote: export and checksum equal the model's, removed ids are still removed (a second
    removal raises, the removed track's own postings find no row of it), and a compaction drops the model's count."""
    abi = _lib.load().aid_abi_version()
    m = snapshot_model()
    victim = int(m.post[0, 1])
    rec = S.records_of(m.post[m.post[:, 1] == victim])
    keeper = int(m.post[m.post[:, 1] != victim][0, 1])
    rec_keep = S.records_of(m.post[m.post[:, 1] == keeper])
    m.remove(victim)
    m.remove(S.BIG_TRACKS + 40)
    path = tmp_path / "model.aidfp"
    path.write_bytes(m.snapshot_bytes(abi, SR, HOP))
    with Engine(SR, min_match=1) as eng:
        eng.index_load(str(path))
        check_store(eng, m)
        for t in (victim, S.BIG_TRACKS + 40):
            with pytest.raises(_lib.EngineError):
                eng.index_remove(t)
        for r in (rec, rec_keep):
            want = O.query(m.live(), r, min_match=1, max_rows=eng.max_results)
            got = eng.query([r])[0]
            assert np.array_equal(got, want) and victim not in got[:, 1].tolist()
        assert keeper in eng.query([rec_keep])[0][:, 1].tolist()
        check_compaction(eng, m)
        assert len(m.post) < 5000
