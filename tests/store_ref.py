"""A numpy model of the posting store (csrc/index_host.cpp: the SoA planes p_hash, p_track, p_t and the tombstones) and
of what is rebuilt from it: the CSR K4 must build, the order-sensitive checksum, the AIDFPIX1 snapshot. Plain numpy,
no engine and no GPU: the GPU tests (test_gpu_store_edges.py, test_gpu_store_model.py) take every expected value from
here or from oracle/, and test_store_ref_host.py pins this file to brute-force loops and checks the preconditions of
every constructed case below.

The one statement of `bucket_key` and the CSR mirror for the test files (tests/k5_fixtures.py keeps its own
bucket_key, which the host test compares with this one)."""

import numpy as np

from aidfp.catalog import checksum_np

U32, U64 = np.uint32, np.uint64
KEYS = 1 << 26
MAGIC = b"AIDFPIX1"

# the sizes at which the store's kernels take a second trip or scan level (csrc/index.hip, csrc/index_host.cpp)
APPEND_TRIP = 1024          # k_append_offsets: clips per trip of its one workgroup
RECORD_TRIP = 16 * 256      # k_records_to_postings: records of one clip per grid-stride trip
SCAN_BLOCK = 1024           # launch_compact / launch_scan: postings (counts) per block
SCAN_LEVEL = 1024 * 1024    # ... and per scan level: above it launch_scan recurses on the block sums
CHECKSUM_GRID = 4096 * 256  # k_index_checksum
BUILD_GRID = 8192 * 256     # k_index_count / k_index_scatter (the atomic build)
SIG_GRID = 16384 * 256      # k_make_sig
TOMB_FLOOR = 1024           # reserve_tracks: the tombstone buffer's first capacity


def bucket_key(h) -> np.ndarray:
    """aidfp_layout.h bucket_key: the CSR bucket of a hash, a permutation of the 26 bits FPSPEC 6 can set (int64)."""
    h = np.asarray(h).astype(np.int64)
    return (((h >> 22) & 0xFF) << 18) | (((h >> 30) & 3) << 16) | (((h >> 12) & 0x7F) << 9) | (((h >> 19) & 0x7) << 6) | (h & 0x3F)


def valid_hash(c) -> np.ndarray:
    """Number c of the 2^26 landmark hashes FPSPEC 6 can form (bits 6..11 clear), so distinct hashes are distinct
    buckets and the oracle (which joins on the whole hash) and the CSR (which joins on the bucket) agree."""
    c = np.asarray(c, dtype=np.int64)
    return ((((c >> 16) & 0x3FF) << 22) | (((c >> 6) & 0x3FF) << 12) | (c & 0x3F)).astype(U32)


def columns(post: np.ndarray):
    """The three contiguous uint32 columns Engine.index_add_postings takes."""
    return tuple(np.ascontiguousarray(post[:, c], dtype=U32) for c in range(3))


def record_rows(track: int, rec: np.ndarray) -> np.ndarray:
    """Records (hash | t << 32) of one clip -> its postings [n, 3] under `track`, in record order."""
    rec = np.asarray(rec, dtype=U64)
    return np.stack([(rec & U64(0xFFFFFFFF)).astype(U32), np.full(len(rec), track, U32), (rec >> U64(32)).astype(U32)],
                    axis=1).reshape(-1, 3)


def records_of(post: np.ndarray) -> np.ndarray:
    """Postings -> query records hash | t << 32 (a query that meets them at d = 0)."""
    return post[:, 0].astype(U64) | (post[:, 2].astype(U64) << U64(32))


# ---------------------------------------------------------------- the CSR mirror
def csr_sorted(post: np.ndarray, removed=()):
    """(keys, posts) of the live postings stably sorted by bucket key (a bucket keeps arrival order): keys int64,
    posts track | t << 32."""
    post = np.asarray(post, dtype=U32).reshape(-1, 3)
    p = post[~np.isin(post[:, 1], np.asarray(list(removed), dtype=U32))]
    keys = bucket_key(p[:, 0])
    order = np.argsort(keys, kind="stable")
    return keys[order], p[order, 1].astype(U64) | (p[order, 2].astype(U64) << U64(32))


def csr_offsets(keys: np.ndarray) -> np.ndarray:
    """offsets[k] = live postings with key < k: the prefix sums of the key histogram, 2^26 + 1 entries."""
    offs = np.zeros(KEYS + 1, U32)
    offs[1:] = np.cumsum(np.bincount(keys, minlength=KEYS)).astype(U32)
    return offs


def csr_mirror(post: np.ndarray, removed=()):
    """The CSR K4 must build from stored postings [n, 3] (hash, track, t): live postings stably sorted by bucket key,
    values track | t << 32, offsets[k] = live postings with key < k."""
    keys, posts = csr_sorted(post, removed)
    return csr_offsets(keys), posts


def offsets_equal(got: np.ndarray, keys: np.ndarray) -> bool:
    """got == csr_offsets(keys), for sorted keys, in one pass over the 2^26 + 1 entries instead of three (the small
    compaction cases run it a hundred times). The wanted array is a step function: 0 up to the first key, and after
    each distinct key k it steps to the count of keys <= k. `got` equals it if and only if it has 2^26 + 1 entries,
    never decreases, starts at 0, and has the wanted values on both sides of every step: between two steps a
    non-decreasing array is held between two equal values."""
    got = np.asarray(got)
    if got.shape != (KEYS + 1,) or got[0] != 0 or not np.all(got[1:] >= got[:-1]):
        return False
    uk, cnt = np.unique(keys, return_counts=True)
    hi = np.cumsum(cnt)
    if len(uk) == 0:
        return int(got[-1]) == 0
    return bool(np.array_equal(got[uk + 1], hi) and np.array_equal(got[uk], hi - cnt) and int(got[-1]) == int(hi[-1]))


def bucket_multisets(posts: np.ndarray, keys: np.ndarray) -> np.ndarray:
    """Every bucket's postings as a sorted multiset (the atomic build keeps no arrival order inside a bucket): the
    (key, track, t) triples packed into one u64 each and sorted. Needs track < 2^18 and t < 2^20."""
    posts = np.asarray(posts, dtype=U64)
    tr, t = posts & U64(0xFFFFFFFF), posts >> U64(32)
    assert len(posts) == len(keys) and (len(posts) == 0 or (int(tr.max()) < (1 << 18) and int(t.max()) < (1 << 20)))
    return np.sort((np.asarray(keys).astype(U64) << U64(38)) | (tr << U64(20)) | t)


# ---------------------------------------------------------------- the model
class StoreModel:
    """post [n, 3] u32 rows (hash, track, t) in arrival order, tomb u8 per track id, n_tracks."""

    def __init__(self):
        self.reset()

    def reset(self) -> None:
        self.post = np.zeros((0, 3), U32)
        self.tomb = np.zeros(0, np.uint8)
        self.n_tracks = 0

    def _slots(self, n_tracks: int) -> None:
        if n_tracks > self.n_tracks:
            self.tomb = np.concatenate([self.tomb, np.zeros(n_tracks - self.n_tracks, np.uint8)])
            self.n_tracks = n_tracks

    def add(self, post: np.ndarray) -> None:
        """Append; n_tracks grows to the largest id + 1. A posting of an already removed id is stored but dead."""
        post = np.asarray(post, dtype=U32).reshape(-1, 3)
        if len(post) == 0:
            return
        self._slots(int(post[:, 1].max()) + 1)
        self.post = np.concatenate([self.post, post])

    def add_track(self, track: int) -> None:
        self._slots(int(track) + 1)

    def remove(self, track: int) -> None:
        if not (0 <= track < self.n_tracks) or self.tomb[track]:
            raise ValueError("track not indexed")
        self.tomb[track] = 1

    def removed(self) -> np.ndarray:
        return np.flatnonzero(self.tomb).astype(U32)

    def dead(self) -> np.ndarray:
        return self.tomb[self.post[:, 1]].astype(bool) if len(self.post) else np.zeros(0, bool)

    def live(self) -> np.ndarray:
        return self.post[~self.dead()]

    def compact(self) -> int:
        """Drop the dead postings, order kept; tombstones stay. Returns the number dropped."""
        keep = ~self.dead()
        dropped = int(len(keep) - keep.sum())
        self.post = self.post[keep]
        return dropped

    def csr_sorted(self):
        return csr_sorted(self.post, self.removed())

    def csr(self):
        return csr_mirror(self.post, self.removed())

    def checksum(self, first: int = 0, count: int = None) -> int:
        count = len(self.post) - first if count is None else count
        if first < 0 or count < 0 or first + count > len(self.post):
            raise ValueError("bad range")
        return checksum_np(self.post[first:first + count])

    def snapshot_bytes(self, abi: int, sr: int, hop: int) -> bytes:
        """The AIDFPIX1 file aid_index_save writes: magic, six int64 {abi, sr, hop, n_post, n_tracks, 0}, the three
        columns, n_tracks tombstone bytes."""
        hdr = np.array([abi, sr, hop, len(self.post), self.n_tracks, 0], "<i8")
        cols = [np.ascontiguousarray(self.post[:, c]).astype("<u4").tobytes() for c in range(3)]
        return MAGIC + hdr.tobytes() + b"".join(cols) + self.tomb[:self.n_tracks].tobytes()

    @classmethod
    def from_snapshot(cls, blob: bytes) -> "StoreModel":
        """The model a snapshot holds; its header's (abi, sr, hop) in `.header`."""
        if blob[:8] != MAGIC or len(blob) < 56:
            raise ValueError("not an AIDFPIX1 snapshot")
        abi, sr, hop, n, nt, zero = (int(v) for v in np.frombuffer(blob, "<i8", 6, 8))
        if n < 0 or nt < 0 or zero != 0 or len(blob) != 56 + 12 * n + nt:
            raise ValueError("corrupt AIDFPIX1 snapshot")
        m = cls()
        m.post = np.stack([np.frombuffer(blob, "<u4", n, 56 + 4 * n * c) for c in range(3)], axis=1).astype(U32).reshape(-1, 3)
        m.tomb = np.frombuffer(blob, np.uint8, nt, 56 + 12 * n).copy()
        m.n_tracks = nt
        m.header = (abi, sr, hop)
        return m


# ---------------------------------------------------------------- constructed cases: compaction patterns
SCRAMBLE = 0x9E3779B1  # odd: position -> hash is a bijection mod 2^32
COMPACT_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 4097, 5 * 1024 + 17)
COMPACT_PATTERNS = ("first", "last", "lane0", "lane63", "all_but_lane63", "alt_waves", "alt_blocks", "block0",
                    "all_but_last_block", "every", "random", "none_with_removed_track")


def compact_mask(pattern: str, n: int) -> np.ndarray:
    """Which of n postings the pattern removes (True = removed), by position: waves of 64, blocks of 1024
    (k_compact_count / k_compact_scatter)."""
    i = np.arange(n)
    if pattern == "first":
        return i == 0
    if pattern == "last":
        return i == n - 1
    if pattern == "lane0":
        return i % 64 == 0
    if pattern == "lane63":
        return i % 64 == 63
    if pattern == "all_but_lane63":
        return i % 64 != 63
    if pattern == "alt_waves":
        return (i // 64) % 2 == 0
    if pattern == "alt_blocks":
        return (i // SCAN_BLOCK) % 2 == 0
    if pattern == "block0":
        return i < SCAN_BLOCK
    if pattern == "all_but_last_block":  # keeps the last block, partial or whole
        return i < SCAN_BLOCK * ((n - 1) // SCAN_BLOCK)
    if pattern == "every":
        return np.ones(n, bool)
    if pattern == "random":
        return np.random.default_rng(n).random(n) < 0.5
    if pattern == "none_with_removed_track":
        return np.zeros(n, bool)
    raise KeyError(pattern)


def compact_case(pattern: str, n: int):
    """(postings, the track to add empty and remove): hash is the position scrambled by an odd multiplier, t the
    position, track 1 where the pattern removes and 0 where it keeps, so a misplaced posting names where it came
    from. `none_with_removed_track` removes the empty track 5 instead: compaction runs and drops nothing."""
    i = np.arange(n, dtype=np.int64)
    post = np.stack([(i * SCRAMBLE) & 0xFFFFFFFF, compact_mask(pattern, n).astype(np.int64), i], axis=1).astype(U32)
    return post, (5 if pattern == "none_with_removed_track" else 1)


# ---------------------------------------------------------------- constructed cases: the large stores
BIG_TRACKS = 3000
BIG_POOL = 200_000
LEVEL_SIZES = (SCAN_LEVEL, SCAN_LEVEL + 1, 2 * SCAN_LEVEL + SCAN_BLOCK + 5)  # nb = 1024, 1025, 2050 in launch_compact


def big_postings(n: int, seed: int = 7) -> np.ndarray:
    """n postings: hashes drawn from a pool of BIG_POOL valid hashes (about n / BIG_POOL postings per bucket), tracks
    uniform over BIG_TRACKS, t below 2^13. The prefix of a larger call with the same seed."""
    pool = valid_hash(np.random.default_rng(seed).choice(KEYS, BIG_POOL, replace=False))
    col = [np.random.default_rng([seed, c]).integers(0, hi, n) for c, hi in enumerate((BIG_POOL, BIG_TRACKS, 1 << 13))]
    return np.stack([pool[col[0]], col[1].astype(U32), col[2].astype(U32)], axis=1).astype(U32)


def big_removed(fraction: float, seed: int = 8) -> np.ndarray:
    """The sorted ids of a random `fraction` of the BIG_TRACKS tracks."""
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(BIG_TRACKS, int(round(BIG_TRACKS * fraction)), replace=False)).astype(U32)


# the atomic build past one grid: k_make_sig's second trip starts at CSR position SIG_GRID, so the LIVE postings must
# pass it; 1 % of the tracks removed leaves about 4.28 M of the 4,325,376 + 128 stored
ATOMIC_N = SIG_GRID + 131072
ATOMIC_REMOVED = 0.01
PLANT_TRACK = BIG_TRACKS  # an id of its own
PLANT_PER_SIDE = 64


def atomic_case():
    """(postings, removed ids, planted query records). The planted track's first 64 postings have hashes >= 0xFFC00000
    (k1 = 1023: the top 2^16 bucket keys, the end of the CSR), its last 64 hashes below 0x00400000 with k1 = 0 (the
    first 2^16 keys, the CSR's start); every planted hash is a bucket of its own among the planted ones. The query
    meets all 128 at d = 0."""
    post = big_postings(ATOMIC_N)
    j = np.arange(PLANT_PER_SIDE, dtype=np.int64)
    top = valid_hash((1023 << 16) | (j * 997 + 13))
    low = valid_hash(j * 991 + 7)
    h = np.concatenate([top, low])
    plant = np.stack([h, np.full(len(h), PLANT_TRACK, U32), (100 + 3 * np.arange(len(h))).astype(U32)], axis=1).astype(U32)
    return np.concatenate([post, plant]), big_removed(ATOMIC_REMOVED), records_of(plant)


# ---------------------------------------------------------------- constructed cases: the appends
APPEND_SR, APPEND_HOP = 16000, 256
APPEND_CLIPS = 1100
APPEND_PREFIXES = (1024, 1025, 1100)
APPEND_EMPTY = {0: 0, 1023: 100, 1024: -1, APPEND_CLIPS - 1: 2047}  # clip -> length; -1: one second of zeros
APPEND_SHIFT = 5000  # the second append's track ids


def append_clips(synth):
    """The 1100 one-second clips (`synth` = aidfp.synth.synth), four of them replaced by clips without a record:
    zero counts on both sides of the 1024-clip trip edge of k_append_offsets, and at both ends."""
    clips = []
    for t in range(APPEND_CLIPS):
        if t in APPEND_EMPTY:
            n = APPEND_EMPTY[t]
            clips.append(np.zeros(APPEND_SR, np.float32) if n < 0 else synth(t, 0, n, APPEND_SR, salt=t))
        else:
            clips.append(synth(t, 0, APPEND_SR, APPEND_SR, salt=t))
    return clips


def long_clips(synth):
    """A 30 s clip (more than RECORD_TRIP records) between a 1 s clip and an empty one."""
    return [synth(1, 0, APPEND_SR, APPEND_SR, salt=1), synth(3, 0, 30 * APPEND_SR, APPEND_SR), np.zeros(0, np.float32)]


def appended_twice(recs, tracks) -> StoreModel:
    """The model after the batch's records were appended under `tracks`, then again under tracks + APPEND_SHIFT."""
    m = StoreModel()
    for shift in (0, APPEND_SHIFT):
        for t, r in zip(tracks, recs):
            m.add_track(int(t) + shift)
            m.add(record_rows(int(t) + shift, r))
    return m


# ---------------------------------------------------------------- random operation traces
TRACE_IDS = tuple(range(51)) + (1023, 1024, 1025, 70000)
TRACE_BIG_IDS = TRACE_IDS[51:]
TRACE_KINDS = ("add_host", "add_device", "add_track", "add_extracted", "remove_live", "remove_bad", "add_dead",
               "compact", "finalize", "save_load", "save_load_fresh", "reset")
TRACE_OPS = 40
TRACE_SEEDS = (29, 53, 70)  # chosen so that the generator alone meets trace_conditions (test_store_ref_host.py)
TRACE_HASH_POOL = 5000
PLANT_RECORDS = 40


class Replay:
    """Applies a trace's operations to a StoreModel and keeps what the tests ask about along the way: the query planted
    with each track (records that meet up to PLANT_RECORDS of its postings at d = 0), the tombstone buffer's capacity
    as reserve_tracks / aid_index_load / build_csr size it, and one fact sheet per operation (`facts`)."""

    def __init__(self, records):
        self.records = records  # track id -> the oracle's records of that id's one-second clip
        self.model = StoreModel()
        self.planted = {}  # track id -> query records, in the order the ids were last added
        self.cap = 0  # tombstone bytes the engine's device buffer holds
        self.loaded = False  # a load since the last reset
        self.dead_pending = False  # a dead-on-arrival add that no finalize has seen yet
        self.facts = []

    def _ensure(self, n_tracks: int, f: dict) -> None:
        m = self.model
        if n_tracks <= m.n_tracks:
            return
        want = max(n_tracks, TOMB_FLOOR)
        if want > self.cap:
            if self.cap:
                f["growth"] = "jump" if want > 2 * self.cap else "double"
                f["growth_with_tombs"] = bool(m.tomb.any())
            self.cap = max(want, 2 * self.cap)

    def _plant(self, post: np.ndarray) -> None:
        for t in np.unique(post[:, 1]).tolist():
            mine = post[post[:, 1] == t][:PLANT_RECORDS]
            self.planted.pop(t, None)
            self.planted[t] = records_of(mine)

    def apply(self, kind: str, arg) -> dict:
        m, f = self.model, {"kind": kind}
        if kind in ("add_host", "add_device", "add_dead"):
            self._ensure(int(arg[:, 1].max()) + 1, f)
            m.add(arg)
            self._plant(arg)
            if kind == "add_dead":
                self.dead_pending = True
        elif kind == "add_track":
            self._ensure(arg + 1, f)
            m.add_track(arg)
        elif kind == "add_extracted":
            self._ensure(max(arg) + 1, f)
            for t in arg:
                m.add_track(t)
                rows = record_rows(t, self.records(t))
                m.add(rows)
                if len(rows):
                    self._plant(rows)
        elif kind == "remove_live":
            m.remove(arg)
        elif kind == "remove_bad":
            try:
                m.remove(arg)
            except ValueError:
                f["raised"] = True
        elif kind == "compact":
            f["dropped"] = m.compact()
            f["after_load"] = self.loaded
        elif kind == "finalize":
            f["dead_seen"] = self.dead_pending
            self.dead_pending = False
            if m.n_tracks == 0:
                self.cap = max(self.cap, TOMB_FLOOR)
        elif kind in ("save_load", "save_load_fresh"):
            blob = m.snapshot_bytes(0, 0, 0)
            self.model = StoreModel.from_snapshot(blob)
            self.cap = max(self.model.n_tracks, TOMB_FLOOR)
            self.loaded = True
        elif kind == "reset":
            m.reset()
            self.planted.clear()
            self.loaded = False
            self.dead_pending = False
        else:
            raise KeyError(kind)
        self.facts.append(f)
        return f

    def queries(self):
        """((id, records) of the most recently added track that is live and has postings stored, (id, records) of
        the most recently added track that is removed); None where there is none."""
        m = self.model
        stored = set(np.unique(m.post[:, 1]).tolist())
        live = dead = None
        for t, rec in self.planted.items():
            if m.tomb[t]:
                dead = (t, rec)
            elif t in stored:
                live = (t, rec)
        return live, dead


def make_trace(seed: int, records, n_ops: int = TRACE_OPS):
    """n_ops operations (kind, argument), a pure function of the seed and of the clips' records."""
    rng = np.random.default_rng(seed)
    pool = valid_hash(rng.choice(KEYS, TRACE_HASH_POOL, replace=False))
    rp = Replay(records)
    ops = []

    def pick_id():
        return int(rng.choice(TRACE_BIG_IDS)) if rng.random() < 0.3 else int(rng.integers(0, 51))

    def not_removed(t):
        return t >= rp.model.n_tracks or not rp.model.tomb[t]

    def postings(ids):
        n = int(rng.integers(1, 3001))
        tr = np.asarray(ids, dtype=np.int64)[rng.integers(0, len(ids), n)]
        return np.stack([pool[rng.integers(0, len(pool), n)], tr, int(rng.integers(0, 2000)) + np.arange(n)],
                        axis=1).astype(U32)

    # a shuffled deck with every kind three times and the rest drawn at random; a kind the state does not allow yet
    # changes places with the next one in the deck that it does allow
    deck = list(TRACE_KINDS) * 3
    deck += [TRACE_KINDS[int(k)] for k in rng.integers(0, len(TRACE_KINDS), n_ops - len(deck))]
    deck = [deck[int(i)] for i in rng.permutation(len(deck))]

    def allowed(kind):
        m = rp.model
        if kind == "remove_live":
            return any(t < m.n_tracks and not m.tomb[t] for t in TRACE_IDS)
        if kind == "add_dead":
            return bool(m.tomb.any())
        return True

    for i in range(n_ops):
        j = next((j for j in range(i, n_ops) if allowed(deck[j])), None)
        if j is None:
            deck[i] = "add_host"
        else:
            deck[i], deck[j] = deck[j], deck[i]
        kind = deck[i]
        m = rp.model
        arg = None
        if kind == "remove_live":
            cand = [t for t in TRACE_IDS if t < m.n_tracks and not m.tomb[t]]
            arg = int(cand[int(rng.integers(0, len(cand)))])
        if kind == "add_dead":
            gone = m.removed().tolist()
            arg = postings([gone[int(rng.integers(0, len(gone)))]])
        if kind in ("add_host", "add_device"):
            ids = [t for t in {pick_id() for _ in range(int(rng.integers(1, 4)))} if not_removed(t)]
            arg = postings(ids or [next(t for t in TRACE_IDS if not_removed(t))])
        elif kind == "add_track":
            arg = pick_id()
        elif kind == "add_extracted":
            ids = [t for t in TRACE_IDS if not_removed(t)]
            a = pick_id()
            a = a if not_removed(a) else ids[0]
            b = ids[int(rng.integers(0, len(ids)))]
            arg = (a, b if b != a else ids[(ids.index(a) + 1) % len(ids)])
        elif kind == "remove_bad":
            gone = m.removed().tolist()
            arg = int(gone[int(rng.integers(0, len(gone)))]) if gone and rng.random() < 0.5 else m.n_tracks + int(rng.integers(0, 9))
        ops.append((kind, arg))
        rp.apply(kind, arg)
    return ops


def trace_conditions(facts) -> dict:
    """What test_store_ref_host.py asserts of every seed's trace."""
    kinds = [f["kind"] for f in facts]
    return {
        "least_kind_count": min(kinds.count(k) for k in TRACE_KINDS),
        "compactions_that_drop": sum(1 for f in facts if f["kind"] == "compact" and f["dropped"] > 0),
        "compactions_that_drop_after_a_load": sum(1 for f in facts if f["kind"] == "compact" and f["dropped"] > 0 and f["after_load"]),
        "growths_after_a_removal": sum(1 for f in facts if f.get("growth_with_tombs")),
        "growth_kinds_after_a_removal": sorted({f["growth"] for f in facts if f.get("growth_with_tombs")}),
        "dead_adds_before_a_finalize": sum(1 for f in facts if f["kind"] == "finalize" and f["dead_seen"]),
        "bad_removals_that_raise": sum(1 for f in facts if f.get("raised")),
    }
