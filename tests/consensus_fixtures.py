"""Constructed indexes for the K8b consensus tests (csrc/exact.hip `exact_consensus`): build the index, not the audio.

A few fixed 16 kHz clips from aidfp.synth are sliced into the exact lane's sub-windows exactly as aid_exact_windows /
aidfp.exact.extract_pcm_window slice them, and each window's records come from the CPU oracle (oracle.fingerprint).
Of each window a *pool* of records is kept: their hashes occur once among all the records of all the windows of all
the clips, and their t_q are pairwise distinct. A catalog track is a `Spec` (c_w, d_w per window): it gets the postings
(hash, track, t_q + d_w) of the first c_w pool records of window w, so K5's row for it in window w has count c_w and
reference_start (tq_min + d_w) * hop / sr, and the consensus sees exactly the totals, window sets and starts the spec
names. Tracks reuse the pool records freely. `steer()` names the decision edges (7 / 8 aligned hashes, halving, the
medians, confidence ties); `bulk()` fills a clip's three windows to the 768 rows the kernel stages.

numpy and the CPU oracles only, no GPU. `expected()` is the all-oracle lane: oracle.query per window (oracle/fp_match.c),
then aidfp.exact's consensus and ranking, which tests/test_glue_parity.py pins to the reference.
test_consensus_fixtures_host.py asserts every edge on that route; test_gpu_consensus_edges.py compares the lane to it."""

import itertools
import uuid
from dataclasses import dataclass, field

import numpy as np

import oracle as O
from aidfp import exact as ex
from aidfp import synth
from aidfp.fingerprint import OlafMatch

SR, HOP = 16000, 256
SEC = HOP / SR
MIN_MATCH, MAX_RESULTS = 1, 256  # the engine's: every vote a row, the most rows a window can have
MAX_STAGED = 3 * 256  # kExactMaxRows
U64 = np.uint64

# name -> (synth track, start sample, samples, snr_db): different audio per clip, so no two clips share a pool hash
CLIPS = {
    "cases": (6, 2 * SR, 5 * SR, None),
    "empty": (0, 0, 0, None),  # between two full clips: the later clips' window bases do not start at 3 * clip
    "bulk": (2, 2 * SR, 5 * SR, None),
    "whole": (1, 2 * SR, 5 * SR + 2, None),  # above 5 s: one query, nothing halved
    "one_window": (16, 11 * SR, int(0.7 * SR), 20),  # only window 0 is sent: every candidate is halved
    "two_windows": (10, 2 * SR, int(1.4 * SR), None),
}


@dataclass
class Spec:
    track: int
    c: tuple  # postings per sent window
    d: tuple  # frame offset per sent window
    tag: str


@dataclass
class Clip:
    name: str
    pcm: np.ndarray
    mode: int  # 1: sub-window consensus, 0: whole-clip aggregation
    windows: list  # (lo, len) of the windows that are sent
    records: list  # per sent window, uint64 (hash | t_q << 32)
    pools: list = field(default_factory=list)
    specs: list = field(default_factory=list)
    rows: list = field(default_factory=list)  # per sent window, the oracle's K5 rows on the batch's postings


@dataclass
class Batch:
    clips: list
    postings: np.ndarray  # uint32 [n, 3] (hash, track, t)

    def clip(self, name: str) -> Clip:
        return next(c for c in self.clips if c.name == name)


def window_plan(n: int, sr: int = SR):
    """(mode, [(lo, len)] of the windows that are sent), by aidfp.exact's own slicing of a clip of n samples."""
    pcm = bytes(4 * n)
    if ex.pcm_duration_sec(pcm, sr) > ex.SHORT_CLIP_THRESHOLD_SEC:
        return 0, [(0, n)]
    out = []
    for a, b in ex.SUB_WINDOWS:
        stop = min(b, n / sr)
        if not a < stop:
            continue
        piece = ex.extract_pcm_window(pcm, a, stop, sr)
        if piece:
            out.append((int(a * sr), len(piece) // 4))
    return 1, out


def _clip(name: str) -> Clip:
    track, start, n, snr = CLIPS[name]
    pcm = synth.synth(track, start, n, SR, snr_db=snr) if n else np.zeros(0, np.float32)
    mode, wins = window_plan(n)
    return Clip(name, pcm, mode, wins, [O.fingerprint(pcm[lo:lo + ln], HOP) for lo, ln in wins])


def _pools(clips) -> None:
    every = np.concatenate([r & U64(0xFFFFFFFF) for c in clips for r in c.records])
    u, cnt = np.unique(every, return_counts=True)
    once = set(u[cnt == 1].tolist())
    for c in clips:
        c.pools = []
        for r in c.records:
            seen, keep = set(), []
            for v in r.tolist():
                if (v & 0xFFFFFFFF) in once and (v >> 32) not in seen:
                    seen.add(v >> 32)
                    keep.append(v)
            c.pools.append(np.array(keep, dtype=U64))


def tq_min(pool: np.ndarray, c: int) -> int:
    return int((pool[:c] >> U64(32)).min())


def steer(pools, tbase: int) -> list:
    """The decision edges for a clip with these pools; an edge whose counts a pool cannot hold is left out (the host
    test says which clip must hold which). d is different for every (track, window) unless the tag says otherwise."""
    W, P = len(pools), [len(p) for p in pools]
    specs = []

    def add(tag, c, d=None):
        k = len(specs)
        if any(cw > pw for cw, pw in zip(c, P)):
            return
        d = tuple(d) if d is not None else tuple(1000 + 701 * k + 97 * w * w if c[w] else 0 for w in range(W))
        specs.append(Spec(tbase + k, tuple(c), d, tag))

    def only(ws, cs):
        c = [0] * W
        for w, cw in zip(ws, cs):
            c[w] = cw
        return c

    # confidence 1.0 at different counts, listed (by window 0's count, then by id) in neither count order
    if W >= 2:
        add("strong42", only((0, 1), (12, 30)))
        add("strong22", only((0, 1), (11, 11)))
        add("strong35", only((0, 1), (10, 25)))
    for w in range(W):
        for total in (15, 16, 17, 2, 40, 18, 7, 8):
            add(f"single{total}", only((w,), (total,)))
    for a, b in itertools.combinations(range(W), 2):
        for ca, cb in ((4, 4), (3, 4), (10, 9)):
            add(f"pair{ca}+{cb}", only((a, b), (ca, cb)))
    if W == 3:
        add("triple3+3+2", (3, 3, 2))
        for k, perm in enumerate(itertools.permutations((1000, 5000, 9000))):  # window orders of low, middle, high
            add("median" + "".join(str(x // 4000) for x in perm), (3, 3, 3), [x + 300 * k for x in perm])
        t0, t1 = tq_min(pools[0], 3), tq_min(pools[1], 3)
        add("median_two_equal", (3, 3, 3), (2000 + t1, 2000 + t0, 7000))  # windows 0 and 1 start at the same frame
    return specs


def bulk(pools, tbase: int, seed: int = 11) -> list:
    """254 tracks in all three windows (1..5 postings each, at least eight of them with a single one in window 0), 3
    in window 0 only and 2 + 2 in windows (0, 1) and (0, 2): 261 / 256 / 256 rows, so window 0 is cut to max_results
    and the clip stages 768 rows. The rows cut are window 0's count-1 rows of the largest ids."""
    rng = np.random.default_rng(seed)
    specs = []
    for k in range(254):
        c = rng.integers(1, 6, 3)
        if k >= 240:
            c[0] = 1
        specs.append(Spec(tbase + k, tuple(int(x) for x in c), tuple(int(x) for x in rng.integers(100, 40000, 3)),
                          "bulk"))
    for c, tag in (((16, 0, 0), "single16"), ((15, 0, 0), "single15"), ((17, 0, 0), "single17"), ((4, 4, 0), "pair4+4"),
                   ((3, 4, 0), "pair3+4"), ((4, 0, 4), "pair4+4"), ((3, 0, 4), "pair3+4")):
        k = len(specs)
        specs.append(Spec(tbase + k, c, tuple(1000 + 701 * k + 97 * w * w if c[w] else 0 for w in range(3)), tag))
    assert all(cw <= len(p) for s in specs for cw, p in zip(s.c, pools))
    return specs


def spec_postings(pools, specs) -> np.ndarray:
    parts = []
    for s in specs:
        for w, pool in enumerate(pools):
            r = pool[:s.c[w]]
            h = (r & U64(0xFFFFFFFF)).astype(np.int64)
            t = (r >> U64(32)).astype(np.int64) + s.d[w]
            parts.append(np.stack([h, np.full(len(r), s.track, np.int64), t], axis=1))
    p = np.concatenate(parts) if parts else np.zeros((0, 3), np.int64)
    assert p.size == 0 or (p.min() >= 0 and p[:, 1].max() < (1 << 20) and p[:, 2].max() < (1 << 31))
    return p.astype(np.uint32)


_BATCH = []


def batch() -> Batch:
    """The one batch of the tests (built once): the clips of CLIPS in that order, track ids 10000 * (clip + 1) + k."""
    if not _BATCH:
        clips = [_clip(name) for name in CLIPS]
        _pools(clips)
        for i, c in enumerate(clips):
            tbase = 10000 * (i + 1)
            c.specs = bulk(c.pools, tbase) if c.name == "bulk" else steer(c.pools, tbase) if c.pools else []
        post = np.concatenate([spec_postings(c.pools, c.specs) for c in clips])
        post = post[np.random.default_rng(5).permutation(len(post))]
        for c in clips:
            c.rows = [O.query(post, r, MIN_MATCH, MAX_RESULTS) for r in c.records]
        _BATCH.append(Batch(clips, post))
    return _BATCH[0]


def name_of(track: int) -> str:
    return str(uuid.UUID(int=int(track)))


def matches(rows: np.ndarray) -> list:
    """K5 rows (count, track, d, tq_min, tq_max) -> OlafMatch, as the service's adapter builds them."""
    return [OlafMatch(int(c), q0 * SEC, q1 * SEC, name_of(t), int(t), (q0 + d) * SEC, (q1 + d) * SEC)
            for c, t, d, q0, q1 in rows.tolist()]


def candidates(clip: Clip) -> list:
    """Every candidate of the clip before the threshold, in first-appearance order (aidfp.exact)."""
    per_window = [matches(r) for r in clip.rows]
    if not per_window:
        return []
    return ex.consensus_score(per_window) if clip.mode else ex.matches_to_candidates(per_window[0])


def expected(clip: Clip, max_out: int) -> np.ndarray:
    """The lane's rows for the clip, entirely off the GPU, in the engine's row type."""
    ranked = ex.rank(candidates(clip), max_out)
    out = np.zeros(len(ranked), dtype=[("track", "<u4"), ("aligned_hashes", "<i4"), ("offset_seconds", "<f8"),
                                       ("confidence", "<f8")])
    for i, c in enumerate(ranked):
        out[i] = (c.track_uuid.int, c.aligned_hashes, c.offset_seconds, c.confidence)
    return out
