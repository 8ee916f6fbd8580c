"""numpy restatement of spec/FPSPEC.md 9.2 (the vector lane's filtered search), built on tests/vec_ref.py and
tests/vec_q8_ref.py: the oracle and the fixtures of tests/test_vec_filter_host.py and tests/test_gpu_vector_filter.py.
A helper, not a test module.

The only new rule is `passes`. The filtered hit list is `V.hit_list(S[q], passes, limit)` and the filtered prefilter
route is `Q.route(..., live=passes, ...)`: sections 9 and 9.1 with "live" read as "passes".
"""

from __future__ import annotations

from collections import namedtuple

import numpy as np
import vec_ref as V

F32 = np.float32
U64 = np.uint64
MAX_EXCLUDE = 8

Filt = namedtuple("Filt", "any_of all_of none_of exclude", defaults=(0, 0, 0, ()))
ZERO = Filt()


def passes(tags, tracks, live, filt) -> np.ndarray:
    """bool [n]: entry e is live, carries a tag of any_of (if any_of != 0), all of all_of, none of none_of, and its
    track is not excluded. filt None is the zero filter."""
    f = ZERO if filt is None else filt
    tags = np.asarray(tags, dtype=U64)
    ok = np.asarray(live, dtype=bool).copy()
    if f.any_of:
        ok &= (tags & U64(f.any_of)) != 0
    ok &= (tags & U64(f.all_of)) == U64(f.all_of)
    ok &= (tags & U64(f.none_of)) == 0
    for t in f.exclude:
        ok &= np.asarray(tracks) != t
    return ok


def normal(filt):
    """What makes two filters the same filter: the masks and the excluded ids as a set."""
    f = ZERO if filt is None else filt
    return (int(f.any_of), int(f.all_of), int(f.none_of), tuple(sorted(set(int(t) for t in f.exclude))))


def allow_words(n: int) -> int:
    """64-bit words per bitmap: ceil(n / 64) rounded up to a multiple of 8 (64 bytes)."""
    return ((n + 63) // 64 + 7) // 8 * 8


# ---- tags of the base catalog (tests/test_gpu_vector.py's Data: entry e belongs to track e % 40) ------------------

BIT_HI = 63


def track_tags(tracks) -> np.ndarray:
    """Bits derived from track % k, so that every mask cuts across the scan chunks and selection slices: bit 0 even
    tracks, bit 1 track % 3 == 0, bit 2 track % 5 == 0, bit 3 track % 7 == 0, bit 63 track % 4 == 1."""
    t = np.asarray(tracks).astype(np.int64)
    out = np.zeros(len(t), U64)
    for bit, (k, r) in {0: (2, 0), 1: (3, 0), 2: (5, 0), 3: (7, 0), BIT_HI: (4, 1)}.items():
        out |= np.where(t % k == r, U64(1) << U64(bit), U64(0))
    return out


KINDS = ("any_of", "all_of", "none_of", "exclude1", "exclude8", "all", "mixed")


def case_filters(kind: str, nq: int, ntracks: int, top_track):
    """One filter per query (None = no filter) for GPU check 1. top_track[q] = the track of query q's best entry."""
    out = []
    for q in range(nq):
        m = q % 15 + 1  # a non-empty subset of bits 0..3
        hi = (1 << BIT_HI) if q % 2 else 0
        ex8 = tuple((q + 5 * j) % ntracks for j in range(MAX_EXCLUDE))
        by_kind = {
            "any_of": Filt(any_of=m | hi),
            "all_of": Filt(all_of=(m & 5) | (hi if q % 4 == 1 else 0)),
            "none_of": Filt(none_of=m | hi),
            "exclude1": Filt(exclude=(int(top_track[q]),)),
            "exclude8": Filt(exclude=ex8[::-1] if q % 2 else ex8),
            "all": Filt(any_of=m, all_of=hi, none_of=8 if not m & 8 else 0, exclude=(q % ntracks, (7 * q + 1) % ntracks)),
        }
        if kind == "mixed":
            out.append(None if q % 7 == 3 else by_kind[KINDS[q % 6]])
        else:
            out.append(by_kind[kind])
    return out


# ---- bitmap and slice edges (GPU check 3): a catalog of N_EDGE entries with its own marker bits --------------------

N_EDGE = 289  # not a multiple of 32: 10 tiles, 5 bitmap words, the last of 33 entries
EDGE_SETS = {  # marker bit -> the entries that carry it
    10: [0],
    11: [N_EDGE - 1],
    12: list(range(256, N_EDGE)),                    # the last, partial word
    13: [3, 70, 71, 200, 288],                       # exactly limit = 5
    14: [31, 32, 64, 255],                           # limit - 1 = 4
    15: [],                                          # nobody
    16: list(range(65, 91)),                         # inside one selection slice of 64, and with 32 inside [64, 96)
    17: list(range(0, N_EDGE, 6))[:26] + list(range(1, N_EDGE, 12)),  # exactly limit = 50 (asserted on the host)
    18: list(range(2, N_EDGE, 6))[:48] + [288],      # limit - 1 = 49
}


def edge_tags(tracks) -> np.ndarray:
    out = track_tags(tracks[:N_EDGE]).copy()
    for bit, es in EDGE_SETS.items():
        out[np.asarray(es, dtype=np.int64)] |= U64(1) << U64(bit)
    return out


def edge_cases(limit: int):
    """[(name, filter, passing entries wanted)] for one limit of GPU check 3."""
    cases = [("first", Filt(all_of=1 << 10), 1), ("last", Filt(any_of=1 << 11), 1),
             ("last_word", Filt(any_of=1 << 12), N_EDGE - 256), ("none", Filt(all_of=1 << 15), 0),
             ("one_slice", Filt(any_of=1 << 16), 26)]
    if limit == 5:
        cases += [("limit", Filt(any_of=1 << 13), 5), ("limit-1", Filt(any_of=1 << 14), 4)]
    if limit == 50:
        cases += [("limit", Filt(any_of=1 << 17), 50), ("limit-1", Filt(any_of=1 << 18), 49)]
    if limit == 1:
        cases += [("many", Filt(none_of=1 << 12), 256)]
    return cases


# ---- the starvation fixture (the issue's constructed catalog) ------------------------------------------------------

class Starve:
    """One tight track of 47 chunks (sigma 0.2 around its centre) stored first as track 0, then 30 tracks of 6 chunks
    (sigma 0.7, each centre plus 0.5 x the long track's centre), and one query at the long track's centre plus noise
    of sigma 0.2. A 4-minute track is 47 chunks of 10 s at a 5 s hop; the hit list has 50 slots."""

    LONG, NSHORT, PER, LIMIT = 47, 30, 6, 50

    def __init__(self, dim: int, seed: int = 21):
        rng = np.random.default_rng(seed)
        c0 = rng.standard_normal(dim)
        cat = [c0 + 0.2 * rng.standard_normal((self.LONG, dim))]
        tracks = [np.zeros(self.LONG, np.uint32)]
        for t in range(1, self.NSHORT + 1):
            ct = rng.standard_normal(dim) + 0.5 * c0
            cat.append(ct + 0.7 * rng.standard_normal((self.PER, dim)))
            tracks.append(np.full(self.PER, t, np.uint32))
        self.dim = dim
        self.cat = np.concatenate(cat).astype(F32)
        self.tracks = np.concatenate(tracks)
        n = len(self.cat)
        self.chunk = np.concatenate([np.arange(self.LONG)] + [np.arange(self.PER)] * self.NSHORT).astype(np.int32)
        self.off = self.chunk * 5.0
        self.q = (c0 + 0.2 * rng.standard_normal(dim)).astype(F32)[None, :]
        self.cn, self.qn = V.normalize(self.cat), V.normalize(self.q)
        self.S = V.scores(self.qn, self.cn)
        self.live = np.ones(n, bool)

    def rows(self, in_scan: bool, top_k=3, weight=0.05, threshold=-1.0, max_out=50):
        """(hit entries, aggregated rows) with track 0 left out after the selection (the reference) or before it."""
        mask = passes(np.zeros(len(self.cat), U64), self.tracks, self.live, Filt(exclude=(0,)) if in_scan else None)
        e = V.hit_list(self.S[0], mask, self.LIMIT)
        rows = V.aggregate(list(zip(self.tracks[e].tolist(), self.S[0][e], self.off[e].tolist())), top_k, weight,
                           None if in_scan else 0, threshold, max_out)
        return e, rows
