"""Constructed catalogs, queries and hit lists for the K9 vector-lane tests (csrc/vector.hip), at the sizes the
product runs: the default scan chunk and slice sizes, every kind of dim, hit lists of 1,024.

Plain numpy, no GPU. A `Cat` is a catalog with its queries, its payload columns and the oracle's results
(tests/vec_ref.py); `dispatch` and `expect_stats` restate the host dispatch of `vec_search_dev` from the constants of
csrc/aidfp_vector.h and the oracle's score matrix, so a test knows which route answers and what aid_vec_stats must
count before anything runs. test_vec_fixtures_host.py checks every claim made here on the oracle alone;
test_gpu_vector_edges.py compares the engine with the oracle, bit for bit.

The geometry (csrc/vector.hip): a scan workgroup of 8 waves takes kVecScanChunk / 32 tiles of 32 rows, wave w the
tiles w, w + 8, ...; the threshold route cuts the entries into slices of kVecMaxSlice, the slice-by-slice route into
slices of kVecSelectSlice; k_vec_filter's block covers 2,048 entries; k_vec_select sorts 256 keys per round of its
threads; k_vec_aggregate is one wave over at most kVecMaxLimit hits."""

from __future__ import annotations

import functools
import re
from pathlib import Path

import numpy as np
import vec_ref as V

F32 = np.float32
_HEADER = Path(__file__).resolve().parents[1] / "audio-ident_amd" / "csrc" / "aidfp_vector.h"
K = {k: int(v) for k, v in re.findall(r"constexpr int (kVec\w+) = (\d+);", _HEADER.read_text())}
MAX_LIMIT, QUERY_BATCH, SCAN_CHUNK = K["kVecMaxLimit"], K["kVecQueryBatch"], K["kVecScanChunk"]
MAX_SLICE, CAND_CAP, SELECT_SLICE = K["kVecMaxSlice"], K["kVecCandCap"], K["kVecSelectSlice"]
FILTER_BLOCK = 2048  # entries per k_vec_filter workgroup (8 per thread)
SORT_ROUND = 256     # keys per round of vec_sort_desc's 256 threads
STAT_NAMES = ("batches_threshold", "batches_ineligible", "batches_overflow", "slice_selects", "max_candidates",
              "grow_copies", "scans_mfma", "scans_valu")

N_A = 5 * 1024 + 45          # (a): 162 tiles, 6 scan workgroups (the last of 2 tiles), 6 threshold slices, 2 select slices
ADD_CALLS_A = (1000, 1100, 3065)  # capacity 1024 -> 3072 -> 6144: two copies, both at an n that is no multiple of 32
N_TRACKS_A = 230


def pow2_ceil(v: int) -> int:
    p = 1
    while p < v:
        p <<= 1
    return p


def score_key(s) -> np.ndarray:
    """vec_score_key: a score's bits mapped so that unsigned order is numeric order (-0 counts as +0)."""
    b = np.ascontiguousarray(s, dtype=F32).view(np.uint32).copy()
    b[b == 0x80000000] = 0
    return np.where(b & 0x80000000, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


# ---- the host dispatch of vec_search_dev, restated ----
def geometry(n: int, limit: int, chunk: int = 0) -> dict:
    """Slice sizes, slice counts and the slice-by-slice pass count of a search over n entries (chunk =
    AID_FORCE_VEC_CHUNK, 0 = the defaults)."""
    sl = max(chunk or SELECT_SLICE, 2 * pow2_ceil(limit))
    keep = min(limit, sl)
    passes, n_in, first_slices, last_sort = 0, n, None, 0
    while True:
        nsl = -(-n_in // sl)
        first_slices = nsl if first_slices is None else first_slices
        passes += 1
        last_sort = n_in
        n_in = nsl * keep
        if nsl == 1:
            break
    mslice = chunk or max(MAX_SLICE, pow2_ceil(-(-n // CAND_CAP)))
    msl = -(-n // mslice)
    tiles = -(-n // 32)
    return {"slice": sl, "keep": keep, "passes": passes, "first_slices": first_slices, "last_sort": last_sort,
            "mslice": mslice, "msl": msl, "eligible": limit <= msl <= CAND_CAP, "scan_tiles": tiles,
            "scan_wgs": -(-tiles // max(1, (chunk or SCAN_CHUNK) // 32)), "filter_blocks": -(-n // FILTER_BLOCK)}


def threshold_counts(S: np.ndarray, live: np.ndarray, limit: int, mslice: int):
    """Per query: (the limit-th largest slice maximum as a key, 0 where fewer slices have a live entry; the number
    of live entries at or above it) -- what k_vec_slice_max, k_vec_threshold and k_vec_filter compute."""
    n = S.shape[1]
    keys = np.where(live[None, :], score_key(S).reshape(S.shape), np.uint32(0))
    msl = -(-n // mslice)
    pad = np.zeros((S.shape[0], msl * mslice), np.uint32)
    pad[:, :n] = keys
    smax = pad.reshape(S.shape[0], msl, mslice).max(axis=2)
    thr = -np.sort(-smax.astype(np.int64), axis=1)[:, limit - 1]
    cnt = ((keys.astype(np.int64) >= thr[:, None]) & live[None, :]).sum(axis=1)
    return thr.astype(np.uint32), cnt


def dispatch(S: np.ndarray, live: np.ndarray, limit: int, chunk: int = 0) -> list:
    """One dict per query batch of a search: route ("threshold", "ineligible" or "overflow"), the candidate counts
    and the k_vec_select launches of the slice-by-slice route."""
    g = geometry(S.shape[1], limit, chunk)
    out = []
    for q0 in range(0, S.shape[0], QUERY_BATCH):
        if not g["eligible"]:
            out.append({"route": "ineligible", "counts": None, "selects": g["passes"]})
            continue
        _, cnt = threshold_counts(S[q0 : q0 + QUERY_BATCH], live, limit, g["mslice"])
        over = int(cnt.max()) > CAND_CAP
        out.append({"route": "overflow" if over else "threshold", "counts": cnt, "selects": g["passes"] if over else 0})
    return out


def expect_stats(S: np.ndarray, live: np.ndarray, limit: int, chunk: int = 0, path: int = 0) -> dict:
    """aid_vec_stats after one search of S's queries over a non-empty catalog, counted from zero."""
    st = dict.fromkeys(STAT_NAMES, 0)
    for b in dispatch(S, live, limit, chunk):
        st["batches_" + b["route"]] += 1
        st["slice_selects"] += b["selects"]
        if b["counts"] is not None:
            st["max_candidates"] = max(st["max_candidates"], int(b["counts"].max()))
        st["scans_valu" if path == 2 else "scans_mfma"] += 1
    return st


def add_stats(a: dict, b: dict) -> dict:
    """Counters of two searches in a row: sums, but the candidate count is a maximum."""
    return {k: max(a[k], b[k]) if k == "max_candidates" else a[k] + b[k] for k in STAT_NAMES}


# ---- catalogs ----
class Cat:
    """cat [n][dim] and q [nq][dim] raw float32; tracks / chunk / off the payload columns; cn, qn, S the oracle's
    normalised vectors and score matrix; info = what the builder claims."""

    def __init__(self, cat, q, tracks=None, info=None):
        self.cat = np.ascontiguousarray(cat, dtype=F32)
        self.q = np.ascontiguousarray(q, dtype=F32)
        self.n, self.dim = self.cat.shape
        self.tracks = (np.arange(self.n) % N_TRACKS_A if tracks is None else np.asarray(tracks)).astype(np.uint32)
        self.chunk = (np.arange(self.n) // 7 % 100).astype(np.int32)
        self.off = (np.arange(self.n) // N_TRACKS_A % 7) * 2.5  # a track's chunks share offsets from the eighth on
        self.info = info or {}
        self.cn, self.qn = V.normalize(self.cat), V.normalize(self.q)
        self.S = V.scores(self.qn, self.cn)

    def extended(self, more: np.ndarray) -> np.ndarray:
        """The oracle's scores of the queries against further raw entries."""
        return V.scores(self.qn, V.normalize(more))


SURVIVORS_E = (7, 2000, 3500, 5160)  # (e): entries with a track of their own, in slices 0, 1, 3 and 5


def tracks_e(n: int = N_A) -> np.ndarray:
    """(e): track = threshold slice of the entry, except the survivors (tracks 100 ..)."""
    t = (np.arange(n) // MAX_SLICE).astype(np.uint32)
    t[list(SURVIVORS_E)] = 100 + np.arange(len(SURVIVORS_E))
    return t


@functools.lru_cache(maxsize=None)
def default_geometry(dim: int) -> Cat:
    """(a): N_A distinct random entries; 33 queries (two query tiles, the second of one row) at dim 64, 5 at 512."""
    rng = np.random.default_rng(100 + dim)
    nq = 33 if dim <= 64 else 5
    return Cat(rng.standard_normal((N_A, dim)), rng.standard_normal((nq, dim)))


@functools.lru_cache(maxsize=None)
def planted_ties() -> Cat:
    """(c): one vector w at entries 3 + 7 i, i < 700 (slices 0 to 4; slice 5 has none); query 0 = w, query 1 random.
    Every copy ties at the top of query 0, inside the candidate cap."""
    rng = np.random.default_rng(21)
    cat = rng.standard_normal((N_A, 64)).astype(F32)
    w = rng.standard_normal(64).astype(F32)
    copies = 3 + 7 * np.arange(700)
    cat[copies] = w
    q = np.stack([w, rng.standard_normal(64).astype(F32)])
    return Cat(cat, q, info={"copies": copies})


@functools.lru_cache(maxsize=None)
def overflow_under_strict_top() -> Cat:
    """(d): 4,200 copies of w = u + 0.5 noise on entries not divisible by 6 (all in slices 0 to 4), ten entries
    u + 0.1 noise_i at 0, 6, ..., 54 above them, query u: the candidate list overflows under a strict top ten."""
    rng = np.random.default_rng(22)
    cat = rng.standard_normal((N_A, 64)).astype(F32)
    u = rng.standard_normal(64)
    w = (u + 0.5 * rng.standard_normal(64)).astype(F32)
    copies = np.flatnonzero(np.arange(5 * MAX_SLICE) % 6 != 0)[:4200]
    top = 6 * np.arange(10)
    cat[copies] = w
    cat[top] = (u[None, :] + 0.1 * rng.standard_normal((10, 64))).astype(F32)
    return Cat(cat, u[None, :], info={"copies": copies, "top": top})


@functools.lru_cache(maxsize=None)
def short_list_small() -> Cat:
    """(e)'s cheap twin: 300 entries of track 0 except six survivors; with track 0 removed and chunk 32 the ten
    slices hold six live entries, and limit 10 goes by a threshold of 0."""
    rng = np.random.default_rng(23)
    tracks = np.zeros(300, np.uint32)
    keep = np.array([0, 31, 32, 170, 171, 299])
    tracks[keep] = 1 + np.arange(6)
    return Cat(rng.standard_normal((300, 64)), rng.standard_normal((3, 64)), tracks=tracks, info={"keep": keep})


@functools.lru_cache(maxsize=None)
def signs() -> Cat:
    """(f): 300 entries c0 + 0.3 noise. Query 0 = -c0 (every score negative), query 1 all zero and query 2 with one
    inf component (both normalise to +0: every score +0), query 3 = c0 (an ordinary row in the same batch)."""
    rng = np.random.default_rng(24)
    c0 = rng.standard_normal(64)
    cat = c0[None, :] + 0.3 * rng.standard_normal((300, 64))
    q = np.stack([-c0, np.zeros(64), c0, c0]).astype(F32)
    q[2, 17] = np.inf
    return Cat(cat, q, tracks=np.arange(300) % 40)


def zero_queries(dim: int) -> np.ndarray:
    """An all-zero query and one with an inf component."""
    q = np.zeros((2, dim), F32)
    q[1] = 1.0
    q[1, dim // 2] = np.inf
    return q


DIMS_G = (32, 96, 1024)  # one stage (the wrap on every step), an odd stage count, the 128 KB LDS launch


@functools.lru_cache(maxsize=None)
def small_dim(dim: int) -> Cat:
    """(g): 70 entries (three tiles, the last of 6 rows), 33 queries, clustered so that tracks collect hits."""
    rng = np.random.default_rng(300 + dim)
    cent = rng.standard_normal((10, dim))
    tracks = np.arange(70) % 10
    cat = cent[tracks] + 0.7 * rng.standard_normal((70, dim))
    q = cent[rng.integers(0, 10, size=33)] + 0.7 * rng.standard_normal((33, dim))
    return Cat(cat, q, tracks=tracks)


# ---- hit lists for k_vec_aggregate: (track uint32, score float32 descending, offset float64) ----
def _scores_desc(rng, n: int, lo: float = 0.2, hi: float = 0.95) -> np.ndarray:
    return np.sort(rng.uniform(lo, hi, size=n).astype(F32))[::-1].copy()


TIE_GROUPS = (5, 69, 133, 197)  # lane 5 of the four rounds of `for (g = lane; g < ng; g += 64)`
TIE_TRACKS = tuple(g * 3 + 11 for g in TIE_GROUPS)


def hits_of(lst):
    """A list's hits as the oracle takes them."""
    t, s, o = lst
    return list(zip(t.tolist(), s, o.tolist()))


@functools.lru_cache(maxsize=None)
def agg_lists() -> dict:
    rng = np.random.default_rng(31)
    n = MAX_LIMIT
    offs = lambda m: rng.integers(0, 9, size=m) * 2.5  # noqa: E731
    out = {"empty": (np.zeros(0, np.uint32), np.zeros(0, F32), np.zeros(0))}
    # 1,024 hits over 200 tracks (four rounds of 64 groups, the last of 8)
    out["tracks200"] = ((rng.integers(0, 200, size=n) * 7 + 3).astype(np.uint32), _scores_desc(rng, n), offs(n))
    # 1,024 hits, 1,024 tracks: every hit leads a group
    out["tracks1024"] = (rng.permutation(n).astype(np.uint32) + 5000, _scores_desc(rng, n), offs(n))
    # 1,024 hits of one track
    out["one_track"] = (np.full(n, 77, np.uint32), _scores_desc(rng, n), offs(n))
    # equal finals in groups 5, 69, 133 and 197 (lane 5 of four rounds): hits 5 .. 197 open groups 5 .. 197 at one
    # score s; every group but those four gets a second, lower hit, so its mean of two is below s (weight 0)
    s = F32(0.75)
    first = np.concatenate([np.linspace(0.95, 0.9, 5).astype(F32), np.full(193, s, F32)])
    again = np.array([g for g in range(198) if g not in TIE_GROUPS], np.uint32)
    second = _scores_desc(rng, len(again), 0.2, 0.7)
    tr = np.concatenate([np.arange(198, dtype=np.uint32), rng.permutation(again)]) * 3 + 11
    out["tie4"] = (tr.astype(np.uint32), np.concatenate([first, second]), np.zeros(len(tr)))
    # tracks with exactly 4, 5 and 6 distinct offsets (7 hits each, in turn), and a track whose offsets 0.0 and -0.0
    # are one offset: two distinct among its three
    tr = np.concatenate([np.tile([1, 2, 3], 7), [4, 4, 4]]).astype(np.uint32)
    of = np.concatenate([np.array([[i % 4, i % 5, i % 6] for i in range(7)], float).ravel() * 5.0, [0.0, -0.0, 5.0]])
    out["offsets"] = (tr, _scores_desc(rng, len(tr)), of)
    return out


def agg_rows(name: str, top_k: int, weight: float, exclude=None, threshold=None, max_out=None):
    return V.aggregate(hits_of(agg_lists()[name]), top_k, weight, exclude, threshold, max_out)


def agg_cases() -> list:
    """Calls of aid_vec_aggregate: (id, list names, top_k, weight, per-list exclude or None, threshold, max_out).
    Several lists per call, empty ones between them."""
    every = ("tracks200", "empty", "tracks1024", "empty", "empty", "one_track", "offsets", "tie4", "empty")
    none = (None,) * len(every)
    rows = agg_rows("tracks200", 3, 0.05)
    at = rows[len(rows) // 2][2]  # a final score in the middle of the list
    tie_from = [r[0] for r in agg_rows("tie4", 3, 0.0)].index(TIE_TRACKS[0])
    return [
        ("all_1024", every, 3, 0.05, none, None, MAX_LIMIT),
        ("all_10", every, 3, 0.05, none, None, 10),
        ("top_k_1", every, 1, 0.05, none, None, MAX_LIMIT),
        ("top_k_2000", every, 2000, 0.3, none, None, MAX_LIMIT),
        ("tie_whole", ("tie4", "empty", "tie4"), 3, 0.0, (None, None, TIE_TRACKS[1]), None, MAX_LIMIT),
        ("tie_cut", ("tie4", "empty", "tie4"), 3, 0.0, (None, None, TIE_TRACKS[1]), None, tie_from + 2),
        ("threshold_kept", ("tracks200", "empty", "tracks1024"), 3, 0.05, (None,) * 3, at, MAX_LIMIT),
        ("threshold_dropped", ("tracks200", "empty", "tracks1024"), 3, 0.05, (None,) * 3, float(np.nextafter(at, np.inf)),
         MAX_LIMIT),
    ]
