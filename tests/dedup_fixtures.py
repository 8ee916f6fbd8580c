"""Constructed catalogs and queries for the K7 dedup tests (csrc/dedup.hip: `dedup_scan`, `dedup_pairs`): each builder
places what the golden fixture (60 entries, one chunk, no tie in any band) never meets -- a tie inside a wave, across
waves, across 64-entry chunks, a best score one bit ahead of its runner-up, a duration exactly on a band bound, a
catalog that scores nothing -- where random fingerprints only meet them by chance.

Plain numpy, no GPU. A case is a `Case`: catalog entries and queries as lists of uint32 arrays with float64 durations,
plus what the builder claims about it (`tied`, `better`, `edge` ...). test_dedup_fixtures_host.py checks every claim
through the CPU oracle (oracle/fp_dedup.c); test_gpu_dedup_edges.py compares the GPU with that oracle, bit for bit.

The scan's geometry (csrc/dedup.hip): one workgroup per (query, chunk of 64 entries), entry e of a chunk scored by
wave e % 4, lanes striding the words by 64."""

from dataclasses import dataclass, field

import numpy as np

U32 = np.uint32
CHUNK = 64  # kDedupChunk
WAVES = 4  # waves of a k_dedup_scan workgroup

CATALOG_SIZES = (1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 257)
QUERY_COUNTS = (1, 2, 65, 300)
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 1000)
LONG = 30000  # about an hour of Chromaprint


@dataclass
class Case:
    cat: list
    cat_dur: np.ndarray
    queries: list
    q_dur: np.ndarray
    info: dict = field(default_factory=dict)


def words(rng, n: int) -> np.ndarray:
    return rng.integers(0, 1 << 32, size=int(n), dtype=np.uint64).astype(U32)


def flip(a: np.ndarray, bits) -> np.ndarray:
    """A copy of `a` with the given bit numbers (0 .. 32 * len(a) - 1, distinct) inverted."""
    out = a.copy()
    bits = np.asarray(bits, dtype=np.int64)
    assert len(np.unique(bits)) == len(bits) and (len(bits) == 0 or (bits.min() >= 0 and bits.max() < 32 * len(a)))
    np.bitwise_xor.at(out, bits >> 5, (U32(1) << (bits & 31).astype(U32)))
    return out


def popcount_diff(a: np.ndarray, b: np.ndarray) -> int:
    n = min(len(a), len(b))
    return int(np.unpackbits((a[:n] ^ b[:n]).view(np.uint8)).sum())


# ---- catalog sizes x query counts: random words, every entry inside every query's band ----
_POOL = {}


def _pool():
    """257 entries and 300 queries drawn once: a smaller case takes a prefix of each. Entry lengths 100..600; every
    second query is a noisy copy of some entry (winners spread over every chunk and wave), the others are random."""
    if not _POOL:
        rng = np.random.default_rng(7001)
        n_cat, nq = max(CATALOG_SIZES), max(QUERY_COUNTS)
        cat = [words(rng, rng.integers(100, 601)) for _ in range(n_cat)]
        cat_dur = rng.uniform(97.0, 103.0, n_cat)
        queries = []
        for i in range(nq):
            if i % 2:
                src = cat[(i * 37) % n_cat]
                q = flip(src, rng.choice(32 * len(src), size=int(rng.integers(1, 200)), replace=False))
                cut = int(rng.integers(-40, 41))
                q = q[:cut] if cut < 0 else np.concatenate([q, words(rng, cut)])
            else:
                q = words(rng, rng.integers(100, 601))
            queries.append(q)
        q_dur = rng.uniform(99.0, 101.0, nq)  # bands hold [90.9, 108.9] at the least
        _POOL.update(cat=cat, cat_dur=cat_dur, queries=queries, q_dur=q_dur)
    return _POOL


def sized(n_cat: int, nq: int) -> Case:
    p = _pool()
    return Case(p["cat"][:n_cat], p["cat_dur"][:n_cat].copy(), p["queries"][:nq], p["q_dur"][:nq].copy(),
                {"n_cat": n_cat, "nq": nq})


# ---- fingerprint lengths ----
def length_pairs():
    """[(query, entry)] for every (la, lb) of LENGTHS x LENGTHS plus one LONG x LONG pair: both are prefixes of one
    random base with a few bits inverted, so the score is high and every word counts."""
    rng = np.random.default_rng(7002)
    base = words(rng, LONG)
    lens = [(la, lb) for la in LENGTHS for lb in LENGTHS] + [(LONG, LONG)]
    out = []
    for la, lb in lens:
        a = flip(base[:la], rng.choice(32 * la, size=min(la, 5), replace=False)) if la else base[:0].copy()
        b = flip(base[:lb], rng.choice(32 * lb, size=min(lb, 3), replace=False)) if lb else base[:0].copy()
        out.append((a, b))
    return out


def length_scan() -> Case:
    """The pairs of length_pairs() as one scan: entry j of pair j has a duration of its own (1.5 apart by ratio), and
    query j has exactly that duration, so entry j is the only one in query j's band: best_idx is j, or -1 at 0.0."""
    pairs = length_pairs()
    dur = 1e-3 * 1.25 ** np.arange(len(pairs), dtype=np.float64)  # a band spans 0.9 .. 1.1: neighbours stay outside
    return Case([b for _, b in pairs], dur, [a for a, _ in pairs], dur.copy(), {"pairs": len(pairs)})


# ---- ties and near ties ----
# name -> (positions of the copies, position that lies outside the band or None)
PLACEMENTS = {
    "same_wave": ((2, 6), None),  # e, e + 4: both wave 2 of chunk 0
    "same_wave_chunk2": ((129, 133), None),
    "next_wave": ((1, 2), None),  # the later one in a higher wave
    "wrapped_wave": ((3, 4), None),  # e + 3, e + 4: the later one in wave 0
    "wrapped_wave_chunk1": ((67, 68), None),
    "chunk_edge": ((63, 64), None),
    "far_chunks": ((5, 133), None),  # 5 and 64 * 2 + 5: the same wave of two chunks
    "three_chunks": ((10, 74, 168), None),
    "five_first_out_of_band": ((3, 20, 70, 71, 140), 3),
}
TIE_N_CAT = 200
_TIE_LEN = 300
_TIE_FLIPS = 40  # the copies differ from the query in 40 of 9600 bits: far above the random entries' 0.5


def tie_case(name: str, kind: str = "tie") -> Case:
    """kind "tie": every copy scores the same bits. "later": the last copy is one bit closer to the query than the
    others. "earlier": the first in-band copy is one bit closer."""
    pos, out_of_band = PLACEMENTS[name]
    rng = np.random.default_rng([7003, sorted(PLACEMENTS).index(name)])
    q = words(rng, _TIE_LEN)
    cat = [words(rng, _TIE_LEN) for _ in range(TIE_N_CAT)]
    cat_dur = rng.uniform(97.0, 103.0, TIE_N_CAT)
    bits = rng.choice(32 * _TIE_LEN, size=_TIE_FLIPS, replace=False)
    in_band = [p for p in pos if p != out_of_band]
    better = {"tie": None, "later": in_band[-1], "earlier": in_band[0]}[kind]
    for p in pos:
        cat[p] = flip(q, bits[1:] if p == better else bits)
    if out_of_band is not None:
        cat_dur[out_of_band] = 150.0
    return Case(cat, cat_dur, [q], np.array([100.0]),
                {"copies": pos, "in_band": in_band, "better": better, "kind": kind, "flips": _TIE_FLIPS})


# ---- nothing scores above 0.0 ----
def zero_case(name: str) -> Case:
    """"complement": every in-band entry is the query's complement (any length) or empty, the out-of-band ones are
    the query itself. "empty_query": a query of no words against an ordinary catalog. "all_out_of_band": copies of
    the query, none within its band."""
    rng = np.random.default_rng([7004, ("complement", "empty_query", "all_out_of_band").index(name)])
    n_cat = 150
    q = words(rng, 260)
    if name == "complement":
        cat, dur = [], []
        for e in range(n_cat):
            if e % 5 == 4:
                cat.append(q.copy())
                dur.append(200.0 if e % 2 else 50.0)
            elif e % 5 == 3:
                cat.append(q[:0].copy())
                dur.append(100.0)
            else:
                n = (260, 100, 400)[e % 3]
                cat.append(np.concatenate([~q, words(rng, 140)])[:n])
                dur.append(float(rng.uniform(91.0, 109.0)))
        return Case(cat, np.array(dur), [q], np.array([100.0]), {"name": name})
    if name == "empty_query":
        s = sized(130, 1)
        return Case(s.cat, s.cat_dur, [q[:0].copy()], np.array([100.0]), {"name": name})
    cat = [flip(q, [e]) for e in range(n_cat)]
    dur = np.where(np.arange(n_cat) % 2 == 0, 89.9, 110.1)
    return Case(cat, dur, [q], np.array([100.0]), {"name": name})


# ---- duration band edges ----
BAND_QUERIES = (100.0, 123.456, 59.29, 1000.0 / 3.0, 7.0, 0.1, 2.5e-5, 86399.99)


def band_case(q_dur: float, edge: str) -> Case:
    """edge "lo" / "hi": entry 1 lies exactly on float(q * 0.9) / float(q * 1.1), entry 0 one binary64 step outside it
    and entry 3 one step outside the other bound; both outside entries are the query itself (score 1.0), entry 1 a
    noisy copy, entry 2 a random mid-band entry. The expected winner is entry 1. edge "nan": the query's duration is
    NaN and nothing matches."""
    rng = np.random.default_rng([7005, int(q_dur * 1000) % 100003, ("lo", "hi", "nan").index(edge)])
    q = words(rng, 200)
    qd = np.float64(q_dur)
    lo, hi = qd * np.float64(0.9), qd * np.float64(1.1)
    below, above = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
    on, out, other = (lo, below, above) if edge != "hi" else (hi, above, below)
    cat = [q.copy(), flip(q, rng.choice(6400, size=100, replace=False)), words(rng, 200), q.copy()]
    cat_dur = np.array([out, on, qd, other], dtype=np.float64)
    return Case(cat, cat_dur, [q], np.array([np.nan if edge == "nan" else qd]),
                {"edge": edge, "lo": lo, "hi": hi, "on": on, "out": out})


# ---- catalog life cycle ----
ADD_SIZES = (1, 63, 64, 1, 200, 2, 65, 3)


def lifecycle_case() -> Case:
    """sum(ADD_SIZES) entries and 300 queries. Empty entries stand at the first and last place of several adds, and
    three adds hold empty entries only (they move no words but must still rebase their offsets). The entries
    that the noisy-copy queries were made from are spread over all the adds."""
    p = _pool()
    rng = np.random.default_rng(7006)
    n = sum(ADD_SIZES)
    cat = [words(rng, rng.integers(100, 601)) for _ in range(n)]
    for i, e in enumerate(rng.permutation(n)[:len(p["cat"])]):
        cat[e] = p["cat"][i].copy()
    ends = np.cumsum(ADD_SIZES)
    for e in (0, 1, 63, 64, 127, 128, 129, 328, 329, 330, n - 1):  # adds 0, 3 and 5 whole, edges of the others, the last
        cat[e] = cat[e][:0]
    cat_dur = rng.uniform(97.0, 103.0, n)
    return Case(cat, cat_dur, p["queries"], p["q_dur"].copy(), {"adds": ADD_SIZES, "ends": ends.tolist()})
