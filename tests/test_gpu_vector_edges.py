"""Vector lane (K9, csrc/vector.hip) at the sizes the product runs, on the constructed catalogs and hit lists of
tests/vec_fixtures.py (whose claims tests/test_vec_fixtures_host.py proves on the oracle): the default scan chunk with
several workgroups and four tiles a wave, catalog growth with a partial last tile, both selection routes on distinct
scores with the route read from aid_vec_stats, dead slices, negative and zero keys, dims 32 / 96 / 1024, and hit lists
of 1,024 in the aggregation. Everything is compared with tests/vec_ref.py bit for bit; the expected counters come from
vec_fixtures.expect_stats (the constants of csrc/aidfp_vector.h and the oracle's scores), never from a run."""

import ctypes

import numpy as np
import pytest
import vec_fixtures as F
import vec_ref as V

from aidfp import _lib as L
from aidfp import vibe
from aidfp.vibe import HIT_DTYPE, VectorIndex, aggregate_hits

pytestmark = pytest.mark.gpu

ZERO = dict.fromkeys(F.STAT_NAMES, 0)


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.fixture()
def eng(gpu_engine):
    gpu_engine.force("vec_path", 0)
    gpu_engine.force("vec_chunk", 0)
    yield gpu_engine
    gpu_engine.force("vec_path", 0)
    gpu_engine.force("vec_chunk", 0)
    L.check(gpu_engine._lib.aid_vec_reset(gpu_engine._h, 512))


def reset(eng, dim):
    L.check(eng._lib.aid_vec_reset(eng._h, dim))


def add(eng, d, lo=0, hi=None, tracks=None):
    hi = d.n if hi is None else hi
    tr = d.tracks if tracks is None else tracks
    L.check(eng._lib.aid_vec_add(eng._h, _p(np.ascontiguousarray(d.cat[lo:hi])), _p(np.ascontiguousarray(tr[lo:hi])),
                                 _p(np.ascontiguousarray(d.chunk[lo:hi])), _p(np.ascontiguousarray(d.off[lo:hi])),
                                 hi - lo, L.AID_PCM_HOST))


def load(eng, d, tracks=None):
    reset(eng, d.dim)
    add(eng, d, tracks=tracks)


def gpu_scores(eng, q, n):
    q = np.ascontiguousarray(q)
    out = np.full((len(q), n), np.nan, np.float32)
    L.check(eng._lib.aid_vec_scores(eng._h, _p(q), len(q), L.AID_PCM_HOST, _p(out), out.size))
    return out


def search(eng, q, limit):
    q = np.ascontiguousarray(q)
    hits = np.zeros((len(q), limit), HIT_DTYPE)
    nh = np.zeros(len(q), np.int32)
    L.check(eng._lib.aid_vec_search(eng._h, _p(q), len(q), L.AID_PCM_HOST, limit, _p(hits), _p(nh), None))
    return [hits[i, : nh[i]] for i in range(len(q))]


def counted_search(eng, q, limit):
    """The hit lists, and aid_vec_stats counted over this search alone."""
    eng.vec_stats(reset=True)
    got = search(eng, q, limit)
    return got, eng.vec_stats()


def check_hits(got, d, S, live, limit, tracks=None, entry_of=None):
    """got[q] equals the oracle's list: entries, score bits and payload. entry_of: oracle entry -> engine entry."""
    tr = d.tracks if tracks is None else tracks
    assert len(got) == len(S)
    for q, g in enumerate(got):
        want = V.hit_list(S[q], live, limit)
        assert len(g) == len(want) == min(limit, int(live.sum())), (limit, q)
        assert np.array_equal(g["entry"], want if entry_of is None else entry_of[want]), (limit, q)
        assert np.array_equal(bits(g["score"]), bits(S[q][want])), (limit, q)
        assert np.array_equal(g["track"], tr[want]) and np.array_equal(g["chunk_index"], d.chunk[want]), (limit, q)
        assert np.array_equal(g["offset_sec"], d.off[want]), (limit, q)


def check_search(eng, d, S, live, limit, chunk=0, path=0, q=None, **kw):
    """One search: the oracle's lists, and the route and launches vec_search_dev's dispatch implies for them."""
    got, st = counted_search(eng, d.q if q is None else q, limit)
    check_hits(got, d, S, live, limit, **kw)
    assert st == F.expect_stats(S, live, limit, chunk, path), limit
    return st


def stored_rows(eng, tmp_path, n, dim):
    """The catalog's tiles as saved, back in [n][dim]."""
    path = tmp_path / "cat.vec"
    L.check(eng._lib.aid_vec_save(eng._h, str(path).encode()))
    raw = path.read_bytes()
    nf = ((n + 31) // 32) * 32 * dim
    assert len(raw) == 24 + nf * 4 + 17 * n
    return V.detile(np.frombuffer(raw[24 : 24 + nf * 4], "<f4"), n, dim)


# ---- (a) default geometry and growth ----
@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("dim", [64, 512])
def test_growth_and_scores_at_the_default_chunk(eng, tmp_path, dim, path):
    """5,165 entries in calls of 1000, 1100 and 3065: six scan workgroups, four tiles a wave, a last tile of 13 rows;
    the catalog is copied twice with a partial last tile. Scores after every call, stored tiles after the last."""
    d = F.default_geometry(dim)
    eng.force("vec_path", path)
    L.check(eng._lib.aid_vec_reset(eng._h, 32))  # another dim first: the block of the test before is dropped
    reset(eng, dim)
    eng.vec_stats(reset=True)
    n = 0
    for m in F.ADD_CALLS_A:
        add(eng, d, n, n + m)
        n += m
        assert np.array_equal(bits(gpu_scores(eng, d.q, n)), bits(d.S[:, :n])), n
    want = dict(ZERO, grow_copies=2, **{"scans_valu" if path == 2 else "scans_mfma": 3})
    assert eng.vec_stats() == want
    if path == 1:
        assert np.array_equal(bits(stored_rows(eng, tmp_path, d.n, dim)), bits(d.cn))


# ---- (b) routes on (a) ----
@pytest.mark.parametrize("dim", [64, 512])
def test_both_routes_on_distinct_scores(eng, dim):
    """Limits 1 and 6 go by threshold (six slices: 6 is msl == limit; three filter blocks), 7, 50 and 1024 slice by
    slice in two passes (at 1024 the second sorts 2,048 keys)."""
    d = F.default_geometry(dim)
    load(eng, d)
    live = np.ones(d.n, bool)
    seen = {}
    for limit in (1, 6, 7, 50, 1024):
        seen[limit] = check_search(eng, d, d.S, live, limit)
    assert [seen[k]["batches_threshold"] for k in (1, 6, 7, 50, 1024)] == [1, 1, 0, 0, 0]
    assert [seen[k]["slice_selects"] for k in (1, 6, 7, 50, 1024)] == [0, 0, 2, 2, 2]
    eng.force("vec_path", 2)
    check_search(eng, d, d.S, live, 6, path=2)


# ---- (c) planted ties inside the cap ----
def test_ties_inside_the_candidate_cap(eng):
    """700 copies of the query: the threshold route collects 700 candidates at limit 1 and 780 at limit 6 (several
    rounds of the sort), does not overflow, and lists the copies in entry order."""
    d = F.planted_ties()
    load(eng, d)
    live = np.ones(d.n, bool)
    for limit in (1, 6, 50):
        st = check_search(eng, d, d.S, live, limit)
        assert st["batches_overflow"] == 0
    assert check_search(eng, d, d.S, live, 6)["max_candidates"] == int(F.dispatch(d.S, live, 6)[0]["counts"].max()) > 700
    got = search(eng, d.q[:1], 50)[0]
    assert np.array_equal(got["entry"], d.info["copies"][:50]) and len(set(bits(got["score"]))) == 1


# ---- (d) overflow under a strict top ----
def test_overflow_with_an_order_above_the_tie(eng):
    """4,200 tied copies under ten distinct better entries: limit 1 goes by threshold, limits 6 and 50 overflow or are
    not eligible, and the slice route lists the ten in score order, then the copies in entry order."""
    d = F.overflow_under_strict_top()
    load(eng, d)
    live = np.ones(d.n, bool)
    assert check_search(eng, d, d.S, live, 1)["batches_threshold"] == 1
    st = check_search(eng, d, d.S, live, 6)
    assert (st["batches_overflow"], st["slice_selects"]) == (1, 2) and st["max_candidates"] > F.CAND_CAP
    check_search(eng, d, d.S, live, 50)
    got = search(eng, d.q, 50)[0]
    assert set(got["entry"][:10]) == set(d.info["top"]) and np.array_equal(got["entry"][10:], d.info["copies"][:40])
    assert (np.diff(got["score"][:11]) < 0).all()


# ---- (e) dead slices and short lists ----
def test_dead_slices_short_lists_and_compaction(eng):
    d = F.default_geometry(64)
    tr = F.tracks_e()
    load(eng, d, tracks=tr)
    for t in (1, 2, 3, 4):
        L.check(eng._lib.aid_vec_remove(eng._h, t))
    live = ~np.isin(tr, [1, 2, 3, 4])  # slices 0 and 5 whole, one survivor in 1 and in 3, none in 2 and 4
    for limit in (1, 3, 6, 7, 50):
        check_search(eng, d, d.S, live, limit, tracks=tr)
    assert check_search(eng, d, d.S, live, 6, tracks=tr)["max_candidates"] == 1071  # threshold 0: every live entry
    for t in (0, 5):
        L.check(eng._lib.aid_vec_remove(eng._h, t))
    live = np.zeros(d.n, bool)
    live[list(F.SURVIVORS_E)] = True
    for limit in (1, 3, 6, 7, 50):
        st = check_search(eng, d, d.S, live, limit, tracks=tr)
        assert (st["batches_threshold"] == 1) == (limit <= 6)
    assert [len(g) for g in search(eng, d.q[:2], 6)] == [4, 4]
    # compaction: the four survivors are entries 0 .. 3 of a one-slice catalog
    n_rm = ctypes.c_int64()
    L.check(eng._lib.aid_vec_compact(eng._h, ctypes.byref(n_rm)))
    assert n_rm.value == d.n - 4
    entry_of = np.cumsum(live) - 1
    for limit in (1, 3, 6, 7, 50):
        got, st = counted_search(eng, d.q, limit)
        check_hits(got, d, d.S, live, limit, tracks=tr, entry_of=entry_of)
        assert st == F.expect_stats(d.S[:, live], np.ones(4, bool), limit), limit
    # and the catalog still grows after it
    more = np.random.default_rng(9).standard_normal((100, 64)).astype(np.float32)
    z = np.zeros(100)
    L.check(eng._lib.aid_vec_add(eng._h, _p(more), _p(np.full(100, 500, np.uint32)), None, _p(z), 100, L.AID_PCM_HOST))
    S2 = np.concatenate([d.S[:, live], d.extended(more)], axis=1)
    assert np.array_equal(bits(gpu_scores(eng, d.q, 104)), bits(S2))


def test_short_list_on_the_threshold_route_forced_chunk(eng):
    """300 entries in ten slices of 32 with six live entries: limit 10 goes by a threshold of 0 and returns six."""
    d = F.short_list_small()
    eng.force("vec_chunk", 32)
    load(eng, d)
    L.check(eng._lib.aid_vec_remove(eng._h, 0))
    live = d.tracks != 0
    st = check_search(eng, d, d.S, live, 10, chunk=32)
    assert (st["batches_threshold"], st["max_candidates"]) == (1, 6)
    assert [len(g) for g in search(eng, d.q, 10)] == [6, 6, 6]


# ---- (f) signs ----
@pytest.mark.parametrize("chunk,limits", [(0, (1, 5)), (32, (1, 5, 10, 50))])
def test_negative_and_zero_scores(eng, chunk, limits):
    """Query 0 scores negative everywhere (keys below 0x80000000 through slice maxima, threshold and filter); queries
    1 and 2 normalise to +0, so every score is +0 and the hits are the first live entries with score bits 0."""
    d = F.signs()
    eng.force("vec_chunk", chunk)
    load(eng, d)
    live = np.ones(d.n, bool)
    assert np.array_equal(bits(gpu_scores(eng, d.q, d.n)), bits(d.S))
    for limit in limits:
        check_search(eng, d, d.S, live, limit, chunk=chunk)
        got = search(eng, d.q, limit)
        assert (got[0]["score"] < 0).all() and (np.diff(got[0]["score"]) <= 0).all()
        for q in (1, 2):
            assert np.array_equal(got[q]["entry"], np.arange(limit)) and not bits(got[q]["score"]).any()
    L.check(eng._lib.aid_vec_remove(eng._h, 0))  # entries 0, 40, 80, ...: the zero rows start at entry 1
    live = d.tracks != 0
    for limit in limits:
        check_search(eng, d, d.S, live, limit, chunk=chunk)
    assert list(search(eng, d.q[1:2], 5)[0]["entry"]) == [1, 2, 3, 4, 5]


def test_zero_queries_overflow_at_the_default_sizes(eng):
    """All 5,165 scores are +0: the candidate list overflows and the slice route still lists entries 0 .. limit - 1."""
    d = F.default_geometry(64)
    load(eng, d)
    zq = F.zero_queries(64)
    Sz = V.scores(V.normalize(zq), d.cn)
    live = np.ones(d.n, bool)
    st = check_search(eng, d, Sz, live, 6, q=zq)
    assert (st["batches_overflow"], st["max_candidates"], st["slice_selects"]) == (1, d.n, 2)
    for g in search(eng, zq, 6):
        assert np.array_equal(g["entry"], np.arange(6)) and not bits(g["score"]).any()


# ---- (g) dims ----
@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("dim", F.DIMS_G)
def test_dims_32_96_1024(eng, tmp_path, dim, path):
    """One stage, an odd number of stages, and the query tile that needs 128 KB of LDS (MFMA path at 1024); 70
    entries (a last tile of 6 rows) and 33 queries (a second query tile of one row)."""
    d = F.small_dim(dim)
    eng.force("vec_path", path)
    load(eng, d)
    eng.vec_stats(reset=True)
    assert np.array_equal(bits(gpu_scores(eng, d.q, d.n)), bits(d.S))
    assert eng.vec_stats() == dict(ZERO, **{"scans_valu" if path == 2 else "scans_mfma": 1})
    assert np.array_equal(bits(stored_rows(eng, tmp_path, d.n, dim)), bits(d.cn))
    live = np.ones(d.n, bool)
    for limit in (1, 5, 70):
        check_search(eng, d, d.S, live, limit, path=path)


# ---- (h) aggregation on long lists ----
def hit_array(lst):
    t, s, o = lst
    h = np.zeros(len(t), HIT_DTYPE)
    h["entry"], h["track"], h["score"], h["offset_sec"] = np.arange(len(t)), t, s, o
    return h


@pytest.mark.parametrize("case", F.agg_cases(), ids=lambda c: c[0])
def test_aggregate_long_lists(eng, case):
    """Lists of 1,024 hits: 200 tracks (four rounds of 64 groups), 1,024 tracks, one track; equal finals in lane 5 of
    four rounds with max_out cutting the tie and a tied track excluded; a threshold on and just above a final;
    4, 5 and 6 distinct offsets; 0.0 and -0.0. Several lists per call, empty ones between them."""
    _, names, top_k, weight, exclude, threshold, max_out = case
    lists = F.agg_lists()
    excl = [vibe.VEC_NO_TRACK if e is None else e for e in exclude]
    got = aggregate_hits(eng, [hit_array(lists[n]) for n in names], top_k, weight, exclude=excl,
                         threshold=-np.inf if threshold is None else threshold, max_out=max_out)
    rows = 0
    for g, name, e in zip(got, names, exclude):
        want = F.agg_rows(name, top_k, weight, e, threshold, max_out)
        assert [tuple(r) for r in g.tolist()] == want, name
        rows += len(want)
    assert rows > 0


def test_lane_at_limit_1024_on_the_default_geometry(eng):
    """aid_vibe_lane at limit 1024 over 5,165 entries of 230 tracks against search-then-aggregate and the oracle."""
    d = F.default_geometry(64)
    ix = VectorIndex(eng, 64)  # its raw calls (engine ids), on a catalog loaded through the C ABI
    add(eng, d)
    live = np.ones(d.n, bool)
    nq = len(d.q)
    hl = [V.hit_list(d.S[q], live, 1024) for q in range(nq)]
    excl = [int(d.tracks[hl[q][0]]) if q % 2 else vibe.VEC_NO_TRACK for q in range(nq)]
    seen_rows = 0
    for top_k, weight, thr, max_out in [(3, 0.05, -1.0, 256), (10, 0.0, 0.12, 10)]:
        lane = ix.vibe_raw(d.q, max_out, excl, thr, top_k, weight, 1024)
        two = aggregate_hits(eng, search(eng, d.q, 1024), top_k, weight, exclude=excl, threshold=thr, max_out=max_out)
        for q in range(nq):
            e = hl[q]
            want = V.aggregate(list(zip(d.tracks[e].tolist(), d.S[q][e], d.off[e].tolist())), top_k, weight,
                               None if excl[q] == vibe.VEC_NO_TRACK else excl[q], thr, max_out)
            assert [tuple(r) for r in lane[q].tolist()] == want, q
            assert [tuple(r) for r in two[q].tolist()] == want, q
            seen_rows += len(want)
    assert seen_rows > 192 * nq  # the first setting lists nearly every track of more than three rounds of groups
