"""The vector lane's filtered search on the GPU (K9f, spec/FPSPEC.md 9.2) against the numpy oracles tests/vec_ref.py,
tests/vec_q8_ref.py and tests/vec_filter_ref.py: hit lists under per-query filters equal the oracle's over the passing
entries (entries, score bits and payload), on the MFMA and VALU scans, on the threshold and the slice-by-slice route,
with the int8 prefilter off and on. The number of passing entries each case relies on is asserted on the CPU in
tests/test_vec_filter_host.py."""

import ctypes
import threading
import uuid

import numpy as np
import pytest
import vec_filter_ref as R
import vec_q8_ref as Q
import vec_ref as V
from test_gpu_vector import NQ, NTRACKS, PATHS, TRIPLE, Data, N, _p, add, bits, check_hits, reset, search
from test_gpu_vector_q8 import CHUNKS, prefilter
from test_gpu_vector_q8 import stats as q8stats
from vec_filter_ref import Filt

from aidfp import _lib as L
from aidfp import vibe
from aidfp.engine import Engine
from aidfp.vibe import HIT_DTYPE, ROW_DTYPE, Filter, VectorIndex, aggregate_hits

pytestmark = pytest.mark.gpu

U64 = np.uint64
LIMITS = (1, 5, 50)
SENTINEL = 0xAB


def cfilters(filts):
    arr = (L.AidVecFilter * max(len(filts), 1))()
    for a, f in zip(arr, filts):
        if f is None:
            continue
        a.any_of, a.all_of, a.none_of, a.n_exclude = f.any_of, f.all_of, f.none_of, len(f.exclude)
        for i, t in enumerate(f.exclude):
            a.exclude[i] = t
    return arr


def fsearch_raw(eng, q, limit, filts):
    """(hits [nq][limit] prefilled with a sentinel, n_hits) of aid_vec_search_filtered; filts None = a NULL pointer."""
    q = np.ascontiguousarray(q)
    hits = np.frombuffer(bytes([SENTINEL]) * (len(q) * limit * HIT_DTYPE.itemsize), HIT_DTYPE).reshape(len(q), limit).copy()
    nh = np.full(len(q), -7, np.int32)
    flt = None if filts is None else cfilters(filts)
    L.check(eng._lib.aid_vec_search_filtered(eng._h, _p(q), len(q), L.AID_PCM_HOST, limit, flt, _p(hits), _p(nh), None))
    return hits, nh


def fsearch(eng, q, limit, filts):
    hits, nh = fsearch_raw(eng, q, limit, filts)
    return [hits[i, : nh[i]] for i in range(len(q))]


def add_tagged(eng, d, lo, hi, tags):
    L.check(eng._lib.aid_vec_add_tagged(
        eng._h, _p(np.ascontiguousarray(d.cat[lo:hi])), _p(np.ascontiguousarray(d.tracks[lo:hi])),
        _p(np.ascontiguousarray(d.chunk[lo:hi])), _p(np.ascontiguousarray(d.off[lo:hi])),
        None if tags is None else _p(np.ascontiguousarray(tags[lo:hi], dtype=U64)), hi - lo, L.AID_PCM_HOST))


def vstats(eng, reset_=True):
    out = (ctypes.c_int64 * 8)()
    L.check(eng._lib.aid_vec_stats(eng._h, out, 8, int(reset_)))
    return [int(v) for v in out]


def gpu_tags(eng, n):
    out = np.full(n, 0xFFFF, U64)
    L.check(eng._lib.aid_vec_tags(eng._h, _p(out), n))
    return out


def counts(eng):
    n_e, n_l, dim = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
    L.check(eng._lib.aid_vec_count(eng._h, ctypes.byref(n_e), ctypes.byref(n_l), ctypes.byref(dim)))
    return n_e.value, n_l.value, dim.value


def check_filtered(got, d, S, masks, limit, entry_of=None, qs=None):
    """got[i] is the oracle's list of query qs[i] over the entries masks[i] passes."""
    for i, q in enumerate(range(len(got)) if qs is None else qs):
        check_hits([got[i]], d, S, masks[i], limit, entry_of=entry_of, qs=[q])


class Cases:
    """The base catalog with its tags and, per filter kind, one filter and one passing mask per query."""

    def __init__(self, d, live=None, tags=None):
        self.d = d
        self.tags = R.track_tags(d.tracks) if tags is None else tags
        self.live = np.ones(N, bool) if live is None else live
        top = [int(d.tracks[V.hit_list(d.S[q], np.ones(N, bool), 1)[0]]) for q in range(NQ)]
        self.filters = {k: R.case_filters(k, NQ, NTRACKS, top) for k in R.KINDS}
        self.masks = {k: [R.passes(self.tags, d.tracks, self.live, f) for f in fl] for k, fl in self.filters.items()}


@pytest.fixture(scope="module")
def d512():
    d = Data(512, 11)
    d.A, d.eps = Q.Catalog(d.cn).view(d.qn)
    return d


@pytest.fixture(scope="module")
def d64():
    return Data(64, 12)


@pytest.fixture(scope="module")
def c512(d512):
    return Cases(d512)


@pytest.fixture(scope="module")
def c64(d64):
    return Cases(d64)


@pytest.fixture(scope="module")
def neardup():
    return Q.NearDup()


@pytest.fixture()
def eng(gpu_engine):
    vstats(gpu_engine)
    q8stats(gpu_engine)
    yield gpu_engine
    gpu_engine.force("vec_path", 0)
    gpu_engine.force("vec_chunk", 0)
    gpu_engine.force("vec_cand", 0)
    prefilter(gpu_engine, 0)
    L.check(gpu_engine._lib.aid_vec_reset(gpu_engine._h, 512))


# ---- 1. equality with the oracle ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,path,chunk", [(512, p, c) for p, c in PATHS] + [(64, 1, 32), (64, 2, 0)])
def test_1_filtered_hits_equal_the_oracle(eng, c512, c64, dim, path, chunk):
    """70 queries (two batches), every query its own filter (64 distinct bitmaps in the first batch for kind "all"),
    some with none, limits 1, 5 and 50."""
    c = c512 if dim == 512 else c64
    d = c.d
    eng.force("vec_path", path)
    eng.force("vec_chunk", chunk)
    reset(eng, dim)
    for lo in (0, 100, 200):  # the catalog, and with it the tags column, grows call by call
        add_tagged(eng, d, lo, lo + 100, c.tags)
    assert np.array_equal(gpu_tags(eng, N), c.tags)
    for kind in R.KINDS:
        for limit in LIMITS:
            check_filtered(fsearch(eng, d.q, limit, c.filters[kind]), d, d.S, c.masks[kind], limit)
    # one filter per batch shape: 1, 33 and 64 queries
    for nq in (1, 33, 64):
        check_filtered(fsearch(eng, d.q[:nq], 5, c.filters["all"][:nq]), d, d.S, c.masks["all"][:nq], 5)


# ---- 2. the zero filter and NULL --------------------------------------------------------------------------------------

@pytest.mark.parametrize("path,chunk", [(1, 0), (1, 32), (2, 64)])
def test_2_zero_filter_and_null_are_the_unfiltered_search(eng, c512, path, chunk):
    d = c512.d
    eng.force("vec_path", path)
    eng.force("vec_chunk", chunk)
    reset(eng, 512)
    add_tagged(eng, d, 0, N, c512.tags)
    L.check(eng._lib.aid_vec_remove(eng._h, 3))
    for limit in LIMITS:
        vstats(eng)
        plain = search(eng, d.q, limit)
        st_plain = vstats(eng)
        null_hits, null_nh = fsearch_raw(eng, d.q, limit, None)
        st_null = vstats(eng)
        zero_hits, zero_nh = fsearch_raw(eng, d.q, limit, [Filt()] * NQ)
        st_zero = vstats(eng)
        some_none = fsearch(eng, d.q, limit, [None] * NQ)
        assert st_plain == st_null == st_zero and sum(st_plain) > 0
        assert np.array_equal(null_nh, zero_nh) and null_hits.tobytes() == zero_hits.tobytes()
        for q in range(NQ):
            assert plain[q].tobytes() == null_hits[q, : null_nh[q]].tobytes() == some_none[q].tobytes()


# ---- 3. bitmap and slice edges ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("path,chunk", PATHS)
def test_3_bitmap_and_slice_edges(eng, d512, path, chunk):
    d = d512
    n = R.N_EDGE
    tags = R.edge_tags(d.tracks)
    live = np.ones(n, bool)
    eng.force("vec_path", path)
    eng.force("vec_chunk", chunk)
    reset(eng, 512)
    add_tagged(eng, d, 0, n, tags)
    S = d.S[:, :n]
    for limit in LIMITS:
        cases = R.edge_cases(limit)
        filts = [cases[q % len(cases)][1] for q in range(NQ)]
        masks = [R.passes(tags, d.tracks[:n], live, f) for f in filts]
        vstats(eng)
        hits, nh = fsearch_raw(eng, d.q, limit, filts)
        st = vstats(eng)
        check_filtered([hits[q, : nh[q]] for q in range(NQ)], d, S, masks, limit)
        for q in range(NQ):
            name, _, want = cases[q % len(cases)]
            assert nh[q] == min(limit, want), (limit, name)
            # what lies past a list, and the whole row of an empty one, is untouched
            assert (hits[q, nh[q]:].view(np.uint8) == SENTINEL).all(), (limit, name)
        # the routes, two batches each: by threshold while there are at least `limit` slices (289 entries are 10
        # slices of 32, 5 of 64, 1 of 1024), where "one_slice" and "first" leave fewer non-empty slices than limit and
        # the threshold is the empty slices' 0; slice by slice above that
        n_slices = -(-n // (chunk or 1024))
        if n_slices >= limit:
            assert (st[0], st[1], st[2], st[3]) == (2, 0, 0, 0), (limit, st)
        else:
            assert (st[0], st[1], st[2]) == (0, 2, 0) and st[3] >= 2, (limit, st)
    if chunk == 32:
        assert -(-n // 32) >= 5 > 1  # limit 5 went by threshold and limit 50 slice by slice, both under filters


# ---- 4. ties ----------------------------------------------------------------------------------------------------------

def test_4_ties_keep_entry_order_among_the_passing_entries(eng, c512):
    d = c512.d
    t_first, t_mid = int(d.tracks[TRIPLE[0]]), int(d.tracks[TRIPLE[1]])
    assert len({t_first, t_mid, int(d.tracks[TRIPLE[2]])}) == 3
    for path, chunk in PATHS:
        eng.force("vec_path", path)
        eng.force("vec_chunk", chunk)
        reset(eng, 512)
        add_tagged(eng, d, 0, N, c512.tags)
        q = d.q[2:3]
        for limit in (2, 50):
            assert list(fsearch(eng, q, limit, [Filt(exclude=(t_mid,))])[0]["entry"][:2]) == [TRIPLE[0], TRIPLE[2]]
            assert list(fsearch(eng, q, limit, [Filt(exclude=(t_first,))])[0]["entry"][:2]) == [TRIPLE[1], TRIPLE[2]]
        assert list(fsearch(eng, q, 1, [Filt(exclude=(t_first, t_mid))])[0]["entry"]) == [TRIPLE[2]]


@pytest.mark.parametrize("chunk,limit", [(0, 3), (32, 50), (32, 1024)])
def test_4_more_passing_ties_than_the_candidate_list_holds(eng, chunk, limit):
    """9000 copies of one vector, every second one tagged: 4500 passing entries tie, the threshold route's candidate
    list (4096) overflows under the filter and the slice-by-slice route answers with the first passing entries."""
    n, dim = 9000, 32
    rng = np.random.default_rng(5)
    v = rng.standard_normal((1, dim)).astype(np.float32)
    q = rng.standard_normal((2, dim)).astype(np.float32)
    s = V.scores(V.normalize(q), V.normalize(v))[:, 0]
    eng.force("vec_chunk", chunk)
    reset(eng, dim)
    cat = np.ascontiguousarray(np.repeat(v, n, axis=0))
    tracks = (np.arange(n) // 2).astype(np.uint32)
    tags = (np.arange(n) % 2).astype(U64) << U64(40)
    L.check(eng._lib.aid_vec_add_tagged(eng._h, _p(cat), _p(tracks), None, _p(np.zeros(n)), _p(tags), n, L.AID_PCM_HOST))
    L.check(eng._lib.aid_vec_remove(eng._h, 0))  # entries 0 and 1
    want = np.arange(3, 3 + 2 * limit, 2)
    vstats(eng)
    got = fsearch(eng, q, limit, [Filt(any_of=1 << 40), Filt(all_of=1 << 40, exclude=(0,))])
    st = vstats(eng)
    assert (st[0], st[1], st[2]) == ((0, 1, 0) if limit == 1024 else (0, 0, 1)) and st[4] == (0 if limit == 1024 else 4499)
    for qi, g in enumerate(got):
        assert np.array_equal(g["entry"], want)
        assert np.array_equal(bits(g["score"]), np.full(limit, bits(s[qi : qi + 1])[0]))
        assert np.array_equal(g["track"], tracks[want]) and np.array_equal(g["chunk_index"], want)


# ---- 5. life cycle ----------------------------------------------------------------------------------------------------

def test_5_life_cycle(eng, c512, tmp_path):
    d = c512.d
    reset(eng, 512)
    add_tagged(eng, d, 0, N, c512.tags)
    filts = c512.filters["mixed"]

    def masks_of(tags, live):
        return [R.passes(tags, d.tracks, live, f) for f in filts]

    # remove a track, then filter
    gone = int(d.tracks[V.hit_list(d.S[0], c512.masks["mixed"][0], 1)[0]])
    L.check(eng._lib.aid_vec_remove(eng._h, gone))
    live = d.tracks != gone
    for limit in LIMITS:
        got = fsearch(eng, d.q, limit, filts)
        check_filtered(got, d, d.S, masks_of(c512.tags, live), limit)
        assert not any((g["track"] == gone).any() for g in got)
    # retag changes the results of the next call
    t2 = (gone + 1) % NTRACKS
    before = fsearch(eng, d.q, 50, [Filt(any_of=1 << 20)] * NQ)
    assert all(len(b) == 0 for b in before)
    L.check(eng._lib.aid_vec_retag(eng._h, t2, ctypes.c_uint64((1 << 20) | (1 << 63))))
    assert eng._lib.aid_vec_retag(eng._h, gone, ctypes.c_uint64(1)) == L.AID_ERR_INVALID   # no live entry
    assert eng._lib.aid_vec_retag(eng._h, 12345, ctypes.c_uint64(1)) == L.AID_ERR_INVALID  # unknown
    tags = c512.tags.copy()
    tags[d.tracks == t2] = (1 << 20) | (1 << 63)
    assert np.array_equal(gpu_tags(eng, N), tags)
    after = fsearch(eng, d.q, 50, [Filt(any_of=1 << 20)] * NQ)
    m20 = R.passes(tags, d.tracks, live, Filt(any_of=1 << 20))
    assert int(m20.sum()) == int((d.tracks == t2).sum()) > 0
    check_filtered(after, d, d.S, [m20] * NQ, 50)
    check_filtered(fsearch(eng, d.q, 5, filts), d, d.S, masks_of(tags, live), 5)

    # save with tags (version 2: the tags column after the tombstones), then compact: tags follow their rows
    path = tmp_path / "tagged.vec"
    L.check(eng._lib.aid_vec_save(eng._h, str(path).encode()))
    raw = path.read_bytes()
    nf = ((N + 31) // 32) * 32 * 512
    assert raw[:8] == b"AIDFPVC1" and np.frombuffer(raw[8:12], "<u4")[0] == 2 and len(raw) == 24 + nf * 4 + 25 * N
    assert np.array_equal(np.frombuffer(raw[24 + nf * 4 + 17 * N:], "<u8"), tags)
    assert np.array_equal(np.frombuffer(raw[24 + nf * 4 + 16 * N: 24 + nf * 4 + 17 * N], np.uint8), (~live).astype(np.uint8))
    n_rm = ctypes.c_int64()
    L.check(eng._lib.aid_vec_compact(eng._h, ctypes.byref(n_rm)))
    assert n_rm.value == N - int(live.sum())
    assert np.array_equal(gpu_tags(eng, int(live.sum())), tags[live])
    entry_of = np.cumsum(live) - 1
    for limit in (5, 50):
        check_filtered(fsearch(eng, d.q, limit, filts), d, d.S, masks_of(tags, live), limit, entry_of=entry_of)

    # the file loads into a fresh engine: the same tags and results; a file cut inside the tags column is refused
    e2 = Engine(44100)
    try:
        # before any tagged call on this engine: what an untagged catalog saves
        L.check(e2._lib.aid_vec_reset(e2._h, 512))
        add(e2, d, 0, N)
        L.check(e2._lib.aid_vec_remove(e2._h, gone))
        plain = tmp_path / "plain.vec"
        L.check(e2._lib.aid_vec_save(e2._h, str(plain).encode()))
        L.check(e2._lib.aid_vec_reset(e2._h, 64))
        L.check(e2._lib.aid_vec_load(e2._h, str(path).encode()))
        assert counts(e2) == (N, int(live.sum()), 512)
        assert np.array_equal(gpu_tags(e2, N), tags)
        check_filtered(fsearch(e2, d.q, 50, filts), d, d.S, masks_of(tags, live), 50)
        cut = tmp_path / "cut.vec"
        cut.write_bytes(raw[:-100])
        short = tmp_path / "short.vec"
        short.write_bytes(raw[: 24 + nf * 4 + 17 * N])  # a version-2 header over a version-1 body
        L.check(e2._lib.aid_vec_retag(e2._h, t2, ctypes.c_uint64(5)))
        tags2 = tags.copy()
        tags2[d.tracks == t2] = 5
        for bad in (cut, short):
            assert e2._lib.aid_vec_load(e2._h, str(bad).encode()) == L.AID_ERR_INVALID
            assert counts(e2) == (N, int(live.sum()), 512) and np.array_equal(gpu_tags(e2, N), tags2)
        check_filtered(fsearch(e2, d.q[:8], 50, filts[:8]), d, d.S, masks_of(tags2, live)[:8], 50)
        # a version-1 file gives tags 0
        L.check(e2._lib.aid_vec_load(e2._h, str(plain).encode()))
        assert not gpu_tags(e2, N).any()
        assert all(len(g) == 0 for g in fsearch(e2, d.q[:3], 5, [Filt(any_of=1)] * 3))
    finally:
        e2.close()

    # an untagged catalog on an engine that has run tagged and filtered calls saves that file byte for byte: added
    # with a NULL column, with zeros, and with tags that a retag has cleared again
    plain_bytes = plain.read_bytes()
    assert np.frombuffer(plain_bytes[8:12], "<u4")[0] == 1 and len(plain_bytes) == 24 + nf * 4 + 17 * N
    for how in ("null", "zeros", "cleared"):
        reset(eng, 512)
        if how == "cleared":
            add_tagged(eng, d, 0, N, c512.tags)
            fsearch(eng, d.q[:2], 5, [Filt(any_of=1)] * 2)
            for t in range(NTRACKS):
                L.check(eng._lib.aid_vec_retag(eng._h, t, ctypes.c_uint64(0)))
        else:
            add_tagged(eng, d, 0, N, None if how == "null" else np.zeros(N, U64))
        L.check(eng._lib.aid_vec_remove(eng._h, gone))
        again = tmp_path / f"again_{how}.vec"
        L.check(eng._lib.aid_vec_save(eng._h, str(again).encode()))
        assert again.read_bytes() == plain_bytes, how


# ---- 6. prefilter on --------------------------------------------------------------------------------------------------

def route_stats(A, eps, S, masks, limit, over=4, cap=Q.CAND_CAP, qs=None):
    r = [Q.route(A[q], eps[q], S[q], masks[i], limit, over, cap=cap) for i, q in enumerate(range(len(masks)) if qs is None else qs)]
    w = [len(x["W"]) for x in r]
    fb = sum(bool(x["fallback"]) for x in r)
    return dict(answered=len(r) - fb, fell_back=fb, w_total=sum(w), w_max=max(w))


def q8_of(st):
    return {k: st[k] for k in ("answered", "fell_back", "w_total", "w_max")}


@pytest.mark.parametrize("chunk", CHUNKS)
def test_6_prefilter_on_gives_the_same_hits_and_the_oracles_routes(eng, c512, chunk):
    c, d = c512, c512.d
    eng.force("vec_chunk", chunk)
    reset(eng, 512)
    add_tagged(eng, d, 0, N, c.tags)
    off = {(k, limit): fsearch(eng, d.q, limit, c.filters[k]) for k in R.KINDS for limit in LIMITS}
    prefilter(eng, 1, 4)
    for kind in R.KINDS:
        for limit in LIMITS:
            q8stats(eng)
            got = fsearch(eng, d.q, limit, c.filters[kind])
            st = q8stats(eng)
            check_filtered(got, d, d.S, c.masks[kind], limit)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, off[(kind, limit)]))
            assert q8_of(st) == route_stats(d.A, d.eps, d.S, c.masks[kind], limit), (kind, limit)
            assert st["fell_back"] == 0
    # check 3's catalog: 289 entries, E over its own rows
    n = R.N_EDGE
    tags = R.edge_tags(d.tracks)
    A, eps = Q.Catalog(d.cn[:n]).view(d.qn)
    for limit in LIMITS:
        cases = R.edge_cases(limit)
        filts = [cases[q % len(cases)][1] for q in range(NQ)]
        masks = [R.passes(tags, d.tracks[:n], np.ones(n, bool), f) for f in filts]
        prefilter(eng, 0)
        reset(eng, 512)
        add_tagged(eng, d, 0, n, tags)
        hits_off, nh_off = fsearch_raw(eng, d.q, limit, filts)
        prefilter(eng, 1, 4)
        q8stats(eng)
        hits_on, nh_on = fsearch_raw(eng, d.q, limit, filts)
        st = q8stats(eng)
        assert np.array_equal(nh_on, nh_off) and hits_on.tobytes() == hits_off.tobytes()
        check_filtered([hits_on[q, : nh_on[q]] for q in range(NQ)], d, d.S[:, :n], masks, limit)
        assert q8_of(st) == route_stats(A, eps, d.S[:, :n], masks, limit), limit


def test_6_filtered_queries_fall_back_inside_a_batch(eng, neardup):
    d = neardup
    tags = R.track_tags(d.tracks)
    live = np.ones(N, bool)
    qs = list(np.arange(NQ) % 10)
    qq = np.ascontiguousarray(d.q[qs])
    top = [int(d.tracks[V.hit_list(d.S[q], live, 1)[0]]) for q in qs]
    for kind in ("any_of", "mixed"):
        filts = R.case_filters(kind, NQ, NTRACKS, top)
        masks = [R.passes(tags, d.tracks, live, f) for f in filts]
        for chunk in CHUNKS:
            eng.force("vec_chunk", chunk)
            prefilter(eng, 0)
            reset(eng, d.dim)
            add_tagged(eng, d, 0, N, tags)
            prefilter(eng, 1, 4)
            eng.force("vec_cand", 64)
            for limit in (1, 5):
                q8stats(eng)
                got = fsearch(eng, qq, limit, filts)
                st = q8stats(eng)
                check_filtered(got, d, d.S, masks, limit, qs=qs)
                want = route_stats(d.A, d.eps, d.S, masks, limit, cap=64, qs=qs)
                assert q8_of(st) == want and want["fell_back"] > 5 and want["answered"] > 5, (kind, limit, want)
            eng.force("vec_cand", 0)


# ---- 7. lane ----------------------------------------------------------------------------------------------------------

def lane_filtered(eng, q, limit, top_k, weight, filts, excl, thr, max_out):
    q = np.ascontiguousarray(q)
    rows = np.zeros((len(q), max_out), ROW_DTYPE)
    nr = np.zeros(len(q), np.int32)
    ex = None if excl is None else np.ascontiguousarray(excl, dtype=np.uint32)
    L.check(eng._lib.aid_vibe_lane_filtered(eng._h, _p(q), len(q), L.AID_PCM_HOST, limit, top_k, weight,
                                            None if filts is None else cfilters(filts), None if ex is None else _p(ex),
                                            thr, max_out, _p(rows), _p(nr), None))
    return [rows[i, : nr[i]] for i in range(len(q))]


@pytest.mark.parametrize("path,chunk,pre", [(1, 64, 0), (2, 0, 0), (1, 32, 1)])
def test_7_lane_equals_search_then_aggregate_and_the_oracle(eng, c512, path, chunk, pre):
    c, d = c512, c512.d
    eng.force("vec_path", path)
    eng.force("vec_chunk", chunk)
    reset(eng, 512)
    prefilter(eng, pre)
    add_tagged(eng, d, 0, N, c.tags)
    live = np.ones(N, bool)
    top1 = [int(V.hit_list(d.S[q], live, 1)[0]) for q in range(NQ)]
    excl = [int(d.tracks[top1[q]]) if q % 2 else vibe.VEC_NO_TRACK for q in range(NQ)]  # post hoc, beside the filter
    seen = 0
    for kind in ("mixed", "all"):
        filts, masks = c.filters[kind], c.masks[kind]
        for limit, top_k, weight, thr, max_out in [(50, 3, 0.05, 0.60, 5), (50, 1, 0.3, 0.2, 50), (5, 10, 0.0, -1.0, 3)]:
            lane = lane_filtered(eng, d.q, limit, top_k, weight, filts, excl, thr, max_out)
            two = aggregate_hits(eng, fsearch(eng, d.q, limit, filts), top_k, weight, exclude=excl, threshold=thr,
                                 max_out=max_out)
            for q in range(NQ):
                e = V.hit_list(d.S[q], masks[q], limit)
                want = V.aggregate(list(zip(d.tracks[e].tolist(), d.S[q][e], d.off[e].tolist())), top_k, weight,
                                   None if excl[q] == vibe.VEC_NO_TRACK else excl[q], thr, max_out)
                assert [tuple(r) for r in lane[q].tolist()] == want, (kind, q)
                assert [tuple(r) for r in two[q].tolist()] == want, (kind, q)
                seen += len(want)
    assert seen > NQ
    # filters NULL: aid_vibe_lane itself
    ix = VectorIndex.__new__(VectorIndex)
    ix.eng, ix.dim = eng, 512
    a = lane_filtered(eng, d.q, 50, 3, 0.05, None, excl, -1.0, 10)  # no threshold: ten rows a query
    b = ix.vibe_raw(d.q, 10, excl, -1.0, 3, 0.05, 50)
    assert sum(map(len, a)) > NQ and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("dim", [64, 512])
def test_7_exclude_in_scan_fills_the_slots_the_excluded_track_took(eng, dim):
    s = R.Starve(dim)
    ids = [uuid.UUID(int=(t + 1) * 0x1234567) for t in range(s.NSHORT + 1)]
    ix = VectorIndex(eng, dim)
    for t in range(s.NSHORT + 1):  # stored track by track, in the fixture's entry order
        e = np.flatnonzero(s.tracks == t)
        ix.upsert_track(ids[t], s.cat[e], s.off[e], s.chunk[e])

    def as_results(rows):
        return [vibe.TrackResult(ids[r[0]], r[2], r[3], r[4], r[1]) for r in rows]

    thr = -1.0  # every row shows
    _, rows_post = s.rows(in_scan=False, threshold=thr, max_out=50)
    _, rows_scan = s.rows(in_scan=True, threshold=thr, max_out=50)
    post = ix.vibe(s.q, 50, exact_match_track_ids=[ids[0]], threshold=thr)
    today = ix.vibe_raw(s.q, 50, [0], thr)  # aid_vibe_lane with its post-hoc exclusion
    scan = ix.vibe(s.q, 50, exact_match_track_ids=[ids[0]], threshold=thr, exclude_in_scan=True)
    assert post == [as_results(rows_post)] and [tuple(r) for r in today[0].tolist()] == rows_post
    assert scan == [as_results(rows_scan)]
    assert len(post[0]) <= 3 and len(scan[0]) >= 15
    assert all(r.track_id != ids[0] for r in post[0] + scan[0])
    assert sum(r.chunk_count for r in scan[0]) == 50 and sum(r.chunk_count for r in post[0]) == 3
    # a query without an exact match keeps every track, either way
    assert ix.vibe(s.q, 50, exact_match_track_ids=[None], threshold=thr, exclude_in_scan=True) == \
        ix.vibe(s.q, 50, threshold=thr)


# ---- 8. bad arguments and the adapter -----------------------------------------------------------------------------------

def test_8_bad_arguments(eng, c512):
    d = c512.d
    reset(eng, 512)
    add_tagged(eng, d, 0, 64, c512.tags)
    h = eng._h
    q = np.ascontiguousarray(d.q[:2])
    hits, nh = np.zeros((2, 5), HIT_DTYPE), np.full(2, -7, np.int32)
    bad = cfilters([Filt(), Filt()])
    bad[1].n_exclude = 9
    assert eng._lib.aid_vec_search_filtered(h, _p(q), 2, L.AID_PCM_HOST, 5, bad, _p(hits), _p(nh), None) == L.AID_ERR_INVALID
    assert "more than 8" in L.last_error() and list(nh) == [-7, -7]
    ok = cfilters([Filt(any_of=1), Filt()])
    assert eng._lib.aid_vec_search_filtered(h, _p(q), 2, L.AID_PCM_HOST, 5, ok, None, _p(nh), None) == L.AID_ERR_INVALID
    assert eng._lib.aid_vec_search_filtered(h, _p(q), 2, L.AID_PCM_HOST, 5, ok, _p(hits), None, None) == L.AID_ERR_INVALID
    assert eng._lib.aid_vec_search_filtered(h, _p(q), 2, L.AID_PCM_HOST, 0, ok, _p(hits), _p(nh), None) == L.AID_ERR_INVALID
    rows, nr = np.zeros((2, 5), ROW_DTYPE), np.zeros(2, np.int32)
    assert eng._lib.aid_vibe_lane_filtered(h, _p(q), 2, L.AID_PCM_HOST, 5, 3, 0.05, bad, None, 0.2, 5, _p(rows), _p(nr),
                                           None) == L.AID_ERR_INVALID
    assert eng._lib.aid_vibe_lane_filtered(h, _p(q), 2, L.AID_PCM_HOST, 5, 3, 0.05, ok, None, 0.2, 5, None, _p(nr),
                                           None) == L.AID_ERR_INVALID
    assert eng._lib.aid_vec_search_filtered(h, _p(q), 0, L.AID_PCM_HOST, 5, ok, None, None, None) == L.AID_OK
    assert eng._lib.aid_vec_retag(h, 999, ctypes.c_uint64(1)) == L.AID_ERR_INVALID
    out = np.zeros(64, U64)
    assert eng._lib.aid_vec_tags(h, _p(out), 63) == L.AID_ERR_INVALID
    assert eng._lib.aid_vec_tags(h, None, 64) == L.AID_ERR_INVALID
    L.check(eng._lib.aid_vec_tags(h, _p(out), 64))
    assert np.array_equal(out, c512.tags[:64])
    # an excluded id that no entry carries is not an error, and an empty catalog answers with empty lists
    got = fsearch(eng, q, 5, [Filt(exclude=(4_000_000,)), Filt(exclude=(4_000_000, 7))])
    assert len(got[0]) == 5 and not (got[1]["track"] == 7).any()
    reset(eng, 512)
    assert all(len(g) == 0 for g in fsearch(eng, q, 5, [Filt(any_of=1), Filt()]))


def test_8_adapter_names_masks_registry_and_threads(eng, c512, tmp_path):
    d = c512.d
    ids = [uuid.UUID(int=(t + 1) * 0x1234567) for t in range(NTRACKS)]
    ix = VectorIndex(eng, 512)
    names = {0: "even", 1: "rock", 2: "live", 3: "seven"}
    for bit, name in names.items():
        assert ix.tag_bit(name) == 1 << bit
    assert ix.tag_bit("rock") == 2  # registered once
    perm = np.concatenate([np.flatnonzero(d.tracks == t) for t in range(NTRACKS)])  # the adapter stores track by track
    for t in range(NTRACKS):
        e = np.flatnonzero(d.tracks == t)
        tg = int(c512.tags[e[0]])
        mine = [names[b] for b in names if tg >> b & 1] + ([1 << R.BIT_HI] if tg >> R.BIT_HI & 1 else [])  # names and a mask
        assert ix.upsert_track(ids[t], d.cat[e], d.off[e], d.chunk[e], tags=mine) == len(e)
    S, tr, ch, off, tags = d.S[:, perm], d.tracks[perm], d.chunk[perm], d.off[perm], c512.tags[perm]
    assert np.array_equal(gpu_tags(eng, N), tags)
    live = np.ones(N, bool)

    def want_hits(q, f, limit=50):
        e = V.hit_list(S[q], R.passes(tags, tr, live, f), limit)
        return [vibe.ChunkHit(ids[tr[i]], float(S[q][i]), int(ch[i]), float(off[i])) for i in e]

    # one Filter for all queries; names, masks and both; caller ids, one of them never stored
    shared = Filter(any_of=("rock", "live"), none_of=1 << R.BIT_HI, exclude_tracks=(ids[3], uuid.uuid4()))
    f_shared = Filt(any_of=0b110, none_of=1 << R.BIT_HI, exclude=(3,))
    assert ix.search(d.q[:9], 50, filters=shared) == [want_hits(q, f_shared) for q in range(9)]
    per_q = [Filter(all_of="even"), None, Filter(any_of=0b1001), Filter(none_of=["seven", 1])]
    f_per_q = [Filt(all_of=1), None, Filt(any_of=0b1001), Filt(none_of=0b1001)]
    assert ix.search(d.q[:4], 5, filters=per_q) == [want_hits(q, f, 5) for q, f in enumerate(f_per_q)]
    assert ix.search(d.q[:4], 5, filters=None) == ix.search(d.q[:4], 5) == [want_hits(q, None, 5) for q in range(4)]
    with pytest.raises(KeyError):
        ix.search(d.q[:1], 5, filters=Filter(any_of="jazz"))
    with pytest.raises(ValueError):
        ix.search(d.q[:2], 5, filters=[shared])
    with pytest.raises(ValueError):
        ix.search(d.q[:1], 5, filters=Filter(exclude_tracks=tuple(ids[:9])))
    # set_tags
    assert ix.set_tags(ids[5], ["rock", "gold"]) and not ix.set_tags(uuid.uuid4(), "rock")
    tags = tags.copy()
    tags[tr == 5] = 2 | ix.tag_bit("gold")
    assert ix.tag_bit("gold") == 1 << 4 and np.array_equal(gpu_tags(eng, N), tags)
    assert ix.search(d.q[:3], 50, filters=Filter(all_of="gold")) == [want_hits(q, Filt(all_of=1 << 4)) for q in range(3)]

    # the registry is saved beside the ids and loaded with them
    ix.save(tmp_path / "ix.vec")
    assert (tmp_path / "ix.vec.tags").read_text().split("\n") == ["even", "rock", "live", "seven", "gold"]
    ix2 = VectorIndex(eng, 512)
    assert len(ix2) == 0
    ix2.load(tmp_path / "ix.vec")
    assert ix2.tag_bit("gold") == 1 << 4 and ix2.tag_bit("new") == 1 << 5
    assert ix2.search(d.q[:3], 50, filters=Filter(all_of="gold")) == [want_hits(q, Filt(all_of=1 << 4)) for q in range(3)]
    (tmp_path / "ix.vec.tags").unlink()  # a missing file: an empty registry
    ix3 = VectorIndex(eng, 512)
    ix3.load(tmp_path / "ix.vec")
    assert ix3.tag_bit("anything") == 1 and len(ix3) == N
    for k in range(1, 64):
        assert ix3.tag_bit(f"t{k}") == 1 << k
    with pytest.raises(ValueError):
        ix3.tag_bit("the 65th")
    assert ix3.tag_bit("t63") == 1 << 63

    # four threads search with different filters while one upserts tracks that none of the filters lets through: the
    # tags column grows under the searches (past the first 1024 rows), and every answer is the oracle's
    ix = ix2
    thread_filters = [Filter(any_of="rock", none_of="new"), Filter(all_of="even", none_of="new"),
                      Filter(none_of=("new", "seven")), Filter(none_of="new", exclude_tracks=(ids[1], ids[2]))]
    thread_filts = [Filt(any_of=2, none_of=32), Filt(all_of=1, none_of=32), Filt(none_of=32 | 8), Filt(none_of=32, exclude=(1, 2))]
    want = [[want_hits(q, f) for q in range(NQ)] for f in thread_filts]
    rng = np.random.default_rng(8)
    extra = rng.standard_normal((25, 32, 512)).astype(np.float32) + d.cat[:25, None, :]  # near stored tracks
    results, errors = {}, []

    def searcher(k):
        try:
            results[k] = [ix.search(d.q, 50, filters=thread_filters[k]) for _ in range(4)]
        except Exception as exc:  # noqa: BLE001
            errors.append(exc)

    def upserter():
        try:
            for j in range(25):
                ix.upsert_track(uuid.UUID(int=0xABC000 + j), extra[j], np.arange(32) * 5.0, tags=("new", "rock", "even"))
        except Exception as exc:  # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=searcher, args=(k,)) for k in range(4)] + [threading.Thread(target=upserter)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    assert ix.counts() == (N + 25 * 32, N + 25 * 32)
    assert all(r == want[k] for k in range(4) for r in results[k])
    # and after the growth the new tracks are there for a filter that asks for them
    got = ix.search(d.q[:1], 50, filters=Filter(all_of="new"))[0]
    assert len(got) == 50 and {h.track_id for h in got} <= {uuid.UUID(int=0xABC000 + j) for j in range(25)}
