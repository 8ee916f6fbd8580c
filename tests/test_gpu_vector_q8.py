"""The vector lane's int8 prefilter on the GPU (K9q, spec/FPSPEC.md 9.1) against the numpy oracles tests/vec_ref.py
and tests/vec_q8_ref.py: approx and eps bit for bit (which is also the check of the int8 MFMA's lane map and of the
kernels' addressing), and hit lists, rows and routes equal to FPSPEC 9's with the prefilter on. The fixtures'
preconditions are checked on the CPU in tests/test_vec_q8_host.py."""

import ctypes
import threading
import uuid

import numpy as np
import pytest
import vec_q8_ref as Q
import vec_ref as V
from test_gpu_vector import Data, _p, add, bits, check_hits, reset, search

from aidfp import _lib as L
from aidfp import vibe
from aidfp.engine import Engine
from aidfp.vibe import VectorIndex

pytestmark = pytest.mark.gpu

N, NQ = Q.N, 70
CHUNKS = [0, 64, 32]  # AID_FORCE_VEC_CHUNK: 1, 5 and 10 scan workgroups, the last of 44 or 12 rows
STAT_NAMES = VectorIndex.PREFILTER_STATS


def prefilter(eng, mode, oversample=4):
    L.check(eng._lib.aid_vec_prefilter(eng._h, mode, oversample))


def stats(eng, reset_=True):
    out = (ctypes.c_int64 * 6)()
    L.check(eng._lib.aid_vec_prefilter_stats(eng._h, out, 6, int(reset_)))
    return dict(zip(STAT_NAMES, (int(v) for v in out)))


def scores_i8(eng, q, n):
    q = np.ascontiguousarray(q)
    approx = np.full((len(q), n), np.nan, np.float32)
    eps = np.full(len(q), np.nan, np.float64)
    L.check(eng._lib.aid_vec_scores_i8(eng._h, _p(q), len(q), L.AID_PCM_HOST, _p(approx), _p(eps), approx.size))
    return approx, eps


@pytest.fixture()
def eng(gpu_engine):
    stats(gpu_engine)
    yield gpu_engine
    gpu_engine.force("vec_chunk", 0)
    gpu_engine.force("vec_cand", 0)
    prefilter(gpu_engine, 0)
    L.check(gpu_engine._lib.aid_vec_reset(gpu_engine._h, 512))


@pytest.fixture(scope="module")
def d512():
    d = Data(512, 11)
    d.q8 = Q.Catalog(d.cn)
    d.A, d.eps = d.q8.view(d.qn)
    return d


@pytest.fixture(scope="module")
def neardup():
    return Q.NearDup()


class Raw:
    """A catalog of raw vectors with the payload columns `add` wants."""

    def __init__(self, cat):
        self.cat = cat
        n = len(cat)
        self.tracks = (np.arange(n) % Q.NTRACKS).astype(np.uint32)
        self.chunk = (np.arange(n) // Q.NTRACKS).astype(np.int32)
        self.off = (self.chunk % 6) * 5.0


@pytest.mark.parametrize("dim", [512, 64, 32, 1024])
def test_approx_and_eps_equal_the_oracle(eng, dim):
    """Asymmetric data, 70 queries (two full tiles and 6 rows), 300 entries (nine tiles and 12 rows)."""
    cat, q = Q.asymmetric(dim, N, NQ)
    c8 = Q.Catalog(V.normalize(cat))
    A, eps = c8.view(V.normalize(q))
    assert len(np.unique(A)) > A.size // 2
    d = Raw(cat)
    for chunk in CHUNKS:
        eng.force("vec_chunk", chunk)
        for n in (1, 33, N):
            reset(eng, dim)
            prefilter(eng, 1)
            add(eng, d, 0, n)
            cn = Q.Catalog(c8.cn[:n])
            for nq in (1, 33, NQ):
                got, geps = scores_i8(eng, q[:nq], n)
                want, weps = (A[:nq], eps[:nq]) if n == N else cn.view(V.normalize(q[:nq]))
                assert np.array_equal(bits(got), bits(want)), (chunk, n, nq)
                assert np.array_equal(geps, weps), (chunk, n, nq)
    assert stats(eng)["i8_scans"] == len(CHUNKS) * 3 * 4  # 70 queries are two batches


@pytest.mark.parametrize("chunk", CHUNKS)
def test_a_clustered_catalog_hits_equal_the_oracle(eng, d512, chunk):
    d = d512
    eng.force("vec_chunk", chunk)
    reset(eng, 512)
    for lo in (0, 100, 200):
        add(eng, d, lo, lo + 100)
    live = np.ones(N, bool)
    for over in (1, 4):
        prefilter(eng, 0)  # a change of oversample alone keeps the planes: off and on rebuilds them as well
        prefilter(eng, 1, over)
        stats(eng)
        for limit in (1, 5, 50, 299, 300, 1024):
            check_hits(search(eng, d.q, limit), d, d.S, live, limit)
        st = stats(eng)
        assert st["fell_back"] == 0 and st["answered"] == 6 * NQ
        want_w = sum(len(Q.route(d.A[q], d.eps[q], d.S[q], live, limit, over)["W"]) for q in range(NQ)
                     for limit in (1, 5, 50, 299, 300, 1024))
        assert st["w_total"] == want_w
    # the three copies tie at the top of query 2 in entry order, as without the prefilter
    assert list(search(eng, d.q[2:3], 2)[0]["entry"]) == [10, 150]


def test_b_life_cycle(eng, d512, tmp_path):
    d = d512
    live = np.ones(N, bool)
    # enabled first, then adds in batches that cross a tile edge
    reset(eng, 512)
    prefilter(eng, 1)
    for lo, hi in ((0, 33), (33, 64), (64, N)):
        add(eng, d, lo, hi)
    a_on, e_on = scores_i8(eng, d.q, N)
    assert np.array_equal(bits(a_on), bits(d.A)) and np.array_equal(e_on, d.eps)
    # enabled after the adds: the same planes
    prefilter(eng, 0)
    assert eng._lib.aid_vec_scores_i8(eng._h, _p(d.q), 1, L.AID_PCM_HOST, _p(a_on.copy()), _p(e_on.copy()), a_on.size) \
        == L.AID_ERR_STATE
    reset(eng, 512)
    add(eng, d, 0, N)
    off_rows = VectorIndex.vibe_raw(_Ix(eng), d.q, 5, None, 0.2, 3, 0.05, 50)
    prefilter(eng, 1)
    a2, e2 = scores_i8(eng, d.q, N)
    assert np.array_equal(bits(a2), bits(a_on)) and np.array_equal(e2, e_on)
    on_rows = VectorIndex.vibe_raw(_Ix(eng), d.q, 5, None, 0.2, 3, 0.05, 50)
    assert sum(map(len, off_rows)) > NQ and all(np.array_equal(a, b) for a, b in zip(on_rows, off_rows))

    # a removed track never takes a slot, even where it holds the best approx
    gone = int(d.tracks[np.argmax(d.A[0])])
    L.check(eng._lib.aid_vec_remove(eng._h, gone))
    live = d.tracks != gone
    for limit in (1, 5, 50, 1024):
        got = search(eng, d.q, limit)
        check_hits(got, d, d.S, live, limit)
        assert not any((g["track"] == gone).any() for g in got)
    # save with the prefilter on (tombstones included), then compact and search
    path = tmp_path / "cat.vec"
    L.check(eng._lib.aid_vec_save(eng._h, str(path).encode()))
    n_rm = ctypes.c_int64()
    L.check(eng._lib.aid_vec_compact(eng._h, ctypes.byref(n_rm)))
    assert n_rm.value == N - int(live.sum())
    entry_of = np.cumsum(live) - 1
    for limit in (5, 50, 1024):
        check_hits(search(eng, d.q, limit), d, d.S, live, limit, entry_of=entry_of)
    c_live = Q.Catalog(d.cn[live])  # E is recomputed over the rows that remain
    a3, e3 = scores_i8(eng, d.q, int(live.sum()))
    w3, we3 = c_live.view(d.qn)
    assert np.array_equal(bits(a3), bits(w3)) and np.array_equal(e3, we3)
    add(eng, d, 0, 40)  # and the catalog still grows after it
    S2 = np.concatenate([d.S[:, live], d.S[:, :40]], axis=1)
    d2 = Raw(np.concatenate([d.cat[live], d.cat[:40]]))
    d2.tracks, d2.chunk, d2.off = (np.concatenate([x[live], x[:40]]) for x in (d.tracks, d.chunk, d.off))
    check_hits(search(eng, d.q[:33], 50), d2, S2, np.ones(S2.shape[1], bool), 50)

    # the file loads into a fresh engine with the prefilter on, and with it off
    live = d.tracks != gone
    e2 = Engine(44100)
    try:
        for mode in (1, 0):
            L.check(e2._lib.aid_vec_reset(e2._h, 64))
            prefilter(e2, mode)
            L.check(e2._lib.aid_vec_load(e2._h, str(path).encode()))
            check_hits(search(e2, d.q, 50), d, d.S, live, 50)
            if mode:
                a4, e4 = scores_i8(e2, d.q[:5], N)  # dead rows count in E
                assert np.array_equal(bits(a4), bits(d.A[:5])) and np.array_equal(e4, d.eps[:5])
                st = stats(e2)
                assert st["answered"] == NQ and st["fell_back"] == 0
            else:
                assert stats(e2) == dict.fromkeys(STAT_NAMES, 0)
    finally:
        e2.close()


class _Ix:
    """Enough of a VectorIndex for its raw calls on a catalog loaded through the C ABI."""

    dim = 512

    def __init__(self, eng):
        self.eng = eng


def test_c_near_duplicates_are_decided_by_the_widened_rescoring(eng, neardup):
    d = neardup
    live = np.ones(N, bool)
    for chunk in CHUNKS:
        eng.force("vec_chunk", chunk)
        reset(eng, d.dim)
        add(eng, d, 0, N)
        for limit, over in ((5, 4), (10, 1), (20, 2)):
            prefilter(eng, 1, over)
            stats(eng)
            check_hits(search(eng, d.q[:6], limit), d, d.S, live, limit)
            w = [len(Q.route(d.A[q], d.eps[q], d.S[q], live, limit, over)["W"]) for q in range(6)]
            st = stats(eng)
            assert (st["w_total"], st["w_max"], st["fell_back"], st["answered"]) == (sum(w), max(w), 0, 6)
            assert st["rescored_pairs"] == 6 * Q.candidates(limit, over) + sum(w)


def test_d_fallbacks_within_a_batch(eng, neardup):
    d = neardup
    live = np.ones(N, bool)
    for chunk in CHUNKS:
        eng.force("vec_chunk", chunk)
        reset(eng, d.dim)
        add(eng, d, 0, N)
        prefilter(eng, 1, 4)
        eng.force("vec_cand", 64)
        for limit in (1, 5):
            stats(eng)
            check_hits(search(eng, d.q, limit), d, d.S, live, limit)  # certified and falling back in one batch
            r = [Q.route(d.A[q], d.eps[q], d.S[q], live, limit, 4, cap=64) for q in range(len(d.q))]
            st = stats(eng)
            assert st["fell_back"] == sum(x["fallback"] for x in r) == 7 and st["answered"] == 3
            assert st["w_total"] == sum(len(x["W"]) for x in r) and st["w_max"] == N  # the zero query: W is all
        eng.force("vec_cand", 0)  # the default cap: nobody falls back
        check_hits(search(eng, d.q, 5), d, d.S, live, 5)
        assert stats(eng)["fell_back"] == 0
    # 70 queries, two batches, every third one falling back
    eng.force("vec_cand", 64)
    qq = np.ascontiguousarray(d.q[np.arange(NQ) % 10])
    got = search(eng, qq, 5)
    check_hits(got, d, d.S, live, 5, qs=list(np.arange(NQ) % 10))
    assert stats(eng)["fell_back"] == 49


def test_bad_arguments(eng, d512):
    reset(eng, 512)
    h = eng._h
    for mode, over in ((2, 4), (-1, 4), (1, 0), (1, 65), (0, 0)):
        assert eng._lib.aid_vec_prefilter(h, mode, over) == L.AID_ERR_INVALID
    q = np.ascontiguousarray(d512.q[:1])
    a, e = np.zeros(N, np.float32), np.zeros(1)
    assert eng._lib.aid_vec_scores_i8(h, _p(q), 1, L.AID_PCM_HOST, _p(a), _p(e), N) == L.AID_ERR_STATE
    assert "prefilter is off" in L.last_error()
    prefilter(eng, 1)
    add(eng, d512, 0, 40)
    assert eng._lib.aid_vec_scores_i8(h, _p(q), 1, L.AID_PCM_HOST, _p(a), _p(e), 39) == L.AID_ERR_INVALID
    assert eng._lib.aid_vec_scores_i8(h, _p(q), 1, L.AID_PCM_HOST, _p(a), None, N) == L.AID_ERR_INVALID
    assert eng._lib.aid_engine_force(h, L.AID_FORCE_VEC_CAND, 4097) == L.AID_ERR_INVALID
    assert eng._lib.aid_engine_force(h, L.AID_FORCE_VEC_CAND, -1) == L.AID_ERR_INVALID
    assert eng._lib.aid_vec_prefilter_stats(h, None, 6, 0) == L.AID_ERR_INVALID
    prefilter(eng, 0)
    reset(eng, 512)
    prefilter(eng, 1)
    assert search(eng, q, 50)[0].size == 0  # an empty catalog answers with empty lists


def test_adapter_prefilter_option_environment_and_threads(eng, d512, monkeypatch):
    d = d512
    with pytest.raises(ValueError):
        VectorIndex(eng, 512, prefilter="int4")
    monkeypatch.setenv("AIDFP_VEC_PREFILTER", "int8")
    assert VectorIndex(eng, 512).prefilter == "int8"
    monkeypatch.delenv("AIDFP_VEC_PREFILTER")
    assert VectorIndex(eng, 512).prefilter == "off"
    ids = [uuid.UUID(int=(t + 1) * 0x1234567) for t in range(Q.NTRACKS)]
    ix = VectorIndex(eng, 512, prefilter="int8", oversample=2)
    perm = np.concatenate([np.flatnonzero(d.tracks == t) for t in range(Q.NTRACKS)])
    for t in range(Q.NTRACKS):
        e = np.flatnonzero(d.tracks == t)
        ix.upsert_track(ids[t], d.cat[e], d.off[e], d.chunk[e])
    S, tr, off = d.S[:, perm], d.tracks[perm], d.off[perm]
    live = np.ones(N, bool)

    def want_rows(q):
        e = V.hit_list(S[q], live, 50)
        rows = V.aggregate(list(zip(tr[e].tolist(), S[q][e], off[e].tolist())), 3, 0.05, None, 0.60, 10)
        return [vibe.TrackResult(ids[r[0]], r[2], r[3], r[4], r[1]) for r in rows]

    want = [want_rows(q) for q in range(NQ)]
    assert sum(map(len, want)) > NQ // 2
    results = {}

    def worker(k):
        results[k] = [ix.vibe(d.q, 10) for _ in range(3)]

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert all(r == want for k in range(2) for r in results[k])
    st = ix.prefilter_stats(reset=True)
    assert st["answered"] == 6 * NQ and st["fell_back"] == 0 and st["i8_scans"] == 12
    assert ix.prefilter_stats() == dict.fromkeys(STAT_NAMES, 0)
