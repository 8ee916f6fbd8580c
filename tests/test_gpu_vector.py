"""Vector lane on the GPU (K9, spec/FPSPEC.md 9): scores, stored vectors, hit lists, aggregation, persistence and
the Python adapter against the numpy oracle tests/vec_ref.py. Comparisons are bit for bit."""

import ctypes
import json
import threading
import uuid
from pathlib import Path

import numpy as np
import pytest
import vec_ref as V

from aidfp import _lib as L
from aidfp import vibe
from aidfp.vibe import HIT_DTYPE, VectorIndex, aggregate_hits

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "ref_vibe.json"
N, NQ, NTRACKS = 300, 70, 40
TRIPLE = (10, 150, 299)  # the same vector stored three times
# (AID_FORCE_VEC_PATH, AID_FORCE_VEC_CHUNK): 64 rows = 5 chunks, the last of 44; 32 rows = 10 chunks, the last of 12.
# With 5 or 10 slices the selection goes by threshold for limit <= 5 and slice by slice above it.
PATHS = [(1, 0), (1, 64), (1, 32), (2, 0), (2, 64)]


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


class Data:
    """One clustered catalog (entry e belongs to track e % 40) with its queries and the oracle's results."""

    def __init__(self, dim, seed):
        rng = np.random.default_rng(seed)
        cent = rng.standard_normal((NTRACKS, dim))
        self.dim = dim
        self.tracks = (np.arange(N) % NTRACKS).astype(np.uint32)
        self.chunk = (np.arange(N) // NTRACKS).astype(np.int32)
        self.off = (self.chunk % 6) * 5.0  # chunks 0 and 6 of a track share an offset
        cat = (cent[self.tracks] + 0.7 * rng.standard_normal((N, dim))).astype(np.float32)
        cat[5] = 0                      # all zero: stored as zeros
        cat[7, 3] = np.inf              # not finite: stored as zeros
        cat[TRIPLE[1]] = cat[TRIPLE[0]]
        cat[TRIPLE[2]] = cat[TRIPLE[0]] * np.float32(2)  # the same direction at another gain: the same unit vector
        q = (cent[rng.integers(0, NTRACKS, size=NQ)] + 0.7 * rng.standard_normal((NQ, dim))).astype(np.float32)
        q[2] = cat[TRIPLE[0]]           # equal to a stored vector: a three-way tie at the top
        q[4] = cat[20]
        self.cat, self.q = cat, q
        self.cn, self.qn = V.normalize(cat), V.normalize(q)
        self.S = V.scores(self.qn, self.cn)


@pytest.fixture(scope="module")
def d512():
    return Data(512, 11)


@pytest.fixture(scope="module")
def d64():
    return Data(64, 12)


@pytest.fixture()
def eng(gpu_engine):
    yield gpu_engine
    gpu_engine.force("vec_path", 0)
    gpu_engine.force("vec_chunk", 0)
    L.check(gpu_engine._lib.aid_vec_reset(gpu_engine._h, 512))


def reset(eng, dim):
    L.check(eng._lib.aid_vec_reset(eng._h, dim))


def add(eng, d, lo, hi):
    L.check(eng._lib.aid_vec_add(eng._h, _p(np.ascontiguousarray(d.cat[lo:hi])), _p(np.ascontiguousarray(d.tracks[lo:hi])),
                                 _p(np.ascontiguousarray(d.chunk[lo:hi])), _p(np.ascontiguousarray(d.off[lo:hi])),
                                 hi - lo, L.AID_PCM_HOST))


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


def check_hits(got, d, S, live, limit, entry_of=None, qs=None):
    """got[q] equals the oracle's list: entries, score bits and payload. entry_of: oracle entry -> engine entry."""
    for i, q in enumerate(range(len(got)) if qs is None else qs):
        want = V.hit_list(S[q], live, limit)
        g = got[i]
        assert len(g) == len(want) == min(limit, int(live.sum())), q
        assert np.array_equal(g["entry"], want if entry_of is None else entry_of[want]), q
        assert np.array_equal(bits(g["score"]), bits(S[q][want])), q
        assert np.array_equal(g["track"], d.tracks[want]) and np.array_equal(g["chunk_index"], d.chunk[want]), q
        assert np.array_equal(g["offset_sec"], d.off[want]), q


@pytest.mark.parametrize("dim", [512, 64])
@pytest.mark.parametrize("path,chunk", PATHS)
def test_scores_equal_the_oracle(eng, d512, d64, path, chunk, dim):
    d = d512 if dim == 512 else d64
    eng.force("vec_path", path)
    eng.force("vec_chunk", chunk)
    for n in (1, 31, 32, 33, N):
        reset(eng, dim)
        add(eng, d, 0, n)
        for nq in (1, 3, 32, 33, NQ):
            got = gpu_scores(eng, d.q[:nq], n)
            assert np.array_equal(bits(got), bits(d.S[:nq, :n])), (n, nq)
    # the special vectors did what the spec says (n = 300 is still loaded)
    assert not d.cn[5].any() and not d.cn[7].any() and not got[:, 5].any() and not got[:, 7].any()
    assert np.array_equal(d.cn[TRIPLE[0]], d.cn[TRIPLE[2]])


@pytest.mark.parametrize("dim,n", [(512, N), (64, 33)])
def test_stored_vectors_equal_the_oracle(eng, d512, d64, tmp_path, dim, n):
    d = d512 if dim == 512 else d64
    reset(eng, dim)
    add(eng, d, 0, n // 2)
    add(eng, d, n // 2, n)
    path = tmp_path / "cat.vec"
    L.check(eng._lib.aid_vec_save(eng._h, str(path).encode()))
    raw = path.read_bytes()
    assert raw[:8] == b"AIDFPVC1"
    ver, fdim, fn = np.frombuffer(raw[8:12], "<u4")[0], np.frombuffer(raw[12:16], "<i4")[0], np.frombuffer(raw[16:24], "<i8")[0]
    assert (ver, fdim, fn) == (1, dim, n)
    nf = ((n + 31) // 32) * 32 * dim
    assert len(raw) == 24 + nf * 4 + 17 * n
    stored = np.frombuffer(raw[24 : 24 + nf * 4], "<f4")
    assert np.array_equal(bits(V.detile(stored, n, dim)), bits(d.cn[:n]))
    assert np.array_equal(np.frombuffer(raw[24 + nf * 4 : 24 + nf * 4 + 4 * n], "<u4"), d.tracks[:n])


@pytest.mark.parametrize("path,chunk", PATHS)
def test_hits_equal_the_oracle(eng, d512, path, chunk):
    d = d512
    eng.force("vec_path", path)
    eng.force("vec_chunk", chunk)
    reset(eng, 512)
    for lo in (0, 100, 200):  # the catalog grows call by call
        add(eng, d, lo, lo + 100)
    live = np.ones(N, bool)
    for limit in (1, 5, 50, 1024):
        check_hits(search(eng, d.q, limit), d, d.S, live, limit)
    # the three copies tie at the top of query 2: ascending entry order, and limit 1 cuts through the tie
    top = search(eng, d.q[2:3], 50)[0]
    assert list(top["entry"][:3]) == list(TRIPLE) and len(set(bits(top["score"][:3]))) == 1
    assert list(search(eng, d.q[2:3], 1)[0]["entry"]) == [TRIPLE[0]]
    assert list(search(eng, d.q[2:3], 2)[0]["entry"]) == list(TRIPLE[:2])

    # remove a track whose entries are in query 0's top 50: they vanish and the list refills from below
    before = search(eng, d.q[:1], 50)[0]
    gone = int(before["track"][0])
    assert np.count_nonzero(before["track"] == gone) >= 2
    L.check(eng._lib.aid_vec_remove(eng._h, gone))
    assert eng._lib.aid_vec_remove(eng._h, gone) == L.AID_ERR_INVALID      # already removed
    assert eng._lib.aid_vec_remove(eng._h, 12345) == L.AID_ERR_INVALID     # unknown
    live = d.tracks != gone
    n_e, n_l = ctypes.c_int64(), ctypes.c_int64()
    L.check(eng._lib.aid_vec_count(eng._h, ctypes.byref(n_e), ctypes.byref(n_l), None))
    assert (n_e.value, n_l.value) == (N, int(live.sum()))
    for limit in (1, 5, 50, 1024):
        got = search(eng, d.q, limit)
        check_hits(got, d, d.S, live, limit)
        assert not any((g["track"] == gone).any() for g in got)
    assert len(search(eng, d.q[:1], 50)[0]) == 50
    # the score matrix still has the removed entries
    assert np.array_equal(bits(gpu_scores(eng, d.q[:3], N)), bits(d.S[:3]))

    # compaction renumbers the entries and changes nothing else
    n_rm = ctypes.c_int64()
    L.check(eng._lib.aid_vec_compact(eng._h, ctypes.byref(n_rm)))
    assert n_rm.value == N - int(live.sum())
    entry_of = np.cumsum(live) - 1
    for limit in (1, 5, 50, 1024):
        check_hits(search(eng, d.q, limit), d, d.S, live, limit, entry_of=entry_of)
    add(eng, d, 0, 40)  # and the catalog still grows after it
    S2 = np.concatenate([d.S[:, live], d.S[:, :40]], axis=1)
    assert np.array_equal(bits(gpu_scores(eng, d.q[:33], S2.shape[1])), bits(S2[:33]))


@pytest.mark.parametrize("chunk,limit", [(0, 3), (32, 50), (32, 1024)])
def test_more_ties_than_the_candidate_list_holds(eng, chunk, limit):
    """5000 copies of one vector: every score ties, the threshold route's candidate list (4096) overflows and the
    slice-by-slice route answers; the hits are the first live entries."""
    n, dim = 5000, 32
    rng = np.random.default_rng(5)
    v = rng.standard_normal((1, dim)).astype(np.float32)
    q = rng.standard_normal((2, dim)).astype(np.float32)
    s = V.scores(V.normalize(q), V.normalize(v))[:, 0]
    eng.force("vec_chunk", chunk)
    reset(eng, dim)
    cat = np.ascontiguousarray(np.repeat(v, n, axis=0))
    tracks = (np.arange(n) // 2).astype(np.uint32)
    L.check(eng._lib.aid_vec_add(eng._h, _p(cat), _p(tracks), None, _p(np.zeros(n)), n, L.AID_PCM_HOST))
    L.check(eng._lib.aid_vec_remove(eng._h, 0))  # entries 0 and 1
    for qi, g in enumerate(search(eng, q, limit)):
        assert np.array_equal(g["entry"], np.arange(2, 2 + limit))
        assert np.array_equal(bits(g["score"]), np.full(limit, bits(s[qi : qi + 1])[0]))
        assert np.array_equal(g["track"], tracks[2 : 2 + limit]) and np.array_equal(g["chunk_index"], np.arange(2, 2 + limit))


def test_aggregate_reproduces_reference_vectors(eng):
    cases = json.loads(GOLDEN.read_text())["cases"]
    lists, excl, want = [], [], []
    for c in cases:
        ids = {}
        for h in c["hits"]:
            ids.setdefault(h["track"], len(ids))
        hl = np.zeros(len(c["hits"]), HIT_DTYPE)
        for i, h in enumerate(c["hits"]):
            hl[i] = (i, ids[h["track"]], h["chunk_index"], h["score"], h["offset_sec"])
        lists.append(hl)
        excl.append(vibe.VEC_NO_TRACK if c["exclude"] is None else ids.get(c["exclude"], 4_000_000))
        want.append([(ids[r["track"]], r["chunk_count"], r["final_score"], r["base_score"], r["diversity_bonus"])
                     for r in c["rows"]])
    # the cases differ in top_k and weight: one call per setting, every list of that setting in it
    for key in sorted({(c["top_k_per_track"], c["diversity_weight"]) for c in cases}):
        sel = [i for i, c in enumerate(cases) if (c["top_k_per_track"], c["diversity_weight"]) == key]
        got = aggregate_hits(eng, [lists[i] for i in sel], key[0], key[1], exclude=[excl[i] for i in sel], max_out=64)
        for i, g in zip(sel, got):
            assert [tuple(r) for r in g.tolist()] == want[i], cases[i]["note"]


def oracle_lane(d, S, live, q, limit, top_k, weight, exclude, threshold, max_out):
    e = V.hit_list(S[q], live, limit)
    return V.aggregate(list(zip(d.tracks[e].tolist(), S[q][e], d.off[e].tolist())), top_k, weight,
                       None if exclude == vibe.VEC_NO_TRACK else exclude, threshold, max_out)


@pytest.mark.parametrize("path,chunk", [(1, 64), (2, 0)])
def test_lane_equals_search_then_aggregate_and_the_oracle(eng, d512, path, chunk):
    d = d512
    eng.force("vec_path", path)
    eng.force("vec_chunk", chunk)
    ix = VectorIndex(eng, 512)  # its raw calls (engine ids), on a catalog loaded through the C ABI
    add(eng, d, 0, N)
    live = np.ones(N, bool)
    top1 = [int(V.hit_list(d.S[q], live, 1)[0]) for q in range(NQ)]
    excl = [int(d.tracks[top1[q]]) if q % 2 else vibe.VEC_NO_TRACK for q in range(NQ)]
    seen_rows = 0
    for limit, top_k, weight, thr, max_out in [(50, 3, 0.05, 0.60, 5), (50, 1, 0.3, 0.2, 50), (1024, 10, 0.0, -1.0, 3)]:
        lane = ix.vibe_raw(d.q, max_out, excl, thr, top_k, weight, limit)
        two = aggregate_hits(eng, search(eng, d.q, limit), top_k, weight, exclude=excl, threshold=thr, max_out=max_out)
        for q in range(NQ):
            want = oracle_lane(d, d.S, live, q, limit, top_k, weight, excl[q], thr, max_out)
            assert [tuple(r) for r in lane[q].tolist()] == want, q
            assert [tuple(r) for r in two[q].tolist()] == want, q
            seen_rows += len(want)
    assert seen_rows > NQ  # the thresholds left something to compare


def test_save_load_round_trip_and_truncated_file(eng, d512, tmp_path):
    d = d512
    reset(eng, 512)
    add(eng, d, 0, N)
    L.check(eng._lib.aid_vec_remove(eng._h, 3))
    live = d.tracks != 3
    path = tmp_path / "cat.vec"
    L.check(eng._lib.aid_vec_save(eng._h, str(path).encode()))
    reset(eng, 64)
    assert search(eng, d64_query(), 5)[0].size == 0
    L.check(eng._lib.aid_vec_load(eng._h, str(path).encode()))
    n_e, n_l, dim = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
    L.check(eng._lib.aid_vec_count(eng._h, ctypes.byref(n_e), ctypes.byref(n_l), ctypes.byref(dim)))
    assert (n_e.value, n_l.value, dim.value) == (N, int(live.sum()), 512)
    check_hits(search(eng, d.q, 50), d, d.S, live, 50)
    # a file cut short, a foreign file and a missing one: refused, catalog untouched
    cut = tmp_path / "cut.vec"
    cut.write_bytes(path.read_bytes()[:-100])
    other = tmp_path / "other.vec"
    other.write_bytes(b"AIDFPIX1" + path.read_bytes()[8:])
    for bad in (cut, other, tmp_path / "missing.vec"):
        assert eng._lib.aid_vec_load(eng._h, str(bad).encode()) == L.AID_ERR_INVALID
        L.check(eng._lib.aid_vec_count(eng._h, ctypes.byref(n_e), ctypes.byref(n_l), ctypes.byref(dim)))
        assert (n_e.value, n_l.value, dim.value) == (N, int(live.sum()), 512)
    check_hits(search(eng, d.q[:8], 50), d, d.S, live, 50)


def d64_query():
    return np.ones((1, 64), np.float32)


def test_bad_arguments_with_an_engine(eng, d512):
    reset(eng, 512)
    h = eng._h
    q = np.ascontiguousarray(d512.q[:1])
    hits, nh = np.zeros(2048, HIT_DTYPE), np.zeros(1, np.int32)
    for dim in (0, 16, 500, 1056):
        assert eng._lib.aid_vec_reset(h, dim) == L.AID_ERR_INVALID
    for limit in (0, -1, 1025):
        assert eng._lib.aid_vec_search(h, _p(q), 1, L.AID_PCM_HOST, limit, _p(hits), _p(nh), None) == L.AID_ERR_INVALID
    assert eng._lib.aid_engine_force(h, L.AID_FORCE_VEC_CHUNK, 48) == L.AID_ERR_INVALID
    assert eng._lib.aid_engine_force(h, L.AID_FORCE_VEC_PATH, 3) == L.AID_ERR_INVALID
    assert search(eng, q, 50)[0].size == 0  # an empty catalog answers with empty lists


def test_adapter_with_uuids_numpy_torch_and_threads(eng, d512, tmp_path):
    import torch

    d = d512
    ids = [uuid.UUID(int=(t + 1) * 0x1234567) for t in range(NTRACKS)]
    ix = VectorIndex(eng, 512)
    perm = np.concatenate([np.flatnonzero(d.tracks == t) for t in range(NTRACKS)])  # the adapter stores track by track
    for t in range(NTRACKS):
        e = np.flatnonzero(d.tracks == t)
        emb = torch.from_numpy(d.cat[e]).cuda() if t % 2 else d.cat[e]  # device tensors and numpy arrays alike
        assert ix.upsert_track(ids[t], emb, d.off[e], d.chunk[e]) == len(e)
    assert ix.counts() == (N, N)
    S = d.S[:, perm]
    tr, ch, off = d.tracks[perm], d.chunk[perm], d.off[perm]

    def want_hits(q, live, limit=50):
        e = V.hit_list(S[q], live, limit)
        return [vibe.ChunkHit(ids[tr[i]], float(S[q][i]), int(ch[i]), float(off[i])) for i in e]

    live = np.ones(N, bool)
    got_np = ix.search(d.q[:5], 50)
    got_t = ix.search(torch.from_numpy(d.q[:5]).cuda(), 50)
    assert got_np == got_t == [want_hits(q, live) for q in range(5)]

    def want_rows(q, live, exclude=None):
        e = V.hit_list(S[q], live, 50)
        rows = V.aggregate(list(zip(tr[e].tolist(), S[q][e], off[e].tolist())), 3, 0.05, exclude, 0.60, 10)
        return [vibe.TrackResult(ids[r[0]], r[2], r[3], r[4], r[1]) for r in rows]

    want = [want_rows(q, live) for q in range(NQ)]
    assert sum(map(len, want)) > NQ // 2
    results = {}

    def worker(k):
        src = torch.from_numpy(d.q).cuda() if k else d.q
        results[k] = [ix.vibe(src, 10) for _ in range(3)]

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert all(r == want for k in range(2) for r in results[k])
    # the exact lane's match is left out per query
    ex_t = int(tr[V.hit_list(S[0], live, 1)[0]])
    assert ix.vibe(d.q[:1], 10, exact_match_track_ids=[ids[ex_t]]) == [want_rows(0, live, exclude=ex_t)]

    # save / load through the adapter, then delete
    ix.save(tmp_path / "ix.vec")
    ix2 = VectorIndex(eng, 512)
    assert len(ix2) == 0
    ix2.load(tmp_path / "ix.vec")
    assert ix2.search(d.q[:5], 50) == got_np
    assert ix2.delete_track(ids[ex_t]) and not ix2.delete_track(ids[ex_t]) and not ix2.delete_track(uuid.uuid4())
    live = tr != ex_t
    assert ix2.search(d.q[:5], 50) == [want_hits(q, live) for q in range(5)]
    # an upsert of a stored track replaces its chunks
    u = 1 if ex_t != 1 else 2
    e = np.flatnonzero(d.tracks == u)
    ix2.upsert_track(ids[u], d.cat[e][:2], d.off[e][:2], d.chunk[e][:2])
    assert ix2.counts() == (N + 2, int(live.sum()) - len(e) + 2)
