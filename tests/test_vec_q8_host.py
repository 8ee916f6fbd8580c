"""The int8 prefilter's oracle on the CPU (spec/FPSPEC.md 9.1, tests/vec_q8_ref.py): known answers of the quantiser,
the error bound |score - approx| <= eps on the data that stress it, and the preconditions of the fixtures that
tests/test_gpu_vector_q8.py runs on the GPU."""

import numpy as np
import pytest
import vec_q8_ref as Q
import vec_ref as V

F32 = np.float32


def test_quantiser_known_answers():
    # a = 127 so s = 1 exactly: ties at .5 go to even, the largest value maps to 127
    y = np.zeros((1, 32), F32)
    y[0, :8] = [127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5]
    i, s, e = Q.quantize(y)
    assert s[0] == 1.0
    assert list(i[0, :8]) == [127, 0, 2, 2, 0, -2, -2, 126]
    # the residual: six values are off by 0.5, one by 0.5 (126.5 -> 126): sqrt(7 * 0.25)
    assert e[0] == F32(np.sqrt(7 * 0.25))
    # the clamp: a / 127 rounds down here, so y / s lands above 127 and rint alone would not do
    found = False
    for a in np.linspace(0.1, 1.0, 2000, dtype=F32):
        s1 = F32(a) / F32(127.0)
        if np.rint(F32(a) / s1) > 127 or np.float64(a) / np.float64(s1) > 127.0:
            found = True
        y = np.zeros((1, 32), F32)
        y[0, 0], y[0, 1] = a, -a
        i, s, _ = Q.quantize(y)
        assert (i[0, 0], i[0, 1]) == (127, -127) and s[0] == s1
    assert found
    # a zero vector: s = +0, every value 0, e = 0
    i, s, e = Q.quantize(np.zeros((2, 64), F32))
    assert not i.any() and not s.any() and not e.any() and not np.signbit(s).any()
    # a one-hot vector: one value at +-127, s = 1 / 127, e = |1 - s * 127| (s is rounded)
    y = np.zeros((2, 64), F32)
    y[0, 5], y[1, 63] = 1.0, -1.0
    i, s, e = Q.quantize(y)
    assert i[0, 5] == 127 and i[1, 63] == -127 and np.count_nonzero(i) == 2
    assert s[0] == s[1] == F32(1.0) / F32(127.0)
    assert e[0] == e[1] == F32(abs(1.0 - float(s[0]) * 127.0))


def test_eps_and_candidate_count():
    assert Q.candidates(50, 4) == 200 and Q.candidates(1, 1) == 1 and Q.candidates(1024, 1) == 1024
    assert Q.candidates(300, 4) == 1024 and Q.candidates(5, 64) == 320
    e = Q.eps(F32(0.25), F32(0.5), 512)
    assert e == (0.25 + 1.25 * 0.5) * (1 + 2.0**-10) + 512 * 2.0**-21
    assert Q.eps(F32(0), F32(0), 32) == 32 * 2.0**-21


def _bound_holds(cat, q):
    cn, qn = V.normalize(cat), V.normalize(q)
    S = V.scores(qn, cn)
    c8 = Q.Catalog(cn)
    A, eps = c8.view(qn)
    err = np.abs(S.astype(np.float64) - A.astype(np.float64))
    assert (err <= eps[:, None]).all(), float((err / eps[:, None]).max())
    return float((err / eps[:, None]).max())


@pytest.mark.parametrize("dim", [32, 64, 512, 1024])
def test_bound_on_random_one_hot_and_equal_magnitude_vectors(dim):
    rng = np.random.default_rng(100 + dim)
    n, nq = 96, 24
    # random, clustered
    cent = rng.standard_normal((8, dim))
    cat = cent[rng.integers(0, 8, n)] + 0.7 * rng.standard_normal((n, dim))
    q = cent[rng.integers(0, 8, nq)] + 0.7 * rng.standard_normal((nq, dim))
    worst = _bound_holds(cat.astype(F32), q.astype(F32))
    # one component dominates: the coarsest step and the largest residual
    hot = 0.02 * rng.standard_normal((n, dim))
    hot[np.arange(n), rng.integers(0, dim, n)] = rng.choice([-1.0, 1.0], n)
    hq = 0.02 * rng.standard_normal((nq, dim))
    hq[np.arange(nq), rng.integers(0, dim, nq)] = 1.0
    worst = max(worst, _bound_holds(hot.astype(F32), hq.astype(F32)))
    worst = max(worst, _bound_holds(hot.astype(F32), q.astype(F32)))
    # equal magnitudes: every component at +-127
    eq = rng.choice([-1.0, 1.0], (n, dim)) * 0.37
    eqq = rng.choice([-1.0, 1.0], (nq, dim)) * 5.0
    i, _, _ = Q.quantize(V.normalize(eq.astype(F32)))
    assert (np.abs(i) == 127).all()
    worst = max(worst, _bound_holds(eq.astype(F32), eqq.astype(F32)))
    worst = max(worst, _bound_holds(eq.astype(F32), hq.astype(F32)))
    assert 0 < worst <= 1


@pytest.fixture(scope="module")
def clustered():
    from test_gpu_vector import Data

    d = Data(512, 11)
    d.q8 = Q.Catalog(d.cn)
    d.A, d.eps = d.q8.view(d.qn)
    return d


def test_fixture_a_has_no_fallback_and_certifies_the_true_list(clustered):
    d = clustered
    live = np.ones(Q.N, bool)
    for over in (1, 4):
        for limit in (1, 5, 50, 299, 300, 1024):
            for q in range(len(d.q)):
                r = Q.route(d.A[q], d.eps[q], d.S[q], live, limit, over)
                assert not r["fallback"]
                assert np.array_equal(r["hits"], V.hit_list(d.S[q], live, limit)), (over, limit, q)


@pytest.fixture(scope="module")
def neardup():
    return Q.NearDup()


def test_fixture_c_is_decided_by_the_widened_rescoring(neardup):
    d = neardup
    live = np.ones(Q.N, bool)
    err = np.abs(d.S.astype(np.float64) - d.A.astype(np.float64))
    assert (err <= d.eps[:, None]).all()
    # the cluster's approx values lie within a fraction of eps of one another while its scores all differ
    assert np.ptp(d.A[0, : d.NDUP]) < d.eps[0] / 4 and len(np.unique(d.S[0, : d.NDUP])) > d.NDUP * 0.9
    outside = 0
    for q in range(6):
        for limit, over in ((5, 4), (10, 1), (20, 2)):
            r = Q.route(d.A[q], d.eps[q], d.S[q], live, limit, over)
            assert r["R"] < len(r["W"]) <= Q.CAND_CAP and not r["fallback"]
            want = V.hit_list(d.S[q], live, limit)
            assert np.array_equal(r["hits"], want)
            outside += int(not np.isin(want, r["first"]).all())
    assert outside > 0  # some true hit was not among the first R by approx: only W has it


def test_fixture_d_mixes_fallbacks_and_certified_queries(neardup):
    d = neardup
    live = np.ones(Q.N, bool)
    for limit in (1, 5):
        fb = [Q.route(d.A[q], d.eps[q], d.S[q], live, limit, 4, cap=64)["fallback"] for q in range(len(d.q))]
        assert all(fb[:6]), fb                  # |W| >= 200 > 64
        assert fb[6]                            # the zero query: W is every live entry
        assert not any(fb[7:]), fb              # a stored unrelated entry: certified
    r = Q.route(d.A[6], d.eps[6], d.S[6], live, 5, 4, cap=64)
    assert len(r["W"]) == Q.N and not d.A[6].any()
