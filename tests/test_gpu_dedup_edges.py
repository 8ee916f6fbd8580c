"""K7 `dedup_scan` / `dedup_pairs` (csrc/dedup.hip) on constructed catalogs (dedup_fixtures.py; their preconditions:
test_dedup_fixtures_host.py) against the CPU oracle (oracle/fp_dedup.c, which tests/test_dedup_glue.py pins to the
reference's vectors): the cross-wave merge, the cross-chunk strict >, partly filled chunks, every fingerprint length
around the wave stride, ties, one-bit near ties, the duration band's bounds and the catalog's life cycle. Every
comparison is equality: best_idx as int64, best_sim as uint64 bit patterns. The C ABI is driven as aidfp/dedup.py
drives it; entry indices, not ids, are compared."""

import ctypes

import numpy as np
import pytest

import dedup_fixtures as F
import oracle as O
from aidfp._lib import check
from aidfp.dedup import _p, _packed

pytestmark = pytest.mark.gpu


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


class Catalog:
    """aid_dedup_reset / _add / _scan on the session's engine, on word arrays."""

    def __init__(self, eng):
        self.lib, self.h = eng._lib, eng._h
        check(self.lib.aid_dedup_reset(self.h))

    def reset(self):
        check(self.lib.aid_dedup_reset(self.h))

    def add(self, arrs, durs):
        words, off = _packed(list(arrs))
        dur = np.ascontiguousarray(durs, dtype=np.float64)
        assert len(dur) == len(arrs)
        check(self.lib.aid_dedup_add(self.h, _p(words), _p(off), _p(dur), len(arrs)))

    def count(self):
        n, nw = ctypes.c_int64(), ctypes.c_int64()
        check(self.lib.aid_dedup_count(self.h, ctypes.byref(n), ctypes.byref(nw)))
        return n.value, nw.value

    def scan(self, queries, q_dur):
        words, off = _packed(list(queries))
        dur = np.ascontiguousarray(q_dur, dtype=np.float64)
        nq = len(queries)
        idx = np.full(nq, -7, dtype=np.int64)
        sim = np.full(nq, -7.0, dtype=np.float64)
        check(self.lib.aid_dedup_scan(self.h, _p(words), _p(off), _p(dur), nq, _p(idx), _p(sim)))
        return idx, sim


def loaded(eng, case) -> Catalog:
    cat = Catalog(eng)
    cat.add(case.cat, case.cat_dur)
    assert cat.count() == (len(case.cat), sum(len(e) for e in case.cat))
    return cat


def assert_scan_equals_oracle(eng, case):
    want_idx, want_sim = O.dedup_scan(case.cat, case.cat_dur, case.queries, case.q_dur)
    idx, sim = loaded(eng, case).scan(case.queries, case.q_dur)
    bad = np.nonzero((idx != want_idx) | (bits(sim) != bits(want_sim)))[0]
    assert len(bad) == 0, (case.info, bad[:5], idx[bad[:5]], want_idx[bad[:5]], sim[bad[:5]], want_sim[bad[:5]])
    return idx, sim


# ---- catalog sizes x query counts: partly filled chunks, several chunks, several workgroups per chunk ----
@pytest.mark.parametrize("nq", F.QUERY_COUNTS)
@pytest.mark.parametrize("n_cat", F.CATALOG_SIZES)
def test_sizes(gpu_engine, n_cat, nq):
    idx, _ = assert_scan_equals_oracle(gpu_engine, F.sized(n_cat, nq))
    assert (idx >= 0).all() and idx.max() < n_cat


# ---- fingerprint lengths: the wave loop strides by 64; min / max swap roles at la = lb ----
def test_lengths_pairs(gpu_engine):
    pairs = F.length_pairs()
    aw, ao = _packed([a for a, _ in pairs])
    bw, bo = _packed([b for _, b in pairs])
    got = np.full(len(pairs), -7.0)
    check(gpu_engine._lib.aid_dedup_pairs(gpu_engine._h, _p(aw), _p(ao), _p(bw), _p(bo), len(pairs), _p(got)))
    want = np.array([O.dedup_similarity(a, b) for a, b in pairs])
    bad = np.nonzero(bits(got) != bits(want))[0]
    assert len(bad) == 0, [(len(pairs[k][0]), len(pairs[k][1]), got[k], want[k]) for k in bad[:5]]
    assert (want > 0).sum() == 82 and want[-1] > 0.99  # not vacuous; the last pair is the 30,000-word one


def test_lengths_scan(gpu_engine):
    idx, _ = assert_scan_equals_oracle(gpu_engine, F.length_scan())
    assert (idx >= 0).sum() == 82


# ---- ties: the earliest of the best wins; near ties: the best wins wherever it stands ----
@pytest.mark.parametrize("kind", ["tie", "later", "earlier"])
@pytest.mark.parametrize("name", list(F.PLACEMENTS))
def test_ties_and_near_ties(gpu_engine, name, kind):
    case = F.tie_case(name, kind)
    idx, _ = assert_scan_equals_oracle(gpu_engine, case)
    want = case.info["in_band"][0] if kind == "tie" else case.info["better"]
    assert idx[0] == want  # what test_dedup_fixtures_host.py shows the oracle to answer


def test_ties_in_one_batch(gpu_engine):
    """The 27 tie and near-tie queries as one batch (27 workgroups per chunk) against the catalogs of several cases:
    one query meets its tie there, the others an ordinary catalog."""
    cases = [F.tie_case(n, k) for n in F.PLACEMENTS for k in ("tie", "later", "earlier")]
    queries = [c.queries[0] for c in cases]
    q_dur = np.full(len(queries), 100.0)
    for c in cases[::4]:
        assert_scan_equals_oracle(gpu_engine, F.Case(c.cat, c.cat_dur, queries, q_dur, c.info))


# ---- nothing scores above 0.0 ----
@pytest.mark.parametrize("name", ["complement", "empty_query", "all_out_of_band"])
def test_nothing_scores(gpu_engine, name):
    idx, sim = assert_scan_equals_oracle(gpu_engine, F.zero_case(name))
    assert idx[0] == -1 and bits(sim)[0] == 0


# ---- duration band edges ----
@pytest.mark.parametrize("edge", ["lo", "hi", "nan"])
def test_band_edges(gpu_engine, edge):
    for q_dur in F.BAND_QUERIES:
        idx, _ = assert_scan_equals_oracle(gpu_engine, F.band_case(q_dur, edge))
        assert idx[0] == (-1 if edge == "nan" else 1), q_dur


def test_band_edges_in_one_catalog(gpu_engine):
    """All the band cases' entries in one catalog and their queries in one batch: an entry on one query's bound is
    an ordinary member, or no member, of another's."""
    cases = [F.band_case(q, e) for q in F.BAND_QUERIES for e in ("lo", "hi", "nan")]
    merged = F.Case([e for c in cases for e in c.cat], np.concatenate([c.cat_dur for c in cases]),
                    [c.queries[0] for c in cases], np.concatenate([c.q_dur for c in cases]), {"merged": len(cases)})
    assert_scan_equals_oracle(gpu_engine, merged)


# ---- catalog life cycle ----
def test_adds_in_pieces_equal_one_add(gpu_engine):
    case = F.lifecycle_case()
    want_idx, want_sim = O.dedup_scan(case.cat, case.cat_dur, case.queries, case.q_dur)
    one_idx, one_sim = loaded(gpu_engine, case).scan(case.queries, case.q_dur)
    cat = Catalog(gpu_engine)
    at = 0
    for k in F.ADD_SIZES:
        cat.add(case.cat[at:at + k], case.cat_dur[at:at + k])
        at += k
    assert at == len(case.cat) and cat.count() == (len(case.cat), sum(len(e) for e in case.cat))
    idx, sim = cat.scan(case.queries, case.q_dur)
    assert np.array_equal(idx, one_idx) and np.array_equal(bits(sim), bits(one_sim))
    assert np.array_equal(idx, want_idx) and np.array_equal(bits(sim), bits(want_sim))
    # a growing catalog: after every add the scan equals the oracle on the entries so far
    cat.reset()
    at = 0
    for k in F.ADD_SIZES:
        cat.add(case.cat[at:at + k], case.cat_dur[at:at + k])
        at += k
        w_idx, w_sim = O.dedup_scan(case.cat[:at], case.cat_dur[:at], case.queries[:40], case.q_dur[:40])
        idx, sim = cat.scan(case.queries[:40], case.q_dur[:40])
        assert np.array_equal(idx, w_idx) and np.array_equal(bits(sim), bits(w_sim)), at


def test_reset_empties_the_catalog(gpu_engine):
    case = F.sized(129, 65)
    cat = loaded(gpu_engine, case)
    idx, _ = cat.scan(case.queries, case.q_dur)
    assert (idx >= 0).all()
    cat.reset()
    assert cat.count() == (0, 0)
    idx, sim = cat.scan(case.queries, case.q_dur)
    assert (idx == -1).all() and (bits(sim) == 0).all()
    cat.add(case.cat[:5], case.cat_dur[:5])  # and it fills again from entry 0
    w_idx, w_sim = O.dedup_scan(case.cat[:5], case.cat_dur[:5], case.queries, case.q_dur)
    idx, sim = cat.scan(case.queries, case.q_dur)
    assert np.array_equal(idx, w_idx) and np.array_equal(bits(sim), bits(w_sim))


def test_no_queries_writes_nothing(gpu_engine):
    case = F.sized(65, 1)
    cat = loaded(gpu_engine, case)
    words, off = _packed([])
    dur = np.zeros(1, dtype=np.float64)
    idx = np.full(4, -7, dtype=np.int64)
    sim = np.full(4, -7.0, dtype=np.float64)
    check(cat.lib.aid_dedup_scan(cat.h, _p(words), _p(off), _p(dur), 0, _p(idx), _p(sim)))
    assert (idx == -7).all() and (sim == -7.0).all()
    sims = np.full(4, -7.0, dtype=np.float64)
    check(cat.lib.aid_dedup_pairs(cat.h, _p(words), _p(off), _p(words), _p(off), 0, _p(sims)))
    assert (sims == -7.0).all()


def test_batch_equals_single_scans(gpu_engine):
    case = F.sized(257, 300)
    want_idx, want_sim = O.dedup_scan(case.cat, case.cat_dur, case.queries, case.q_dur)
    cat = loaded(gpu_engine, case)
    idx, sim = cat.scan(case.queries, case.q_dur)
    assert np.array_equal(idx, want_idx) and np.array_equal(bits(sim), bits(want_sim))
    for q in range(len(case.queries)):
        i1, s1 = cat.scan(case.queries[q:q + 1], case.q_dur[q:q + 1])
        assert i1[0] == idx[q] and bits(s1)[0] == bits(sim)[q], q
