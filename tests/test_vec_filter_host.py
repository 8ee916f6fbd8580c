"""The filtered search's oracle on the CPU (spec/FPSPEC.md 9.2, tests/vec_filter_ref.py): known answers of `passes`
for each clause, the starvation fixture's preconditions, and the number of passing entries that every filtered case
of tests/test_gpu_vector_filter.py relies on."""

import numpy as np
import pytest
import vec_filter_ref as R
import vec_q8_ref as Q
import vec_ref as V
from test_gpu_vector import NQ, NTRACKS, Data, N
from vec_filter_ref import Filt

U64 = np.uint64


def test_passes_known_answers_for_each_clause():
    tags = np.array([0b0000, 0b0001, 0b0011, 0b0100, 0b0111, 1 << 63, (1 << 63) | 1, 0b0001], U64)
    tracks = np.array([0, 1, 2, 3, 4, 5, 6, 7], np.uint32)
    live = np.array([1, 1, 1, 1, 1, 1, 1, 0], bool)

    def p(**kw):
        return list(np.flatnonzero(R.passes(tags, tracks, live, Filt(**kw))))

    assert p() == [0, 1, 2, 3, 4, 5, 6]                    # the zero filter: the live entries, tagged or not
    assert list(np.flatnonzero(R.passes(tags, tracks, live, None))) == [0, 1, 2, 3, 4, 5, 6]
    assert np.array_equal(R.passes(tags, tracks, live, Filt()), live)
    assert p(any_of=0b0001) == [1, 2, 4, 6]                # entry 7 carries it but is dead
    assert p(any_of=0b0110) == [2, 3, 4]                   # one bit of the mask is enough
    assert p(all_of=0b0011) == [2, 4]                      # every bit of the mask
    assert p(all_of=0b0110) == [4]
    assert p(none_of=0b0001) == [0, 3, 5]
    assert p(any_of=1 << 63) == [5, 6] and p(all_of=(1 << 63) | 1) == [6]  # bit 63 is a bit like the others
    assert p(exclude=(2,)) == [0, 1, 3, 4, 5, 6]
    assert p(exclude=(2, 2, 9999, 0)) == [1, 3, 4, 5, 6]   # duplicates and an id nobody carries
    assert p(any_of=0b0111, all_of=0b0001, none_of=0b0100, exclude=(1,)) == [2, 6]
    assert p(any_of=0b1000) == [] and p(all_of=0b1001) == []
    assert R.normal(Filt(exclude=(3, 1, 3))) == R.normal(Filt(exclude=(1, 3))) != R.normal(Filt(exclude=(1,)))
    assert R.normal(None) == R.normal(Filt())


def test_bitmap_geometry():
    assert [R.allow_words(n) for n in (1, 64, 65, 289, 512, 513, 500_000)] == [8, 8, 8, 8, 8, 16, 7816]


@pytest.mark.parametrize("dim", [64, 512])
def test_starvation_fixture_preconditions(dim):
    """Post-hoc exclusion leaves the hits of at most 3 other tracks; excluding in the scan fills all 50 slots from at
    least 15 tracks (this builder's draw order gives 1 and 22 at dim 64, 2 and 17 at dim 512)."""
    s = R.Starve(dim)
    assert len(s.cat) == 47 + 30 * 6
    e_post, rows_post = s.rows(in_scan=False)
    e_scan, rows_scan = s.rows(in_scan=True)
    others_post = set(s.tracks[e_post].tolist()) - {0}
    print(dim, "post-hoc:", len(others_post), "other tracks; in scan:", len(set(s.tracks[e_scan].tolist())), "tracks")
    assert len(e_post) == 50 and np.count_nonzero(s.tracks[e_post] == 0) == 47
    assert len(others_post) <= 3 and len(rows_post) == len(others_post)
    assert len(e_scan) == 50 and 0 not in s.tracks[e_scan]
    assert len(set(s.tracks[e_scan].tolist())) >= 15 and len(rows_scan) >= 15
    assert all(r[0] != 0 for r in rows_post + rows_scan)


@pytest.fixture(scope="module")
def d512():
    return Data(512, 11)


def test_filter_kinds_cut_across_the_catalog(d512):
    d = d512
    tags = R.track_tags(d.tracks)
    live = np.ones(N, bool)
    top = [int(d.tracks[V.hit_list(d.S[q], live, 1)[0]]) for q in range(NQ)]
    for kind in R.KINDS:
        fl = R.case_filters(kind, NQ, NTRACKS, top)
        counts = [int(R.passes(tags, d.tracks, live, f).sum()) for f in fl]
        if kind in ("any_of", "none_of", "exclude1", "exclude8"):
            assert min(counts) >= 30, (kind, counts)
        if kind in ("exclude1", "exclude8"):
            assert min(counts) >= 2 * 50
        if kind == "exclude1":  # the excluded track held the best entry
            assert all(top[q] not in d.tracks[V.hit_list(d.S[q], R.passes(tags, d.tracks, live, fl[q]), 50)] for q in range(NQ))
        if kind == "all_of":  # empty, shorter than 50, and unfiltered lists in one call
            assert 0 in counts and any(0 < c < 50 for c in counts) and N in counts
        if kind == "all":
            assert len({R.normal(f) for f in fl[:64]}) == 64  # 64 distinct bitmaps in the first batch
            assert any(0 < c < 50 for c in counts) and any(c >= 100 for c in counts)
        if kind == "mixed":
            assert sum(f is None for f in fl) == 10 and len({R.normal(f) for f in fl[:64]}) > 32
    # every mask cuts across slices of 32: no chunk of 32 entries is all in or all out for the single bits
    for bit in (0, 1, 2, R.BIT_HI):
        m = R.passes(tags, d.tracks, live, Filt(any_of=1 << bit))
        per = m[: N // 32 * 32].reshape(-1, 32).sum(axis=1)
        assert (per > 0).all() and (per < 32).all(), bit


def test_edge_cases_pass_the_counts_they_claim(d512):
    d = d512
    tags = R.edge_tags(d.tracks)
    tracks = d.tracks[: R.N_EDGE]
    live = np.ones(R.N_EDGE, bool)
    assert len(tags) == R.N_EDGE == 289 and R.N_EDGE % 32 != 0
    for limit in (1, 5, 50):
        names = set()
        for name, f, want in R.edge_cases(limit):
            m = R.passes(tags, tracks, live, f)
            assert int(m.sum()) == want, (limit, name)
            names.add(name)
            if name == "first":
                assert list(np.flatnonzero(m)) == [0]
            if name == "last":
                assert list(np.flatnonzero(m)) == [R.N_EDGE - 1]
            if name == "last_word":
                assert np.flatnonzero(m).min() == 256
            if name == "one_slice":
                e = np.flatnonzero(m)
                assert e.min() // 32 == e.max() // 32 == 2 and e.min() // 64 == e.max() // 64
            if name == "limit":
                assert want == limit
            if name == "limit-1":
                assert want == limit - 1
        assert {"first", "last", "last_word", "none", "one_slice"} <= names
        if limit > 1:
            assert {"limit", "limit-1"} <= names
    # with slices of 32 and limit 5 the threshold route runs (10 slices >= 5) and "one_slice" leaves one non-empty
    # slice, fewer than limit: the limit-th largest slice maximum is the empty slices' 0
    assert -(-R.N_EDGE // 32) >= 5


def test_prefilter_route_under_a_filter_is_section_9_1_over_the_passing_entries(d512):
    """Q.route with live = passes: H is a subset of W (FPSPEC 9.1's claim for any fixed subset of the entries) and the
    hits are the filtered hit list."""
    d = d512
    c8 = Q.Catalog(d.cn)
    A, eps = c8.view(d.qn)
    tags = R.track_tags(d.tracks)
    live = np.ones(N, bool)
    top = [int(d.tracks[V.hit_list(d.S[q], live, 1)[0]]) for q in range(NQ)]
    fl = R.case_filters("all", NQ, NTRACKS, top)
    for q in range(0, NQ, 3):
        m = R.passes(tags, d.tracks, live, fl[q])
        for limit in (1, 5, 50):
            r = Q.route(A[q], eps[q], d.S[q], m, limit, 4)
            want = V.hit_list(d.S[q], m, limit)
            assert np.array_equal(r["hits"], want) and set(want) <= set(r["W"].tolist()) and m[r["W"]].all()
