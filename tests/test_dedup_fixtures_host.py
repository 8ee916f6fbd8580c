"""The preconditions of test_gpu_dedup_edges.py, on the CPU oracle alone (oracle/fp_dedup.c): every builder of
dedup_fixtures.py holds the case it names -- the tie is a tie of the best score, the one-bit cases differ by one
popcount, the band-edge entries sit on the bound and are members, the zero cases score nothing -- so a builder can
never quietly turn an edge case into an ordinary one."""

import numpy as np
import pytest

import dedup_fixtures as F
import oracle as O


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def scan(case):
    return O.dedup_scan(case.cat, case.cat_dur, case.queries, case.q_dur)


def sims(case, q=0):
    return np.array([O.dedup_similarity(case.queries[q], e) for e in case.cat])


def in_band(case, q=0):
    """Membership as the oracle decides it: an entry is in the band iff a catalog of that entry alone, holding the
    query's own words, is found."""
    out = []
    for d in case.cat_dur:
        idx, _ = O.dedup_scan([case.queries[q]], [d], [case.queries[q]], [case.q_dur[q]])
        out.append(idx[0] == 0)
    return np.array(out)


def test_similarity_wrapper_known_answers():
    a = np.array([0, 0xFFFFFFFF, 0x0F0F0F0F], dtype=np.uint32)
    assert O.dedup_similarity(a, a) == 1.0
    assert O.dedup_similarity(a, ~a) == 0.0
    assert O.dedup_similarity(a, a[:0]) == 0.0
    assert O.dedup_similarity(a[:1], a) == 1.0 / 3.0  # (32 / 32) * (1 / 3)
    assert O.dedup_similarity(a, F.flip(a, [95])) == (95.0 / 96.0) * (3.0 / 3.0)


def test_builders_are_deterministic():
    for build in (lambda: F.sized(65, 2), F.length_scan, lambda: F.tie_case("far_chunks", "later"),
                  lambda: F.zero_case("complement"), lambda: F.band_case(123.456, "hi"), F.lifecycle_case):
        a, b = build(), build()
        assert all(np.array_equal(x, y) for x, y in zip(a.cat + a.queries, b.cat + b.queries))
        assert np.array_equal(bits(a.cat_dur), bits(b.cat_dur)) and np.array_equal(bits(a.q_dur), bits(b.q_dur))


# ---- sizes ----
def test_sized_cases_cover_every_chunk_and_wave():
    assert F.CATALOG_SIZES == (1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 257) and F.QUERY_COUNTS == (1, 2, 65, 300)
    c = F.sized(257, 300)
    assert len(c.cat) == 257 and len(c.queries) == 300
    lens = np.array([len(e) for e in c.cat])
    assert lens.min() >= 100 and lens.max() <= 600 and len(np.unique(lens)) > 100
    for q in (0, 1, 150, 299):  # every entry inside the band, by the oracle's own comparison
        assert in_band(c, q).all()
    lo, hi = c.q_dur.max() * 0.9, c.q_dur.min() * 1.1
    assert lo < c.cat_dur.min() and c.cat_dur.max() < hi  # ... and for every other query, with room to spare
    idx, sim = scan(c)
    assert (idx >= 0).all() and (sim > 0).all()
    assert len(set((idx // F.CHUNK).tolist())) == 5  # winners in every chunk of the 257-entry catalog
    assert len(set((idx % F.WAVES).tolist())) == F.WAVES  # ... and in every wave
    for n_cat in F.CATALOG_SIZES:  # a smaller catalog is a prefix: its winners lie inside it
        i, _ = scan(F.sized(n_cat, 65))
        assert (i >= 0).all() and i.max() < n_cat


# ---- lengths ----
def test_length_pairs_cover_the_square_and_are_isolated_in_the_scan():
    pairs = F.length_pairs()
    got = {(len(a), len(b)) for a, b in pairs}
    assert got == {(la, lb) for la in F.LENGTHS for lb in F.LENGTHS} | {(F.LONG, F.LONG)}
    assert F.LENGTHS == (0, 1, 2, 63, 64, 65, 127, 128, 129, 1000) and F.LONG == 30000 and len(pairs) == 101
    c = F.length_scan()
    idx, sim = scan(c)
    for j, (a, b) in enumerate(pairs):
        s = O.dedup_similarity(a, b)
        assert bits([s])[0] == bits(sim)[j]  # only entry j is in query j's band: the scan's score is the pair's
        assert idx[j] == (j if s > 0 else -1)
        assert (s > 0) == (len(a) > 0 and len(b) > 0)
    assert (idx >= 0).sum() == 82  # all but the 19 pairs with an empty side
    # both roles of min / max: shorter query, shorter entry, equal
    assert any(len(a) < len(b) for a, b in pairs) and any(len(a) > len(b) for a, b in pairs)


# ---- ties, near ties ----
def _wave(e):
    return e % F.CHUNK % F.WAVES


def test_placements_are_where_their_names_say():
    P = {k: v[0] for k, v in F.PLACEMENTS.items()}
    a, b = P["same_wave"]
    assert b == a + 4 and a // F.CHUNK == b // F.CHUNK and _wave(a) == _wave(b)
    a, b = P["same_wave_chunk2"]
    assert b == a + 4 and a // F.CHUNK == b // F.CHUNK == 2 and _wave(a) == _wave(b)
    a, b = P["next_wave"]
    assert b == a + 1 and a // F.CHUNK == b // F.CHUNK and _wave(b) == _wave(a) + 1
    for name in ("wrapped_wave", "wrapped_wave_chunk1"):
        a, b = P[name]
        assert b == a + 1 and a // F.CHUNK == b // F.CHUNK and _wave(b) < _wave(a)  # the later entry, a lower wave
    assert P["chunk_edge"] == (63, 64)
    a, b = P["far_chunks"]
    assert a == 5 and (b - 5) % F.CHUNK == 0 and b // F.CHUNK >= 2
    assert len({p // F.CHUNK for p in P["three_chunks"]}) == 3 and len(P["three_chunks"]) == 3
    pos, out = F.PLACEMENTS["five_first_out_of_band"]
    assert len(pos) == 5 and out == pos[0]
    assert max(max(p) for p in P.values()) < F.TIE_N_CAT


@pytest.mark.parametrize("name", list(F.PLACEMENTS))
def test_tie_is_a_tie_of_the_best_score(name):
    c = F.tie_case(name, "tie")
    s, band = sims(c), in_band(c)
    copies, inb = c.info["copies"], c.info["in_band"]
    assert len(inb) >= 2 and band[list(inb)].all()
    assert [p for p in copies if not band[p]] == [p for p in copies if p not in inb]
    best = s[band].max()
    tied = np.nonzero(band & (bits(s) == bits([best])[0]))[0]
    assert tied.tolist() == list(inb)  # two or more entries share the best score's bits, and no other entry does
    assert np.all(bits(s[list(copies)]) == bits([best])[0])  # an out-of-band copy scores the same, and is ignored
    others = np.delete(s, list(copies))
    assert others.max() < 0.6 < best
    idx, sim = scan(c)
    assert idx[0] == inb[0] and bits(sim)[0] == bits([best])[0]  # the earliest of the best


@pytest.mark.parametrize("kind", ["later", "earlier"])
@pytest.mark.parametrize("name", list(F.PLACEMENTS))
def test_near_tie_differs_by_one_bit(name, kind):
    c = F.tie_case(name, kind)
    q, inb, better = c.queries[0], c.info["in_band"], c.info["better"]
    assert better == (inb[-1] if kind == "later" else inb[0])
    diff = {p: F.popcount_diff(q, c.cat[p]) for p in c.info["copies"]}
    assert diff[better] == c.info["flips"] - 1
    assert all(diff[p] == c.info["flips"] for p in c.info["copies"] if p != better)  # exactly one popcount apart
    s = sims(c)
    assert all(s[better] > s[p] for p in inb if p != better)  # one bit is a different binary64
    idx, sim = scan(c)
    assert idx[0] == better and bits(sim)[0] == bits(s[[better]])[0]
    tie_idx, _ = scan(F.tie_case(name, "tie"))
    if kind == "later":
        assert tie_idx[0] != better  # the tie and the near tie have different answers


# ---- zero ----
@pytest.mark.parametrize("name", ["complement", "empty_query", "all_out_of_band"])
def test_zero_cases_score_nothing_in_band(name):
    c = F.zero_case(name)
    s, band = sims(c), in_band(c)
    idx, sim = scan(c)
    assert idx[0] == -1 and bits(sim)[0] == 0
    if name == "complement":
        assert band.sum() >= 100 and (s[band] == 0.0).all()
        assert (~band).sum() >= 20 and (s[~band] == 1.0).all()  # ignoring the band would find a perfect match
        assert sum(len(e) == 0 for e in c.cat) >= 20
        assert {len(e) for e, b in zip(c.cat, band) if b and len(e)} == {100, 260, 400}  # shorter, equal, longer
    elif name == "empty_query":
        # in_band() probes with the query's own words, and an empty query finds nothing: probe with a stand-in
        stand_in = F.Case(c.cat, c.cat_dur, F.sized(1, 1).queries, c.q_dur)
        assert len(c.queries[0]) == 0 and in_band(stand_in).all() and len(c.cat) > 2 * F.CHUNK
        assert min(len(e) for e in c.cat) >= 100
    else:
        assert not band.any() and s.min() > 0.99 and len(c.cat) > 2 * F.CHUNK  # only the band keeps them out


# ---- band edges ----
@pytest.mark.parametrize("edge", ["lo", "hi"])
@pytest.mark.parametrize("q_dur", F.BAND_QUERIES)
def test_band_edge_entries_sit_on_the_bound(q_dur, edge):
    c = F.band_case(q_dur, edge)
    qd = c.q_dur[0]
    bound = qd * (0.9 if edge == "lo" else 1.1)  # the product in binary64, as the reference's SELECT computes it
    assert bits([c.cat_dur[1]])[0] == bits([bound])[0]
    step = -np.inf if edge == "lo" else np.inf
    assert c.cat_dur[0] == np.nextafter(bound, step) and c.cat_dur[0] != bound
    other = qd * (1.1 if edge == "lo" else 0.9)
    assert c.cat_dur[3] == np.nextafter(other, -step)
    band = in_band(c)
    assert band.tolist() == [False, True, True, False]  # the oracle's membership: on the bound is in, a step off is out
    s = sims(c)
    assert s[0] == 1.0 and s[3] == 1.0 and 0.9 < s[1] < 1.0 and s[2] < 0.6
    idx, sim = scan(c)
    assert idx[0] == 1 and bits(sim)[0] == bits(s[[1]])[0]


def test_nan_duration_matches_nothing():
    c = F.band_case(100.0, "nan")
    assert np.isnan(c.q_dur[0])
    idx, sim = scan(c)
    assert idx[0] == -1 and bits(sim)[0] == 0
    assert sims(c)[0] == 1.0  # there is a perfect match to be had


# ---- life cycle ----
def test_lifecycle_case_has_empty_entries_at_add_edges():
    c = F.lifecycle_case()
    assert sum(F.ADD_SIZES) == len(c.cat) == 399 and F.ADD_SIZES[:5] == (1, 63, 64, 1, 200)
    empty = {e for e, x in enumerate(c.cat) if len(x) == 0}
    starts = [0] + c.info["ends"][:-1]
    whole = [k for k, (a, b) in enumerate(zip(starts, c.info["ends"])) if set(range(a, b)) <= empty]
    assert len(whole) >= 3  # adds that hold empty entries only
    assert sum(a in empty for a in starts) >= 5 and sum(b - 1 in empty for b in c.info["ends"]) >= 5
    idx, sim = scan(c)
    assert len(idx) == 300 and (idx >= 0).all()
    hit = {int(np.searchsorted(c.info["ends"], i, "right")) for i in idx}
    assert {1, 2, 4, 6} <= hit  # winners inside every add that holds words in bulk
