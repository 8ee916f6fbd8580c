"""The K9 fixtures (tests/vec_fixtures.py) are what they claim to be, shown on the oracle alone (tests/vec_ref.py, no
GPU): each catalog reaches the geometry it is built for, the threshold route's candidate counts fall inside or
outside the cap as stated, the planted ties are one bit pattern, the top-k claims hold, and the counters the GPU tests
expect from aid_vec_stats follow from the constants of csrc/aidfp_vector.h and the oracle's score matrix."""

import numpy as np
import pytest
import vec_fixtures as F
import vec_ref as V


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def all_live(d):
    return np.ones(d.n, bool)


def routes(S, live, limit, chunk=0):
    return [b["route"] for b in F.dispatch(S, live, limit, chunk)]


def test_constants_are_the_ones_the_fixtures_were_sized_for():
    assert (F.MAX_LIMIT, F.QUERY_BATCH, F.SCAN_CHUNK) == (1024, 64, 1024)
    assert (F.MAX_SLICE, F.CAND_CAP, F.SELECT_SLICE) == (1024, 4096, 4096)


def test_score_key_is_monotone_and_maps_both_zeros_alike():
    x = np.array([-np.inf, -3.0, -1e-30, -0.0, 0.0, 1e-30, 0.5, 1.0, np.inf], np.float32)
    k = F.score_key(x).astype(np.int64)
    assert k[3] == k[4] == 0x80000000 and np.all(np.diff(np.delete(k, 3)) > 0) and k.min() > 0


@pytest.mark.parametrize("dim", [64, 512])
def test_a_default_geometry(dim):
    d = F.default_geometry(dim)
    assert (d.n, len(d.q)) == (5165, 33 if dim == 64 else 5)
    g = F.geometry(d.n, 1)
    tiles_per_wg, waves = F.SCAN_CHUNK // 32, 8
    assert (g["scan_tiles"], g["scan_wgs"], d.n - 32 * (g["scan_tiles"] - 1)) == (162, 6, 13)
    assert g["scan_tiles"] - 5 * tiles_per_wg == 2      # the last workgroup: two tiles, six waves idle
    assert tiles_per_wg // waves == 4                   # a wave of a full workgroup takes four tiles
    assert (g["msl"], g["filter_blocks"], g["first_slices"]) == (6, 3, 2)
    # growth: capacity after each add call, as vec_grow rounds it; a copy happens where rows were stored before
    cap, n, copies, caps = 0, 0, 0, []
    for m in F.ADD_CALLS_A:
        if n + m > cap:
            copies += n > 0
            assert n % 32 != 0 or n == 0
            cap = -(-max(n + m, 2 * cap) // 1024) * 1024
        n += m
        caps.append(cap)
    assert (caps, copies, n) == ([1024, 3072, 6144], 2, d.n)
    # distinct data: no two entries score alike for a query, so any mix-up of tiles, rows or workgroups shows
    assert all(len(np.unique(bits(row))) > d.n - 10 for row in d.S)


@pytest.mark.parametrize("dim", [64, 512])
def test_b_routes_and_counters_on_a(dim):
    d = F.default_geometry(dim)
    live = all_live(d)
    want = {1: ("threshold", 0), 6: ("threshold", 0), 7: ("ineligible", 2), 50: ("ineligible", 2), 1024: ("ineligible", 2)}
    for limit, (route, selects) in want.items():
        st = F.expect_stats(d.S, live, limit)
        assert routes(d.S, live, limit) == [route]
        assert st["batches_" + route] == 1 and st["slice_selects"] == selects and st["scans_mfma"] == 1
        assert sum(st[k] for k in ("batches_threshold", "batches_ineligible", "batches_overflow")) == 1
    assert F.geometry(d.n, 6)["msl"] == 6                       # msl == limit exactly
    assert F.geometry(d.n, 1024)["last_sort"] == 2048           # the second pass sorts 2 x 1024 keys
    assert F.expect_stats(d.S, live, 1)["max_candidates"] == 1  # distinct scores: the maximum alone reaches itself
    cnt = F.dispatch(d.S, live, 6)[0]["counts"]
    assert cnt.min() >= 6 and cnt.max() <= F.CAND_CAP
    if dim == 64:
        assert cnt.max() > F.SORT_ROUND  # some list takes several rounds of the sort's threads


def test_c_planted_ties_stay_inside_the_cap():
    d = F.planted_ties()
    live, copies = all_live(d), d.info["copies"]
    assert len(copies) == 700 and copies.max() < 5 * F.MAX_SLICE
    assert len(np.unique(bits(d.S[0][copies]))) == 1            # one bit pattern
    assert np.array_equal(V.hit_list(d.S[0], live, 6), copies[:6])
    assert d.S[0][copies[0]] > np.delete(d.S[0], copies).max()
    for limit in (1, 6):
        (b,) = F.dispatch(d.S, live, limit)
        assert b["route"] == "threshold"
        assert F.SORT_ROUND < b["counts"][0] <= F.CAND_CAP and b["counts"][0] >= 700
        assert limit <= b["counts"][1] and limit <= b["counts"][0]
    assert list(F.dispatch(d.S, live, 1)[0]["counts"]) == [700, 1]
    assert F.dispatch(d.S, live, 6)[0]["counts"][0] > 700       # slice 5 has no copy: its maximum is the threshold
    assert routes(d.S, live, 50) == ["ineligible"]


def test_d_overflow_under_a_strict_top():
    d = F.overflow_under_strict_top()
    live, copies, top = all_live(d), d.info["copies"], d.info["top"]
    assert len(copies) == 4200 and not (copies % 6 == 0).any() and copies.max() < 5 * F.MAX_SLICE
    assert set(copies // F.MAX_SLICE) == {0, 1, 2, 3, 4}
    s = d.S[0]
    assert len(np.unique(bits(s[copies]))) == 1
    rest = np.delete(s, np.concatenate([copies, top]))
    assert s[top].min() > s[copies[0]] > rest.max() + 0.3
    assert len(np.unique(bits(s[top]))) == 10                   # a strict order above the tie
    want = V.hit_list(s, live, 50)
    assert set(want[:10]) == set(top) and np.array_equal(want[10:], copies[:40])
    assert list(want[:10]) != sorted(want[:10])                 # and not entry order: the sort has to order them
    assert list(F.dispatch(d.S, live, 1)[0]["counts"]) == [1] and routes(d.S, live, 1) == ["threshold"]
    for limit in range(2, 7):
        (b,) = F.dispatch(d.S, live, limit)
        assert b["route"] == "overflow" and b["counts"][0] > F.CAND_CAP and b["selects"] == 2
    assert routes(d.S, live, 50) == ["ineligible"]


def test_e_dead_slices_and_short_lists():
    d = F.default_geometry(64)
    tr = F.tracks_e()
    assert sorted(set(np.array(F.SURVIVORS_E) // F.MAX_SLICE)) == [0, 1, 3, 5]
    live = ~np.isin(tr, [1, 2, 3, 4])
    assert int(live.sum()) == 1069 + 2
    for s in (2, 4):                                            # slices with no live entry: slice maximum 0
        assert not live[s * 1024 : (s + 1) * 1024].any()
    thr, cnt = F.threshold_counts(d.S, live, 6, F.MAX_SLICE)
    assert not thr.any() and (cnt == 1071).all()                # four live maxima, the sixth largest is 0
    thr3, cnt3 = F.threshold_counts(d.S, live, 3, F.MAX_SLICE)
    assert thr3.all() and (cnt3 >= 3).all() and (cnt3 < 1071).any()
    for limit, route in ((1, "threshold"), (3, "threshold"), (6, "threshold"), (7, "ineligible"), (50, "ineligible")):
        assert routes(d.S, live, limit) == [route]
    assert F.expect_stats(d.S, live, 6)["max_candidates"] == 1071
    live4 = ~np.isin(tr, [0, 1, 2, 3, 4, 5])
    assert list(np.flatnonzero(live4)) == list(F.SURVIVORS_E)
    assert routes(d.S, live4, 6) == ["threshold"] and F.expect_stats(d.S, live4, 6)["max_candidates"] == 4
    assert len(V.hit_list(d.S[0], live4, 6)) == 4               # fewer live entries than the limit on this route
    # after compaction four entries are one slice: only limit 1 is eligible
    S4 = d.S[:, live4]
    assert [routes(S4, np.ones(4, bool), limit) for limit in (1, 3)] == [["threshold"], ["ineligible"]]
    # the cheap twin
    t = F.short_list_small()
    live_t = t.tracks != 0
    assert int(live_t.sum()) == 6 and F.geometry(t.n, 10, 32)["msl"] == 10
    assert routes(t.S, live_t, 10, 32) == ["threshold"]
    assert not F.threshold_counts(t.S, live_t, 10, 32)[0].any()
    assert F.expect_stats(t.S, live_t, 10, 32)["max_candidates"] == 6


def test_f_signs():
    d = F.signs()
    live = all_live(d)
    assert d.S[0].max() < -0.9 and len(np.unique(bits(d.S[0]))) > 290
    assert (F.score_key(d.S[0]) < 0x80000000).all()             # keys below the positive half
    assert not bits(d.S[1]).any() and not bits(d.S[2]).any()    # every score +0, bit pattern 0
    assert not d.qn[1].any() and not d.qn[2].any() and d.S[3].min() > 0.9
    for limit in (1, 5, 10):                                    # chunk 32: ten slices, thresholds below 0x80000000
        thr, cnt = F.threshold_counts(d.S[:1], live, limit, 32)
        assert 0 < thr[0] < 0x80000000 and limit <= cnt[0] <= 300
        assert routes(d.S, live, limit, 32) == ["threshold"]
    assert routes(d.S, live, 50, 32) == ["ineligible"]
    assert routes(d.S, live, 1, 0) == ["threshold"] and routes(d.S, live, 5, 0) == ["ineligible"]
    assert F.expect_stats(d.S, live, 1, 0)["max_candidates"] == 300  # the zero rows: every entry ties at the maximum
    # the zero queries on (a): every entry is a candidate, the list overflows, the hits are entries 0 .. limit - 1
    a = F.default_geometry(64)
    zq = F.zero_queries(64)
    assert not V.normalize(zq).any()
    Sz = V.scores(V.normalize(zq), a.cn)
    assert not bits(Sz).any()
    (b,) = F.dispatch(Sz, all_live(a), 6)
    assert b["route"] == "overflow" and list(b["counts"]) == [a.n, a.n]
    assert np.array_equal(V.hit_list(Sz[0], all_live(a), 6), np.arange(6))


@pytest.mark.parametrize("dim", F.DIMS_G)
def test_g_small_dims(dim):
    d = F.small_dim(dim)
    assert (d.n, len(d.q)) == (70, 33) and dim % 32 == 0
    assert {32: 1, 96: 3, 1024: 32}[dim] == dim // 32           # stages of the MFMA scan's chain
    assert (32 * dim * 4 > 65536) == (dim == 1024)              # the query tile in LDS: only 1,024 asks for more than 64 KB
    assert all(len(np.unique(bits(row))) == d.n for row in d.S)
    assert routes(d.S, all_live(d), 1) == ["threshold"] and routes(d.S, all_live(d), 5) == ["ineligible"]


def groups_of(lst):
    return list(dict.fromkeys(lst[0].tolist()))


def test_h_aggregation_lists():
    L = F.agg_lists()
    for name, (t, s, o) in L.items():
        assert len(t) == len(s) == len(o) <= F.MAX_LIMIT and s.dtype == np.float32, name
        assert (np.diff(s) <= 0).all() and (t != 0xFFFFFFFF).all(), name  # descending, as FPSPEC 9 requires
    assert len(L["tracks200"][0]) == 1024 and 192 < len(groups_of(L["tracks200"])) <= 200  # four rounds of 64 groups
    assert len(groups_of(L["tracks1024"])) == 1024 and len(groups_of(L["one_track"])) == 1
    assert len(L["one_track"][0]) == 1024
    # one_track: top_k 1, 3 and 2000 give the first score, the mean of three, the mean of all
    s = L["one_track"][1].astype(np.float64)
    for top_k in (1, 3, 2000):
        (row,) = F.agg_rows("one_track", top_k, 0.0)
        acc = 0.0
        for x in s[: min(top_k, 1024)]:
            acc += x
        assert row[1] == 1024 and row[3] == acc / min(top_k, 1024)
    # tie4: the four single-hit groups of lane 5 have one final score, rank in group order, nothing else ties with them
    g = groups_of(L["tie4"])
    assert len(g) == 198 and [g[i] for i in F.TIE_GROUPS] == list(F.TIE_TRACKS)
    assert [int((L["tie4"][0] == t).sum()) for t in F.TIE_TRACKS] == [1, 1, 1, 1]
    rows = F.agg_rows("tie4", 3, 0.0)
    ids = [r[0] for r in rows]
    at = ids.index(F.TIE_TRACKS[0])
    assert ids[at : at + 4] == list(F.TIE_TRACKS) and len({r[2] for r in rows[at : at + 4]}) == 1
    assert [r[2] for r in rows].count(rows[at][2]) == 4 and at >= 1
    cut = [c for c in F.agg_cases() if c[0] == "tie_cut"][0]
    assert cut[6] == at + 2                                     # max_out cuts inside the tie
    assert [r[0] for r in F.agg_rows("tie4", 3, 0.0, None, None, cut[6])][-2:] == list(F.TIE_TRACKS[:2])
    ex = F.agg_rows("tie4", 3, 0.0, F.TIE_TRACKS[1], None, cut[6])
    assert [r[0] for r in ex][-2:] == [F.TIE_TRACKS[0], F.TIE_TRACKS[2]]
    # offsets: exactly 4, 5 and 6 distinct ones saturate at five; 0.0 and -0.0 are one
    off = {r[0]: r for r in F.agg_rows("offsets", 3, 0.05)}
    t, _, o = L["offsets"]
    assert [len(set(o[t == k].tolist())) for k in (1, 2, 3)] == [4, 5, 6]
    assert [off[k][4] for k in (1, 2, 3)] == [0.8 * 0.05, 0.05, 0.05]
    assert np.signbit(o[t == 4]).tolist() == [False, True, False] and off[4][4] == min(2 / 5.0, 1.0) * 0.05
    # the threshold cases: equal to a row's final keeps it, the next double drops it and nothing else
    kept = [c for c in F.agg_cases() if c[0] == "threshold_kept"][0]
    dropped = [c for c in F.agg_cases() if c[0] == "threshold_dropped"][0]
    a = F.agg_rows("tracks200", 3, 0.05, None, kept[5])
    b = F.agg_rows("tracks200", 3, 0.05, None, dropped[5])
    assert a[-1][2] == kept[5] and len(b) == len(a) - 1 and 0 < len(b)
    # every call mixes lists with empty ones, and max_out 10 cuts a list of 1,024 rows
    assert all("empty" in c[1] and len(c[1]) == len(c[4]) for c in F.agg_cases())
    assert len(F.agg_rows("tracks1024", 3, 0.05, None, None, 10)) == 10 and len(F.agg_rows("tracks1024", 3, 0.05)) == 1024


def test_h_lane_at_limit_1024_has_230_tracks():
    d = F.default_geometry(64)
    assert len(np.unique(d.tracks)) == F.N_TRACKS_A == 230
    e = V.hit_list(d.S[0], all_live(d), 1024)
    assert len(e) == 1024 and len(np.unique(d.tracks[e])) > 192  # more than three rounds of 64 groups
