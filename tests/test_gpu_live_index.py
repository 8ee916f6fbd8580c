"""The live index (aid_index_live; DESIGN 4b "Live ingest"): a store no longer makes the next query rebuild the whole
CSR. The built CSR stays as the main segment, postings stored since go into a small delta CSR, every query votes over
both and its rows are merged, and a delta past its cap is folded into main.

The reference everywhere is a SECOND ENGINE that got the same postings in the same order and was built once, with the
feature off; where the queries are host records, also the CPU oracle (oracle/fp_match.c, FPSPEC 7) on the exported
postings. Nothing is compared with another path of the engine under test. The expected build counts follow from the
policy of csrc/aidfp_live_plan.h as include/aidfp.h words it (tail 0: nothing; tail <= cap: the delta alone; tail >
cap: a fold; an append with an older track id, compact, reset, load: the full build), restated beside each
assertion."""

import numpy as np
import pytest

import k5_fixtures as F
import oracle as O
from aidfp import synth
from aidfp._lib import AID_ERR_STATE, EngineError
from aidfp.engine import Engine
from store_ref import csr_mirror  # the CSR K4 must build: live postings stably sorted by bucket key

pytestmark = pytest.mark.gpu
SR = 16000
N_MAIN, N_NEW = 24, 8
UNSEEN = 77
REASONS = ("fallback_heavy", "fallback_table", "fallback_distinct", "fallback_tracks", "fallback_rows")


def add(eng, post):
    h, tr, t = F.columns(post)
    eng.index_add_postings(h.ctypes.data, tr.ctypes.data, t.ctypes.data, len(post), device=False)


def same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (i, g[:4], w[:4])


def oracle_rows(eng, rec):
    return O.query(eng.index_export(), rec, min_match=eng.min_match, max_rows=eng.max_results)


# ---------------------------------------------------------------- synthetic audio, extracted once
@pytest.fixture(scope="module")
def audio():
    """Records of tracks 0 .. 31 (12 s each at 16 kHz) and seven 4 s query clips with noise: from tracks of the first
    24 (main), of the last 8 (stored while live) and from a track the index never sees."""
    with Engine(SR) as eng:
        recs = eng.extract_host([synth.synth(t, 0, 12 * SR, SR) for t in range(N_MAIN + N_NEW)])
    src = [3, 17, 23, 24, 29, 31, UNSEEN]
    clips = [synth.synth(t, SR * (1 + i) + 13 * i, 4 * SR + 5 * i, SR, snr_db=20, salt=i) for i, t in enumerate(src)]
    assert all(len(r) > 500 for r in recs)
    return recs, clips, src


def store(eng, recs, tracks):
    for t in tracks:
        eng.index_add_records(t, recs[t])


def all_paths(eng, clips):
    """The clips through query_pcm, query (host records) and query_windows (device PCM, windows in place)."""
    import torch

    a = eng.query_pcm(clips)
    b = eng.query(eng.extract_host(clips))
    flat = np.concatenate(clips)
    dev = torch.from_numpy(flat).cuda()
    off = np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64)
    c = eng.query_windows(dev.data_ptr(), off[:-1], off[1:])
    return a, b, c


# ---------------------------------------------------------------- 1. rows equal a single build on every path
@pytest.mark.parametrize("path", [0, 2])
def test_rows_equal_single_build(audio, path):
    recs, clips, src = audio
    with Engine(SR, min_match=5) as live, Engine(SR, min_match=5) as one:
        live.force("k5_path", path)
        one.force("k5_path", path)
        store(live, recs, range(N_MAIN))
        live.index_finalize()
        live.index_live(1 << 20)
        for t in range(N_MAIN, N_MAIN + N_NEW):  # store + query cycles: each rebuilds the delta alone
            store(live, recs, [t])
            rows = live.query_pcm(clips[:4])
            assert rows[0][0][1] == src[0]
            if t >= src[3]:
                assert rows[3][0][1] == src[3]  # a track stored while live answers at once
        st = live.index_live_stats()
        n_main = sum(len(r) for r in recs[:N_MAIN])
        n_new = sum(len(r) for r in recs[N_MAIN:])
        # one main build (the finalize) across eight store + query cycles, one delta build per cycle, nothing folded
        assert (st["main_builds"], st["delta_builds"], st["folds"]) == (1, N_NEW, 0), st
        assert (st["main_postings"], st["delta_postings"], st["tracks_at_main"]) == (n_main, n_new, N_MAIN), st
        assert not any(st["fallbacks"].values()), st
        assert live.index_stats()["live"] == n_main + n_new
        store(one, recs, range(N_MAIN + N_NEW))
        one.index_finalize()
        assert np.array_equal(live.index_export(), one.index_export())
        got, want = all_paths(live, clips), all_paths(one, clips)
        for g, w in zip(got, want):
            same(g, w)
        for i, t in enumerate(src[:-1]):
            assert want[0][i][0][1] == t and want[0][i][0][0] >= 20, (i, want[0][i][:2])  # the clips do match
        host_recs = one.extract_host(clips)
        for g, r in zip(got[1], host_recs):
            assert np.array_equal(g, oracle_rows(one, r))
        assert live.index_live_stats()["main_builds"] == 1
        with pytest.raises(EngineError) as ei:  # postings sit in the delta: no single CSR to export
            live.index_csr(offsets=False)
        assert ei.value.code == AID_ERR_STATE and "delta" in str(ei.value)


# ---------------------------------------------------------------- 2. merge edges, constructed
MR = 4


def counted(counts, ids, hbase, n_rec=16, d0=20):
    """Postings of tracks `ids`, track j sharing the query's first counts[j] records at its own offset: rows
    (counts[j], ids[j], d0 + 7 j, 4, 4 + 3 (counts[j] - 1)). The query: n_rec records on hashes hbase .."""
    tq = 4 + 3 * np.arange(n_rec)
    h = F.hashes(hbase, n_rec)
    parts = [F._postings(h[:c], t, tq[:c] + d0 + 7 * j) for j, (c, t) in enumerate(zip(counts, ids))]
    return (np.concatenate(parts) if parts else np.zeros((0, 3), F.U32)), F.records(h, tq)


def merge_fixture():
    """(main postings, delta postings, queries, min_match): every merge edge in one index, hashes disjoint per case.
    Main holds track ids below 3000, the delta ids from 3000 on."""
    main, delta, queries = [], [], {}

    def case(name, m, d, rec):
        main.extend(m)
        delta.extend(d)
        queries[name] = rec

    a, ra = counted([12, 10, 8, 6], [0, 1, 2, 3], 0)
    b, _ = counted([11, 9, 7, 5], [3000, 3001, 3002, 3003], 0, d0=90)
    case("interleaved", [a], [b], ra)  # 12 11 10 9 of 8 rows
    a, ra = counted([9, 9, 9], [10, 15, 12], 100)
    b, _ = counted([9, 9, 9], [3012, 3010, 3011], 100, d0=90)
    case("equal_counts", [a], [b], ra)  # 10 12 15 then the delta's smallest id
    a, ra = counted([9, 7], [20, 21], 200)
    case("delta_empty", [a], [], ra)
    b, rb = counted([9, 7, 6, 5, 5], [3020, 3021, 3022, 3023, 3024], 300)
    case("main_empty", [], [b], rb)
    _, rn = counted([], [], 400)
    case("both_empty", [], [], rn)
    a, ra = counted([4, 3], [30, 31], 500)  # below min_match 5 in main, a row in the delta
    b, _ = counted([6], [3030], 500, d0=90)
    case("below_min_match", [a], [b], ra)
    # hand-backs: 2,100 distinct frames of one (track, d) overflow the LDS path's distinct set (kFastDistinctCap 2048)
    run_m, rec_m, _ = F.long_run(2100, track=40, hbase=10000)
    run_d, rec_d, _ = F.long_run(2100, track=3040, d=31, hbase=20000)
    case("handback_main", [run_m], [], rec_m)
    case("handback_delta", [], [run_d], rec_d)
    queries["handback_both"] = np.concatenate([rec_m, rec_d])
    return np.concatenate(main), np.concatenate(delta), queries, 5


@pytest.fixture(scope="module", params=[0, 1], ids=["host_merge", "device_merge"])
def merge_engines(request):
    """(live engine: main + delta, reference engine: one build, queries). Device merge: the host-row calls merge with
    k_rows_merge, as the exact lane always does."""
    main, delta, queries, mm = merge_fixture()
    with Engine(SR, min_match=mm, max_results=MR) as live, Engine(SR, min_match=mm, max_results=MR) as one:
        add(live, main)
        live.index_finalize()
        live.index_live(1 << 20)
        add(live, delta)
        live.force("rows_merge", request.param)
        add(one, main)
        add(one, delta)
        one.index_finalize()
        yield live, one, queries


@pytest.mark.parametrize("path", [0, 2])
def test_merge_edges(merge_engines, path):
    live, one, queries = merge_engines
    live.force("k5_path", path)
    one.force("k5_path", path)
    names = list(queries)
    post = one.index_export()
    want = {k: O.query(post, queries[k], min_match=5, max_rows=MR) for k in names}
    # what the fixture is for
    assert want["interleaved"][:, :2].tolist() == [[12, 0], [11, 3000], [10, 1], [9, 3001]]
    assert want["equal_counts"][:, :2].tolist() == [[9, 10], [9, 12], [9, 15], [9, 3010]]
    assert want["delta_empty"][:, :2].tolist() == [[9, 20], [7, 21]]
    assert want["main_empty"][:, :2].tolist() == [[9, 3020], [7, 3021], [6, 3022], [5, 3023]]
    assert len(want["both_empty"]) == 0
    assert want["below_min_match"][:, :2].tolist() == [[6, 3030]]
    assert want["handback_both"][:, :2].tolist() == [[2100, 40], [2100, 3040]]
    for k in names:  # one query per call
        live.match_stats(reset=True)
        got = live.query([queries[k]])[0]
        st = live.match_stats()
        assert np.array_equal(got, want[k]), (k, got, want[k])
        assert np.array_equal(one.query([queries[k]])[0], want[k]), k
        assert st["queries"] == 1, st  # counted once, over two passes
        if path == 0:
            n_hb = {"handback_main": 1, "handback_delta": 1, "handback_both": 2}.get(k, 0)
            assert st["fallback_distinct"] == n_hb and sum(st[r] for r in REASONS) == n_hb, (k, st)
            assert st["queries_lds"] == 2 and st["queries_global"] == n_hb, (k, st)
    # more queries than one merge workgroup covers (4), a count that is no multiple of it, every case mixed
    batch = [names[i % len(names)] for i in range(3 * len(names) - 1)]
    got = live.query([queries[k] for k in batch])
    for k, g in zip(batch, got):
        assert np.array_equal(g, want[k]), k
    live.force("k5_path", 0)
    one.force("k5_path", 0)


def test_merge_lists_longer_than_the_lds_staging():
    """max_results 300 is above the 256 rows per list k_rows_merge stages in LDS: it merges in global memory."""
    a, ra = counted([15 - (j % 9) for j in range(280)], list(range(280)), 0)
    b, _ = counted([14 - (j % 8) for j in range(150)], [1000 + j for j in range(150)], 0, d0=2500)
    for dev in (0, 1):
        with Engine(SR, min_match=5, max_results=300) as live:
            add(live, a)
            live.index_finalize()
            live.index_live(1 << 20)
            add(live, b)
            live.force("rows_merge", dev)
            got = live.query([ra, ra[:7], ra])
            want = O.query(np.concatenate([a, b]), ra, min_match=5, max_rows=300)
            assert len(want) == 300 and len(set(want[:, 1].tolist()) & set(range(1000, 1150))) > 50
            assert np.array_equal(got[0], want) and np.array_equal(got[2], want)
            assert np.array_equal(got[1], O.query(np.concatenate([a, b]), ra[:7], min_match=5, max_rows=300))


# ---------------------------------------------------------------- 3. the disjointness rule
def test_old_track_id_falls_back_to_the_full_build():
    a, ra, mm = F.tracks(10, 5)
    extra, rx, _ = F.long_run(20, track=3, hbase=5000)  # more postings for a track main already holds
    new, rn, _ = F.long_run(20, track=10, hbase=6000)
    with Engine(SR, min_match=mm) as live, Engine(SR, min_match=mm) as one:
        add(live, a)
        live.index_finalize()
        live.index_live(1 << 20)
        add(live, new)  # id 10 = the track count at main's build: kept
        assert np.array_equal(live.query([rn])[0], [[20, 10, 17, 0, 19]])
        st = live.index_live_stats()
        assert (st["main_builds"], st["delta_builds"], st["fallbacks"]["old_track"]) == (1, 1, 0), st
        add(live, extra)  # id 3 < 10: no delta can hold it
        for p in (a, new, extra):
            add(one, p)
        one.index_finalize()
        qs = [ra, rx, rn, np.concatenate([ra, rx])]
        same(live.query(qs), one.query(qs))
        same(live.query(qs), [oracle_rows(one, q) for q in qs])
        st = live.index_live_stats()
        assert (st["main_builds"], st["delta_builds"], st["folds"]) == (2, 1, 0), st
        assert st["fallbacks"]["old_track"] == 1 and st["delta_postings"] == 0, st
        assert st["main_postings"] == len(a) + len(new) + len(extra)


# ---------------------------------------------------------------- 4. removal while live
def test_removal_while_live():
    a, ra, mm = F.tracks(6, 5)
    b, _, _ = F.tracks(6, 5, seed=1, tbase=100)  # the same query's records, other tracks
    c, _, _ = F.tracks(3, 5, seed=2, tbase=200)
    with Engine(SR, min_match=mm) as live, Engine(SR, min_match=mm) as one:
        add(live, a)
        live.index_finalize()
        live.index_live(len(b) + len(c))  # the third store stays within the cap, a fourth would not
        add(live, b)
        assert len(live.query([ra])[0]) == 12
        live.index_remove(2)    # of main
        live.index_remove(103)  # of the delta
        add(one, a)
        add(one, b)
        one.index_remove(2)
        one.index_remove(103)
        one.index_finalize()
        got = live.query([ra])[0]
        kept = one.index_export()
        kept = kept[~np.isin(kept[:, 1], [2, 103])]
        assert np.array_equal(got, one.query([ra])[0])
        assert np.array_equal(got, O.query(kept, ra, min_match=mm, max_rows=one.max_results))
        assert sorted(got[:, 1].tolist()) == [0, 1, 3, 4, 5, 100, 101, 102, 104, 105]
        add(live, c)  # a delta rebuild: it drops track 103's postings, main still holds track 2's
        add(one, c)
        one.index_finalize()
        got = live.query([ra])[0]
        assert np.array_equal(got, one.query([ra])[0])
        assert sorted(got[:, 1].tolist()) == [0, 1, 3, 4, 5, 100, 101, 102, 104, 105, 200, 201, 202]
        st = live.index_live_stats()
        assert (st["main_builds"], st["delta_builds"], st["folds"]) == (1, 2, 0), st
        d, _, _ = F.tracks(1, 5, seed=3, tbase=300)
        add(live, d)  # tail = cap + 5: a fold
        add(one, d)
        one.index_finalize()
        got = live.query([ra])[0]
        assert np.array_equal(got, one.query([ra])[0])
        assert sorted(got[:, 1].tolist()) == [0, 1, 3, 4, 5, 100, 101, 102, 104, 105, 200, 201, 202, 300]
        st = live.index_live_stats()
        # (a fold first builds the delta over the whole tail, then merges: no build of main)
        assert (st["main_builds"], st["delta_builds"], st["folds"], st["delta_postings"]) == (1, 3, 1, 0), st
        # the fold carried track 2's postings along (only a full build drops them); the rows above skip them, and an
        # explicit finalize with nothing stored since runs the full build, as ever
        live.index_finalize()
        assert live.index_live_stats()["main_builds"] == 2
        _, pl = live.index_csr(offsets=False)
        _, po = one.index_csr(offsets=False)
        assert np.array_equal(pl, po)


# ---------------------------------------------------------------- 5. cap and fold
def test_cap_and_fold(audio):
    recs, clips, src = audio
    cap = 3000
    with Engine(SR, min_match=5) as live, Engine(SR, min_match=5) as one:
        store(live, recs, range(4))
        live.index_finalize()
        live.index_live(cap)
        tail = folds = deltas = 0
        for t in range(4, 16):  # one track at a time, a query between
            store(live, recs, [t])
            rows = live.query_pcm(clips[:1])[0]
            assert rows[0][1] == src[0]
            tail += len(recs[t])
            deltas += 1  # the delta is built over the tail either way
            if tail > cap:  # the policy: past the cap it is folded into main (K4m: no build of main)
                folds, tail = folds + 1, 0
            st = live.index_live_stats()
            assert (st["main_builds"], st["delta_builds"], st["folds"], st["delta_postings"]) == \
                (1, deltas, folds, tail), (t, st)
        assert folds >= 2 and deltas - folds >= 2, (folds, deltas, [len(r) for r in recs[4:16]])
        store(one, recs, range(16))
        one.index_finalize()
        same(live.query_pcm(clips), one.query_pcm(clips))
        before = live.index_live_stats()
        live.index_finalize()  # one CSR over everything: a last fold, or with nothing stored since the full build, as ever
        after = live.index_live_stats()
        pending = 1 if before["delta_postings"] else 0
        assert after["delta_postings"] == 0
        assert (after["folds"], after["main_builds"]) == (before["folds"] + pending, 1 + (1 - pending)), (before, after)
        offs, posts = live.index_csr()
        ref_offs, ref_posts = csr_mirror(one.index_export())
        assert np.array_equal(posts, ref_posts) and np.array_equal(offs, ref_offs)
        o1, p1 = one.index_csr()
        assert np.array_equal(posts, p1) and np.array_equal(offs, o1)


# ---------------------------------------------------------------- 7. tickets
HB_TRACKS = 900  # per segment: at min_match 1 every bucket is hot, and windows of 9 s over this many 30 s tracks
#                  find more candidate tracks than the LDS path's tables hold (256), while the single build over both
#                  stays below the global path's documented limit of 1024 candidate tracks (a 9 s window finds
#                  about 0.43 candidate tracks per indexed track)


def ingest(eng, tracks, seconds=30):
    """Synthetic tracks generated, extracted and appended on the device (aid_index_add_extracted), 240 per batch."""
    import torch

    n = seconds * SR
    pcm = torch.empty(240 * n, dtype=torch.float32, device="cuda")
    for b0 in range(0, len(tracks), 240):
        tr = np.ascontiguousarray(tracks[b0:b0 + 240], dtype=np.uint32)
        eng.synth(pcm.data_ptr(), tr, np.zeros(len(tr), np.int64), n)
        eng.extract_device(pcm.data_ptr(), np.arange(len(tr) + 1, dtype=np.int64) * n)
        eng.index_add_extracted(tr)
    eng.sync()


@pytest.fixture(scope="module")
def handback_pair():
    """(live engine with 900 tracks in main and 900 in the delta, reference engine built once over the 1800, device
    PCM of four 20 s clips, window starts and ends, hand-backs of the five windows over main alone)."""
    import torch

    with Engine(SR, min_match=1) as live, Engine(SR, min_match=1) as one:
        n = 20 * SR
        pcm = torch.empty(4 * n, dtype=torch.float32, device="cuda")
        live.synth(pcm.data_ptr(), np.array([3, 77, 1000, 1799], np.uint32), np.zeros(4, np.int64), n,
                   noise_a=synth.noise_halfwidth(20.0), salt=5)
        torch.cuda.synchronize()
        st = np.array([0, 7 * SR, n + 3 * SR, 2 * n + 11, 3 * n + 5 * SR], np.int64)
        en = st + 9 * SR
        ingest(live, np.arange(HB_TRACKS))
        live.index_finalize()
        live.index_live(1 << 26)
        live.match_stats(reset=True)
        live.query_windows(pcm.data_ptr(), st, en)  # one pass: main alone
        ms = live.match_stats(reset=True)
        hb_main = sum(ms[r] for r in REASONS)
        ingest(live, np.arange(HB_TRACKS, 2 * HB_TRACKS))
        ingest(one, np.arange(HB_TRACKS))
        ingest(one, np.arange(HB_TRACKS, 2 * HB_TRACKS))
        one.index_finalize()
        yield live, one, pcm, st, en, hb_main


def test_tickets_over_two_segments(handback_pair):
    """Two tickets submitted with a live delta, a store + query between submit and collect (it rebuilds the delta, which
    the tickets hold), collected in reverse order, with queries that hand back in each segment. Rows equal the
    synchronous call's before the store, the reference engine's and the oracle's."""
    live, one, pcm, st, en, hb_main = handback_pair
    live.match_stats(reset=True)
    want = live.query_windows(pcm.data_ptr(), st, en)
    ms = live.match_stats(reset=True)
    hb_two = sum(ms[r] for r in REASONS)
    print("hand-backs: main alone", hb_main, "main + delta", hb_two, ms)
    # main's pass is the same with or without a delta: what two passes hand back beyond it is the delta's
    assert ms["queries"] == len(st) and hb_main >= 1 and hb_two - hb_main >= 1, (hb_main, hb_two, ms)
    same(want, one.query_windows(pcm.data_ptr(), st, en))
    post = one.index_export()
    host = pcm.cpu().numpy()
    for k in (1, 3):  # a window of a main track, one of a delta track
        assert np.array_equal(want[k], O.query(post, O.fingerprint(host[st[k]:en[k]], 256), min_match=1,
                                               max_rows=one.max_results)), k
    clips = [host[st[k]:en[k]] for k in range(3, 5)]
    before = live.index_live_stats()
    a = live.query_windows_submit(pcm.data_ptr(), st[:3], en[:3])
    b = live.query_pcm_submit(clips)
    new = 2 * HB_TRACKS + 5
    live.index_add_records(new, live.extract_host([synth.synth(new, 0, 10 * SR, SR)])[0])  # a store ...
    mid = live.query_pcm([synth.synth(new, SR, 5 * SR, SR, snr_db=20)])[0]  # ... and a query: the delta is rebuilt
    assert mid[0][1] == new
    gb, ga = b.collect(), a.collect()
    ms = live.match_stats()
    same(ga + gb, want)
    assert sum(ms[r] for r in REASONS) >= hb_two, ms  # collect answered the same hand-backs
    after = live.index_live_stats()
    assert after["main_builds"] == before["main_builds"] and after["folds"] == before["folds"]
    assert after["delta_builds"] == before["delta_builds"] + 1


def test_ticket_collected_after_a_fold(handback_pair):
    """A fold between submit and collect replaces both segments; the ticket still answers from the ones it holds."""
    live, one, pcm, st, en, _ = handback_pair
    n_live, n_one = live.index_stats()["postings"], one.index_stats()["postings"]
    if n_live > n_one:  # what the test above stored, if it ran: the reference gets the same postings
        add(one, live.index_export(n_one, n_live - n_one))
        one.index_finalize()
    want = one.query_windows(pcm.data_ptr(), st, en)
    t = live.query_windows_submit(pcm.data_ptr(), st, en)
    before = live.index_live_stats()
    assert before["delta_postings"] > 0
    live.index_live(1 << 20)  # a change while a delta is live folds first
    after = live.index_live_stats()
    assert (after["folds"], after["main_builds"], after["delta_postings"]) == \
        (before["folds"] + 1, before["main_builds"], 0), (before, after)
    same(t.collect(), want)
    same(live.query_windows(pcm.data_ptr(), st, en), want)


# ---------------------------------------------------------------- 8. the lane
def test_exact_lane_and_speed_lane(audio):
    recs, clips, src = audio
    with Engine(SR, min_match=5) as live, Engine(SR, min_match=5) as one:
        store(live, recs, range(N_MAIN))
        live.index_finalize()
        live.index_live(1 << 20)
        store(live, recs, range(N_MAIN, N_MAIN + N_NEW))
        store(one, recs, range(N_MAIN + N_NEW))
        one.index_finalize()
        # 4 s clips fan out into three sub-windows + consensus; 7 s clips are queried whole
        long = [synth.synth(t, 3 * SR, 7 * SR + 3, SR, snr_db=20, salt=t) for t in (5, 26, UNSEEN)]
        lane = list(clips) + long
        live.match_stats(reset=True)
        got, want = live.exact_lane(lane), one.exact_lane(lane)
        ms = live.match_stats()
        n_win = 3 * len(clips) + len(long)
        assert ms["queries"] == n_win and ms["queries_lds"] + ms["queries_global"] >= 2 * n_win, ms
        for i, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w), i
        for i, t in enumerate(src[:-1] + [5, 26]):
            w = want[i if i < len(src) - 1 else i + 1]
            assert len(w) and w[0]["track"] == t, (i, t, w[:2])
        assert st_ok(live)
        g2, s2 = live.exact_lane_speeds(clips[2:5], speeds_pm=(-20, 0, 25))
        w2, sw = one.exact_lane_speeds(clips[2:5], speeds_pm=(-20, 0, 25))
        assert s2 == sw == [0, 0, 0]
        for g, w in zip(g2, w2):
            assert len(w) and np.array_equal(g, w)
        assert st_ok(live)


def st_ok(eng):
    st = eng.index_live_stats()
    return (st["main_builds"], st["delta_builds"], st["folds"]) == (1, 1, 0)


# ---------------------------------------------------------------- 9. persistence and the off-switch
def test_save_load_and_off_switch(audio, tmp_path):
    recs, clips, src = audio
    with Engine(SR, min_match=5) as live, Engine(SR, min_match=5) as fresh:
        store(live, recs, range(N_MAIN))
        live.index_finalize()
        live.index_live(1 << 20)
        store(live, recs, range(N_MAIN, N_MAIN + N_NEW))
        want = live.query_pcm(clips)
        path = tmp_path / "live.aidfp"
        live.index_save(path)  # the planes are the source of truth: the file does not know about segments
        fresh.index_load(path)
        same(fresh.query_pcm(clips), want)
        assert fresh.index_live_stats()["main_builds"] == 1 and fresh.index_live_stats()["delta_builds"] == 0
        # two passes per query while the delta holds postings ...
        live.match_stats(reset=True)
        live.query_pcm(clips)
        ms = live.match_stats(reset=True)
        assert ms["queries"] == len(clips) and ms["queries_lds"] + ms["queries_global"] == 2 * len(clips), ms
        # ... the off-switch folds, and queries are back to one
        live.index_live(0)
        st = live.index_live_stats()
        assert (st["main_builds"], st["folds"], st["delta_postings"]) == (1, 1, 0), st
        same(live.query_pcm(clips), want)
        ms = live.match_stats(reset=True)
        assert ms["queries"] == len(clips) and ms["queries_lds"] + ms["queries_global"] == len(clips), ms
        offs_l, posts_l = live.index_csr(offsets=False)
        fresh.index_finalize()
        _, posts_f = fresh.index_csr(offsets=False)
        assert np.array_equal(posts_l, posts_f)
        # off: a store makes the next query rebuild everything, as ever
        live.index_add_records(900, recs[0])
        live.query_pcm(clips[:1])
        st = live.index_live_stats()
        assert (st["main_builds"], st["delta_builds"]) == (2, 1), st
        # a load with the feature on falls back to the full build and empties the delta
        live.index_live(1 << 20)
        live.index_add_records(901, recs[1])
        live.query_pcm(clips[:1])
        assert live.index_live_stats()["delta_postings"] == len(recs[1])
        live.index_load(path)
        same(live.query_pcm(clips), want)
        st = live.index_live_stats()
        assert st["fallbacks"]["load"] == 1 and st["delta_postings"] == 0, st
