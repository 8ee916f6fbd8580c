"""The preconditions of test_gpu_extract_dense.py, on the CPU oracle alone (oracle/fp_oracle.c, FPSPEC 5-6): every
fixture of dense_fixtures.py reaches the density, the walk length or the edge its GPU test needs, so a fixture can
never quietly stop meeting the bound it was built for. The bounds are the constants of csrc/aidfp_layout.h and
csrc/landmarks.hip, named beside each literal. walk_stats (plain Python) must also count the oracle's records."""

import functools

import numpy as np
import pytest

import dense_fixtures as D
import oracle as O

K3_THREADS = 512  # kK3
PEAK_CAP = 64 * ((1024 + 63 + 7) // 8)  # kHashChunkPeakCap = 64 * ceil((kHashChunk + kZoneDT) / 8)


def hash_capacity(F):
    return 10 * 64 * ((F + 7) // 8)  # hash_capacity(F) = kFan * peak_capacity(F)


BUILDERS = {
    "lattice2048": lambda: D.lattice(1100, 2048),
    "lattice2048_k8": lambda: D.lattice(64, 2048, k0=8),
    "lattice512": lambda: D.lattice(1100, 512),
    "lattice512_diag3": lambda: D.lattice(1100, 512, diag=3),
    "noise": lambda: D.noise(D.NOISE_FRAMES, 512, 0),
    "noise3": lambda: D.noise3(512, 1),
    "zone": D.zone_edges,
}


@functools.lru_cache(maxsize=None)
def measured(name):
    """(frames, oracle peaks, oracle records, walk_stats of those peaks) of a fixture, computed once."""
    x, hop = BUILDERS[name]()
    return _measure(x, hop)


def _measure(x, hop):
    F = O.num_frames(len(x), hop)
    pk = O.peaks(O.stft_power(x, hop)).reshape(-1, 2)
    rec = O.fingerprint(x, hop)
    st = D.walk_stats(pk, F)
    assert st["records"] == len(rec)  # the replayed walk and the oracle count the same records
    return F, pk, rec, st


def test_peak_cap_is_the_layout_constant():
    assert PEAK_CAP == 8704 and D.CHUNK == 1024 and D.ZONE_DT == 63 and D.FAN == 10  # aidfp_layout.h


def test_lattice_at_hop_2048_meets_the_bound_with_equality():
    F, pk, rec, st = measured("lattice2048")
    print("lattice2048", F, len(pk), st)
    assert F == 1100 and len(st["anchors"]) == 2  # two K3 chunks: the COUNT pass runs
    assert max(st["list"]) == PEAK_CAP  # kHashChunkPeakCap, met exactly: one entry more would leave plist
    per8 = np.bincount(pk[:, 0] // 8, minlength=(F + 7) // 8)
    assert np.all(per8 == 64) and st["max_per_8"] == 64  # FPSPEC 5: one peak per 16-bin x 8-frame cell, every cell
    assert st["max_per_frame"] == 64 and np.all(pk[:, 0] % 8 == 0)  # mask rows: all 64 cells, then 7 empty rows
    assert pk[:, 1].min() == 15 and pk[:, 1].max() == 1023
    assert st["anchors"][0] > 16 * K3_THREADS - 1  # pa_per = ceil(n_anchor / kK3) = 16 anchors per thread
    assert st["walk_ge64"] >= 8000  # tmask_ok == false for nearly every anchor
    assert st["fan_cut"] >= 8000  # kFan ends the walk
    assert 0.99 * hash_capacity(F) <= len(rec) <= hash_capacity(F)  # the clip's record region, 99 % full


def test_small_lattice_after_it():
    F, pk, rec, st = measured("lattice2048_k8")
    assert F == 64 and len(pk) == 512 and pk[:, 1].min() == 8 and pk[:, 1].max() == 1016
    assert st["walk_ge64"] > 400 and 0.85 * hash_capacity(F) <= len(rec) <= hash_capacity(F)


@pytest.mark.parametrize("name", ["lattice512", "lattice512_diag3", "noise", "noise3"])
def test_dense_at_hop_512(name):
    F, pk, rec, st = measured(name)
    print(name, F, len(pk), st)
    assert len(st["anchors"]) > 1  # more than one chunk: COUNT and WRITE both run
    assert max(st["anchors"]) > 2 * K3_THREADS  # pa_per >= 3: several anchors per thread (kK3 = 512)
    assert max(st["list"]) <= PEAK_CAP
    # both WRITE branches: the first anchor's bitmask (every target nearer than 64) and the re-walk
    assert st["walk_ge64"] >= 100 and st["walk_lt64"] >= 100
    assert st["fan_cut"] > 0 and st["skip_df"] > 0 and st["skip_same"] > 0
    assert len(rec) <= hash_capacity(F)
    if name != "lattice512":
        assert pk[:, 1].min() == 1 and pk[:, 1].max() == 1023  # both ends of the band
    if name == "lattice512_diag3":
        # peaks at (nearly) every bin: each position inside a mask word, a 64-bin block and a 16-bin cell
        assert len(np.unique(pk[:, 1])) >= 1000 and len(np.unique(pk[:, 1] % 64)) == 64
    if name == "noise3":
        assert len(st["anchors"]) == 3 and min(st["anchors"]) > 2 * K3_THREADS


def test_int16_lattice_keeps_its_peaks():
    x, hop = D.lattice(1100, 512)
    q = D.to_s16(x)
    wide = (q.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    F, pk, rec, st = _measure(wide, hop)
    _, pk_f, _, st_f = measured("lattice512")
    assert len(pk) == len(pk_f) and st["anchors"] == st_f["anchors"] and st["list"] == st_f["list"]
    assert st["walk_ge64"] >= 100 and st["walk_lt64"] >= 100


def test_zone_edges_are_exactly_the_design():
    F, pk, rec, st = measured("zone")
    pairs, F_plan = D.zone_plan()
    assert F == F_plan
    assert np.array_equal(pk, D.zone_peaks())
    assert np.array_equal(rec, D.zone_records())
    inside = [(dt, df) for dt, df, ok in D.ZONE_PAIRS if ok]
    assert sorted(inside) == sorted([(63, 127), (63, -127), (1, 127), (1, -127)])  # kZoneDT, kZoneDF
    assert sorted((dt, df) for dt, df, ok in D.ZONE_PAIRS if not ok) == sorted([(64, 0), (1, 128), (1, -128), (0, 200)])
    assert len(rec) == len(inside) * len(D.ZONE_GROUPS)  # four records per group, none for a pair outside the zone
    got = {(int(r >> np.uint64(32)), int(r) & 0xFFFFFFFF) for r in rec}
    for t1, k1, t2, k2, ok in pairs:
        assert (((t1, (k1 << 22) | (k2 << 12) | (t2 - t1)) in got) == ok), (t1, k1, t2, k2)
    assert st["skip_df"] == 2 * len(D.ZONE_GROUPS) and st["skip_same"] == len(D.ZONE_GROUPS)
    # pairs are isolated, and the ends of both axes are used
    starts = [p[0] for p in pairs]
    assert all(b - a >= D.ZONE_GAP for a, b in zip(starts, starts[1:]))
    assert {1, 1023} <= {p[1] for p in pairs} and {1, 1023} <= {p[3] for p in pairs}
    assert pk[0, 0] == 0 and pk[-1, 0] == F - 1 and len(st["anchors"]) > 1


def test_chunk_edges():
    clips, hop = D.chunk_edges()
    assert [O.num_frames(len(x), hop) for x in clips] == list(D.CHUNK_EDGE_FRAMES) == [1024, 1025, 1087, 1088, 2048, 2049]
    for F, x in zip(D.CHUNK_EDGE_FRAMES, clips):
        _, pk, rec, st = _measure(x, hop)
        assert np.array_equal(pk, D.chunk_edge_peaks(F)), F
        frames = set(pk[:, 0].tolist())
        named = [f for f in (1016, 1023, 1024, 1080, 1086, 1087) if f < F]  # kHashChunk - 1, kHashChunk, + kZoneDT - 1
        assert set(named) <= frames, F
        assert np.sum(pk[:, 0] == 1016) >= 60 and (F <= 1080 or np.sum(pk[:, 0] == 1080) >= 60)  # the dense bursts
        t1 = (rec >> np.uint64(32)).astype(np.int64)
        t2 = t1 + (rec & np.uint64(0xFFF)).astype(np.int64)
        crossing = int(np.sum((t1 <= 1023) & (t2 >= 1024)))
        assert (crossing >= 1) == (F > 1024), F  # a chunk-0 anchor whose target lies in chunk 1's frames
        if F >= 1087:
            assert np.any((t1 == 1023) & (t2 == 1086))  # dt = kZoneDT: the last frame of chunk 0's list
            assert np.any((t1 <= 1023) & (t2 == 1080))
        if F >= 1088:
            assert not np.any((t1 <= 1023) & (t2 == 1087)) and np.any((t1 == 1024) & (t2 == 1087))
        if F >= 2049:
            assert np.any((t1 == 2047) & (t2 == 2048)) and len(st["anchors"]) == 3


def test_builders_are_deterministic():
    for build in (lambda: D.lattice(40, 512, diag=3, seed=2), lambda: D.lattice(17, 2048), lambda: D.noise(5, 512, 3),
                  D.zone_edges):
        (a, ha), (b, hb) = build(), build()
        assert a.dtype == np.float32 and ha == hb and np.array_equal(a, b)
    (a, _), (b, _) = D.chunk_edges(), D.chunk_edges()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not np.array_equal(D.lattice(17, 2048, seed=0)[0], D.lattice(17, 2048, seed=1)[0])


def test_walk_stats_on_a_hand_made_list():
    """Two frames: anchor (0, 100) passes over its own frame's second peak, skips one target for |df| > 127 and
    accepts two."""
    st = D.walk_stats(np.array([[0, 100], [0, 400], [5, 100], [5, 227], [5, 228], [69, 100]]))
    assert st["anchors"] == [6] and st["list"] == [6] and st["max_per_frame"] == 3 and st["max_per_8"] == 5
    # (0,100) -> (5,100), (5,227); (0,400) -> none (|df| >= 172); (5,*) -> (69,100) is dt 64: none
    assert st["records"] == 2 and st["skip_same"] == 1 + 2 + 1 and st["skip_df"] == 1 + 3
    assert st["max_walk"] == 2 and st["walk_lt64"] == 1 and st["walk_ge64"] == 0 and st["fan_cut"] == 0
