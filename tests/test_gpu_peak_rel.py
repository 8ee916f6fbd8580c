"""The per-clip relative peak threshold (spec/FPSPEC.md 5.1, aid_config.peak_rel) on the GPU, bit-exact against the
oracle route: for a clip x, P = oracle.stft_power(x), thr_c = max(floor, r * fmax-reduce(P)) in binary32, then
oracle.peaks(P, thr_c) and oracle.fingerprint(x, hop, thr_c). The oracle takes thr per call, so nothing under
oracle/ knows about the rule; every expected value comes from it, never from the engine.

Unless a test says otherwise: 16 kHz, hop 256, floor 2^-20, r = float32(1e-4)."""

import asyncio
import ctypes
import uuid

import numpy as np
import pytest
import torch

import oracle as O
from aidfp import _lib
from aidfp import exact as ex
from aidfp import fingerprint as fp
from aidfp import synth
from aidfp.engine import Engine, exact_windows, peaks_from_mask
from aidfp.fingerprint import OlafMatch

pytestmark = pytest.mark.gpu
SR, HOP = 16000, 256
FLOOR = 2.0 ** -20
R = np.float32(1e-4)
F32 = np.float32


def thr_of(P, floor=FLOOR, r=R):
    """FPSPEC 5.1 in binary32: a NaN never raises the maximum, +0 for no frames, one multiply, then the floor."""
    pmax = np.fmax.reduce(P.ravel(), initial=F32(0.0)).astype(np.float32)
    with np.errstate(over="ignore"):
        t = F32(r) * pmax
    return np.maximum(F32(floor), t).astype(np.float32)


def route(x, hop=HOP, floor=FLOOR, r=R):
    """(thr_c, peaks [n, 2], records) of one clip by the oracle."""
    P = O.stft_power(x, hop)
    t = thr_of(P, floor, r)
    pk = O.peaks(P, float(t)) if len(P) else np.zeros((0, 2), np.int32)
    return t, pk.reshape(-1, 2), O.fingerprint(x, hop, float(t))


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def gained(track, start, n, gain, sr=SR, snr=None, salt=0):
    return (synth.synth(track, start, n, sr, snr_db=snr, salt=salt) * F32(gain)).astype(np.float32)


def check_batch(eng, clips, routes, fmt="f32", send=None):
    """One extraction call of `clips` (or their other representation `send`) against the clips' oracle routes."""
    got = eng.extract_host(send if send is not None else clips, fmt=fmt)
    thr = eng.thresholds()
    counts = eng.counts()
    assert thr.dtype == np.float32 and len(thr) == len(clips)
    for c, (x, (t, pk, rec)) in enumerate(zip(clips, routes)):
        assert bits(thr[c]) == bits(t), f"clip {c}: thr_c {thr[c]!r} vs {t!r}"
        assert np.array_equal(peaks_from_mask(eng.peakmask(c, len(x))), pk), f"clip {c}: peak masks differ"
        assert counts[c] == len(rec)
        assert np.array_equal(got[c], rec), f"clip {c}: records differ"
    return got


@pytest.fixture(scope="module")
def rel_eng():
    eng = Engine(SR, peak_threshold=FLOOR, peak_rel=float(R))
    assert eng.hop == HOP and bits(eng.peak_rel) == bits(R) and eng.peak_threshold == FLOOR
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def abs_eng():
    eng = Engine(SR)
    assert eng.peak_rel == 0.0 and eng.peak_threshold == 4.0
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def mixed():
    """F = 0, 1, 7, 8, 9 frames, about 2 s and two 10 s clips; loud and quiet clips next to each other."""
    lens = [2047, 2048, 2048 + 6 * HOP, 2048 + 7 * HOP + 3, 2048 + 8 * HOP, 2 * SR + 1, 10 * SR, 10 * SR]
    gains = [1.0, 1 / 32, 0.5, 0.1259, 1 / 8, 1.0, 1 / 32, 1.0]
    clips = [gained(10 + i, 321 * i, n, g, snr=20 if i % 2 else None, salt=i) for i, (n, g) in enumerate(zip(lens, gains))]
    routes = [route(x) for x in clips]
    return clips, routes


def test_parity_mixed_batch(rel_eng, mixed):
    clips, routes = mixed
    assert [O.num_frames(len(x), HOP) for x in clips[:5]] == [0, 1, 7, 8, 9]
    assert len(routes[6][2]) > 1000 and len(routes[7][2]) > 1000  # a condition on the inputs, not a measurement
    assert len({int(bits(t)) for t, _, _ in routes}) >= 6  # the clips really have thresholds of their own
    assert all(t > FLOOR for t, _, _ in routes[1:])
    check_batch(rel_eng, clips, routes)


@pytest.mark.parametrize("what,value", [("plane_rows", 618), ("k2_strips_x100", 25), ("k2_strips_x100", 300)])
def test_parity_forced_splits(rel_eng, mixed, what, value):
    """plane_rows 618: the call splits into three K1 -> K2 groups ([0..5], [6], [7]), so a group's clips index the
    maxima from the group's first clip on; fixed K2 strips: several workgroups of a clip read its one threshold."""
    clips, routes = mixed
    rel_eng.force(what, value)
    try:
        check_batch(rel_eng, clips, routes)
    finally:
        rel_eng.force(what, 0)


def test_gain_invariance(rel_eng, abs_eng):
    """A power-of-two gain scales every binary32 power exactly, so thr_c scales with it and the records are the
    same arrays. The absolute default finds nothing in the quiet copy: this test fails without the feature."""
    x = synth.synth(3, 1000, 10 * SR, SR, snr_db=20, salt=5)
    batch = [x, x * F32(0.25), x * F32(1 / 32)]
    got = rel_eng.extract_host(batch)
    thr = rel_eng.thresholds()
    assert len(got[0]) > 1000
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
    assert np.array_equal(got[0], route(x)[2])
    assert thr[0] == thr[1] * F32(16) == thr[2] * F32(1024)
    quiet = abs_eng.extract_host(batch)
    assert len(quiet[0]) > 1000 and len(quiet[2]) == 0
    assert len(O.fingerprint(batch[2], HOP)) == 0


def test_floor(rel_eng, abs_eng):
    x = synth.synth(4, 0, 3 * SR, SR)
    faint = x * F32(2.0 ** -14)  # r * Pmax < floor < Pmax: the floor decides, and peaks remain above it
    zero = np.zeros(2 * SR, np.float32)
    clips = [x, faint, zero, x * F32(1 / 32)]
    routes = [route(c) for c in clips]
    Pf = O.stft_power(faint, HOP)
    assert R * Pf.max() < F32(FLOOR) < Pf.max()
    assert routes[1][0] == F32(FLOOR) and routes[2][0] == F32(FLOOR) and routes[0][0] > FLOOR
    assert len(routes[1][2]) > 0 and len(routes[2][2]) == 0
    assert np.array_equal(routes[1][2], O.fingerprint(faint, HOP, FLOOR))
    check_batch(rel_eng, clips, routes)
    # peak_rel = 0: the absolute rule, and the readout says so
    got = abs_eng.extract_host(clips)
    assert np.array_equal(bits(abs_eng.thresholds()), bits(np.full(len(clips), 4.0, np.float32)))
    for c, xc in enumerate(clips):
        assert np.array_equal(got[c], O.fingerprint(xc, HOP, 4.0)), c
    assert len(got[0]) > 100


@pytest.mark.parametrize("sr,hop", [(SR, 128), (SR, 256), (SR, 512), (SR, 1024), (SR, 2048), (44100, 0)])
def test_every_k1_instantiation(sr, hop):
    """K1 is compiled per hop (ring rows per frame); each instantiation has its own copy of the maximum."""
    with Engine(sr, hop=hop, peak_threshold=FLOOR, peak_rel=float(R)) as eng:
        assert eng.hop == (hop or 512)
        clips = [gained(20, 0, sr + 17, 1.0, sr=sr, snr=20, salt=1), gained(21, 500, sr, 1 / 8, sr=sr)]
        routes = [route(x, eng.hop) for x in clips]
        assert all(len(r[2]) > 20 for r in routes)
        check_batch(eng, clips, routes)


def test_s16_equals_float(rel_eng):
    """aid_extract_s16 on q = the float call on q / 32768 (FPSPEC 8), also under the relative rule."""
    q = [(synth.synth_int16(30 + i, 99 * i, n, SR, synth.noise_halfwidth(20 if i else None), i) >> sh).astype(np.int16)
         for i, (n, sh) in enumerate([(3 * SR, 0), (2 * SR + 1, 5), (2048 + 7 * HOP, 3), (2047, 0)])]
    wide = [(a.astype(np.float32) / F32(32768.0)).astype(np.float32) for a in q]
    routes = [route(x) for x in wide]
    assert len(routes[0][2]) > 100 and len(routes[1][2]) > 100
    got16 = check_batch(rel_eng, wide, routes, fmt="s16", send=q)
    got32 = check_batch(rel_eng, wide, routes)
    assert all(np.array_equal(a, b) for a, b in zip(got16, got32))


def test_non_finite(rel_eng):
    """A NaN sample (its frames are NaN: they never raise the maximum and hold no peak) and a 1e30 sample (its
    frames overflow to +inf: thr_c = +inf, no peak), each between ordinary clips that must not notice."""
    a, b, c = gained(40, 0, 2 * SR, 1.0), gained(41, 0, 2 * SR, 1 / 32, snr=20, salt=2), gained(42, 7, 2 * SR + 5, 0.5)
    nan = gained(43, 0, 2 * SR, 1.0)
    nan[9000] = np.nan
    big = gained(44, 0, 2 * SR, 1.0)
    big[12345] = 1e30
    clips = [a, nan, b, big, c]
    routes = [route(x) for x in clips]
    Pn, Pb = O.stft_power(nan, HOP), O.stft_power(big, HOP)
    assert np.isnan(Pn).any() and not np.isnan(Pn).all() and np.isfinite(routes[1][0]) and len(routes[1][1]) > 0
    assert np.isinf(Pb).any() and np.isposinf(routes[3][0]) and len(routes[3][1]) == 0
    got = rel_eng.extract_host(clips)
    thr = rel_eng.thresholds()
    for i, (x, (t, pk, rec)) in enumerate(zip(clips, routes)):
        assert bits(thr[i]) == bits(t), i
        assert np.array_equal(peaks_from_mask(rel_eng.peakmask(i, len(x))), pk), f"clip {i}: peak masks differ"
    for i in (0, 2, 4):
        assert np.array_equal(got[i], routes[i][2]) and len(got[i]) > 100, i
    alone = rel_eng.extract_host([a, b, c])
    assert all(np.array_equal(alone[k], got[i]) for k, i in enumerate((0, 2, 4)))


# ---- query routes ----
N_TRACKS, TRACK_S = 8, 8


@pytest.fixture(scope="module")
def indexed(rel_eng, abs_eng):
    """8 tracks indexed by extraction on the relative engine (and on the default one, under its own rule); the
    oracle's postings of the same tracks by the oracle route."""
    tracks = [synth.synth(t, 0, TRACK_S * SR, SR) for t in range(N_TRACKS)]
    for eng in (rel_eng, abs_eng):
        eng.index_reset()
        eng.extract_host(tracks)
        eng.index_add_extracted(np.arange(N_TRACKS, dtype=np.uint32))
        eng.index_finalize()
    post = []
    for t, x in enumerate(tracks):
        rec = route(x)[2]
        post.append(np.stack([(rec & np.uint64(0xFFFFFFFF)).astype(np.uint32), np.full(len(rec), t, np.uint32),
                              (rec >> np.uint64(32)).astype(np.uint32)], axis=1))
    return np.concatenate(post)


def _quiet_query(t, start_s, n, salt):
    return gained(t, int(start_s * SR), n, 1 / 32, snr=20, salt=salt)


def _oracle_rows(eng, post, x):
    return O.query(post, route(x)[2], min_match=eng.min_match, max_rows=eng.max_results)


def test_query_routes(rel_eng, abs_eng, indexed):
    post = indexed
    n = 5 * SR
    clips = [_quiet_query(1, 0.5, n, 51), _quiet_query(6, 1.0, n, 52), _quiet_query(3, 2.0, n + 1, 53)]
    want = [_oracle_rows(rel_eng, post, x) for x in clips]
    assert [int(w[0][1]) for w in want] == [1, 6, 3]
    got = rel_eng.query_pcm(clips)
    pend = rel_eng.query_pcm_submit(clips)
    got2 = pend.collect()
    for g, g2, w in zip(got, got2, want):
        assert np.array_equal(g, w) and np.array_equal(g2, w)
    # windows of one device buffer: every window is a clip of its own, with its own Pmax
    buf = np.concatenate(clips)
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64)
    dev = torch.from_numpy(buf).cuda()
    st = [int(offs[i] + lo) for i, c in enumerate(clips) for lo, ln in exact_windows(len(c), SR)[1]]
    en = [int(offs[i] + lo + ln) for i, c in enumerate(clips) for lo, ln in exact_windows(len(c), SR)[1]]
    wgot = rel_eng.query_windows(dev.data_ptr(), st, en)
    wthr = rel_eng.thresholds()
    assert len(st) == 7 and sum(len(r) > 0 for r in wgot) >= 6  # 3 + 3 sub-windows, and the longer clip whole
    for k in range(len(st)):
        piece = buf[st[k]:en[k]]
        assert bits(wthr[k]) == bits(route(piece)[0]), k
        assert np.array_equal(wgot[k], _oracle_rows(rel_eng, post, piece)), k
    assert len({int(b) for b in bits(wthr[:3])}) > 1  # sub-windows of one clip: thresholds of their own
    # the exact lane = consensus over its three windows, each by the oracle route
    lane = rel_eng.exact_lane(clips, max_out=10)
    sec = rel_eng.hop / SR

    async def oracle_query(piece: bytes):
        rows = _oracle_rows(rel_eng, post, np.frombuffer(piece, dtype="<f4").astype(np.float32))
        return [OlafMatch(int(c), tq0 * sec, tq1 * sec, str(uuid.UUID(int=int(tr) + 1)), int(tr), (tq0 + d) * sec,
                          (tq1 + d) * sec) for c, tr, d, tq0, tq1 in rows.tolist()]

    for i, x in enumerate(clips):
        ref = asyncio.run(ex.run_exact_lane(x.astype("<f4").tobytes(), 10, query=oracle_query, sample_rate=SR))
        assert len(lane[i]) == len(ref) > 0, (i, lane[i], ref)
        for g, w in zip(lane[i], ref):
            assert int(g["track"]) == w.track.int - 1 and int(g["aligned_hashes"]) == w.aligned_hashes
            assert float(g["offset_seconds"]) == w.offset_seconds and float(g["confidence"]) == w.confidence
    assert [int(lane[i][0]["track"]) for i in range(3)] == [1, 6, 3]
    # the default engine hears nothing in the same queries
    assert all(len(r) == 0 for r in abs_eng.query_pcm(clips))
    assert all(len(r) == 0 for r in abs_eng.query_windows(dev.data_ptr(), st, en))
    assert all(len(r) == 0 for r in abs_eng.exact_lane(clips, max_out=10))
    assert np.array_equal(bits(abs_eng.thresholds()), bits(np.full(abs_eng.thresholds().shape, 4.0, np.float32)))


# ---- service and stream ----
def _bytes(x):
    return np.asarray(x, dtype="<f4").tobytes()


def test_service_top_db(tmp_path, monkeypatch):
    monkeypatch.delenv("AIDFP_PEAK_TOP_DB", raising=False)
    monkeypatch.delenv("AIDFP_PEAK_FLOOR", raising=False)
    names = [f"track-{i}" for i in range(3)]
    tracks = [_bytes(synth.synth(50 + i, 0, 15 * SR, SR)) for i in range(3)]
    query = _bytes(gained(51, 4 * SR, 5 * SR, 1 / 32, snr=20, salt=8))

    def run(svc):
        try:
            for name, t in zip(names, tracks):
                assert svc.index_track(t, name)
            return svc.query(query), svc._eng().peak_rel, svc._eng().peak_threshold
        finally:
            svc.close()

    found, rel, floor = run(fp.FingerprintService(tmp_path / "arg", peak_top_db=40, peak_floor=FLOOR))
    assert bits(rel) == bits(R) and floor == FLOOR
    assert found and found[0].reference_path == names[1]
    monkeypatch.setenv("AIDFP_PEAK_TOP_DB", "40")
    monkeypatch.setenv("AIDFP_PEAK_FLOOR", repr(FLOOR))
    by_env = run(fp.FingerprintService(tmp_path / "env"))
    assert by_env == (found, rel, floor)
    monkeypatch.delenv("AIDFP_PEAK_TOP_DB")
    monkeypatch.delenv("AIDFP_PEAK_FLOOR")
    none, rel0, thr0 = run(fp.FingerprintService(tmp_path / "default"))
    assert none == [] and rel0 == 0.0 and thr0 == 4.0


def test_stream_bank_identifies_a_quiet_stream():
    from aidfp.catalog import ingest_synthetic
    from aidfp.stream import StreamBank

    QSR, seg_s = 48000, 12.0
    orders = [[2, 5], [7, 0]]
    with Engine(SR, peak_threshold=FLOOR, peak_rel=float(R)) as eng:
        ingest_synthetic(eng, np.arange(8, dtype=np.uint32), 20.0, local=True)
        eng.index_finalize()
        seg = int(seg_s * QSR)
        st = np.stack([np.stack([np.concatenate([gained(t, 0, seg, 1 / 32, sr=QSR, snr=30, salt=2 * i + ch + 1)
                                                 for t in order]) for ch in range(2)], axis=1)
                       for i, order in enumerate(orders)])  # [S, n, 2]
        bank = StreamBank(eng, len(orders), stream_sr=QSR)
        res = [[] for _ in orders]
        for a in range(0, st.shape[1], 200001):
            out = bank.push(st[:, a:a + 200001])
            for i in range(len(orders)):
                res[i] += out[i]
    hits = total = 0
    for i, order in enumerate(orders):
        assert len(res[i]) == int((2 * seg_s - 5.0) // 2.5) + 1
        for r in res[i]:
            a, b = r.start_s, r.start_s + 5.0
            if int(a // seg_s) == int((b - 1e-9) // seg_s):
                total += 1
                hits += r.best_track == order[int(a // seg_s)]
    assert total >= 8 and hits == total


def test_validation():
    L = _lib.load()
    for bad in (-1.0, 1.0, float("nan"), 2.0 ** -61, float("inf"), 1.5):
        cfg = _lib.AidConfig()
        assert L.aid_config_default(SR, ctypes.byref(cfg)) == _lib.AID_OK
        cfg.peak_rel = bad
        h = ctypes.c_void_p()
        assert L.aid_engine_create(ctypes.byref(cfg), ctypes.byref(h)) == _lib.AID_ERR_INVALID, bad
        assert not h.value and "peak_rel" in _lib.last_error()
    for ok in (2.0 ** -60, float(np.nextafter(F32(1.0), F32(0.0)))):
        with Engine(SR, peak_rel=ok) as eng:
            assert eng.peak_rel == ok
