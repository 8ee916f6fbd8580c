"""Native int16 PCM through extraction, the windowed and pipelined queries and the exact lane (spec/FPSPEC.md 8,
the _s16 entry points of include/aidfp.h), bit-exact against the CPU oracle applied to q / 32768.

Every expected value comes from oracle/ on the widened samples, never from the engine's own float path. The inputs
include full-range random samples and a full-scale square wave (tests/s16_inputs.py)."""

import asyncio
import ctypes
import uuid

import numpy as np
import pytest
import torch

import oracle as O
from aidfp import _lib
from aidfp import exact as ex
from aidfp.engine import Engine, exact_windows, peaks_from_mask
from aidfp.fingerprint import OlafMatch
from s16_inputs import random_q, square_q, synth_q, widen

pytestmark = pytest.mark.gpu
LENS = [0, 2047, 2048, 2049, 5000, 2048 + 512 * 70]
SR16, HOP16 = 16000, 256
N_TRACKS, TRACK_S = 8, 8


def _mixed_clips(sr):
    """Every length with synthetic, full-range random and full-scale square-wave content."""
    clips = []
    for i, n in enumerate(LENS):
        clips += [synth_q(20 + i, 555 * i, n, sr, snr_db=20 if i % 2 else None, salt=3), random_q(n, 100 + i),
                  square_q(n, 29 + 2 * i)]
    return clips


@pytest.mark.parametrize("sr,hop", [(44100, 512), (16000, 256)])
def test_host_power_peaks_hashes_bit_exact(sr, hop):
    clips = _mixed_clips(sr)
    assert min(c.min() for c in clips if len(c)) == -32768 and max(c.max() for c in clips if len(c)) == 32767
    wide = [widen(q) for q in clips]
    with Engine(sr, keep_power=True) as eng:
        assert eng.hop == hop
        eng.extract_host(clips, fmt="s16")
        for c, x in enumerate(wide):
            P = eng.power(c, len(x))
            R = O.stft_power(x, hop)
            assert P.shape == R.shape
            assert np.array_equal(P.view(np.uint32), R.view(np.uint32)), f"clip {c}: power bits differ"
    with Engine(sr) as eng:
        got = eng.extract_host(clips, fmt="s16")
        counts = eng.counts()
        for c, x in enumerate(wide):
            ref_pk = O.peaks(O.stft_power(x, hop)) if len(x) >= 2048 else np.zeros((0, 2), np.int32)
            pk = peaks_from_mask(eng.peakmask(c, len(x)))
            assert np.array_equal(pk, ref_pk.reshape(-1, 2)), f"clip {c}: peaks differ"
            ref = O.fingerprint(x, hop)
            assert counts[c] == len(ref)
            assert np.array_equal(got[c], ref), f"clip {c}: hashes differ"
        assert sum(len(g) for g in got) > 100


@pytest.fixture(scope="module")
def indexed():
    """A 16 kHz engine whose index holds the oracle's records of 8 short synthetic tracks, and its postings."""
    eng = Engine(SR16)
    for t in range(N_TRACKS):
        eng.index_add_records(t, O.fingerprint(widen(synth_q(t, 0, TRACK_S * SR16, SR16)), HOP16))
    eng.index_finalize()
    yield eng, eng.index_export()
    eng.close()


def _excerpt(t, start_s, n, salt):
    return synth_q(t, int(start_s * SR16), n, SR16, snr_db=20, salt=salt)


def _oracle_rows(eng, post, x):
    return O.query(post, O.fingerprint(x, HOP16), min_match=eng.min_match, max_rows=eng.max_results)


def test_device_windows_in_place(indexed):
    """One int16 device buffer, clips at an even and at an odd sample offset: extraction in place, then
    query_windows over overlapping windows (the exact lane's three sub-windows of each 5 s clip and one window
    that starts at an odd sample)."""
    eng, post = indexed
    n = 5 * SR16
    clips = [_excerpt(2, 1.0, n, 41), _excerpt(5, 2.0, n, 42), random_q(n, 7)]
    offs = np.array([0, n + 1, 2 * n + 4], np.int64)  # even, odd, even
    buf = np.zeros(3 * n + 8, np.int16)
    for q, o in zip(clips, offs):
        buf[o:o + n] = q
    dev = torch.from_numpy(buf).cuda()
    # extraction of [offs[c], offs[c + 1]): the gaps' zeros belong to the clips
    ext = np.append(offs, len(buf))
    eng.extract_device(dev.data_ptr(), ext, fmt="s16")
    for c in range(3):
        assert np.array_equal(eng.hashes(c), O.fingerprint(widen(buf[ext[c]:ext[c + 1]]), HOP16)), c
    _, plan = exact_windows(n, SR16)
    st = [int(o + lo) for o in offs for lo, ln in plan] + [int(offs[0]) + 12345]
    en = [int(o + lo + ln) for o in offs for lo, ln in plan] + [int(offs[0]) + 12345 + 3 * SR16]
    assert any(s % 2 for s in st) and any(s % 2 == 0 for s in st)
    got = eng.query_windows(dev.data_ptr(), st, en, fmt="s16")
    assert sum(len(r) > 0 for r in got) >= 6
    for k in range(len(st)):
        assert np.array_equal(got[k], _oracle_rows(eng, post, widen(buf[st[k]:en[k]]))), k
    # the same windows in two halves
    a = eng.query_windows_submit(dev.data_ptr(), st[:4], en[:4], fmt="s16")
    b = eng.query_windows_submit(dev.data_ptr(), st[4:], en[4:], fmt="s16")
    rows = b.collect()
    rows = a.collect() + rows
    for g, w in zip(rows, got):
        assert np.array_equal(g, w)


def test_clip_groups(gpu_engine):
    """4 short s16 clips split into several K1 -> K2 clip groups: same hashes."""
    clips = [synth_q(60, 0, 30000, 44100), random_q(25000, 11), synth_q(61, 99, 40000, 44100, snr_db=20, salt=2),
             square_q(21000, 50)]
    frames = [gpu_engine.num_frames(len(c)) for c in clips]
    gpu_engine.force("plane_rows", max(frames))  # no two clips fit one group
    try:
        got = gpu_engine.extract_host(clips, fmt="s16")
    finally:
        gpu_engine.force("plane_rows", 0)
    for c, q in enumerate(clips):
        assert np.array_equal(got[c], O.fingerprint(widen(q), 512)), c
    assert sum(len(g) for g in got) > 100


@pytest.mark.parametrize("gather", [0, 1])
def test_exact_lane_equals_oracle_lane(indexed, gather):
    """exact_lane(fmt="s16"), sub-windows read in place and through the converting gather, against the all-oracle
    lane: the oracle's records of each reference-sliced window, oracle/fp_match.c, then aidfp.exact's per-window
    consensus and ranking (the route of tests/test_gpu_lane_parity.py)."""
    eng, post = indexed
    clips = [_excerpt(1, 0.5, 5 * SR16, 51), _excerpt(6, 1.0, 65601, 52), _excerpt(3, 2.0, 3 * SR16, 53),
             random_q(19200, 9)]
    eng.force("lane_gather", gather)
    try:
        got = eng.exact_lane(clips, max_out=10, fmt="s16")
    finally:
        eng.force("lane_gather", 0)
    sec = eng.hop / SR16

    async def oracle_query(piece: bytes):
        rows = _oracle_rows(eng, post, np.frombuffer(piece, dtype="<f4").astype(np.float32))
        return [OlafMatch(int(c), tq0 * sec, tq1 * sec, str(uuid.UUID(int=int(tr) + 1)), int(tr), (tq0 + d) * sec,
                          (tq1 + d) * sec) for c, tr, d, tq0, tq1 in rows.tolist()]

    for i, q in enumerate(clips):
        want = asyncio.run(ex.run_exact_lane(widen(q).astype("<f4").tobytes(), 10, query=oracle_query,
                                             sample_rate=SR16))
        r = got[i]
        assert len(r) == len(want), (i, r, want)
        for x, w in zip(r, want):
            assert int(x["track"]) == w.track.int - 1 and int(x["aligned_hashes"]) == w.aligned_hashes
            assert float(x["offset_seconds"]) == w.offset_seconds and float(x["confidence"]) == w.confidence
    assert [int(got[i][0]["track"]) for i in range(3)] == [1, 6, 3]


def test_query_pcm_submit_out_of_order(indexed):
    eng, post = indexed
    a_clips = [_excerpt(0, 1.0, 4 * SR16, 61), random_q(30001, 13)]
    b_clips = [_excerpt(7, 0.0, 5 * SR16 + 1, 62), _excerpt(4, 2.5, 3 * SR16, 63), square_q(20000, 8)]
    want = eng.query_pcm(a_clips + b_clips, fmt="s16")
    a = eng.query_pcm_submit(a_clips, fmt="s16")
    b = eng.query_pcm_submit(b_clips, fmt="s16")
    gb = b.collect()
    ga = a.collect()
    assert sum(len(r) > 0 for r in want) >= 3
    for q, w, g in zip(a_clips + b_clips, want, ga + gb):
        assert np.array_equal(w, g)
        assert np.array_equal(w, _oracle_rows(eng, post, widen(q)))


def test_errors(indexed):
    eng, _ = indexed
    x = np.zeros(4096, np.float32)
    for call in (lambda: eng.extract_host([x], fmt="s16"), lambda: eng.query_pcm([x], fmt="s16"),
                 lambda: eng.query_pcm_submit([x], fmt="s16"), lambda: eng.exact_lane([x], fmt="s16"),
                 lambda: eng.extract_host([x.astype(np.int32)], fmt="s16"),
                 lambda: eng.extract_host([x.astype(np.int16)], fmt="s24")):
        with pytest.raises(ValueError):
            call()
    offs = np.array([0, 4096], np.int64)
    L = _lib.load()
    for loc in (_lib.AID_PCM_HOST, _lib.AID_PCM_DEVICE):
        assert L.aid_extract_s16(eng._h, None, offs.ctypes.data_as(ctypes.c_void_p), 1, loc, None) == _lib.AID_ERR_INVALID
        assert "aid_extract_s16: null pcm" in _lib.last_error()
    rows = np.zeros(5 * eng.max_results, np.int32)
    nrows = np.zeros(1, np.int32)
    assert L.aid_query_pcm_s16(eng._h, None, offs.ctypes.data_as(ctypes.c_void_p), 1, _lib.AID_PCM_HOST,
                               rows.ctypes.data_as(ctypes.c_void_p), nrows.ctypes.data_as(ctypes.c_void_p),
                               None) == _lib.AID_ERR_INVALID
    # an int16 array without fmt is still cast to float, as before: integer values, not q / 32768
    q = synth_q(1, 0, 8192, SR16)
    assert np.array_equal(eng.extract_host([q])[0], O.fingerprint(q.astype(np.float32), HOP16))
