"""The Python layer of the content fingerprint (aidfp/chroma.py, ContentIndex.add_pcm / check_pcm) on the GPU:
ChromaPrinter.fingerprints against the oracle (tests/chroma_ref.py) applied to aid_resample's own output, the
`generate_chromaprint` drop-in, and the device path from K11 into K7 against the string path on the same
fingerprints. Comparisons are for equality."""

import asyncio
import ctypes

import numpy as np
import pytest

import chroma_ref as R

pytestmark = pytest.mark.gpu


def p(a):
    return ctypes.c_void_p(a.ctypes.data)


@pytest.fixture
def printer(gpu_engine):
    from aidfp.chroma import ChromaPrinter

    return ChromaPrinter(gpu_engine)


def resampled(eng, x, channels, sr, fmt):
    """aid_resample's 11025 Hz mono output of one clip, on the host."""
    import torch

    src = torch.from_numpy(x).cuda()
    n = len(x) // channels
    m = eng.resample_len(n, sr, 11025)
    dst = torch.zeros(m, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert eng.resample(src.data_ptr(), n, channels, sr, 11025, dst.data_ptr(), m, None, fmt) == m
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def test_resample_plans_to_11025(gpu_engine):
    for sr, want in ((16000, (441, 640)), (44100, (1, 4)), (48000, (147, 640))):
        assert tuple(gpu_engine.resample_plan(sr, 11025)[:2]) == want


def test_fingerprints_from_16k_s16_and_48k_stereo(gpu_engine, printer):
    x16 = np.clip(np.round(R.song(21, 4.0, sr=16000) * 30000.0), -32768, 32767).astype(np.int16)
    mono = R.song(22, 3.5, sr=48000)
    st = np.stack([mono, np.roll(mono, 7) * np.float32(0.5)], axis=1).reshape(-1).astype(np.float32)
    for clips, sr, fmt, ch in (([x16, x16[:50000]], 16000, "s16", 1), ([st], 48000, "f32", 2)):
        got = printer.fingerprints(clips, sr=sr, fmt=fmt, channels=ch)
        for g, c in zip(got, clips):
            want = R.words(resampled(gpu_engine, c, ch, sr, fmt))
            assert len(want) >= 4 and g.dtype == np.uint32 and np.array_equal(g, want)
    # 11025 Hz mono goes in as it is, from the host and from the device
    import torch

    y = R.song(23, 3.0)
    want = R.words(y)
    assert np.array_equal(printer.fingerprints([y])[0], want)
    assert np.array_equal(printer.fingerprints([torch.from_numpy(y).cuda()])[0], want)
    rows = printer.rows([y])[0]
    assert np.array_equal(rows, R.rows(y)) and np.array_equal(printer.words_from_rows([rows])[0], want)


def test_generate_chromaprint_drop_in(gpu_engine, printer):
    from aidfp import chroma
    from aidfp.dedup import parse_fingerprint

    chroma.use(printer)
    try:
        x = np.clip(np.round(R.song(24, 5.0, sr=16000) * 30000.0), -32768, 32767).astype(np.int16)
        run = lambda pcm, d: asyncio.run(chroma.generate_chromaprint(pcm, d))
        assert run(b"", 5.0) is None
        assert run(x[:30000].tobytes(), 5.0) is None  # 20672 samples at 11025 Hz: no word
        assert run(x.tobytes(), 2.9) is None  # cut to 2 s, as fpcalc -length does
        fp = run(x.tobytes(), 4.7)  # cut to 4 s
        want = R.words(resampled(gpu_engine, x[:64000], 1, 16000, "s16"))
        assert fp == chroma.format_fingerprint(want) and np.array_equal(parse_fingerprint(fp), want)
        assert fp != run(x.tobytes(), 5.0)
    finally:
        chroma.use(None)


@pytest.fixture(scope="module")
def tracks():
    a = R.song(31, 30.0)
    return {"a": a, "copy": R.add_noise(a, 20.0, 32), "other": R.song(33, 30.0)}


def test_content_index_pcm_path_equals_string_path(gpu_engine, printer, tracks):
    from aidfp.chroma import format_fingerprint
    from aidfp.dedup import ContentIndex

    fps = {k: format_fingerprint(w) for k, w in zip(tracks, printer.fingerprints(list(tracks.values())))}
    assert len(fps["a"].split(",")) == R.n_words(len(tracks["a"])) == 221
    ids, durs = ["A", "B"], [30.0, 30.0]
    by_string = ContentIndex(gpu_engine)
    assert by_string.add(ids, [fps["a"], fps["other"]], durs) == 2
    want = {k: by_string.scan([fps[k]], [30.0]) for k in ("copy", "other", "a")}
    want_short = by_string.check(fps["copy"], 30.0)
    by_pcm = ContentIndex(gpu_engine)  # resets the engine's catalog
    short = tracks["a"][:20000]  # no word: skipped
    assert by_pcm.add_pcm(["S"] + ids + ["N"], [short, tracks["a"], tracks["other"], tracks["a"]], 11025,
                          [2.0] + durs + [None]) == 2
    assert by_pcm.ids == ids
    for k in ("copy", "other", "a"):
        hit, score = by_pcm.check_pcm(tracks[k], 11025, 30.0, with_score=True)
        (sid,), (ssim,) = want[k]
        assert score == ssim, k
        assert hit == (sid if ssim >= 0.85 else None), k
    assert by_pcm.check_pcm(tracks["copy"], 11025, 30.0) == want_short == "A"
    assert want["copy"][1][0] >= 0.85 and want["a"][1][0] == 1.0
    # the unrelated track is in the catalog itself ("B"); a third one is found nowhere
    third = R.song(34, 30.0)
    assert by_pcm.check_pcm(third, 11025, 30.0) is None
    assert by_pcm.check_pcm(third, 11025, 30.0, with_score=True)[1] < 0.85
    assert by_pcm.check_pcm(short, 11025, 2.0) is None


def test_dedup_scan_at_device_words_equal_host_words(gpu_engine, printer, tracks):
    import torch
    from aidfp import _lib
    from aidfp.dedup import ContentIndex

    L, h = gpu_engine._lib, gpu_engine._h
    words = printer.fingerprints(list(tracks.values()))
    flat = np.concatenate(words)
    off = np.concatenate([[0], np.cumsum([len(w) for w in words])]).astype(np.int64)
    ContentIndex(gpu_engine)
    dev = torch.from_numpy(flat.view(np.int32)).cuda()
    torch.cuda.synchronize()
    dur = np.array([30.0, 29.0, 31.0])
    assert L.aid_dedup_add_at(h, ctypes.c_void_p(dev.data_ptr()), p(off[:3]), p(dur), 2, _lib.AID_PCM_DEVICE) == 0
    last = off[2:] - off[2]
    assert L.aid_dedup_add_at(h, p(flat[off[2]:]), p(last), p(dur[2:]), 1, _lib.AID_PCM_HOST) == 0
    qd = np.array([30.0, 30.0, 30.0])
    i0, s0 = np.zeros(3, np.int64), np.zeros(3)
    i1, s1 = np.full(3, -9, np.int64), np.zeros(3)
    assert L.aid_dedup_scan(h, p(flat), p(off), p(qd), 3, p(i0), p(s0)) == 0
    assert L.aid_dedup_scan_at(h, ctypes.c_void_p(dev.data_ptr()), p(off), p(qd), 3, _lib.AID_PCM_DEVICE, p(i1), p(s1)) == 0
    assert np.array_equal(i0, i1) and np.array_equal(s0, s1) and list(i0) == [0, 1, 2] and np.all(s0 == 1.0)
    assert L.aid_dedup_scan_at(h, p(flat), p(off), p(qd), 3, 7, p(i1), p(s1)) == _lib.AID_ERR_INVALID
