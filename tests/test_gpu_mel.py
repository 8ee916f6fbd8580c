"""K10 (csrc/mel.hip, aid_logmel) against the oracle tests/mel_ref.py (spec/FPSPEC.md 10): every comparison is for
equality of the float values, a few chunks per test. The oracle takes the engine's own filter table (aid_mel_filters),
which tests/test_mel_plan_host.py holds to the captured extractor's within one binary32 ulp."""

import ctypes
import json
from pathlib import Path

import numpy as np
import pytest

import mel_ref as R

pytestmark = pytest.mark.gpu
L = R.L
GOLD = Path(__file__).resolve().parent / "golden"
RUN = 4  # frames of one K10 workgroup (aidfp_mel_plan.h kMelRun)


def run_edges():
    """First and last frame of every workgroup's run, the short last run included (1001 = 250 * 4 + 1)."""
    return {t for t in range(R.T) if t % RUN in (0, RUN - 1)} | {R.T - 1}


@pytest.fixture(scope="module")
def clap():
    from aidfp import clap as C

    return C


@pytest.fixture
def lm(gpu_engine, clap):
    m = clap.LogMel(gpu_engine)  # (re)configures the shared engine: slaney, 50 .. 14000 Hz
    m.W = m.filters()
    return m


def images(out) -> np.ndarray:
    a = out.cpu().numpy()
    assert a.shape[1:] == (1, R.T, R.BANDS) and not np.isnan(a).any()
    return a[:, 0]


def check_chunks(got, meta, clips, W, frames_of):
    """Every chunk of `meta` at frames_of(r, fill) against the oracle."""
    for c, m in zip(got, meta):
        r, fill = int(m["r"]), int(m["r"]) * int(m["rep"])
        fr = sorted(frames_of(r, fill))
        want = R.logmel(clips[int(m["clip"])], W, fr, start=int(m["start"]), r=r, fill=fill)
        bad = np.argwhere(c[fr] != want)
        assert len(bad) == 0, (dict(zip(m.dtype.names, m.tolist())), fr[bad[0][0]], bad[0][1], c[fr][tuple(bad[0])],
                               want[tuple(bad[0])], len(bad))


@pytest.mark.parametrize("bank,kind", [("slaney", R.SLANEY), ("htk", R.HTK)])
def test_full_chunk_both_banks(gpu_engine, clap, bank, kind):
    m = clap.LogMel(gpu_engine, bank=bank)
    W = m.filters()
    ref = R.bank(kind)
    assert np.array_equal(R.supports(W)[0], R.supports(ref)[0]) and R.supports(W)[2] == 299
    assert np.all(np.abs(W.astype(np.float64) - ref.astype(np.float64)) <= np.spacing(ref).astype(np.float64))
    x = np.resize(R.fixture_input(3), L)
    out, meta = m.chunks(x)
    assert [(int(c["start"]), int(c["r"]), int(c["rep"])) for c in meta] == [(0, L, 1), (240000, 240000, 1)]
    check_chunks(images(out), meta, [x], W, lambda r, fill: range(R.T))


@pytest.mark.parametrize("fmt", ["f32", "s16"])
def test_batch_of_lengths(lm, fmt):
    """479800 puts the real end inside the right reflection; 480001 and 288000 have a second, short chunk."""
    lengths = [48000, 288000, 479800, 480001]
    rng = np.random.default_rng(11)
    clips = [np.resize(R.fixture_input(i % 4), n) * np.float32(0.9) + (1e-3 * rng.standard_normal(n)).astype(np.float32)
             for i, n in enumerate(lengths)]
    if fmt == "s16":
        q = [np.clip(np.round(c * 32767.0), -32768, 32767).astype(np.int16) for c in clips]
        out, meta = lm.chunks(q, fmt="s16")
        clips = [R.s16_to_f32(c) for c in q]
    else:
        out, meta = lm.chunks(clips)
    assert [(int(m["clip"]), int(m["start"]), int(m["r"])) for m in meta] == [
        (0, 0, 48000), (1, 0, 288000), (1, 240000, 48000), (2, 0, 479800), (2, 240000, 239800), (3, 0, L),
        (3, 240000, 240001)]
    check_chunks(images(out), meta, clips, lm.W, lambda r, fill: set(R.fixture_frames(r)) | run_edges())


def test_repeatpad_and_long_queries(lm):
    rng = np.random.default_rng(12)
    for r in (1, 144000, 160001, 240000, 479999):
        x = (0.3 * rng.standard_normal(r)).astype(np.float32)
        out, meta = lm._run(x, None, "f32", R.REPEATPAD, 0)
        assert (int(meta[0]["r"]), int(meta[0]["rep"])) == (r, L // r)
        check_chunks(images(out), meta, [x], lm.W, lambda r_, fill: set(R.fixture_frames(r_, fill)) | {3, 4, 992})
    n = L + 7777
    x = (0.3 * rng.standard_normal(n)).astype(np.float32)
    for start in (0, n - L):
        got = images(lm.query(x, start=start))
        fr = sorted(set(R.fixture_frames(L)) | {500})
        assert np.array_equal(got[0][fr], R.logmel(x, lm.W, fr, start=start, r=L))
    with pytest.raises(Exception):
        lm.query(x, start=n - L + 1)


@pytest.mark.parametrize("pos", [1, 511, 512, L - 2])
def test_impulse_tells_reflect_from_symmetric(lm, pos):
    x = np.zeros(L, np.float32)
    x[pos] = 0.5
    got = images(lm.chunks(x)[0])[0]
    fr = [0, 1, 2, 3] if pos < L // 2 else [997, 998, 999, 1000]
    want = R.logmel(x, lm.W, fr)
    assert np.array_equal(got[fr], want)
    assert (want > -100).any()
    far = [t for t in range(R.T) if abs(480 * t - pos) > 1500 and abs(480 * t - (2 * (L - 1) - pos)) > 1500]
    assert np.all(got[far] == -100.0)


def test_silence_and_below_floor(lm):
    got = images(lm.chunks([np.zeros(L, np.float32), np.zeros(100000, np.float32)])[0])
    assert got.shape[0] == 3 and np.all(got == np.float32(-100.0))
    x = (1e-7 * np.sin(2 * np.pi * 1000.0 * np.arange(L) / R.SR)).astype(np.float32)
    assert np.all(R.logmel(x, lm.W, [0, 500, 1000]) == -100.0)
    assert np.all(images(lm.chunks(x)[0]) == np.float32(-100.0))


def test_clip_at_the_end_of_its_allocation(lm):
    """The clip's last sample is the tensor's last element, f32 and s16, at an odd sample offset."""
    import torch

    n = 479800
    x = R.fixture_input(3)
    for fmt, host in (("f32", x), ("s16", np.round(x * 20000.0).astype(np.int16))):
        t = torch.from_numpy(np.concatenate([np.zeros(3, host.dtype), host])).cuda()
        out, meta = lm.chunks(t, lengths=[3, n], fmt=fmt)
        assert [(int(m["clip"]), int(m["start"])) for m in meta] == [(1, 0), (1, 240000)]
        ref = host if fmt == "f32" else R.s16_to_f32(host)
        check_chunks(images(out), meta, [None, ref], lm.W, lambda r, fill: set(R.fixture_frames(r)) | {992})


def test_custom_bank_equals_builtin(gpu_engine, clap, lm):
    x = R.fixture_input(0)
    a = images(lm.chunks(x)[0])
    m2 = clap.LogMel(gpu_engine, filters=lm.W)
    assert np.array_equal(m2.filters(), lm.W)
    b = images(m2.chunks(x)[0])
    assert np.array_equal(a, b)
    bad = lm.W.copy()
    bad[R.supports(lm.W)[0][30] + 1, 30] = 0  # a gap
    with pytest.raises(Exception):
        clap.LogMel(gpu_engine, filters=bad)
    clap.LogMel(gpu_engine)  # leave the engine on the default bank


def test_small_out_is_invalid_and_untouched(gpu_engine, lm, clap):
    import torch
    from aidfp import _lib

    x = R.fixture_input(1)  # 160001 samples twice -> 2 chunks
    pcm = np.concatenate([x, x])
    off, ln = np.array([0, len(x)], np.int64), np.array([len(x), len(x)], np.int64)
    out = torch.full((1, R.T, R.BANDS), 7.5, dtype=torch.float32, device="cuda")
    n = ctypes.c_int64(-1)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    rc = gpu_engine._lib.aid_logmel(gpu_engine._h, p(pcm), p(off), p(ln), 2, _lib.AID_PCM_HOST, 0, 0,
                                    ctypes.c_void_p(out.data_ptr()), 1, _lib.AID_PCM_DEVICE, None, ctypes.byref(n), None)
    assert rc == _lib.AID_ERR_INVALID and n.value == 2 and "capacity" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.5).all())
    host = np.full((2, R.T, R.BANDS), 7.5, np.float32)  # a host `out` of the right size is filled
    rc = gpu_engine._lib.aid_logmel(gpu_engine._h, p(pcm), p(off), p(ln), 2, _lib.AID_PCM_HOST, 0, 0, p(host), 2,
                                    _lib.AID_PCM_HOST, None, ctypes.byref(n), None)
    assert rc == 0 and n.value == 2 and np.array_equal(host[0], host[1])
    assert np.array_equal(host[0][[0, 333, 1000]], R.logmel(x, lm.W, [0, 333, 1000]))


def test_generate_chunked_embeddings_with_stub_model(lm, clap):
    """A fixed seeded linear map of the features on the device stands in for the model."""
    import torch

    n = 720000
    x = np.resize(R.fixture_input(2), n)
    g = torch.Generator().manual_seed(3)
    A = (torch.randn(R.T * R.BANDS, 32, generator=g) / 100.0).cuda()

    class Stub:
        def get_audio_features(self, input_features):
            assert input_features.is_cuda and input_features.shape[1:] == (1, R.T, R.BANDS)
            return input_features.reshape(input_features.shape[0], -1) @ A

    got = clap.generate_chunked_embeddings(x.tobytes(), Stub(), lm, batch=2)
    gold = json.loads((GOLD / "ref_clap_chunks.json").read_text())["chunks"][str(n)]
    assert [[c.offset_sec, c.chunk_index, c.duration_sec] for c in got] == gold and len(got) == 3
    plan = R.chunk_plan(n)
    feats = np.stack([R.logmel(x, lm.W, range(R.T), start=s, r=r) for s, r, *_ in plan])
    dev = torch.from_numpy(feats).cuda()[:, None]
    want = torch.cat([Stub().get_audio_features(dev[0:2]), Stub().get_audio_features(dev[2:3])]).cpu().numpy()
    assert np.array_equal(np.array([c.embedding for c in got], np.float32), want)  # the same batches of the same map
    assert np.array_equal(images(lm.chunks(x)[0]), feats)  # the features themselves: equal
    assert clap.chunk_plan(n) == [tuple(g_) for g_ in gold]
    e1 = clap.generate_embedding(x[:100000], Stub(), lm)
    assert e1.shape == (32,)
    fus, longer = lm.query(x[:100000], fusion=True)
    assert fus.shape == (1, 4, R.T, R.BANDS) and longer is False and bool((fus[:, 0] == fus[:, 3]).all())
