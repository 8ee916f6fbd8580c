"""K6 over native int16 PCM (aid_resample_s16, aid_resample_batch_split_s16; spec/FPSPEC.md 8): bit-exact against
oracle/fp_resample.c applied to q / 32768, stereo downmixed on the host first as (xL + xR) * 0.5f."""

import numpy as np
import pytest
import torch

import oracle as O
from s16_inputs import random_q, square_q, widen

pytestmark = pytest.mark.gpu
N = 20011  # frames: odd, and several blocks of every kernel (1024, kDecR * 256 and up * 16 outputs per block)


def _mono(q: np.ndarray) -> np.ndarray:
    """The oracle's input: the converted samples, stereo downmixed."""
    x = widen(q)
    return x if x.ndim == 1 else ((x[:, 0] + x[:, 1]) * np.float32(0.5)).astype(np.float32)


def _inputs(stereo: bool, seed: int):
    if not stereo:
        return [random_q(N, seed), square_q(N, 23)]
    sq = np.stack([square_q(N, 23), np.roll(square_q(N, 31), 5)], axis=1)  # reaches -65536 and 65534 before * 0.5
    return [random_q(N, seed, 2), sq]


def _gpu(eng, q, sr_in, sr_out, lead=0):
    """aid_resample_s16 of q, read `lead` frames into a device buffer (lead = 0: 16-B aligned)."""
    ch = 1 if q.ndim == 1 else 2
    buf = np.zeros((lead + len(q)) * ch, np.int16)
    buf[lead * ch:] = q.reshape(-1)
    src = torch.from_numpy(buf).cuda()
    m = eng.resample_len(len(q), sr_in, sr_out)
    dst = torch.full((m,), float("nan"), dtype=torch.float32, device="cuda")
    got = eng.resample(src.data_ptr() + 2 * lead * ch, len(q), ch, sr_in, sr_out, dst.data_ptr(), m, fmt="s16")
    torch.cuda.synchronize()
    assert got == m
    return dst.cpu().numpy()


@pytest.mark.parametrize("sr_in,sr_out,stereo", [(48000, 16000, False), (48000, 16000, True), (44100, 16000, False),
                                                 (44100, 16000, True), (44100, 48000, False), (44100, 48000, True),
                                                 (16000, 16000, True), (16000, 16000, False)])
def test_rate_pairs_bit_exact(gpu_engine, sr_in, sr_out, stereo):
    for q in _inputs(stereo, sr_in + sr_out):
        assert q.min() == -32768 and q.max() == 32767
        ref = O.resample(_mono(q), sr_in, sr_out)
        got = _gpu(gpu_engine, q, sr_in, sr_out)
        assert got.shape == ref.shape
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (sr_in, sr_out, stereo)


@pytest.mark.parametrize("stereo,lead", [(True, 3), (False, 1), (False, 6)])
def test_fallback_load_path(gpu_engine, stereo, lead):
    """The same 48 -> 16 kHz input behind a source pointer that is not 16-byte aligned (stereo: 3 frames = 12 bytes
    in; mono: 2 and 12 bytes in): the single-frame loads are taken instead of the 16-byte ones."""
    for q in _inputs(stereo, 48000 + 16000):
        ref = O.resample(_mono(q), 48000, 16000)
        got = _gpu(gpu_engine, q, 48000, 16000, lead=lead)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (stereo, lead)


@pytest.mark.parametrize("sr_in,sr_out,ch", [(48000, 16000, 2), (44100, 16000, 1), (48000, 44100, 2)])
def test_batch_split_equals_whole_signal(gpu_engine, sr_in, sr_out, ch):
    """3 streams, the input in two parts (300 history frames, then the chunk read in place from a longer buffer,
    some streams 16-byte aligned and some not): the outputs whose windows straddle the seam, and all after them,
    equal the whole-signal oracle result sliced."""
    up, down, hl, J = gpu_engine.resample_plan(sr_in, sr_out)
    S, n_all, k, h = 3, 20000, 10000, 300
    q = random_q(S * n_all, 5 + sr_in, ch).reshape(S, n_all * ch)
    q[1] = np.stack([square_q(n_all, 41)] * ch, axis=1).reshape(-1) if ch == 2 else square_q(n_all, 41)
    x = np.zeros((S, n_all * ch + 4), np.int16)  # stride > one stream's samples
    x[:, : n_all * ch] = q
    whole = torch.from_numpy(x).cuda()
    hist = torch.from_numpy(np.ascontiguousarray(x[:, (k - h) * ch: k * ch])).cuda()
    cur = whole[:, k * ch:]  # in place: a strided view of the whole input
    assert {(cur[i].data_ptr() % 16 == 0) for i in range(S)} == {True, False}
    m0 = -(-((k - h + J - 1) * up - hl) // down)  # first output whose window starts at or after frame k - h
    cnt = (n_all * up - 1 - hl) // down + 1 - m0   # through the last output with its inputs in range
    first_after = -(-((k + J - 1) * up - hl) // down)  # first output that reads the chunk alone
    assert m0 < first_after < m0 + cnt
    out = torch.full((S, cnt + 3), float("nan"), dtype=torch.float32, device="cuda")
    gpu_engine.resample_batch_split(hist.data_ptr(), h * ch, h, cur.data_ptr(), x.shape[1], S, k, n_all - k, ch,
                                    sr_in, sr_out, m0, cnt, out.data_ptr(), cnt + 3, fmt="s16")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i in range(S):
        qi = q[i].reshape(n_all, ch) if ch == 2 else q[i]
        ref = O.resample(_mono(qi), sr_in, sr_out)[m0:m0 + cnt]
        assert np.array_equal(got[i, :cnt].view(np.uint32), ref.view(np.uint32)), (sr_in, sr_out, ch, i)
        assert np.isnan(got[i, cnt:]).all()
