"""Every kernel form of K6 `resample` (audio-ident_amd/csrc/resample.hip) at its edges, bit for bit against the CPU
oracle (oracle/fp_resample.c on the same samples; int16 input as q / 32768, stereo downmixed as (xL + xR) * 0.5f).

tests/resample_cases.py is the case table: rate pairs that reach k_decimate, k_resample_phase at its block widths,
`t`-loop trips and largest windows, k_resample MODE 2 (integer decimation) and MODE 0 (per-lane phase rows).
tests/test_resample_plan_host.py proves on the CPU that each row runs the form it names, so a moved threshold fails
there instead of a case here sliding silently onto another kernel.

Every destination has NaN guard elements before and after the range a call may write, and every source buffer has
sentinel samples (far out of any signal's range) before and after the frames a call may read."""

import numpy as np
import pytest
import torch

import oracle as O
import resample_cases as RC
from s16_inputs import random_q, widen

pytestmark = pytest.mark.gpu
GUARD = 8  # floats; keeps dst + GUARD 16-byte aligned
KINDS = ("f32-mono", "f32-stereo", "s16-mono", "s16-stereo")
CASE_IDS = [c.id for c in RC.CASES]
MODE2, MODE0, DEC3, PHASE = RC.BY_ID["96000to16000"], RC.BY_ID["1031to1025"], RC.BY_ID["48000to16000"], \
    RC.BY_ID["256to257"]
ONE_PER_PATH = [MODE2, DEC3, PHASE, MODE0]


def _case(sr_in, sr_out):
    up, down, _, J = RC.ratio(sr_in, sr_out)
    return RC.Case(sr_in, sr_out, up, down, J, RC.launch_plan(up, down, J).path, "")


def _block(c):
    return RC.launch_plan(c.up, c.down, c.J).block


def _signal(kind, n, seed):
    stereo = kind.endswith("stereo")
    if kind.startswith("s16"):
        return random_q(n, seed, 2 if stereo else 1)
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 2) if stereo else n) * 0.4).astype(np.float32)


def _ref(c, data):
    """The oracle on the whole signal `data` ([n] or [n, 2], float32 or int16)."""
    if data.dtype == np.int16:
        x = widen(data)
        data = x if x.ndim == 1 else ((x[:, 0] + x[:, 1]) * np.float32(0.5)).astype(np.float32)
    return O.resample(data, c.sr_in, c.sr_out)


def _same(got, ref):
    return got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def _dev(data, lead=0):
    """`data` on the device, `lead` frames into a 16-byte aligned buffer, sentinels around it -> (tensor, pointer)."""
    ch = data.ndim
    sentinel = 32767 if data.dtype == np.int16 else 1e30
    buf = np.full((lead + len(data) + 8) * ch, sentinel, data.dtype)
    buf[lead * ch:(lead + len(data)) * ch] = data.reshape(-1)
    t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + lead * ch * data.dtype.itemsize


def _fmt(data):
    return "s16" if data.dtype == np.int16 else "f32"


def _run(eng, c, data, count, in_base=0, m_first=0, lead=0, dst_off=0, hist=None):
    """Outputs [m_first, m_first + count) from stream frames [in_base, in_base + n) = data (and, with hist, the
    frames just before them), through aid_resample_batch_split[_s16] with one stream."""
    keep, src = _dev(data, lead)
    hkeep, hptr = _dev(hist) if hist is not None and len(hist) else (None, 0)
    dst = torch.full((GUARD + dst_off + count + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    eng.resample_batch_split(hptr, 0, len(hist) if hptr else 0, src, 0, 1, in_base, len(data), data.ndim, c.sr_in,
                             c.sr_out, m_first, count, dst.data_ptr() + 4 * (GUARD + dst_off), 0, fmt=_fmt(data))
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert np.isnan(out[:GUARD + dst_off]).all() and np.isnan(out[GUARD + dst_off + count:]).all()
    return out[GUARD + dst_off:GUARD + dst_off + count]


def _whole(eng, c, data, lead=0):
    """aid_resample[_s16] of the whole signal."""
    keep, src = _dev(data, lead)
    m = eng.resample_len(len(data), c.sr_in, c.sr_out)
    dst = torch.full((GUARD + m + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    got = eng.resample(src, len(data), data.ndim, c.sr_in, c.sr_out, dst.data_ptr() + 4 * GUARD, m, fmt=_fmt(data))
    torch.cuda.synchronize()
    assert got == m
    out = dst.cpu().numpy()
    assert np.isnan(out[:GUARD]).all() and np.isnan(out[GUARD + m:]).all()
    return out[GUARD:GUARD + m]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cid", CASE_IDS)
def test_block_exact_counts_and_short_signals(gpu_engine, cid, kind):
    """1, B - 1, B, B + 1 and 2 B + 3 outputs (B = the row's outputs per workgroup): the whole-signal form where a
    signal of that many outputs exists, else the first `count` outputs of the shortest signal that has them. Then a
    5-frame signal (shorter than any filter here) and an empty one, which writes nothing."""
    c = RC.BY_ID[cid]
    B = _block(c)
    for i, cnt in enumerate((1, B - 1, B, B + 1, 2 * B + 3)):
        n = -(-cnt * c.down // c.up)  # the shortest signal with at least cnt outputs
        data = _signal(kind, n, 100 * CASE_IDS.index(cid) + i)
        if data.dtype == np.int16 and data.size >= 2:
            assert data.min() == -32768 and data.max() == 32767
        ref = _ref(c, data)
        assert len(ref) >= cnt
        got = _whole(gpu_engine, c, data) if len(ref) == cnt else _run(gpu_engine, c, data, cnt)
        assert _same(got, ref[:cnt]), (cid, kind, cnt)
    short = _signal(kind, 5, 7)
    assert len(short) < c.J  # every output's window reaches past both ends of the signal
    assert _same(_whole(gpu_engine, c, short), _ref(c, short)), (cid, kind)
    assert len(_whole(gpu_engine, c, _signal(kind, 0, 0))) == 0


LEADS = [("f32-mono", (0, 1, 2, 3)), ("f32-stereo", (0, 1)), ("s16-mono", (0, 1, 6)), ("s16-stereo", (0, 3))]


@pytest.mark.parametrize("kind,leads", LEADS, ids=[k for k, _ in LEADS])
@pytest.mark.parametrize("c", [MODE2, MODE0], ids=lambda c: c.id)
def test_load_paths(gpu_engine, c, kind, leads):
    """stage_window's 16-byte loads (source 16-byte aligned, interior blocks) and its single-frame loads (a source
    pointer 4, 8 or 12 bytes into a word; s16: 2 and 12 bytes) give the same outputs."""
    data = _signal(kind, -(-(2 * _block(c) + 3) * c.down // c.up), 11)
    ref = _ref(c, data)
    frame = data.ndim * data.dtype.itemsize
    for lead in leads:
        _, ptr = _dev(data, lead)
        assert (ptr % 16 == 0) == (lead == 0) and ptr % 16 == lead * frame % 16  # the offset breaks the alignment
        assert _same(_whole(gpu_engine, c, data, lead=lead), ref), (c.id, kind, lead)


@pytest.mark.parametrize("kind", ["f32-mono", "s16-stereo"])
def test_decimate3_dst_alignment(gpu_engine, kind):
    """k_decimate stores a thread's four outputs as one 16-byte word when the address allows it and all four exist,
    else one by one: dst 0..3 floats into a word, a first output that is not a multiple of 4, and counts that are
    not, so an aligned launch has both stores in it."""
    c = DEC3
    data = _signal(kind, 3 * (1021 + 2051 + 40), 13)
    ref = _ref(c, data)
    for dst_off in range(4):
        for m_first in (0, 1, 2, 3, 1021):
            for cnt in (5, 2051):
                assert cnt % 4 and (4 * (GUARD + dst_off) % 16 == 0) == (dst_off == 0)
                got = _run(gpu_engine, c, data, cnt, m_first=m_first, dst_off=dst_off)
                assert _same(got, ref[m_first:m_first + cnt]), (kind, dst_off, m_first, cnt)


@pytest.mark.parametrize("kind", ["f32-stereo", "s16-mono"])
@pytest.mark.parametrize("c", ONE_PER_PATH, ids=lambda c: c.id)
def test_range_chunks_equal_whole(gpu_engine, c, kind):
    """The output cut into ~10 random chunks, each computed from only the input frames it reads (the streaming range
    form), equals the oracle on the whole signal."""
    B = _block(c)
    up, down, hl, J = RC.ratio(c.sr_in, c.sr_out)
    data = _signal(kind, -(-(5 * B + 17) * down // up), 17)
    ref = _ref(c, data)
    rng = np.random.default_rng(B)
    cuts = sorted(set(rng.integers(1, len(ref), size=10).tolist())) + [len(ref)]
    assert any(m % B for m in cuts[:-1])
    out = np.full(len(ref), np.nan, np.float32)
    m = 0
    for end in cuts:
        lo = max(0, (m * down + hl) // up - (J - 1))  # first input the chunk reads
        hi = min(len(data), ((end - 1) * down + hl) // up + 1)  # one past the last
        out[m:end] = _run(gpu_engine, c, data[lo:hi], end - m, in_base=lo, m_first=m)
        m = end
    assert _same(out, ref), (c.id, kind)


@pytest.mark.parametrize("kind", ["f32-mono", "f32-stereo"])
@pytest.mark.parametrize("c", [MODE2, MODE0], ids=lambda c: c.id)
def test_split_input_across_the_seam(gpu_engine, c, kind):
    """aid_resample_batch_split: the last h frames before frame k as the history part, the frames from k on as the
    chunk, for h = 0, 1, J - 1 and J + 5. Every output whose window starts at or after frame k - h, the ones whose
    windows straddle the seam included, equals the whole-signal oracle result."""
    up, down, hl, J = RC.ratio(c.sr_in, c.sr_out)
    k = 3001
    data = _signal(kind, k + -(-(2 * _block(c) + 300) * down // up), 19)
    ref = _ref(c, data)
    for h in (0, 1, J - 1, J + 5):
        m0 = -(-((k - h + J - 1) * up - hl) // down)  # first output whose window starts at or after frame k - h
        first_after = -(-((k + J - 1) * up - hl) // down)  # first output that reads the chunk alone
        assert (m0 < first_after) == (h > 0) and first_after < len(ref)
        got = _run(gpu_engine, c, data[k:], len(ref) - m0, in_base=k, m_first=m0, hist=data[k - h:k])
        assert _same(got, ref[m0:]), (c.id, kind, h)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", [MODE2, MODE0], ids=lambda c: c.id)
def test_five_streams_in_one_launch(gpu_engine, c, kind):
    """5 streams of different data in one launch, their bases alternately 16-byte aligned and 8 bytes off: each equals
    its own oracle result, and the gaps between them in dst stay NaN."""
    S = 5
    probe = _signal(kind, 1, 0)
    ch, item = probe.ndim, probe.dtype.itemsize
    n = -(-(2 * _block(c) + 3) * c.down // c.up)
    stride = n * ch + 1
    while stride * item % 16 != 8 or stride % 2:
        stride += 1
    x = np.full((S, stride), 32767 if item == 2 else 1e30, probe.dtype)
    streams = [_signal(kind, n, 23 + i) for i in range(S)]
    for i, d in enumerate(streams):
        x[i, :n * ch] = d.reshape(-1)
    src = torch.from_numpy(x).cuda()
    assert [src[i].data_ptr() % 16 for i in range(S)] == [0, 8, 0, 8, 0]
    cnt = gpu_engine.resample_len(n, c.sr_in, c.sr_out)
    dst = torch.full((GUARD + S * (cnt + 3) + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    gpu_engine.resample_batch_split(0, 0, 0, src.data_ptr(), stride, S, 0, n, ch, c.sr_in, c.sr_out, 0, cnt,
                                    dst.data_ptr() + 4 * GUARD, cnt + 3, fmt="s16" if item == 2 else "f32")
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert np.isnan(out[:GUARD]).all() and np.isnan(out[-GUARD:]).all()
    got = out[GUARD:-GUARD].reshape(S, cnt + 3)
    for i, d in enumerate(streams):
        assert _same(got[i, :cnt], _ref(c, d)), (c.id, kind, i)
        assert np.isnan(got[i, cnt:]).all()


FAR = [(48000, 16000), (48000, 44100), (2, 1), (1, 1025)]  # decimate3, phase, MODE 2, MODE 0


@pytest.mark.parametrize("kind", ["f32-stereo", "s16-mono"])
@pytest.mark.parametrize("sr_in,sr_out", FAR)
def test_stream_positions_past_2_to_the_31(gpu_engine, sr_in, sr_out, kind):
    """A short signal x placed at stream frame in_base = k * down, its outputs asked for from m_first = k * up, with
    k * down > 2^33 (a 48 kHz stream passes 2^31 frames after 12.4 hours). The reference is the oracle on x at base 0,
    and the equality is exact by construction: output m reads phase (m * down + hl) % up and the inputs
    (m * down + hl) / up - j. Adding k * up to m adds k * up * down to m * down + hl, which leaves the phase unchanged
    and adds exactly k * down to the input index; samples outside [in_base, in_base + n) are zero for the kernel as
    samples outside [0, n) are for the oracle. Once as the range form, once with the first J + 3 frames as the
    history part of the split form."""
    c = _case(sr_in, sr_out)
    assert c.path == {16000: RC.DECIMATE3, 44100: RC.PHASE, 1: RC.UNIFORM, 1025: RC.GLOBAL_TAPS}[sr_out]
    k = (1 << 33) // c.down + 12345
    assert k * c.down > 1 << 33 and k * c.up > 1 << 31  # input and output positions both past 32 bits
    data = _signal(kind, max(-(-(2 * _block(c) + 3) * c.down // c.up), 3 * c.J) + 5, 29)
    ref = _ref(c, data)
    assert len(ref) > 2 * _block(c)
    got = _run(gpu_engine, c, data, len(ref), in_base=k * c.down, m_first=k * c.up)
    assert _same(got, ref), (sr_in, sr_out, kind)
    h = c.J + 3
    got = _run(gpu_engine, c, data[h:], len(ref), in_base=k * c.down + h, m_first=k * c.up, hist=data[:h])
    assert _same(got, ref), (sr_in, sr_out, kind, "split")


def _window_holds(c, n_out, idx):
    """Per output, whether one of the input indices `idx` lies in its window [c / up - (J - 1), c / up]."""
    up, down, hl, J = RC.ratio(c.sr_in, c.sr_out)
    i0 = (np.arange(n_out, dtype=np.int64) * down + hl) // up
    return np.any([(i0 - (J - 1) <= i) & (i <= i0) for i in idx], axis=0)


@pytest.mark.parametrize("c", ONE_PER_PATH, ids=lambda c: c.id)
def test_values(gpu_engine, c):
    """All zeros; +0 and -0 mixed; inputs in the subnormal range (1e-43 <= |x| <= 1e-38: the oracle is the
    specification, FPSPEC 8, so they are neither flushed nor rounded differently); one NaN and one +Inf."""
    n = -(-(2 * _block(c) + 3) * c.down // c.up)
    rng = np.random.default_rng(31)
    zeros = np.zeros(n, np.float32)
    signed = np.where(rng.integers(0, 2, n) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    assert np.signbit(signed).any() and not np.signbit(signed).all()
    tiny = (10.0 ** rng.uniform(-43, -38, n) * rng.choice((-1.0, 1.0), n)).astype(np.float32)
    assert (tiny != 0).all() and (np.abs(tiny) < np.finfo(np.float32).tiny).mean() > 0.5
    for x in (zeros, signed, tiny):
        ref = _ref(c, x)
        assert _same(_whole(gpu_engine, c, x), ref), c.id
    assert np.any(_ref(c, tiny) != 0)
    x = (rng.standard_normal(n) * 0.4).astype(np.float32)
    a, b = n // 4, 3 * n // 4
    x[a], x[b] = np.nan, np.inf
    ref, got = _ref(c, x), _whole(gpu_engine, c, x)
    hit = _window_holds(c, len(ref), (a, b))
    assert hit.any() and (~hit).any() and np.isnan(ref).any() and np.isinf(ref).any()
    assert np.isfinite(ref[~hit]).all() and _same(got[~hit], ref[~hit])
    assert np.array_equal(np.isnan(got), np.isnan(ref))  # NaN payloads need not match
    assert _same(got[~np.isnan(ref)], ref[~np.isnan(ref)])


def test_rejections(gpu_engine):
    """A window above 64 KB of LDS and a tap table above 2^24 floats are refused with AID_ERR_INVALID before anything
    is written; their nearest accepted neighbours run. (473 -> 2 is accepted: tests/test_resample_plan_host.py.)"""
    from aidfp._lib import AID_ERR_INVALID, EngineError

    for kind in ("f32-mono", "s16-stereo"):
        data = _signal(kind, 64, 37)
        for sr_in, sr_out, _ in RC.REFUSED:
            keep, src = _dev(data)
            dst = torch.full((GUARD + 4 + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
            with pytest.raises(EngineError) as e:
                gpu_engine.resample_batch_split(0, 0, 0, src, 0, 1, 0, len(data), data.ndim, sr_in, sr_out, 0, 4,
                                                dst.data_ptr() + 4 * GUARD, 0, fmt=_fmt(data))
            assert e.value.code == AID_ERR_INVALID, (sr_in, sr_out)
            torch.cuda.synchronize()
            assert np.isnan(dst.cpu().numpy()).all()
        for sr_in, sr_out in RC.ACCEPTED_NEIGHBOURS:
            c = _case(sr_in, sr_out)
            assert _same(_whole(gpu_engine, c, data), _ref(c, data)), (sr_in, sr_out, kind)
