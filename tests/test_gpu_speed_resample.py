"""K6s, aid_resample_speeds and its int16 form aid_resample_s16_speeds (spec/FPSPEC.md 8.2): every speed variant of
every clip of one call is bit-equal to the CPU oracle's resample of that clip for the rate pair (sr_in * 1000, 16000 * (1000 + pm)).

Clip lengths 1, 60, 1023, 1024, 1025 and 16001 are mixed within one call (a variant of one block, of exactly one, of
one and a sample, and of several; clips shorter than a filter), the clips start at frame 3 of the device buffer, so
some start at an odd sample, and the speeds (-40, -1, 0, 1, 7, 40) include up == down (16 kHz mono at speed 0) and
the large-up pair of 44.1 kHz at speed 7 (up 4,028)."""

import numpy as np
import pytest
import torch

import oracle as O
from aidfp import _lib
from aidfp._lib import EngineError
from aidfp.engine import Engine
from s16_inputs import random_q, widen

pytestmark = pytest.mark.gpu
SR_E = 16000
LENS = [1, 60, 1023, 1024, 1025, 16001]
SPEEDS = (-40, -1, 0, 1, 7, 40)
FIRST = 3  # the first clip's frame in the device buffer
GUARD = 256  # floats behind the output, which no call may touch
SETUPS = [(48000, 2), (16000, 1), (44100, 1)]


@pytest.fixture(scope="module")
def eng():
    e = Engine(SR_E)
    yield e
    e.close()


def make_input(lens, channels, fmt, seed):
    """(host array of FIRST + sum(lens) frames, offsets): the clips back to back from frame FIRST on."""
    n = FIRST + sum(lens)
    if fmt == "s16":
        buf = random_q(n, seed, channels)
    else:
        rng = np.random.default_rng(seed)
        buf = rng.uniform(-1.0, 1.0, n if channels == 1 else (n, channels)).astype(np.float32)
    return buf, np.cumsum([FIRST] + list(lens)).astype(np.int64)


def expected(buf, offsets, sr_in, speeds, fmt):
    x = widen(buf) if fmt == "s16" else buf
    return [O.resample(x[offsets[c]:offsets[c + 1]], sr_in * 1000, SR_E * (1000 + pm))
            for c in range(len(offsets) - 1) for pm in speeds]


def run_call(eng, buf, offsets, channels, sr_in, speeds, fmt, cap=None):
    """One call into a guarded device buffer; returns (dst_offsets, the whole buffer back on the host, total)."""
    total = sum(eng.speed_len(int(offsets[c + 1] - offsets[c]), sr_in, pm) for c in range(len(offsets) - 1)
                for pm in speeds)
    dev = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    dst = torch.full((total + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    off = eng.resample_speeds(dev.data_ptr(), offsets, channels, sr_in, speeds, dst.data_ptr(),
                              total if cap is None else cap, fmt=fmt)
    torch.cuda.synchronize()
    return off, dst.cpu().numpy(), total


@pytest.mark.parametrize("fmt", ["f32", "s16"])
@pytest.mark.parametrize("sr_in,channels", SETUPS)
def test_every_pair_bit_equal(eng, sr_in, channels, fmt):
    buf, offsets = make_input(LENS, channels, fmt, 100 + sr_in // 1000 + channels)
    assert any(int(o) % 2 for o in offsets[:-1]) and any(int(o) % 2 == 0 for o in offsets[:-1])
    want = expected(buf, offsets, sr_in, SPEEDS, fmt)
    off, got, total = run_call(eng, buf, offsets, channels, sr_in, SPEEDS, fmt)
    assert off[0] == 0 and off[-1] == total == sum(len(w) for w in want)
    assert np.isnan(got[total:]).all()  # nothing written past the packed variants
    for k, w in enumerate(want):
        c, v = divmod(k, len(SPEEDS))
        g = got[off[k]:off[k + 1]]
        assert len(g) == len(w), (c, SPEEDS[v])
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), f"clip {c} speed {SPEEDS[v]}: bits differ"
    if sr_in == SR_E:  # speed 0 there is up == down: the samples themselves
        x = widen(buf) if fmt == "s16" else buf
        k = 5 * len(SPEEDS) + SPEEDS.index(0)
        assert np.array_equal(got[off[k]:off[k + 1]], x[offsets[5]:offsets[6]])


@pytest.mark.parametrize("fmt", ["f32", "s16"])
def test_one_speed_one_clip(eng, fmt):
    for lens, speeds in (([16001], (7,)), ([1025, 60], (-40,)), ([4000], SPEEDS)):
        buf, offsets = make_input(lens, 2, fmt, 7 + len(lens))
        want = expected(buf, offsets, 48000, speeds, fmt)
        off, got, total = run_call(eng, buf, offsets, 2, 48000, speeds, fmt)
        assert len(off) == len(lens) * len(speeds) + 1 and off[-1] == total
        for k, w in enumerate(want):
            assert np.array_equal(got[off[k]:off[k + 1]].view(np.uint32), w.view(np.uint32)), k
        assert np.isnan(got[total:]).all()


@pytest.mark.parametrize("fmt", ["f32", "s16"])
def test_cap_one_short(eng, fmt):
    buf, offsets = make_input(LENS, 1, fmt, 31)
    total = sum(eng.speed_len(n, 44100, pm) for n in LENS for pm in SPEEDS)
    with pytest.raises(EngineError) as err:
        run_call(eng, buf, offsets, 1, 44100, SPEEDS, fmt, cap=total - 1)
    assert err.value.code == _lib.AID_ERR_INVALID and "capacity" in str(err.value)
    # the refused call launched nothing: a guard pattern over the whole buffer stays as it was
    dev = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    dst = torch.full((total + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    off = np.zeros(len(LENS) * len(SPEEDS) + 1, np.int64)
    pm = np.asarray(SPEEDS, np.int32)
    fn = eng._fn("aid_resample_speeds", fmt)
    rc = fn(eng._h, dev.data_ptr(), offsets.ctypes.data, len(LENS), 1, 44100, pm.ctypes.data, len(pm), dst.data_ptr(),
            total - 1, off.ctypes.data, None)
    torch.cuda.synchronize()
    assert rc == _lib.AID_ERR_INVALID
    assert off[-1] == total  # the offsets are written all the same: their last entry is the capacity needed
    assert np.isnan(dst.cpu().numpy()).all()
    # and with the full capacity the same buffer is filled up to `total` and no further
    rc = fn(eng._h, dev.data_ptr(), offsets.ctypes.data, len(LENS), 1, 44100, pm.ctypes.data, len(pm), dst.data_ptr(),
            total, off.ctypes.data, None)
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert rc == 0 and not np.isnan(out[:total]).any() and np.isnan(out[total:]).all()


def test_rejections(eng):
    buf, offsets = make_input([100], 1, "f32", 1)
    dev = torch.from_numpy(buf).cuda()
    dst = torch.zeros(4096, dtype=torch.float32, device="cuda")
    for kw in (dict(speeds=()), dict(speeds=tuple(range(257))), dict(speeds=(0, -501)), dict(speeds=(1001,)),
               dict(sr_in=0), dict(sr_in=2147484), dict(channels=3), dict(sr_in=384000, speeds=(-500,))):
        a = dict(dict(speeds=(0,), sr_in=48000, channels=1), **kw)
        with pytest.raises(EngineError) as err:
            eng.resample_speeds(dev.data_ptr(), offsets, a["channels"], a["sr_in"], a["speeds"], dst.data_ptr(), 4096)
        assert err.value.code == _lib.AID_ERR_INVALID, kw
    with pytest.raises(EngineError):  # a stereo float frame is one 8-byte word
        eng.resample_speeds(dev.data_ptr() + 4, offsets, 2, 48000, (0,), dst.data_ptr(), 4096)
    assert eng.speed_plan(44100, 7)[0] == 4028 and eng.speed_len(80000, SR_E, 40) == 83200
    with pytest.raises(ValueError):
        eng.speed_plan(48000, -501)
