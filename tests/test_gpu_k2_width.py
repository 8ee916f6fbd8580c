"""K2 workgroup width (peaks.hip k_peak_pick<W>, aid_engine_force K2_WIDTH): 2-wave workgroups own bins 0..511 and
walk a strip a second time over bins 512..1023 when its upper half is hot; 4-wave workgroups own the whole row.
Every width and strip multiplier gives the oracle's peaks and hashes bit for bit, on inputs built around the
bin-512 boundary between the two column groups.

Clips are 3 s (255 frames). At 1 and 3 strips per resident slot a handful of them gets the shortest strip (16
rows, so 16 strips per clip and many strip edges); 0.01 strips per slot gives strips of 90 rows and more, whose
length differs between the widths.
"""

import functools

import numpy as np
import pytest

import oracle as O
from aidfp import synth
from aidfp.engine import Engine, peaks_from_mask

pytestmark = pytest.mark.gpu
SR = 44100
HOP = 512
N = SR * 3
WIDTHS = [2, 4]
X100 = [100, 300, 1]


def _am_tones(rng, bins, n=N, amp=0.05):
    """AM tones at FFT bins `bins` over a 1e-4 noise floor (as test_gpu_extract's band-limited quarters)."""
    t = np.arange(n) / SR
    x = np.zeros(n)
    for k in bins:
        am = 0.5 + 0.5 * np.sin(2 * np.pi * rng.uniform(1, 4) * t + rng.uniform(0, 6))
        x += amp * am * np.sin(2 * np.pi * (k * SR / 2048.0) * t + rng.uniform(0, 6))
    return x + rng.standard_normal(n) * 1e-4


def _f32(x):
    return np.clip(x, -1, 1).astype(np.float32)


def _burst(x, k, onset_frame, seconds=0.3, amp=0.05):
    """Adds a tone burst at bin k whose first sample is the first one that only frame `onset_frame` on reads."""
    a = (onset_frame - 1) * HOP + 2048
    m = int(seconds * SR)
    t = np.arange(m) / SR
    x[a:a + m] += amp * np.hanning(m) * np.sin(2 * np.pi * (k * SR / 2048.0) * t)
    return x


@functools.lru_cache(maxsize=None)
def _case(name):
    """(clips, reference peaks, reference hashes, sides) of a case, computed once; sides[c] = (below, above): whether
    the clip must have peaks below / at or above bin 512."""
    rng = np.random.default_rng(11)
    if name == "straddle":
        sets = [[505, 519], [496], [511, 513], [512], [527, 528], [250, 262]]
        clips = [_f32(_am_tones(rng, b)) for b in sets]
        sides = [(True, True), (True, False), (True, True), (False, True), (False, True), (True, False)]
    elif name == "partial":
        clips, sides = [], []
        for onset in (100, 105, 110, 115, 121):  # onsets at 4, 9, 14, 3 and 9 rows into a 16-row strip
            x = synth.synth(20 + onset, 0, N, SR, salt=7).astype(np.float64)
            x = _burst(x, 700, onset)
            x = _burst(x, 520, onset + 60)  # chunk 32: the lower group's boundary pad
            clips.append(_f32(x))
            sides.append((True, True))
    elif name == "fullband":
        clips = [synth.synth(40 + i, 1000 * i, N + 313 * i, SR, snr_db=None if i % 2 else 20, salt=7, fmax_hz=20000)
                 for i in range(6)]
        sides = [(True, True)] * 6
    elif name == "nonfinite":
        a = _f32(_am_tones(rng, [510, 514]) + synth.synth(41, 0, N, SR, snr_db=20, salt=7))
        a[[5000, 70000, 120001]] = [np.nan, np.inf, -np.inf]
        b = _f32(_am_tones(rng, [505, 519], amp=0.2)) * np.float32(3e18)  # inf powers around bin 512
        c = np.zeros(N, np.float32)  # flat, exactly tied spectrum: equal powers on both sides of bin 512
        c[::512] = 8.0
        c[256::1024] = -4.0
        d = (rng.integers(-3, 4, N) / 4).astype(np.float32)  # coarse values, many equal powers, full band
        clips = [a, b, c, d]
        sides = [(True, True), (False, False), (False, False), (True, True)]
    else:
        raise KeyError(name)
    peaks = [O.peaks(O.stft_power(x, HOP)).reshape(-1, 2) for x in clips]
    hashes = [O.fingerprint(x, HOP) for x in clips]
    for c, (pk, (below, above)) in enumerate(zip(peaks, sides)):  # a case without peaks where it aims proves nothing
        assert not below or np.any(pk[:, 1] < 512), f"{name} clip {c}: no reference peak below bin 512"
        assert not above or np.any(pk[:, 1] >= 512), f"{name} clip {c}: no reference peak at or above bin 512"
    return clips, peaks, hashes


@pytest.fixture(scope="module")
def eng():
    with Engine(SR) as e:
        yield e


def _check(e, name, width=None):
    clips, peaks, hashes = _case(name)
    got = e.extract_host(clips)
    if width is not None:
        assert e.match_stats()["k2_width"] == width
    for c, x in enumerate(clips):
        pk = peaks_from_mask(e.peakmask(c, len(x)))
        assert np.array_equal(pk, peaks[c]), f"{name} clip {c}: peaks differ"
        assert np.array_equal(got[c], hashes[c]), f"{name} clip {c}: hashes differ"


@pytest.mark.parametrize("x100", X100)
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("name", ["straddle", "partial", "fullband", "nonfinite"])
def test_width_bit_exact(eng, name, width, x100):
    """straddle: tones within 15 bins of each other across bin 512 (one suppresses the other through the boundary
    pad), on and beside it, and a control inside the lower group. partial: band-limited clips with a 0.3 s burst at
    bin 700 (strips before its onset take the second walk for a halo row only) and one at bin 520 (seen by the lower
    group through its boundary pad only). fullband: every strip is walked twice. nonfinite: NaN / inf samples, inf
    powers and exactly tied powers around bin 512."""
    try:
        eng.force("k2_width", width)
        eng.force("k2_strips_x100", x100)
        _check(eng, name, width)
    finally:
        eng.force("k2_width", 0)
        eng.force("k2_strips_x100", 0)


def test_width_adapts():
    """No history: width 4. Band-limited calls move the engine to width 2 (the cold-wave count of a width-4 call says
    that no strip needs a second walk); full-band calls bring it back to 4 once a width-2 call has counted the strips
    it walked twice. The counts are read without a sync, here one call late at most, as every call's results are
    fetched before the next. Every call, those around the switches included, gives the oracle's results."""
    band = [_f32(_am_tones(np.random.default_rng(3 + i), [40 + 37 * i, 300 + 20 * i])) for i in range(6)]
    band_pk = [O.peaks(O.stft_power(x, HOP)).reshape(-1, 2) for x in band]
    band_h = [O.fingerprint(x, HOP) for x in band]
    full, full_pk, full_h = _case("fullband")

    def call(e, clips, pks, hs):
        got = e.extract_host(clips)
        for c, x in enumerate(clips):
            assert np.array_equal(peaks_from_mask(e.peakmask(c, len(x))), pks[c]), f"clip {c}: peaks differ"
            assert np.array_equal(got[c], hs[c]), f"clip {c}: hashes differ"
        return e.match_stats()["k2_width"]

    with Engine(SR) as e:
        widths = [call(e, band, band_pk, band_h) for _ in range(8)]
        assert widths[0] == 4 and widths[-1] == 2, widths
        widths = [call(e, full, full_pk, full_h) for _ in range(3)]
        assert widths[-1] == 4, widths  # back within 3 calls
        widths = [call(e, band, band_pk, band_h) for _ in range(3)]
        assert widths == [4, 4, 4], widths  # held at 4 for a while after the fall-back: no flapping
