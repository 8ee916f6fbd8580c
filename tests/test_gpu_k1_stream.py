"""K1's real-split tail (csrc/stft.hip, aidfp_hotword.h): the packed hot word, the bit-tested store guards, mirror
store 0 whose lane 0 carries bin 512, and the K1_WAVES knob that makes small calls split the way large ones do (waves
that cross clip edges, waves with two frames). Every case runs twice against the oracle, bit for bit: with
keep_power (the power plane: every block stored, every bin's bits) and without (peaks, records and counts: a hot
chunk whose store or hot bit got lost loses its peaks).

NaN powers: FPSPEC pins no NaN payload, so the plane must hold a NaN exactly where the oracle's does and the
oracle's bits everywhere else.
"""

import functools

import numpy as np
import pytest
import torch

import oracle as O
from aidfp import synth
from aidfp.engine import Engine, peaks_from_mask
from s16_inputs import random_q, synth_q, widen

pytestmark = pytest.mark.gpu
SR = 44100
HOP = 512


def _n(frames, hop=HOP):
    return 2048 + hop * (frames - 1) if frames > 0 else 100


def _same_power(P, R):
    nan = np.isnan(R)
    return P.shape == R.shape and np.array_equal(np.isnan(P), nan) and \
        np.array_equal(P.view(np.uint32)[~nan], R.view(np.uint32)[~nan])


def _ref(x, hop, thr=None):
    x = np.ascontiguousarray(x, dtype=np.float32)
    P = O.stft_power(x, hop)
    if len(x) < 2048:
        return P, np.zeros((0, 2), np.int32), np.zeros(0, np.uint64)
    if thr is None:
        return P, O.peaks(P).reshape(-1, 2), O.fingerprint(x, hop)
    return P, O.peaks(P, thr).reshape(-1, 2), O.fingerprint(x, hop, thr)


def _check_engine(e, keep, clips, refs, run, what):
    run(e)
    counts = e.counts()
    for c, (x, (P, pk, rec)) in enumerate(zip(clips, refs)):
        if keep:
            assert _same_power(e.power(c, len(x)), P), f"{what} clip {c}: power bits differ"
        assert np.array_equal(peaks_from_mask(e.peakmask(c, len(x))), pk), f"{what} clip {c}: peaks differ"
        assert np.array_equal(e.hashes(c), rec), f"{what} clip {c}: records differ"
        assert counts[c] == len(rec), f"{what} clip {c}: count differs"


def _check(clips, refs, hop=HOP, waves=(0,), fmt="f32", run=None, **kw):
    """`clips` as the call takes them, `refs` = _ref of what they mean as float32. Both keep modes, every wave count."""
    wide = [widen(q) if fmt == "s16" else q for q in clips]
    for keep in (True, False):
        with Engine(SR, hop=hop, keep_power=keep, **kw) as e:
            for w in waves:
                e.force("k1_waves", w)
                _check_engine(e, keep, wide, refs, run or (lambda e: e.extract_host(clips, fmt=fmt)),
                              f"keep {keep} waves {w}")


# ---- uniform calls at every wave count: 4 waves cross clip edges, 24 get 5 or 6 frames (3 x 41) or share clips
# (8 x 5: 40 frames, 20 waves of 2), the default spreads 2 frames per wave
@functools.lru_cache(maxsize=None)
def _uniform(n_clips, frames, hop=HOP):
    clips = [synth.synth(30 + i, 700 * i, _n(frames, hop), SR, snr_db=20 if i % 2 else None, salt=frames) for i in range(n_clips)]
    refs = [_ref(x, hop) for x in clips]
    assert sum(len(r[2]) for r in refs) > 0
    return clips, refs


@pytest.mark.parametrize("n_clips,frames", [(3, 41), (8, 5)])
def test_uniform_calls(n_clips, frames):
    clips, refs = _uniform(n_clips, frames)
    assert all(O.num_frames(len(x), HOP) == frames for x in clips)
    _check(clips, refs, waves=(4, 24, 0))


def test_non_uniform_call():
    """Clips of 0, 1, 17 and 300 frames: ranges cross edges of clips of very different lengths, and a frameless clip
    lies between two of them."""
    frames = [17, 0, 1, 300]
    clips = [synth.synth(50 + i, 0, _n(f), SR, snr_db=20, salt=2) for i, f in enumerate(frames)]
    assert [O.num_frames(len(x), HOP) for x in clips] == frames
    _check(clips, [_ref(x, HOP) for x in clips], waves=(4, 24, 0))


def test_odd_sample_offset():
    """Device PCM read in place, the second and third clips starting at odd samples."""
    n = _n(41)
    clips = [synth.synth(60 + i, 0, n, SR, snr_db=20, salt=4) for i in range(3)]
    offs = np.array([0, n + 1, 2 * n + 3, 3 * n + 3], np.int64)
    buf = np.zeros(int(offs[-1]), np.float32)
    for x, o in zip(clips, offs):
        buf[o:o + n] = x
    parts = [buf[offs[c]:offs[c + 1]] for c in range(3)]  # the gaps' zeros belong to the clips
    dev = torch.from_numpy(buf).cuda()

    def run(e):
        e.extract_device(dev.data_ptr(), offs)
        e.sync()

    _check(parts, [_ref(x, HOP) for x in parts], waves=(4, 0), run=run)


def test_s16():
    n = _n(41)
    clips = [synth_q(70, 0, n, SR, snr_db=20, salt=5), random_q(n, 11), synth_q(71, 999, n, SR, salt=6)]
    _check(clips, [_ref(widen(q), HOP) for q in clips], waves=(4, 0), fmt="s16")


def test_peak_rel():
    """FPSPEC 5.1: each clip against the oracle at max(floor, r * its largest power); K1 also folds the maximum."""
    floor, r = 2.0 ** -20, np.float32(1e-4)
    base = synth.synth(80, 0, _n(41), SR, snr_db=20, salt=7)
    clips = [(base * np.float32(g)).astype(np.float32) for g in (1 / 64, 1.0, 1 / 8)]
    refs = []
    for x in clips:
        pmax = np.fmax.reduce(O.stft_power(x, HOP).ravel(), initial=np.float32(0.0)).astype(np.float32)
        refs.append(_ref(x, HOP, float(np.maximum(np.float32(floor), r * pmax))))
    assert all(len(ref[2]) for ref in refs)
    _check(clips, refs, waves=(4, 0), peak_threshold=floor, peak_rel=float(r))


@pytest.mark.parametrize("hop", [128, 256, 1024, 2048])
def test_hops(hop):
    """The other ring instantiations (1, 2, 8 and 16 new rows per frame) share the tail."""
    clips, refs = _uniform(3, 41, hop)
    _check(clips, refs, hop=hop, waves=(4, 0))


# ---- every store guard and every mirror / lane-0 bit on its own
TONE_BINS = [0, 1, 15, 16, 63, 64, 65, 448, 511, 512, 513, 575, 576, 959, 960, 1022, 1023]


def _am_tone(k, frames=41):
    """A tone at bin k whose amplitude swings at 8 Hz (about 11 frames a period): peaks in several frames, so records."""
    n = _n(frames)
    t = np.arange(n, dtype=np.float64)
    x = 0.05 * (0.55 + 0.45 * np.sin(2 * np.pi * 8.0 * t / SR)) * np.cos(2 * np.pi * k * t / 2048.0)
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _tone_case():
    rng = np.random.default_rng(5)
    n = _n(41)
    clips = [_am_tone(k) for k in TONE_BINS]
    clips.append((0.1 * rng.standard_normal(n)).astype(np.float32))  # full band
    clips.append(np.zeros(n, np.float32))  # silence
    for bad in (np.nan, np.inf):
        x = synth.synth(90, 0, n, SR, snr_db=20, salt=8)
        x[n // 2 + 1] = bad
        clips.append(x)
    refs = [_ref(x, HOP) for x in clips]
    # the cases are what they say: a tone's hot chunks (some bin > thr) lie within one chunk of the tone's own
    for k, (P, pk, rec) in zip(TONE_BINS, refs):
        hot = np.flatnonzero((P > O.DEFAULT_THR).any(axis=0)) // 16
        assert len(hot) and set(hot) <= {max(k // 16 - 1, 0), k // 16, min(k // 16 + 1, 63)}, (k, sorted(set(hot)))
        assert len(pk) or k < 2, k  # the peak rule leaves bin 0 without peaks: the power plane speaks for it
    full, silent, nan, inf = refs[len(TONE_BINS):]
    assert len(set(np.flatnonzero((full[0] > O.DEFAULT_THR).any(axis=0)) // 16)) == 64 and len(full[2])
    assert not silent[0].any() and not len(silent[1])
    assert np.isnan(nan[0]).any() and np.isnan(inf[0]).any() and len(nan[2]) and len(inf[2])
    return clips, refs


def test_single_tones_and_extremes():
    """One clip per tone (bins on both sides of every store's first and last chunk, of the direct / mirror seam at 512
    and of the lane-0 bins 576, 960), then a full-band, a silent, a NaN and an inf clip, in one call."""
    clips, refs = _tone_case()
    _check(clips, refs, waves=(24, 0))
