"""K2 -> K3 row flags (csrc/aidfp_layout.h, peaks.hip, landmarks.hip): K2 stores a row's 4 mask words of a 256-bin
quarter only when they hold a peak and says so in one flag bit per (row, quarter); K3 and aid_result_peakmask go by
the flags, and a mask word without its flag is whatever an earlier call left there. So the failure this file looks
for is stale memory: every case dirties the engine's mask with a dense call first (or runs dense and sparse calls in
turn), and every call must give the oracle's peaks, records and counts bit for bit.

The flags are indexed by K2 strip (32 rows a word, per strip), so the cases also put peaks on the first and last row
of flag words and strips, at both K2 widths, across clip groups (a strip length per group) and K3 chunks. Strip
lengths depend on the device's resident workgroup slots; a case that needs one reads the strip count of a call
(match_stats) and derives the length from it.
"""

import functools

import numpy as np
import pytest

import dense_fixtures as D
import oracle as O
from aidfp import synth
from aidfp.engine import Engine, peaks_from_mask
from test_gpu_k2_width import _am_tones, _f32

pytestmark = pytest.mark.gpu
SR = 44100
HOP = 512
N3 = SR * 3  # 255 frames
WIDTHS = [2, 4]


def _frames(n, hop=HOP):
    return 0 if n < 2048 else 1 + (n - 2048) // hop


def _strip_len(frames, strips):
    """The strip length of a one-group call that had `strips` K2 strips: peak_strip_len takes the smallest L >= 16
    whose strip count fits its budget, and that is the smallest L with at most the count it ended up with."""
    for L in range(16, max([16] + frames) + 1):
        if sum(-(-f // L) for f in frames) <= strips:
            return L
    raise AssertionError("no strip length gives that count")


def _ref(x, hop=HOP, thr=None):
    P = O.stft_power(x, hop)
    if thr is None:
        return O.peaks(P).reshape(-1, 2), O.fingerprint(x, hop)
    return O.peaks(P, thr).reshape(-1, 2), O.fingerprint(x, hop, thr)


def _check(e, clips, refs, what=""):
    got = e.extract_host(clips)
    counts = e.counts()
    for c, (x, (pk, rec)) in enumerate(zip(clips, refs)):
        assert np.array_equal(peaks_from_mask(e.peakmask(c, len(x))), pk), f"{what} clip {c}: peaks differ"
        assert np.array_equal(got[c], rec), f"{what} clip {c}: records differ"
        assert counts[c] == len(rec), f"{what} clip {c}: count differs"


def _dirty(e, lens, seed=1):
    """A call of white-noise clips of these lengths: peaks (and stored mask words) in every quarter of nearly every
    row. Its results are not looked at; what it leaves in the mask plane is the point."""
    rng = np.random.default_rng(seed)
    e.extract_host([rng.standard_normal(n).astype(np.float32) for n in lens])


class _Forced:
    def __init__(self, e, **kw):
        self.e, self.kw = e, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.e.force(k, v)
        return self.e

    def __exit__(self, *exc):
        for k in self.kw:
            self.e.force(k, 0)


@pytest.fixture(scope="module")
def eng():
    with Engine(SR) as e:
        yield e


# ---- stale memory: dense and sparse calls in turn on one engine (hop 2048: the lattice is exact there)
STALE_F = [96, 70, 96, 40]  # frames; 96 = three whole flag words of a 96-row strip


@functools.lru_cache(maxsize=None)
def _stale_case():
    hop = 2048
    dense, sparse = [], []
    for i, F in enumerate(STALE_F):
        dense.append(D.noise(F, hop, 20 + i)[0] if i % 2 else D.lattice(F, hop, diag=1, seed=i)[0])
        n = D.n_samples(F, hop)
        t = np.arange(n) / SR
        x = np.zeros(n)
        if i == 1:  # one AM tone in the lowest quarter, in the clip's first third only
            x[:n // 3] = (0.05 * (0.5 + 0.5 * np.sin(2 * np.pi * 3 * t)) * np.sin(2 * np.pi * (100 * SR / 2048.0) * t))[:n // 3]
        elif i == 2:  # a tone above bin 512 only, first third
            x[:n // 3] = (0.05 * np.sin(2 * np.pi * (700 * SR / 2048.0) * t))[:n // 3]
        sparse.append(x.astype(np.float32))  # 0 and 3: silence
    dref = [_ref(x, hop) for x in dense]
    sref = [_ref(x, hop) for x in sparse]
    # the case proves nothing unless the dense call flags every quarter and the sparse one leaves whole quarters and
    # whole 32-row words alone where the dense one stored words
    for c, ((dp, _), (sp, _)) in enumerate(zip(dref, sref)):
        dq = {(int(t) // 32, int(k) // 256) for t, k in dp}
        sq = {(int(t) // 32, int(k) // 256) for t, k in sp}
        assert {q for _, q in dq} == {0, 1, 2, 3}, f"dense clip {c}: a quarter without a peak"
        assert len({q for _, q in sq}) <= 1, f"sparse clip {c}: peaks in more than one quarter"
        assert dq - sq, f"clip {c}: no stored word for the sparse call to leave stale"
        if STALE_F[c] >= 64:
            assert any(all((w, q) not in sq for q in range(4)) and any((w, q) in dq for q in range(4))
                       for w in range(STALE_F[c] // 32)), f"sparse clip {c}: no whole 32-row word without a peak"
    assert len(sref[1][0]) and len(sref[2][0]) and np.all(sref[1][0][:, 1] < 256) and np.all(sref[2][0][:, 1] >= 512)
    return dense, dref, sparse, sref


@pytest.mark.parametrize("x100", [100, 1])
@pytest.mark.parametrize("width", WIDTHS)
def test_stale_memory(width, x100):
    """Dense, then sparse with the same clip count and lengths, then the reverse order, then fewer and more clips
    than the call before. x100 = 1 gives strips of 96 rows (three flag words), 100 strips of 16."""
    dense, dref, sparse, sref = _stale_case()
    calls = [("dense", dense, dref), ("sparse", sparse, sref), ("dense again", dense, dref),
             ("sparse again", sparse, sref), ("fewer", sparse[1:3], sref[1:3]),
             ("more", dense + sparse, dref + sref), ("sparse after more", sparse, sref),
             ("fewer dense", dense[:3], dref[:3]), ("mixed", sparse[:2] + dense[2:], sref[:2] + dref[2:])]
    with Engine(SR, hop=2048) as e, _Forced(e, k2_width=width, k2_strips_x100=x100):
        for what, clips, refs in calls:
            _check(e, clips, refs, what)
            assert e.match_stats()["k2_width"] == width


# ---- word and strip edges
EDGE_CLIPS = 6
LOW_BINS = [60, 100, 140, 180, 220, 260, 300, 340]
HIGH_BINS = [560, 600, 640, 680, 720, 760, 800, 840]


def _tone_at(x, k, frame, wide=8, amp=0.05):
    """Adds a tone at bin k under a Hann envelope `wide` frames long centred on the centre of frame `frame` (cut at
    the clip's ends): its power is largest in that frame."""
    c, m = frame * HOP + 1024, wide * HOP
    a = c - m // 2
    lo, hi = max(a, 0), min(a + m, len(x))
    t = np.arange(m) / SR
    x[lo:hi] += (amp * np.hanning(m) * np.sin(2 * np.pi * (k * SR / 2048.0) * t))[lo - a:hi - a]


def _edge_rows(L, F):
    rows = []
    for t0 in range(0, F, L):
        n = min(L, F - t0)
        rows += [t0 + r for r in (0, 31, 32, 63, 64, n - 1) if r < n]
    return sorted(set(rows))


@functools.lru_cache(maxsize=None)
def _edge_case(L):
    """EDGE_CLIPS clips of 255 frames with a tone burst peaking on strip-relative rows 0, 31, 32, 63, 64 and the last
    row of every strip of length L. Even clips stay below bin 512 (no second walk at width 2), odd ones use bins
    above it as well (every strip walked twice)."""
    F = _frames(N3)
    clips, refs = [], []
    for c in range(EDGE_CLIPS):
        x = np.zeros(N3)
        want = []
        for i, row in enumerate(_edge_rows(L, F)):
            k = (HIGH_BINS if c % 2 and i % 2 else LOW_BINS)[(i // (1 + c % 2) + c) % 8]
            _tone_at(x, k, row)
            want.append((row, k))
        x = _f32(x)
        pk, rec = _ref(x)
        have = {(int(t), int(k)) for t, k in pk}
        assert set(want) <= have, f"L {L} clip {c}: no reference peak at {sorted(set(want) - have)}"
        assert (c % 2 == 1) == bool(np.any(pk[:, 1] >= 512))
        clips.append(x)
        refs.append((pk, rec))
    return clips, refs


@pytest.mark.parametrize("x100", [100, 300, 1])
@pytest.mark.parametrize("width", WIDTHS)
def test_word_edges(eng, width, x100):
    """3 s clips at 16-row strips (x100 100 and 300: one partial word per strip, many strip edges) and at long strips
    (x100 1: three words or more), with reference peaks on the first and last rows of the words and of the strips."""
    with _Forced(eng, k2_width=width, k2_strips_x100=x100):
        _dirty(eng, [N3] * EDGE_CLIPS)  # also shows the strip count of clips of these lengths
        L = _strip_len([_frames(N3)] * EDGE_CLIPS, eng.match_stats()["k2_strips"])
        assert L == 16 if x100 != 1 else L >= 65, L
        clips, refs = _edge_case(L)
        _check(eng, clips, refs, f"L {L}")
        assert eng.match_stats()["k2_width"] == width
        assert _strip_len([_frames(N3)] * EDGE_CLIPS, eng.match_stats()["k2_strips"]) == L


# ---- clip groups: a strip length and a flag base per group
GROUP_LENS = [N3, int(SR * 2.2), 100, 2048 + 13 * HOP, int(SR * 3.5), int(SR * 1.7), SR * 4, int(SR * 1.2)]
GROUP_ROWS = 300


@functools.lru_cache(maxsize=None)
def _group_case():
    clips = [synth.synth(60 + i, 500 * i, n, SR, snr_db=20 if i % 2 else None, salt=3) for i, n in enumerate(GROUP_LENS)]
    groups, acc = 1, 0
    for n in GROUP_LENS:  # aidfp_extract_plan.h: a clip that would pass the cap opens a group
        if acc > 0 and acc + _frames(n) > GROUP_ROWS:
            groups, acc = groups + 1, 0
        acc += _frames(n)
    assert groups >= 3 and _frames(GROUP_LENS[2]) == 0 and _frames(GROUP_LENS[3]) == 14
    return clips, [_ref(x) for x in clips]


@pytest.mark.parametrize("x100", [100, 1])
@pytest.mark.parametrize("width", WIDTHS)
def test_clip_groups(eng, width, x100):
    """plane_rows 300: at least three groups in one call, an empty clip and a 14-frame clip in the middle; at x100 1
    every group has its own strip length."""
    clips, refs = _group_case()
    with _Forced(eng, k2_width=width, k2_strips_x100=x100, plane_rows=GROUP_ROWS):
        _dirty(eng, GROUP_LENS)
        _check(eng, clips, refs)
        _check(eng, clips[::-1], refs[::-1], "reversed")


# ---- several K3 chunks
CHUNK_LENS = [SR * 13, N3, SR]  # 1116, 255 and 83 frames


@functools.lru_cache(maxsize=None)
def _chunk_case():
    clips = [synth.synth(80 + i, 0, n, SR, snr_db=None if i else 20, salt=5) for i, n in enumerate(CHUNK_LENS)]
    refs = [_ref(x) for x in clips]
    t = refs[0][0][:, 0]
    assert np.any((t >= 961) & (t < 1024)) and np.any((t >= 1024) & (t < 1087))  # peaks on both sides of the boundary
    return clips, refs


@pytest.mark.parametrize("x100", [100, 1])
@pytest.mark.parametrize("width", WIDTHS)
def test_multi_chunk(eng, width, x100):
    """A 13 s clip (two K3 chunks: the COUNT pass and the chunk bases read flags) beside short ones. At 16-row strips
    the zone of chunk 0 (frames 1024..1086) crosses strip edges; at long strips the chunk boundary lies inside one."""
    clips, refs = _chunk_case()
    frames = [_frames(n) for n in CHUNK_LENS]
    with _Forced(eng, k2_width=width, k2_strips_x100=x100):
        _dirty(eng, CHUNK_LENS)
        _check(eng, clips, refs)
        L = _strip_len(frames, eng.match_stats()["k2_strips"])
        if x100 == 100:
            assert any(1024 < edge < 1087 for edge in range(0, frames[0], L)), L
        else:
            assert L > 63 and 1024 % L != 0, L


# ---- no peaks at all
@pytest.mark.parametrize("width", WIDTHS)
def test_no_peaks(eng, width):
    lens = [N3, SR, 2048 + 13 * HOP, N3 + 777]
    with _Forced(eng, k2_width=width):
        _dirty(eng, lens)
        got = eng.extract_host([np.zeros(n, np.float32) for n in lens])
        assert all(len(g) == 0 for g in got) and not np.any(eng.counts())
        for c, n in enumerate(lens):
            m = eng.peakmask(c, n)
            assert m.shape == (_frames(n), 16) and not np.any(m), f"clip {c}: mask not zero"


# ---- the relative threshold
def test_peak_rel():
    """r = 1e-4: a quiet and a loud copy of a clip in one call, each against the oracle at its own threshold
    (FPSPEC 5.1: max(floor, r * the clip's largest power), in binary32), after a dense call."""
    floor, r = 2.0 ** -20, np.float32(1e-4)
    base = synth.synth(90, 0, N3, SR, snr_db=20, salt=9)
    clips = [(base * np.float32(g)).astype(np.float32) for g in (1 / 64, 1.0)]
    refs = []
    for x in clips:
        pmax = np.fmax.reduce(O.stft_power(x, HOP).ravel(), initial=np.float32(0.0)).astype(np.float32)
        thr = float(np.maximum(np.float32(floor), r * pmax))
        refs.append(_ref(x, thr=thr))
    assert len(refs[0][1]) and len(refs[1][1])
    with Engine(SR, peak_threshold=floor, peak_rel=float(r)) as e:
        _dirty(e, [N3, N3])
        _check(e, clips, refs)
        _check(e, clips[::-1], refs[::-1], "swapped")
