"""numpy restatement of spec/FPSPEC.md 10 (the CLAP log-mel front end): the oracle of tests/test_mel_host.py and
tests/test_gpu_mel.py. A helper, not a test module.

Every binary32 operation of the spec is one numpy float32 operation or one vec_ref.fmaf (the correctly rounded
fused multiply-add), vectorised over the frames of a frame list, so an edge case costs a few frames, not 1001.
"""

from __future__ import annotations

import numpy as np

from vec_ref import fmaf

F32 = np.float32
F64 = np.float64

SR = 48000
N = 1024
HOP = 480
L = 480000
CHUNK_HOP = 240000
MIN_CHUNK = 48000
T = 1001
BANDS = 64
BINS = 513
ZERO, REPEATPAD = 0, 1
SLANEY, HTK = 0, 1

# 10 * log10(M), FPSPEC 10 "dB": C_HI + C_LO = 10 log10(2), DB_COEF = Q(f) ~ 10 log10(1 + f) / f on [sqrt(1/2) - 1, sqrt(2) - 1]
DB_SQRT2 = F32(float.fromhex("0x1.6a09e6p+0"))
DB_C_HI = F32(float.fromhex("0x1.8152p+1"))
DB_C_LO = F32(float.fromhex("-0x1.f6ce2ap-17"))
DB_COEF = np.array([float.fromhex(h) for h in (
    "0x1.15f2cep+2", "-0x1.15f2cep+1", "0x1.7298fep+0", "-0x1.15f2fcp+0", "0x1.bcc62p-1", "-0x1.729872p-1",
    "0x1.3c05d4p-1", "-0x1.143018p-1", "0x1.09a088p-1", "-0x1.026534p-1", "0x1.24486ep-2")], dtype=F32)
MEL_FLOOR = F32(1e-10)


# ---- chunk plan ----
def chunk_plan(n: int):
    """chunk_audio's tuples without the audio: [(start, r, offset_sec, chunk_index, duration_sec)]."""
    out = []
    s, idx = 0, 0
    while s < n:
        r = min(L, n - s)
        if r < MIN_CHUNK:
            break
        out.append((s, r, s / SR, idx, r / SR))
        idx += 1
        s += CHUNK_HOP
    return out


def query_plan(n: int, start: int = 0):
    """repeatpad: (start, r, rep) of the one chunk of a query of n >= 1 samples."""
    if n > L:
        assert 0 <= start <= n - L
        return start, L, 1
    return 0, n, L // n


# ---- tables ----
def _tw(n: int, count: int):
    j = np.arange(count, dtype=F64)
    return np.cos(2.0 * np.pi * j / n).astype(F32), (-np.sin(2.0 * np.pi * j / n)).astype(F32)


WIN = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N, dtype=F64) / N)).astype(F32)
T8 = _tw(8, 8)
T64 = _tw(64, 64)
T512 = _tw(512, 512)
T1K = _tw(1024, 512)


# ---- filter banks (binary64, rounded once) ----
def _hz_to_mel(f: float, slaney: bool) -> float:
    if not slaney:
        return 2595.0 * np.log10(1.0 + f / 700.0)
    if f >= 1000.0:
        return 15.0 + np.log(f / 1000.0) * (27.0 / np.log(6.4))
    return 3.0 * f / 200.0


def _mel_to_hz(m: np.ndarray, slaney: bool) -> np.ndarray:
    if not slaney:
        return 700.0 * (np.power(10.0, m / 2595.0) - 1.0)
    f = 200.0 * m / 3.0
    lg = m >= 15.0
    f[lg] = 1000.0 * np.exp((np.log(6.4) / 27.0) * (m[lg] - 15.0))
    return f


def bank(kind: int, fmin: float = 50.0, fmax: float = 14000.0) -> np.ndarray:
    """[513][64] float32: the slaney (slaney scale and norm) or htk (htk scale, no norm) bank."""
    slaney = kind == SLANEY
    m0, m1 = _hz_to_mel(float(fmin), slaney), _hz_to_mel(float(fmax), slaney)
    step = (m1 - m0) / (BANDS + 1)
    mels = np.arange(BANDS + 2, dtype=F64) * step + m0
    mels[-1] = m1
    ff = _mel_to_hz(mels, slaney)
    fk = np.arange(BINS, dtype=F64) * ((SR / 2.0) / (BINS - 1))
    down = -(ff[None, :-2] - fk[:, None]) / (ff[1:-1] - ff[:-2])[None, :]
    up = (ff[None, 2:] - fk[:, None]) / (ff[2:] - ff[1:-1])[None, :]
    w = np.minimum(down, up)
    w = np.where(w > 0.0, w, 0.0)
    if slaney:
        w = w * (2.0 / (ff[2:] - ff[:-2]))[None, :]
    return w.astype(F32)


def supports(W: np.ndarray):
    """(lo[64], hi[64], K) of a [513][64] table; raises on an empty or gapped band."""
    lo, hi = np.zeros(BANDS, np.int32), np.zeros(BANDS, np.int32)
    for m in range(BANDS):
        nz = np.flatnonzero(W[:, m])
        if len(nz) == 0:
            raise ValueError(f"band {m} is empty")
        if nz[-1] - nz[0] + 1 != len(nz):
            raise ValueError(f"band {m} has a gap")
        lo[m], hi[m] = nz[0], nz[-1] + 1
    return lo, hi, int(hi.max())


# ---- source mapping and framing ----
def s16_to_f32(q: np.ndarray) -> np.ndarray:
    return q.astype(F32) / F32(32768)


def frame_samples(x: np.ndarray, start: int, r: int, fill: int, frames) -> np.ndarray:
    """[F][1024] float32: u[480 t - 512 .. 480 t + 512) of the chunk x[start .. start + r), whose v[0..L) takes
    v[j] = x[start + j mod r] for j < fill (fill = r: zero mode; rep * r: repeatpad), else 0, reflected per chunk."""
    x = np.asarray(x, dtype=F32)
    t = np.asarray(list(frames), dtype=np.int64)
    p = HOP * t[:, None] - N // 2 + np.arange(N, dtype=np.int64)[None, :]
    p = np.where(p < 0, -p, p)
    p = np.where(p >= L, 2 * (L - 1) - p, p)
    live = p < fill
    src = start + np.where(live, p % r, 0)
    return np.where(live, x[src], F32(0)).astype(F32)


# ---- FFT ----
def _add(a, b):
    return a[0] + b[0], a[1] + b[1]


def _sub(a, b):
    return a[0] - b[0], a[1] - b[1]


def cmul(x, w):
    return fmaf(x[0], w[0], -(x[1] * w[1])), fmaf(x[0], w[1], x[1] * w[0])


def dft4(x0, x1, x2, x3):
    t0, t1, t2, t3 = _add(x0, x2), _sub(x0, x2), _add(x1, x3), _sub(x1, x3)
    return _add(t0, t2), (t1[0] + t3[1], t1[1] - t3[0]), _sub(t0, t2), (t1[0] - t3[1], t1[1] + t3[0])


def dft8(x):
    e = dft4(x[0], x[2], x[4], x[6])
    o = list(dft4(x[1], x[3], x[5], x[7]))
    o[1] = cmul(o[1], (T8[0][1], T8[1][1]))
    o[2] = (o[2][1], -o[2][0])
    o[3] = cmul(o[3], (T8[0][3], T8[1][3]))
    return [_add(e[k], o[k]) for k in range(4)] + [_sub(e[k], o[k]) for k in range(4)]


def _twiddle(v, tab, idx):
    """cmul by tab[idx] where idx != 0 (idx broadcasts against v), unchanged elsewhere."""
    w = (tab[0][idx], tab[1][idx])
    y = cmul(v, (np.broadcast_to(w[0], v[0].shape), np.broadcast_to(w[1], v[0].shape)))
    keep = np.broadcast_to(idx == 0, v[0].shape)
    return np.where(keep, v[0], y[0]), np.where(keep, v[1], y[1])


def fft512(zr: np.ndarray, zi: np.ndarray):
    """Z[F][512] (re, im) of z[F][512]: FPSPEC 10 stages A, B, C."""
    F = zr.shape[0]
    n2 = np.arange(64)
    # stage A: over n1, per n2
    a = dft8([(zr[:, 64 * n1:64 * n1 + 64], zi[:, 64 * n1:64 * n1 + 64]) for n1 in range(8)])
    a = [_twiddle(a[k1], T512, (n2 * k1)[None, :]) for k1 in range(8)]  # a[k1][F][n2]
    Ar = np.stack([v[0] for v in a], axis=1).reshape(F, 8, 8, 8)  # [F][k1][m1][m2]
    Ai = np.stack([v[1] for v in a], axis=1).reshape(F, 8, 8, 8)
    # stage B: over m1, per (k1, m2)
    b = dft8([(Ar[:, :, m1, :], Ai[:, :, m1, :]) for m1 in range(8)])  # b[j1][F][k1][m2]
    m2 = np.arange(8)
    b = [_twiddle(b[j1], T64, (m2 * j1)[None, None, :]) for j1 in range(8)]
    # stage C: over m2, per (k1, j1)
    c = dft8([(np.stack([b[j1][0][:, :, q] for j1 in range(8)], axis=2),
               np.stack([b[j1][1][:, :, q] for j1 in range(8)], axis=2)) for q in range(8)])  # c[j2][F][k1][j1]
    Zr = np.empty((F, 512), F32)
    Zi = np.empty((F, 512), F32)
    k1 = np.arange(8)[:, None]
    j1 = np.arange(8)[None, :]
    for j2 in range(8):
        idx = (k1 + 8 * j1 + 64 * j2).reshape(-1)
        Zr[:, idx] = c[j2][0].reshape(F, 64)
        Zi[:, idx] = c[j2][1].reshape(F, 64)
    return Zr, Zi


def power(frames_u: np.ndarray, K: int) -> np.ndarray:
    """P[F][K] of framed samples [F][1024]."""
    xw = (frames_u.astype(F32) * WIN[None, :]).astype(F32)
    Zr, Zi = fft512(np.ascontiguousarray(xw[:, 0::2]), np.ascontiguousarray(xw[:, 1::2]))
    k = np.arange(K)
    mk = (512 - k) & 511
    a, b, c, d = Zr[:, k], Zi[:, k], Zr[:, mk], Zi[:, mk]
    er, ei, orr, oi = a + c, b - d, b + d, c - a
    tr, ti = cmul((orr, oi), (np.broadcast_to(T1K[0][k], a.shape), np.broadcast_to(T1K[1][k], a.shape)))
    xr, xi = er + tr, ei + ti
    return (fmaf(xr, xr, xi * xi) * F32(0.25)).astype(F32)


def db10(M: np.ndarray) -> np.ndarray:
    """The pinned 10 * log10(M) of normal positive float32 M."""
    M = np.ascontiguousarray(M, dtype=F32)
    bits = M.view(np.uint32)
    e = (bits >> np.uint32(23)).astype(np.int32) - 127
    m = ((bits & np.uint32(0x7FFFFF)) | np.uint32(0x3F800000)).view(F32)
    big = m >= DB_SQRT2
    m = np.where(big, m * F32(0.5), m).astype(F32)
    ef = (e + big).astype(F32)
    f = (m - F32(1)).astype(F32)
    q = np.full(f.shape, DB_COEF[-1], F32)
    for c in DB_COEF[-2::-1]:
        q = fmaf(q, f, c).reshape(f.shape)
    t = fmaf(ef, DB_C_LO, (f * q).astype(F32)).reshape(f.shape)
    return fmaf(ef, DB_C_HI, t).reshape(f.shape)


def mel_db(P: np.ndarray, W: np.ndarray) -> np.ndarray:
    """[F][64]: per band the ascending fma chain over its support, the floor, then dB."""
    lo, hi, K = supports(W)
    assert P.shape[1] >= K
    acc = np.zeros((P.shape[0], BANDS), F32)
    bands = np.arange(BANDS)
    for j in range(int((hi - lo).max())):
        on = lo + j < hi
        k = np.where(on, lo + j, lo)
        nxt = fmaf(W[k, bands][None, :], P[:, k], acc).reshape(acc.shape)
        acc = np.where(on[None, :], nxt, acc)
    return db10(np.maximum(acc, MEL_FLOOR))


def logmel(x: np.ndarray, W: np.ndarray, frames, start: int = 0, r: int | None = None, fill: int | None = None) -> np.ndarray:
    """[F][64] of the chunk x[start .. start + r) (default: all of x from start, at most L, zero mode) at `frames`."""
    if r is None:
        r = min(L, len(x) - start)
    if fill is None:
        fill = r
    K = supports(W)[2]
    return mel_db(power(frame_samples(x, start, r, fill, frames), K), W)


# ---- the fixture inputs of tests/golden/ref_clap_mel.npz (only the outputs are stored) ----
FIXTURE_LENGTHS = (48000, 160001, 288000, 479800)


def fixture_input(i: int, seed: int = 20261021) -> np.ndarray:
    """Deterministic float32 input i of FIXTURE_LENGTHS[i] samples: tones, a chirp, noise at several levels."""
    n = FIXTURE_LENGTHS[i]
    rng = np.random.default_rng(seed + i)
    t = np.arange(n, dtype=F64) / SR
    if i == 0:  # tone plus chirp
        x = 0.4 * np.sin(2 * np.pi * 440.0 * t + 0.3) + 0.3 * np.sin(2 * np.pi * (200.0 + 4000.0 * t) * t)
    elif i == 1:  # noise plus a tone
        x = 0.1 * rng.standard_normal(n) + 0.2 * np.sin(2 * np.pi * 3000.0 * t)
    elif i == 2:  # decaying chirp up to 12 kHz over a low noise floor
        x = 0.5 * np.exp(-t / 3.0) * np.sin(2 * np.pi * (100.0 + 1000.0 * t) * t) + 1e-4 * rng.standard_normal(n)
    else:  # harmonics with a slow tremolo
        x = sum(0.2 / h * np.sin(2 * np.pi * 220.0 * h * t + h) for h in range(1, 9)) * (0.6 + 0.4 * np.sin(2 * np.pi * 0.7 * t))
        x = x + 1e-3 * rng.standard_normal(n)
    return x.astype(F32)


def fixture_frames(r: int, fill: int | None = None):
    """The named frames of a fixture: 0, 1, 2, those straddling r (and the end of the repeated part), 998-1000."""
    fr = {0, 1, 2, 998, 999, 1000}
    for edge in {r, fill if fill is not None else r}:
        fr |= {t for t in range(edge // HOP - 1, edge // HOP + 3) if 0 <= t < T}
    return sorted(fr)


def deviation_classes(got: np.ndarray, ref: np.ndarray):
    """max |got - ref| in dB, split by how far a band lies below its frame's maximum in `ref`:
    [0-20, 20-40, 40-60, > 60] (None for an empty class)."""
    below = ref.max(axis=1, keepdims=True) - ref
    err = np.abs(got.astype(F64) - ref.astype(F64))
    out = []
    for a, b in ((0, 20), (20, 40), (40, 60), (60, np.inf)):
        sel = (below >= a) & (below < b)
        out.append(float(err[sel].max()) if sel.any() else None)
    return out
