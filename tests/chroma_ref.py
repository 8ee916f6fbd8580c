"""numpy restatement of spec/FPSPEC.md 11 (the content fingerprint): the oracle of tests/test_chroma_ref_host.py and
tests/test_gpu_chroma*.py. A helper, not a test module.

Every binary32 operation of the spec is one numpy float32 operation or one vec_ref.fmaf (the correctly rounded fused
multiply-add), vectorised over frames and items. Each stage is callable alone: `power`, `rows` (C), `features` (F),
`words_from_features`. `rows64` / `features64` / `words64` restate the same pipeline in float64 with np.fft.rfft and
the `log1p` form of the classifiers.
"""

from __future__ import annotations

import numpy as np

from mel_ref import _twiddle, cmul, dft4, dft8
from vec_ref import fmaf

F32 = np.float32
F64 = np.float64

SR = 11025
N = 4096
HOP = 1365
BIN_LO, BIN_HI = 10, 1308
BANDS = 12
ITEM = 16
ITEM_ROWS = 20
ZERO_WORD = 627964279
GRAY = np.array([0, 1, 3, 2], dtype=np.uint32)
R_MIN = F32(0.01)

# (type, y, h, w; t0, t1, t2)
CLASSIFIERS = (
    (0, 4, 3, 15, 1.98215, 2.35817, 2.63523),
    (4, 4, 6, 15, -1.03809, -0.651211, -0.282167),
    (1, 0, 4, 16, -0.298702, 0.119262, 0.558497),
    (3, 8, 2, 12, -0.105439, 0.0153946, 0.135898),
    (3, 4, 4, 8, -0.142891, 0.0258736, 0.200632),
    (4, 0, 3, 5, -0.826319, -0.590612, -0.368214),
    (1, 2, 2, 9, -0.557409, -0.233035, 0.0534525),
    (2, 7, 3, 4, -0.0646826, 0.00620476, 0.0784847),
    (2, 6, 2, 16, -0.192387, -0.029699, 0.215855),
    (2, 1, 3, 2, -0.0397818, -0.00568076, 0.0292026),
    (5, 10, 1, 15, -0.53823, -0.369934, -0.190235),
    (3, 6, 2, 10, -0.124877, 0.0296483, 0.139239),
    (2, 1, 1, 14, -0.101475, 0.0225617, 0.231971),
    (3, 5, 6, 4, -0.0799915, -0.00729616, 0.063262),
    (1, 9, 2, 12, -0.272556, 0.019424, 0.302559),
    (3, 4, 2, 14, -0.164292, -0.0321188, 0.0846339),
)
# thresholds as binary32, then E = (float)exp((double)t)
THRESH = np.array([c[4:] for c in CLASSIFIERS], dtype=F32)
E = np.exp(THRESH.astype(F64)).astype(F32)


def n_frames(n: int) -> int:
    return 1 + (n - N) // HOP if n >= N else 0


def n_words(n: int) -> int:
    return max(0, n_frames(n) - (ITEM_ROWS - 1))


# ---- tables ----
def _tw(n: int, count: int):
    j = np.arange(count, dtype=F64)
    return np.cos(2.0 * np.pi * j / n).astype(F32), (-np.sin(2.0 * np.pi * j / n)).astype(F32)


WIN64 = 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(N, dtype=F64) / (N - 1))
WIN = WIN64.astype(F32)
T16 = _tw(16, 16)
T128 = _tw(128, 128)
T2048 = _tw(2048, 2048)
T4096 = _tw(4096, 2048)


def note_table() -> np.ndarray:
    """note(k) of bins [10, 1308): uint8[1298]."""
    k = np.arange(BIN_LO, BIN_HI, dtype=F64)
    o = np.log2((k * 11025.0 / 4096.0) / 27.5)
    return (12.0 * (o - np.floor(o))).astype(np.int64).astype(np.uint8)


def runs(notes: np.ndarray | None = None):
    """[(lo, len, note)]: consecutive bins with the same note."""
    notes = note_table() if notes is None else notes
    out = []
    for i, n in enumerate(notes):
        if out and out[-1][2] == int(n):
            out[-1][1] += 1
        else:
            out.append([BIN_LO + i, 1, int(n)])
    return [tuple(r) for r in out]


def rects(j: int):
    """(a, b): the rectangle lists (x0, x1, y0, y1) of classifier j, rows counted from the item's first."""
    t, y, h, w = CLASSIFIERS[j][:4]
    h2, w2, h3, w3, h23, w23 = h // 2, w // 2, h // 3, w // 3, 2 * h // 3, 2 * w // 3
    if t == 0:
        return [(0, w, y, y + h)], []
    if t == 1:
        return [(0, w, y + h2, y + h)], [(0, w, y, y + h2)]
    if t == 2:
        return [(w2, w, y, y + h)], [(0, w2, y, y + h)]
    if t == 3:
        return ([(0, w2, y + h2, y + h), (w2, w, y, y + h2)], [(0, w2, y, y + h2), (w2, w, y + h2, y + h)])
    if t == 4:
        return [(0, w, y + h3, y + h23)], [(0, w, y, y + h3), (0, w, y + h23, y + h)]
    return [(w3, w23, y, y + h)], [(0, w3, y, y + h), (w23, w, y, y + h)]


# ---- framing and FFT ----
def s16_to_f32(q: np.ndarray) -> np.ndarray:
    return q.astype(F32) / F32(32768)


def frame_samples(x: np.ndarray, frames=None) -> np.ndarray:
    """[F][4096]: frame t covers x[1365 t .. 1365 t + 4096), no padding."""
    x = np.asarray(x, dtype=F32)
    t = np.arange(n_frames(len(x))) if frames is None else np.asarray(list(frames), dtype=np.int64)
    return x[HOP * t[:, None] + np.arange(N)[None, :]] if len(t) else np.zeros((0, N), F32)


def dft16(v):
    s = [list(dft4(v[b], v[b + 4], v[b + 8], v[b + 12])) for b in range(4)]
    for b in range(1, 4):
        for c in range(1, 4):
            w = (np.broadcast_to(T16[0][b * c], s[b][c][0].shape), np.broadcast_to(T16[1][b * c], s[b][c][0].shape))
            s[b][c] = cmul(s[b][c], w)
    out = [None] * 16
    for c in range(4):
        y = dft4(s[0][c], s[1][c], s[2][c], s[3][c])
        for d in range(4):
            out[c + 4 * d] = y[d]
    return out


def _cm(v):
    return tuple(np.asarray(p, dtype=F32).reshape(v[0].shape) for p in v)


def fft2048(zr: np.ndarray, zi: np.ndarray):
    """Z[F][2048] (re, im) of z[F][2048]: FPSPEC 11 stages A, B, C (2048 = 16 * 16 * 8)."""
    F = zr.shape[0]
    n2 = np.arange(128)
    a = dft16([(zr[:, 128 * n1:128 * n1 + 128], zi[:, 128 * n1:128 * n1 + 128]) for n1 in range(16)])
    a = [_twiddle(_cm(a[k1]), T2048, (n2 * k1)[None, :]) for k1 in range(16)]  # a[k1][F][n2]
    Ar = np.stack([v[0] for v in a], axis=1).reshape(F, 16, 16, 8)  # [F][k1][m1][m2]
    Ai = np.stack([v[1] for v in a], axis=1).reshape(F, 16, 16, 8)
    b = dft16([(Ar[:, :, m1, :], Ai[:, :, m1, :]) for m1 in range(16)])  # b[j1][F][k1][m2]
    m2 = np.arange(8)
    b = [_twiddle(_cm(b[j1]), T128, (m2 * j1)[None, None, :]) for j1 in range(16)]
    c = dft8([(np.stack([b[j1][0][:, :, q] for j1 in range(16)], axis=2),
               np.stack([b[j1][1][:, :, q] for j1 in range(16)], axis=2)) for q in range(8)])  # c[j2][F][k1][j1]
    Zr = np.empty((F, 2048), F32)
    Zi = np.empty((F, 2048), F32)
    k1 = np.arange(16)[:, None]
    j1 = np.arange(16)[None, :]
    for j2 in range(8):
        idx = (k1 + 16 * j1 + 256 * j2).reshape(-1)
        Zr[:, idx] = np.asarray(c[j2][0], F32).reshape(F, 256)
        Zi[:, idx] = np.asarray(c[j2][1], F32).reshape(F, 256)
    return Zr, Zi


def power(frames_x: np.ndarray) -> np.ndarray:
    """P[F][1298] (bins 10 .. 1307) of framed samples [F][4096]."""
    xw = (frames_x.astype(F32) * WIN[None, :]).astype(F32)
    Zr, Zi = fft2048(np.ascontiguousarray(xw[:, 0::2]), np.ascontiguousarray(xw[:, 1::2]))
    k = np.arange(BIN_LO, BIN_HI)
    mk = 2048 - k
    a, b, c, d = Zr[:, k], Zi[:, k], Zr[:, mk], Zi[:, mk]
    er, ei, orr, oi = a + c, b - d, b + d, c - a
    tr, ti = cmul((orr, oi), (np.broadcast_to(T4096[0][k], a.shape), np.broadcast_to(T4096[1][k], a.shape)))
    tr, ti = np.asarray(tr, F32).reshape(a.shape), np.asarray(ti, F32).reshape(a.shape)
    xr, xi = er + tr, ei + ti
    return (fmaf(xr, xr, xi * xi).reshape(a.shape) * F32(0.25)).astype(F32)


def chroma(P: np.ndarray) -> np.ndarray:
    """C[F][12] of P[F][1298]: run sums in ascending bin order, then the runs of a note in bin order."""
    C = np.zeros((P.shape[0], BANDS), F32)
    for lo, ln, note in runs():
        s = np.zeros(P.shape[0], F32)
        for k in range(lo - BIN_LO, lo - BIN_LO + ln):
            s = s + P[:, k]
        C[:, note] = C[:, note] + s
    return C


def rows(x: np.ndarray, frames=None, chunk: int = 256) -> np.ndarray:
    """C[F][12] of a clip (all frames, or the listed ones)."""
    fr = frame_samples(x, frames)
    out = [chroma(power(fr[i:i + chunk])) for i in range(0, len(fr), chunk)]
    return np.concatenate(out) if out else np.zeros((0, BANDS), F32)


def features(C: np.ndarray) -> np.ndarray:
    """F[T - 4][12]: the 5-tap smoothing and the normaliser."""
    C = np.asarray(C, dtype=F32)
    T = C.shape[0]
    if T < 5:
        return np.zeros((0, BANDS), F32)
    sh = (T - 4, BANDS)
    g = (F32(0.25) * C[0:T - 4]).astype(F32)
    g = fmaf(F32(0.75), C[1:T - 3], g).reshape(sh)
    g = fmaf(F32(1.0), C[2:T - 2], g).reshape(sh)
    g = fmaf(F32(0.75), C[3:T - 1], g).reshape(sh)
    g = fmaf(F32(0.25), C[4:T], g).reshape(sh)
    s = np.zeros(T - 4, F32)
    for c in range(BANDS):
        s = fmaf(g[:, c], g[:, c], s).reshape(T - 4)
    r = np.sqrt(s).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = (g / r[:, None]).astype(F32)
    return np.where((r < R_MIN)[:, None], F32(0), f).astype(F32)


def areas(F: np.ndarray):
    """(a, b)[items][16] of F[rows][12], items = rows - 15: sums in the spec's order, in F's dtype."""
    F = np.asarray(F)
    n = max(0, F.shape[0] - (ITEM - 1))
    a = np.zeros((n, len(CLASSIFIERS)), F.dtype)
    b = np.zeros((n, len(CLASSIFIERS)), F.dtype)

    def area(r):
        s = np.zeros(n, F.dtype)
        for x in range(r[0], r[1]):
            for y in range(r[2], r[3]):
                s = s + F[x:x + n, y]
        return s

    for j in range(len(CLASSIFIERS)):
        ra, rb = rects(j)
        for dst, rs in ((a, ra), (b, rb)):
            if rs:
                v = area(rs[0])
                for r in rs[1:]:
                    v = v + area(r)
                dst[:, j] = v
    return a, b


def decisions_ratio(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """[items][16][3] bool: 1 + a >= E_i * (1 + b) in binary32."""
    A = (F32(1) + a.astype(F32)).astype(F32)
    B = (F32(1) + b.astype(F32)).astype(F32)
    return A[:, :, None] >= (E[None, :, :] * B[:, :, None]).astype(F32)


def decisions_log(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """The same decisions as log(1 + a) - log(1 + b) >= t_i in binary64."""
    d = np.log1p(a.astype(F64)) - np.log1p(b.astype(F64))
    return d[:, :, None] >= THRESH.astype(F64)[None, :, :]


def pack(dec: np.ndarray) -> np.ndarray:
    q = dec.sum(axis=2)
    v = np.zeros(dec.shape[0], np.uint32)
    for j in range(len(CLASSIFIERS)):
        v = (v << np.uint32(2)) | GRAY[q[:, j]]
    return v


def words_from_features(F: np.ndarray) -> np.ndarray:
    a, b = areas(np.asarray(F, dtype=F32))
    return pack(decisions_ratio(a, b))


def words_from_rows(C: np.ndarray) -> np.ndarray:
    return words_from_features(features(C))


def words(x: np.ndarray) -> np.ndarray:
    return words_from_rows(rows(x))


# ---- the float64 restatement ----
def rows64(x: np.ndarray) -> np.ndarray:
    fr = frame_samples(x).astype(F64) * WIN64[None, :]
    P = np.abs(np.fft.rfft(fr, axis=1)[:, BIN_LO:BIN_HI]) ** 2
    notes = note_table()
    C = np.zeros((P.shape[0], BANDS), F64)
    for c in range(BANDS):
        C[:, c] = P[:, notes == c].sum(axis=1)
    return C


def features64(C: np.ndarray) -> np.ndarray:
    T = C.shape[0]
    if T < 5:
        return np.zeros((0, BANDS), F64)
    g = 0.25 * C[0:T - 4] + 0.75 * C[1:T - 3] + C[2:T - 2] + 0.75 * C[3:T - 1] + 0.25 * C[4:T]
    r = np.sqrt((g * g).sum(axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        f = g / r[:, None]
    return np.where((r < 0.01)[:, None], 0.0, f)


def words64(x: np.ndarray) -> np.ndarray:
    a, b = areas(features64(rows64(x)))
    return pack(decisions_log(a, b))


# ---- inputs and scoring ----
def song(seed: int, seconds: float, sr: int = SR) -> np.ndarray:
    """A seeded synthetic song: a chord of three notes with harmonics every 0.2 .. 0.6 s over a quiet noise floor."""
    rng = np.random.default_rng(seed)
    n = int(round(seconds * sr))
    t = np.arange(n, dtype=F64) / sr
    x = 0.003 * rng.standard_normal(n)
    pos = 0
    while pos < n:
        ln = int(rng.uniform(0.2, 0.6) * sr)
        seg = slice(pos, min(n, pos + ln))
        env = np.exp(-3.0 * (t[seg] - t[pos]))
        for midi in rng.choice(np.arange(40, 88), size=3, replace=False):
            f0 = 440.0 * 2.0 ** ((midi - 69) / 12.0)
            for h in (1, 2, 3):
                if f0 * h < 0.45 * sr:
                    x[seg] += (0.15 / h) * env * np.sin(2 * np.pi * f0 * h * t[seg] + rng.uniform(0, 6.28))
        pos += ln
    return x.astype(F32)


def add_noise(x: np.ndarray, snr_db: float, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    p = float(np.mean(x.astype(F64) ** 2))
    return (x + np.sqrt(p / 10.0 ** (snr_db / 10.0)) * rng.standard_normal(len(x))).astype(F32)


def similarity(a: np.ndarray, b: np.ndarray) -> float:
    """The reference's `_fingerprint_similarity` on word arrays (app/audio/dedup.py:127-166)."""
    mn, mx = min(len(a), len(b)), max(len(a), len(b))
    if mn == 0:
        return 0.0
    diff = sum(bin(int(p) ^ int(q)).count("1") for p, q in zip(a[:mn], b[:mn]))
    return ((mn * 32 - diff) / (mn * 32)) * (mn / mx)


def differing_bits(a: np.ndarray, b: np.ndarray) -> int:
    assert len(a) == len(b)
    return sum(bin(int(p) ^ int(q)).count("1") for p, q in zip(a, b))
