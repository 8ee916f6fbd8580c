"""numpy restatement of spec/FPSPEC.md 9 (the vector lane): the oracle of tests/test_vec_host.py and
tests/test_gpu_vector.py. A helper, not a test module.

binary32 fmaf is emulated exactly and vectorised: the product of two float32 is exact in float64, the sum
p + c is rounded once to float64 with its exact error e by TwoSum, and the only case where rounding that float64
to float32 differs from rounding the exact sum (double rounding) is a float64 that sits exactly on a binary32
midpoint while e != 0: it is moved one float64 step toward the sign of e first. Valid while every value stays in
binary32's normal range, which the tests' inputs do.
"""

from __future__ import annotations

import numpy as np

F32 = np.float32
F64 = np.float64


def fmaf(a, b, c) -> np.ndarray:
    """Correctly rounded binary32 a * b + c of float32 arrays (broadcast)."""
    a64 = np.asarray(a, dtype=F32).astype(F64)
    b64 = np.asarray(b, dtype=F32).astype(F64)
    c64 = np.asarray(c, dtype=F32).astype(F64)
    p = a64 * b64  # exact: 24 x 24 bits
    s = p + c64
    bb = s - p
    e = (p - (s - bb)) + (c64 - bb)  # TwoSum: p + c = s + e exactly
    s = np.atleast_1d(s)
    e = np.broadcast_to(np.atleast_1d(e), s.shape)
    tie = ((s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) & (e != 0)
    if tie.any():
        s = np.where(tie, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def fmaf_naive(a, b, c) -> np.ndarray:
    """A float64 multiply-add rounded to float32: wrong on the tie cases (kept to show the correction is needed)."""
    return (np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64) + np.asarray(c, F32).astype(F64)).astype(F32)


def tie_cases(n: int = 2000, seed: int = 7):
    """n triples whose exact a * b + c lies within 2^-70 (relative) of a binary32 midpoint, on either side:
    a * b = +-h * (1 - x^2) with h = half an ulp of c and x = i * 2^-23, so the float64 sum is the midpoint itself."""
    rng = np.random.default_rng(seed)
    out_a, out_b, out_c = [], [], []
    while len(out_a) < n:
        m = 4 * n
        i = rng.integers(1, 363, size=m).astype(F64)
        ex = rng.integers(-20, 21, size=m)
        cm = (1.0 + rng.integers(0, 1 << 23, size=m).astype(F64) * 2.0**-23) * 2.0**ex
        c = (cm * rng.choice([-1.0, 1.0], size=m)).astype(F32)
        a = ((1.0 + i * 2.0**-23) * 2.0 ** (ex - 12) * rng.choice([-1.0, 1.0], size=m)).astype(F32)
        b = ((1.0 - i * 2.0**-23) * 2.0**-12).astype(F32)
        p = a.astype(F64) * b.astype(F64)
        s = p + c.astype(F64)
        bb = s - p
        e = (p - (s - bb)) + (c.astype(F64) - bb)
        ok = ((s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) & (e != 0)
        out_a += list(a[ok])
        out_b += list(b[ok])
        out_c += list(c[ok])
    return (np.array(out_a[:n], F32), np.array(out_b[:n], F32), np.array(out_c[:n], F32))


def normalize(x: np.ndarray) -> np.ndarray:
    """[n][dim] float32 -> unit vectors: ss by the fmaf chain from +0, y = x / sqrtf(ss), both correctly rounded;
    a vector whose ss is 0 or not finite becomes all +0."""
    x = np.ascontiguousarray(x, dtype=F32)
    ss = np.zeros(x.shape[0], F32)
    with np.errstate(all="ignore"):
        for k in range(x.shape[1]):
            ss = fmaf(x[:, k], x[:, k], ss)
        ok = np.isfinite(ss) & (ss > 0)
        d = np.sqrt(np.where(ok, ss, F32(1)).astype(F32))
        y = (x / d[:, None]).astype(F32)
    y[~ok] = 0
    return y


def scores(qn: np.ndarray, cn: np.ndarray) -> np.ndarray:
    """[nq][n] float32: per pair one chain acc = fmaf(q_k, c_k, acc), k ascending, from +0 (normalised inputs)."""
    acc = np.zeros((qn.shape[0], cn.shape[0]), F32)
    for k in range(qn.shape[1]):
        acc = fmaf(qn[:, k][:, None], cn[:, k][None, :], acc)
    return acc


def hit_list(score_row: np.ndarray, live: np.ndarray, limit: int) -> np.ndarray:
    """Entry indices of the `limit` live entries of the largest score: score descending, then entry ascending."""
    idx = np.flatnonzero(live)
    order = np.lexsort((idx, -score_row[idx].astype(F64)))
    return idx[order][:limit]


def aggregate(hits, top_k: int, weight: float, exclude=None, threshold: float | None = None, max_out: int | None = None):
    """hits: [(track, score, offset_sec)] in hit-list order -> [(track, chunk_count, final, base, bonus)], binary64."""
    groups: dict = {}
    for t, s, o in hits:
        groups.setdefault(t, []).append((float(s), float(o)))
    rows = []
    for t, ch in groups.items():  # order of first appearance
        if exclude is not None and t == exclude:
            continue
        m = min(top_k, len(ch))
        acc = 0.0
        for s, _ in ch[:m]:
            acc = acc + s
        base = acc / m
        bonus = min(len({o for _, o in ch}) / 5.0, 1.0) * weight
        rows.append((t, len(ch), base + bonus, base, bonus))
    rows.sort(key=lambda r: r[2], reverse=True)  # stable
    if threshold is not None:
        rows = [r for r in rows if r[2] >= threshold]
    if max_out is not None:
        rows = rows[:max_out]
    return rows


def detile(stored: np.ndarray, n: int, dim: int) -> np.ndarray:
    """The engine's stored layout (rows in tiles of 32; within a tile the float at (i, k) sits at
    ((k >> 3) * 2 + (k & 1)) * 128 + i * 4 + ((k & 7) >> 1)) back to [n][dim]."""
    tiles = (n + 31) // 32
    t = np.asarray(stored, F32).reshape(tiles, dim // 8, 2, 32, 4)  # [tile][g][h][i][j], k = 8g + 2j + h
    return np.ascontiguousarray(t.transpose(0, 3, 1, 4, 2).reshape(tiles * 32, dim)[:n])
