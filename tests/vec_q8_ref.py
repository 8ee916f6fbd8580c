"""numpy restatement of spec/FPSPEC.md 9.1 (the vector lane's int8 prefilter), built on tests/vec_ref.py: the
oracle of tests/test_vec_q8_host.py and tests/test_gpu_vector_q8.py, and the fixtures both share. A helper, not a
test module.

Everything the engine decides is restated: the quantiser (s, the int8 values, the residual e), approx, eps, R, the
first-stage candidates, tau, W and the route (prefilter or f32 fallback). numpy's float32 and float64 operations are
IEEE operations rounded one by one, which is what the spec pins.
"""

from __future__ import annotations

import numpy as np
import vec_ref as V

F32 = np.float32
F64 = np.float64
CAND_CAP = 4096  # kVecCandCap: the default cap on |W|
MAX_R = 1024


def quantize(y: np.ndarray):
    """[n][dim] float32 unit (or zero) vectors -> (i int8 [n][dim], s float32 [n], e float32 [n])."""
    y = np.ascontiguousarray(y, dtype=F32)
    a = np.abs(y).max(axis=1).astype(F32)
    s = (a / F32(127.0)).astype(F32)
    with np.errstate(all="ignore"):
        t = (y / s[:, None]).astype(F32)
    t[s == 0] = 0
    i = np.clip(np.rint(t), -127, 127).astype(np.int32)
    d = y.astype(F64) - s.astype(F64)[:, None] * i.astype(F64)
    d2 = d * d
    r2 = np.zeros(len(y), F64)
    for k in range(y.shape[1]):  # k ascending, one rounded add each
        r2 = r2 + d2[:, k]
    return i.astype(np.int8), s, np.sqrt(r2).astype(F32)


def approx(qi, qs, ci, cs) -> np.ndarray:
    """[nq][n] float32: (float)idot * (s_q * s_c), the product of the scales rounded first."""
    idot = qi.astype(np.int32) @ ci.astype(np.int32).T
    assert np.abs(idot).max(initial=0) < 2**24
    t = (qs.astype(F32)[:, None] * cs.astype(F32)[None, :]).astype(F32)
    return (idot.astype(F32) * t).astype(F32)


def eps(e_q, E, dim: int) -> np.ndarray:
    """(e_q + (1 + e_q) * E) * (1 + 2^-10) + dim * 2^-21 in binary64, left to right."""
    eq = np.asarray(e_q, dtype=F32).astype(F64)
    return (eq + (1.0 + eq) * F64(F32(E))) * F64(1.0 + 2.0**-10) + F64(dim) * F64(2.0**-21)


def candidates(limit: int, oversample: int) -> int:
    return min(MAX_R, max(limit, oversample * limit))


class Catalog:
    """The int8 view of stored unit vectors cn [n][dim] (dead rows included in E)."""

    def __init__(self, cn: np.ndarray):
        self.cn = np.ascontiguousarray(cn, dtype=F32)
        self.dim = cn.shape[1]
        self.ci, self.cs, self.ce = quantize(self.cn)
        self.E = F32(self.ce.max(initial=0))

    def view(self, qn: np.ndarray):
        """(approx [nq][n], eps [nq]) of normalised queries."""
        qi, qs, qe = quantize(qn)
        return approx(qi, qs, self.ci, self.cs), eps(qe, self.E, self.dim)


def route(approx_row, eps_q, score_row, live, limit: int, oversample: int = 4, cap: int = CAND_CAP):
    """One query -> dict(R, first, tau, W, fallback, hits): `first` the R live entries of largest approx (ties to the
    lower entry), tau the limit-th largest FPSPEC 9 score among them (None with fewer than `limit` live entries),
    W the live entries the bound cannot rule out, fallback = |W| > cap, hits = the best `limit` of W."""
    R = candidates(limit, oversample)
    first = V.hit_list(approx_row, live, R)
    idx = np.flatnonzero(live)
    if len(first) < limit:
        tau, W = None, idx
    else:
        tau = np.sort(score_row[first].astype(F64))[::-1][limit - 1]
        W = idx[approx_row[idx].astype(F64) >= tau - F64(eps_q)]
    order = np.lexsort((W, -score_row[W].astype(F64)))
    return dict(R=R, first=first, tau=tau, W=W, fallback=len(W) > cap, hits=W[order][:limit])


# ---- fixtures shared by the host and the GPU tests -------------------------------------------------------------

N, NTRACKS = 300, 40


class NearDup:
    """Fixture (c)/(d): entries [0, 200) differ from one vector by much less than a quantisation step (their approx
    values are equal or nearly so, their scores all differ), entries [200, 300) are unrelated. Queries 0..5 sit near
    the cluster, query 6 is all zero, queries 7..9 are stored unrelated entries."""

    DIM, NDUP = 512, 200

    def __init__(self, seed: int = 21):
        rng = np.random.default_rng(seed)
        dim = self.DIM
        b = rng.standard_normal(dim)
        cat = rng.standard_normal((N, dim))
        cat[: self.NDUP] = b + 2e-3 * rng.standard_normal((self.NDUP, dim))  # a step is ~0.03 at this scale
        self.cat = cat.astype(F32)
        q = np.zeros((10, dim))
        q[:6] = b + 0.3 * rng.standard_normal((6, dim))
        q[7:] = self.cat[[210, 250, 299]]
        self.q = q.astype(F32)
        self.dim = dim
        self.tracks = (np.arange(N) % NTRACKS).astype(np.uint32)
        self.chunk = (np.arange(N) // NTRACKS).astype(np.int32)
        self.off = (self.chunk % 6) * 5.0
        self.cn, self.qn = V.normalize(self.cat), V.normalize(self.q)
        self.S = V.scores(self.qn, self.cn)
        self.q8 = Catalog(self.cn)
        self.A, self.eps = self.q8.view(self.qn)


def asymmetric(dim: int, n: int = N, nq: int = 70, seed: int = 3):
    """Data of the lane-map check: every row, every column and every k differ in scale, so a swapped row, column or
    k pairing changes the integer sums. Returns raw (catalog, queries)."""
    rng = np.random.default_rng(seed + dim)
    kk = 1.0 + np.arange(dim) / dim
    cat = rng.standard_normal((n, dim)) * kk * (1.0 + np.arange(n) / n)[:, None]
    q = rng.standard_normal((nq, dim)) * kk[::-1] * (2.0 - np.arange(nq) / nq)[:, None]
    cat[:, 0] += 3.0  # no row is symmetric about zero
    q[:, 1] -= 2.0
    return cat.astype(F32), q.astype(F32)
