"""Vector lane (spec/FPSPEC.md 9), host side: the oracle's own arithmetic is checked against libm and against
vectors captured from the reference, and the new C ABI is present and refuses bad calls without a device."""

import ctypes
import ctypes.util
import json
from pathlib import Path

import numpy as np
import pytest
import vec_ref as V

from aidfp import _lib

GOLDEN = Path(__file__).resolve().parent / "golden" / "ref_vibe.json"
NEW_SYMBOLS = ["aid_vec_reset", "aid_vec_add", "aid_vec_remove", "aid_vec_compact", "aid_vec_count", "aid_vec_search",
               "aid_vec_scores", "aid_vec_aggregate", "aid_vibe_lane", "aid_vec_save", "aid_vec_load", "aid_vec_stats"]


@pytest.fixture(scope="module")
def libm_fmaf():
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.fmaf.restype = ctypes.c_float
    m.fmaf.argtypes = [ctypes.c_float] * 3
    return lambda a, b, c: np.array([m.fmaf(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], np.float32)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def test_fmaf_emulation_random_triples(libm_fmaf):
    rng = np.random.default_rng(1)
    n = 200_000
    a = rng.standard_normal(n).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    c = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, size=n)).astype(np.float32)
    c[::5] = (-(a[::5].astype(np.float64) * b[::5])).astype(np.float32)  # cancellation: the result is the product's tail
    assert np.array_equal(bits(V.fmaf(a, b, c)), bits(libm_fmaf(a, b, c)))


def test_fmaf_emulation_tie_cases(libm_fmaf):
    a, b, c = V.tie_cases(2000)
    want = libm_fmaf(a, b, c)
    assert np.array_equal(bits(V.fmaf(a, b, c)), bits(want))
    # the cases are what they claim to be: a float64 multiply-add rounds a good part of them the wrong way
    assert np.count_nonzero(bits(V.fmaf_naive(a, b, c)) != bits(want)) > 100


def test_detile_inverts_the_stored_layout():
    n, dim = 45, 64
    x = np.arange(n * dim, dtype=np.float32).reshape(n, dim)
    stored = np.zeros(((n + 31) // 32) * 32 * dim, np.float32)
    for r in range(n):
        for k in range(dim):
            stored[(r >> 5) * 32 * dim + ((k >> 3) * 2 + (k & 1)) * 128 + (r & 31) * 4 + ((k & 7) >> 1)] = x[r, k]
    assert np.array_equal(V.detile(stored, n, dim), x)


def test_aggregation_reproduces_reference_vectors():
    cases = json.loads(GOLDEN.read_text())["cases"]
    assert len(cases) >= 35
    for c in cases:
        hits = [(h["track"], np.float32(h["score"]), h["offset_sec"]) for h in c["hits"]]
        assert all(float(np.float32(h["score"])) == h["score"] for h in c["hits"])  # float32 values stored as floats
        got = V.aggregate(hits, c["top_k_per_track"], c["diversity_weight"], c["exclude"])
        want = [(r["track"], r["chunk_count"], r["final_score"], r["base_score"], r["diversity_bonus"]) for r in c["rows"]]
        assert got == want, c["note"]


def test_new_symbols_in_signature_table():
    names = {n for n, _, _ in _lib.SIGNATURES}
    assert not [s for s in NEW_SYMBOLS if s not in names]
    assert (_lib.AID_FORCE_VEC_PATH, _lib.AID_FORCE_VEC_CHUNK) == (10, 11)
    assert ctypes.sizeof(_lib.AidVecHit) == 24 and ctypes.sizeof(_lib.AidVibeRow) == 32


def test_null_engine_and_bad_arguments_are_refused_without_a_device():
    L = _lib.load()
    q = np.zeros(512, np.float32)
    p = ctypes.c_void_p(q.ctypes.data)
    n = ctypes.c_int64()
    inv = _lib.AID_ERR_INVALID
    assert L.aid_vec_reset(None, 512) == inv
    assert L.aid_vec_reset(None, 500) == inv
    assert L.aid_vec_add(None, p, p, p, p, 1, _lib.AID_PCM_HOST) == inv
    assert L.aid_vec_remove(None, 0) == inv
    assert L.aid_vec_compact(None, ctypes.byref(n)) == inv
    assert L.aid_vec_count(None, ctypes.byref(n), ctypes.byref(n), None) == inv
    assert L.aid_vec_search(None, p, 1, _lib.AID_PCM_HOST, 50, p, p, None) == inv
    assert L.aid_vec_search(None, p, 1, _lib.AID_PCM_HOST, 0, p, p, None) == inv
    assert L.aid_vec_scores(None, p, 1, _lib.AID_PCM_HOST, p, 1) == inv
    assert L.aid_vec_aggregate(None, p, p, 1, 3, 0.05, None, 0.0, 1, p, p) == inv
    assert L.aid_vibe_lane(None, p, 1, _lib.AID_PCM_HOST, 2000, 3, 0.05, None, 0.6, 1, p, p, None) == inv
    assert L.aid_vec_save(None, b"/nonexistent") == inv
    assert L.aid_vec_load(None, b"/nonexistent") == inv
    assert "null engine" in _lib.last_error()
