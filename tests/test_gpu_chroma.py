"""K11 (csrc/chroma.hip: aid_chroma_rows, aid_chroma, aid_chroma_words) against the oracle tests/chroma_ref.py
(spec/FPSPEC.md 11). Every comparison is for equality: of the float values of the chroma rows, of the words.

The batch: clips of 4096 samples (one frame), 30031 (the first length with a word), 31395 / 31396 (20 / 21 frames),
and 4096 + 1365 * 2R -+ 1 (2R and 2R + 1 frames: a last run that is full, and one of a single frame), R = the frames
of a K11a workgroup. One-sample fillers between them put every clip at an odd sample offset, so s16 clips start at
2-byte and f32 clips at 4-byte alignment only."""

import ctypes

import numpy as np
import pytest

import chroma_ref as R

pytestmark = pytest.mark.gpu
HOST, DEVICE = 0, 1
RUN = 4  # kChromaRun (aidfp_chroma_plan.h), AID_CHROMA_RUN
LENGTHS = [4096, 30031, 31395, 31396, 4096 + 1365 * 2 * RUN - 1, 4096 + 1365 * 2 * RUN + 1]


def p(a):
    return ctypes.c_void_p(a.ctypes.data)


def quantise(x):
    return np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)


class Batch:
    """The clips packed at odd offsets, in both formats, with the oracle's rows and words per clip (computed once)."""

    def __init__(self):
        from aidfp import _lib

        assert _lib.AID_CHROMA_RUN == RUN
        rng = np.random.default_rng(20261021)
        src = R.song(7, 6.0)
        parts, self.real = [], []
        pos = 0
        for n in LENGTHS:
            fill = 1 if pos % 2 == 0 else 2  # the next clip starts at an odd offset
            parts.append((0.01 * rng.standard_normal(fill)).astype(np.float32))
            pos += fill
            start = int(rng.integers(0, len(src) - n))
            parts.append((src[start:start + n] * np.float32(0.8)).astype(np.float32))
            self.real.append(len(parts) - 1)
            assert pos % 2 == 1
            pos += n
        self.off = np.zeros(len(parts) + 1, np.int64)
        self.off[1:] = np.cumsum([len(q) for q in parts])
        self.pcm = {"f32": np.concatenate(parts)}
        self.pcm["s16"] = quantise(self.pcm["f32"])
        self.clips = {"f32": parts, "s16": [R.s16_to_f32(quantise(q)) for q in parts]}
        self.rows = {f: [R.rows(c) for c in self.clips[f]] for f in ("f32", "s16")}
        self.words = {f: [R.words_from_rows(c) for c in self.rows[f]] for f in ("f32", "s16")}
        frames = [len(r) for r in self.rows["f32"]]
        assert [frames[i] for i in self.real] == [1, 20, 20, 21, 2 * RUN, 2 * RUN + 1]
        assert [len(self.words["f32"][i]) for i in self.real] == [0, 1, 1, 2, 0, 0]


@pytest.fixture(scope="module")
def batch():
    return Batch()


def fn(eng, name, fmt):
    return getattr(eng._lib, name if fmt == "f32" else name + "_pcm16")


def run_rows(eng, pcm, off, fmt, loc):
    import torch

    keep = torch.from_numpy(pcm).cuda() if loc == DEVICE else pcm
    ptr = ctypes.c_void_p(keep.data_ptr()) if loc == DEVICE else p(keep)
    if loc == DEVICE:
        torch.cuda.synchronize()
    n = len(off) - 1
    roff = np.zeros(n + 1, np.int64)
    got = ctypes.c_int64(-1)
    total = sum(R.n_frames(int(m)) for m in np.diff(off))
    out = np.full((max(1, total), 12), np.nan, np.float32)
    rc = fn(eng, "aid_chroma_rows", fmt)(eng._h, ptr, p(off), n, loc, p(out), p(roff), total, ctypes.byref(got), None)
    assert rc == 0 and got.value == total
    return [out[roff[c]:roff[c + 1]] for c in range(n)]


def run_words(eng, pcm, off, fmt, loc=HOST, cap=None):
    n = len(off) - 1
    woff = np.full(n + 1, -7, np.int64)
    got = ctypes.c_int64(-1)
    total = sum(R.n_words(int(m)) for m in np.diff(off))
    cap = total if cap is None else cap
    out = np.full(max(1, total), 0xDEADBEEF, np.uint32)
    rc = fn(eng, "aid_chroma", fmt)(eng._h, p(pcm), p(off), n, loc, p(out), p(woff), cap, HOST, ctypes.byref(got), None)
    return rc, got.value, out, woff


@pytest.mark.parametrize("loc", [HOST, DEVICE])
@pytest.mark.parametrize("fmt", ["f32", "s16"])
def test_rows_equal_oracle(gpu_engine, batch, fmt, loc):
    got = run_rows(gpu_engine, batch.pcm[fmt], batch.off, fmt, loc)
    for c, (g, want) in enumerate(zip(got, batch.rows[fmt])):
        assert g.shape == want.shape, c
        bad = np.argwhere(g != want)
        assert len(bad) == 0, (c, len(want), bad[0], g[tuple(bad[0])], want[tuple(bad[0])], len(bad))
    assert all(np.all(batch.rows[fmt][i] > 0) for i in batch.real)


@pytest.mark.parametrize("fmt", ["f32", "s16"])
def test_words_equal_oracle(gpu_engine, batch, fmt):
    rc, n, out, woff = run_words(gpu_engine, batch.pcm[fmt], batch.off, fmt)
    want = batch.words[fmt]
    assert rc == 0 and n == 4
    assert np.array_equal(woff, np.concatenate([[0], np.cumsum([len(w) for w in want])]))
    assert np.array_equal(out[:n], np.concatenate(want))


def test_30030_samples_give_no_word(gpu_engine):
    x = R.song(8, 6.0)
    pcm = np.concatenate([x[:30030], x[:30031], x[:4095], x[100:30131]])
    off = np.array([0, 30030, 60061, 64156, 94187], np.int64)
    rc, n, out, woff = run_words(gpu_engine, pcm, off, "f32")
    assert rc == 0 and n == 2 and list(woff) == [0, 0, 1, 1, 2]
    assert out[0] == R.words(x[:30031])[0] and out[1] == R.words(x[100:30131])[0]
    L = gpu_engine._lib
    assert [L.aid_chroma_len(m) for m in (0, 4095, 30030, 30031, 31395, 31396)] == [0, 0, 0, 1, 1, 2]


def test_zero_clip_known_answer(gpu_engine):
    import torch

    for fmt, dt in (("f32", np.float32), ("s16", np.int16)):
        pcm = np.zeros(40001, dt)
        off = np.array([0, 1, 40001], np.int64)
        rc, n, out, woff = run_words(gpu_engine, pcm, off, fmt)
        assert rc == 0 and n == R.n_words(40000) == 8 and list(woff) == [0, 0, 8]
        assert np.all(out[:n] == np.uint32(R.ZERO_WORD)) and R.ZERO_WORD == 0x256DF977
    # device input and device output
    x = torch.zeros(40000, dtype=torch.float32, device="cuda")
    w = torch.zeros(8, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    got = ctypes.c_int64()
    off = np.array([0, 40000], np.int64)
    woff = np.zeros(2, np.int64)
    rc = gpu_engine._lib.aid_chroma(gpu_engine._h, ctypes.c_void_p(x.data_ptr()), p(off), 1, DEVICE,
                                    ctypes.c_void_p(w.data_ptr()), p(woff), 8, DEVICE, ctypes.byref(got), None)
    assert rc == 0 and got.value == 8
    torch.cuda.synchronize()
    assert np.all(w.cpu().numpy().view(np.uint32) == np.uint32(R.ZERO_WORD))


def test_normaliser_takes_both_branches(gpu_engine):
    """The clip is scaled so that r = |G| lies on either side of 0.01 from row to row."""
    x = R.song(9, 6.0)
    C = R.rows(x)
    T = len(C)
    G = 0.25 * C[0:T - 4] + 0.75 * C[1:T - 3] + C[2:T - 2] + 0.75 * C[3:T - 1] + 0.25 * C[4:T]
    r = np.sqrt((G.astype(np.float64) ** 2).sum(axis=1))
    y = (x * np.float32(np.sqrt(0.01 / np.median(r)))).astype(np.float32)  # P and r scale with the gain squared
    F = R.features(R.rows(y))
    zero = ~F.any(axis=1)
    assert zero.sum() >= 5 and (~zero).sum() >= 5 and np.any(zero[1:] != zero[:-1])
    want = R.words_from_features(F)
    rc, n, out, _ = run_words(gpu_engine, y, np.array([0, len(y)], np.int64), "f32")
    assert rc == 0 and n == len(want) and np.array_equal(out[:n], want)


def test_capacity_one_too_small(gpu_engine, batch):
    from aidfp import _lib

    rc, n, out, woff = run_words(gpu_engine, batch.pcm["f32"], batch.off, "f32", cap=3)
    assert rc == _lib.AID_ERR_INVALID and n == 4 and "capacity" in _lib.last_error()
    assert np.all(out == np.uint32(0xDEADBEEF)) and np.all(woff == -7)


# ---- K11b alone ----
@pytest.fixture
def printer(gpu_engine):
    from aidfp.chroma import ChromaPrinter

    return ChromaPrinter(gpu_engine)


def test_every_cell_of_the_image(printer):
    """Per cell of the 16 x 12 image an item whose only non-zero cell is that one (192 cells, a small and a large
    value each): every rectangle edge of all six classifier types."""
    items = []
    for v in (0.75, 30.0):
        for x in range(16):
            for y in range(12):
                F = np.zeros((16, 12), np.float32)
                F[x, y] = v
                items.append(F)
    got = printer.words_from_rows(items, raw_features=True)
    want = [R.words_from_features(F) for F in items]
    assert all(len(g) == 1 for g in got)
    assert np.array_equal(np.concatenate(got), np.concatenate(want))
    flat = np.concatenate(want)
    for j in range(16):  # every classifier's two bits move for some cell
        assert len({int(w >> (2 * (15 - j))) & 3 for w in flat}) > 1, j


def test_threshold_equality_counts_as_reached(printer):
    """Per classifier and threshold an item with b = 0 and a = E_i - 1, so A == E_i * B exactly, where E_i - 1 and
    1 + (E_i - 1) are exact in binary32; the next value below E_i must not reach it."""
    items, at = [], []
    for j in range(16):
        ra, _ = R.rects(j)
        x, _, y, _ = ra[0]
        for i in range(3):
            a = np.float32(np.float64(R.E[j, i]) - 1.0)
            if np.float64(a) != np.float64(R.E[j, i]) - 1.0 or np.float32(1) + a != R.E[j, i]:
                continue
            for v in (a, np.nextafter(a, np.float32(-2))):
                F = np.zeros((16, 12), np.float32)
                F[x, y] = v
                items.append(F)
                at.append((j, i, bool(np.float32(1) + v >= R.E[j, i])))
    assert len(items) >= 2 * 30  # most of the 48 thresholds are representable
    want = []
    for F, (j, i, reached) in zip(items, at):
        a, b = R.areas(F)
        assert b[0, j] == 0 and bool(R.decisions_ratio(a, b)[0, j, i]) == reached
        want.append(R.words_from_features(F))
    assert any(r for *_, r in at) and any(not r for *_, r in at)
    got = printer.words_from_rows(items, raw_features=True)
    assert np.array_equal(np.concatenate(got), np.concatenate(want))


def test_items_stay_inside_their_clip(printer):
    rng = np.random.default_rng(5)
    feats = [rng.random((20, 12), dtype=np.float32), rng.random((15, 12), dtype=np.float32),
             rng.random((25, 12), dtype=np.float32), rng.random((16 + 240 + 3, 12), dtype=np.float32)]
    got = printer.words_from_rows(feats, raw_features=True)
    assert [len(g) for g in got] == [5, 0, 10, 244]  # the last clip spans two workgroups
    for g, F in zip(got, feats):
        assert np.array_equal(g, R.words_from_features(F))
    rows = [(rng.random((24, 12), dtype=np.float32) * np.float32(3.0)), rng.random((19, 12), dtype=np.float32),
            rng.random((21, 12), dtype=np.float32)]
    got = printer.words_from_rows(rows)
    assert [len(g) for g in got] == [5, 0, 2]
    for g, C in zip(got, rows):
        assert np.array_equal(g, R.words_from_rows(C))
