"""The oracle of the content fingerprint (tests/chroma_ref.py, spec/FPSPEC.md 11) checked on the host: the known
answer of silence, the binary32 pipeline against its float64 restatement (np.fft.rfft, log1p) on six seeded 20 s
inputs, the ratio form of the classifiers against the log form, what the words mean for dedup at the reference's own
threshold, and the text form of a fingerprint.

Measured on the six inputs (recorded in FPSPEC 11): the chroma rows differ from float64 by at most 1.74e-6 relative
per element, asserted here with a 4x margin; no word bit differs (0 of 26,880), capped here at twice that count plus
2 bits per input, since one classifier flip changes at most 2 bits; the ratio test and the log form agree on all
40,320 decisions."""

import numpy as np
import pytest

import chroma_ref as R

ROWS_REL_MEASURED = 1.74e-6
BITS_MEASURED = 0


@pytest.fixture(scope="module")
def inputs():
    out = []
    for s in range(6):
        x = R.song(100 + s, 20.0)
        C = R.rows(x)
        out.append({"x": x, "C": C, "F": R.features(C)})
    return out


def test_silence_known_answer():
    w = R.words(np.zeros(40000, np.float32))
    assert len(w) == R.n_words(40000) == 8 and np.all(w == np.uint32(627964279)) and R.ZERO_WORD == 0x256DF977
    assert len(R.words(np.zeros(30030, np.float32))) == 0 and len(R.words(np.zeros(30031, np.float32))) == 1
    assert np.all(R.features(R.rows(np.zeros(40000, np.float32))) == 0)


def test_rows_against_float64(inputs):
    worst = 0.0
    for d in inputs:
        C64 = R.rows64(d["x"])
        assert d["C"].shape == C64.shape == (R.n_frames(len(d["x"])), 12) and np.all(C64 > 0)
        worst = max(worst, float(np.max(np.abs(d["C"].astype(np.float64) - C64) / C64)))
    print(f"chroma rows, max relative error against float64: {worst:.3g}")
    assert worst <= 4 * ROWS_REL_MEASURED


def test_words_against_float64(inputs):
    for d in inputs:
        w, w64 = R.words_from_features(d["F"]), R.words64(d["x"])
        assert len(w) == len(w64) == R.n_words(len(d["x"])) == 140
        bits = R.differing_bits(w, w64)
        print(f"differing word bits against float64: {bits} of {32 * len(w)}")
        assert bits <= 2 * BITS_MEASURED + 2


def test_ratio_test_equals_log_form(inputs):
    n = 0
    for d in inputs:
        a, b = R.areas(d["F"])
        ratio, log = R.decisions_ratio(a, b), R.decisions_log(a, b)
        assert np.array_equal(ratio, log)
        n += ratio.size
        assert 0.05 < ratio.mean() < 0.95  # both outcomes occur
    assert n == 6 * 140 * 16 * 3


def test_dedup_meaning_at_the_reference_threshold():
    x = R.song(200, 20.0)
    w = R.words(x)
    copy = R.similarity(w, R.words(R.add_noise(x, 20.0, 1)))
    others = [R.words(R.song(300 + s, 10.0)) for s in range(6)]
    worst = max(R.similarity(others[i], others[j]) for i in range(6) for j in range(i + 1, 6))
    print(f"copy at SNR 20 dB: {copy:.4f}; unrelated songs: at most {worst:.4f}")
    assert copy >= 0.85 and worst < 0.85
    assert R.similarity(w, w) == 1.0 and R.similarity(w, R.words((x / np.float32(32)).astype(np.float32))) == 1.0


def test_stages_compose(inputs):
    d = inputs[0]
    fr = R.frame_samples(d["x"], [0, 7])
    assert fr.shape == (2, 4096) and np.array_equal(fr[1], d["x"][7 * 1365:7 * 1365 + 4096])
    P = R.power(fr)
    assert P.shape == (2, 1298) and np.array_equal(R.chroma(P), d["C"][[0, 7]])
    assert np.array_equal(R.rows(d["x"], [0, 7]), d["C"][[0, 7]])
    assert np.array_equal(R.words_from_rows(d["C"]), R.words(d["x"]))
    nz = d["F"].any(axis=1)
    norm = np.sqrt((d["F"].astype(np.float64) ** 2).sum(axis=1))
    assert nz.all() and np.all(np.abs(norm - 1.0) < 1e-6)


def test_fingerprint_text_round_trip():
    from aidfp.chroma import format_fingerprint
    from aidfp.dedup import parse_fingerprint

    w = np.array([0, 1, 627964279, 2**31 - 1, 2**31, 2**31 + 5, 2**32 - 1], dtype=np.uint32)
    s = format_fingerprint(w)
    assert s == "0,1,627964279,2147483647,-2147483648,-2147483643,-1"
    assert np.array_equal(parse_fingerprint(s), w) and parse_fingerprint(s).dtype == np.uint32
    assert format_fingerprint(parse_fingerprint("-5,7")) == "-5,7"
    words = R.words(R.song(5, 4.0))
    assert np.array_equal(parse_fingerprint(format_fingerprint(words)), words) and (words >= 2**31).any()
