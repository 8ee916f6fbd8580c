"""The oracle of the CLAP log-mel front end (tests/mel_ref.py, spec/FPSPEC.md 10) against what the reference runs:
the installed transformers ClapFeatureExtractor, captured by tests/golden/make_clap_fixtures.py into
tests/golden/ref_clap_mel.npz (inputs are regenerated here from their seed; only outputs are stored). No GPU.

Measured by the capture script (profiles/logmel_oracle_vs_transformers.txt), max |dB difference| to the extractor
over the named frames of the four inputs, both modes, both banks, by how far a band lies below its frame's maximum:
    oracle (binary32, FPSPEC 10):      0-20 dB 7.6e-06   20-40 dB 1.9e-05   40-60 dB 9.5e-05   > 60 dB 4.4e-01
    scipy.fft.rfft on float32:         0-20 dB 7.6e-06   20-40 dB 4.6e-05   40-60 dB 1.8e-04   > 60 dB 4.2e-01
Within 60 dB the oracle deviates 0.54 x what a library binary32 FFT does. The asserted bound for bands within 60 dB
is 2 x the oracle's captured maximum (both sides are deterministic; the factor covers libm differences between
machines). Below 60 dB every binary32 FFT is at its noise floor, as the scipy row shows; that class is reported only.
"""

from pathlib import Path

import numpy as np
import pytest

import mel_ref as R

GOLD = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD / "ref_clap_mel.npz")


@pytest.fixture(scope="module")
def banks():
    return {"slaney": R.bank(R.SLANEY, 50.0, 14000.0), "htk": R.bank(R.HTK, 50.0, 14000.0)}


@pytest.mark.parametrize("name,kind", [("slaney", R.SLANEY), ("htk", R.HTK)])
@pytest.mark.parametrize("fmin", [50, 0])
def test_banks_equal_the_extractors(gold, name, kind, fmin):
    """Same supports, every weight within 1 binary32 ulp (both are binary64 results rounded once)."""
    W = R.bank(kind, float(fmin), 14000.0)
    lo, hi, K = R.supports(W)
    assert np.array_equal(lo, gold[f"bank_{name}_{fmin}_lo"]) and np.array_equal(hi, gold[f"bank_{name}_{fmin}_hi"])
    assert K == 299
    got = np.concatenate([W[lo[m]:hi[m], m] for m in range(64)])
    want = gold[f"bank_{name}_{fmin}_w"].astype(np.float32)
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(want).astype(np.float64))


def test_fft_is_not_worse_than_a_library_binary32_fft(gold):
    """If the oracle's within-60 dB figure were more than 10 x scipy's binary32 FFT, the spec's FFT would be wrong."""
    assert float(gold["oracle_within60"]) <= 10.0 * float(gold["scipy_within60"])
    assert float(gold["oracle_within60"]) < 1e-3  # and the figure itself is a rounding-level one, in dB


@pytest.mark.parametrize("mode", ["zero", "repeatpad"])
@pytest.mark.parametrize("i", range(4))
def test_oracle_against_captured_extractor(gold, banks, mode, i):
    n = R.FIXTURE_LENGTHS[i]
    x = R.fixture_input(i)
    fill = n if mode == "zero" else (R.L // n) * n
    frames = R.fixture_frames(n, fill)
    assert np.array_equal(gold[f"frames_{mode}_{i}"], frames)
    bound = 2.0 * float(gold["oracle_within60"])
    P = R.power(R.frame_samples(x, 0, n, fill, frames), 299)
    for name, W in banks.items():
        ref = gold[f"mel_{mode}_{name}_{i}"]
        got = R.mel_db(P, W)
        dev = R.deviation_classes(got, ref)
        print(f"input {i} {mode} {name}: 0-20 / 20-40 / 40-60 / > 60 dB below the frame maximum: {dev}")
        assert all(d is None or d <= bound for d in dev[:3]), (name, dev, bound)


def test_oracle_against_live_extractor(gold, banks):
    """The same comparison on a fresh seed, through the installed extractor itself."""
    tr = pytest.importorskip("transformers")
    import warnings

    x = R.fixture_input(1, seed=977)
    n = len(x)
    frames = R.fixture_frames(n, (R.L // n) * n)
    P = R.power(R.frame_samples(x, 0, n, (R.L // n) * n, frames), 299)
    bound = 2.0 * float(gold["oracle_within60"])
    for name, trunc in (("slaney", "rand_trunc"), ("htk", "fusion")):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fe = tr.ClapFeatureExtractor(frequency_min=50, frequency_max=14000, truncation=trunc, padding="repeatpad")
            ref = fe(x, sampling_rate=R.SR, return_tensors="np")["input_features"][0][0][frames].astype(np.float32)
        dev = R.deviation_classes(R.mel_db(P, banks[name]), ref)
        print(f"live {name}: {dev}")
        assert all(d is None or d <= bound for d in dev[:3]), (name, dev, bound)


def test_db10_against_float64():
    """The pinned 10 log10 over the reachable range [1e-10, 2^40]. Bound from its steps: the last fma rounds the
    result once (half an ulp of D); before it, the Horner chain's last step (half an ulp of 4.34, times |f| <= 0.4143),
    the earlier steps (each shrunk by |f|), the product f * q and the C_lo fma (half an ulp of 1.5 each) add less than
    4e-7 in all; the degree-10 polynomial itself is off by 1.1e-9. Measured: 4.05e-6 dB and 2.13 ulp at most, 93 % of
    the results correctly rounded."""
    rng = np.random.default_rng(5)
    M = np.concatenate([
        np.exp(rng.uniform(np.log(1e-10), np.log(2.0**40), 400000)),
        1.0 + rng.uniform(-1e-3, 1e-3, 50000),
        np.sqrt(2.0) * 2.0 ** rng.integers(-34, 40, 50000) * (1.0 + rng.uniform(-1e-6, 1e-6, 50000)),
        [1e-10, 1.0, 2.0**40]]).astype(np.float32)
    M = M[M >= R.MEL_FLOOR]
    got = R.db10(M).astype(np.float64)
    ref = 10.0 * np.log10(M.astype(np.float64))
    err = np.abs(got - ref)
    print("max abs", err.max(), "max ulp", (err / np.spacing(np.abs(ref).astype(np.float32))).max())
    assert np.all(err <= 0.5 * np.spacing(np.abs(got).astype(np.float32)).astype(np.float64) + 4e-7)
    assert R.db10(np.float32([1e-10]))[0] == np.float32(-100.0)  # silence
    assert R.db10(np.float32([1.0]))[0] == 0.0


def test_chunk_plan_equals_chunk_audio():
    import json

    g = json.loads((GOLD / "ref_clap_chunks.json").read_text())
    for n in g["lengths"]:
        assert [[off, idx, dur] for _, _, off, idx, dur in R.chunk_plan(n)] == g["chunks"][str(n)], n


def test_reflect_not_symmetric():
    """u[-1] = v[1] and u[L] = v[L - 2]: the edge sample itself is not repeated."""
    x = np.arange(R.L, dtype=np.float32)
    u = R.frame_samples(x, 0, R.L, R.L, [0, 1000])
    assert u[0, 511] == 1 and u[0, 512] == 0 and u[0, 0] == 512
    assert u[1, 511] == R.L - 1 and u[1, 512] == R.L - 2 and u[1, 1023] == R.L - 513
