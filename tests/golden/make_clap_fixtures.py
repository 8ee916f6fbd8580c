"""Capture the reference's CLAP front end as fixtures.

Runs ONLY in the build container: it imports `chunk_audio` from the reference (/root/reference, read-only; nothing of
it is copied or shipped) and the installed `transformers.ClapFeatureExtractor` (constructed from its arguments: no
download, no weights). Output:

  tests/golden/ref_clap_chunks.json   chunk_audio's (offset_sec, chunk_index, duration_sec) tuples per length
  tests/golden/ref_clap_mel.npz       both filter banks (fmin 50 and the class default 0), stored by band support,
                                      and the extractor's output at the named frames of four inputs
                                      (tests/mel_ref.py fixture_input, regenerated from a seed: only outputs are
                                      stored), zero mode through chunk_audio and repeatpad through the extractor
  profiles/logmel_oracle_vs_transformers.txt   what the oracle (tests/mel_ref.py) deviates from the extractor on
                                      those inputs, and what a library binary32 FFT (scipy.fft.rfft on float32) does

Run: python tests/golden/make_clap_fixtures.py
"""

from __future__ import annotations

import json
import sys
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
REF = Path("/root/reference/audio-ident-service")
LENGTHS = [0, 1, 47999, 48000, 287999, 288000, 479999, 480000, 480001, 720000, 86400000]
CLASSES = ("0-20 dB", "20-40 dB", "40-60 dB", "> 60 dB")


def pack_bank(W: np.ndarray):
    lo = np.array([np.flatnonzero(W[:, m])[0] for m in range(64)], np.int32)
    hi = np.array([np.flatnonzero(W[:, m])[-1] + 1 for m in range(64)], np.int32)
    assert all(np.all(W[lo[m]:hi[m], m] != 0) for m in range(64))
    return lo, hi, np.concatenate([W[lo[m]:hi[m], m] for m in range(64)]).astype(np.float64)


def scipy_f32_logmel(u: np.ndarray, W64: np.ndarray) -> np.ndarray:
    """The same frames through a library binary32 FFT: float32 window product, scipy.fft.rfft on float32 (complex64),
    then the extractor's own float64 tail."""
    import scipy.fft

    import mel_ref as R

    X = scipy.fft.rfft((u * R.WIN[None, :]).astype(np.float32), axis=1)
    assert X.dtype == np.complex64
    P = np.abs(X, dtype=np.float64) ** 2
    return (10.0 * np.log10(np.maximum(1e-10, P @ W64))).astype(np.float32)


def main() -> None:
    sys.path.insert(0, str(REF))
    sys.path.insert(0, str(ROOT / "tests"))
    warnings.simplefilter("ignore")
    from app.audio.embedding import chunk_audio
    from transformers import ClapFeatureExtractor

    import mel_ref as R

    chunks = {}
    for n in LENGTHS:
        got = chunk_audio(np.zeros(n, np.float32).tobytes())
        assert all(len(a) == R.L for a, *_ in got)
        chunks[str(n)] = [[float(off), int(idx), float(dur)] for _, off, idx, dur in got]
    (HERE / "ref_clap_chunks.json").write_text(json.dumps({"lengths": LENGTHS, "chunks": chunks}, indent=0) + "\n")

    out = {}
    fe = {}
    for fmin in (50, 0):
        for kind, trunc in (("slaney", "rand_trunc"), ("htk", "fusion")):
            fe[(kind, fmin)] = ClapFeatureExtractor(frequency_min=fmin, frequency_max=14000, truncation=trunc,
                                                    padding="repeatpad")
            W = getattr(fe[(kind, fmin)], "mel_filters_slaney" if kind == "slaney" else "mel_filters")
            out[f"bank_{kind}_{fmin}_lo"], out[f"bank_{kind}_{fmin}_hi"], out[f"bank_{kind}_{fmin}_w"] = pack_bank(W)

    worst = {"oracle": [0.0] * 4, "scipy": [0.0] * 4}
    lines = []
    for i, n in enumerate(R.FIXTURE_LENGTHS):
        x = R.fixture_input(i)
        for mode in ("zero", "repeatpad"):
            if mode == "zero":
                wave = chunk_audio(x.tobytes())[0][0]  # the zero-padded chunk the reference hands its processor
                fill = n
            else:
                wave = x  # the extractor repeats and pads
                fill = (R.L // n) * n
            frames = R.fixture_frames(n, fill)
            out[f"frames_{mode}_{i}"] = np.array(frames, np.int32)
            u = R.frame_samples(x, 0, n, fill, frames)
            for kind, code in (("slaney", R.SLANEY), ("htk", R.HTK)):
                ext = fe[(kind, 50)]
                feat = ext(wave, sampling_rate=R.SR, return_tensors="np")["input_features"][0]
                ref = np.ascontiguousarray(feat[0][frames]).astype(np.float32)  # fusion: four copies of the same image
                out[f"mel_{mode}_{kind}_{i}"] = ref
                W64 = getattr(ext, "mel_filters_slaney" if kind == "slaney" else "mel_filters")
                W = R.bank(code, 50.0, 14000.0)
                for who, got in (("oracle", R.mel_db(R.power(u, R.supports(W)[2]), W)), ("scipy", scipy_f32_logmel(u, W64))):
                    dev = R.deviation_classes(got, ref)
                    worst[who] = [max(a, b or 0.0) for a, b in zip(worst[who], dev)]
                    lines.append(f"input {i} (n = {n}) {mode:9s} {kind:6s} {who:6s} " +
                                 "  ".join(f"{c}: {'-' if d is None else format(d, '.3e')}" for c, d in zip(CLASSES, dev)))
    out["oracle_within60"] = np.float64(max(worst["oracle"][:3]))
    out["scipy_within60"] = np.float64(max(worst["scipy"][:3]))
    np.savez_compressed(HERE / "ref_clap_mel.npz", **out)
    head = ["max |dB - ClapFeatureExtractor dB| at the fixtures' named frames, by how far a band lies below its frame's maximum",
            "oracle = tests/mel_ref.py (FPSPEC 10, binary32); scipy = scipy.fft.rfft on float32, float64 tail",
            "overall oracle: " + "  ".join(f"{c}: {d:.3e}" for c, d in zip(CLASSES, worst["oracle"])),
            "overall scipy:  " + "  ".join(f"{c}: {d:.3e}" for c, d in zip(CLASSES, worst["scipy"])),
            f"within 60 dB: oracle {float(out['oracle_within60']):.3e}, scipy {float(out['scipy_within60']):.3e}, "
            f"ratio {float(out['oracle_within60']) / float(out['scipy_within60']):.2f}", ""]
    (ROOT / "profiles" / "logmel_oracle_vs_transformers.txt").write_text("\n".join(head + lines) + "\n")
    print("\n".join(head))


if __name__ == "__main__":
    main()
