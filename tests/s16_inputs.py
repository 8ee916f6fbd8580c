"""int16 test inputs of the s16 PCM tests (spec/FPSPEC.md 8) and their exact widening.

The expected values of those tests come from the oracle applied to widen(q); the inputs must exercise the
conversion, which the synthetic tracks alone do not (their samples stay far from full scale): full-range random
samples and a full-scale square wave change their power bits under a wrong divisor, a missing sign extension or a
swapped halfword."""

import numpy as np

from aidfp import synth


def widen(q: np.ndarray) -> np.ndarray:
    """x = float(q) * 2^-15, exact in binary32: what every s16 path must compute on."""
    return (np.asarray(q).astype(np.float32) / np.float32(32768.0)).astype(np.float32)


def synth_q(track: int, start: int, n: int, sr: int, snr_db=None, salt: int = 0) -> np.ndarray:
    """aidfp.synth's clip before its final / 32768, as int16."""
    return synth.synth_int16(track, start, n, sr, synth.noise_halfwidth(snr_db), salt).astype(np.int16)


def random_q(n: int, seed: int, channels: int = 1) -> np.ndarray:
    """Uniform over the whole int16 range, seeded; both ends of the range are present from 2 samples on."""
    shape = n if channels == 1 else (n, channels)
    q = np.random.default_rng(seed).integers(-32768, 32768, shape, dtype=np.int64).astype(np.int16)
    if q.size >= 2:
        q.flat[q.size // 3], q.flat[2 * q.size // 3] = -32768, 32767
    return q


def square_q(n: int, period: int = 37) -> np.ndarray:
    """A full-scale square wave: -32768 and 32767, `period` samples each."""
    return np.where((np.arange(n) // period) % 2 == 0, -32768, 32767).astype(np.int16)
