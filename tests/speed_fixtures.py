"""The fixture of the speed-lane tests (spec/FPSPEC.md 8.2, 7.1): a small 16 kHz catalog, captures of its tracks played
fast or slow, and the all-oracle route every engine result is compared with.

Catalog: 8 synthetic tracks of 12 s at 16 kHz, indexed from the oracle's records. Clips: int16 captures at 48 kHz
stereo and at 16 kHz mono of known tracks at true speeds +20, -30 and +13 per mille, one at the nominal speed, one
of a track the catalog does not hold and one too short for any frame. A capture at speed pm is the track synthesised
at the capture rate and resampled by the oracle for the rate pair (1000 + pm, 1000): tempo and pitch move together,
and the capture is shorter when played fast. Each channel then gets white noise of sigma 0.01 before it is quantised.

The grid is (-30, -20, -2, 0, 2, 12, 14, 20, 22): +20 and -30 are on it, +13 lies 1 per mille from 12 and from 14.

The oracle route of a clip: per speed oracle.resample(x, sr_in * 1000, 16000 * (1000 + pm)), aidfp.exact's lane over
the oracle's fingerprint and matcher (as tests/test_gpu_s16_extract.py::test_exact_lane_equals_oracle_lane), then
aidfp.exact.select_speed. tests/test_speed_fixtures_host.py asserts what the GPU tests rely on, with the oracle
alone."""

import asyncio
import functools
import uuid
from dataclasses import dataclass

import numpy as np

import oracle as O
from aidfp import exact as ex
from aidfp.fingerprint import OlafMatch
from s16_inputs import synth_q, widen

SR_E, HOP = 16000, 256
N_TRACKS, TRACK_S = 8, 12
GRID = (-30, -20, -2, 0, 2, 12, 14, 20, 22)
MIN_MATCH, MAX_RESULTS = 10, 50  # the engine's FPSPEC defaults
MAX_OUT = 10
UNSEEN_TRACK = 20


@dataclass(frozen=True)
class Clip:
    name: str
    q: np.ndarray  # int16, [n] mono or [n, 2] stereo
    sr: int
    track: int | None  # the catalog track it was taken from (None: unseen or too short)
    speed: int  # its true speed, per mille

    @property
    def channels(self) -> int:
        return 1 if self.q.ndim == 1 else 2

    @property
    def positive(self) -> bool:
        return self.track is not None

    @property
    def x(self) -> np.ndarray:
        return widen(self.q)


def capture(track: int, start_s: float, dur_s: float, sr: int, pm: int, stereo: bool, seed: int) -> np.ndarray:
    """dur_s seconds, heard at `sr`, of `track` from start_s on, played at speed pm."""
    n_src = int(round(dur_s * sr * (1000 + pm) / 1000))
    x = widen(synth_q(track, int(start_s * sr), n_src, sr))
    y = O.resample(x, 1000 + pm, 1000) if pm else x
    rng = np.random.default_rng(seed)
    ch = [y + rng.normal(0.0, 0.01, len(y)).astype(np.float32) for _ in range(2 if stereo else 1)]
    q = [np.clip(np.rint(c.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16) for c in ch]
    return np.stack(q, axis=1) if stereo else q[0]


@functools.lru_cache(maxsize=None)
def records() -> tuple:
    """The oracle's records of the catalog's tracks."""
    return tuple(O.fingerprint(widen(synth_q(t, 0, TRACK_S * SR_E, SR_E)), HOP) for t in range(N_TRACKS))


@functools.lru_cache(maxsize=None)
def postings() -> np.ndarray:
    """uint32 [n, 3] (hash, track, t) of the whole catalog, in track order."""
    rows = []
    for t, r in enumerate(records()):
        rows.append(np.stack([(r & np.uint64(0xFFFFFFFF)).astype(np.uint32), np.full(len(r), t, np.uint32),
                              (r >> np.uint64(32)).astype(np.uint32)], axis=1))
    return np.concatenate(rows)


@functools.lru_cache(maxsize=None)
def clips_48k() -> tuple:
    return (Clip("48k +20", capture(1, 2.0, 5.0, 48000, 20, True, 1), 48000, 1, 20),
            Clip("48k -30", capture(2, 3.0, 5.0, 48000, -30, True, 2), 48000, 2, -30),
            Clip("48k +13", capture(3, 1.0, 5.0, 48000, 13, True, 3), 48000, 3, 13),
            Clip("48k nominal", capture(0, 4.0, 4.0, 48000, 0, True, 4), 48000, 0, 0),
            Clip("48k short", capture(5, 1.0, 0.1, 48000, 0, True, 5), 48000, None, 0))


@functools.lru_cache(maxsize=None)
def clips_16k() -> tuple:
    return (Clip("16k +20", capture(4, 3.0, 4.5, SR_E, 20, False, 11), SR_E, 4, 20),
            Clip("16k -30", capture(5, 1.5, 5.0, SR_E, -30, False, 12), SR_E, 5, -30),
            Clip("16k +13", capture(6, 2.5, 5.0, SR_E, 13, False, 13), SR_E, 6, 13),
            Clip("16k nominal", capture(7, 5.0, 5.0, SR_E, 0, False, 14), SR_E, 7, 0),
            Clip("16k unseen", capture(UNSEEN_TRACK, 2.0, 5.0, SR_E, 0, False, 15), SR_E, None, 0),
            Clip("16k short", capture(2, 0.0, 0.1, SR_E, 0, False, 16), SR_E, None, 0))


def all_clips() -> tuple:
    return clips_48k() + clips_16k()


def name_of(track: int) -> str:
    return str(uuid.UUID(int=int(track) + 1))


def track_of(match) -> int:
    return match.track.int - 1


def oracle_lane(x16: np.ndarray, max_out: int = MAX_OUT) -> list:
    """aidfp.exact's lane over the oracle's fingerprint and matcher for one 16 kHz float clip: ExactMatch rows."""
    sec = HOP / SR_E

    async def oracle_query(piece: bytes):
        rows = O.query(postings(), O.fingerprint(np.frombuffer(piece, dtype="<f4").astype(np.float32), HOP),
                       min_match=MIN_MATCH, max_rows=MAX_RESULTS)
        return [OlafMatch(int(c), tq0 * sec, tq1 * sec, name_of(tr), int(tr), (tq0 + d) * sec, (tq1 + d) * sec)
                for c, tr, d, tq0, tq1 in rows.tolist()]

    return asyncio.run(ex.run_exact_lane(np.ascontiguousarray(x16, "<f4").tobytes(), max_out, query=oracle_query,
                                         sample_rate=SR_E))


def variant(clip: Clip, pm: int) -> np.ndarray:
    """The speed-pm variant of a clip (FPSPEC 8.2), by the oracle."""
    return O.resample(clip.x, clip.sr * 1000, SR_E * (1000 + pm))


@functools.lru_cache(maxsize=None)
def oracle_route(name: str, grid: tuple = GRID, max_out: int = MAX_OUT):
    """(rows, speed) of the clip called `name`: the all-oracle speed lane."""
    clip = next(c for c in all_clips() if c.name == name)
    per_variant = [oracle_lane(variant(clip, pm), max_out) for pm in grid]
    rows, pm = ex.select_speed(per_variant, grid, max_out)
    return tuple(rows), pm


def same_rows(got, want) -> bool:
    """Engine rows against ExactMatch rows: track, aligned_hashes, binary64 offset_seconds, confidence, order."""
    return len(got) == len(want) and all(
        int(g["track"]) == track_of(w) and int(g["aligned_hashes"]) == w.aligned_hashes
        and float(g["offset_seconds"]) == w.offset_seconds and float(g["confidence"]) == w.confidence
        for g, w in zip(got, want))
