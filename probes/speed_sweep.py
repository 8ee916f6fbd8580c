"""How close must an assumed speed be to the true one? CPU only, oracle only (no GPU, no engine).

The measurement behind the 2 per mille step of aidfp.exact.speed_grid (spec/FPSPEC.md 7.1, 8.2). Set-up: FPSPEC v1
through oracle.resample -> oracle.fingerprint -> oracle.query with min_match 1. The index holds 24 synthetic tracks of
20 s, synthesised at 48 kHz and ingested 48 kHz -> 16 kHz. A query is a 5 s clip of one of them at 48 kHz, played at a
true speed of 0, +20 or -30 per mille (resampled for the rate pair (1000 + true, 1000)), with white noise of sigma
0.01, then resampled to 16 kHz under an ASSUMED speed (the rate pair (48000 * 1000, 16000 * (1000 + assumed))) and
matched whole. Reported per residual |true - assumed|: the true track's score (distinct anchor frames) and the best
wrong track's, over all queries and both signs of the residual.

The first run of this measurement rested on eight queries per point; this one takes --queries per true speed
(default 100, so 300 per residual).

    python probes/speed_sweep.py > profiles/speed_residual_cpu.txt
"""

import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "audio-ident_amd", ROOT / "oracle"):
    sys.path.insert(0, str(p))

import oracle as O  # noqa: E402
from aidfp import synth  # noqa: E402

SR_E, SR_Q, HOP = 16000, 48000, 256
N_TRACKS, TRACK_S, CLIP_S = 24, 20, 5
TRUE_SPEEDS = (0, 20, -30)
RESIDUALS = (0, 1, 2, 3, 4, 5, 8, 12)


def track_48k(t: int, start: int, n: int) -> np.ndarray:
    return (synth.synth_int16(t, start, n, SR_Q, 0, 0).astype(np.float32) / np.float32(32768.0)).astype(np.float32)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=100, help="queries per true speed")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    t0 = time.time()
    post = []
    for t in range(N_TRACKS):
        r = O.fingerprint(O.resample(track_48k(t, 0, TRACK_S * SR_Q), SR_Q, SR_E), HOP)
        post.append(np.stack([(r & np.uint64(0xFFFFFFFF)).astype(np.uint32), np.full(len(r), t, np.uint32),
                              (r >> np.uint64(32)).astype(np.uint32)], axis=1))
    post = np.concatenate(post)
    rng = np.random.default_rng(args.seed)
    true_scores = {(s, r): [] for s in TRUE_SPEEDS for r in RESIDUALS}
    wrong_scores = {(s, r): [] for s in TRUE_SPEEDS for r in RESIDUALS}
    for s in TRUE_SPEEDS:
        for q in range(args.queries):
            t = int(rng.integers(0, N_TRACKS))
            n_src = CLIP_S * SR_Q * (1000 + s) // 1000  # the passage a 5 s capture plays at speed s
            start = int(rng.integers(0, TRACK_S * SR_Q - n_src))
            x = track_48k(t, start, n_src)
            y = O.resample(x, 1000 + s, 1000) if s else x
            y = (y + rng.normal(0.0, 0.01, len(y)).astype(np.float32)).astype(np.float32)
            for r in RESIDUALS:
                assumed = s + (r if q % 2 == 0 else -r)
                z = O.resample(y, SR_Q * 1000, SR_E * (1000 + assumed))
                rows = O.query(post, O.fingerprint(z, HOP), min_match=1, max_rows=N_TRACKS)
                by_track = {int(row[1]): int(row[0]) for row in rows}
                true_scores[(s, r)].append(by_track.pop(t, 0))
                wrong_scores[(s, r)].append(max(by_track.values(), default=0))
    print(f"# speed residual sweep, CPU oracle only: {N_TRACKS} tracks x {TRACK_S} s (48 kHz -> 16 kHz), "
          f"{args.queries} queries of {CLIP_S} s per true speed, noise sigma 0.01, min_match 1, seed {args.seed}")
    print("# score = distinct anchor frames of the best offset (FPSPEC 7); true = the query's own track, "
          "wrong = the best other track")
    print("# true_pm residual_pm  n  true_min true_p10 true_median true_max  wrong_max  found_at_min_match_10")
    for s in TRUE_SPEEDS:
        for r in RESIDUALS:
            a = np.array(true_scores[(s, r)])
            w = np.array(wrong_scores[(s, r)])
            print(f"{s:+4d} {r:3d} {len(a):4d}  {a.min():4d} {int(np.percentile(a, 10)):4d} {int(np.median(a)):4d} "
                  f"{a.max():4d}  {w.max():4d}  {float((a >= 10).mean()):.2f}")
    print("# all true speeds together")
    for r in RESIDUALS:
        a = np.concatenate([true_scores[(s, r)] for s in TRUE_SPEEDS])
        w = np.concatenate([wrong_scores[(s, r)] for s in TRUE_SPEEDS])
        print(f" all {r:3d} {len(a):4d}  {a.min():4d} {int(np.percentile(a, 10)):4d} {int(np.median(a)):4d} {a.max():4d}  "
              f"{w.max():4d}  {float((a >= 10).mean()):.2f}")
    print(f"# {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
