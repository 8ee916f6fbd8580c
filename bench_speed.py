#!/usr/bin/env python3
"""bench_speed.py -- the speed fan-out (K6s) and the speed-tolerant exact lane (spec/FPSPEC.md 8.2, 7.1) on one MI355X.

Workload: 256 clips of 5 s of 48 kHz stereo int16 PCM resident on the device (captures of catalog tracks at the
nominal speed, noise at 20 dB SNR) against a 16 kHz index of 10,000 synthetic tracks of 30 s, under the default grid of
41 speeds (-40 .. +40 per mille in steps of 2): 10,496 (clip, speed) pairs per call.

Two A/Bs, each alternating on the same card, medians over the alternations with the spread (min..max) of both routes:

  1. resample: one aid_resample_s16_speeds call (ONE launch) against the route the library already offered: one
     aid_resample_s16 per (clip, speed), 10,496 launches. Both end in a device synchronise. The new kernel's own time
     comes from the engine's events (AID_K_RESAMPLE_SPEEDS) in a run of its own; its bytes (every variant's input
     window read once, every output written once) over that time is set against the 8 TB/s HBM peak.
  2. lane: one aid_exact_lane_s16_speeds call against, per speed, that resample loop into a float buffer, one
     aid_exact_lane over the device PCM and aidfp.exact.select_speed on the host. Clips/s and the device-to-host
     bytes of each route.

Before timing, the two routes' outputs are compared on the timed inputs: the variants bit for bit, the lane's rows
and speeds field for field. One JSON line per A/B, then one summary line.
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT / "audio-ident_amd"))

HBM_PEAK = 8.0e12
SR_E, SR_Q = 16000, 48000


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--track-seconds", type=float, default=30.0)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-out", type=int, default=10)
    ap.add_argument("--skip-lane", action="store_true")
    args = ap.parse_args()

    import torch

    from aidfp import exact as ex
    from aidfp import synth
    from aidfp.catalog import ingest_synthetic
    from aidfp.engine import Engine

    grid = ex.speed_grid()
    pm = np.asarray(grid, np.int32)
    C, V = args.clips, len(grid)
    n = int(round(args.seconds * SR_Q))
    eng = Engine(SR_E, device=0)
    ingest_synthetic(eng, np.arange(args.tracks, dtype=np.uint32), args.track_seconds, batch=256, local=True)
    eng.index_finalize()

    # the clips: [C][n][2] int16, the two channels with noise of their own
    rng = np.random.default_rng(7)
    tracks = rng.integers(0, args.tracks, C).astype(np.uint32)
    starts = rng.integers(0, int((args.track_seconds - args.seconds - 1) * SR_Q), C).astype(np.int64)
    tmp = torch.empty(C * n, dtype=torch.float32, device="cuda")
    stereo = torch.empty(C, n, 2, dtype=torch.float32, device="cuda")
    for ch in range(2):
        eng.synth(tmp.data_ptr(), tracks, starts, n, noise_a=synth.noise_halfwidth(20.0), salt=3 + ch, sample_rate=SR_Q)
        stereo[:, :, ch] = tmp.view(C, n)
    q = (stereo * 32768.0).to(torch.int16).contiguous()
    del tmp, stereo
    offsets = (np.arange(C + 1, dtype=np.int64) * n)
    lens = [eng.speed_len(n, SR_Q, int(s)) for s in grid]
    total = C * sum(lens)
    dst = torch.empty(total, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    # ---- 1. resample: one call against one aid_resample per (clip, speed)
    def fanout_new():
        t0 = time.perf_counter()
        off = eng.resample_speeds(q.data_ptr(), offsets, 2, SR_Q, pm, dst.data_ptr(), total, fmt="s16")
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, off

    old = torch.empty(total, dtype=torch.float32, device="cuda")

    def fanout_old(only_speed=None, out=None):
        """The parent's route: aid_resample_s16 per pair, into the packed layout (or one speed's [C][len] block)."""
        t0 = time.perf_counter()
        base, o = q.data_ptr(), 0
        for c in range(C):
            for v in range(V):
                if only_speed is None:
                    eng.resample(base + c * n * 4, n, 2, SR_Q * 1000, SR_E * (1000 + grid[v]), old.data_ptr() + 4 * o,
                                 lens[v], fmt="s16")
                    o += lens[v]
                elif v == only_speed:
                    eng.resample(base + c * n * 4, n, 2, SR_Q * 1000, SR_E * (1000 + grid[v]),
                                 out.data_ptr() + 4 * c * lens[v], lens[v], fmt="s16")
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(max(1, args.warmup)):
        _, off = fanout_new()
        fanout_old()
    same = bool(torch.equal(dst.view(torch.int32), old.view(torch.int32)))
    tn, to = [], []
    for _ in range(args.alternations):
        tn.append(fanout_new()[0])
        to.append(fanout_old())
    eng.profile_enable(True)
    eng.profile_select([12])  # AID_K_RESAMPLE_SPEEDS
    eng.profile_read(reset=True)
    for _ in range(3):
        fanout_new()
    k_ms, k_n = eng.profile_read(reset=True)["resample_speeds"]
    eng.profile_enable(False)
    eng.profile_select(None)
    k_ms /= max(k_n, 1)
    # bytes the algorithm needs: each variant reads its clip once (4 B per stereo s16 frame) and writes its output
    need = C * V * n * 4 + total * 4
    a, b = stats(tn), stats(to)
    line1 = {"ab": "resample", "clips": C, "speeds": V, "pairs": C * V, "variant_samples": total, "bit_equal": same,
             "resample_speeds": a, "resample_per_pair": b, "new_over_old": round(a["median_ms"] / b["median_ms"], 4),
             "old_spread_rel": round((b["max_ms"] - b["min_ms"]) / b["median_ms"], 3),
             "k6s_kernel_ms": round(k_ms, 3), "k6s_bytes": need,
             "k6s_hbm_fraction": round(need / (k_ms * 1e-3) / HBM_PEAK, 4) if k_ms > 0 else None}
    print(json.dumps(line1), flush=True)
    del old
    if args.skip_lane:
        eng.close()
        return 0 if same else 1

    # ---- 2. lane: one call against per-speed resample loop + aid_exact_lane + select_speed on the host
    mo = args.max_out

    def lane_new():
        t0 = time.perf_counter()
        rows, speeds = eng.exact_lane_speeds(None, SR_Q, 2, pm, mo, pcm_ptr=q.data_ptr(), offsets=offsets, fmt="s16")
        return (time.perf_counter() - t0) * 1e3, rows, speeds

    per_speed = torch.empty(C * max(lens), dtype=torch.float32, device="cuda")

    def lane_old():
        t0 = time.perf_counter()
        per_variant = []
        for v in range(V):
            fanout_old(only_speed=v, out=per_speed)
            per_variant.append(eng.exact_lane(None, mo, pcm_ptr=per_speed.data_ptr(),
                                              offsets=np.arange(C + 1, dtype=np.int64) * lens[v]))
        picked = [ex.select_speed([per_variant[v][c] for v in range(V)], grid, mo) for c in range(C)]
        return (time.perf_counter() - t0) * 1e3, [p[0] for p in picked], [p[1] for p in picked]

    for _ in range(max(1, args.warmup)):
        _, rn, sn = lane_new()
        _, ro, so = lane_old()
    agree = sn == so and all(np.array_equal(x, y) for x, y in zip(rn, ro))
    top1 = float(np.mean([len(r) > 0 and int(r[0]["track"]) == int(t) for r, t in zip(rn, tracks)]))
    tn, to = [], []
    for _ in range(args.alternations):
        tn.append(lane_new()[0])
        to.append(lane_old()[0])
    a, b = stats(tn), stats(to)
    row_bytes = 24
    line2 = {"ab": "lane", "clips": C, "speeds": V, "max_out": mo, "rows_and_speeds_equal": bool(agree),
             "top1": round(top1, 4), "speeds_chosen": {str(s): int(sn.count(s)) for s in sorted(set(sn))},
             "lane_speeds": a, "lane_per_speed": b, "new_over_old": round(a["median_ms"] / b["median_ms"], 4),
             "old_spread_rel": round((b["max_ms"] - b["min_ms"]) / b["median_ms"], 3),
             "new_clips_per_s": round(C / (a["median_ms"] * 1e-3), 1), "old_clips_per_s": round(C / (b["median_ms"] * 1e-3), 1),
             "new_d2h_bytes": C * mo * row_bytes + 2 * C * 4, "old_d2h_bytes": V * (C * mo * row_bytes + C * 4)}
    print(json.dumps(line2), flush=True)
    print(json.dumps({
        "metric": f"speed-tolerant exact lane, {C} clips x {args.seconds:g} s of 48 kHz stereo s16, {V} speeds, "
                  f"{args.tracks}-track index, clips per second (median), 1 GPU",
        "value": line2["new_clips_per_s"], "unit": "clips/s", "higher_is_better": True, "n_gpus": 1,
        "data": "synthetic", "resample_ms": line1["resample_speeds"]["median_ms"],
        "resample_per_pair_ms": line1["resample_per_pair"]["median_ms"], "lane_per_speed_clips_per_s": line2["old_clips_per_s"],
    }), flush=True)
    eng.close()
    return 0 if same and agree else 1


if __name__ == "__main__":
    sys.exit(main())
