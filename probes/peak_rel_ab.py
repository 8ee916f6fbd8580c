"""What the per-clip relative peak threshold (spec/FPSPEC.md 5.1) costs on the headline workload, as alternating
rounds of one run on one box.

The bench batch (256 x 10 s at 44.1 kHz, device-resident) under three engine configurations:
  * default:       peak_rel = 0, threshold 4.0 (FPSPEC 5);
  * rel_floor4:    peak_rel = 1e-4 with the floor at 4.0: K1's maximum and K2's per-clip threshold alone, the hot
                   blocks are those of the default;
  * rel_floor2m20: peak_rel = 1e-4 with the floor at 2^-20, what quiet queries need: K1 stores and K2 reads every
                   block that holds a value above the floor.
Per configuration: K1 and K2 per launch from HIP events (aid_profile_*), the whole extraction (K1-K3) per step from
the host clock without the profiler, and the mean number of records per clip.

usage: python probes/peak_rel_ab.py [--steps N] [--rounds R] [--out FILE]   (FILE is appended to)
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "audio-ident_amd"))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from aidfp.engine import Engine

    SR, CLIPS, SEC = 44100, 256, 10
    n = SR * SEC
    rel = float(np.float32(1e-4))
    engines = {"default": Engine(SR), "rel_floor4": Engine(SR, peak_rel=rel),
               "rel_floor2m20": Engine(SR, peak_threshold=2.0 ** -20, peak_rel=rel)}
    pcm = torch.empty(CLIPS * n, dtype=torch.float32, device="cuda")
    engines["default"].synth(pcm.data_ptr(), np.arange(CLIPS, dtype=np.uint32) + 1, np.zeros(CLIPS, np.int64), n)
    torch.cuda.synchronize()
    offs = np.arange(CLIPS + 1, dtype=np.int64) * n

    def step_ms(eng) -> float:
        eng.extract_device(pcm.data_ptr(), offs)
        eng.sync()
        t = time.perf_counter()
        for _ in range(args.steps):
            eng.extract_device(pcm.data_ptr(), offs)
        eng.sync()
        return (time.perf_counter() - t) / args.steps * 1e3

    def kernels_ms(eng) -> tuple[float, float]:
        eng.profile_enable(True)
        eng.profile_select([0, 1])  # AID_K_STFT, AID_K_PEAKS
        eng.profile_read(reset=True)
        for _ in range(args.steps):
            eng.extract_device(pcm.data_ptr(), offs)
        eng.sync()
        prof = eng.profile_read(reset=True)
        eng.profile_select(None)
        eng.profile_enable(False)
        return prof["stft_power"][0] / prof["stft_power"][1], prof["peak_pick"][0] / prof["peak_pick"][1]

    rounds = {k: {"k1_ms": [], "k2_ms": [], "extract_ms": []} for k in engines}
    for r in range(args.rounds + 1):  # round 0 warms up (allocations, clocks, K2's adaptive strips)
        for name, eng in engines.items():
            k1, k2 = kernels_ms(eng)
            ex = step_ms(eng)
            if r:
                rounds[name]["k1_ms"].append(k1)
                rounds[name]["k2_ms"].append(k2)
                rounds[name]["extract_ms"].append(ex)
    out = {"probe": "peak_rel_ab", "batch": f"{CLIPS} x {SEC} s at {SR} Hz", "peak_rel": rel, "steps": args.steps,
           "rounds": args.rounds}
    for name, eng in engines.items():
        eng.extract_device(pcm.data_ptr(), offs)
        counts = eng.counts()
        thr = eng.thresholds()
        row = {"records_per_clip": round(float(counts.mean()), 1), "thr_c_min": float(thr.min()),
               "thr_c_max": float(thr.max())}
        for key, vals in rounds[name].items():
            row[key] = round(float(np.median(vals)), 4)
            row[key + "_rounds"] = [round(v, 4) for v in vals]
        out[name] = row
    for name in ("rel_floor4", "rel_floor2m20"):
        for key in ("k1_ms", "k2_ms", "extract_ms"):
            out[name][key + "_over_default"] = round(out[name][key] / out["default"][key], 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    for eng in engines.values():
        eng.close()


if __name__ == "__main__":
    main()
