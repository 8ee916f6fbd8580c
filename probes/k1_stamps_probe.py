#!/usr/bin/env python3
"""What the two ends of K1 cost, by per-wave stamps (diagnostic build, AID_K1_STAMPS).

    python probes/k1_stamps_probe.py

Loads the diagnostic copy of the library (audio-ident_amd/build/k1stamps/libaidfp.so, built by
build_ext.build(variant="k1stamps", defines=("AID_K1_STAMPS",)); built here if it is missing), runs the bench batch
(256 x 10 s), reads the stamps of the last launch and prints one JSON line:
  entry_to_first_frame: cycles from a wave's entry until the ring of its first segment has landed (table staging,
    the barrier, the clip search, the descriptor loads, 16 ring loads), median and 90th percentile, and in us at the
    wave's own clock (its life in cycles over its life on the 100 MHz clock);
  exit_spread_us: last exit minus median exit on the 100 MHz clock (the whole device's), and the launch's length on it,
    with the percentiles of the waves' entries, exits and lives that say whether late waves started late or ran long;
  crossing: waves whose range crossed a clip edge (two segments) against the others, median exit after the launch's
    first entry."""
import ctypes
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
VARIANT = ROOT / "audio-ident_amd" / "build" / "k1stamps" / "libaidfp.so"
os.environ["AIDFP_LIB"] = str(VARIANT)
sys.path.insert(0, str(ROOT / "audio-ident_amd"))
WORDS = 6


def main():
    if not VARIANT.exists():
        import build_ext

        build_ext.build(variant="k1stamps", defines=("AID_K1_STAMPS",))
    import torch

    from aidfp import _lib
    from aidfp.engine import Engine

    fn = _lib.load().aid_diag_k1_stamps
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int]
    torch.cuda.set_device(0)
    eng = Engine(44100, device=0)
    n, clips = 441000, 256
    pcm = torch.empty(clips * n, dtype=torch.float32, device="cuda")
    offs = np.arange(clips + 1, dtype=np.int64) * n
    eng.synth(pcm.data_ptr(), np.arange(clips, dtype=np.uint32), np.zeros(clips, np.int64), n)
    for _ in range(60):  # warm + clocks
        eng.extract_device(pcm.data_ptr(), offs)
    torch.cuda.synchronize()
    waves = torch.cuda.get_device_properties(0).multi_processor_count * 16
    buf = np.zeros((waves, WORDS), dtype=np.uint64)
    if fn(buf.ctypes.data, waves) != 0:
        raise SystemExit("aid_diag_k1_stamps failed")
    eng.close()
    s = buf.astype(np.int64)
    live = s[:, 5] > 0
    s = s[live]
    head = (s[:, 1] - s[:, 0]).astype(np.float64)
    life_cyc, life_ticks = (s[:, 2] - s[:, 0]).astype(np.float64), (s[:, 4] - s[:, 3]).astype(np.float64)
    mhz = float(np.median(life_cyc / np.maximum(life_ticks, 1.0)) * 100.0)  # cycles per 10 ns tick
    t0 = s[:, 3].min()
    exit_us = (s[:, 4] - t0) / 100.0
    cross = s[:, 5] > 1
    out = {"library": str(VARIANT.relative_to(ROOT)), "waves": int(live.sum()), "in_kernel_clock_mhz": round(mhz, 1),
           "entry_to_first_frame": {"median_cycles": float(np.median(head)), "p90_cycles": float(np.percentile(head, 90)),
                                    "median_us": round(float(np.median(head)) / mhz, 3)},
           "wave_life_median_us": round(float(np.median(life_ticks)) / 100.0, 2),
           "launch_us": round(float(exit_us.max()), 2),
           "exit_spread_us": round(float(exit_us.max() - np.median(exit_us)), 2),
           "exit_p90_p99_us": [round(float(np.percentile(exit_us, q)), 2) for q in (90, 99)],
           "entry_median_p90_p99_last_us": [round(float(np.percentile((s[:, 3] - t0) / 100.0, q)), 2) for q in (50, 90, 99, 100)],
           "wave_life_p90_p99_max_us": [round(float(np.percentile(life_ticks, q)) / 100.0, 2) for q in (90, 99, 100)],
           "crossing": {"waves": int(cross.sum()),
                        "median_exit_us": round(float(np.median(exit_us[cross])), 2) if cross.any() else None,
                        "others_median_exit_us": round(float(np.median(exit_us[~cross])), 2),
                        "median_life_us": round(float(np.median(life_ticks[cross])) / 100.0, 2) if cross.any() else None,
                        "others_median_life_us": round(float(np.median(life_ticks[~cross])) / 100.0, 2)}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
