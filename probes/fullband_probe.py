"""K2 strip sizing on band-limited vs full-band audio: the bench batch (partials <= 8 kHz) and the bench's full-band
batch (partials <= 20 kHz), extracted with the engine's adaptive strip sizing and with fixed strips-per-slot
multipliers (aid_engine_force K2_STRIPS_X100), at the adaptive K2 width or at fixed ones (K2_WIDTH). Prints
per-launch K1/K2/K3 times, the K2 width and the strip count per setting. Diagnostic only.

usage: python probes/fullband_probe.py [--width W[,W..]] [--mixed PCT[,PCT..]] [x100 ...]
       (0 = adaptive, for both; default widths: 0; default multipliers: 0 100 125 150 175 200;
        --mixed adds batches whose first PCT % of clips are full-band, the rest band-limited)
"""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "audio-ident_amd"))


def run(eng, pcm, offs, steps=40):
    import torch

    for _ in range(60):  # warm up + let the adaptive sizing see a few counts
        eng.extract_device(pcm.data_ptr(), offs)
    torch.cuda.synchronize()
    eng.profile_select(None)
    eng.profile_enable(True)
    eng.profile_read(reset=True)
    t = time.perf_counter()
    for _ in range(steps):
        eng.extract_device(pcm.data_ptr(), offs)
    eng.sync()
    dt = (time.perf_counter() - t) / steps
    prof = eng.profile_read(reset=True)
    eng.profile_enable(False)
    st = eng.match_stats()
    return {"ms_per_step": round(dt * 1e3, 4), **{k: round(ms / n, 4) for k, (ms, n) in prof.items() if n},
            "k2_width": st["k2_width"], "k2_strips": st["k2_strips"]}


def main():
    import torch

    from aidfp.engine import Engine

    args, widths = sys.argv[1:], [0]
    if args and args[0] == "--width":
        widths, args = [int(w) for w in args[1].split(",")], args[2:]
    mixed = []
    if args and args[0] == "--mixed":
        mixed, args = [int(m) for m in args[1].split(",")], args[2:]
    settings = [int(a) for a in args] or [0, 100, 125, 150, 175, 200]
    eng = Engine(44100, device=0)
    n, clips = 441000, 256
    pcm = torch.empty(clips * n, dtype=torch.float32, device="cuda")
    offs = np.arange(clips + 1, dtype=np.int64) * n
    tracks = np.arange(clips, dtype=np.uint32)
    out = {}
    batches = [("band_limited", 0), ("full_band", clips)] + [(f"mixed_{m}", clips * m // 100) for m in mixed]
    for name, nfull in batches:  # clips [0, nfull) with partials up to 20 kHz, the others up to 8 kHz
        if nfull:
            eng.synth(pcm.data_ptr(), tracks[:nfull] + 500000, np.zeros(nfull, np.int64), n, fmax_hz=20000)
        if nfull < clips:
            eng.synth(pcm.data_ptr() + 4 * n * nfull, tracks[nfull:], np.zeros(clips - nfull, np.int64), n, fmax_hz=8000)
        for w in widths:
            eng.force("k2_width", w)
            for x in settings:
                eng.force("k2_strips_x100", x)
                out[f"{name}/{x or 'adaptive'}" + (f"/w{w}" if w else "")] = run(eng, pcm, offs)
    eng.force("k2_strips_x100", 0)
    eng.force("k2_width", 0)
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
