"""StreamBank, bench_stream.py --bank's set-up (S lockstep 48 kHz stereo streams, 16 kHz index, 8 pushes of 2.5 s),
timed two ways: push() (synchronous) and push_submit / collect one push behind (the ticket path). Rounds alternate
the two; the first round is a warm-up. One JSON line."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "audio-ident_amd"))


def main():
    import torch

    from aidfp import synth
    from aidfp.catalog import ingest_synthetic
    from aidfp.engine import Engine
    from aidfp.stream import StreamBank

    S, tracks_n, rounds = 256, 1000, 7
    QSR, SSR = 48000, 16000
    torch.cuda.set_device(0)
    eng = Engine(SSR, device=0)
    ingest_synthetic(eng, np.arange(tracks_n, dtype=np.uint32), 30.0, source_sr=44100)
    eng.index_finalize()
    chunk = int(2.5 * QSR)
    n_push = 8
    T = n_push * chunk
    tracks = np.random.default_rng(42).integers(0, tracks_n, S).astype(np.uint32)
    stereo = torch.empty(S, T, 2, dtype=torch.float32, device="cuda")
    tmp = torch.empty(S * T, dtype=torch.float32, device="cuda")
    for ch in range(2):
        eng.synth(tmp.data_ptr(), tracks, np.zeros(S, np.int64), T, noise_a=synth.noise_halfwidth(30.0), salt=11 + ch,
                  sample_rate=QSR)
        stereo[:, :, ch] = tmp.view(S, T)
    del tmp
    res = {"sync": [], "pipelined": []}
    windows = {}
    for rnd in range(rounds):
        for mode in ("sync", "pipelined"):
            bank = StreamBank(eng, S, stream_sr=QSR)
            torch.cuda.synchronize()
            n = 0
            pending = None
            t0 = time.perf_counter()
            for a in range(0, T, chunk):
                if mode == "sync":
                    n += sum(len(ws) for ws in bank.push(stereo[:, a:a + chunk]))
                else:
                    p = bank.push_submit(stereo[:, a:a + chunk])
                    if pending is not None:
                        n += sum(len(ws) for ws in pending.collect())
                    pending = p
            if pending is not None:
                n += sum(len(ws) for ws in pending.collect())
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            windows[mode] = n
            if rnd:
                res[mode].append(wall)
    out = {"streams": S, "pushes": n_push, "windows": windows, "match_stats": eng.match_stats()}
    for mode, walls in res.items():
        out[mode] = {"audio_s_per_s": round(S * T / QSR / float(np.median(walls)), 1),
                     "push_ms_median": round(float(np.median(walls)) / n_push * 1e3, 4),
                     "rounds_push_ms": [round(w / n_push * 1e3, 4) for w in walls]}
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
