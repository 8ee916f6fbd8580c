#!/usr/bin/env python3
"""bench_mel.py -- K10, the CLAP log-mel front end (spec/FPSPEC.md 10) on one MI355X.

Workload: one device-resident 48 kHz float32 track whose chunk plan (10 s chunks, 5 s hop) has 256 or 2048 chunks;
one step = one aid_logmel call that writes the [chunks][1001][64] images into a device buffer. Reported: wall ms per
call (host clock around call + synchronise), device ms per call (events on the call's stream around it), chunks/s.

Against it, on the same card in alternating runs, the torch route a user would otherwise write: the chunks as rows of
a strided view, torch.stft (1024 / 480, periodic Hann, centre reflect), |X|^2, matmul with the same filter bank,
10 log10 of the clamp, in batches of 256 chunks. Medians over the alternations with the spread (min..max).
Where transformers is importable the host ClapFeatureExtractor is timed on a few chunks as well (one thread).
One JSON line per size and one for the host extractor; --out also writes the lines to a text file.
"""

from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT / "audio-ident_amd"))

L_WIN, HOP_C, T, BANDS = 480000, 240000, 1001, 64


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, nargs="+", default=[256, 2048])
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50, help="calls per timed run")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-chunks", type=int, default=4, help="chunks the host extractor is timed on (0: skip)")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()

    import torch

    from aidfp import _lib as L
    from aidfp import clap
    from aidfp.engine import Engine

    dev = torch.device("cuda:0")
    eng = Engine(16000, device=0)
    lm = clap.LogMel(eng)
    W = torch.from_numpy(lm.filters()).to(dev)  # [513][64]
    window = torch.hann_window(1024, periodic=True, device=dev)
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    for C in args.chunks:
        n = HOP_C * C + 47999  # C chunks: all full but the last (287999 samples)
        g = torch.Generator(device=dev).manual_seed(C)
        track = torch.zeros(HOP_C * (C - 1) + L_WIN, device=dev)  # zero-extended so every chunk is a full row of a view
        track[:n] = 0.1 * torch.randn(n, generator=g, device=dev)
        meta = clap.plan([n])
        assert len(meta) == C
        out = torch.empty((C, T, BANDS), device=dev)
        off, ln = np.zeros(1, np.int64), np.array([n], np.int64)
        nch = ctypes.c_int64()
        stream = torch.cuda.current_stream(dev)

        def k10_call():
            L.check(eng._lib.aid_logmel(eng._h, ctypes.c_void_p(track.data_ptr()), ctypes.c_void_p(off.ctypes.data),
                                        ctypes.c_void_p(ln.ctypes.data), 1, L.AID_PCM_DEVICE, L.AID_MEL_ZERO, 0,
                                        ctypes.c_void_p(out.data_ptr()), C, L.AID_PCM_DEVICE, None, ctypes.byref(nch),
                                        ctypes.c_void_p(stream.cuda_stream)))

        rows = track.as_strided((C, L_WIN), (HOP_C, 1))
        ref = torch.empty((C, T, BANDS), device=dev)

        def torch_call():
            for a in range(0, C, 256):
                X = torch.stft(rows[a:a + 256], 1024, hop_length=480, window=window, center=True, pad_mode="reflect",
                               return_complex=True)  # [b][513][1001]
                P = X.real * X.real + X.imag * X.imag
                ref[a:a + 256] = 10.0 * torch.log10(torch.clamp(P.transpose(1, 2) @ W, min=1e-10))

        def timed(fn, steps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            for _ in range(steps):
                fn()
            e1.record(stream)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps * 1e3, e0.elapsed_time(e1) / steps

        for _ in range(args.warmup):
            k10_call()
            torch_call()
        torch.cuda.synchronize()
        diff = float((out - ref).abs().max())
        kw, kd, tw, td = [], [], [], []
        for _ in range(args.alternations):
            w, d = timed(k10_call, args.steps)
            kw.append(w)
            kd.append(d)
            w, d = timed(torch_call, args.steps)
            tw.append(w)
            td.append(d)
        med = statistics.median
        emit({"bench": "logmel", "chunks": C, "audio_s": round(n / 48000, 1),
              "k10_wall_ms": round(med(kw), 3), "k10_wall_ms_min_max": [round(min(kw), 3), round(max(kw), 3)],
              "k10_device_ms": round(med(kd), 3), "k10_chunks_per_s": round(C / med(kw) * 1e3, 1),
              "torch_wall_ms": round(med(tw), 3), "torch_wall_ms_min_max": [round(min(tw), 3), round(max(tw), 3)],
              "torch_device_ms": round(med(td), 3), "torch_chunks_per_s": round(C / med(tw) * 1e3, 1),
              "k10_over_torch_speed": round(med(tw) / med(kw), 3), "max_abs_db_k10_vs_torch": diff,
              "alternations": args.alternations, "steps": args.steps})
        del track, out, ref, rows
        torch.cuda.empty_cache()

    if args.host_chunks > 0:
        try:
            import warnings

            warnings.simplefilter("ignore")
            from transformers import ClapFeatureExtractor

            torch.set_num_threads(1)
            fe = ClapFeatureExtractor(frequency_min=50, frequency_max=14000, truncation="rand_trunc", padding="repeatpad")
            x = (0.1 * np.random.default_rng(1).standard_normal(L_WIN)).astype(np.float32)
            fe(x, sampling_rate=48000, return_tensors="np")
            t0 = time.perf_counter()
            for _ in range(args.host_chunks):
                fe(x, sampling_rate=48000, return_tensors="np")
            ms = (time.perf_counter() - t0) / args.host_chunks * 1e3
            emit({"bench": "logmel_host_extractor", "ms_per_chunk": round(ms, 2), "chunks_per_s": round(1e3 / ms, 2),
                  "chunks_timed": args.host_chunks})
        except ImportError:
            emit({"bench": "logmel_host_extractor", "skipped": "transformers not importable"})
    eng.close()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
