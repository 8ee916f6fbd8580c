#!/usr/bin/env python3
"""BASELINE config 5: 48 kHz stereo streaming, 50 %-overlap 5 s windows, continuous
identification on 1 GPU.

A 10-minute synthetic stream is the concatenation of 30 s segments of catalog
tracks (left/right = the same track with independent noise at SNR 30 dB). It is
pushed in real-time-sized chunks (default 2.5 s = one window hop) through
aidfp.stream.StreamIdentifier: GPU downmix -> window -> K1-K3 -> K5 against a
48 kHz index. Reports sustained audio-s/s (stream time / processing time),
per-push latency percentiles, and top-1 accuracy over windows that lie inside a
single segment.

--bank S measures the serving shape instead: S live streams in lockstep through aidfp.stream.StreamBank (one K6
launch and one windowed query per push), 2.5 s device-resident chunks against a 16 kHz index. --pcm s16 pushes
int16 chunks (StreamBank(pcm_format="s16")); --pcm both runs f32 and s16 banks in alternating rounds of one run
(a same-box A/B) and prints one line per format: sustained audio-s/s, the push's K6 time from HIP events and its
HBM fraction on that format's own algorithmic bytes. --host-chunks pushes host arrays (the pinned staging copy is
then part of the push).
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent / "audio-ident_amd"))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1000)
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--chunk-s", type=float, default=2.5)
    ap.add_argument("--index-sr", type=int, default=48000,
                    help="index rate; != 48000 resamples the stream on the GPU (16000 = the reference's Olaf rate)")
    ap.add_argument("--source-sr", type=int, default=44100,
                    help="rate the catalog tracks are synthesised at before K6 brings them to --index-sr, as ingest "
                         "decodes each file with ffmpeg -ar (decode.py:41-60); 0 = synthesise at the index rate")
    ap.add_argument("--bank", type=int, default=0, help="S > 0: S lockstep streams through StreamBank (see above)")
    ap.add_argument("--pcm", choices=("f32", "s16", "both"), default="f32", help="--bank: chunk sample format")
    ap.add_argument("--rounds", type=int, default=5, help="--bank: rounds per format (the first is a warm-up)")
    ap.add_argument("--host-chunks", action="store_true", help="--bank: push host arrays instead of device tensors")
    args = ap.parse_args()
    if args.bank > 0:
        return bank_main(args)
    if args.pcm != "f32":
        ap.error("--pcm applies to --bank (the single-stream StreamIdentifier takes float chunks)")
    SR = 48000
    ISR = args.index_sr
    import torch

    from aidfp import synth
    from aidfp.catalog import ingest_synthetic
    from aidfp.engine import Engine
    from aidfp.stream import StreamIdentifier

    torch.cuda.set_device(0)
    eng = Engine(ISR, device=0)
    ingest_synthetic(eng, np.arange(args.tracks, dtype=np.uint32), 30.0, source_sr=args.source_sr or None)
    rng = np.random.default_rng(42)
    seg = 30 * SR
    n_seg = int(args.minutes * 60 / 30)
    seg_tracks = rng.integers(0, args.tracks, n_seg)
    left = np.concatenate([synth.synth(int(t), 0, seg, SR, snr_db=30.0, salt=11) for t in seg_tracks])
    right = np.concatenate([synth.synth(int(t), 0, seg, SR, snr_db=30.0, salt=12) for t in seg_tracks])
    stereo = np.stack([left, right], axis=1)

    sid = StreamIdentifier(eng, stream_sr=SR)
    chunk = int(args.chunk_s * SR)
    lat = []
    results = []
    sid.push(stereo[:chunk])  # warm-up (first allocations)
    sid = StreamIdentifier(eng, stream_sr=SR)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for a in range(0, len(stereo), chunk):
        t = time.perf_counter()
        results += sid.push(stereo[a:a + chunk])
        torch.cuda.synchronize()
        lat.append(time.perf_counter() - t)
    total = time.perf_counter() - t0
    ok = n = 0
    for r in results:
        s0 = int(round(r.start_s * SR))
        si, sj = s0 // seg, (s0 + int(round(sid.win * SR / ISR)) - 1) // seg
        if si != sj:
            continue
        n += 1
        ok += r.best_track == int(seg_tracks[si])
    stream_s = len(stereo) / SR
    print(json.dumps({
        "metric": "48 kHz stereo stream, 5 s / 2.5 s windows: sustained audio-s/s, 1 GPU",
        "index_sr": ISR, "index_source_sr": args.source_sr or ISR, "front_end": "downmix" if ISR == SR else f"downmix + resample 48000 -> {ISR} (K6)",
        "value": round(stream_s / total, 1), "unit": "audio-s/s", "n_gpus": 1,
        "stream_s": stream_s, "windows": len(results), "chunk_s": args.chunk_s,
        "push_latency_ms": {p: round(1e3 * float(np.percentile(lat, q)), 3) for p, q in (("p50", 50), ("p95", 95), ("p99", 99))},
        "top1_windows_inside_segment": round(ok / max(1, n), 4), "index_tracks": args.tracks, "data": "synthetic",
    }), flush=True)
    eng.close()
    return 0


def bank_main(args) -> int:
    import torch

    from aidfp import synth
    from aidfp.catalog import ingest_synthetic
    from aidfp.engine import Engine
    from aidfp.stream import StreamBank

    QSR, SSR, HBM_PEAK_GBS = 48000, 16000, 8000.0
    S = args.bank
    torch.cuda.set_device(0)
    eng = Engine(SSR, device=0)
    ingest_synthetic(eng, np.arange(args.tracks, dtype=np.uint32), 30.0, source_sr=args.source_sr or None)
    eng.index_finalize()
    chunk = int(args.chunk_s * QSR)
    n_push = 8
    T = n_push * chunk
    tracks = np.random.default_rng(42).integers(0, args.tracks, S).astype(np.uint32)
    stereo = torch.empty(S, T, 2, dtype=torch.float32, device="cuda")
    tmp = torch.empty(S * T, dtype=torch.float32, device="cuda")
    for ch in range(2):
        eng.synth(tmp.data_ptr(), tracks, np.zeros(S, np.int64), T, noise_a=synth.noise_halfwidth(30.0), salt=11 + ch,
                  sample_rate=QSR)
        stereo[:, :, ch] = tmp.view(S, T)
    del tmp
    data = {"f32": stereo, "s16": (stereo * 32768.0).to(torch.int16)}  # the generator's samples are q / 32768
    fmts = ("f32", "s16") if args.pcm == "both" else (args.pcm,)
    if args.host_chunks:
        data = {f: data[f].cpu().numpy() for f in fmts}
    up, down, hl, J = eng.resample_plan(QSR, SSR)
    res = {f: [] for f in fmts}
    for rnd in range(args.rounds):
        for f in fmts:
            bank = StreamBank(eng, S, stream_sr=QSR, **({} if f == "f32" else {"pcm_format": f}))
            torch.cuda.synchronize()
            eng.profile_enable(True)
            eng.profile_select([6])  # AID_K_RESAMPLE
            eng.profile_read(reset=True)
            hits = windows = 0
            t0 = time.perf_counter()
            for a in range(0, T, chunk):
                for i, ws in enumerate(bank.push(data[f][:, a:a + chunk])):
                    windows += len(ws)
                    hits += sum(w.best_track == int(tracks[i]) for w in ws)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            ms, cnt = eng.profile_read(reset=True)["resample"]
            eng.profile_select(None)
            eng.profile_enable(False)
            if rnd:
                res[f].append((wall, ms / cnt, hits / max(1, windows)))
    for f in fmts:
        wall = float(np.median([r[0] for r in res[f]]))
        k_ms = float(np.median([r[1] for r in res[f]]))
        alg = S * ((8 if f == "f32" else 4) * chunk + 4 * (chunk * up // down))
        print(json.dumps({
            "metric": f"{S} x 48 kHz stereo streams in lockstep (StreamBank), 5 s / 2.5 s windows: audio-s/s, 1 GPU",
            "value": round(S * T / QSR / wall, 1), "unit": "audio-s/s", "n_gpus": 1, "pcm": f, "streams": S,
            "chunk_s": args.chunk_s, "pushes": n_push, "chunks": "host" if args.host_chunks else "device",
            "push_ms": round(wall / n_push * 1e3, 4), "k6_ms_per_push": round(k_ms, 4),
            "k6_roofline": {"bound": "hbm", "achieved": round(alg / (k_ms * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS,
                            "unit": "GB/s", "frac": round(alg / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                            "algorithmic_bytes_per_push": alg},
            "rounds_k6_ms": [round(r[1], 4) for r in res[f]], "rounds_push_ms": [round(r[0] / n_push * 1e3, 3) for r in res[f]],
            "top1_windows": round(float(np.median([r[2] for r in res[f]])), 4), "index_tracks": args.tracks,
            "index_sr": SSR, "data": "synthetic",
        }), flush=True)
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
