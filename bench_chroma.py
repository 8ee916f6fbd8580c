#!/usr/bin/env python3
"""bench_chroma.py -- K11, the content fingerprint (spec/FPSPEC.md 11) on one MI355X.

Workload: 256 clips of 30 s of 16 kHz s16 mono on the device (the service's upload format); one step = K6 to
11025 Hz (all clips in one aid_resample_batch_split_s16 launch) + one aid_chroma call that leaves the 256 x 221 words
on the device. Reported: wall ms per step (host clock around the calls and a synchronise), device ms (events on the
stream), clips/s, and the same for K11 alone on the resampled clips.

Against it, on the same card in alternating runs, the torch route a user would otherwise write, on the engine's own
11025 Hz output (so without any resampling): torch.stft (4096 / 1365, symmetric Hamming, no centring), |X|^2 of bins
10..1307, index_add_ into the 12 bands, a 5-tap conv1d, the normaliser, and the 16 classifiers as one conv2d with
their rectangle masks. Its words are compared with K11's by differing bits (torch sums in its own order, so equality
is not expected). Medians over the alternations with the spread (min..max). The numpy oracle (tests/chroma_ref.py) is
timed on one clip on one host thread. One JSON line each; --out also writes the lines to a text file.
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
sys.path.insert(0, str(ROOT / "tests"))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="steps per timed run")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true", help="K11 only (sweeps of diagnostic builds)")
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--tag", type=str, default="")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()

    import torch

    import chroma_ref as R
    from aidfp import _lib as L
    from aidfp.engine import Engine

    dev = torch.device("cuda:0")
    eng = Engine(16000, device=0)
    lib, h = eng._lib, eng._h
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    B, n16 = args.clips, int(round(args.seconds * 16000))
    m = eng.resample_len(n16, 16000, 11025)
    T, W = R.n_frames(m), R.n_words(m)
    rng = np.random.default_rng(1)
    base = [np.clip(np.round(R.song(s, args.seconds, sr=16000) * 30000.0), -32768, 32767).astype(np.int16) for s in range(4)]
    host = np.stack([np.roll(base[c % 4], 997 * c) for c in range(B)])
    host = (host + rng.integers(-40, 41, size=host.shape)).astype(np.int16)
    pcm16 = torch.from_numpy(host).to(dev)
    pcm11 = torch.zeros((B, m), dtype=torch.float32, device=dev)
    words = torch.zeros(B * W, dtype=torch.int32, device=dev)
    off = (np.arange(B + 1, dtype=np.int64) * m)
    woff = np.zeros(B + 1, np.int64)
    got = ctypes.c_int64()
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    torch.cuda.synchronize()

    def k6_call():
        eng.resample_batch_split(0, 0, 0, pcm16.data_ptr(), n16, B, 0, n16, 1, 16000, 11025, 0, m, pcm11.data_ptr(), m,
                                 stream.cuda_stream, "s16")

    def k11_call():
        L.check(lib.aid_chroma(h, ctypes.c_void_p(pcm11.data_ptr()), ctypes.c_void_p(off.ctypes.data), B,
                               L.AID_PCM_DEVICE, ctypes.c_void_p(words.data_ptr()), ctypes.c_void_p(woff.ctypes.data),
                               B * W, L.AID_PCM_DEVICE, ctypes.byref(got), sp))

    def engine_call():
        k6_call()
        k11_call()

    # ---- the torch route ----
    window = torch.from_numpy(R.WIN).to(dev)
    notes = torch.from_numpy(R.note_table().astype(np.int64)).to(dev)
    taps = torch.tensor([0.25, 0.75, 1.0, 0.75, 0.25], device=dev).reshape(1, 1, 5).repeat(12, 1, 1)
    masks = np.zeros((32, 1, 16, 12), np.float32)
    for j in range(16):
        for k, rs in enumerate(R.rects(j)):
            for x0, x1, y0, y1 in rs:
                masks[2 * j + k, 0, x0:x1, y0:y1] = 1.0
    masks = torch.from_numpy(masks).to(dev)
    Eth = torch.from_numpy(R.E).to(dev)  # [16][3]
    gray = torch.tensor([0, 1, 3, 2], device=dev)
    shifts = torch.arange(15, -1, -1, device=dev) * 2
    twords = torch.zeros((B, W), dtype=torch.int64, device=dev)

    def torch_call():
        for a in range(0, B, 64):
            X = torch.stft(pcm11[a:a + 64], 4096, hop_length=1365, window=window, center=False, return_complex=True)
            P = (X.real * X.real + X.imag * X.imag)[:, 10:1308, :]  # [b][1298][T]
            C = torch.zeros((P.shape[0], 12, T), device=dev).index_add_(1, notes, P)
            G = torch.nn.functional.conv1d(C, taps, groups=12)  # [b][12][T - 4]
            r = torch.sqrt((G * G).sum(dim=1, keepdim=True))
            F = torch.where(r < 0.01, torch.zeros_like(G), G / r).transpose(1, 2).unsqueeze(1)  # [b][1][T - 4][12]
            ab = 1.0 + torch.nn.functional.conv2d(F, masks).squeeze(-1)  # [b][32][W]
            A, Bv = ab[:, 0::2, :], ab[:, 1::2, :]
            q = (A.unsqueeze(-1) >= Eth[None, :, None, :] * Bv.unsqueeze(-1)).sum(dim=-1)  # [b][16][W]
            twords[a:a + 64] = (gray[q] << shifts[None, :, None]).sum(dim=1)

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
        engine_call()
        if not args.no_torch:
            torch_call()
    torch.cuda.synchronize()
    assert got.value == B * W
    res = {"bench": "chroma", "tag": args.tag, "clips": B, "seconds": args.seconds, "frames_per_clip": T,
           "words_per_clip": W, "alternations": args.alternations, "steps": args.steps}
    if not args.no_torch:
        kw = words.cpu().numpy().view(np.uint32).reshape(B, W)
        tw = twords.cpu().numpy().astype(np.uint32)
        res["differing_bits_k11_vs_torch"] = int(np.unpackbits((kw ^ tw).view(np.uint8)).sum())
        res["bits"] = B * W * 32
    ew, ed, cw, cd, tw_, td = [], [], [], [], [], []
    for _ in range(args.alternations):
        w, d = timed(engine_call, args.steps)
        ew.append(w)
        ed.append(d)
        w, d = timed(k11_call, args.steps)
        cw.append(w)
        cd.append(d)
        if not args.no_torch:
            w, d = timed(torch_call, args.steps)
            tw_.append(w)
            td.append(d)
    med = statistics.median
    res.update({"k6_k11_wall_ms": round(med(ew), 3), "k6_k11_wall_ms_min_max": [round(min(ew), 3), round(max(ew), 3)],
                "k6_k11_device_ms": round(med(ed), 3), "k6_k11_clips_per_s": round(B / med(ew) * 1e3, 1),
                "k11_wall_ms": round(med(cw), 3), "k11_wall_ms_min_max": [round(min(cw), 3), round(max(cw), 3)],
                "k11_device_ms": round(med(cd), 3), "k11_clips_per_s": round(B / med(cw) * 1e3, 1)})
    if not args.no_torch:
        res.update({"torch_wall_ms": round(med(tw_), 3), "torch_wall_ms_min_max": [round(min(tw_), 3), round(max(tw_), 3)],
                    "torch_device_ms": round(med(td), 3), "torch_clips_per_s": round(B / med(tw_) * 1e3, 1),
                    "k11_over_torch_speed": round(med(tw_) / med(cw), 3)})
    emit(res)

    if not args.no_oracle:
        x = pcm11[0].cpu().numpy()
        t0 = time.perf_counter()
        w = R.words(x)
        s = time.perf_counter() - t0
        same = bool(np.array_equal(w, words.cpu().numpy().view(np.uint32)[:W]))
        emit({"bench": "chroma_numpy_oracle", "s_per_clip": round(s, 3), "clips_per_s": round(1.0 / s, 2),
              "equals_k11": same})
    eng.close()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
