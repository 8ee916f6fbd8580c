"""f32 against s16 PCM on the extraction paths, as alternating rounds of one run on one box.

The bench batch (256 x 10 s at 44.1 kHz) in three forms, each in both formats (the s16 samples are the generator's
own int16 values, the f32 samples their widening q / 32768, so both compute the same records):
  * host_pinned:  page-locked host clips handed to aid_extract / aid_extract_s16 in place: K1-K3 plus the ONE H2D copy
                  of the span (451.6 MB as f32, 225.8 MB as s16); audio-s/s and the bytes per second the whole step
                  moves over PCIe (the copy alone is faster: the kernels follow it on the same stream);
  * extract_host: one Engine.extract_host(clips, fmt=...) call on a list of host arrays: the same plus Python's
                  concatenation of the clips (beyond the page-locked staging's 64 MiB into pageable memory) and the
                  fetch of every clip's records;
  * k1_device:    the batch resident in HBM, AID_K_STFT per launch from HIP events: what the s16 ring (packed pairs,
                  converted at the window multiply) costs or gains in K1 itself.

usage: python probes/hostfed_s16_ab.py [--steps N] [--rounds R]
"""
import argparse
import ctypes
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
    args = ap.parse_args()

    import torch
    from aidfp._lib import check
    from aidfp.engine import AID_PCM_HOST, Engine

    SR, CLIPS, SEC = 44100, 256, 10
    n = SR * SEC
    eng = Engine(SR)
    f32 = torch.empty(CLIPS * n, dtype=torch.float32, device="cuda")
    eng.synth(f32.data_ptr(), np.arange(CLIPS, dtype=np.uint32) + 1, np.zeros(CLIPS, np.int64), n)
    s16 = (f32 * 32768.0).to(torch.int16)
    assert torch.equal(s16.float() / 32768.0, f32)
    dev = {"f32": f32, "s16": s16}
    pinned = {k: v.cpu().pin_memory() for k, v in dev.items()}
    lists = {k: list(v.numpy().reshape(CLIPS, n)) for k, v in pinned.items()}
    offs = np.arange(CLIPS + 1, dtype=np.int64) * n
    offs_p = offs.ctypes.data_as(ctypes.c_void_p)
    fn = {"f32": eng._lib.aid_extract, "s16": eng._lib.aid_extract_s16}
    audio = CLIPS * SEC
    bytes_per = {"f32": 4 * CLIPS * n, "s16": 2 * CLIPS * n}

    def timed(call) -> float:
        call()
        eng.sync()
        t = time.perf_counter()
        for _ in range(args.steps):
            call()
        eng.sync()
        return (time.perf_counter() - t) / args.steps

    def k1_ms(fmt: str) -> float:
        eng.profile_enable(True)
        eng.profile_select([0])  # AID_K_STFT
        eng.profile_read(reset=True)
        for _ in range(args.steps):
            eng.extract_device(dev[fmt].data_ptr(), offs, fmt=fmt)
        eng.sync()
        ms, cnt = eng.profile_read(reset=True)["stft_power"]
        eng.profile_select(None)
        eng.profile_enable(False)
        return ms / cnt

    def host_pinned(f: str) -> float:
        return timed(lambda: check(fn[f](eng._h, ctypes.c_void_p(pinned[f].data_ptr()), offs_p, CLIPS, AID_PCM_HOST,
                                         None)))

    rounds = {form: {"f32": [], "s16": []} for form in ("host_pinned", "extract_host", "k1_device")}
    for r in range(args.rounds + 1):  # round 0 warms up (allocations, clocks)
        for f in ("f32", "s16"):
            a = host_pinned(f)
            t = time.perf_counter()
            eng.extract_host(lists[f], fmt=f)
            b = time.perf_counter() - t
            c = k1_ms(f)
            if r:
                rounds["host_pinned"][f].append(a)
                rounds["extract_host"][f].append(b)
                rounds["k1_device"][f].append(c * 1e-3)
    out = {"batch": f"{CLIPS} x {SEC} s at {SR} Hz", "steps": args.steps, "rounds": args.rounds}
    for form, by in rounds.items():
        out[form] = {}
        for f in ("f32", "s16"):
            s = float(np.median(by[f]))
            row = {"ms": round(s * 1e3, 4), "rounds_ms": [round(x * 1e3, 4) for x in by[f]]}
            if form != "k1_device":
                row["audio_s_per_s"] = round(audio / s, 1)
                row["pcie_bytes_per_step"] = bytes_per[f]
                row["step_gbs"] = round(bytes_per[f] / s / 1e9, 1)
            out[form][f] = row
        out[form]["s16_over_f32_time"] = round(out[form]["s16"]["ms"] / out[form]["f32"]["ms"], 4)
    # the two formats give the same records
    check(fn["f32"](eng._h, ctypes.c_void_p(pinned["f32"].data_ptr()), offs_p, CLIPS, AID_PCM_HOST, None))
    ref = [eng.hashes(c) for c in range(0, CLIPS, 37)]
    check(fn["s16"](eng._h, ctypes.c_void_p(pinned["s16"].data_ptr()), offs_p, CLIPS, AID_PCM_HOST, None))
    got = [eng.hashes(c) for c in range(0, CLIPS, 37)]
    out["records_equal"] = all(np.array_equal(a, b) for a, b in zip(ref, got))
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
