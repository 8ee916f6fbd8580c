#!/usr/bin/env python
"""bench_live.py -- what the live index (aid_index_live) costs and saves, on the service leg's index: 10,000 synthetic
30 s tracks at 16 kHz from 44.1 kHz sources (aidfp.catalog.ingest_synthetic, as bench.py's service leg builds it).

Two engines hold the same catalog in one process: OFF (the feature off: every store makes the next query rebuild the
whole CSR) and ON (aid_index_live with --cap postings). Every comparison alternates the two and reports medians.

  (a) a store + query cycle: one 30 s track through index_add_records, then a 16-clip query_pcm.
  (b) the second pass's price: a 64-clip query_pcm and a 256-window query_windows with an empty delta (OFF: one pass)
      and with a delta holding --delta-tracks tracks (ON), and the delta build's own device time (its 2^26-key floor).
  (c) fold time: aid_index_finalize on ON (the delta built over the tail, then K4m) against OFF (the full radix build)
      after both took the same 2^20, 2^22 and 2^24 new postings (copies of stored postings under new track ids).

With AIDFP_LIB naming a library built from an older tree (no aid_index_live), or with --off-only, only the OFF side of
(a) and (b) runs: the same figures for that build, one engine in the process. One JSON line on stdout; --out also writes a readable table."""

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

SR = 16000


def med(xs):
    return round(statistics.median(xs) * 1e3, 3)  # ms


def timed(fn, torch):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=10000)
    ap.add_argument("--cycles", type=int, default=15)
    ap.add_argument("--delta-tracks", type=int, default=1000)
    ap.add_argument("--cap", type=int, default=1 << 24)
    ap.add_argument("--fold-reps", type=int, default=3)
    ap.add_argument("--fold-caps", default="20,22,24", help="log2 of the postings added before each timed fold")
    ap.add_argument("--off-only", action="store_true", help="only the OFF engine (the figures an older build gives)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from aidfp import synth
    from aidfp.catalog import ingest_synthetic
    from aidfp.engine import Engine

    if not torch.cuda.is_available():
        print("bench_live: no GPU", file=sys.stderr)
        return 2
    off = Engine(SR)
    have_live = hasattr(off._lib, "aid_index_live") and not args.off_only
    on = Engine(SR) if have_live else None
    engines = [e for e in (off, on) if e is not None]
    T = args.tracks
    for e in engines:
        ingest_synthetic(e, np.arange(T, dtype=np.uint32), 30.0, batch=1024, source_sr=44100, local=True)
        e.index_finalize()
    n_main = off.index_stats()["postings"]
    res: dict = {"index": {"tracks": T, "postings": n_main, "index_sr": SR, "source_sr": 44100},
                 "live_index": bool(have_live), "cap": args.cap}

    # new tracks' records (ids from T on) and query clips, made on the GPU once, untimed
    n_new = args.cycles + 4 + (args.delta_tracks if have_live else 0)
    n = 30 * SR
    recs = []
    pcm = torch.empty(256 * n, dtype=torch.float32, device="cuda")
    for b0 in range(0, n_new, 256):
        tr = np.arange(T + b0, T + min(b0 + 256, n_new), dtype=np.uint32)
        off.synth(pcm.data_ptr(), tr, np.zeros(len(tr), np.int64), n)
        off.extract_device(pcm.data_ptr(), np.arange(len(tr) + 1, dtype=np.int64) * n)
        off.sync()
        recs += [off.hashes(c) for c in range(len(tr))]
    del pcm
    rng = np.random.default_rng(5)
    nq = 5 * SR
    truth = rng.integers(0, T, 256).astype(np.uint32)
    qdev = torch.empty(256 * nq, dtype=torch.float32, device="cuda")
    off.synth(qdev.data_ptr(), truth, rng.integers(0, 25 * SR, 256).astype(np.int64), nq,
              noise_a=synth.noise_halfwidth(20.0), salt=9)
    torch.cuda.synchronize()
    qhost = qdev.view(256, nq).cpu().numpy()
    clips16, clips64 = list(qhost[:16]), list(qhost[:64])
    st = np.arange(256, dtype=np.int64) * nq
    en = st + nq
    if on is not None:
        on.index_live(args.cap)
    for e in engines:  # warm every shape
        e.query_pcm(clips16)
        e.query_pcm(clips64)
        e.query_windows(qdev.data_ptr(), st, en)

    # (a) store + query cycle, alternating
    nxt = 0
    cyc = {id(e): [] for e in engines}
    for i in range(args.cycles + 2):
        for e in engines:
            def cycle(e=e):
                e.index_add_records(T + nxt, recs[nxt])
                e.query_pcm(clips16)
            dt = timed(cycle, torch)
            if i >= 2:  # two warm-up cycles
                cyc[id(e)].append(dt)
        nxt += 1
    res["a_store_query_cycle_ms"] = {"live_off": med(cyc[id(off)])}
    if on is not None:
        res["a_store_query_cycle_ms"]["live_on"] = med(cyc[id(on)])
        res["a_live_stats"] = on.index_live_stats()

    # (b) the second pass: OFF has one CSR over everything, ON a delta of --delta-tracks tracks
    if on is not None:
        for k in range(args.delta_tracks):
            for e in engines:
                e.index_add_records(T + nxt, recs[nxt])
            nxt += 1
        on.profile_enable(True)
        on.profile_read(reset=True)
        res["b_delta_build_host_ms"] = round(timed(lambda: on.query_pcm(clips16[:1]), torch) * 1e3, 3)
        res["b_delta_build_device_ms"] = round(on.profile_read(reset=True)["index_build"][0], 3)
        on.profile_enable(False)
        res["b_delta_postings"] = on.index_live_stats()["delta_postings"]
    off.index_finalize()
    b = {}
    for name, fn in (("query_pcm_64", lambda e: e.query_pcm(clips64)),
                     ("query_windows_256", lambda e: e.query_windows(qdev.data_ptr(), st, en))):
        ts = {id(e): [] for e in engines}
        for i in range(22):
            for e in engines:
                dt = timed(lambda e=e: fn(e), torch)
                if i >= 2:
                    ts[id(e)].append(dt)
        b[name] = {"one_pass": med(ts[id(off)])}
        if on is not None:
            b[name]["delta_%d_tracks" % args.delta_tracks] = med(ts[id(on)])
    res["b_query_ms"] = b
    if on is not None:  # the same rows either way
        g, w = on.query_pcm(clips64), off.query_pcm(clips64)
        res["b_rows_equal"] = bool(all(np.array_equal(x, y) for x, y in zip(g, w)))
        res["b_top1"] = float(np.mean([len(r) > 0 and r[0][1] == t for r, t in zip(g, truth[:64])]))

    # (c) fold against the full build
    if on is not None:
        on.index_finalize()
        on.profile_enable(True)
        off.profile_enable(True)
        folds = {}
        for lg in [int(x) for x in args.fold_caps.split(",")]:
            m = min(1 << lg, n_main)
            h = torch.empty(m, dtype=torch.int32, device="cuda")
            tr = torch.empty(m, dtype=torch.int32, device="cuda")
            t = torch.empty(m, dtype=torch.int32, device="cuda")
            t_fold, t_full, d_merge, d_dbuild, d_full = [], [], [], [], []
            for r in range(args.fold_reps + 1):
                off.index_export_device(h.data_ptr(), tr.data_ptr(), t.data_ptr(), 0, m)
                tr += int(off.index_stats()["tracks"])  # new ids, above every stored one
                torch.cuda.synchronize()
                for e in engines:
                    e.index_add_postings(h.data_ptr(), tr.data_ptr(), t.data_ptr(), m, device=True)
                    e.profile_read(reset=True)
                a = timed(on.index_finalize, torch)
                bfull = timed(off.index_finalize, torch)
                pon, poff = on.profile_read(reset=True), off.profile_read(reset=True)
                if r >= 1:
                    t_fold.append(a)
                    t_full.append(bfull)
                    d_merge.append(pon["index_merge"][0] * 1e-3)
                    d_dbuild.append(pon["index_build"][0] * 1e-3)
                    d_full.append(poff["index_build"][0] * 1e-3)
            folds["2^%d" % lg] = {"added": m, "postings_after": off.index_stats()["postings"],
                                  "fold_host_ms": med(t_fold), "full_build_host_ms": med(t_full),
                                  "fold_delta_build_device_ms": med(d_dbuild), "fold_merge_device_ms": med(d_merge),
                                  "full_build_device_ms": med(d_full)}
            del h, tr, t
        res["c_fold_ms"] = folds
        ck = (on.index_checksum(), off.index_checksum())
        _, p_on = on.index_csr(offsets=False)
        _, p_off = off.index_csr(offsets=False)
        res["c_csr_equal"] = bool(ck[0] == ck[1] and np.array_equal(p_on, p_off))
    for e in engines:
        e.close()
    print(json.dumps(res))
    if args.out:
        lines = ["bench_live.py " + " ".join(sys.argv[1:]), json.dumps(res["index"]), ""]
        for k, v in res.items():
            if k != "index":
                lines.append(f"{k}: {json.dumps(v)}")
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
