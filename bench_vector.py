#!/usr/bin/env python3
"""bench_vector.py -- K9, the vector lane's exact top-K search on one MI355X.

Workload: a catalog of 500k unit vectors of 512 floats (a 100k-track library in 10 s chunks with a 5 s hop; 1 GB
resident in HBM) and batches of 1, 32 and 256 query embeddings already on the device. One step = one
aid_vec_search(limit 50): normalise the queries, score every catalog entry, select, hits back on the host.
Against it, on the same card in alternating runs, what a user would otherwise write:
torch.topk(Q @ C.T, 50) on pre-normalised float32 tensors, values and indices copied to the host. The torch route
sums in whatever order its GEMM picks; the engine's scores are the pinned fmaf chain of spec/FPSPEC.md 9.

Reported per batch size: median ms per call over the alternations with the spread (min..max), queries/s and the
catalog bytes over the call time as a fraction of the 8 TB/s HBM peak; the MFMA scan against the VALU scan
(AID_FORCE_VEC_PATH) at 32 queries; and how many of torch's top-50 entries the exact list shares.
One JSON line per batch size, then one summary line.

--prefilter int8 switches the int8 prefilter on (aid_vec_prefilter, spec/FPSPEC.md 9.1) before the catalog is loaded:
the same hit lists from an int8 scan with exact rescoring. Each line then carries the prefilter's counters per call
(queries answered and fallen back, mean and largest |W|); the MFMA / VALU comparison is left to the `off` runs. For
an A/B, alternate whole runs of `--prefilter off` and `--prefilter int8` on one card (profiles/vec_q8_ab.txt).

--filter exclude1 | tag50 runs the same calls through aid_vec_search_filtered (spec/FPSPEC.md 9.2): with exclude1
every query excludes one random track, with tag50 every query asks for a tag (`any_of` one bit) that a random half of
the tracks carry. The catalog and the queries are the same as with `--filter none`, which calls aid_vec_search as
before. Each line then carries aid_vec_stats [0], [2] and [4] (batches answered by the threshold route, batches that
overflowed a candidate list, the largest candidate count). For the extra cost alternate whole runs of the three on one
card (profiles/vec_filter_ab.txt).
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

HBM_PEAK = 8.0e12


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=500_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--limit", type=int, default=50)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 32, 256])
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200, help="calls per timed run")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--prefilter", choices=["off", "int8"], default="off")
    ap.add_argument("--oversample", type=int, default=4)
    ap.add_argument("--filter", choices=["none", "exclude1", "tag50"], default="none")
    args = ap.parse_args()

    import torch

    from aidfp import _lib as L
    from aidfp.engine import Engine
    from aidfp.vibe import HIT_DTYPE

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(42)
    n, dim = args.entries, args.dim
    eng = Engine(16000, device=0)
    L.check(eng._lib.aid_vec_reset(eng._h, dim))
    L.check(eng._lib.aid_vec_prefilter(eng._h, 1 if args.prefilter == "int8" else 0, args.oversample))
    cat = torch.randn((n, dim), generator=g, device=dev, dtype=torch.float32)
    g_f = torch.Generator(device="cpu").manual_seed(43)  # the filters' own draws: catalog and queries stay the same
    n_tracks = (n + 4) // 5
    track_tag = (torch.rand(n_tracks, generator=g_f) < 0.5).to(torch.int64).to(dev)  # bit 0 on a random half
    step = 50_000
    for a in range(0, n, step):
        b = min(n, a + step)
        tr = (torch.arange(a, b, device=dev, dtype=torch.int32) // 5).contiguous()
        ci = (torch.arange(a, b, device=dev, dtype=torch.int32) % 5).contiguous()
        off = (ci.to(torch.float64) * 5.0).contiguous()
        torch.cuda.synchronize()
        if args.filter == "tag50":
            tg = track_tag[tr.to(torch.int64)].contiguous()
            torch.cuda.synchronize()
            L.check(eng._lib.aid_vec_add_tagged(eng._h, ctypes.c_void_p(cat[a:b].data_ptr()), ctypes.c_void_p(tr.data_ptr()),
                                                ctypes.c_void_p(ci.data_ptr()), ctypes.c_void_p(off.data_ptr()),
                                                ctypes.c_void_p(tg.data_ptr()), b - a, L.AID_PCM_DEVICE))
            continue
        L.check(eng._lib.aid_vec_add(eng._h, ctypes.c_void_p(cat[a:b].data_ptr()), ctypes.c_void_p(tr.data_ptr()),
                                     ctypes.c_void_p(ci.data_ptr()), ctypes.c_void_p(off.data_ptr()), b - a, L.AID_PCM_DEVICE))
    cn = torch.nn.functional.normalize(cat, dim=1)
    del cat
    cat_bytes = n * dim * 4

    def make_filters(nq):
        if args.filter == "none":
            return None
        flt = (L.AidVecFilter * nq)()
        ex = torch.randint(0, n_tracks, (nq,), generator=g_f).tolist()
        for k in range(nq):
            if args.filter == "tag50":
                flt[k].any_of = 1
            else:
                flt[k].n_exclude, flt[k].exclude[0] = 1, ex[k]
        return flt

    def run_engine(q, steps, flt=None):
        hits = np.zeros((q.shape[0], args.limit), HIT_DTYPE)
        nh = np.zeros(q.shape[0], np.int32)
        ph, pn, pq = ctypes.c_void_p(hits.ctypes.data), ctypes.c_void_p(nh.ctypes.data), ctypes.c_void_p(q.data_ptr())
        t0 = time.perf_counter()
        if flt is None:
            for _ in range(steps):
                L.check(eng._lib.aid_vec_search(eng._h, pq, q.shape[0], L.AID_PCM_DEVICE, args.limit, ph, pn, None))
        else:
            for _ in range(steps):
                L.check(eng._lib.aid_vec_search_filtered(eng._h, pq, q.shape[0], L.AID_PCM_DEVICE, args.limit, flt, ph, pn,
                                                         None))
        return (time.perf_counter() - t0) / steps * 1e3, hits

    def run_torch(qn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            v, i = torch.topk(qn @ cn.T, args.limit)
            v, i = v.cpu(), i.cpu()
        return (time.perf_counter() - t0) / steps * 1e3, i.numpy()

    def stats(xs):
        return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}

    summary = {}
    for nq in args.queries:
        q = torch.randn((nq, dim), generator=g, device=dev, dtype=torch.float32)
        q[0] = cn[12345] + 0.3 * q[0] / dim**0.5  # one query near a stored vector
        qn = torch.nn.functional.normalize(q, dim=1)
        torch.cuda.synchronize()
        flt = make_filters(nq)
        run_engine(q, args.warmup, flt)
        run_torch(qn, args.warmup)
        te, tt = [], []
        pst = (ctypes.c_int64 * 6)()
        vst = (ctypes.c_int64 * 8)()
        L.check(eng._lib.aid_vec_prefilter_stats(eng._h, pst, 6, 1))
        L.check(eng._lib.aid_vec_stats(eng._h, vst, 8, 1))
        for _ in range(args.alternations):
            ms, hits = run_engine(q, args.steps, flt)
            te.append(ms)
            ms, ti = run_torch(qn, args.steps)
            tt.append(ms)
        L.check(eng._lib.aid_vec_prefilter_stats(eng._h, pst, 6, 1))
        L.check(eng._lib.aid_vec_stats(eng._h, vst, 8, 1))
        shared = float(np.mean([len(set(hits[k]["entry"].tolist()) & set(ti[k].tolist())) / args.limit for k in range(nq)]))
        e, t = stats(te), stats(tt)
        line = {"queries": nq, "entries": n, "dim": dim, "limit": args.limit, "alternations": args.alternations,
                "steps": args.steps, "prefilter": args.prefilter, "filter": args.filter,
                "vec_stats": {"by_threshold": int(vst[0]), "overflowed": int(vst[2]), "cand_max": int(vst[4])}, "engine": e, "torch_topk": t,
                "engine_queries_per_s": round(nq / (e["median_ms"] * 1e-3), 1),
                "torch_queries_per_s": round(nq / (t["median_ms"] * 1e-3), 1),
                "engine_hbm_fraction": round(cat_bytes / (e["median_ms"] * 1e-3) / HBM_PEAK, 4),
                "torch_hbm_fraction": round(cat_bytes / (t["median_ms"] * 1e-3) / HBM_PEAK, 4),
                "engine_over_torch": round(e["median_ms"] / t["median_ms"], 3),
                "torch_spread_rel": round((t["max_ms"] - t["min_ms"]) / t["median_ms"], 3),
                "top_entries_shared_with_torch": round(shared, 4), "nearest_found": bool(hits[0]["entry"][0] == 12345)}
        if args.filter != "none":  # torch searched the whole catalog: the shared fraction says nothing here
            del line["top_entries_shared_with_torch"], line["nearest_found"]
        if args.prefilter == "int8":
            calls = args.alternations * args.steps
            line["prefilter_per_call"] = {"answered": pst[0] / calls, "fell_back": pst[1] / calls,
                                          "w_mean": round(pst[2] / max(1, pst[0] + pst[1]), 1), "w_max": int(pst[3]),
                                          "rescored_pairs": pst[4] / calls, "i8_scans": pst[5] / calls,
                                          "oversample": args.oversample}
        elif nq == 32 and args.filter == "none":  # the two scans against each other
            ab = {}
            for name, path in (("mfma", 1), ("valu", 2)):
                eng.force("vec_path", path)
                run_engine(q, 1)
                ab[name] = stats([run_engine(q, max(1, args.steps // 2))[0] for _ in range(max(3, args.alternations // 2))])
            eng.force("vec_path", 0)
            line["scan_ab"] = ab
        print(json.dumps(line), flush=True)
        summary[str(nq)] = {"engine_ms": e["median_ms"], "torch_ms": t["median_ms"]}
    print(json.dumps({
        "metric": f"exact top-{args.limit} search over {n} x {dim} float32 vectors, ms per call (median), 1 GPU",
        "value": summary.get("32", next(iter(summary.values())))["engine_ms"], "unit": "ms per 32-query call",
        "higher_is_better": False, "n_gpus": 1, "dtype": "float32 (pinned fmaf chain)", "data": "synthetic (random normal vectors)",
        "prefilter": args.prefilter, "filter": args.filter, "by_queries": summary,
    }), flush=True)
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
