#!/usr/bin/env python3
"""bench.py -- fingerprint-extraction throughput on MI355X (BASELINE.json metric).

Workload (BASELINE.json configs[1]): a batch of 256 x 10 s
44.1 kHz mono synthetic clips, resident in HBM (generated on the device by
aid_synth). One step = one pass of K1 stft_power -> K2 peak_pick -> K3
landmark_hash over the whole batch through the C ABI.

N GPUs: one process per GPU (torch.distributed, RCCL backend), each rank
fingerprints its own 256-clip batch (extraction shards by clip, no data-path
collective: weak scaling). value = audio-seconds of all ranks / max-rank time.
`python bench.py --gpus N` with no WORLD_SIZE in the environment starts the N
ranks itself (a child `torch.distributed.run`, before anything touches the GPU)
and exits with its status; under a launcher WORLD_SIZE must equal --gpus.

A plain run (`bench.py --gpus 1 --steps N --warmup W`) does only what the headline needs: set-up, W warm-up
steps and the clock settle, the N timed steps, the outputs of the last timed step if `--dump-outputs DIR` is
given, and the result line (value, ms_per_step, K1's events of the timed region). Everything below -- the
checks against the oracle, the CPU baselines, the per-kernel breakdown and roofline, and the other workloads
-- runs only with `--full`; the `--no-*` and per-leg options select among the legs of a `--full` run.

`--dump-outputs DIR` writes what the last timed step left in the engine, as a caller reads it back
(aid_result_counts, aid_result_hashes), to DIR/<name>.npy in float64 (every value is an integer below 2^32, so
exact): `counts` [clips], and `hash` / `t1` [sum of counts], the records' two 32-bit halves, clips concatenated
in order. The inputs are generated from fixed seeds, so two runs with the same arguments dump the same data.

Extra keys of the `--full` line (none of them is `value`):
  * roofline -- the dominant kernel's algorithmic HBM bytes per launch / its mean launch
    time from HIP events on the launch stream in the timed region, against 8.0 TB/s; plus
    which unit binds: traffic_frac (PMC bytes) and valu_issue_frac (SQ_INSTS_VALU) per
    extraction kernel, from the newest committed profiles/;
  * fullband -- the same batch with partials up to 20 kHz (no cold upper blocks);
  * catalog -- BASELINE config 3: 100k x 30 s tracks sharded over the ranks, extract +
    the RCCL all-gather of the postings (aid_index_allgather) + the index build, then the replicas
    checked (replicas_identical: device checksums compared across ranks; shard_parity: 8 tracks of
    every rank's shard against the oracle on rank 0); its exact_lane sub-key is BASELINE config 4
    against that index (10k + 1k noisy 5 s clips per rank, aid_exact_lane), with parity: 64 of the
    timed clips checked against the oracle at the catalog's scale (records, K5 rows on every path,
    the lane's rows against an all-oracle lane);
  * service -- the drop-in olaf_query path through the query coalescer at 1 / 16 / 64 clients;
  * stream -- BASELINE config 5 at serving scale: 256 live 48 kHz stereo streams per rank through
    aidfp.stream.StreamBank (one batched K6 + one windowed K1-K5 call per 2.5 s push), with parity
    of the first windows against the oracle route;
  * cpu_baseline -- the bit-exact C oracle on the host cores, and the NumPy/SciPy path, on
    rank 0 at N=1 over bounded samples of the same clips.
A failed check (headline parity, catalog checks, stream parity) exits 1; a leg that hangs past
--leg-deadline exits 3 after the line is printed.
"""

from __future__ import annotations

import argparse
import datetime
import gc
import json
import os
import socket
import subprocess
import sys
import threading
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT / "audio-ident_amd"))

METRIC = "audio-seconds fingerprinted/sec/GPU; landmark-hash bit-exact vs CPU ref"
SR = 44100
CLIPS = 256
CLIP_S = 10
HBM_PEAK_GBS = 8000.0
SIMDS = 1024          # 256 CUs x 4 SIMDs (MI355X_MICROARCH)
CLOCK_HZ = 2.4e9      # max engine clock
VALU_CYCLES = 2       # a wave64 VALU instruction issues over 2 cycles on a SIMD-32
KERNEL_SQ = {"stft_power": "k_stft_power", "peak_pick": "k_peak_pick", "landmark_write": "k_landmarks"}
KERNEL_PMC = {"stft_power": "stft_power", "peak_pick": "peak_pick", "landmark_write": "landmarks"}


def launch_plan(gpus: int, env) -> str:
    """'run' in this process, 'spawn' N ranks, or 'error' (a launcher started another world size)."""
    ws = env.get("WORLD_SIZE")
    if ws is None:
        return "spawn" if gpus > 1 else "run"
    return "run" if int(ws) == gpus else "error"


def spawn_ranks(gpus: int) -> int:
    """`torch.distributed.run` with one rank per GPU as a CHILD process (never an exec: this process has not
    touched the GPU and does not), forwarding our arguments; returns its exit status."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}",
           "--master-addr", "127.0.0.1", f"--master-port={port}", str(Path(__file__).resolve()), *sys.argv[1:]]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.run(cmd, env=env).returncode


def algorithmic_bytes(frames: int, samples: int) -> dict:
    """Per-launch algorithmic HBM bytes of each extraction kernel."""
    return {
        # K1 reads every PCM sample once, writes 1024 fp32 bins per frame
        "stft_power": 4 * samples + 4 * 1024 * frames,
        # K2 reads the power plane once, writes a 128-byte peak mask per frame
        "peak_pick": 4 * 1024 * frames + 128 * frames,
    }


def load_pmc() -> tuple[dict, str | None]:
    """HBM bytes per launch (2 x FETCH_SIZE + WRITE_SIZE, gfx950 correction) from the newest committed PMC
    summary: {kernel: bytes}."""
    for f in sorted((ROOT / "profiles").glob("pmc_*.json"), reverse=True):
        try:
            d = json.loads(f.read_text()).get("kernels", {})
            out = {k: float(d[v]["hbm_bytes_per_launch"]) for k, v in KERNEL_PMC.items()
                   if v in d and d[v].get("hbm_bytes_per_launch")}
            if out:
                return out, f.name
        except Exception:
            continue
    return {}, None


def load_pmc_k5() -> tuple[dict | None, str | None]:
    """The K5 (config-4 match) summary of the newest committed PMC file that has one (tools/k5_pmc_summary.py):
    HBM bytes and kernel time per exact-lane call, per K5 kernel and in sum."""
    for f in sorted((ROOT / "profiles").glob("pmc_*.json"), reverse=True):
        try:
            d = json.loads(f.read_text())
        except Exception:
            continue
        if isinstance(d.get("k5"), dict):
            return d["k5"], f.name
    return None, None


def load_sq() -> tuple[dict, str | None]:
    """SQ_INSTS_VALU (and the rest) per launch from the newest committed SQ summary (sq_*.txt lines
    `<dir> <kernel> <counter> n= <n> mean=<v>`): {kernel: {counter: mean}}."""
    for f in sorted((ROOT / "profiles").glob("sq_*.txt"), reverse=True):
        out: dict = {}
        try:
            for ln in f.read_text().splitlines():
                parts = ln.split()
                if len(parts) >= 5 and parts[-1].startswith("mean="):
                    out.setdefault(parts[1], {})[parts[2]] = float(parts[-1][5:])
        except Exception:
            continue
        if "SQ_INSTS_VALU" in out.get(KERNEL_SQ["stft_power"], {}):  # an extraction-kernel summary
            return out, f.name
    return {}, None


def cpu_info() -> dict:
    """Host CPU model and the cores this process may use: the affinity set, capped by a cgroup CPU quota
    (a GPU box shows the whole machine's CPUs to nproc but grants a share)."""
    model = "unknown"
    try:
        for ln in Path("/proc/cpuinfo").read_text().splitlines():
            if ln.startswith("model name"):
                model = ln.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    visible = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        q, per = Path("/sys/fs/cgroup/cpu.max").read_text().split()
        if q != "max":
            quota = float(q) / float(per)
    except (OSError, ValueError):
        pass
    usable = visible if quota is None else max(1, min(visible, int(quota)))
    return {"model": model, "cpus_visible": visible, "cgroup_quota_cpus": quota, "cores": usable}


def parity(eng, host_pcm: np.ndarray, ref=None) -> dict:
    """Hashes of the bench batch (left by the last step) against the C oracle, bit for bit.

    `ref` = the oracle's records for the first len(ref) clips when the cpu_baseline leg already
    computed them; otherwise the oracle runs here on the first 8 clips."""
    if ref is None:
        sys.path.insert(0, str(ROOT / "oracle"))
        import oracle as O  # checker only

        ref = O.fingerprint_batch(host_pcm[:8], 512, threads=min(8, os.cpu_count() or 1))
    bad = [c for c in range(len(ref)) if not np.array_equal(eng.hashes(c), ref[c])]
    return {"clips": len(ref), "hashes": int(sum(len(r) for r in ref)), "bit_exact": not bad,
            "mismatched_clips": bad[:8], "oracle": "oracle/fp_oracle.c"}


MAG_BANDS_DB = ((0, 20), (20, 40), (40, 60), (60, 80))
MAG_REL_TOL = 1e-4  # north_star: "STFT magnitudes match within 1e-4 rel"
MAG_TOL_WITHIN_DB = 60  # ... per bin, for every bin within this many dB of its frame's peak


def magnitude_parity(host_pcm: np.ndarray, clips: int = 4, sr: int = 44100) -> dict:
    """Per-bin relative error of the product path's binary32 power (aid_result_power of an AID_FLAG_KEEP_POWER
    engine, K1's own output) against float64 numpy (oracle.stft_power_f64: pocketfft of the same frames), as
    magnitudes |sqrt(P) - sqrt(P64)| / sqrt(P64), bucketed by dB below the frame's peak.
    binary32 delivers 1e-4 per bin down to MAG_TOL_WITHIN_DB below the frame peak (a bin's absolute rounding
    error is set by the frame's energy, so its relative error grows as the bin falls below the peak);
    `ok` asserts exactly that band. The power bits are also checked against the C oracle."""
    sys.path.insert(0, str(ROOT / "oracle"))
    import oracle as O  # checker only

    from aidfp.engine import Engine

    x = [np.ascontiguousarray(c) for c in host_pcm[:clips]]
    hop = 512 if sr >= 32000 else 256  # FPSPEC 1
    stats = {f"{a}-{b}dB": {"bins": 0, "max_rel": 0.0} for a, b in MAG_BANDS_DB}
    p999 = {k: [] for k in stats}
    bits_equal = True
    with Engine(sr, keep_power=True) as eng:
        eng.extract_host(x)
        for c, xc in enumerate(x):
            P = eng.power(c, len(xc))
            bits_equal &= bool(np.array_equal(P.view(np.uint32), O.stft_power(xc, hop).view(np.uint32)))
            R = O.stft_power_f64(xc, hop)
            peak = R.max(axis=1, keepdims=True)
            with np.errstate(divide="ignore", invalid="ignore"):
                db = 10.0 * np.log10(peak / R)
                rel = np.abs(np.sqrt(P.astype(np.float64)) - np.sqrt(R)) / np.sqrt(R)
            for (a, b), k in zip(MAG_BANDS_DB, stats):
                m = (db >= a) & (db < b) & (R > 0)
                if m.any():
                    stats[k]["bins"] += int(m.sum())
                    stats[k]["max_rel"] = max(stats[k]["max_rel"], float(rel[m].max()))
                    p999[k].append(float(np.percentile(rel[m], 99.9)))
    for k in stats:
        stats[k]["p999_rel"] = max(p999[k]) if p999[k] else None
        stats[k]["max_rel"] = float(f"{stats[k]['max_rel']:.3e}")
    within = [k for (a, b), k in zip(MAG_BANDS_DB, stats) if b <= MAG_TOL_WITHIN_DB]
    return {"clips": len(x), "per_bin": stats, "tolerance_rel": MAG_REL_TOL, "tolerance_within_db": MAG_TOL_WITHIN_DB,
            "ok": bits_equal and all(stats[k]["max_rel"] <= MAG_REL_TOL for k in within),
            "power_bits_equal_oracle": bits_equal,
            "note": "magnitude = sqrt(binary32 power of K1) vs sqrt(float64 numpy power), per bin; bands in dB below "
                    "the frame's peak power"}


def cpu_baseline(host_pcm: np.ndarray, min_s: float = 6.0) -> tuple[dict, list]:
    """The C oracle on the host cores over the bench batch: passes of all 256 clips on every usable core until
    `min_s` seconds have elapsed (>= 1 pass), then 64 clips on one thread; then the NumPy/SciPy path
    (oracle.fingerprint_numpy) over 16 clips on one process and on a process pool. Returns the oracle's
    records of the batch (for the parity check) and the baseline dict."""
    sys.path.insert(0, str(ROOT / "oracle"))
    import oracle as O  # checker / CPU baseline only

    ci = cpu_info()
    threads = ci["cores"]
    sample = host_pcm[: min(len(host_pcm), 256)]
    O.fingerprint_batch(sample[:2], 512, threads=1)  # warm (tables)
    passes = 0
    t = time.perf_counter()
    while True:
        ref = O.fingerprint_batch(sample, 512, threads=threads)
        passes += 1
        dt_mt = time.perf_counter() - t
        if dt_mt >= min_s:
            break
    one = sample[:64]
    t = time.perf_counter()
    O.fingerprint_batch(one, 512, threads=1)
    dt_1 = time.perf_counter() - t
    audio_mt = passes * sample.shape[0] * sample.shape[1] / SR
    audio_1 = one.shape[0] * one.shape[1] / SR
    np_leg = numpy_baseline(sample[:16], threads)
    cat = catalog_cpu_estimate(O, ref, audio_mt / dt_mt, threads, batch_s=sample.shape[0] * sample.shape[1] / SR)
    return ref, {
        "value": round(audio_mt / dt_mt, 1),
        "unit": "audio-s/s",
        "cores": threads,
        "kind": "port",
        "cpu_model": ci["model"],
        "cpus_visible": ci["cpus_visible"],
        "cgroup_quota_cpus": ci["cgroup_quota_cpus"],
        "sample": f"{passes} pass(es) over the {sample.shape[0]} x {CLIP_S} s clips of the same batch through "
                  f"oracle/fp_oracle.c (bit-exact C restatement, -O2) on {threads} host threads ({dt_mt:.1f} s); "
                  f"single-thread {audio_1 / dt_1:.1f} audio-s/s over {one.shape[0]} clips ({dt_1:.1f} s)",
        "single_thread": round(audio_1 / dt_1, 1),
        "numpy_scipy": np_leg,
        "catalog": cat,
    }


def catalog_cpu_estimate(O, ref: list, extract_rate: float, threads: int, batch_s: float, tracks: int = 100000,
                         track_s: float = 30.0) -> dict:
    """Config 3 on the host (sub-sampled, extrapolated, labelled): the catalog's extraction at the
    multi-thread oracle rate measured above, plus the index build as the oracle's sort (fp_index_sort, one thread)
    of the batch's own postings, scaled n log n to the catalog's posting count (the batch's postings per audio
    second times the catalog's audio: ~580 M for generator v2, as the bench's catalog leg holds)."""
    p = np.concatenate([np.stack([(r & np.uint64(0xFFFFFFFF)).astype(np.uint32), np.full(len(r), c, np.uint32),
                                  (r >> np.uint64(32)).astype(np.uint32)], axis=1) for c, r in enumerate(ref)])
    p = np.ascontiguousarray(p)
    t = time.perf_counter()
    O.lib().fp_index_sort(O._ptr(p), len(p))
    ts = time.perf_counter() - t
    n = len(p)
    audio = tracks * track_s
    postings = int(round(n * audio / batch_s))
    sort_s = ts * (postings / n) * (np.log2(postings) / np.log2(max(n, 2)))
    extract_s = audio / extract_rate
    return {"value": float(round(audio / (extract_s + sort_s), 1)), "unit": "audio-s/s", "extrapolated": True,
            "sample": f"extraction at the {threads}-thread oracle rate above ({extract_s:.0f} s for {tracks} x "
                      f"{track_s:.0f} s); index sort of the batch's {n} postings in {ts:.3f} s on one thread, scaled "
                      f"n log n to {postings} postings ({sort_s:.0f} s)"}


def _np_worker(args):
    x, hop = args
    sys.path.insert(0, str(ROOT / "oracle"))
    import oracle as O

    return O.fingerprint_numpy(x, hop)


def numpy_baseline(clips: np.ndarray, procs: int) -> dict:
    """oracle.fingerprint_numpy (float64 rfft + scipy.ndimage.maximum_filter + vectorised pairing): one
    process (pocketfft is single-threaded), then a process pool of `procs` workers."""
    import multiprocessing as mp

    sys.path.insert(0, str(ROOT / "oracle"))
    import oracle as O

    O.fingerprint_numpy(clips[0], 512)  # warm (scipy import)
    t = time.perf_counter()
    for x in clips[:4]:
        O.fingerprint_numpy(x, 512)
    dt1 = time.perf_counter() - t
    audio1 = 4 * clips.shape[1] / SR
    work = [(clips[i % len(clips)], 512) for i in range(max(len(clips), 2 * procs))]
    ctx = mp.get_context("spawn")
    with ctx.Pool(procs) as pool:
        pool.map(_np_worker, work[:procs])  # start-up
        t = time.perf_counter()
        pool.map(_np_worker, work)
        dtp = time.perf_counter() - t
    return {"value_1proc": round(audio1 / dt1, 1), "value_pool": round(len(work) * clips.shape[1] / SR / dtp, 1),
            "procs": procs, "unit": "audio-s/s",
            "sample": f"4 clips on one process ({dt1:.1f} s), {len(work)} clips on {procs} processes ({dtp:.1f} s)",
            "note": "float64 NumPy/SciPy restatement of FPSPEC 4-6 (oracle.fingerprint_numpy); its records equal "
                    "the oracle's on the synthetic clips (tests/test_oracle.py), but it is not the bit-exact checker"}


def roofline_units(kern: dict, pmc: dict, sq: dict) -> dict:
    """Per extraction kernel: which unit binds, from the committed counters and this run's durations."""
    out = {}
    for k, v in kern.items():
        ms = v.get("ms_per_launch")
        if not ms:
            continue
        d = {"ms_per_launch": round(ms, 5)}
        if k in pmc:
            d["traffic_bytes"] = pmc[k]
            d["traffic_gbs"] = round(pmc[k] / (ms * 1e-3) / 1e9, 1)
            d["traffic_frac"] = round(pmc[k] / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
        c = sq.get(KERNEL_SQ.get(k, ""), {})
        if "SQ_INSTS_VALU" in c:
            d["valu_insts"] = c["SQ_INSTS_VALU"]
            d["valu_issue_frac"] = round(c["SQ_INSTS_VALU"] * VALU_CYCLES / (SIMDS * CLOCK_HZ * ms * 1e-3), 4)
        if "SQ_INSTS_LDS" in c:
            d["lds_insts"] = c["SQ_INSTS_LDS"]
        out[k] = d
    return out


def dump_outputs(eng, out_dir: Path, rank: int = 0) -> dict:
    """The last extraction's results as a caller of aid_extract receives them (counts per clip; every clip's
    records hash | t1 << 32, split into their 32-bit halves), as float64 .npy files under `out_dir`. Ranks
    above 0 (N > 1) write <name>_rank<r>.npy. Returns {name: elements}."""
    out_dir.mkdir(parents=True, exist_ok=True)
    counts = eng.counts()
    recs = [eng.hashes(c) for c in range(len(counts))]
    rec = np.concatenate(recs) if recs else np.zeros(0, np.uint64)
    arrays = {"counts": counts.astype(np.float64),
              "hash": (rec & np.uint64(0xFFFFFFFF)).astype(np.float64),
              "t1": (rec >> np.uint64(32)).astype(np.float64)}
    sfx = f"_rank{rank}" if rank else ""
    for name, a in arrays.items():
        np.save(out_dir / f"{name}{sfx}.npy", a)
    return {k: int(a.size) for k, a in arrays.items()}


def headline_roofline(kern: dict, frames: int, samples: int, step_s: float) -> dict:
    """The `roofline` object of the line: the dominant extraction kernel's algorithmic bytes over its time,
    the committed counters per kernel, and the whole step (step_s seconds) on the same accounting."""
    alg = algorithmic_bytes(frames, samples)
    dom = max(("stft_power", "peak_pick"), key=lambda k: kern[k]["ms_per_launch"] if k in kern else 0.0)
    dom_ms = kern[dom]["ms_per_launch"]
    achieved = alg[dom] / (dom_ms * 1e-3) / 1e9
    pmc, pmc_src = load_pmc()
    sq, sq_src = load_sq()
    units = roofline_units(kern, pmc, sq)
    return {
        "kernel": dom,
        "bound": "hbm",
        "achieved": round(achieved, 1),
        "peak": HBM_PEAK_GBS,
        "unit": "GB/s",
        "frac": round(achieved / HBM_PEAK_GBS, 4),
        "traffic": pmc.get(dom),
        "algorithmic_bytes_per_launch": alg[dom],
        "duration_ms": round(dom_ms, 5),
        "duration_source": kern[dom]["pass"],
        "traffic_frac": units.get(dom, {}).get("traffic_frac"),
        "valu_issue_frac": units.get(dom, {}).get("valu_issue_frac"),
        "per_kernel": units,
        "traffic_source": pmc_src,
        "sq_source": sq_src,
        "extraction_kernels_ms_per_step": round(sum(v["ms_per_launch"] for v in kern.values()), 4),
        # the whole step against the same staged-dataflow accounting (K1 + K2 bytes of SURVEY 8(d); K3's
        # mask reads and record writes are < 1 % and left out): how far the pipeline is from streaming
        "step_staged_bytes": alg["stft_power"] + alg["peak_pick"],
        "step_achieved": round((alg["stft_power"] + alg["peak_pick"]) / step_s / 1e9, 1),
        # the step on the bytes it actually moves: PMC bytes of K1 + K2 + K3 per step / ms_per_step / 8 TB/s
        "step_traffic_bytes": (sum(pmc[k] for k in KERNEL_PMC) if all(k in pmc for k in KERNEL_PMC) else None),
        "step_traffic_frac": (round(sum(pmc[k] for k in KERNEL_PMC) / step_s / 1e9 / HBM_PEAK_GBS, 4)
                              if all(k in pmc for k in KERNEL_PMC) else None),
        "note": "frac = SURVEY 8(d) staged-dataflow bytes (PCM + the full power plane) / the kernel's time. K1 "
                "stores only hot 64-bin blocks and K2 reads only those, so the bytes actually moved (traffic, PMC "
                "2 x FETCH_SIZE + WRITE_SIZE) are below that on band-limited audio: traffic_frac says how busy HBM "
                "is, valu_issue_frac (SQ_INSTS_VALU x 2 cycles / (1024 SIMDs x 2.4 GHz x duration)) how busy the "
                "vector issue is -- the larger of the two is the binding unit",
    }


def run_steps(eng, pcm_ptr, offs, stream, steps, torch):
    for _ in range(steps):
        eng.extract_device(pcm_ptr, offs, stream)
    torch.cuda.synchronize()


def settle(eng, pcm_ptr, offs, stream, seconds, torch) -> int:
    """Keep stepping (untimed) until the GPU has been busy for `seconds`: an idle MI355X needs ~25 ms of
    load to reach its steady clocks (probes/ramp_probe.py)."""
    n = 0
    t = time.perf_counter()
    while time.perf_counter() - t < seconds:
        run_steps(eng, pcm_ptr, offs, stream, 10, torch)
        n += 10
    return n


def breakdown(eng, pcm_ptr, offs, stream, steps, torch) -> dict:
    """Untimed pass with events on every extraction kernel: {kernel: (ms, launches)}."""
    eng.profile_select(None)
    eng.profile_enable(True)
    eng.profile_read(reset=True)
    run_steps(eng, pcm_ptr, offs, stream, steps, torch)
    prof = eng.profile_read(reset=True)
    eng.profile_enable(False)
    return {k: {"ms_per_launch": ms / cnt, "launches": cnt} for k, (ms, cnt) in prof.items() if cnt}


def fullband_leg(eng, pcm, offs, stream, args, rank, torch, dist) -> dict:
    """The same batch shape with partials in [100, 20000) Hz: every 64-bin block up to ~20 kHz is hot, so
    K1 stores and K2 loads the whole band (the headline data stops at 8 kHz, ~60 % cold blocks)."""
    tracks = np.arange(CLIPS, dtype=np.uint32) + np.uint32(rank * CLIPS + 500000)
    n = SR * CLIP_S

    def warm():
        eng.synth(pcm.data_ptr(), tracks, np.zeros(CLIPS, np.int64), n, fmax_hz=20000)
        run_steps(eng, pcm.data_ptr(), offs, stream, max(1, args.warmup), torch)
        settle(eng, pcm.data_ptr(), offs, stream, args.settle, torch)

    _agreed(warm, "fullband (warm-up)", dist)
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_steps(eng, pcm.data_ptr(), offs, stream, args.steps, torch)
    if dist:
        dist.barrier()
    el = time.perf_counter() - t0
    el = _max_over_ranks(el, dist, torch)
    world = dist.get_world_size() if dist else 1
    kern = _agreed(lambda: breakdown(eng, pcm.data_ptr(), offs, stream, max(1, min(args.steps, 20)), torch),
                   "fullband (breakdown)", dist)
    out = {"value": round(world * CLIPS * CLIP_S * args.steps / el, 1), "unit": "audio-s/s",
           "ms_per_step": round(el / args.steps * 1e3, 4), "hashes_per_step_per_gpu": int(eng.counts().sum()),
           "kernels": {k: round(v["ms_per_launch"], 5) for k, v in kern.items()},
           "data": "aid_synth_band fmax 20 kHz (same seed rules, track ids offset by 500000)"}
    if rank == 0:
        sys.path.insert(0, str(ROOT / "oracle"))
        import oracle as O  # checker only

        host = pcm.view(CLIPS, n)[:4].cpu().numpy()
        ref = O.fingerprint_batch(host, 512, threads=min(8, os.cpu_count() or 1))
        out["parity"] = {"clips": 4, "bit_exact": all(np.array_equal(eng.hashes(c), ref[c]) for c in range(4))}
    return out


_T0 = time.perf_counter()


def _log(msg: str) -> None:
    """Progress on stderr (rank 0): which leg runs, so a long run shows it is alive."""
    if os.environ.get("RANK", "0") == "0":
        print(f"[bench {time.perf_counter() - _T0:7.1f} s] {msg}", file=sys.stderr, flush=True)


def _agreed(fn, what: str, dist):
    """Run the rank-local step fn() and, at N > 1, agree on its success before any later collective
    (aidfp.catalog.agreed): a failure on one rank raises on every rank instead of leaving the others
    blocked in the next barrier / all-reduce."""
    if not dist:
        return fn()
    from aidfp.catalog import agreed

    return agreed(fn, what)


def _max_over_ranks(x: float, dist, torch) -> float:
    if not dist:
        return x
    on_dev = dist.get_backend() == "nccl"
    t = torch.tensor([x], dtype=torch.float64, device="cuda" if on_dev else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def catalog_leg(args, rank, world, dist, torch) -> dict:
    """BASELINE config 3: args.catalog_tracks x args.catalog_seconds synthetic tracks, shard(rank) generated and
    fingerprinted on each GPU, the postings replicated by ONE exchange (native aid_index_allgather over RCCL;
    under the gloo rehearsal, pack/splice around gloo), then the full CSR built on every GPU. value = the job's
    audio-seconds / the slowest rank's ingest time (extract + exchange + build; on-device generation excluded,
    reported apart), as bench_catalog.py."""
    from aidfp.catalog import ingest_synthetic
    from aidfp.engine import Engine

    exchange = "native" if (not dist or dist.get_backend() == "nccl") else "torch"
    eng = Engine(SR, device=torch.cuda.current_device())
    try:
        tracks = np.arange(args.catalog_tracks, dtype=np.uint32)
        if dist:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        # ingest agrees on its own rank-local steps (extraction, the exchange's prepare round); the last
        # agreement covers the index build
        # 256 tracks per extraction call: K1/K2 run 5-14 % faster per audio-second on 2.7 GB power planes than on
        # 1,024 tracks' 10.8 GB (profiles/r05zo_catalog_batch.txt)
        st = _agreed(lambda: ingest_synthetic(eng, tracks, args.catalog_seconds, batch=256, exchange=exchange),
                     "catalog ingest", dist)
        torch.cuda.synchronize()
        if dist:
            dist.barrier()
        wall = time.perf_counter() - t0
        ph = [wall - st.t_synth, st.t_extract - st.t_synth, st.t_exchange, st.t_build, st.t_comm_init, st.t_synth]
        if dist:
            on_dev = dist.get_backend() == "nccl"
            t = torch.tensor(ph, dtype=torch.float64, device="cuda" if on_dev else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            ph = t.tolist()
            per_rank = [None] * world
            dist.all_gather_object(per_rank, int(st.postings_local))
        else:
            per_rank = [int(st.postings_local)]
        ingest, te, tx, tb, ti, tsyn = ph
        stats = eng.index_stats()
        # the replicas checked after the timing: checksums compared across ranks, and on rank 0 every rank's
        # shard against the oracle (a rank-local checker: it reports, it does not raise)
        from aidfp.catalog import replica_check

        replicas = replica_check(eng)
        sp = None
        if rank == 0 and args.shard_parity_tracks > 0:
            try:
                sp = shard_parity(eng, tracks, args.catalog_seconds, world, torch, args.shard_parity_tracks)
            except Exception as exc:
                sp = {"bit_exact": False, "error": f"{type(exc).__name__}: {exc}"}
        audio = args.catalog_tracks * args.catalog_seconds
        gathered = 12 * sum(per_rank)  # bytes of (hash, track, t) every rank receives
        exact = None
        if args.exact_clips > 0:
            try:  # exact_leg agrees on its rank-local part, so every rank takes this branch alike
                exact = exact_leg(eng, args, rank, world, dist, torch)
            except Exception as exc:  # the catalog figure stands on its own
                exact = {"error": f"{type(exc).__name__}: {exc}"}
        return {"value": round(audio / ingest, 1), "unit": "audio-s/s", "tracks": args.catalog_tracks,
                "track_seconds": args.catalog_seconds, "ingest_s": round(ingest, 4),
                "phase_s_max_over_ranks": {"extract": round(te, 4), "allgather": round(tx, 4), "build": round(tb, 4),
                                           "comm_init": round(ti, 4), "synth_generation": round(tsyn, 4)},
                "exchange": st.exchange, "rccl_nranks": st.rccl_nranks or None,
                "postings_per_rank": per_rank, "postings_union": int(st.postings_total),
                "postings_held": int(stats["postings"]), "postings_live": int(stats["live"]),
                "allgather_bytes_per_rank": gathered,
                "allgather_gbs_per_rank": round(gathered / tx / 1e9, 1) if world > 1 and tx > 0 else None,
                "union_equals_sum_of_shards": int(st.postings_total) == sum(per_rank),
                "replicas_identical": replicas["replicas_identical"], "replica_checksums": replicas,
                "shard_parity": sp, "exact_lane": exact}
    finally:
        eng.close()


def exact_leg(eng, args, rank, world, dist, torch) -> dict:
    """BASELINE config 4 against the catalog this leg just built (every rank holds the whole union): per rank
    args.exact_clips 5 s query clips of catalog tracks plus 10 % more from unseen tracks, at SNR 20 dB mixed at
    half gain as the reference corpus's noisy variant (bench_match.py "noise20"), through aid_exact_lane in
    args.exact_batch-clip calls (sub-window fan-out, K1-K5 and the consensus in one call; reference
    app/search/exact.py:70-353). value = all ranks' clips / the slowest rank's GPU time (weak scaling: queries
    are independent). Accuracy in the shape of scripts/eval_exact.py:46-54 (top-1 target 0.98 on clean). An
    untimed second pass of the same clips with events on the K5 kernels gives the match roofline: 8 B per
    posting K5 read + 8 B per query record / the K5 kernels' time (bench_match.py lane())."""
    import types

    from bench_match import CATEGORIES, HBM_PEAK_GBS as PEAK, K5_KERNELS, run_batches

    n_pos = args.exact_clips
    n_neg = n_pos // 10
    n = n_pos + n_neg
    rng = np.random.default_rng(1000 + rank)
    truth = np.concatenate([rng.integers(0, args.catalog_tracks, n_pos),
                            np.arange(n_neg) + args.catalog_tracks + 10**6 + rank * n]).astype(np.uint32)
    starts = np.concatenate([rng.integers(0, int((args.catalog_seconds - 5.0) * SR), n_pos),
                             np.zeros(n_neg, np.int64)]).astype(np.int64)
    clip_n = 5 * SR
    batch = args.exact_batch
    a = types.SimpleNamespace(batch=batch, sr=SR)
    cat = CATEGORIES["noise20"]

    # clips checked against the oracle after the timed region: negatives and positives of the timed calls
    prng = np.random.default_rng(2000 + rank)
    n_chk = min(args.lane_parity_clips, n)
    n_chk_neg = min(n_neg, max(1, n_chk // 8)) if n_chk else 0
    sel = np.sort(np.concatenate([prng.choice(n_pos, min(n_pos, n_chk - n_chk_neg), replace=False),
                                  n_pos + prng.choice(n_neg, n_chk_neg, replace=False)]).astype(np.int64))

    def warm():
        pcm = torch.empty(min(n, batch) * clip_n, dtype=torch.float32, device="cuda")
        w = min(n, batch)  # warm-up at the full call size: the engine's scratch for a full call is sized here
        run_batches(a, eng, truth[:w], starts[:w], w, cat, pcm, clip_n, False)
        torch.cuda.synchronize()
        return pcm

    # agreed, then a barrier: the ranks' timed lanes start together (ranks sharing a GPU in a gloo rehearsal would
    # otherwise time one rank's lane against another rank's catalog build)
    pcm = _agreed(warm, "exact lane (warm-up)", dist)
    if dist is not None:
        dist.barrier()

    def local():
        nonlocal pcm
        res, t_gpu = run_batches(a, eng, truth, starts, n_pos, cat, pcm, clip_n, True, keep=sel)
        kept = res.pop("kept", {})
        # untimed: the same clips again with events on the K5 kernels and the posting counters
        eng.match_stats(reset=True)
        eng.profile_select(None)
        eng.profile_enable(True)
        eng.profile_read(reset=True)
        run_batches(a, eng, truth, starts, n_pos, cat, pcm, clip_n, False)
        prof = eng.profile_read(reset=True)
        eng.profile_enable(False)
        ms = eng.match_stats(reset=True)
        pcm = None  # the clip buffer goes before the parity check's own allocations
        par = lane_parity(eng, truth, starts, n_pos, sel, kept, cat, torch) if len(sel) else None
        return res, t_gpu, prof, ms, par

    res, t_gpu, prof, ms, par = _agreed(local, "exact lane", dist)
    t_max = _max_over_ranks(t_gpu, dist, torch)
    k5_s = sum(prof[k][0] for k in K5_KERNELS if k in prof) * 1e-3
    # algorithmic bytes: every vote reads its 8-B posting ONCE, every query record is read once. The LDS path's
    # second (insert) pass and the global path's per-partition re-reads are the implementation's, not the
    # algorithm's: they are reported as issued_bytes, and the bytes that reach HBM come from the PMC passes
    alg = 8 * ms["votes"] + 8 * ms["records"]
    issued = 8 * ms["posting_reads"] + 2 * ms.get("sig_reads", 0) + 8 * ms["records"]
    pmc_k5, pmc_src = load_pmc_k5()
    roof = {"kernels": list(K5_KERNELS), "bound": "hbm", "unit": "GB/s", "peak": PEAK,
            "algorithmic_bytes": alg, "issued_bytes": issued, "k5_seconds": round(k5_s, 4),
            "achieved": round(alg / k5_s / 1e9, 1) if k5_s else None,
            "frac": round(alg / k5_s / 1e9 / PEAK, 4) if k5_s else None,
            "issued_frac": round(issued / k5_s / 1e9 / PEAK, 4) if k5_s else None,
            "per_kernel_ms": {k: round(prof[k][0], 3) for k in K5_KERNELS if k in prof and prof[k][1]},
            "pmc": pmc_k5, "pmc_source": pmc_src,
            "source": "rank 0, untimed second pass of the same clips with HIP events on the K5 kernels",
            "note": "algorithmic bytes = 8 B x votes (one posting read per vote) + 8 B x query records; issued bytes "
                    "count what the kernels read: the LDS path's two enumerations of 2-B posting signatures (counting, "
                    "insert; the 8-B postings of hot votes are not counted), the global path's 8-B re-reads; the "
                    "vote filters and exact tables stay in LDS / the caches and are not counted; pmc = the K5 "
                    "kernels' HBM bytes per config-4 lane call (2 x FETCH_SIZE + WRITE_SIZE) from the newest "
                    "committed K5 PMC summary"}
    if pmc_k5 and pmc_k5.get("hbm_bytes_per_call") and pmc_k5.get("k5_ms_per_call"):
        roof["traffic_frac"] = round(pmc_k5["hbm_bytes_per_call"] / (pmc_k5["k5_ms_per_call"] * 1e-3) / 1e9 / PEAK, 4)
    return {"value": round(world * n / t_max, 1), "unit": "clips/s", "clips_per_rank": n, "positives_per_rank": n_pos,
            "negatives_per_rank": n_neg, "gpu_s_max_over_ranks": round(t_max, 4),
            "category": "noise20 (SNR 20 dB, gain 0.5)", "rank0": res, "match_stats": ms, "roofline": roof,
            "parity": par, "path": f"aid_exact_lane, {batch} clips per call, 3 sub-windows each"}


def _postings_where(eng, values: np.ndarray, torch, column: int = 0, chunk: int = 1 << 26) -> np.ndarray:
    """The index's stored postings whose `column` (0 hash, 1 track, 2 t) is one of `values`, as a host [m, 3]
    uint32 (hash, track, t) array in storage order. The planes are exported to the device chunk by chunk
    (aid_index_export) and filtered there (a sorted-table lookup per posting), so only the matching postings
    reach the host."""
    q = torch.from_numpy(np.unique(np.asarray(values, dtype=np.uint32)).view(np.int32).copy()).cuda()
    q, _ = torch.sort(q)  # int32 order of the uint32 bits: the same order on both sides of the lookup
    total = eng.index_stats()["postings"]
    n = min(chunk, max(total, 1))
    planes = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3)]
    parts = []
    for o in range(0, total, chunk):
        c = min(chunk, total - o)
        eng.index_export_device(*(p.data_ptr() for p in planes), o, c)
        h = planes[column][:c]
        i = torch.searchsorted(q, h).clamp_(max=len(q) - 1)
        m = q[i] == h
        parts.append(torch.stack([p[:c][m] for p in planes], dim=1).cpu().numpy().view(np.uint32))
    del planes
    return np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros((0, 3), np.uint32))


def _oracle_subset(eng, hashes: np.ndarray, torch) -> np.ndarray:
    """The index's stored postings whose hash is one of `hashes`, sorted for fp_query: only the postings the
    sampled queries can vote through reach the host. Exact for voting: a query touches only postings whose hash
    equals one of its records'."""
    sys.path.insert(0, str(ROOT / "oracle"))
    import oracle as O  # checker only

    sub = _postings_where(eng, hashes, torch, column=0)
    O.lib().fp_index_sort(O._ptr(sub), len(sub))
    return sub


def shard_parity(eng, tracks: np.ndarray, seconds: float, world: int, torch, per_rank: int = 8) -> dict:
    """Rank 0, after the exchange: `per_rank` tracks of every rank's shard, synthesised on
    the host (aidfp.synth, bit-identical to the device generator) and fingerprinted by oracle/fp_oracle.c, must
    appear in this replica exactly as the postings (hash, track, t) the oracle's records give -- the shards that
    crossed the exchange (RCCL under the driver's N > 1 runs) arrived intact. Checker only, after the timing."""
    from concurrent.futures import ThreadPoolExecutor

    from aidfp import synth
    from aidfp.catalog import shard

    sys.path.insert(0, str(ROOT / "oracle"))
    import oracle as O  # checker only

    t0 = time.perf_counter()
    n = int(round(seconds * SR)) & ~1
    picks = []
    for r in range(world):
        sh = np.asarray(shard(tracks, r, world))
        if len(sh):
            picks += [int(x) for x in np.unique(sh[np.linspace(0, len(sh) - 1, min(per_rank, len(sh))).astype(int)])]
    with ThreadPoolExecutor(max(1, min(16, cpu_info()["cores"]))) as pool:
        recs = list(pool.map(lambda t: O.fingerprint(synth.synth(t, 0, n, SR), 512), picks))
    got = _postings_where(eng, np.array(picks, np.uint32), torch, column=1)
    bad = []
    for t, r in zip(picks, recs):
        mine = got[got[:, 1] == t]
        a = np.sort((mine[:, 0].astype(np.uint64)) | (mine[:, 2].astype(np.uint64) << np.uint64(32)))
        if not np.array_equal(a, np.sort(r)):
            bad.append(t)
    return {"tracks_checked": len(picks), "ranks": world, "postings_checked": int(sum(len(r) for r in recs)),
            "bit_exact": not bad, "mismatched_tracks": bad[:8], "seconds": round(time.perf_counter() - t0, 2),
            "oracle": "aidfp.synth (host) + oracle/fp_oracle.c records vs this replica's postings of those tracks"}


def lane_parity(eng, truth, starts, n_pos: int, sel, kept: dict, cat, torch) -> dict:
    """Config 4 pinned at its configured scale: for the sampled clips `sel` of the timed
    exact-lane calls, against the whole catalog index (reference app/audio/fingerprint.py:185-202,
    app/search/exact.py:132-293):
      * window records: the engine's extraction of each sub-window equals oracle/fp_oracle.c's;
      * K5 rows: aid_query over the oracle's window records, on the LDS path, the global path and the automatic
        choice, equals oracle/fp_match.c fp_query over the index's postings with those hashes (every vote the
        query can cast) -- count, track, d, tq_min, tq_max, order;
      * the lane: the rows aid_exact_lane returned in the timed 4096-clip calls equal an all-oracle lane -- the
        oracle's records, fp_query, then aidfp.exact.run_exact_lane's per-window path (the reference's
        sub-window slicing, consensus, MIN_ALIGNED_HASHES, confidence and stable rank, pinned to reference
        vectors by tests/test_glue_parity.py): tracks, aligned counts, binary64 offsets and confidences, order.
    Checker only: runs after the timed region."""
    import asyncio
    import ctypes
    import uuid
    from concurrent.futures import ThreadPoolExecutor

    sys.path.insert(0, str(ROOT / "oracle"))
    import oracle as O  # checker only
    from aidfp import exact as ex
    from aidfp import synth
    from aidfp.engine import exact_windows
    from aidfp.fingerprint import OlafMatch
    from bench_match import _apply

    t0 = time.perf_counter()
    clip_n = 5 * SR
    m = len(sel)
    pcm = torch.empty(m * clip_n, dtype=torch.float32, device="cuda")
    # the sampled clips exactly as the timed calls generated them (same synth arguments, same degradation)
    eng.synth(pcm.data_ptr(), truth[sel], starts[sel], clip_n, noise_a=synth.noise_halfwidth(cat["snr"]), salt=77)
    _apply(pcm, m, clip_n, cat["gain"], cat["band"], SR)
    host = pcm.view(m, clip_n).cpu().numpy()
    del pcm
    _, plan = exact_windows(clip_n, SR)
    # the reference's own slicing of each clip (exact.py:150-160) must be the engine's window plan
    clip_bytes = [host[i].astype("<f4").tobytes() for i in range(m)]
    pieces = []
    for i in range(m):
        for w, (a, b) in enumerate(ex.SUB_WINDOWS):
            pc = ex.extract_pcm_window(clip_bytes[i], a, min(b, ex.pcm_duration_sec(clip_bytes[i], SR)), SR)
            lo, ln = plan[w]
            if pc != host[i, lo:lo + ln].astype("<f4").tobytes():
                return {"clips": m, "rows_bit_exact": False, "lane_equal": False,
                        "error": f"window plan differs from the reference slicing (clip {i}, window {w})"}
            pieces.append(pc)
    wins = [np.frombuffer(pc, dtype="<f4").astype(np.float32) for pc in pieces]
    threads = max(1, min(16, cpu_info()["cores"]))
    with ThreadPoolExecutor(threads) as pool:
        recs = list(pool.map(lambda x: O.fingerprint(x, eng.hop), wins))
    got = eng.extract_host(wins)
    records_ok = all(np.array_equal(g, r) for g, r in zip(got, recs))
    sub = _oracle_subset(eng, np.concatenate([r & np.uint64(0xFFFFFFFF) for r in recs]), torch)
    t_sub = time.perf_counter() - t0

    def fp_rows(r: np.ndarray) -> np.ndarray:
        qh = np.ascontiguousarray((r & np.uint64(0xFFFFFFFF)).astype(np.uint32))
        qt = np.ascontiguousarray((r >> np.uint64(32)).astype(np.uint32))
        out = (O.Row * eng.max_results)()
        k = int(O.lib().fp_query(O._ptr(sub), len(sub), O._ptr(qh), O._ptr(qt), len(r), eng.min_match,
                                 ctypes.addressof(out), eng.max_results))
        return np.array([[x.match_count, x.track, x.d, x.tq_min, x.tq_max] for x in out[:k]],
                        dtype=np.int64).reshape(-1, 5)

    with ThreadPoolExecutor(threads) as pool:
        oracle_rows = list(pool.map(fp_rows, recs))
    paths = {}
    for name, force in (("auto", 0), ("lds", 1), ("global", 2)):
        eng.match_stats(reset=True)
        eng.force("k5_path", force)
        try:
            rows = eng.query(recs)
        finally:
            eng.force("k5_path", 0)
        st = eng.match_stats(reset=True)
        bad = [i for i, (a, b) in enumerate(zip(rows, oracle_rows)) if not np.array_equal(a, b)]
        paths[name] = {"bit_exact": not bad, "mismatched_windows": bad[:8], "queries_lds": st["queries_lds"],
                       "queries_global": st["queries_global"]}
    by_piece = dict(zip(pieces, oracle_rows))
    sec = eng.hop / SR

    async def oracle_query(piece: bytes):
        return [OlafMatch(int(c), tq0 * sec, tq1 * sec, str(uuid.UUID(int=int(tr) + 1)), int(tr), (tq0 + d) * sec,
                          (tq1 + d) * sec) for c, tr, d, tq0, tq1 in by_piece[piece].tolist()]

    lane_bad = []
    for i, q in enumerate(sel):
        want = asyncio.run(ex.run_exact_lane(clip_bytes[i], 10, query=oracle_query, sample_rate=SR))
        r = kept[int(q)]
        same = len(r) == len(want) and all(
            int(x["track"]) == w.track.int - 1 and int(x["aligned_hashes"]) == w.aligned_hashes
            and float(x["offset_seconds"]) == w.offset_seconds and float(x["confidence"]) == w.confidence
            for x, w in zip(r, want))
        if not same:
            lane_bad.append(int(q))
    votes = [int(sum(np.searchsorted(sub[:, 0], h, "right") - np.searchsorted(sub[:, 0], h, "left")
                     for h in (r & np.uint64(0xFFFFFFFF)).astype(np.uint32))) for r in recs[:3]]
    return {"clips": m, "windows": len(recs), "negatives": int(sum(int(q) >= n_pos for q in sel)),
            "records_bit_exact": records_ok, "rows_bit_exact": all(p["bit_exact"] for p in paths.values()),
            "k5_paths": paths, "lane_equal": not lane_bad, "lane_mismatched_clips": lane_bad[:8],
            "index_postings": int(eng.index_stats()["postings"]), "oracle_subset_postings": int(len(sub)),
            "votes_first_windows": votes, "seconds": round(time.perf_counter() - t0, 2),
            "subset_seconds": round(t_sub, 2),
            "oracle": "oracle/fp_oracle.c records, oracle/fp_match.c fp_query over the index postings with the "
                      "windows' hashes, aidfp.exact.run_exact_lane (per-window path) for the consensus"}


def stream_leg(args, rank, world, dist, torch) -> dict:
    """BASELINE config 5 at serving scale: args.stream_count live 48 kHz stereo streams (browser capture,
    AudioRecorder.svelte:86-106) identified continuously against a 16 kHz index of args.stream_tracks x 30 s tracks
    ingested from 44.1 kHz sources through K6 (ffmpeg -ar 16000 of decode.py:41-60). Each stream is a sequence of
    30 s catalog segments, independent noise per channel at SNR 30 dB. Every push hands 2.5 s (one window hop) of
    every stream to aidfp.stream.StreamBank: ONE K6 launch (downmix + 48k -> 16k for all streams) and ONE
    aid_query_windows call (K1-K3 in place over the windows the push completed, then K5). The streams' PCM is
    generated in HBM before the timed region (a push copies its chunk into the bank's history like a network
    receive buffer would); value = stream-seconds of all streams / the pushes' wall time. Latency = per push, the
    call to the rows on the host. top-1 over windows that lie inside one segment. Every rank serves its own
    streams against its own replica (streams are independent)."""
    from aidfp.catalog import ingest_synthetic
    from aidfp.engine import Engine
    from aidfp.stream import StreamBank

    SSR, QSR = 16000, 48000
    S, T = args.stream_count, args.stream_tracks
    seg_s = 30.0
    n_seg = max(1, int(round(args.stream_seconds / seg_s)))
    chunk = int(args.stream_chunk_s * QSR)
    seg = int(seg_s * QSR)
    eng = Engine(SSR, device=torch.cuda.current_device())
    out: dict = {}
    try:
        def build():
            t = time.perf_counter()
            st = ingest_synthetic(eng, np.arange(T, dtype=np.uint32), 30.0, batch=1024, source_sr=44100, local=True)
            torch.cuda.synchronize()
            out["index"] = {"tracks": T, "track_seconds": 30.0, "source_sr": 44100, "index_sr": SSR,
                            "postings": int(st.postings_total), "build_s": round(time.perf_counter() - t, 3)}
            rng = np.random.default_rng(500 + rank)
            seg_tracks = rng.integers(0, T, (S, n_seg)).astype(np.uint32)
            stereo = torch.empty(S, n_seg * seg, 2, dtype=torch.float32, device="cuda")
            tmp = torch.empty(S * n_seg * seg, dtype=torch.float32, device="cuda")
            from aidfp import synth

            noise = synth.noise_halfwidth(30.0)
            for ch in range(2):  # each segment from its track's start, independent noise per channel
                eng.synth(tmp.data_ptr(), seg_tracks.ravel(), np.zeros(S * n_seg, np.int64), seg, noise_a=noise,
                          salt=11 + ch, sample_rate=QSR)
                stereo[:, :, ch] = tmp.view(S, n_seg * seg)
            del tmp
            torch.cuda.synchronize()
            return seg_tracks, stereo

        seg_tracks, stereo = _agreed(build, "stream (index + streams)", dist)
        total_n = stereo.shape[1]

        def run(n_streams, measure: bool, pipelined: bool = False):
            bank = StreamBank(eng, n_streams, stream_sr=QSR)
            bank.timings = []
            eng.match_stats(reset=True)
            lat, res = [], [[] for _ in range(n_streams)]
            pending = None

            def take(r):
                for i in range(n_streams):
                    res[i] += r[i]

            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for a in range(0, total_n, chunk):
                t = time.perf_counter()
                if pipelined:  # submit push N + 1, then collect push N: one push's host work beside the other's kernels
                    p = bank.push_submit(stereo[:n_streams, a:a + chunk])
                    if pending is not None:
                        take(pending.collect())
                    pending = p
                else:
                    take(bank.push(stereo[:n_streams, a:a + chunk]))
                lat.append(time.perf_counter() - t)
            if pending is not None:
                take(pending.collect())
            torch.cuda.synchronize()
            return time.perf_counter() - t0, lat, res, bank.timings, eng.match_stats(reset=True)

        def local():
            run(S, False)  # warm-up: first-use allocations of the bank and the engine's scratch
            run(S, False, True)
            # a serving process moves its start-up objects out of the cyclic collector's reach (gc.freeze), as a
            # long-running server does after start-up: a full collection over this process's ~10^6 objects (torch, the
            # legs before) otherwise lands inside some push (a 70 ms push in r05j, all of it outside the engine calls)
            gc.collect()
            gc.freeze()
            try:
                return run(S, True), run(S, True, True)
            finally:
                gc.unfreeze()

        (wall, lat, res, tim, mst), (wall_p, lat_p, res_p, _, _) = _agreed(local, "stream (pushes)", dist)
        wall_p_max = _max_over_ranks(wall_p, dist, torch)
        same = all(len(a) == len(b) and all(x.start_s == y.start_s and np.array_equal(x.rows, y.rows)
                                            for x, y in zip(a, b)) for a, b in zip(res, res_p))
        lat_p_ms = 1e3 * np.array(lat_p)
        out["pipelined"] = {
            "value": round(world * S * total_n / QSR / wall_p_max, 1), "unit": "stream-audio-s/s",
            "push_call_ms": {f"p{q}": round(float(np.percentile(lat_p_ms, q)), 3) for q in (50, 95, 99)},
            "rows_equal_sync": bool(same),
            "note": "StreamBank.push_submit: each iteration submits push N + 1 (aid_query_windows_submit) and then "
                    "collects push N; a push's windows come back one push later, bit for bit those of push()"}
        worst = int(np.argmax(lat))
        out["slowest_push"] = {"index": worst, "ms": round(1e3 * lat[worst], 3),
                               "append_resample_windows_ms": [round(1e3 * x, 3) for x in tim[worst]]}
        out["match_stats"] = mst
        wall_max = _max_over_ranks(wall, dist, torch)
        hits = inside = windows = 0
        for i in range(S):
            for r in res[i]:
                windows += 1
                a, b = r.start_s, r.start_s + 5.0
                j = int(a // seg_s)
                if j == int((b - 1e-9) // seg_s):
                    inside += 1
                    hits += r.best_track == int(seg_tracks[i, j])
        lat_ms = 1e3 * np.array(lat)
        stream_s = S * total_n / QSR
        out.update({
            "value": round(world * stream_s / wall_max, 1), "unit": "stream-audio-s/s", "streams_per_rank": S,
            "stream_seconds": total_n / QSR, "pushes": len(lat), "chunk_s": args.stream_chunk_s,
            "windows_per_rank": windows, "wall_s_max_over_ranks": round(wall_max, 4),
            "push_latency_ms": {**{f"p{q}": round(float(np.percentile(lat_ms, q)), 3) for q in (50, 95, 99)},
                                "max": round(float(lat_ms.max()), 3), "all": [round(float(x), 3) for x in lat_ms]},
            "realtime_factor_per_gpu": round(stream_s / wall_max, 1),
            "top1_inside_segments": round(hits / max(1, inside), 4), "windows_inside_segments": inside,
            "path": "aidfp.stream.StreamBank: per push one aid_resample_batch_split (48 kHz stereo -> 16 kHz mono, all "
                    "streams, the chunk read in place + each stream's last J - 1 input frames) + one aid_query_windows "
                    "(K1-K3 in place over every completed 5 s / 2.5 s-hop window, K5)",
            "data": "synthetic 30 s catalog segments at 48 kHz, SNR 30 dB per channel, generated in HBM"})
        if rank == 0 and args.stream_parity_streams > 0:
            try:
                out["parity"] = stream_parity(eng, stereo, seg_tracks, res, args.stream_parity_streams, torch)
            except Exception as exc:
                out["parity"] = {"bit_exact": False, "error": f"{type(exc).__name__}: {exc}"}
        del stereo
    finally:
        eng.close()
    return out


def stream_parity(eng, stereo, seg_tracks, res, n_streams: int, torch, max_windows: int = 8) -> dict:
    """The first `n_streams` streams' first windows against the oracle route (checker only, after the timing): the
    host downmix (L + R) * 0.5f and oracle/fp_resample.c's 48k -> 16k (FPSPEC 8), each window fingerprinted by
    oracle/fp_oracle.c and matched by oracle/fp_match.c fp_query over this index's postings with its hashes; the
    rows must equal the ones StreamBank returned."""
    import ctypes

    sys.path.insert(0, str(ROOT / "oracle"))
    import oracle as O  # checker only

    t0 = time.perf_counter()
    QSR, SSR = 48000, eng.sample_rate
    win, hop = int(round(5.0 * SSR)) & ~1, int(round(2.5 * SSR)) & ~1
    nw = min(max_windows, len(res[0]))
    need = ((nw - 1) * hop + win) * QSR // SSR + 4096  # stream frames the first nw windows (and their filter) read
    recs, want = [], []
    for i in range(n_streams):
        x = stereo[i, :min(need, stereo.shape[1])].cpu().numpy()
        mono = ((x[:, 0] + x[:, 1]) * np.float32(0.5)).astype(np.float32)
        y = O.resample(mono, QSR, SSR)
        for j in range(nw):
            s0 = int(round(res[i][j].start_s * SSR))
            recs.append(O.fingerprint(y[s0:s0 + win], eng.hop))
            want.append(res[i][j].rows)
    sub = _oracle_subset(eng, np.concatenate([r & np.uint64(0xFFFFFFFF) for r in recs]), torch)
    bad = []
    for k, r in enumerate(recs):
        qh = np.ascontiguousarray((r & np.uint64(0xFFFFFFFF)).astype(np.uint32))
        qt = np.ascontiguousarray((r >> np.uint64(32)).astype(np.uint32))
        rows = (O.Row * eng.max_results)()
        m = int(O.lib().fp_query(O._ptr(sub), len(sub), O._ptr(qh), O._ptr(qt), len(r), eng.min_match,
                                 ctypes.addressof(rows), eng.max_results))
        got = np.array([[x.match_count, x.track, x.d, x.tq_min, x.tq_max] for x in rows[:m]], np.int64).reshape(-1, 5)
        if not np.array_equal(got, want[k]):
            bad.append(k)
    return {"streams": n_streams, "windows": len(recs), "bit_exact": not bad, "mismatched_windows": bad[:8],
            "seconds": round(time.perf_counter() - t0, 2),
            "oracle": "host downmix + oracle/fp_resample.c + oracle/fp_oracle.c + oracle/fp_match.c fp_query"}


def service_leg(args, rank, world, dist, torch) -> dict:
    """The drop-in path itself, in the reference's deployment shape: `aidfp.fingerprint.olaf_query` (the
    reference's async API, app/audio/fingerprint.py:158-219) through FingerprintService and its query
    coalescer, against a 16 kHz index (the reference's boundary rate, fingerprint.py:10) of
    args.service_tracks x 30 s tracks built as ingest does -- 44.1 kHz sources brought to 16 kHz by K6 (ffmpeg
    -ar 16000, decode.py:41-60). Queries are 5 s of 48 kHz stereo browser capture (AudioRecorder.svelte:86-106;
    independent noise per channel at SNR 20 dB) downmixed and resampled to 16 kHz by K6 (decode.py:41-60, the
    ffmpeg step before olaf_query; untimed), sent as f32le bytes. At each level c, c coroutines on one event
    loop await olaf_query back to back until args.service_requests requests are answered: latency p50/p95/p99,
    qps, the coalescer's mean batch, top-1. Every rank serves its own replica (queries are replicas)."""
    import asyncio
    import tempfile

    from aidfp import fingerprint as fp
    from aidfp import synth
    from aidfp.catalog import ingest_synthetic

    SSR, QSR = 16000, 48000
    T = args.service_tracks
    n_req = args.service_requests
    levels = (1, 16, 64)
    out: dict = {}
    with tempfile.TemporaryDirectory() as db:
        svc = fp.FingerprintService(Path(db), device=torch.cuda.current_device(),
                                    coalesce_workers=args.service_workers, pipeline=bool(args.service_pipeline),
                                    split_min=args.service_split_min, split_parts=args.service_split_parts,
                                    coalesce_window_s=None if args.service_window_ms is None
                                    else args.service_window_ms * 1e-3)
        svc.persist = False

        def build():
            eng = svc._eng()
            t = time.perf_counter()
            st = ingest_synthetic(eng, np.arange(T, dtype=np.uint32), 30.0, batch=1024, source_sr=44100, local=True)
            eng.index_finalize()
            torch.cuda.synchronize()
            out["index"] = {"tracks": T, "track_seconds": 30.0, "source_sr": 44100, "index_sr": SSR,
                            "postings": int(st.postings_total), "build_s": round(time.perf_counter() - t, 3)}
            # the service's name maps for the catalog (what index_track would have recorded per store)
            svc.register_tracks({f"track-{i}": i for i in range(T)})
            rng = np.random.default_rng(77 + rank)
            truth = rng.integers(0, T, n_req).astype(np.uint32)
            starts = rng.integers(0, 25 * QSR, n_req).astype(np.int64)
            nq = 5 * QSR
            noise = synth.noise_halfwidth(20.0)
            lr = [torch.empty(n_req * nq, dtype=torch.float32, device="cuda") for _ in range(2)]
            for k, buf in enumerate(lr):
                eng.synth(buf.data_ptr(), truth, starts, nq, noise_a=noise, salt=31 + k, sample_rate=QSR)
            stereo = torch.stack([x.view(n_req, nq) for x in lr], dim=2).contiguous()  # [req][frame][L, R]
            m = eng.resample_len(nq, QSR, SSR)
            mono = torch.empty(n_req * m + 2, dtype=torch.float32, device="cuda")
            for i in range(n_req):
                eng.resample(stereo[i].data_ptr(), nq, 2, QSR, SSR, mono.data_ptr() + 4 * i * m, m)
            torch.cuda.synchronize()
            host = mono[: n_req * m].view(n_req, m).cpu().numpy()
            return truth, [host[i].astype("<f4").tobytes() for i in range(n_req)]

        truth, reqs = _agreed(build, "service (index + queries)", dist)
        fp.set_service(svc)
        try:
            def run_levels():
                res = {}
                # warm: first-use allocations of the largest batch shape (page-locked staging, the engine's buffers
                # and a second ticket), i.e. the top level's fan-out, untimed; lone queries warmed only batches of one
                # and left those allocations inside the top level's first round
                async def warm():
                    await asyncio.gather(*(fp.olaf_query(reqs[i % n_req]) for i in range(max(levels))))

                for _ in range(3):
                    asyncio.run(warm())
                gc.collect()  # start-up objects out of the cyclic collector's reach, as a serving process does
                gc.freeze()
                for c in levels:
                    lat = np.zeros(n_req)
                    hits = np.zeros(n_req, dtype=bool)
                    nxt = [0]

                    async def client():
                        while nxt[0] < n_req:
                            i = nxt[0]
                            nxt[0] += 1
                            t = time.perf_counter()
                            r = await fp.olaf_query(reqs[i])
                            lat[i] = time.perf_counter() - t
                            hits[i] = bool(r) and r[0].reference_path == f"track-{int(truth[i])}"

                    async def level():
                        await asyncio.gather(*(client() for _ in range(c)))

                    svc._coalescer.batches.clear()
                    svc._coalescer.overlapped = 0
                    t0 = time.perf_counter()
                    asyncio.run(level())
                    wall = time.perf_counter() - t0
                    b = np.array(svc._coalescer.batches)
                    res[str(c)] = {"requests": n_req, "qps": round(n_req / wall, 1),
                                   **{f"p{q}_ms": round(1e3 * float(np.percentile(lat, q)), 3) for q in (50, 95, 99)},
                                   # the same without each client's first request (the level's start-up round)
                                   "p95_ms_after_first_round": round(1e3 * float(np.percentile(lat[c:], 95)), 3),
                                   "mean_batch": round(float(b.mean()), 2) if len(b) else 0.0,
                                   "overlapped_batches": int(svc._coalescer.overlapped),
                                   "top1": round(float(hits.mean()), 4)}
                gc.unfreeze()
                return res

            res = _agreed(run_levels, "service (queries)", dist)
        finally:
            fp.set_service(None)
            svc.close()
    if dist:
        allq = [None] * world
        dist.all_gather_object(allq, {c: v["qps"] for c, v in res.items()})
        out["qps_all_ranks"] = {c: round(sum(q[c] for q in allq), 1) for c in res}
    out["levels_rank0" if dist else "levels"] = res
    worst_p95 = max(v["p95_ms"] for v in res.values())
    out["budgets"] = {"p95_ms_max_over_levels": worst_p95,
                      "eval_exact_p95_ms": 2000.0, "eval_exact_p95_ok": worst_p95 <= 2000.0,
                      "exact_lane_timeout_ms": 3000.0, "p99_within_timeout": max(v["p99_ms"] for v in res.values()) <= 3000.0,
                      "sources": "scripts/eval_exact.py:53 (p95 <= 2000 ms); app/search/orchestrator.py:31 (3 s)"}
    out["pipelined"] = bool(args.service_pipeline)
    out["split_min"] = args.service_split_min if args.service_pipeline else None
    out["split_parts"] = args.service_split_parts if args.service_pipeline else None
    out["coalesce_window_ms"] = round(svc._coalescer.window_s * 1e3, 3)
    out["path"] = ("aidfp.fingerprint.olaf_query -> QueryCoalescer -> "
                   + ("aid_query_pcm_submit / _collect, batch N + 1 submitted before batch N is collected"
                      if args.service_pipeline else "aid_query_pcm")
                   + " (K1-K3 + K5 per coalesced batch); 48 kHz stereo -> 16 kHz by K6 before the call, as ffmpeg in "
                   "decode.py")
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="after the headline also run the checks against the oracle, the CPU baselines, the per-kernel "
                         "breakdown / roofline and the other workloads (fullband, catalog + exact lane, service, "
                         "stream); without it only the headline is measured and the options below are not used")
    ap.add_argument("--dump-outputs", type=Path, default=None, metavar="DIR",
                    help="write the last timed step's results (counts, hash, t1) to DIR/<name>.npy as float64")
    ap.add_argument("--no-cpu", action="store_true", help="skip the cpu_baseline leg")
    ap.add_argument("--settle", type=float, default=0.1,
                    help="seconds of untimed steps after the warmup steps (GPU clock ramp); 0 = none")
    ap.add_argument("--no-fullband", action="store_true", help="skip the full-band workload key")
    ap.add_argument("--no-catalog", action="store_true", help="skip the config-3 catalog leg")
    ap.add_argument("--leg-deadline", type=float, default=float(os.environ.get("AIDFP_BENCH_LEG_DEADLINE", 300)),
                    help="seconds after the headline within which the extra legs must finish; past it the line is "
                         "printed without them and the process ends (0 = no deadline)")
    ap.add_argument("--catalog-tracks", type=int, default=100000)
    ap.add_argument("--catalog-seconds", type=float, default=30.0)
    ap.add_argument("--exact-batch", type=int, default=4096, help="config-4 clips per aid_exact_lane call")
    ap.add_argument("--exact-clips", type=int, default=10000,
                    help="config-4 positive query clips per rank against the catalog leg's index, plus 10 %% "
                         "negatives from unseen tracks (BASELINE configs[3]: 10k; 0 = skip)")
    ap.add_argument("--shard-parity-tracks", type=int, default=8,
                    help="tracks of every rank's shard rank 0 checks against the oracle after the exchange (0 = none)")
    ap.add_argument("--lane-parity-clips", type=int, default=64,
                    help="exact-lane clips per rank checked against the oracle at the catalog's scale (0 = none)")
    ap.add_argument("--no-stream", action="store_true", help="skip the config-5 multi-stream leg")
    ap.add_argument("--stream-count", type=int, default=256, help="live 48 kHz stereo streams per rank (config 5)")
    ap.add_argument("--stream-tracks", type=int, default=10000, help="tracks of the stream leg's 16 kHz index")
    ap.add_argument("--stream-seconds", type=float, default=60.0, help="length of every stream (30 s segments)")
    ap.add_argument("--stream-chunk-s", type=float, default=2.5, help="seconds of every stream per push")
    ap.add_argument("--stream-parity-streams", type=int, default=2,
                    help="streams whose first windows rank 0 checks against the oracle route (0 = none)")
    ap.add_argument("--no-service", action="store_true", help="skip the drop-in service leg")
    ap.add_argument("--service-tracks", type=int, default=10000)
    ap.add_argument("--service-workers", type=int, default=1, help="coalescer dispatcher threads of the service leg")
    ap.add_argument("--service-pipeline", type=int, default=1, choices=(0, 1),
                    help="1: the coalescer submits batch N + 1 before it collects batch N (aid_query_pcm_submit)")
    ap.add_argument("--service-split-min", type=int, default=16,
                    help="pipelined: a batch of at least this many requests gathered with none in flight runs as two "
                         "halves (0: never split)")
    ap.add_argument("--service-window-ms", type=float, default=None,
                    help="the coalescer's collection window after a batch of more than one request (default: the "
                         "service's, 0 when pipelined)")
    ap.add_argument("--service-split-parts", type=int, default=2,
                    help="pipelined: parts of a split batch (= batches in flight at most)")
    ap.add_argument("--service-requests", type=int, default=512)
    ap.add_argument("--dry-run", action="store_true",
                    help="set up the ranks, print one line per rank and exit without touching the GPU (tests)")
    args = ap.parse_args()

    plan = launch_plan(args.gpus, os.environ)
    if plan == "error":
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={os.environ['WORLD_SIZE']}", file=sys.stderr)
        return 2
    if plan == "spawn":
        return spawn_ranks(args.gpus)

    import torch

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.dry_run:
        import torch.distributed as dist

        line = {"dry_run": True, "rank": rank, "world": world, "local_rank": local}
        if world > 1:
            dist.init_process_group("gloo")
            line["world"] = dist.get_world_size()
            for r in range(line["world"]):  # one rank at a time: whole lines on the shared stdout
                if r == rank:
                    print(json.dumps(line), flush=True)
                dist.barrier()
            dist.destroy_process_group()
        else:
            print(json.dumps(line), flush=True)
        return 0
    dist = None
    if world > 1:
        import torch.distributed as dist

        # AIDFP_BENCH_BACKEND=gloo: rehearsal of the N-rank path on fewer GPUs than ranks (ranks share
        # devices round-robin; RCCL refuses two ranks on one GPU). The driver's runs use RCCL, one GPU each.
        backend = os.environ.get("AIDFP_BENCH_BACKEND", "nccl")
        # bounded collectives: every rank-local step is agreed on before the next collective (_agreed), and a
        # hang that slips past that still ends within the timeout instead of holding the node
        timeout = datetime.timedelta(seconds=float(os.environ.get("AIDFP_BENCH_PG_TIMEOUT", "300")))
        if backend == "nccl":
            torch.cuda.set_device(local)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local), timeout=timeout)
        else:
            torch.cuda.set_device(local % torch.cuda.device_count())
            dist.init_process_group(backend, timeout=timeout)
        world = dist.get_world_size()
        rank = dist.get_rank()
    else:
        torch.cuda.set_device(0)

    from aidfp.engine import Engine

    n = SR * CLIP_S
    offs = np.arange(CLIPS + 1, dtype=np.int64) * n
    stream = torch.cuda.current_stream().cuda_stream

    def setup():
        eng = Engine(SR, device=torch.cuda.current_device())
        pcm = torch.empty(CLIPS * n, dtype=torch.float32, device="cuda")
        tracks = np.arange(CLIPS, dtype=np.uint32) + np.uint32(rank * CLIPS)
        eng.synth(pcm.data_ptr(), tracks, np.zeros(CLIPS, np.int64), n)
        run_steps(eng, pcm.data_ptr(), offs, stream, max(0, args.warmup), torch)
        settle_steps = settle(eng, pcm.data_ptr(), offs, stream, args.settle, torch)
        return eng, pcm, settle_steps, int(eng.counts().sum())

    _log(f"headline: world {world}")
    eng, pcm, settle_steps, hashes_per_step = _agreed(setup, "headline (set-up)", dist)
    frames = CLIPS * eng.num_frames(n)

    # events inside the timed region on K1 (stft_power, the dominant kernel) only: every timed launch
    # carries two dispatch-attached events, ~6 us of end-of-kernel work per launch on MI355X
    # (probes/prof_overhead.py). The per-kernel breakdown comes from an untimed pass after the timed region.
    eng.profile_select([0])
    eng.profile_enable(True)
    eng.profile_read(reset=True)
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        eng.extract_device(pcm.data_ptr(), offs, stream)
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    prof = eng.profile_read(reset=True)
    eng.profile_enable(False)
    dumped = None
    if args.dump_outputs is not None:  # the last timed step's results, before anything else runs on the engine
        dumped = _agreed(lambda: dump_outputs(eng, args.dump_outputs, rank), "dump outputs", dist)
    kern = {}
    if args.full:  # an untimed pass of its own with events on every extraction kernel
        kern = {k: {**v, "pass": "untimed breakdown"}
                for k, v in breakdown(eng, pcm.data_ptr(), offs, stream, max(1, min(args.steps, 20)), torch).items()}
    for k, (ms, cnt) in prof.items():  # the timed region's own events win where they exist
        if cnt:
            kern[k] = {"ms_per_launch": ms / cnt, "launches": cnt, "pass": "timed region"}
    elapsed = _max_over_ranks(elapsed, dist, torch)

    audio_s = world * CLIPS * CLIP_S * args.steps
    value = audio_s / elapsed
    roofline = fullband = cpu = par = None  # --full only

    def make_line(catalog, service, stream) -> dict:
        return {
            "metric": METRIC,
            "value": round(value, 1),
            "unit": "audio-s/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "settle_steps": settle_steps,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic (aid_synth: seed-42 integer-exact partials + noise, generated in HBM)",
            "config": {
                "workload": "BASELINE configs[1]: 256 x 10 s 44.1 kHz mono clips, fingerprint extraction per GPU",
                "clips_per_gpu": CLIPS,
                "clip_seconds": CLIP_S,
                "sample_rate": SR,
                "n_fft": 2048,
                "hop": 512,
                "parallelism": f"clip-sharded x{world} (no data-path collective)",
                "process_group": dist.get_backend() if dist else None,
            },
            "realtime_factor_per_gpu": round(value / world, 1),
            "hashes_per_step_per_gpu": hashes_per_step,
            "kernels": kern,
            "roofline": roofline,
            "fullband": fullband,
            "catalog": catalog,
            "service": service,
            "stream": stream,
            "cpu_baseline": cpu,
            "parity": par,
            "full": bool(args.full),
            "dump_outputs": dumped,
        }

    if not args.full:  # a plain run: the headline and nothing else
        del pcm
        eng.close()
        if rank == 0:
            print(json.dumps(make_line(None, None, None)), flush=True)
        if dist:
            dist.destroy_process_group()
        return 0

    roofline = headline_roofline(kern, frames, CLIPS * n, elapsed / args.steps)
    host = None
    if rank == 0:
        host = pcm.view(CLIPS, n).cpu().numpy()
        ref = None
        if world == 1 and not args.no_cpu:
            ref, cpu = cpu_baseline(host)
        # untimed: the batch's hashes (from the last step) against the oracle's
        par = parity(eng, host, ref)
        if world == 1:  # per-bin magnitude criterion (north_star 1e-4 rel) on 4 clips of the batch, untimed
            try:
                par["magnitude"] = magnitude_parity(host, 4, SR)
            except Exception as exc:  # reported, never fatal: the hashes above are the gate
                par["magnitude"] = {"ok": False, "error": f"{type(exc).__name__}: {exc}"}

    _log("headline done; cpu baseline / parity done")
    fullband = None
    if not args.no_fullband:
        fullband = fullband_leg(eng, pcm, offs, stream, args, rank, torch, dist)
    del pcm
    eng.close()
    torch.cuda.empty_cache()

    _log("fullband done")
    # The extra legs (catalog ingest with its RCCL exchange, exact lane, service) run after the headline is measured.
    # A leg that never returns (a collective stuck on some rank) must not cost the headline line: past the deadline a
    # watchdog prints the line with the unfinished legs marked and ends the process (every rank runs the same timer)
    legs = {"catalog": None, "service": None, "stream": None}
    stage = ["catalog"]  # the leg running now, for the watchdog's report
    emitted = threading.Lock()
    finished = threading.Event()

    def emit_line() -> bool:
        if not emitted.acquire(blocking=False):
            return False
        if rank == 0:
            print(json.dumps(make_line(legs["catalog"], legs["service"], legs["stream"])), flush=True)
        return True

    def watchdog():
        if finished.wait(args.leg_deadline):
            return
        hung = [k for k in legs if legs[k] is None and not getattr(args, f"no_{k}")]
        for k in hung:
            legs[k] = {"error": f"deadline: not finished {args.leg_deadline:.0f} s after the headline",
                       "stopped_in": stage[0]}
        _log(f"leg deadline passed in {stage[0]!r} (unfinished: {', '.join(hung)}): printing the line without them "
             "and exiting non-zero")
        if emit_line():
            sys.stdout.flush()
            sys.stderr.flush()
            # a hung leg is a failed run (exit 3), whatever the headline measured; 1 if the headline failed parity
            os._exit(1 if not ok_headline() else 3)

    def ok_headline() -> bool:
        ok = par is None or par["bit_exact"]
        if fullband and "parity" in fullband:
            ok = ok and fullband["parity"]["bit_exact"]
        return ok

    def ok_lane() -> bool:
        """The catalog's own checks, when they ran: the config-4 lane's parity at the catalog's scale
        (catalog.exact_lane.parity), identical replicas on every rank and the shards' postings against the oracle."""
        cat = legs["catalog"] or {}
        if cat.get("replicas_identical") is False:
            return False
        if (cat.get("shard_parity") or {}).get("bit_exact") is False:
            return False
        if ((legs["stream"] or {}).get("parity") or {}).get("bit_exact") is False:
            return False
        if ((legs["stream"] or {}).get("pipelined") or {}).get("rows_equal_sync") is False:
            return False
        lp = (cat.get("exact_lane") or {}).get("parity")
        if not lp:
            return True
        return bool(lp.get("records_bit_exact") and lp.get("rows_bit_exact") and lp.get("lane_equal"))

    if args.leg_deadline > 0 and not (args.no_catalog and args.no_service and args.no_stream):
        threading.Thread(target=watchdog, daemon=True).start()
    catalog = None
    if not args.no_catalog:
        try:
            catalog = catalog_leg(args, rank, world, dist, torch)
        except Exception as exc:  # the headline stands on its own
            catalog = {"error": f"{type(exc).__name__}: {exc}"}
        legs["catalog"] = catalog

    _log("catalog + exact lane done")
    stage[0] = "service"
    service = None
    if not args.no_service:
        try:  # service_leg agrees on its rank-local parts, so every rank takes this branch alike
            service = service_leg(args, rank, world, dist, torch)
        except Exception as exc:  # the headline stands on its own
            service = {"error": f"{type(exc).__name__}: {exc}"}
        legs["service"] = service

    _log("service done")
    stage[0] = "stream"
    stream = None
    if not args.no_stream:
        try:  # stream_leg agrees on its rank-local parts, so every rank takes this branch alike
            stream = stream_leg(args, rank, world, dist, torch)
        except Exception as exc:  # the headline stands on its own
            stream = {"error": f"{type(exc).__name__}: {exc}"}
        legs["stream"] = stream
    _log("stream done")
    if os.environ.get("AIDFP_DUMP_MAPS"):  # diagnostics: the process's mappings, to symbolise an exit-time trace
        Path(os.environ["AIDFP_DUMP_MAPS"]).write_text(Path("/proc/self/maps").read_text())
    finished.set()
    if not emit_line():  # the watchdog printed the line and is ending the process
        threading.Event().wait()
    if dist:
        dist.destroy_process_group()
    if not ok_lane():
        _log("catalog checks FAILED (catalog.replicas_identical, catalog.shard_parity or catalog.exact_lane.parity)")
    return 0 if ok_headline() and ok_lane() else 1


if __name__ == "__main__":
    sys.exit(main())
