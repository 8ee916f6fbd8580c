"""Constructed PCM for the K2 / K3 tests at the peak-density bound (spec/FPSPEC.md 5-6): each builder puts peaks
where synthesised music never does -- one in every 16-bin x 8-frame cell (the most FPSPEC 5 allows), at every bin
1..1023, on and just outside the target zone, and on the frames where K3's 1024-frame chunks and their 63-frame
zones begin and end.

Plain numpy, no GPU. Every builder is deterministic and returns (float32 PCM, hop); chunk_edges returns one clip
per length. walk_stats replays FPSPEC 6 over a peak list in plain Python, sharing no code
with the kernel or the oracle, and counts what the K3 tests rest on.

test_dense_fixtures_host.py runs every fixture through the CPU oracle and asserts those counts against the
constants of csrc/aidfp_layout.h and csrc/landmarks.hip."""

import numpy as np

N_FFT = 2048
CHUNK = 1024  # kHashChunk: anchor frames per K3 workgroup
ZONE_DT = 63  # kZoneDT
ZONE_DF = 127  # kZoneDF
FAN = 10  # kFan
_N = np.arange(N_FFT)


def n_samples(F: int, hop: int) -> int:
    """The shortest clip of F frames (FPSPEC 1)."""
    return (F - 1) * hop + N_FFT


def tones(bins, amps, phases) -> np.ndarray:
    """One frame length (2048 samples, float64) of bin-centred sines: sum of amps[i] * sin(2 pi bins[i] n / 2048 +
    phases[i]). Under the periodic Hann window such a tone has power (512 * amp)^2 at its bin, a quarter of that at
    the two bins beside it and nothing further out."""
    bins = np.atleast_1d(np.asarray(bins, dtype=np.float64))
    amps = np.broadcast_to(np.asarray(amps, dtype=np.float64), bins.shape)
    phases = np.broadcast_to(np.asarray(phases, dtype=np.float64), bins.shape)
    return (amps[:, None] * np.sin(2.0 * np.pi * bins[:, None] * _N[None, :] / N_FFT + phases[:, None])).sum(axis=0)


def lattice_bins(k0: int, diag: int = 0, m: int = 0) -> np.ndarray:
    """The bins 1..1023 congruent to k0 + diag * m mod 16: one per 16-bin cell (bin 0 is never a peak)."""
    k = np.arange((k0 + diag * m) % 16, 1024, 16)
    return k[k >= 1]


def lattice(F: int, hop: int, k0: int = 15, diag: int = 0, seed: int = 0, amp: float = 0.01):
    """F frames; every eighth frame f = 8 m begins a 2048-sample burst of tones at lattice_bins(k0, diag, m), with
    amplitudes amp * (1 + 0.5 u) and uniform phases drawn per burst (u, then the phases) from default_rng(seed).
    At hop 2048 frames do not overlap and the peaks are exactly the lattice: 64 (63 in a row of bins = 0 mod 16)
    per aligned 8 frames, FPSPEC 5's bound with equality. At smaller hops the bursts overlap the frames around
    them. Returns (pcm, hop)."""
    rng = np.random.default_rng(seed)
    x = np.zeros(n_samples(F, hop), dtype=np.float64)
    for m in range((F + 7) // 8):
        k = lattice_bins(k0, diag, m)
        u = rng.random(len(k))
        ph = rng.uniform(0.0, 2.0 * np.pi, len(k))
        a = 8 * m * hop
        x[a:a + N_FFT] += tones(k, amp * (1.0 + 0.5 * u), ph)
    return x.astype(np.float32), hop


def noise(F: int, hop: int, seed: int):
    """F frames of unit white noise: about 2.1 peaks per frame, at every bin. Returns (pcm, hop)."""
    return np.random.default_rng(seed).standard_normal(n_samples(F, hop)).astype(np.float32), hop


NOISE_FRAMES = 1201  # two K3 chunks
NOISE3_FRAMES = 2601  # three


def noise3(hop: int, seed: int):
    """The three-chunk variant of noise()."""
    return noise(NOISE3_FRAMES, hop, seed)


def to_s16(x: np.ndarray) -> np.ndarray:
    """round(x * 32768) as int16 (the clip must stay inside the range)."""
    q = np.rint(np.asarray(x, dtype=np.float64) * 32768.0)
    assert q.min() >= -32768 and q.max() <= 32767
    return q.astype(np.int16)


# ---- zone edges ----
# (dt, df, hashes): target = anchor + (dt, df). dt = 0 is a second peak in the anchor's own frame
ZONE_PAIRS = ((63, 127, True), (63, -127, True), (1, 127, True), (1, -127, True),
              (64, 0, False), (1, 128, False), (1, -128, False), (0, 200, False))
# anchor bins of the two groups, one per pair: the middle of the band, then the band's ends (bins 1 and 1023 as
# anchors and as targets)
ZONE_GROUPS = ((500,) * 8, (1, 1023, 896, 128, 1023, 1, 1023, 1))
ZONE_GAP = 128  # frames between a pair's last peak and the next pair's anchor
ZONE_AMP = 0.05


def zone_plan():
    """(pairs, F): pairs = [(t1, k1, t2, k2, hashes)] in time order. The first anchor is at frame 0; the last
    pair hashes and its target is the clip's last frame F - 1."""
    order = [(g, p) for g in range(len(ZONE_GROUPS)) for p in range(len(ZONE_PAIRS))]
    order.append(order.pop(len(ZONE_PAIRS)))  # (group 1, dt 63, bin 1 -> 128) last: an in-zone pair ends the clip
    pairs, t = [], 0
    for g, p in order:
        dt, df, ok = ZONE_PAIRS[p]
        k1 = ZONE_GROUPS[g][p]
        assert 1 <= k1 <= 1023 and 1 <= k1 + df <= 1023
        pairs.append((t, k1, t + dt, k1 + df, ok))
        t += dt + ZONE_GAP
    return pairs, t - ZONE_GAP + 1


def zone_peaks() -> np.ndarray:
    """The designed peak list [n, 2] int32 (t, k), in (t, k) order."""
    pairs, _ = zone_plan()
    pk = sorted({(t1, k1) for t1, k1, _, _, _ in pairs} | {(t2, k2) for _, _, t2, k2, _ in pairs})
    return np.array(pk, dtype=np.int32)


def zone_records() -> np.ndarray:
    """The records FPSPEC 6 gives the design, written out pair by pair: hash | t1 << 32 of every in-zone pair."""
    pairs, _ = zone_plan()
    return np.array([(k1 << 22) | (k2 << 12) | (t2 - t1) | (t1 << 32) for t1, k1, t2, k2, ok in pairs if ok],
                    dtype=np.uint64)


def zone_edges(hop: int = 2048):
    """Isolated anchor / target pairs on and just outside the target zone (ZONE_PAIRS x ZONE_GROUPS), 128 frames
    apart: one tone of amplitude 0.05 and phase 0 per peak (phase 0: a tone at bin 1 then leaves bin 0 empty).
    Returns (pcm, hop). hop must be 2048: a frame per peak, no overlap."""
    assert hop == N_FFT
    pairs, F = zone_plan()
    x = np.zeros(n_samples(F, hop), dtype=np.float64)
    for t, k in zone_peaks().tolist():
        x[t * hop:t * hop + N_FFT] += tones(k, ZONE_AMP, 0.0)
    return x.astype(np.float32), hop


# ---- chunk edges ----
CHUNK_EDGE_FRAMES = (1024, 1025, 1087, 1088, 2048, 2049)
CHUNK_EDGE_BURSTS = (1016, 1080)  # the lattice's 64 tones (k0 = 15)
# single tones: the last anchor frame of chunk 0, the first of chunk 1, the last frame inside and the first outside
# chunk 0's zone; then the same edges of chunk 1 in the longest clips. Their bins lie midway between two lattice
# bins: a tone within 7 frames of a burst is the louder and replaces the burst's two peaks beside it (FPSPEC 5).
# Near the top of the band, so an anchor there has fewer than 10 targets and the fan does not cut the late ones
CHUNK_EDGE_TONES = ((1023, 1015), (1024, 999), (1086, 983), (1087, 967), (2040, 295), (2047, 311), (2048, 327))


def chunk_edges(hop: int = 2048):
    """One clip per length of CHUNK_EDGE_FRAMES, each holding the bursts and tones above whose frame it has.
    Returns (clips, hop)."""
    assert hop == N_FFT
    rng = np.random.default_rng(5)
    k = lattice_bins(15)
    bursts = {f: tones(k, 0.01 * (1.0 + 0.5 * rng.random(len(k))), rng.uniform(0.0, 2.0 * np.pi, len(k)))
              for f in CHUNK_EDGE_BURSTS}
    clips = []
    for F in CHUNK_EDGE_FRAMES:
        x = np.zeros(n_samples(F, hop), dtype=np.float64)
        for f, b in bursts.items():
            if f < F:
                x[f * hop:f * hop + N_FFT] += b
        for f, kk in CHUNK_EDGE_TONES:
            if f < F:
                x[f * hop:f * hop + N_FFT] += tones(kk, ZONE_AMP, 0.0)
        clips.append(x.astype(np.float32))
    return clips, hop


def chunk_edge_peaks(F: int) -> np.ndarray:
    """The designed peak list of the chunk_edges clip of F frames."""
    tn = [(f, k) for f, k in CHUNK_EDGE_TONES if f < F]
    pk = [(f, int(k)) for f in CHUNK_EDGE_BURSTS if f < F for k in lattice_bins(15)
          if not any(abs(f - ft) <= 7 and abs(k - kt) <= 15 for ft, kt in tn)]
    return np.array(sorted(pk + tn), dtype=np.int32)


# ---- the K3 walk, replayed ----
def walk_stats(peaks: np.ndarray, F=None) -> dict:
    """FPSPEC 6 over a (t, k)-ordered peak list, counting what K3 (csrc/landmarks.hip) meets on it:
      anchors[q], list[q]  peaks in chunk q's anchor frames [1024 q, 1024 q + 1024) and in its list, which goes on
                           for 63 more frames
      max_per_frame, max_per_8  most peaks in a frame / in 8 frames aligned to a multiple of 8
      walk_ge64            anchors with an accepted target 64 or more list positions past the anchor
      walk_lt64            anchors with at least one accepted target, all nearer than that
      max_walk             the largest list position of an accepted target (anchor + 1 is position 0)
      fan_cut              anchors whose walk ends at the fan of 10
      skip_df, skip_same   walk steps passed over for |df| > 127 / for lying in the anchor's own frame
      records              accepted targets in all
    F (the clip's frames) defaults to the last peak's frame + 1."""
    pk = np.asarray(peaks).reshape(-1, 2)
    t, k = pk[:, 0].tolist(), pk[:, 1].tolist()
    n = len(t)
    F = (t[-1] + 1 if n else 0) if F is None else F
    nck = (F + CHUNK - 1) // CHUNK
    ta = np.asarray(t, dtype=np.int64)
    st = {"anchors": [int(np.sum((ta >= q * CHUNK) & (ta < (q + 1) * CHUNK))) for q in range(nck)],
          "list": [int(np.sum((ta >= q * CHUNK) & (ta < (q + 1) * CHUNK + ZONE_DT))) for q in range(nck)],
          "max_per_frame": int(np.bincount(ta).max()) if n else 0,
          "max_per_8": int(np.bincount(ta // 8).max()) if n else 0,
          "walk_ge64": 0, "walk_lt64": 0, "max_walk": -1, "fan_cut": 0, "skip_df": 0, "skip_same": 0, "records": 0}
    for i in range(n):
        got, far = 0, False
        for j in range(i + 1, n):
            dt = t[j] - t[i]
            if dt > ZONE_DT or got == FAN:
                break
            if dt <= 0:
                st["skip_same"] += 1
                continue
            if abs(k[j] - k[i]) > ZONE_DF:
                st["skip_df"] += 1
                continue
            got += 1
            pos = j - i - 1
            far = far or pos >= 64
            st["max_walk"] = max(st["max_walk"], pos)
        st["records"] += got
        st["fan_cut"] += got == FAN
        st["walk_ge64"] += far
        st["walk_lt64"] += got > 0 and not far
    return st
