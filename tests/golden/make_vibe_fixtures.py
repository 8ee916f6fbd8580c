"""Capture the reference's chunk -> track aggregation as JSON vectors.

Runs ONLY in the build container: it imports the reference Python from /root/reference (read-only; nothing of it
is copied or shipped). Output: tests/golden/ref_vibe.json -- inputs and outputs of
  app/search/aggregation.py  aggregate_chunk_hits  (:63-138)
over hit lists as Qdrant returns them (score descending). Scores are float32 values stored as floats.

Run: python tests/golden/make_vibe_fixtures.py
"""

from __future__ import annotations

import json
import sys
import uuid
from pathlib import Path

import numpy as np

OUT = Path(__file__).resolve().parent / "ref_vibe.json"
REF = Path("/root/reference/audio-ident-service")


def f32(x) -> float:
    return float(np.float32(x))


def main() -> None:
    sys.path.insert(0, str(REF))
    from app.search.aggregation import ChunkHit, aggregate_chunk_hits

    rng = np.random.default_rng(20261020)
    tracks = [str(uuid.UUID(int=int(rng.integers(1, 2**62)) * 104729)) for _ in range(12)]
    cases = []

    def run(hits, top_k, weight, exclude, note):
        hits = sorted(hits, key=lambda h: -h[1])  # stable: equal scores keep their order
        got = aggregate_chunk_hits([ChunkHit(uuid.UUID(t), s, ci, o) for t, s, ci, o in hits], top_k_per_track=top_k,
                                   diversity_weight=weight,
                                   exact_match_track_id=uuid.UUID(exclude) if exclude else None)
        cases.append({"note": note, "top_k_per_track": top_k, "diversity_weight": weight, "exclude": exclude,
                      "hits": [{"track": t, "score": s, "chunk_index": ci, "offset_sec": o} for t, s, ci, o in hits],
                      "rows": [{"track": str(r.track_id), "final_score": r.final_score, "base_score": r.base_score,
                                "diversity_bonus": r.diversity_bonus, "chunk_count": r.chunk_count} for r in got]})

    def rand_hits(n, n_tracks, quant=None, offsets=None):
        hits = []
        for _ in range(n):
            t = tracks[int(rng.integers(0, n_tracks))]
            s = f32(rng.uniform(0.2, 0.99))
            if quant:
                s = f32(round(s * quant) / quant)  # few distinct scores: ties within and across tracks
            ci = int(rng.integers(0, 40))
            o = float(ci * 5) if offsets is None else float(rng.choice(offsets))
            hits.append((t, s, ci, o))
        return hits

    run([], 3, 0.05, None, "empty list")
    run([], 3, 0.05, tracks[0], "empty list with an excluded track")
    run([(tracks[0], f32(0.75), 0, 0.0)], 3, 0.05, None, "one hit")
    k = 0
    for n, n_tracks in [(1, 1), (5, 2), (12, 3), (20, 1), (33, 5), (50, 12), (50, 7), (50, 2), (41, 9), (17, 12)]:
        for top_k, weight in [(1, 0.0), (3, 0.05), (10, 0.3)]:
            if (k + n) % 3 == 0 and top_k != 3:
                k += 1
                continue
            ex = None
            if k % 4 == 1:
                ex = tracks[0]  # usually present
            elif k % 4 == 3:
                ex = tracks[11] if n_tracks < 12 else str(uuid.UUID(int=12345))  # absent
            run(rand_hits(n, n_tracks, quant=20 if k % 2 else None), top_k, weight, ex, f"random {n} hits / {n_tracks} tracks")
            k += 1
    # a track with more than 5 distinct offsets next to one whose offsets repeat
    hits = [(tracks[0], f32(0.9 - 0.01 * i), i, 5.0 * i) for i in range(9)]
    hits += [(tracks[1], f32(0.88 - 0.01 * i), i, 10.0 * (i % 2)) for i in range(8)]
    hits += [(tracks[2], f32(0.5), 3, 15.0)] * 3
    for top_k, weight in [(1, 0.3), (3, 0.05), (10, 0.0)]:
        run(hits, top_k, weight, None, "more than 5 distinct offsets / repeated offsets")
    run(hits, 3, 0.05, tracks[1], "repeated-offset track excluded")
    # equal final_score between two tracks: first appearance order must survive the sort
    eq = [(tracks[3], f32(0.5), 0, 0.0), (tracks[4], f32(0.75), 0, 0.0), (tracks[5], f32(0.5), 1, 5.0),
          (tracks[4], f32(0.25), 1, 0.0), (tracks[6], f32(0.5), 2, 10.0)]
    run(eq, 3, 0.05, None, "equal final scores (tracks 3, 4, 5, 6)")
    run(eq, 1, 0.0, None, "equal final scores, top_k 1")
    run(eq, 10, 0.3, tracks[5], "equal final scores, one of them excluded")
    run([(tracks[i % 4], f32(0.625), i, 5.0 * (i % 3)) for i in range(24)], 3, 0.05, None, "every score equal")
    OUT.write_text(json.dumps({"source": "MacPhobos/audio-ident reference, captured by tests/golden/make_vibe_fixtures.py",
                               "cases": cases}))
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes): {len(cases)} cases")


if __name__ == "__main__":
    main()
