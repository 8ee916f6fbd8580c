"""The vibe lane on the GPU -- drop-in for the Qdrant side of audio-ident-service.

The reference keeps 512-dim CLAP chunk embeddings in a Qdrant collection (cosine distance, HNSW over int8
scalar quantisation, app/audio/qdrant_setup.py:50-64), asks it for the 50 nearest chunks of a query
(`_query_qdrant`, app/search/vibe.py:164-218) and folds them into track scores (`aggregate_chunk_hits`,
app/search/aggregation.py:63-138). Here the catalog lives in HBM (`VectorIndex`, C ABI aid_vec_*), one call scores
a whole batch of queries against all of it exactly (K9, csrc/vector.hip) and aggregates on the device
(aid_vibe_lane). The arithmetic is pinned by spec/FPSPEC.md 9: the same scores, hits and rows on every run.

The CLAP model stays with the caller: embeddings come in as float vectors (numpy, or torch tensors already on the
device, which are read in place). So do the metadata lookup and `similarity = min(final_score, 1.0)`
(vibe.py:131-159).
"""

from __future__ import annotations

import ctypes
import os
import threading
import uuid
from dataclasses import dataclass
from typing import Sequence

import numpy as np

from . import _lib as L
from ._lib import AidVecHit, AidVibeRow, check

VEC_NO_TRACK = 0xFFFFFFFF
HIT_DTYPE = np.dtype([("entry", "<u4"), ("track", "<u4"), ("chunk_index", "<i4"), ("score", "<f4"), ("offset_sec", "<f8")])
ROW_DTYPE = np.dtype([("track", "<u4"), ("chunk_count", "<i4"), ("final_score", "<f8"), ("base_score", "<f8"),
                      ("diversity_bonus", "<f8")])
assert HIT_DTYPE.itemsize == ctypes.sizeof(AidVecHit) and ROW_DTYPE.itemsize == ctypes.sizeof(AidVibeRow)


@dataclass(frozen=True)
class ChunkHit:
    """aggregation.py:25-39."""

    track_id: uuid.UUID
    score: float
    chunk_index: int
    offset_sec: float


@dataclass(frozen=True)
class TrackResult:
    """aggregation.py:42-60. `top_chunk_scores` stays empty: the lane returns the aggregate, not the chunks."""

    track_id: uuid.UUID
    final_score: float
    base_score: float
    diversity_bonus: float
    chunk_count: int
    top_chunk_scores: tuple = ()


@dataclass(frozen=True)
class Filter:
    """One query's filter (spec/FPSPEC.md 9.2; Qdrant's payload filter acting before the search, not after it). A
    chunk passes if it carries at least one tag of `any_of` (when given), every tag of `all_of`, no tag of `none_of`,
    and belongs to none of `exclude_tracks` (at most 8 caller track ids; one that was never stored is dropped).
    Tags are names of the index's registry (`VectorIndex.tag_bit`) or bit masks, one or several."""

    any_of: object = ()
    all_of: object = ()
    none_of: object = ()
    exclude_tracks: tuple = ()


def _p(a: np.ndarray) -> ctypes.c_void_p:
    return ctypes.c_void_p(a.ctypes.data)


def _vectors(x, dim: int):
    """(pointer, n, location, keep-alive) of [n][dim] float32 vectors: a numpy array (host) or a torch tensor
    (on the device: read in place; on the host: through numpy)."""
    if hasattr(x, "data_ptr"):  # torch tensor
        import torch

        if x.dim() == 1:
            x = x.unsqueeze(0)
        if x.shape[-1] != dim:
            raise ValueError(f"embeddings must be [n][{dim}]")
        if x.is_cuda:
            x = x.to(torch.float32).contiguous()
            torch.cuda.current_stream(x.device).synchronize()  # the engine reads it on its own stream
            return ctypes.c_void_p(x.data_ptr()), int(x.shape[0]), L.AID_PCM_DEVICE, x
        x = x.detach().numpy()
    a = np.ascontiguousarray(np.atleast_2d(np.asarray(x, dtype=np.float32)))
    if a.ndim != 2 or a.shape[1] != dim:
        raise ValueError(f"embeddings must be [n][{dim}]")
    return _p(a), int(a.shape[0]), L.AID_PCM_HOST, a


class VectorIndex:
    """Device-resident catalog of chunk embeddings; keeps the engine id <-> uuid.UUID map as ContentIndex does."""

    PREFILTERS = {"off": 0, "int8": 1}

    def __init__(self, engine, dim: int = 512, prefilter: str | None = None, oversample: int = 4):
        """prefilter: "off" or "int8" (aid_vec_prefilter: an int8 scan with exact rescoring, the same results for
        less bandwidth and 25 % more memory); None reads the environment's AIDFP_VEC_PREFILTER, default off."""
        if prefilter is None:
            prefilter = os.environ.get("AIDFP_VEC_PREFILTER", "off")
        if prefilter not in self.PREFILTERS:
            raise ValueError(f"prefilter must be one of {sorted(self.PREFILTERS)}, not {prefilter!r}")
        self.eng = engine
        self.dim = int(dim)
        self.prefilter = prefilter
        self._ids: list = []   # engine track id -> caller id
        self._num: dict = {}   # caller id -> engine track id
        self._live: set = set()
        self._tags: list = []  # tag name -> bit, by position (at most 64)
        self._lock = threading.Lock()
        check(engine._lib.aid_vec_reset(engine._h, self.dim))
        check(engine._lib.aid_vec_prefilter(engine._h, self.PREFILTERS[prefilter], int(oversample)))

    # -- catalog --
    def _track(self, track_id) -> int:
        t = self._num.get(track_id)
        if t is None:
            t = len(self._ids)
            self._ids.append(track_id)
            self._num[track_id] = t
        return t

    # -- tags (FPSPEC 9.2) --
    MAX_TAGS = 64

    def tag_bit(self, name: str) -> int:
        """The bit mask (one bit set) of tag `name`, registered on first use; the 65th name raises ValueError."""
        with self._lock:
            return self._tag_bit_locked(name)

    def _tag_bit_locked(self, name: str, register: bool = True) -> int:
        if not isinstance(name, str) or not name or "\n" in name:
            raise ValueError(f"a tag name is a non-empty string without line breaks, not {name!r}")
        if name not in self._tags:
            if not register:
                raise KeyError(f"unknown tag {name!r}")
            if len(self._tags) >= self.MAX_TAGS:
                raise ValueError(f"the tag registry holds {self.MAX_TAGS} names; {name!r} would be one more")
            self._tags.append(name)
        return 1 << self._tags.index(name)

    def _mask_locked(self, tags, register: bool) -> int:
        """Names and bit masks, one or an iterable of them, OR-ed into one 64-bit word."""
        if isinstance(tags, (str, int, np.integer)):
            tags = (tags,)
        m = 0
        for t in tags:
            if isinstance(t, str):
                m |= self._tag_bit_locked(t, register)
            else:
                t = int(t)
                if not 0 <= t < 1 << 64:
                    raise ValueError(f"a tag mask is a 64-bit word, not {t}")
                m |= t
        return m

    def upsert_track(self, track_id, embeddings, offsets, chunk_indices=None, tags=()) -> int:
        """Store one track's chunks (replacing the ones it had); returns how many. tags: names (registered on first
        use) or bit masks that every chunk of the track carries, for `Filter`."""
        ptr, n, loc, keep = _vectors(embeddings, self.dim)
        off = np.ascontiguousarray(offsets, dtype=np.float64)
        ci = np.arange(n, dtype=np.int32) if chunk_indices is None else np.ascontiguousarray(chunk_indices, dtype=np.int32)
        if len(off) != n or len(ci) != n:
            raise ValueError("one offset and one chunk index per embedding")
        with self._lock:
            if track_id in self._live:
                self._delete_locked(track_id)
            if n == 0:
                return 0
            mask = self._mask_locked(tags, register=True)
            t = self._track(track_id)
            tr = np.full(n, t, dtype=np.uint32)
            tg = np.full(n, mask, dtype=np.uint64)
            if loc == L.AID_PCM_DEVICE:  # payload columns follow the vectors' location
                import torch

                dev = keep.device
                cols = [torch.from_numpy(a).to(dev) for a in (tr.view(np.int32), ci, off, tg.view(np.int64))]
                torch.cuda.current_stream(dev).synchronize()
                args = [ctypes.c_void_p(c.data_ptr()) for c in cols]
            else:
                args = [_p(tr), _p(ci), _p(off), _p(tg)]
            if mask:
                check(self.eng._lib.aid_vec_add_tagged(self.eng._h, ptr, args[0], args[1], args[2], args[3], n, loc))
            else:
                check(self.eng._lib.aid_vec_add(self.eng._h, ptr, args[0], args[1], args[2], n, loc))
            self._live.add(track_id)
        return n

    def _delete_locked(self, track_id) -> None:
        check(self.eng._lib.aid_vec_remove(self.eng._h, self._num[track_id]))
        self._live.discard(track_id)

    def delete_track(self, track_id) -> bool:
        """Remove every chunk of a track; False if it has none (Qdrant's delete is a no-op then)."""
        with self._lock:
            if track_id not in self._live:
                return False
            self._delete_locked(track_id)
            return True

    def set_tags(self, track_id, tags) -> bool:
        """Replace the tags of every chunk of a stored track (names or bit masks); False if it has no chunk."""
        with self._lock:
            if track_id not in self._live:
                return False
            mask = self._mask_locked(tags, register=True)
            check(self.eng._lib.aid_vec_retag(self.eng._h, self._num[track_id], ctypes.c_uint64(mask)))
            return True

    def _filters(self, filters, nq: int):
        """None, or the AidVecFilter array [nq] of one `Filter` for all queries or of one per query (None = no filter).
        A name that was never registered raises KeyError: no chunk carries it, which is rarely what was meant."""
        if filters is None:
            return None
        if isinstance(filters, Filter):
            filters = [filters] * nq
        if len(filters) != nq:
            raise ValueError("one filter (or None) per query")
        arr = (L.AidVecFilter * max(nq, 1))()
        with self._lock:
            for q, f in enumerate(filters):
                if f is None:
                    continue
                a = arr[q]
                a.any_of = self._mask_locked(f.any_of, register=False)
                a.all_of = self._mask_locked(f.all_of, register=False)
                a.none_of = self._mask_locked(f.none_of, register=False)
                ex = sorted({self._num[t] for t in f.exclude_tracks if t in self._num})
                if len(ex) > L.AID_VEC_MAX_EXCLUDE:
                    raise ValueError(f"a filter excludes at most {L.AID_VEC_MAX_EXCLUDE} tracks")
                a.n_exclude = len(ex)
                for i, t in enumerate(ex):
                    a.exclude[i] = t
        return arr

    def compact(self) -> int:
        n = ctypes.c_int64()
        check(self.eng._lib.aid_vec_compact(self.eng._h, ctypes.byref(n)))
        return n.value

    def counts(self) -> tuple[int, int]:
        """(entries stored, entries live)."""
        n, live, dim = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
        check(self.eng._lib.aid_vec_count(self.eng._h, ctypes.byref(n), ctypes.byref(live), ctypes.byref(dim)))
        return n.value, live.value

    def __len__(self) -> int:
        return self.counts()[1]

    PREFILTER_STATS = ("answered", "fell_back", "w_total", "w_max", "rescored_pairs", "i8_scans")

    def prefilter_stats(self, reset: bool = False) -> dict:
        """aid_vec_prefilter_stats by name: queries answered by the int8 prefilter and queries that fell back to the
        f32 scan, the sum and the largest of |W|, pairs rescored, int8 scan launches."""
        out = (ctypes.c_int64 * len(self.PREFILTER_STATS))()
        check(self.eng._lib.aid_vec_prefilter_stats(self.eng._h, out, len(self.PREFILTER_STATS), int(reset)))
        return dict(zip(self.PREFILTER_STATS, (int(v) for v in out)))

    # -- queries --
    def search_raw(self, embeddings, limit: int = 50, filters=None) -> list[np.ndarray]:
        """Per query a HIT_DTYPE array (engine ids), best first. filters: None, one `Filter` for all queries, or one
        per query (None = no filter); a filtered query's list holds passing chunks only, and may be shorter."""
        ptr, nq, loc, _keep = _vectors(embeddings, self.dim)
        hits = np.zeros((max(nq, 1), limit), dtype=HIT_DTYPE)
        nh = np.zeros(max(nq, 1), dtype=np.int32)
        flt = self._filters(filters, nq) if filters is not None else None
        if flt is None:
            check(self.eng._lib.aid_vec_search(self.eng._h, ptr, nq, loc, int(limit), _p(hits), _p(nh), None))
        else:
            check(self.eng._lib.aid_vec_search_filtered(self.eng._h, ptr, nq, loc, int(limit), flt, _p(hits), _p(nh), None))
        return [hits[q, : nh[q]].copy() for q in range(nq)]

    def search(self, embeddings, limit: int = 50, filters=None) -> list[list[ChunkHit]]:
        """`_query_qdrant` for a batch of queries: per query the `limit` nearest chunks (that pass its filter)."""
        ids = self._ids
        return [[ChunkHit(ids[int(h["track"])], float(h["score"]), int(h["chunk_index"]), float(h["offset_sec"])) for h in hs]
                for hs in self.search_raw(embeddings, limit, filters)]

    def vibe_raw(self, embeddings, max_results: int, exclude=None, threshold: float = 0.60, top_k_per_track: int = 3,
                 diversity_weight: float = 0.05, limit: int = 50, filters=None) -> list[np.ndarray]:
        """Per query a ROW_DTYPE array (engine ids); exclude: per query an engine track id or VEC_NO_TRACK, dropped
        in the aggregation; filters: as in `search_raw`, acting before the selection."""
        ptr, nq, loc, _keep = _vectors(embeddings, self.dim)
        rows = np.zeros((max(nq, 1), max_results), dtype=ROW_DTYPE)
        nr = np.zeros(max(nq, 1), dtype=np.int32)
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint32)
        if filters is None:
            check(self.eng._lib.aid_vibe_lane(self.eng._h, ptr, nq, loc, int(limit), int(top_k_per_track),
                                              float(diversity_weight), None if ex is None else _p(ex), float(threshold),
                                              int(max_results), _p(rows), _p(nr), None))
        else:
            check(self.eng._lib.aid_vibe_lane_filtered(self.eng._h, ptr, nq, loc, int(limit), int(top_k_per_track),
                                                       float(diversity_weight), self._filters(filters, nq),
                                                       None if ex is None else _p(ex), float(threshold),
                                                       int(max_results), _p(rows), _p(nr), None))
        return [rows[q, : nr[q]].copy() for q in range(nq)]

    def vibe(self, embeddings, max_results: int, exact_match_track_ids: Sequence | None = None, threshold: float = 0.60,
             top_k_per_track: int = 3, diversity_weight: float = 0.05, limit: int = 50, filters=None,
             exclude_in_scan: bool = False) -> list[list[TrackResult]]:
        """Steps 3-6 of run_vibe_lane (vibe.py:100-129) for a batch of query embeddings, in one engine call.
        exact_match_track_ids: per query the track to leave out, or None. By default it is dropped from the
        aggregated rows after its chunks have taken their slots among the `limit` hits, as the reference does; with
        exclude_in_scan its chunks are filtered out before the selection, so the slots go to other tracks."""
        ex = None
        if exact_match_track_ids is not None:
            if exclude_in_scan:
                nq = len(exact_match_track_ids)
                per_q = [filters] * nq if filters is None or isinstance(filters, Filter) else list(filters)
                if len(per_q) != nq:
                    raise ValueError("one filter (or None) per query")
                filters = []
                for f, t in zip(per_q, exact_match_track_ids):
                    if t is not None:
                        f = Filter(exclude_tracks=(t,)) if f is None else \
                            Filter(f.any_of, f.all_of, f.none_of, tuple(f.exclude_tracks) + (t,))
                    filters.append(f)
            else:
                ex = [VEC_NO_TRACK if t is None else self._num.get(t, VEC_NO_TRACK) for t in exact_match_track_ids]
        ids = self._ids
        return [[TrackResult(ids[int(r["track"])], float(r["final_score"]), float(r["base_score"]),
                             float(r["diversity_bonus"]), int(r["chunk_count"])) for r in rows]
                for rows in self.vibe_raw(embeddings, max_results, ex, threshold, top_k_per_track, diversity_weight, limit,
                                          filters)]

    # -- persistence --
    def save(self, path: str) -> None:
        """The catalog to `path` (AIDFPVC1) and the id map beside it (`path`.ids, one id per line)."""
        check(self.eng._lib.aid_vec_save(self.eng._h, str(path).encode()))
        with open(str(path) + ".ids", "w") as f:
            f.write("\n".join(str(i) for i in self._ids))
        tags_path = str(path) + ".tags"  # the tag registry, one name per line in bit order; none = no file
        if self._tags:
            with open(tags_path, "w") as f:
                f.write("\n".join(self._tags))
        elif os.path.exists(tags_path):
            os.remove(tags_path)

    def load(self, path: str, parse=uuid.UUID) -> None:
        with open(str(path) + ".ids") as f:
            ids = [parse(s) for s in f.read().split("\n") if s]
        tags = []
        if os.path.exists(str(path) + ".tags"):
            with open(str(path) + ".tags") as f:
                tags = [s for s in f.read().split("\n") if s]
        if len(tags) > self.MAX_TAGS or len(set(tags)) != len(tags):
            raise ValueError(f"{path}.tags: at most {self.MAX_TAGS} distinct tag names")
        check(self.eng._lib.aid_vec_load(self.eng._h, str(path).encode()))
        n, live, dim = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
        check(self.eng._lib.aid_vec_count(self.eng._h, ctypes.byref(n), ctypes.byref(live), ctypes.byref(dim)))
        with self._lock:
            self.dim = dim.value
            self._ids = ids
            self._tags = tags
            self._num = {t: i for i, t in enumerate(ids)}
            self._live = set()
            if live.value:  # the tracks that still have a live entry: ask the catalog's own save file
                hdr = 24
                tiles = (n.value + 31) // 32
                with open(path, "rb") as f:
                    f.seek(hdr + tiles * 32 * self.dim * 4)
                    tr = np.frombuffer(f.read(4 * n.value), dtype="<u4")
                    f.seek(hdr + tiles * 32 * self.dim * 4 + 16 * n.value)
                    dead = np.frombuffer(f.read(n.value), dtype=np.uint8)
                self._live = {ids[int(t)] for t in np.unique(tr[dead == 0])}


def aggregate_hits(engine, hit_lists: Sequence[np.ndarray], top_k_per_track: int = 3, diversity_weight: float = 0.05,
                   exclude=None, threshold: float = -np.inf, max_out: int | None = None) -> list[np.ndarray]:
    """aid_vec_aggregate: `aggregate_chunk_hits` over host hit lists (HIT_DTYPE arrays, engine ids), as the dedup
    lane's pairs call replays reference fixtures without a search."""
    nq = len(hit_lists)
    hoff = np.zeros(nq + 1, dtype=np.int64)
    if nq:
        hoff[1:] = np.cumsum([len(h) for h in hit_lists])
    hits = np.concatenate([np.asarray(h, dtype=HIT_DTYPE) for h in hit_lists]) if hoff[-1] else np.zeros(1, HIT_DTYPE)
    hits = np.ascontiguousarray(hits)
    if max_out is None:
        max_out = max(1, max((len(h) for h in hit_lists), default=1))
    rows = np.zeros((max(nq, 1), max_out), dtype=ROW_DTYPE)
    nr = np.zeros(max(nq, 1), dtype=np.int32)
    ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint32)
    check(engine._lib.aid_vec_aggregate(engine._h, _p(hits), _p(hoff), nq, int(top_k_per_track), float(diversity_weight),
                                        None if ex is None else _p(ex), float(threshold), int(max_out), _p(rows), _p(nr)))
    return [rows[q, : nr[q]].copy() for q in range(nq)]


# ---- async drop-ins with the reference's names and argument order: `client` is a VectorIndex ----

async def upsert_track_embeddings(client: VectorIndex, track_id: uuid.UUID, chunks, metadata: dict | None = None) -> int:
    """qdrant_setup.py:81-156. chunks: objects with .embedding, .offset_sec and .chunk_index (AudioChunk);
    the metadata payload stays in the caller's database."""
    if not chunks:
        return 0
    emb = np.stack([np.asarray(c.embedding, dtype=np.float32) for c in chunks])
    return client.upsert_track(track_id, emb, [float(c.offset_sec) for c in chunks], [int(c.chunk_index) for c in chunks])


async def delete_track_embeddings(client: VectorIndex, track_id: uuid.UUID) -> None:
    """qdrant_setup.py:159-181."""
    client.delete_track(track_id)


async def query_chunks(client: VectorIndex, embedding, limit: int = 50) -> list[ChunkHit]:
    """Stands in for `_query_qdrant` (vibe.py:164-218): the `limit` nearest chunks of one embedding."""
    return client.search(np.asarray(embedding, dtype=np.float32)[None, :], limit)[0]
