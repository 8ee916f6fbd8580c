"""The CLAP front end on the GPU -- drop-in for the host side of app/audio/embedding.py (spec/FPSPEC.md 10).

The reference cuts a 48 kHz track into 10 s chunks on the host (`chunk_audio`, embedding.py:101-152) and turns each
into a [1001][64] log-mel image with ClapFeatureExtractor (a float64 rfft per frame in numpy) before its model sees
a sample. Here one call (`aid_logmel`, K10 in csrc/mel.hip) does both for a batch of clips that already sit on the
device (K6 resamples to 48 kHz there) and leaves the images where a device model reads them.

The model (HTSAT + projection) stays with the caller: anything with `get_audio_features(input_features=...)`.
"""

from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Any, Sequence

import numpy as np

from . import _lib as L
from ._lib import AidMelChunk, check

SAMPLE_RATE = 48000
WINDOW = L.AID_MEL_WINDOW
FRAMES = L.AID_MEL_FRAMES
BANDS = L.AID_MEL_BANDS
CHUNK_DTYPE = np.dtype([("clip", "<i4"), ("chunk_index", "<i4"), ("start", "<i8"), ("r", "<i4"), ("rep", "<i4"),
                        ("offset_sec", "<f8"), ("duration_sec", "<f8")])
assert CHUNK_DTYPE.itemsize == ctypes.sizeof(AidMelChunk)
BANKS = {"slaney": L.AID_MEL_BANK_SLANEY, "htk": L.AID_MEL_BANK_HTK}
_NP = {"f32": np.float32, "s16": np.int16}


@dataclass
class AudioChunk:
    """embedding.py:26-33."""

    embedding: list
    offset_sec: float
    chunk_index: int
    duration_sec: float


def _p(a: np.ndarray) -> ctypes.c_void_p:
    return ctypes.c_void_p(a.ctypes.data)


def plan(lengths: Sequence[int], mode: int = L.AID_MEL_ZERO, start: int = 0) -> np.ndarray:
    """aid_mel_plan: the chunks of clips of these lengths, a CHUNK_DTYPE array (host only, no engine)."""
    lib = L.load()
    ln = np.ascontiguousarray(lengths, dtype=np.int64)
    n = ctypes.c_int64()
    check(lib.aid_mel_plan(_p(ln), len(ln), int(mode), int(start), ctypes.byref(n), None, 0))
    meta = np.zeros(max(n.value, 1), dtype=CHUNK_DTYPE)
    check(lib.aid_mel_plan(_p(ln), len(ln), int(mode), int(start), ctypes.byref(n), _p(meta), n.value))
    return meta[: n.value]


def chunk_plan(n_samples: int) -> list[tuple[float, int, float]]:
    """The tuples of `chunk_audio` without the audio: (offset_sec, chunk_index, duration_sec) per chunk."""
    return [(float(c["offset_sec"]), int(c["chunk_index"]), float(c["duration_sec"])) for c in plan([int(n_samples)])]


def _pcm(x, lengths, fmt: str):
    """(pointer, location, clip offsets, clip lengths, keep-alive) of a batch of clips: one numpy array, bytes or
    torch tensor holding the clips back to back (`lengths`; default one clip), or a list of numpy arrays."""
    dt = _NP[fmt]
    if hasattr(x, "data_ptr"):  # torch tensor
        import torch

        want = torch.float32 if fmt == "f32" else torch.int16
        if x.dtype != want:
            raise ValueError(f"fmt={fmt!r} takes a {want} tensor")
        x = x.reshape(-1).contiguous()
        if x.is_cuda:
            torch.cuda.current_stream(x.device).synchronize()  # the engine reads it on its own stream
            ptr, loc, keep, total = ctypes.c_void_p(x.data_ptr()), L.AID_PCM_DEVICE, x, int(x.numel())
        else:
            a = x.numpy()
            ptr, loc, keep, total = _p(a), L.AID_PCM_HOST, a, len(a)
    else:
        if isinstance(x, (bytes, bytearray, memoryview)):
            a = np.frombuffer(x, dtype=dt)
        elif isinstance(x, (list, tuple)):
            parts = [np.ascontiguousarray(c, dtype=dt).reshape(-1) for c in x]
            if lengths is None:
                lengths = [len(c) for c in parts]
            a = np.concatenate(parts) if parts else np.zeros(0, dt)
        else:
            a = np.ascontiguousarray(x, dtype=dt).reshape(-1)
        ptr, loc, keep, total = _p(a), L.AID_PCM_HOST, a, len(a)
    ln = np.ascontiguousarray([total] if lengths is None else lengths, dtype=np.int64)
    if (ln < 0).any() or int(ln.sum()) > total:
        raise ValueError("lengths exceed the samples given")
    off = np.zeros(len(ln), dtype=np.int64)
    off[1:] = np.cumsum(ln)[:-1]
    return ptr, loc, off, ln, keep


class LogMel:
    """ClapFeatureExtractor on the device. bank "slaney" is the extractor's `mel_filters_slaney` (truncation other
    than "fusion"), "htk" its `mel_filters` (fusion); `filters` uploads a [513][64] table of the caller's instead."""

    def __init__(self, engine, bank: str = "slaney", fmin: float = 50.0, fmax: float = 14000.0, filters=None):
        self.eng = engine
        if filters is not None:
            w = np.ascontiguousarray(filters, dtype=np.float32)
            if w.shape != (L.AID_MEL_BINS, BANDS):
                raise ValueError("filters must be [513][64]")
            check(engine._lib.aid_mel_configure(engine._h, L.AID_MEL_BANK_CUSTOM, 0.0, 0.0, _p(w)))
        else:
            check(engine._lib.aid_mel_configure(engine._h, BANKS[bank], float(fmin), float(fmax), None))

    def filters(self) -> np.ndarray:
        w = np.zeros((L.AID_MEL_BINS, BANDS), dtype=np.float32)
        check(self.eng._lib.aid_mel_filters(self.eng._h, _p(w)))
        return w

    def _run(self, pcm, lengths, fmt: str, mode: int, start: int):
        import torch

        ptr, loc, off, ln, keep = _pcm(pcm, lengths, fmt)
        chunks = plan(ln, mode, start)
        dev = keep.device if loc == L.AID_PCM_DEVICE else torch.device("cuda", self.eng.device)
        out = torch.empty((len(chunks), 1, FRAMES, BANDS), dtype=torch.float32, device=dev)
        meta = np.zeros(max(len(chunks), 1), dtype=CHUNK_DTYPE)
        n = ctypes.c_int64()
        s = torch.cuda.current_stream(dev)
        fn = self.eng._lib.aid_logmel if fmt == "f32" else self.eng._lib.aid_logmel_pcm16
        check(fn(self.eng._h, ptr, _p(off), _p(ln), len(ln), loc, mode, int(start), ctypes.c_void_p(out.data_ptr()),
                 len(chunks), L.AID_PCM_DEVICE, _p(meta), ctypes.byref(n), ctypes.c_void_p(s.cuda_stream)))
        if loc == L.AID_PCM_HOST:
            s.synchronize()  # the copy of the caller's samples has left host memory
        assert n.value == len(chunks)
        return out, meta[: n.value]

    def chunks(self, pcm, lengths=None, fmt: str = "f32"):
        """Ingest: every chunk of every clip as chunk_audio cuts them -> (device tensor [C][1][1001][64], CHUNK_DTYPE
        meta array). The kernel runs on torch's current stream, so a model called next reads finished images."""
        return self._run(pcm, lengths, fmt, L.AID_MEL_ZERO, 0)

    def query(self, pcm, start: int = 0, fmt: str = "f32", fusion: bool = False):
        """One query clip -> [1][1][1001][64]: repeatpad when shorter than 10 s, the 10 s from `start` when longer.
        fusion=True: ([1][4][1001][64] expanded view, is_longer=False), the processor's output for inputs <= 10 s."""
        out, meta = self._run(pcm, None, fmt, L.AID_MEL_REPEATPAD, start)
        if not fusion:
            return out
        if len(meta) and int(meta[0]["r"]) == WINDOW and int(meta[0]["rep"]) == 1 and _n_samples(pcm, fmt) > WINDOW:
            raise ValueError("fusion features of inputs longer than 10 s are not supported")
        return out.expand(-1, 4, -1, -1), False


def _n_samples(pcm, fmt: str) -> int:
    if hasattr(pcm, "numel"):
        return int(pcm.numel())
    if isinstance(pcm, (bytes, bytearray, memoryview)):
        return len(pcm) // np.dtype(_NP[fmt]).itemsize
    return int(np.asarray(pcm).size)


def _unwrap(raw):
    """embedding.py:85-93: the return types of get_audio_features across model versions."""
    import torch

    if isinstance(raw, torch.Tensor):
        return raw
    if getattr(raw, "pooler_output", None) is not None:
        return raw.pooler_output
    if hasattr(raw, "last_hidden_state"):
        return raw.last_hidden_state[:, 0, :]
    return raw


_default: LogMel | None = None


def use(logmel: LogMel | None) -> None:
    """The LogMel the drop-ins below run on when neither `processor` nor `model.logmel` is one."""
    global _default
    _default = logmel


def _engine_of(model, processor):
    """The reference passes its ClapProcessor here; it is accepted and ignored unless it is a LogMel."""
    for lm in (processor, getattr(model, "logmel", None), _default):
        if isinstance(lm, LogMel):
            return lm
    raise ValueError("no LogMel: call aidfp.clap.use(LogMel(engine)), set model.logmel, or pass one as `processor`")


def generate_embedding(audio_48k, model: Any, processor: Any = None) -> np.ndarray:
    """embedding.py:62-98 for one query clip. `processor` is accepted for the reference's signature and
    ignored unless it is a LogMel (see use())."""
    import torch

    if not hasattr(audio_48k, "data_ptr"):
        audio_48k = np.asarray(audio_48k, dtype=np.float32)
    feats = _engine_of(model, processor).query(audio_48k)
    with torch.no_grad():
        emb = _unwrap(model.get_audio_features(input_features=feats))
    return emb.squeeze().detach().cpu().numpy()


def generate_chunked_embeddings(pcm_48k_f32le, model: Any, processor: Any = None, batch: int = 64) -> list[AudioChunk]:
    """embedding.py:155-194: every chunk's embedding, the model fed `batch` images at a time."""
    import torch

    feats, meta = _engine_of(model, processor).chunks(pcm_48k_f32le)
    out: list[AudioChunk] = []
    with torch.no_grad():
        for a in range(0, len(meta), int(batch)):
            emb = _unwrap(model.get_audio_features(input_features=feats[a:a + batch])).detach().cpu().numpy()
            emb = emb.reshape(len(meta[a:a + batch]), -1)
            for e, c in zip(emb, meta[a:a + batch]):
                out.append(AudioChunk(e.tolist(), float(c["offset_sec"]), int(c["chunk_index"]), float(c["duration_sec"])))
    return out
