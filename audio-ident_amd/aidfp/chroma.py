"""The content fingerprint on the GPU -- drop-in for `generate_chromaprint` of audio-ident-service/app/audio/dedup.py
(:53-124, one `fpcalc -raw` subprocess per upload) in the raw-Chromaprint form (spec/FPSPEC.md 11, K11 in
csrc/chroma.hip): 32-bit words from 11025 Hz mono PCM, which `ContentIndex` (aidfp/dedup.py, K7) scans.

PARITY WITH fpcalc IS UNPINNED: the spec is the engine's own, written without fpcalc at hand. Dedup only needs
self-consistency (`_fingerprint_similarity` compares words position by position), so fingerprint the catalog and the
uploads with this engine, and do not mix these fingerprints with a database filled by fpcalc until someone has compared
the two on a machine that has fpcalc.
"""

from __future__ import annotations

import ctypes
from typing import Sequence

import numpy as np

from . import _lib as L
from ._lib import check

RATE = L.AID_CHROMA_RATE
BANDS = L.AID_CHROMA_BANDS
_NP = {"f32": np.float32, "s16": np.int16}


def _p(a: np.ndarray) -> ctypes.c_void_p:
    return ctypes.c_void_p(a.ctypes.data)


def chroma_len(n: int) -> int:
    """Words of a clip of n samples at 11025 Hz (host only)."""
    return int(L.load().aid_chroma_len(int(n)))


def plan(lengths: Sequence[int]):
    """aid_chroma_plan: (word offsets int64[n + 1], frames, words) of clips of these lengths (host only)."""
    ln = np.ascontiguousarray(lengths, dtype=np.int64)
    off = np.zeros(len(ln) + 1, dtype=np.int64)
    nf, nw = ctypes.c_int64(), ctypes.c_int64()
    check(L.load().aid_chroma_plan(_p(ln), len(ln), _p(off), ctypes.byref(nf), ctypes.byref(nw)))
    return off, nf.value, nw.value


def format_fingerprint(words) -> str:
    """uint32 words -> signed decimal, comma separated, as `fpcalc -raw -signed` prints them; the inverse of
    aidfp.dedup.parse_fingerprint."""
    w = np.asarray(words, dtype=np.uint32)
    return ",".join(str(int(v)) for v in w.view(np.int32))


def _upload(a: np.ndarray, dev):
    import torch

    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)  # torch takes writable arrays only


class ChromaPrinter:
    """K11 for batches of clips. Clips are numpy arrays, bytes or torch tensors (host or device) of `fmt` samples,
    interleaved when channels == 2."""

    def __init__(self, engine):
        self.eng = engine

    # ---- input: every clip at 11025 Hz mono, packed, on the device (or the host when nothing has to change) ----
    def _clip(self, c, fmt: str):
        """One clip as a flat torch tensor (device) or numpy array (host) of fmt samples."""
        if hasattr(c, "data_ptr"):
            import torch

            want = torch.float32 if fmt == "f32" else torch.int16
            if c.dtype != want:
                raise ValueError(f"fmt={fmt!r} takes a {want} tensor")
            c = c.reshape(-1).contiguous()
            return c if c.is_cuda else c.numpy()
        if isinstance(c, (bytes, bytearray, memoryview)):
            return np.frombuffer(c, dtype=_NP[fmt])
        return np.ascontiguousarray(c, dtype=_NP[fmt]).reshape(-1)

    def _packed(self, clips, sr: int, fmt: str, channels: int):
        """(pointer, location, fmt, offsets int64[n + 1], keep-alive) of the clips at 11025 Hz mono."""
        import torch

        if fmt not in _NP or channels not in (1, 2):
            raise ValueError("fmt is 'f32' or 's16', channels 1 or 2")
        parts = [self._clip(c, fmt) for c in clips]
        if any(len(p) % channels for p in parts):
            raise ValueError("a stereo clip has an odd number of samples")
        dev = torch.device("cuda", self.eng.device)
        on_dev = [hasattr(p, "data_ptr") for p in parts]
        if any(on_dev):
            torch.cuda.current_stream(dev).synchronize()  # the engine reads them on its own stream
        if int(sr) == RATE and channels == 1:
            ln = [len(p) for p in parts]
            off = np.zeros(len(parts) + 1, dtype=np.int64)
            off[1:] = np.cumsum(ln)
            if not any(on_dev):
                a = np.concatenate(parts) if parts else np.zeros(0, _NP[fmt])
                return _p(a), L.AID_PCM_HOST, fmt, off, a
            t = torch.cat([p if d else _upload(p, dev) for p, d in zip(parts, on_dev)])
            torch.cuda.current_stream(dev).synchronize()
            return ctypes.c_void_p(t.data_ptr()), L.AID_PCM_DEVICE, fmt, off, t
        frames = [len(p) // channels for p in parts]
        ln = [self.eng.resample_len(n, sr, RATE) for n in frames]
        off = np.zeros(len(parts) + 1, dtype=np.int64)
        off[1:] = np.cumsum(ln)
        out = torch.empty(max(1, int(off[-1])), dtype=torch.float32, device=dev)
        srcs = []
        for p, d in zip(parts, on_dev):
            src = p if d else _upload(p, dev)
            if src.data_ptr() % (src.element_size() * channels):  # a stereo frame is read as one word
                src = src.clone()
            srcs.append(src)
        torch.cuda.current_stream(dev).synchronize()  # uploads and copies are complete before the engine reads them
        for src, n, o, m in zip(srcs, frames, off[:-1], ln):
            if m > 0:
                self.eng.resample(src.data_ptr(), n, channels, sr, RATE, out.data_ptr() + 4 * int(o), m, None, fmt)
        keep = srcs
        return ctypes.c_void_p(out.data_ptr()), L.AID_PCM_DEVICE, "f32", off, (out, keep)

    def _fn(self, name: str, fmt: str):
        return getattr(self.eng._lib, name if fmt == "f32" else name + "_pcm16")

    # ---- K11 ----
    def fingerprints_device(self, clips, sr: int = RATE, fmt: str = "f32", channels: int = 1):
        """(words: torch int32 tensor on the device holding the uint32 words of every clip in clip order, word
        offsets int64[n + 1] on the host). Queued on the engine's own stream, which aid_dedup_*_at run on too."""
        import torch

        ptr, loc, f, off, keep = self._packed(clips, sr, fmt, channels)
        woff, _, nw = plan(np.diff(off))
        words = torch.empty(max(1, nw), dtype=torch.int32, device=torch.device("cuda", self.eng.device))
        got = ctypes.c_int64()
        check(self._fn("aid_chroma", f)(self.eng._h, ptr, _p(off), len(off) - 1, loc,
                                        ctypes.c_void_p(words.data_ptr()), _p(woff), nw, L.AID_PCM_DEVICE,
                                        ctypes.byref(got), None))
        assert got.value == nw
        torch.cuda.synchronize(words.device)  # the staged inputs (keep) may go
        return words[:nw], woff

    def fingerprints(self, clips, sr: int = RATE, fmt: str = "f32", channels: int = 1) -> list[np.ndarray]:
        """Per clip its uint32 words (empty below 30031 samples at 11025 Hz)."""
        ptr, loc, f, off, keep = self._packed(clips, sr, fmt, channels)
        woff, _, nw = plan(np.diff(off))
        words = np.zeros(max(1, nw), dtype=np.uint32)
        got = ctypes.c_int64()
        check(self._fn("aid_chroma", f)(self.eng._h, ptr, _p(off), len(off) - 1, loc, _p(words), _p(woff), nw,
                                        L.AID_PCM_HOST, ctypes.byref(got), None))
        assert got.value == nw
        return [words[woff[c]:woff[c + 1]].copy() for c in range(len(off) - 1)]

    def rows(self, clips, sr: int = RATE, fmt: str = "f32", channels: int = 1) -> list[np.ndarray]:
        """Per clip K11a's chroma rows C[frames][12] (float32), for tests and diagnosis."""
        ptr, loc, f, off, keep = self._packed(clips, sr, fmt, channels)
        n = len(off) - 1
        roff = np.zeros(n + 1, dtype=np.int64)
        got = ctypes.c_int64()
        fn = self._fn("aid_chroma_rows", f)
        rc = fn(self.eng._h, ptr, _p(off), n, loc, None, _p(roff), 0, ctypes.byref(got), None)
        if rc != L.AID_OK and got.value == 0:
            check(rc)
        out = np.zeros((max(1, got.value), BANDS), dtype=np.float32)
        check(fn(self.eng._h, ptr, _p(off), n, loc, _p(out), _p(roff), got.value, ctypes.byref(got), None))
        return [out[roff[c]:roff[c + 1]].copy() for c in range(n)]

    def words_from_rows(self, rows: Sequence[np.ndarray], raw_features: bool = False) -> list[np.ndarray]:
        """K11b on host rows: per clip an array [rows][12] of C (a word reads 20 rows), or of F with raw_features
        (smoothing and normalisation skipped, a word reads 16)."""
        parts = [np.ascontiguousarray(r, dtype=np.float32).reshape(-1, BANDS) for r in rows]
        roff = np.zeros(len(parts) + 1, dtype=np.int64)
        roff[1:] = np.cumsum([len(p) for p in parts])
        flat = np.ascontiguousarray(np.concatenate(parts)) if parts and roff[-1] else np.zeros((1, BANDS), np.float32)
        woff = np.zeros(len(parts) + 1, dtype=np.int64)
        got = ctypes.c_int64()
        fn = self.eng._lib.aid_chroma_words
        rc = fn(self.eng._h, _p(flat), _p(roff), len(parts), int(bool(raw_features)), None, _p(woff), 0, ctypes.byref(got))
        if rc != L.AID_OK and got.value == 0:
            check(rc)
        words = np.zeros(max(1, got.value), dtype=np.uint32)
        check(fn(self.eng._h, _p(flat), _p(roff), len(parts), int(bool(raw_features)), _p(words), _p(woff), got.value,
                 ctypes.byref(got)))
        return [words[woff[c]:woff[c + 1]].copy() for c in range(len(parts))]


_default: ChromaPrinter | None = None


def use(printer: ChromaPrinter | None) -> None:
    """The ChromaPrinter `generate_chromaprint` runs on (default: one on aidfp.dedup's shared engine)."""
    global _default
    _default = printer


def _printer() -> ChromaPrinter:
    global _default
    if _default is None:
        from .dedup import _default_engine

        _default = ChromaPrinter(_default_engine())
    return _default


async def generate_chromaprint(pcm_16k_s16le: bytes, duration: float) -> str | None:
    """Drop-in for dedup.py:53-124: the raw fingerprint of 16 kHz s16le mono PCM as signed decimal text, None for
    empty input or when no word results. Like fpcalc's `-length`, only the first int(duration) seconds are read."""
    if not pcm_16k_s16le:
        return None
    x = np.frombuffer(pcm_16k_s16le, dtype=np.int16, count=len(pcm_16k_s16le) // 2)
    x = x[: max(0, int(duration)) * 16000]
    if len(x) == 0:
        return None
    words = _printer().fingerprints([x], sr=16000, fmt="s16")[0]
    return format_fingerprint(words) if len(words) else None
