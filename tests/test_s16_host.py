"""Host side of the s16 PCM format (no GPU): request parsing, format selection, and the binding table."""

import numpy as np
import pytest

from aidfp import _lib
from aidfp import fingerprint as fp
from aidfp.engine import _fmt_suffix, _host_clips


def test_pcm_parses_s16_and_drops_a_trailing_byte():
    q = np.array([-32768, 32767, -1, 0, 258], dtype="<i2")
    for buf in (q.tobytes(), q.tobytes() + b"\x7f"):
        x = fp.FingerprintService._pcm(buf, "s16")
        assert x.dtype == np.int16 and np.array_equal(x, q)
    assert len(fp.FingerprintService._pcm(b"\x01", "s16")) == 0
    # the default stays f32le, whole samples only
    f = np.array([0.5, -1.0], dtype="<f4")
    x = fp.FingerprintService._pcm(f.tobytes() + b"\x00\x00\x00")
    assert x.dtype == np.float32 and np.array_equal(x, f)


def test_service_parses_in_its_own_format(tmp_path):
    q = np.arange(-3, 4, dtype="<i2")
    s = fp.FingerprintService(tmp_path / "a", pcm_format="s16")
    f = fp.FingerprintService(tmp_path / "b")
    try:
        assert s._clip(q.tobytes() + b"\x00").dtype == np.int16 and len(s._clip(q.tobytes() + b"\x00")) == 7
        assert f._clip(q.tobytes()).dtype == np.float32 and len(f._clip(q.tobytes())) == 3
        assert s._fmt_kw == {"fmt": "s16"} and f._fmt_kw == {}
    finally:
        s.close()
        f.close()


def test_format_selection(tmp_path, monkeypatch):
    monkeypatch.delenv("AIDFP_PCM_FORMAT", raising=False)
    assert fp.resolve_pcm_format() == "f32"
    assert fp.FingerprintService(tmp_path / "a").pcm_format == "f32"
    monkeypatch.setenv("AIDFP_PCM_FORMAT", "s16")
    assert fp.resolve_pcm_format() == "s16"
    assert fp.FingerprintService(tmp_path / "b").pcm_format == "s16"
    assert fp.FingerprintService(tmp_path / "c", pcm_format="f32").pcm_format == "f32"  # the argument wins
    monkeypatch.setenv("AIDFP_PCM_FORMAT", "s24")
    with pytest.raises(ValueError, match="s24"):
        fp.FingerprintService(tmp_path / "d")
    with pytest.raises(ValueError, match="u8"):
        fp.FingerprintService(tmp_path / "e", pcm_format="u8")


def test_engine_format_names_and_dtypes():
    assert _fmt_suffix("f32") == "" and _fmt_suffix("s16") == "_s16"
    with pytest.raises(ValueError):
        _fmt_suffix("s32")
    q = np.array([[1, -2], [3, 4]], np.int16)
    assert _host_clips([q], "s16")[0].dtype == np.int16 and _host_clips([q], "s16")[0].tolist() == [1, -2, 3, 4]
    assert _host_clips([q], "f32")[0].dtype == np.float32  # no dispatch on dtype: an int16 array is cast, as before
    for bad in (q.astype(np.float32), q.astype(np.int32), q.astype(np.uint16)):
        with pytest.raises(ValueError, match="int16"):
            _host_clips([bad], "s16")


def test_every_pcm_entry_point_has_an_s16_twin():
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    twins = [n for n in sig if n.endswith("_s16")]
    assert sorted(twins) == sorted(n + "_s16" for n in ("aid_extract", "aid_query_pcm", "aid_query_pcm_submit",
                                                       "aid_query_windows", "aid_query_windows_submit",
                                                       "aid_exact_lane", "aid_resample", "aid_resample_batch_split"))
    L = _lib.load()
    for n in twins:
        assert sig[n] == sig[n[:-4]] and hasattr(L, n)
