"""Host side of the per-clip relative peak threshold (spec/FPSPEC.md 5.1; no GPU): the ABI keeps its size and
version, the config default is off, the new readout is exported, and the dB conversion rounds once."""

import ctypes

import numpy as np
import pytest

from aidfp import _lib
from aidfp import fingerprint as fp
from aidfp.engine import Engine, top_db_to_rel


def test_config_layout_and_default():
    assert ctypes.sizeof(_lib.AidConfig) == 64
    assert _lib.AidConfig.peak_rel.offset == 28 and _lib.AidConfig.peak_rel.size == 4
    L = _lib.load()
    assert L.aid_abi_version() == 1
    for sr in (16000, 44100):
        cfg = _lib.AidConfig()
        cfg.peak_rel = 0.5  # the default must overwrite it
        assert L.aid_config_default(sr, ctypes.byref(cfg)) == _lib.AID_OK
        assert cfg.peak_rel == 0.0 and cfg.peak_threshold == 4.0
        assert list(cfg.reserved) == [0] * 8


def test_thresholds_readout_is_exported():
    L = _lib.load()
    assert hasattr(L, "aid_result_thresholds")
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    assert sig["aid_result_thresholds"] == (ctypes.c_int, [_lib.P, _lib.P])
    assert L.aid_result_thresholds(None, None) == _lib.AID_ERR_INVALID


def test_top_db_to_rel():
    r = top_db_to_rel(40.0)
    assert np.float32(r).view(np.uint32) == np.float32(1e-4).view(np.uint32)
    assert np.float32(r) == r  # a binary32 value
    for db in (3.0, 17.5, 60.0, 120.0):
        want = np.float32(10.0 ** (-db / 10.0))
        assert np.float32(top_db_to_rel(db)).view(np.uint32) == want.view(np.uint32)
        assert 2.0 ** -60 <= top_db_to_rel(db) < 1.0
    for bad in (0.0, -1.0, -40.0, float("nan")):
        with pytest.raises(ValueError):
            top_db_to_rel(bad)
    with pytest.raises(ValueError):
        top_db_to_rel(200.0)  # 1e-20 < 2^-60


def test_engine_rejects_both_arguments():
    with pytest.raises(ValueError, match="not both"):
        Engine(16000, peak_rel=1e-4, top_db=40.0)
    with pytest.raises(ValueError):
        Engine(16000, top_db=0.0)


def test_service_resolves_the_rule(monkeypatch):
    monkeypatch.delenv("AIDFP_PEAK_TOP_DB", raising=False)
    monkeypatch.delenv("AIDFP_PEAK_FLOOR", raising=False)
    assert fp.resolve_peak_rule() == {}
    assert fp.resolve_peak_rule(40.0) == {"peak_rel": top_db_to_rel(40.0)}
    assert fp.resolve_peak_rule(40.0, 2.0 ** -20) == {"peak_rel": top_db_to_rel(40.0), "peak_threshold": 2.0 ** -20}
    monkeypatch.setenv("AIDFP_PEAK_TOP_DB", "30")
    monkeypatch.setenv("AIDFP_PEAK_FLOOR", "0.5")
    assert fp.resolve_peak_rule() == {"peak_rel": top_db_to_rel(30.0), "peak_threshold": 0.5}
    assert fp.resolve_peak_rule(40.0)["peak_rel"] == top_db_to_rel(40.0)  # the argument wins
    monkeypatch.setenv("AIDFP_PEAK_TOP_DB", "-3")
    with pytest.raises(ValueError):
        fp.resolve_peak_rule()
    with pytest.raises(ValueError):
        fp.resolve_peak_rule(40.0, 0.0)
