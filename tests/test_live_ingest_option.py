"""FingerprintService's live_ingest option and the AIDFP_LIVE_INGEST variable (no GPU: the engine is created on first
use): None = the environment, else off; an int = the delta's postings cap; the variable takes 0 / off, on (the default
cap, 2^24 postings) or a number."""

import pytest

from aidfp import fingerprint as fp


@pytest.mark.parametrize("env,want", [(None, 0), ("", 0), ("0", 0), ("off", 0), ("OFF", 0), ("on", 1 << 24),
                                      (" On ", 1 << 24), ("4096", 4096), ("16777216", 1 << 24)])
def test_env(monkeypatch, env, want):
    if env is None:
        monkeypatch.delenv("AIDFP_LIVE_INGEST", raising=False)
    else:
        monkeypatch.setenv("AIDFP_LIVE_INGEST", env)
    assert fp.resolve_live_ingest() == want
    assert fp.resolve_live_ingest(123) == 123  # the argument wins
    assert fp.resolve_live_ingest(0) == 0


@pytest.mark.parametrize("env", ["yes", "-1", "1e6", "on off"])
def test_bad_env(monkeypatch, env):
    monkeypatch.setenv("AIDFP_LIVE_INGEST", env)
    with pytest.raises(ValueError):
        fp.resolve_live_ingest()


def test_bad_argument():
    for bad in (-1, True):
        with pytest.raises(ValueError):
            fp.resolve_live_ingest(bad)


def test_service_takes_the_option(tmp_path, monkeypatch):
    monkeypatch.setenv("AIDFP_LIVE_INGEST", "on")
    a = fp.FingerprintService(tmp_path / "a")
    b = fp.FingerprintService(tmp_path / "b", live_ingest=0)
    c = fp.FingerprintService(tmp_path / "c", live_ingest=5000)
    try:
        assert (a.live_ingest, b.live_ingest, c.live_ingest) == (fp.LIVE_INGEST_DEFAULT_CAP, 0, 5000)
        assert fp.LIVE_INGEST_DEFAULT_CAP == 1 << 24
    finally:
        for s in (a, b, c):
            s.close()
