"""FingerprintService.exact_batch(speed_search=...) (spec/FPSPEC.md 8.2, 7.1) on the 16 kHz clips of
tests/speed_fixtures.py: off by default and then today's rows; "fallback" leaves a clip the nominal lane identifies
alone and finds the sped ones with their speed; "always" equals the engine call."""

import asyncio

import numpy as np
import pytest

import speed_fixtures as sf
from aidfp import exact as ex
from aidfp import fingerprint as fp
from s16_inputs import synth_q, widen

pytestmark = pytest.mark.gpu


def f32_bytes(x) -> bytes:
    return np.ascontiguousarray(x, "<f4").tobytes()


@pytest.fixture(scope="module")
def svc(tmp_path_factory):
    s = fp.FingerprintService(tmp_path_factory.mktemp("speed_svc"))
    for t in range(sf.N_TRACKS):
        assert s.index_track(f32_bytes(widen(synth_q(t, 0, sf.TRACK_S * sf.SR_E, sf.SR_E))), sf.name_of(t))
    yield s
    s.close()


def summary(ranked):
    return [[(c.track_uuid, c.aligned_hashes, c.offset_seconds, c.confidence, c.speed_pm) for c in r] for r in ranked]


def test_off_by_default(svc, monkeypatch):
    monkeypatch.delenv("AIDFP_SPEED_SEARCH", raising=False)
    clips = sf.clips_16k()
    pcms = [f32_bytes(c.x) for c in clips]
    got = svc.exact_batch(pcms, 5)
    eng = svc._eng()
    want = [ex.candidates_from_rows(r, svc._names, 5) for r in eng.exact_lane([c.x for c in clips])]
    assert summary(got) == summary(want)
    assert summary(svc.exact_batch(pcms, 5, speed_search=None)) == summary(got)
    # only the nominal clip is found, at speed 0
    assert [len(r) > 0 for r in got] == [c.positive and c.speed == 0 for c in clips]
    assert all(c.speed_pm == 0 for r in got for c in r)


def test_fallback(svc, monkeypatch):
    clips = sf.clips_16k()
    pcms = [f32_bytes(c.x) for c in clips]
    nominal = svc.exact_batch(pcms, 5)
    got = svc.exact_batch(pcms, 5, speed_search="fallback", speeds_pm=sf.GRID)
    for c, n, g in zip(clips, nominal, got):
        if not c.positive:
            assert g == [], c.name
            continue
        assert g and g[0].track_uuid.int - 1 == c.track and g[0].aligned_hashes >= ex.STRONG_MATCH_HASHES, c.name
        if c.speed == 0:  # the nominal lane's own answer, kept
            assert summary([g]) == summary([n])
            assert g[0].speed_pm == 0
        else:
            assert abs(g[0].speed_pm - c.speed) <= (0 if c.speed in sf.GRID else 1), c.name
            assert all(x.speed_pm == g[0].speed_pm for x in g)
    # through the async batch entry point, with the environment switch
    monkeypatch.setenv("AIDFP_SPEED_SEARCH", "fallback")
    out = asyncio.run(ex.run_exact_lane_batch(pcms, 5, service=svc, speeds_pm=sf.GRID))
    assert [[(m.track, m.aligned_hashes, m.offset_seconds, m.confidence, m.speed_pm) for m in r] for r in out] == \
        [[(c.track_uuid, c.aligned_hashes, c.offset_seconds, c.confidence, c.speed_pm) for c in r] for r in got]


def test_always_equals_the_engine_call(svc):
    clips = sf.clips_16k()
    pcms = [f32_bytes(c.x) for c in clips]
    got = svc.exact_batch(pcms, 5, speed_search="always", speeds_pm=sf.GRID)
    rows, speeds = svc._eng().exact_lane_speeds([c.x for c in clips], sf.SR_E, 1, sf.GRID)
    want = [ex.candidates_from_rows(r, svc._names, 5) for r in rows]
    for w, pm in zip(want, speeds):
        for c in w:
            c.speed_pm = pm
    assert summary(got) == summary(want)
    for c, g in zip(clips, got):
        assert bool(g) == c.positive, c.name
        if c.positive:
            assert g[0].track_uuid.int - 1 == c.track
    with pytest.raises(ValueError):
        svc.exact_batch(pcms, 5, speed_search="sometimes")
