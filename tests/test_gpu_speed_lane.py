"""aid_exact_lane_speeds (spec/FPSPEC.md 8.2, 7.1) on the fixture of tests/speed_fixtures.py against the all-oracle
route: per speed oracle.resample, aidfp.exact's lane over the oracle's fingerprint and matcher, then
aidfp.exact.select_speed. Track, aligned_hashes, binary64 offset_seconds, confidence, row order and the chosen speed
are compared, for f32 and s16 clips, host and device PCM, one clip group and one group per clip. The fixture's own
preconditions (every sped clip is found at its speed by the oracle route and not at the nominal speed) are
tests/test_speed_fixtures_host.py's."""

import numpy as np
import pytest
import torch

import speed_fixtures as sf
from aidfp.engine import Engine

pytestmark = pytest.mark.gpu
SETS = {"48k": sf.clips_48k, "16k": sf.clips_16k}


@pytest.fixture(scope="module")
def eng():
    e = Engine(sf.SR_E)
    assert (e.min_match, e.max_results, e.hop) == (sf.MIN_MATCH, sf.MAX_RESULTS, sf.HOP)
    for t, r in enumerate(sf.records()):
        e.index_add_records(t, r)
    e.index_finalize()
    yield e
    e.close()


def samples(clip, fmt):
    return clip.q if fmt == "s16" else clip.x


def run_lane(eng, clips, fmt, where, grid=sf.GRID):
    sr, ch = clips[0].sr, clips[0].channels
    if where == "host":
        return eng.exact_lane_speeds([samples(c, fmt) for c in clips], sr, ch, grid, sf.MAX_OUT, fmt=fmt)
    # one device buffer, the clips back to back from frame 1 on (so some start at an odd sample)
    frames = [len(c.q) for c in clips]
    offsets = np.cumsum([1] + frames).astype(np.int64)
    host = np.zeros((int(offsets[-1]),) + clips[0].q.shape[1:], np.int16 if fmt == "s16" else np.float32)
    for c, o in zip(clips, offsets):
        host[o:o + len(c.q)] = samples(c, fmt)
    dev = torch.from_numpy(host).cuda()
    return eng.exact_lane_speeds(None, sr, ch, grid, sf.MAX_OUT, pcm_ptr=dev.data_ptr(), offsets=offsets, fmt=fmt)


def check_against_oracle(clips, rows, speeds):
    assert len(rows) == len(speeds) == len(clips)
    for c, r, pm in zip(clips, rows, speeds):
        want, want_pm = sf.oracle_route(c.name)
        assert pm == want_pm, (c.name, pm, want_pm)
        assert sf.same_rows(r, want), (c.name, r, want)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("fmt", ["f32", "s16"])
@pytest.mark.parametrize("which", ["48k", "16k"])
def test_equals_oracle_route(eng, which, fmt, where):
    clips = SETS[which]()
    rows, speeds = run_lane(eng, clips, fmt, where)
    check_against_oracle(clips, rows, speeds)


@pytest.mark.parametrize("which", ["48k", "16k"])
def test_one_group_per_clip(eng, which):
    clips = SETS[which]()
    eng.force("speed_group", 1)  # every clip's variants exceed it: no two clips share a group
    try:
        rows, speeds = run_lane(eng, clips, "s16", "device")
    finally:
        eng.force("speed_group", 0)
    check_against_oracle(clips, rows, speeds)
    # and a budget that holds two of the long clips' variants but not three
    two = sum(eng.speed_len(len(clips[0].q), clips[0].sr, pm) for pm in sf.GRID) * 2 + 100
    eng.force("speed_group", two)
    try:
        rows, speeds = run_lane(eng, clips, "f32", "host")
    finally:
        eng.force("speed_group", 0)
    check_against_oracle(clips, rows, speeds)


def test_top1_of_every_positive_clip(eng):
    """What the feature is for: every clip of a catalog track, played up to 3 % fast or slow, is identified, with
    its speed. The nominal lane alone finds none of the sped ones."""
    for which in SETS:
        clips = SETS[which]()
        rows, speeds = run_lane(eng, clips, "s16", "host")
        for c, r, pm in zip(clips, rows, speeds):
            if c.positive:
                assert len(r) and int(r[0]["track"]) == c.track, c.name
                assert int(r[0]["aligned_hashes"]) >= 20
                assert abs(pm - c.speed) <= (0 if c.speed in sf.GRID else 1), (c.name, pm)
            else:
                assert len(r) == 0 and pm == 0, c.name
    sped = [c for c in sf.clips_16k() if c.positive and c.speed]
    assert all(len(r) == 0 for r in eng.exact_lane([c.q for c in sped], sf.MAX_OUT, fmt="s16"))


@pytest.mark.parametrize("fmt", ["f32", "s16"])
def test_speed_zero_at_the_engine_rate_is_the_lane(eng, fmt):
    clips = sf.clips_16k()
    want = eng.exact_lane([samples(c, fmt) for c in clips], sf.MAX_OUT, fmt=fmt)
    rows, speeds = run_lane(eng, clips, fmt, "host", grid=(0,))
    assert any(len(w) for w in want)
    for c, r, w, pm in zip(clips, rows, want, speeds):
        assert np.array_equal(r, w), c.name
        assert pm == 0
    rows, speeds = run_lane(eng, clips, fmt, "device", grid=(0,))
    assert all(np.array_equal(r, w) for r, w in zip(rows, want)) and set(speeds) == {0}


def test_errors_and_empty(eng):
    from aidfp import _lib
    from aidfp._lib import EngineError

    assert eng.exact_lane_speeds([], 48000, 2, sf.GRID) == ([], [])
    x = sf.clips_16k()[0].x
    for kw in (dict(speeds_pm=()), dict(speeds_pm=(0, 1001)), dict(sr_in=2147484)):
        a = dict(dict(sr_in=sf.SR_E, channels=1, speeds_pm=(0,)), **kw)
        with pytest.raises(EngineError) as err:
            eng.exact_lane_speeds([x], a["sr_in"], a["channels"], a["speeds_pm"], sf.MAX_OUT)
        assert err.value.code == _lib.AID_ERR_INVALID, kw
    with pytest.raises((EngineError, ValueError)):
        eng.exact_lane_speeds([x[:99]], sf.SR_E, 3, (0,))
    with pytest.raises(ValueError):
        eng.exact_lane_speeds([x[:101]], 48000, 2, (0,))  # half a stereo frame
    with pytest.raises(ValueError):
        eng.exact_lane_speeds([x], sf.SR_E, 1, (0,), fmt="s16")  # float samples are not narrowed silently
    # the engine still answers after the refused calls
    rows, speeds = eng.exact_lane_speeds([sf.clips_16k()[3].x], sf.SR_E, 1, (0,), sf.MAX_OUT)
    assert int(rows[0][0]["track"]) == 7 and speeds == [0]
