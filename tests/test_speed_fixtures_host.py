"""What the speed-lane GPU tests rely on in tests/speed_fixtures.py, asserted with the oracle alone (no GPU): every
positive clip is found by the all-oracle speed route at its own speed, no sped clip is found at the nominal speed,
and the unseen and the short clip are never found. A clip that does not meet these is replaced in the fixture; the
assertions stay."""

import pytest

import speed_fixtures as sf
from aidfp.exact import STRONG_MATCH_HASHES

POSITIVE = [c for c in sf.all_clips() if c.positive]
SPED = [c for c in POSITIVE if c.speed != 0]
NEGATIVE = [c for c in sf.all_clips() if not c.positive]


def test_fixture_shape():
    names = [c.name for c in sf.all_clips()]
    assert len(set(names)) == len(names)
    assert sorted(c.speed for c in sf.clips_48k() if c.positive) == sorted(c.speed for c in sf.clips_16k() if c.positive)
    assert {c.speed for c in POSITIVE} == {20, -30, 13, 0}
    assert all(c.channels == 2 and c.sr == 48000 for c in sf.clips_48k())
    assert all(c.channels == 1 and c.sr == sf.SR_E for c in sf.clips_16k())
    assert {20, -30, 0} <= set(sf.GRID) and 13 not in sf.GRID and min(abs(13 - g) for g in sf.GRID) == 1
    assert len(sf.records()) == sf.N_TRACKS and all(len(r) > 1000 for r in sf.records())
    assert len({c.track for c in POSITIVE}) == len(POSITIVE)  # every positive clip has a track of its own
    # the short clips give no frame at any speed of the grid
    for c in NEGATIVE:
        if "short" in c.name:
            assert max(len(sf.variant(c, pm)) for pm in sf.GRID) < 2048


@pytest.mark.parametrize("clip", POSITIVE, ids=lambda c: c.name)
def test_positive_clip_found_at_its_speed(clip):
    rows, pm = sf.oracle_route(clip.name)
    assert rows, clip.name
    assert sf.track_of(rows[0]) == clip.track
    assert rows[0].aligned_hashes >= STRONG_MATCH_HASHES
    if clip.speed in sf.GRID:
        assert pm == clip.speed
    else:
        assert abs(pm - clip.speed) <= 1


@pytest.mark.parametrize("clip", SPED, ids=lambda c: c.name)
def test_sped_clip_not_found_at_nominal_speed(clip):
    assert sf.oracle_lane(sf.variant(clip, 0)) == []


@pytest.mark.parametrize("clip", NEGATIVE, ids=lambda c: c.name)
def test_negative_clip_never_found(clip):
    rows, pm = sf.oracle_route(clip.name)
    assert rows == () and pm == 0
    for g in sf.GRID:
        assert sf.oracle_lane(sf.variant(clip, g)) == []
