"""aidfp.exact.select_speed and speed_grid (spec/FPSPEC.md 7.1, 8.2) on constructed rows, no GPU: the host mirror of the
engine's speed selection, which the all-oracle route of tests/test_gpu_speed_lane.py uses. Every expected winner is
worked out by hand from the rule: the largest key (largest aligned_hashes among the rows within max_out), then the
smaller |pm|, then the smaller pm, then the lower position; no rows and speed 0 when every key is 0."""

import uuid

import numpy as np
import pytest

from aidfp import exact as ex
from aidfp.engine import Engine


def rows(*pairs):
    """Engine rows (track, aligned_hashes) in rank order, as exact_lane returns them."""
    r = np.zeros(len(pairs), dtype=Engine.EXACT_DTYPE)
    for i, (t, a) in enumerate(pairs):
        r[i] = (t, a, 0.25 * t, min(a / 20, 1.0))
    return r


def tracks(r):
    return [(int(x["track"]), int(x["aligned_hashes"])) for x in r]


def test_larger_key_wins():
    got, pm = ex.select_speed([rows((1, 12)), rows((2, 9), (1, 30)), rows((1, 29))], (0, 14, -2))
    assert pm == 14 and tracks(got) == [(2, 9), (1, 30)]  # the winner's rows unchanged, not re-ranked
    # the key is the largest aligned_hashes of a variant, not its first row's: confidence saturates at 20
    got, pm = ex.select_speed([rows((5, 21), (6, 20)), rows((7, 20), (8, 40))], (0, 2))
    assert pm == 2 and tracks(got) == [(7, 20), (8, 40)]


def test_ties():
    r = lambda t: rows((t, 25))
    assert ex.select_speed([r(1), r(2), r(3)], (20, -2, 12))[1] == -2  # smaller |pm|
    assert ex.select_speed([r(1), r(2)], (2, -2))[1] == -2  # then the negative one
    assert ex.select_speed([r(1), r(2)], (-2, 2))[1] == -2
    got, pm = ex.select_speed([r(1), r(2), r(3)], (4, -4, -4))  # a duplicated speed: the earlier position
    assert pm == -4 and tracks(got) == [(2, 25)]
    got, pm = ex.select_speed([r(1), r(2), r(3), rows((4, 24))], (6, 6, 6, 0))
    assert pm == 6 and tracks(got) == [(1, 25)]


def test_all_empty():
    got, pm = ex.select_speed([rows(), rows(), rows()], (-2, 0, 2))
    assert len(got) == 0 and pm == 0
    got, pm = ex.select_speed([rows(), rows((3, 8))], (0, 40))
    assert pm == 40 and tracks(got) == [(3, 8)]


def test_key_within_max_out():
    a = rows((1, 20), (2, 20), (3, 90))  # stable ranking by confidence: the 90 sits third
    b = rows((4, 21))
    assert ex.select_speed([a, b], (0, 2))[1] == 0
    got, pm = ex.select_speed([a, b], (0, 2), max_out=2)
    assert pm == 2 and tracks(got) == [(4, 21)]
    got, pm = ex.select_speed([a, rows((4, 19))], (0, 2), max_out=2)  # the winner's rows are cut to max_out
    assert pm == 0 and tracks(got) == [(1, 20), (2, 20)]


def test_other_row_types_and_errors():
    m = [[ex.ExactMatch(uuid.UUID(int=1), 0.5, 1.0, 10)], [ex.ExactMatch(uuid.UUID(int=2), 1.0, 2.0, 33)]]
    got, pm = ex.select_speed(m, (0, -30))
    assert pm == -30 and got[0].aligned_hashes == 33
    c = [[ex.ScoredCandidate(uuid.UUID(int=1), 10, 1.0)], []]
    assert ex.select_speed(c, (2, 0))[1] == 2
    with pytest.raises(ValueError):
        ex.select_speed([rows()], (0, 2))


def test_speed_grid():
    g = ex.speed_grid()
    assert len(g) == 41 and g[0] == -40 and g[-1] == 40 and 0 in g
    assert all(b - a == 2 for a, b in zip(g, g[1:]))
    # every integer speed of the range is within 1 per mille of a grid point
    assert max(min(abs(s - x) for x in g) for s in range(-40, 41)) == 1
    assert ex.speed_grid(-5, 5, 2) == (-4, -2, 0, 2, 4)  # anchored at 0
    assert ex.speed_grid(10, 20, 5) == (10, 15, 20)
    assert ex.speed_grid(0, 0, 1) == (0,)
    for bad in ((-501, 0, 2), (0, 1001, 2), (5, -5, 2), (-4, 4, 0)):
        with pytest.raises(ValueError):
            ex.speed_grid(*bad)
