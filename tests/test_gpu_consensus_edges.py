"""K8b `exact_consensus` (csrc/exact.hip) on a constructed index (consensus_fixtures.py; its preconditions:
test_consensus_fixtures_host.py): totals at 7 and 8 aligned hashes, halved and not, medians in every window order,
confidence ties cut by max_out, a clip that fills the 768 staged rows with one window cut at max_results, and the
whole-clip, one-window, two-window and empty clip shapes in one call. The expectation is the all-oracle lane
(consensus_fixtures.expected: oracle/fp_match.c rows of the oracle's own records, then aidfp.exact's consensus and
ranking), never the engine's per-window path. Every comparison is equality: tracks, aligned_hashes, the bits of
offset_seconds and confidence, the order and the row count."""

import numpy as np
import pytest

import consensus_fixtures as F
from aidfp.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    return F.batch()


@pytest.fixture(scope="module")
def eng(B):
    e = Engine(F.SR, min_match=F.MIN_MATCH, max_results=F.MAX_RESULTS)
    assert e.hop == F.HOP
    h, tr, t = (np.ascontiguousarray(B.postings[:, c]) for c in range(3))
    e.index_add_postings(h.ctypes.data, tr.ctypes.data, t.ctypes.data, len(B.postings), device=False)
    e.index_finalize()
    yield e
    e.close()


def assert_rows_equal(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    assert got["track"].tolist() == want["track"].tolist(), what
    assert got["aligned_hashes"].tolist() == want["aligned_hashes"].tolist(), what
    for f in ("offset_seconds", "confidence"):
        assert np.array_equal(got[f].view(np.uint64), want[f].view(np.uint64)), (what, f)


def cuts(B):
    out = {1, 3, F.MAX_STAGED}
    for name in ("cases", "bulk"):
        k = len(F.expected(B.clip(name), F.MAX_STAGED))
        out |= {k - 1, k, k + 1}
    return sorted(out)


def test_window_records_equal_the_oracles(eng, B):
    """What the construction stands on: the engine's records of every sent window are the oracle's."""
    wins = [c.pcm[lo:lo + ln] for c in B.clips for lo, ln in c.windows]
    want = [r for c in B.clips for r in c.records]
    got = eng.extract_host(wins)
    assert len(got) == len(want) == 10
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), i


def test_lane_equals_the_oracle_lane_at_every_cut(eng, B):
    pcm = [c.pcm for c in B.clips]
    ks = cuts(B)
    assert len(ks) == 9
    for max_out in ks:
        lane = eng.exact_lane(pcm, max_out)
        assert len(lane) == len(B.clips)
        for c, got in zip(B.clips, lane):
            assert_rows_equal(got, F.expected(c, max_out), (c.name, max_out))
    full = eng.exact_lane(pcm)  # the default: every candidate the consensus can keep
    assert [len(r) for r in full] == [len(F.expected(c, F.MAX_STAGED)) for c in B.clips]
    assert len(full[2]) > 64 and len(full[1]) == 0


def test_lane_gather_gives_the_same_rows(eng, B):
    pcm = [c.pcm for c in B.clips]
    eng.force("lane_gather", 1)
    try:
        staged = eng.exact_lane(pcm)
    finally:
        eng.force("lane_gather", 0)
    for c, got in zip(B.clips, staged):
        assert_rows_equal(got, F.expected(c, F.MAX_STAGED), (c.name, "lane_gather"))


def test_clips_alone_and_reordered(eng, B):
    """Each clip alone, and the batch in reverse with two empty clips first: a clip's rows do not depend on where
    its windows stand in the call."""
    for c in B.clips:
        assert_rows_equal(eng.exact_lane([c.pcm])[0], F.expected(c, F.MAX_STAGED), (c.name, "alone"))
    order = [B.clip("empty"), B.clip("empty")] + B.clips[::-1]
    for c, got in zip(order, eng.exact_lane([c.pcm for c in order], 10)):
        assert_rows_equal(got, F.expected(c, 10), (c.name, "reordered"))
