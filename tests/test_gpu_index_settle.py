"""GPU: every reader of the hash index settles an in-flight append first.

aid_index_add_extracted appends without waiting for its batch's posting count when the planes have room (the count
comes back behind an event; index_host.cpp settle_postings). test_gpu_match.py's
test_async_append_equals_per_clip_records has stats, a host append, export and save as the first reader after such
an append; this file has the other readers. Expected postings come from the records extract_host returned, never
from the engine's own index calls."""

import numpy as np
import pytest

from aidfp import synth
from aidfp.catalog import checksum_np
from aidfp.engine import Engine

pytestmark = pytest.mark.gpu
SR = 16000
TRACKS_A = np.array([11, 12], np.uint32)
TRACKS_B = np.array([21, 22], np.uint32)


@pytest.fixture(scope="module")
def clips():
    """Two batches of the same shape (2 clips x 2 s), read-only."""
    return tuple([synth.synth(int(t), 0, 2 * SR, SR, salt=int(t)) for t in tr] for tr in (TRACKS_A, TRACKS_B))


def _rows(track, rec):
    return np.stack([(rec & np.uint64(0xFFFFFFFF)).astype(np.uint32), np.full(len(rec), track, np.uint32),
                     (rec >> np.uint64(32)).astype(np.uint32)], axis=1)


def _append_two(eng, clips):
    """Batch A grows the planes to its postings plus one batch's hash capacity; batch B, of the same shape, fits
    that headroom, so its append is asynchronous and its count is in flight when this returns. Returns the expected
    postings per clip, in call order."""
    want = []
    for tracks, batch in zip((TRACKS_A, TRACKS_B), clips):
        recs = eng.extract_host(batch)
        eng.index_add_extracted(tracks)
        want += [_rows(t, r) for t, r in zip(tracks, recs)]
    assert all(len(w) > 0 for w in want)
    return want


def _checksum(eng, want):
    post = np.concatenate(want)
    assert eng.index_checksum(0, len(post)) == checksum_np(post)  # count given: no stats call before the checksum
    return want


def _shard_info(eng, want):
    assert eng.index_shard_info(0) == (sum(map(len, want)), int(TRACKS_B.max()) + 1)
    return want


def _pack(eng, want):
    import torch

    post = np.concatenate(want)
    stride = len(post) + 3  # padded: the tail of every plane is zeroed
    planes = torch.full((3, stride), -1, dtype=torch.int32, device="cuda")
    eng.index_pack(0, planes.data_ptr(), stride)
    got = planes.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:, :len(post)].T, post)
    assert not got[:, len(post):].any()
    return want


def _reserve_splice(eng, want):
    import torch

    n, nt = sum(map(len, want)), int(TRACKS_B.max()) + 1
    eng.index_reserve(0, n, nt)
    planes = torch.zeros((3, n), dtype=torch.int32, device="cuda")
    eng.index_pack(0, planes.data_ptr(), n)
    assert eng.index_splice(0, planes.data_ptr(), [n], n, nt) == n
    return want


def _remove_compact(eng, want):
    eng.index_remove(int(TRACKS_B[0]))  # a track of the batch in flight
    assert eng.index_compact() == len(want[2])
    return want[:2] + want[3:]


def _finalize(eng, want):
    eng.index_finalize()
    assert eng.index_stats()["live"] == sum(map(len, want))
    return want


def _add_postings_device(eng, want):
    import torch

    extra = _rows(31, np.arange(1, 6, dtype=np.uint64) * np.uint64((1 << 32) + 7))
    cols = [torch.from_numpy(np.ascontiguousarray(extra[:, c]).view(np.int32)).cuda() for c in range(3)]
    eng.index_add_postings(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), len(extra), device=True)
    return want + [extra]


@pytest.mark.parametrize("reader", [_checksum, _shard_info, _pack, _reserve_splice, _remove_compact, _finalize,
                                    _add_postings_device], ids=lambda f: f.__name__.lstrip("_"))
def test_first_reader_after_async_append(clips, reader):
    """The reader is the very next engine call after an asynchronous append: it sees both batches whole, and the
    stored postings afterwards are the expected ones in call order."""
    with Engine(SR) as eng:
        want = reader(eng, _append_two(eng, clips))
        assert np.array_equal(eng.index_export(), np.concatenate(want))
