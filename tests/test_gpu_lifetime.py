"""Every device block, page-locked block and event an engine allocates goes when the engine is destroyed
(aid_live_allocations). Other tests' engines may be alive in the process, so counts are compared with their values
before a cycle, never with zero."""

import ctypes

import numpy as np
import pytest

from aidfp import _lib as L
from aidfp._lib import AID_PCM_HOST, EngineError
from aidfp.engine import Engine, _p

pytestmark = pytest.mark.gpu

SR = 16000  # hop 256: the smallest shapes that still reach every lazily created resource


def live() -> tuple[int, int, int]:
    d, p, e = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert L.load().aid_live_allocations(ctypes.byref(d), ctypes.byref(p), ctypes.byref(e)) == 0
    return d.value, p.value, e.value


def _dedup(eng: Engine, n: int, salt: int) -> None:
    rng = np.random.default_rng(salt)
    words = rng.integers(0, 2**32, size=n * 120, dtype=np.uint32)
    off = np.arange(n + 1, dtype=np.int64) * 120
    dur = np.full(n, 15.0)
    assert eng._lib.aid_dedup_add(eng._h, _p(words), _p(off), _p(dur), n) == 0
    idx, sim = np.zeros(n, np.int64), np.zeros(n, np.float64)
    assert eng._lib.aid_dedup_scan(eng._h, _p(words), _p(off), _p(dur), n, _p(idx), _p(sim)) == 0


def _vec(eng: Engine) -> None:
    from aidfp.vibe import HIT_DTYPE

    rng = np.random.default_rng(3)
    vecs = rng.standard_normal((70, 32)).astype(np.float32)
    tracks = np.arange(70, dtype=np.uint32)
    offs = np.zeros(70, np.float64)
    assert eng._lib.aid_vec_reset(eng._h, 32) == 0
    assert eng._lib.aid_vec_add(eng._h, _p(vecs), _p(tracks), None, _p(offs), 70, AID_PCM_HOST) == 0
    hits, nh = np.zeros((2, 5), dtype=HIT_DTYPE), np.zeros(2, np.int32)
    assert eng._lib.aid_vec_search(eng._h, _p(vecs), 2, AID_PCM_HOST, 5, _p(hits), _p(nh), None) == 0
    assert list(nh) == [5, 5] and hits[0, 0]["track"] == 0 and hits[1, 0]["track"] == 1


def _cycle(tmp_path) -> None:
    """One engine through every call that allocates, closed at the end; the error path that must not leak while
    the engine is alive is checked on the way."""
    import torch

    n = 2 * SR
    eng = Engine(SR, peak_rel=0.01)
    try:
        eng.profile_enable(True)
        dev = torch.empty(3 * n, dtype=torch.float32, device="cuda")
        eng.synth(dev.data_ptr(), [1, 2, 3], np.zeros(3, np.int64), n)
        x = dev.cpu().numpy().reshape(3, n)
        # host-PCM extraction of 0 s and 1 s, then a larger one (every per-call buffer grows)
        small = eng.extract_host([x[0, :0], x[0, :SR]])
        assert len(small[0]) == 0 and len(small[1]) > 0
        eng.index_add_extracted([0, 1])  # the posting planes' first growth
        big = eng.extract_host([x[0], x[1], x[2, :SR], x[2, :0]])
        assert all(len(b) > 0 for b in big[:3])
        eng.index_add_extracted([2, 3, 4, 5])  # they grow again, keeping the stored postings
        eng.extract_host([x[2, SR:]])
        eng.index_add_extracted([6])  # within the headroom: the append whose count comes back asynchronously
        assert eng.index_stats()["postings"] == len(small[1]) + sum(len(b) for b in big) + len(eng.hashes(0))
        eng.index_finalize()
        rows = eng.query_pcm([x[1]])  # synchronous: the LDS pass
        assert rows[0][0][1] == 3
        eng.force("k5_path", 2)
        assert eng.query_pcm([x[1]])[0][0][1] == 3  # the global path's histogram, bitmap and set
        eng.force("k5_path", 0)
        got = eng.query_windows_submit(dev.data_ptr(), [0, n], [n, 2 * n]).collect()  # a ticket, collected
        assert [g[0][1] for g in got] == [2, 3]
        out = torch.empty(2 * n, dtype=torch.float32, device="cuda")
        assert eng.resample(dev.data_ptr(), n, 1, SR, 8000, out.data_ptr(), 2 * n) == n // 2
        assert eng.resample(dev.data_ptr(), n, 1, SR, 24000, out.data_ptr(), 2 * n) == 3 * n // 2
        torch.cuda.synchronize()
        assert eng.spectrogram(x[0, :SR]).shape == (eng.num_frames(SR), 1024)
        _dedup(eng, 3, 1)
        _dedup(eng, 5, 2)
        _vec(eng)
        eng.index_remove(3)
        assert eng.index_compact() == len(big[1])
        path = tmp_path / "index.bin"
        eng.index_save(str(path))
        eng.index_load(str(path))
        # a file truncated inside the first column: the load fails, the engine lives on, nothing leaks
        cut = tmp_path / "cut.bin"
        cut.write_bytes(path.read_bytes()[: 8 + 48 + 10])
        before = live()
        with pytest.raises(EngineError, match="truncated index file"):
            eng.index_load(str(cut))
        assert live() == before
        assert eng.profile_read()
    finally:
        eng.close()


def test_engine_frees_all_it_allocated(tmp_path):
    for cycle in range(3):
        before = live()
        _cycle(tmp_path)
        after = live()
        print(f"cycle {cycle}: (device, pinned, events) {before} -> {after}")
        assert after == before, f"cycle {cycle}: (device, pinned, events) {before} -> {after}"


def test_failed_create_leaves_nothing():
    before = live()
    with pytest.raises(EngineError, match="hop must be one of"):
        Engine(SR, hop=100)
    assert live() == before
