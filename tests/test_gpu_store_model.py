"""The posting store driven through long mixed sequences of operations, against the numpy model (tests/store_ref.py):
adds from the host, from device tensors, of an empty track and of an extraction, removals (of a live id, and refused
ones), adds to a removed id (dead on arrival), compact, finalize, save and load (into the same engine and into a fresh
one that replaces it), reset, and track ids that regrow the tombstone buffer while earlier tombstones exist. The
existing tests check one transition each from a fresh engine; here the state carries over 40 operations.

The traces come from store_ref.make_trace, a pure function of the seed; test_store_ref_host.py replays them without a
GPU and asserts what they cover. Expected values: the model and oracle/fp_match.c; no other engine call."""

import numpy as np
import pytest

import oracle as O
import store_ref as S
from aidfp import _lib, synth
from aidfp.engine import Engine

pytestmark = pytest.mark.gpu
SR, HOP = S.APPEND_SR, S.APPEND_HOP
MIN_MATCH = 5


class ClipRecords:
    """Track id -> the oracle's records of its one-second clip (the call), and the clip itself."""

    def __init__(self):
        self.cache = {}

    def _get(self, t):
        if t not in self.cache:
            clip = synth.synth(t, 0, SR, SR, salt=t)
            self.cache[t] = (clip, O.fingerprint(clip, HOP))
        return self.cache[t]

    def __call__(self, t):
        return self._get(t)[1]

    def clip(self, t):
        return self._get(t)[0]


@pytest.fixture(scope="module")
def clip_records():
    return ClipRecords()


def new_engine(live):
    eng = Engine(SR, min_match=MIN_MATCH)
    eng.index_live(live)
    return eng


def check_store(eng, m):
    st = eng.index_stats()
    assert (st["postings"], st["tracks"]) == (len(m.post), m.n_tracks)
    got = eng.index_export()
    bad = np.flatnonzero((got != m.post).any(axis=1))
    assert len(bad) == 0, f"{len(bad)} stored postings differ, first at {bad[:5]}"
    assert eng.index_checksum() == m.checksum()


@pytest.mark.parametrize("live", [0, 2000], ids=["live_off", "live_2000"])
@pytest.mark.parametrize("seed", S.TRACE_SEEDS)
def test_operation_sequence_equals_the_model(seed, live, clip_records, tmp_path):
    import torch

    ops = S.make_trace(seed, clip_records)
    rp = S.Replay(clip_records)
    eng = new_engine(live)
    path = str(tmp_path / "store.aidfp")
    try:
        for i, (kind, arg) in enumerate(ops):
            where = f"seed {seed}, operation {i}: {kind}"
            if kind in ("add_host", "add_dead"):
                h, tr, t = S.columns(arg)
                eng.index_add_postings(h.ctypes.data, tr.ctypes.data, t.ctypes.data, len(arg), device=False)
            elif kind == "add_device":
                dev = [torch.from_numpy(c.view(np.int32)).cuda() for c in S.columns(arg)]
                eng.index_add_postings(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), len(arg), device=True)
            elif kind == "add_track":
                eng.index_add_records(arg, np.zeros(0, np.uint64))
            elif kind == "add_extracted":
                got = eng.extract_host([clip_records.clip(t) for t in arg])
                assert all(np.array_equal(g, clip_records(t)) for g, t in zip(got, arg)), where
                eng.index_add_extracted(np.asarray(arg, dtype=np.uint32))
            elif kind == "remove_live":
                eng.index_remove(arg)
            elif kind == "remove_bad":
                with pytest.raises(_lib.EngineError):
                    eng.index_remove(arg)
            elif kind == "compact":
                dropped = eng.index_compact()
            elif kind == "finalize":
                eng.index_finalize()
            elif kind == "save_load":
                eng.index_save(path)
                eng.index_load(path)
            elif kind == "save_load_fresh":
                eng.index_save(path)
                eng.close()
                eng = new_engine(live)
                eng.index_load(path)
            elif kind == "reset":
                eng.index_reset()
            f = rp.apply(kind, arg)
            m = rp.model
            if kind == "compact":
                assert dropped == f["dropped"], where
            check_store(eng, m)
            if kind == "finalize":  # one CSR over everything, with live ingest on as well (a fold or a rebuild)
                assert eng.index_stats()["live"] == len(m.live()), where
                offs, posts = eng.index_csr()
                keys, ref_posts = m.csr_sorted()
                assert np.array_equal(posts, ref_posts), where
                assert S.offsets_equal(offs, keys), where
            if i % 3 == 2:
                planted, gone = rp.queries()
                for q in (planted, gone):
                    if q is None:
                        continue
                    want = O.query(m.live(), q[1], min_match=MIN_MATCH, max_rows=eng.max_results)
                    got = eng.query([q[1]])[0]
                    assert np.array_equal(got, want), (where, q[0], got[:4], want[:4])
                    if q is gone:  # a removed track: no row of it, compacted or not
                        assert q[0] not in got[:, 1].tolist(), where
    finally:
        eng.close()
