"""FingerprintService(live_ingest=...): ingest while serving. The same store -> query -> store -> delete -> query
sequence through a service with the live index and through one without gives identical matches, while the live
service's engine builds its main segment once; a restart replays the journal as a bulk load that ends in one build.
The resolution of the option and of AIDFP_LIVE_INGEST needs no GPU: tests/test_live_ingest_option.py."""

import uuid

import pytest

from aidfp import fingerprint as fp
from aidfp import synth

pytestmark = pytest.mark.gpu
SR = 16000


def _bytes(track, start_s, dur_s, snr=None, salt=0):
    return synth.synth(track, int(start_s * SR), int(dur_s * SR), SR, snr_db=snr, salt=salt).astype("<f4").tobytes()


def test_live_service_equals_plain_service(tmp_path):
    names = [str(uuid.UUID(int=0xD000 + i)) for i in range(6)]
    tracks = [_bytes(i, 0, 20) for i in range(6)]
    queries = [_bytes(i, 3.0 + i, 5.0, snr=20, salt=40 + i) for i in range(6)]
    live = fp.FingerprintService(tmp_path / "live", live_ingest=1 << 20)
    ref = fp.FingerprintService(tmp_path / "ref")
    assert live.live_ingest == 1 << 20 and ref.live_ingest == 0
    try:
        def both(fn):
            a, b = fn(live), fn(ref)
            assert a == b, (a, b)
            return a

        for k in range(3):  # store
            assert both(lambda s: s.index_track(tracks[k], names[k]))
        first = [both(lambda s: s.query(q)) for q in queries]  # query: the one main build
        assert all(first[i] and first[i][0].reference_path == names[i] for i in range(3))
        assert not any(m.reference_path in names[3:] for r in first for m in r)
        assert live._engine.index_live_stats()["main_builds"] == 1
        for k in range(3, 6):  # store, with a query after each: delta builds only
            assert both(lambda s: s.index_track(tracks[k], names[k]))
            r = both(lambda s: s.query(queries[k]))
            assert r and r[0].reference_path == names[k]
        assert both(lambda s: s.delete_track(names[1]))  # delete, one track of each segment
        assert both(lambda s: s.delete_track(names[4]))
        assert both(lambda s: s.index_track(tracks[1], names[4]))  # a re-store under a deleted name
        last = [both(lambda s: s.query(q)) for q in queries]
        assert all(m.reference_path != names[1] for r in last for m in r)
        assert last[1] and last[1][0].reference_path == names[4]
        assert last[0] and last[0][0].reference_path == names[0]
        assert both(lambda s: s.exact_batch(queries[:4], 5))
        st = live._engine.index_live_stats()
        # main was built once, at the first query; every later store went into the delta (3 + the re-store)
        assert (st["main_builds"], st["folds"]) == (1, 0) and st["delta_builds"] == 4, st
        assert not any(st["fallbacks"].values()), st
        assert ref._engine.index_live_stats()["main_builds"] >= 5  # without it every store + query rebuilds
    finally:
        live.close()
        ref.close()
    again = fp.FingerprintService(tmp_path / "live", live_ingest=1 << 20)  # the journal replay: a bulk load
    try:
        assert [again.query(q) for q in queries] == last
        st = again._engine.index_live_stats()
        assert (st["main_builds"], st["delta_builds"], st["folds"]) == (1, 0, 0), st
        assert not any(st["fallbacks"].values()), st
        again.checkpoint()  # aid_index_compact drops the deleted tracks' postings: the full build, counted
        assert [again.query(q) for q in queries] == last
        st = again._engine.index_live_stats()
        assert st["main_builds"] == 2 and st["fallbacks"]["compact"] == 1, st
    finally:
        again.close()
