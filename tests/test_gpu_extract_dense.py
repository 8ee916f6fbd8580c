"""K2 (csrc/peaks.hip) and K3 (csrc/landmarks.hip) at the peak-density bound, on constructed clips
(dense_fixtures.py; their preconditions: test_dense_fixtures_host.py): a peak in every 16-bin x 8-frame cell, so a
K3 chunk list of exactly kHashChunkPeakCap entries and a record region 99 % full between two other clips; 16
anchors per K3 thread with targets 64 and more list positions away (the WRITE pass's re-walk) in clips of several
chunks (the COUNT pass); white noise; peaks at every bin; pairs on and just outside the target zone; peaks on the
frames where chunks and their zones end. Every comparison is bit for bit against the CPU oracle
(oracle/fp_oracle.c, FPSPEC 5-6): peaks, counts and records."""

import functools

import numpy as np
import pytest

import dense_fixtures as D
import oracle as O
from aidfp import synth
from aidfp.engine import Engine, peaks_from_mask
from s16_inputs import widen

pytestmark = pytest.mark.gpu
SR = 44100
HOP = 512
SHORT = 1500  # samples: shorter than a frame


def _oracle(x, hop):
    pk = O.peaks(O.stft_power(x, hop)).reshape(-1, 2) if len(x) >= 2048 else np.zeros((0, 2), np.int32)
    return pk, O.fingerprint(x, hop)


@functools.lru_cache(maxsize=None)
def _batch(name):
    """(clips, hop, reference peaks, reference records) of a call, built and judged by the oracle once."""
    if name == "bound":  # a sparse clip, the lattice at the bound, a second lattice: the full region has neighbours
        hop = 2048
        clips = [synth.synth(31, 0, D.n_samples(200, hop), SR, salt=7), D.lattice(1100, hop)[0],
                 D.lattice(64, hop, k0=8)[0]]
    elif name == "dense":
        hop = HOP
        clips = [D.lattice(1100, hop)[0], D.lattice(1100, hop, diag=3)[0], D.noise(D.NOISE_FRAMES, hop, 0)[0],
                 D.noise3(hop, 1)[0], np.zeros(D.n_samples(300, hop), np.float32),
                 D.noise(1, hop, 2)[0][:SHORT]]
    elif name == "edges":
        zone, hop = D.zone_edges()
        clips = [zone] + D.chunk_edges(hop)[0]
    elif name == "s16":
        hop = HOP
        clips = [widen(D.to_s16(D.lattice(1100, hop)[0]))]
    else:
        raise KeyError(name)
    refs = [_oracle(x, hop) for x in clips]
    for x in clips:
        x.setflags(write=False)
    return clips, hop, [r[0] for r in refs], [r[1] for r in refs]


def _check(eng, name, lens=None):
    """The engine's last extraction against the oracle: peaks, counts, records of every clip."""
    clips, _, peaks, recs = _batch(name)
    counts = eng.counts()
    assert counts.tolist() == [len(r) for r in recs], name
    for c, x in enumerate(clips):
        pk = peaks_from_mask(eng.peakmask(c, len(x) if lens is None else lens[c]))
        assert np.array_equal(pk, peaks[c]), f"{name} clip {c}: peaks differ"
        assert np.array_equal(eng.hashes(c), recs[c]), f"{name} clip {c}: records differ"


@pytest.fixture(scope="module")
def eng2048():
    with Engine(SR, hop=2048) as e:
        yield e


def test_at_the_bound(eng2048):
    """The hop-2048 lattice: chunk 0's list is kHashChunkPeakCap = 8704 entries, 16 anchors per thread, nearly
    every accepted target 64 or more positions out, 87,674 records in a region of hash_capacity = 88,320. An
    overrun of the list or of the region would corrupt the walk or a neighbour's records. Twice: the second call
    finds its descriptors cached."""
    clips, hop, _, recs = _batch("bound")
    assert len(recs[1]) >= 0.99 * eng2048.hash_capacity(len(clips[1])) and len(recs[0]) > 0 and len(recs[2]) > 0
    for _ in range(2):
        got = eng2048.extract_host(clips)
        _check(eng2048, "bound")
        for c in range(len(clips)):
            assert np.array_equal(got[c], recs[c]), c


def test_bound_batch_indexed_and_queried(eng2048):
    """The same call into the index: the export is the three clips' records under their tracks, in order, and
    queries of the whole lattice and of its first 200 frames give the oracle's rows on those postings."""
    clips, hop, _, recs = _batch("bound")
    tracks = [7, 3, 11]
    eng2048.index_reset()
    eng2048.extract_host(clips)
    eng2048.index_add_extracted(tracks)
    post = eng2048.index_export()
    want = np.concatenate([np.stack([(r & np.uint64(0xFFFFFFFF)).astype(np.uint32), np.full(len(r), t, np.uint32),
                                     (r >> np.uint64(32)).astype(np.uint32)], axis=1) for r, t in zip(recs, tracks)])
    assert np.array_equal(post, want)
    eng2048.index_finalize()
    queries = [recs[1], O.fingerprint(clips[1][:D.n_samples(200, hop)], hop)]
    got = eng2048.query(queries)
    for q, g in zip(queries, got):
        ref = O.query(post, q, min_match=eng2048.min_match, max_rows=eng2048.max_results)
        assert len(ref) > 0 and ref[0][1] == 3
        assert np.array_equal(g, ref), (g[:3], ref[:3])
    eng2048.index_reset()


def _device_batch(clips):
    """The clips back to back in one device buffer behind one pad sample: the first clip starts at sample 1."""
    import torch

    offs = 1 + np.concatenate([[0], np.cumsum([len(x) for x in clips])]).astype(np.int64)
    buf = np.zeros(int(offs[-1]), np.float32)
    buf[1:] = np.concatenate(clips)
    return torch.from_numpy(buf).cuda(), offs


def test_dense_at_the_default_hop(gpu_engine):
    """Hop 512: the overlapping lattice (4,701 anchors in a chunk, both WRITE branches), the diagonal lattice
    (peaks at every bin), white noise of two and of three chunks, silence and a clip without a frame, in one call;
    then the same clips from one device buffer with the lattice at an odd sample offset."""
    import torch

    clips, hop, _, recs = _batch("dense")
    assert gpu_engine.hop == hop
    got = gpu_engine.extract_host(clips)
    _check(gpu_engine, "dense")
    assert [len(g) for g in got[-2:]] == [0, 0] and min(len(g) for g in got[:4]) > 20000
    dev, offs = _device_batch(clips)
    assert offs[0] % 2 == 1  # the lattice
    gpu_engine.extract_device(dev.data_ptr(), offs, torch.cuda.current_stream().cuda_stream)
    _check(gpu_engine, "dense")


@pytest.mark.parametrize("what,value", [("k2_width", 2), ("k2_width", 4), ("k2_strips_x100", 1),
                                        ("k2_strips_x100", 100), ("plane_rows", 700)])
def test_engine_variations_on_the_dense_batch(what, value):
    """K2's two workgroup widths, its longest and its default strips, and a plane bound of 700 rows (every dense
    clip is longer: each is alone in its K1 -> K2 group), on the dense batch."""
    clips, hop, _, _ = _batch("dense")
    with Engine(SR) as eng:
        eng.force(what, value)
        eng.extract_host(clips)
        if what == "k2_width":
            assert eng.match_stats()["k2_width"] == value
        if what == "plane_rows":
            assert min(eng.num_frames(len(x)) for x in clips[:4]) > value
        _check(eng, "dense")


def test_zone_and_chunk_edges(eng2048):
    """Pairs at dt 63 / 64, |df| 127 / 128 and dt 0, anchors at bins 1 and 1023 and at the first and last frame;
    clips that end on, one past and around frames 1024 and 1087 with peaks on those frames. The zone clip's
    records are also the list written out from the design, so the oracle and the kernel cannot share a misreading
    of FPSPEC 6."""
    clips, hop, _, recs = _batch("edges")
    got = eng2048.extract_host(clips)
    _check(eng2048, "edges")
    assert np.array_equal(got[0], D.zone_records()) and len(got[0]) == 8
    assert np.array_equal(peaks_from_mask(eng2048.peakmask(0, len(clips[0]))), D.zone_peaks())
    for c, F in enumerate(D.CHUNK_EDGE_FRAMES, start=1):
        assert np.array_equal(peaks_from_mask(eng2048.peakmask(c, len(clips[c]))), D.chunk_edge_peaks(F)), F


def test_dense_int16(gpu_engine):
    """The hop-512 lattice as int16 PCM: the reference is the oracle on q / 32768 (s16_inputs.widen)."""
    clips, hop, _, recs = _batch("s16")
    q = D.to_s16(D.lattice(1100, hop)[0])
    assert np.array_equal(widen(q), clips[0])
    got = gpu_engine.extract_host([q], fmt="s16")
    _check(gpu_engine, "s16")
    assert np.array_equal(got[0], recs[0]) and len(recs[0]) > 40000
