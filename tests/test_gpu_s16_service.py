"""Native int16 PCM through the serving layers: StreamBank(pcm_format="s16") against the oracle route, and
FingerprintService(pcm_format="s16") (coalescer, persistence, the olaf_c-compatible CLI through AIDFP_PCM_FORMAT)
against an f32 service fed q / 32768."""

import os
import subprocess
import sys
import uuid
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest
import torch

from aidfp import fingerprint as fp
from aidfp import synth
from aidfp.engine import Engine
from s16_inputs import synth_q, widen

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
SR = 16000


def test_stream_bank_s16_equals_oracle_route():
    """2 live 48 kHz stereo int16 streams against a 16 kHz index (the sizes of
    tests/test_gpu_stream.py::test_stream_bank_equals_oracle_route): chunks of unequal length, so the in-place device
    chunks start at every alignment a 4-byte frame has within 16 bytes and the history's split moves; host-array
    chunks in between (the int16 pinned staging); one push in two halves (push_submit). The windows equal the
    oracle route on q / 32768: host downmix, oracle/fp_resample.c, oracle/fp_oracle.c, oracle/fp_match.c."""
    import bench
    from aidfp.catalog import ingest_synthetic
    from aidfp.stream import StreamBank

    SSR, QSR = 16000, 48000
    with Engine(SSR) as eng:
        ingest_synthetic(eng, np.arange(60, dtype=np.uint32), 30.0, batch=64, source_sr=44100, local=True)
        eng.index_finalize()
        S, n_seg, seg = 2, 2, 12 * QSR
        seg_tracks = np.random.default_rng(3).integers(0, 60, (S, n_seg)).astype(np.uint32)
        stereo = torch.empty(S, n_seg * seg, 2, dtype=torch.float32, device="cuda")
        tmp = torch.empty(S * n_seg * seg, dtype=torch.float32, device="cuda")
        for ch in range(2):
            eng.synth(tmp.data_ptr(), seg_tracks.ravel(), np.zeros(S * n_seg, np.int64), seg,
                      noise_a=synth.noise_halfwidth(30.0), salt=11 + ch, sample_rate=QSR)
            stereo[:, :, ch] = tmp.view(S, n_seg * seg)
        q = (stereo * 32768.0).to(torch.int16)  # the generator's own int16 samples (its output is q / 32768)
        assert torch.equal(q.float() / 32768.0, stereo)
        bank = StreamBank(eng, S, stream_sr=QSR, pcm_format="s16")
        res = [[] for _ in range(S)]
        sizes = [65761, 65760, 65763, 65762, 40001]
        a = k = 0
        while a < q.shape[1]:
            chunk = q[:, a:a + sizes[k % len(sizes)]]
            if k % 3 == 1:
                chunk = chunk.cpu().numpy()
            r = bank.push_submit(chunk).collect() if k == 4 else bank.push(chunk)
            for i in range(S):
                res[i] += r[i]
            a += sizes[k % len(sizes)]
            k += 1
        assert bank._hist[0].dtype == torch.int16 and bank._cur.dtype == torch.int16 and bank._pin.dtype == torch.int16
        assert all(len(res[i]) == int((n_seg * 12.0 - 5.0) // 2.5) + 1 for i in range(S))
        assert sum(len(w.rows) > 0 for i in range(S) for w in res[i]) > 0
        par = bench.stream_parity(eng, stereo, seg_tracks, res, S, torch, max_windows=8)
        with pytest.raises(ValueError):
            bank.push(stereo[:, :100])  # float chunks are not narrowed silently
    assert par["windows"] == S * 8
    assert par["bit_exact"], par


def _s16_bytes(track, start_s, dur_s, snr=None, salt=0):
    return synth_q(track, int(start_s * SR), int(dur_s * SR), SR, snr_db=snr, salt=salt).astype("<i2").tobytes()


def _f32_bytes(s16: bytes) -> bytes:
    return widen(np.frombuffer(s16, dtype="<i2")).astype("<f4").tobytes()


def test_service_s16(tmp_path):
    names = [str(uuid.UUID(int=0xC000 + i)) for i in range(3)]  # the exact lane keeps UUID-named tracks only
    tracks = [_s16_bytes(i, 0, 20) for i in range(3)]
    queries = [_s16_bytes(i % 3, 2.0 + i, 5.0, snr=20, salt=70 + i) + (b"\x01" if i % 2 else b"") for i in range(12)]
    svc = fp.FingerprintService(tmp_path / "s16", pcm_format="s16")
    ref = fp.FingerprintService(tmp_path / "f32")
    try:
        for name, t in zip(names, tracks):
            assert svc.index_track(t, name) and ref.index_track(_f32_bytes(t), name)
        with ThreadPoolExecutor(8) as pool:  # concurrent requests: the coalescer merges them into s16 batches
            got = list(pool.map(svc.query, queries))
        want = [ref.query(_f32_bytes(b[: len(b) // 2 * 2])) for b in queries]
        assert got == want
        assert all(g and g[0].reference_path == names[i % 3] for i, g in enumerate(got))
        exact = svc.exact_batch(queries[:3], 5)
        assert exact == ref.exact_batch([_f32_bytes(b[: len(b) // 2 * 2]) for b in queries[:3]], 5) and all(exact)
        assert svc.delete_track(names[2]) and not svc.delete_track(names[2])
        assert all(m.reference_path != names[2] for m in svc.query(queries[2]))
    finally:
        svc.close()
        ref.close()
    again = fp.FingerprintService(tmp_path / "s16", pcm_format="s16")  # a restart reads the persisted index
    try:
        r = again.query(queries[1])
        assert r == want[1] and r[0].reference_path == names[1]
        assert all(m.reference_path != names[2] for m in again.query(queries[2]))
    finally:
        again.close()


def test_cli_inherits_format_from_env(tmp_path):
    """`aidfp.cli store` / `query` on raw s16le files with AIDFP_PCM_FORMAT=s16 in the child's environment print the
    CSV an f32 service gives for the same audio as f32le."""
    track, query = _s16_bytes(4, 0, 20), _s16_bytes(4, 6.0, 5.0, snr=20, salt=9)
    (tmp_path / "track.raw").write_bytes(track)
    (tmp_path / "query.raw").write_bytes(query)
    env = dict(os.environ, AIDFP_DB=str(tmp_path / "cli_db"), AIDFP_PCM_FORMAT="s16",
               PYTHONPATH=os.pathsep.join([str(ROOT / "audio-ident_amd")] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    cli = [sys.executable, "-m", "aidfp.cli"]
    st = subprocess.run(cli + ["store", str(tmp_path / "track.raw"), "the-track"], env=env, capture_output=True,
                        text=True, timeout=300)
    assert st.returncode == 0, st.stderr
    out = subprocess.run(cli + ["query", str(tmp_path / "query.raw"), "query"], env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr
    ref = fp.FingerprintService(tmp_path / "f32_db")
    try:
        assert ref.index_track(_f32_bytes(track), "the-track")
        want = [fp.format_match(m) for m in ref.query(_f32_bytes(query))]
    finally:
        ref.close()
    assert want and want[0].split(", ")[3] == "the-track"
    assert out.stdout.strip().splitlines() == want
