"""Host-side checks of audio-ident_amd/csrc/aidfp_mel_plan.h (compiled with g++, no GPU): the planning half of the
CLAP log-mel front end (spec/FPSPEC.md 10). One stand-alone program with its own main reads cases and prints what
the header computes: the chunk plan of a length in either mode, the supports and K of both shipped banks and of broken
tables, K10's grid and output size. Expected values are the reference's captured chunk_audio tuples
(tests/golden/ref_clap_chunks.json), the captured filter banks (tests/golden/ref_clap_mel.npz) or restated here from
the spec; none is taken from the program's output. The same cases run a second time through a build with
-fsanitize=address,undefined (the sanitizer's runtime linked statically into the program).

K is 1 + the highest bin any band weights. For both shipped banks that is 299: the last triangle ends at 14 kHz =
bin 298.67, so bin 298 is the highest with a non-zero weight (the captured banks say the same)."""

import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
SRC = r"""
#include <cstdio>
#include <iostream>
#include <string>
#include "aidfp_mel_plan.h"
using namespace aid;
int main() {
    std::string cmd;
    std::vector<MelChunk> plan;  // reused, as the engine reuses its own
    while (std::cin >> cmd) {
        if (cmd == "plan") {
            int mode, nc;
            long long start;
            std::cin >> mode >> start >> nc;
            std::vector<int64_t> len(nc);
            for (auto &x : len) std::cin >> x;
            const int st = mel_plan(len.data(), nc, mode, start, plan);
            std::printf("plan %d %zu", st, plan.size());
            for (const MelChunk &c : plan)
                std::printf(" %d %d %lld %d %d %.17g %.17g %lld", c.clip, c.chunk_index, (long long)c.start, c.r, c.rep,
                            c.offset_sec, c.duration_sec, (long long)c.fill());
            std::printf("\n");
        } else if (cmd == "bank") {
            int kind, broken;
            double fmin, fmax;
            std::cin >> kind >> fmin >> fmax >> broken;
            std::vector<float> W;
            int st = mel_build_bank(kind, fmin, fmax, W);
            MelSupport s;
            if (st == kMelOk) {
                if (W.size() != (size_t)kMelBins * kMelBands) return 2;
                if (broken == 1) {  // a gap inside band 30
                    if (mel_supports(W.data(), s) != kMelOk || s.hi[30] - s.lo[30] < 3) return 5;
                    W[(size_t)(s.lo[30] + 1) * kMelBands + 30] = 0.f;
                }
                if (broken == 2)
                    for (int k = 0; k < kMelBins; ++k) W[(size_t)k * kMelBands + 7] = 0.f;  // band 7 all zero
                if (broken == 3) {  // band 63 runs on through the Nyquist bin
                    if (mel_supports(W.data(), s) != kMelOk) return 5;
                    for (int k = s.lo[63]; k < kMelBins; ++k) W[(size_t)k * kMelBands + 63] = 1.f;
                }
                if (broken == 4) W[(size_t)100 * kMelBands + 30] = -1.f;                    // a negative weight
                st = mel_supports(W.data(), s);
            }
            std::printf("bank %d", st);
            if (st == kMelOk) {
                std::printf(" %d %d", s.K, s.max_len);
                for (int m = 0; m < kMelBands; ++m) std::printf(" %d %d", s.lo[m], s.hi[m]);
                for (int m = 0; m < kMelBands; ++m)
                    for (int k = s.lo[m]; k < s.hi[m]; ++k) std::printf(" %a", (double)W[(size_t)k * kMelBands + m]);
            }
            std::printf("\n");
        } else if (cmd == "cap") {
            long long chunks, cap;
            std::cin >> chunks >> cap;
            std::printf("cap %lld %lld %d\n", (long long)mel_grid(chunks), (long long)mel_out_floats(chunks),
                        mel_fits(chunks, cap) ? 1 : 0);
        } else {
            return 3;
        }
    }
    std::printf("consts %d %d %d %d %d %d %d %d %d %d\n", kMelN, kMelHop, kMelWindow, kMelChunkHop, kMelMinChunk,
                kMelFrames, kMelBands, kMelRun, kMelRuns, kMelStage);
    return 0;
}
"""

OK, BAD_MODE, BAD_LENGTH, BAD_START, TOO_MANY, EMPTY_BAND, GAP_BAND, NYQUIST, BAD_RANGE = range(9)  # MelStatus
L, HOP_C, RUN = 480000, 240000, 4
LENGTHS = [0, 1, 47999, 48000, 287999, 288000, 479999, 480000, 480001, 720000, 86400000]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def run(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("mel_plan_" + request.param)
    (d / "mel_check.cpp").write_text(SRC)
    exe = d / "mel_check"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                    *(san if request.param == "sanitized" else []),
                    "-I", str(ROOT / "audio-ident_amd" / "csrc"), str(d / "mel_check.cpp"), "-o", str(exe)], check=True)

    def run_(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        rows = out.stdout.strip().split("\n")
        assert rows[-1] == f"consts 1024 480 {L} {HOP_C} 48000 1001 64 {RUN} {-(-1001 // RUN)} {(RUN - 1) * 480 + 1024}"
        assert len(rows) == len(lines) + 1
        return [r.split()[1:] for r in rows[:-1]]

    return run_


def _chunks(row):
    st, n = int(row[0]), int(row[1])
    f = row[2:]
    assert len(f) == 8 * n
    return st, [(int(f[8 * i]), int(f[8 * i + 1]), int(f[8 * i + 2]), int(f[8 * i + 3]), int(f[8 * i + 4]),
                 float(f[8 * i + 5]), float(f[8 * i + 6]), int(f[8 * i + 7])) for i in range(n)]


def test_zero_mode_equals_chunk_audio(run):
    """Per length the reference's (offset_sec, chunk_index, duration_sec) tuples, doubles compared for equality."""
    gold = json.loads((GOLD / "ref_clap_chunks.json").read_text())
    assert gold["lengths"] == LENGTHS
    rows = run([f"plan 0 0 1 {n}" for n in LENGTHS])
    for n, row in zip(LENGTHS, rows):
        st, got = _chunks(row)
        want = gold["chunks"][str(n)]
        assert st == OK and len(got) == len(want), n
        for (clip, idx, start, r, rep, off, dur, fill), (woff, widx, wdur) in zip(got, want):
            assert (clip, idx, off, dur, rep, fill) == (0, widx, woff, wdur, 1, r), n
            assert start == HOP_C * idx and r == min(L, n - start) and r >= 48000
    # the 30-minute track: starts 0, 240000, .. while at least 48000 samples remain: 1 + (n - 48000) // 240000
    assert len(_chunks(rows[-1])[1]) == 1 + (86400000 - 48000) // HOP_C == 360


def test_zero_mode_batch_numbers_clips(run):
    st, got = _chunks(run(["plan 0 0 4 48000 0 720000 47999"])[0])
    assert st == OK
    assert [(c[0], c[1], c[2], c[3]) for c in got] == [(0, 0, 0, 48000), (2, 0, 0, 480000), (2, 1, 240000, 480000),
                                                            (2, 2, 480000, 240000)]


def test_repeatpad_rep_and_zero_tail(run):
    rs = [1, 144000, 160001, 240000, 479999]
    rows = run([f"plan 1 0 1 {r}" for r in rs])
    for r, row in zip(rs, rows):
        st, got = _chunks(row)
        assert st == OK and len(got) == 1
        clip, idx, start, rr, rep, off, dur, fill = got[0]
        assert (clip, idx, start, rr, off, dur) == (0, 0, 0, r, 0.0, r / 48000)
        assert rep == L // r and fill == (L // r) * r
        assert L - fill == {1: 0, 144000: 48000, 160001: 159998, 240000: 0, 479999: 1}[r]  # the zero tail


def test_repeatpad_long_query_takes_start(run):
    n = L + 1234
    rows = run([f"plan 1 0 1 {n}", f"plan 1 1234 1 {n}", f"plan 1 1235 1 {n}", f"plan 1 -1 1 {n}", f"plan 1 7 2 {L} 0",
                "plan 2 0 1 48000", "plan 0 0 1 -5"])
    for row, start in zip(rows[:2], (0, 1234)):
        st, got = _chunks(row)
        assert st == OK and got == [(0, 0, start, L, 1, start / 48000, 10.0, L)]
    assert int(rows[2][0]) == BAD_START and int(rows[3][0]) == BAD_START
    st, got = _chunks(rows[4])  # exactly L: start is not used; the empty clip has no chunk
    assert st == OK and got == [(0, 0, 0, L, 1, 0.0, 10.0, L)]
    assert int(rows[5][0]) == BAD_MODE and int(rows[6][0]) == BAD_LENGTH


@pytest.mark.parametrize("kind,name", [(0, "slaney"), (1, "htk")])
@pytest.mark.parametrize("fmin", [50, 0])
def test_bank_supports_and_K(run, kind, name, fmin):
    """Supports equal the captured bank's, K = 1 + the highest weighted bin = 299, weights within 1 binary32 ulp."""
    z = np.load(GOLD / "ref_clap_mel.npz")
    lo, hi, w = z[f"bank_{name}_{fmin}_lo"], z[f"bank_{name}_{fmin}_hi"], z[f"bank_{name}_{fmin}_w"]
    row = run([f"bank {kind} {fmin} 14000 0"])[0]
    assert int(row[0]) == OK
    K, max_len = int(row[1]), int(row[2])
    got = np.array(row[3:3 + 128], dtype=np.int64).reshape(64, 2)
    assert np.array_equal(got[:, 0], lo) and np.array_equal(got[:, 1], hi)
    assert K == int(hi.max()) == 299 and max_len == int((hi - lo).max())
    gw = np.array([float.fromhex(s) for s in row[3 + 128:]], dtype=np.float32)
    want = w.astype(np.float32)
    assert gw.shape == want.shape
    assert np.all(np.abs(gw.astype(np.float64) - want.astype(np.float64)) <= np.spacing(want).astype(np.float64))


def test_broken_tables_are_rejected(run):
    rows = run(["bank 0 50 14000 1", "bank 0 50 14000 2", "bank 1 50 14000 3", "bank 1 50 14000 4",
                "bank 0 14000 50 0", "bank 0 50 24001 0", "bank 1 -1 14000 0"])
    assert [int(r[0]) for r in rows] == [GAP_BAND, EMPTY_BAND, NYQUIST, EMPTY_BAND, BAD_RANGE, BAD_RANGE, BAD_RANGE]


def test_capacity_is_int64(run):
    runs = -(-1001 // RUN)
    rows = run(["cap 360 360", "cap 360 359", "cap 500000 500000", "cap 40000000 40000000", "cap 0 0"])
    assert rows[0] == [str(360 * runs), str(360 * 1001 * 64), "1"]  # the 30-minute track
    assert rows[1][2] == "0"
    assert rows[2] == [str(500000 * runs), str(500000 * 1001 * 64), "1"]  # config 3's catalog: 3.2e10 floats
    assert rows[3][1] == str(40000000 * 1001 * 64) and int(rows[3][1]) > 2**41
    assert rows[4] == ["0", "0", "1"]
