"""Host-side checks of audio-ident_amd/csrc/aidfp_resample_plan.h (compiled with g++, no GPU): which kernel form of K6
`resample` a rate pair runs, its launch shape, and what aid_resample refuses. One stand-alone program reads cases and
prints what the header computes. Every expected value is restated in Python (tests/resample_cases.py) from the rules:

    phase form      1 < up <= 1024 and (16 up - 1) down / up + J + 2 <= 12288 floats; block up * 16 outputs,
                    min(256, ceil(up / 64) * 64) threads, that window of LDS
    decimate3       (up, down, J) == (1, 3, 61); 1024 outputs, 256 threads, 1023 * 3 + 61 + 4 floats
    MODE 2 / MODE 0 up == 1 / any other pair; 1024 outputs, 256 threads, 1023 down / up + J + 2 floats
    refused         a window above 64 KB (tested first), or up * J above 2^24

none is taken from the program's output. The same cases run a second time through a build with
-fsanitize=address,undefined (the sanitizer's runtime linked statically into the program, which has its own main).

This is the guard that makes tests/test_gpu_resample_paths.py mean what it says: if a threshold moves, the case table
here fails instead of a GPU case sliding silently onto another kernel.

MODE 1 (the tap table staged in LDS beside the window, when up > 1 and up * J <= 12288 floats) was removed after the
scan in test_no_pair_could_stage_its_taps_in_lds found no pair that could reach it.

One boundary differs from the issue that asked for these tests, which named 473 -> 2 as the first refused pair after
471 -> 2. By
the rule above (up, down, J) = (2, 473, 4731) has a phase window of 31 * 473 / 2 + 4733 = 12,064 floats and is still
the phase form, as is every odd down through 481 (12,268 floats); 483 -> 2 is the first past it (12,319), and its
1,024-output window (251,887 floats) is refused. Both 473 and the true edge 481 / 483 are asserted here."""

import math
import random
import shutil
import subprocess
from pathlib import Path

import pytest

import oracle as O
import resample_cases as RC

ROOT = Path(__file__).resolve().parent.parent
SRC = r"""
#include <cstdio>
#include <iostream>
#include <numeric>
#include <string>
#include "aidfp_resample_plan.h"
#include "resample_design.h"
using namespace aid;
static void show(const ResLaunch &r) {
    std::printf(" %d %d %lld %d %lld\n", r.path, r.status, (long long)r.block, r.threads, (long long)r.lds_floats);
}
int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "plan") {  // a reduced pair as given
            int up, down, J;
            std::cin >> up >> down >> J;
            std::printf("plan");
            show(resample_launch_plan(up, down, J));
        } else if (cmd == "rates") {  // as the engine goes: resample_plan, then the launch plan
            int sr_in, sr_out;
            std::cin >> sr_in >> sr_out;
            ResamplePlan p;
            if (!resample_plan(sr_in, sr_out, p)) return 4;
            std::printf("rates %d %d %d %d %d %lld %lld", p.up, p.down, p.hl, p.J, (int)use_phase(p.up, p.down, p.J),
                        (long long)window_floats(p.up, p.down, p.J), (long long)resample_lds_floats(p.up, p.down, p.J));
            show(resample_launch_plan(p.up, p.down, p.J));
        } else if (cmd == "scan") {  // the path of every coprime (up, down) <= n, up-major, one digit each
            int n;
            std::cin >> n;
            std::printf("scan ");
            for (int up = 1; up <= n; ++up)
                for (int down = 1; down <= n; ++down) {
                    if (std::gcd(up, down) != 1) continue;
                    ResamplePlan p;
                    if (!resample_plan(down, up, p) || p.up != up || p.down != down) return 5;
                    std::putchar('0' + resample_launch_plan(p.up, p.down, p.J).path);
                }
            std::printf("\n");
        } else {
            return 3;
        }
    }
    std::printf("consts %d %d %d %d %d %d %d %lld %lld %lld\n", kResThreads, kResPerThread, kResBlock, kResR, kDecR,
                kDecThreads, kResMaxPhaseUp, (long long)kResMaxPhaseWindow, (long long)kResMaxLds,
                (long long)kResMaxTaps);
    return 0;
}
"""


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def run(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("resample_plan_" + request.param)
    (d / "resample_check.cpp").write_text(SRC)
    exe = d / "resample_check"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *(san if request.param == "sanitized" else []),
                    "-I", str(ROOT / "audio-ident_amd" / "csrc"), str(d / "resample_check.cpp"), "-o", str(exe)],
                   check=True)

    def run_(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        rows = out.stdout.strip().split("\n")
        assert rows[-1] == f"consts 256 4 {RC.RES_BLOCK} {RC.RES_R} 4 256 {RC.MAX_PHASE_UP} {RC.MAX_PHASE_WINDOW} " \
                           f"{RC.MAX_LDS} {RC.MAX_TAPS}"
        assert len(rows) == len(lines) + 1
        return [r.split()[1:] for r in rows[:-1]]

    return run_


def by_rates(run, pairs):
    """[(up, down, hl, J, use_phase, window, lds, Launch)] of the program for (sr_in, sr_out) pairs."""
    out = []
    for tok in run([f"rates {a} {b}" for a, b in pairs]):
        v = [int(t) for t in tok]
        out.append((*v[:7], RC.Launch(*v[7:])))
    return out


def check_pair(got, sr_in, sr_out):
    up, down, hl, J = RC.ratio(sr_in, sr_out)
    assert got[:4] == (up, down, hl, J), (sr_in, sr_out)
    assert got[4] == int(RC.use_phase(up, down, J)), (sr_in, sr_out)
    assert got[5] == got[6] == RC.window_floats(up, down, J), (sr_in, sr_out)
    assert got[7] == RC.launch_plan(up, down, J), (sr_in, sr_out)
    return got[7]


def test_case_table(run):
    """Every row of the GPU case table: the (up, down, J) it claims, the path it names, and that path's block size,
    thread count and LDS floats."""
    for c, got in zip(RC.CASES, by_rates(run, [(c.sr_in, c.sr_out) for c in RC.CASES])):
        up, down, _, J = RC.ratio(c.sr_in, c.sr_out)
        assert (up, down, J) == (c.up, c.down, c.J), c.id
        assert O.resample_ratio(c.sr_in, c.sr_out) == RC.ratio(c.sr_in, c.sr_out), c.id  # the oracle's own rule
        pl = check_pair(got, c.sr_in, c.sr_out)
        assert pl.path == c.path and pl.status == RC.OK, (c.id, RC.PATH_NAMES[pl.path])
        want_block = {RC.PHASE: c.up * 16}.get(c.path, 1024)
        want_threads = {RC.PHASE: min(256, -(-c.up // 64) * 64)}.get(c.path, 256)
        want_lds = {RC.PHASE: (16 * c.up - 1) * c.down // c.up + c.J + 2,
                    RC.DECIMATE3: 1023 * 3 + 61 + 4}.get(c.path, 1023 * c.down // c.up + c.J + 2)
        assert (pl.block, pl.threads, pl.lds_floats) == (want_block, want_threads, want_lds), c.id
        assert pl.lds_floats * 4 <= 65536
    # what the rows are for, spelled out
    shape = {c.id: RC.launch_plan(c.up, c.down, c.J) for c in RC.CASES}
    assert shape["15to1"].lds_floats * 4 == 62592  # 62.6 KB
    assert [shape[i].threads for i in ("1to2", "65to64", "64to65", "256to257", "695to1024")] == [64, 64, 128, 256, 256]
    assert shape["765to1024"].lds_floats == 12262 and shape["481to2"].lds_floats == 12268
    assert RC.BY_ID["471to2"].J % 8 == 7 and RC.BY_ID["481to2"].J % 8 == 3
    assert -(-5 * 1025 // 1024) == 6  # 1 -> 1025: 5 input samples are 6 blocks
    assert {c.path for c in RC.CASES} == {RC.UNIFORM, RC.DECIMATE3, RC.PHASE, RC.GLOBAL_TAPS}


def test_rates_the_suite_already_runs(run):
    """The rate pairs of the older K6 tests keep the forms they had: eight phase pairs, one decimate3, one MODE 0,
    and MODE 2 with down == 1 for equal rates."""
    pairs = [(48000, 44100), (44100, 16000), (16000, 48000), (44100, 48000), (22050, 16000), (96000, 44100),
             (8000, 44100), (44100, 8000), (48000, 16000), (44101, 48000), (16000, 16000), (16000, 8000)]
    got = [check_pair(g, a, b).path for g, (a, b) in zip(by_rates(run, pairs), pairs)]
    assert got == [RC.PHASE] * 8 + [RC.DECIMATE3, RC.GLOBAL_TAPS, RC.UNIFORM, RC.UNIFORM]
    assert sorted({RC.ratio(a, b)[0] for a, b in pairs[:8]}) == [3, 80, 147, 160, 320, 441]


def test_boundaries(run):
    pairs = [(765, 1024), (767, 1024), (1, 1025), (15, 1), (16, 1), (471, 2), (473, 2), (481, 2), (483, 2),
             (1, 1024), (1, 1000000), (3, 1), (1, 1)]
    pl = {p: check_pair(g, *p) for p, g in zip(pairs, by_rates(run, pairs))}
    assert pl[(765, 1024)].path == RC.PHASE and pl[(767, 1024)].path == RC.GLOBAL_TAPS  # (up, down) = (1024, 765 / 767)
    assert 16383 * 765 // 1024 + 23 == 12262 <= 12288 < 16383 * 767 // 1024 + 23 == 12294
    assert pl[(1, 1024)].path == RC.PHASE and pl[(1, 1025)].path == RC.GLOBAL_TAPS  # up 1024 / 1025, both accepted
    assert pl[(15, 1)].path == RC.UNIFORM  # (1, 15): accepted
    assert pl[(16, 1)] == RC.Launch(RC.REJECT, RC.BAD_WINDOW, 0, 0, 0)  # (1, 16): 1023 * 16 + 323 floats = 66,764 B
    assert (1023 * 15 + 303) * 4 == 62592 <= 65536 < (1023 * 16 + 323) * 4 == 66764
    # up 2: phase through down 481 (see the module docstring for 473), refused from 483 on
    assert [pl[(d, 2)].path for d in (471, 473, 481)] == [RC.PHASE] * 3
    assert [31 * d // 2 + 10 * d + 3 for d in (471, 473, 481, 483)] == [12013, 12064, 12268, 12319]
    assert pl[(483, 2)] == RC.Launch(RC.REJECT, RC.BAD_WINDOW, 0, 0, 0)
    assert 1023 * 483 // 2 + 4833 == 251887  # floats: far above 64 KB
    up, down, _, J = RC.ratio(1, 1000000)
    assert up * J == 21000000 > 1 << 24 and RC.window_floats(up, down, J) == 23
    assert pl[(1, 1000000)] == RC.Launch(RC.REJECT, RC.BAD_TAPS, 0, 0, 0)
    assert pl[(3, 1)].path == RC.DECIMATE3 and pl[(1, 1)].path == RC.UNIFORM
    # the refusals the GPU test sends through the ABI are these
    for a, b, st in RC.REFUSED:
        assert RC.launch_plan(*RC.ratio(a, b)[:2], RC.ratio(a, b)[3]) == RC.Launch(RC.REJECT, st, 0, 0, 0)
    for a, b in RC.ACCEPTED_NEIGHBOURS:
        assert RC.launch_plan(*RC.ratio(a, b)[:2], RC.ratio(a, b)[3]).path != RC.REJECT


def test_plan_of_raw_triples(run):
    """resample_launch_plan on (up, down, J) given directly: decimate3 needs all three of (1, 3, 61), the window test
    comes before the table test, and the largest tap table that is accepted."""
    triples = [(1, 3, 61), (1, 3, 60), (1, 3, 62), (1, 4, 81), (2, 3, 31), (1 << 24, 1, 1), ((1 << 24) + 1, 1, 1),
               (798915, 1, 21), (798916, 1, 21), (1, 1 << 20, 20 * (1 << 20) + 1), (1024, 1, 21), (1025, 1, 21)]
    got = [RC.Launch(*map(int, t)) for t in run([f"plan {u} {d} {j}" for u, d, j in triples])]
    for t, g in zip(triples, got):
        assert g == RC.launch_plan(*t), t
    assert [g.path for g in got[:5]] == [RC.DECIMATE3, RC.UNIFORM, RC.UNIFORM, RC.UNIFORM, RC.PHASE]
    assert [g.status for g in got[5:10]] == [RC.OK, RC.BAD_TAPS, RC.OK, RC.BAD_TAPS, RC.BAD_WINDOW]
    assert 798915 * 21 <= 1 << 24 < 798916 * 21


def test_random_pairs(run):
    rng = random.Random(6)
    pairs = [(rng.randrange(1, 3000), rng.randrange(1, 3000)) for _ in range(3000)]
    pairs += [(rng.randrange(1, 200000), rng.randrange(1, 200000)) for _ in range(1000)]
    pairs += [(a, b) for a in (8000, 11025, 16000, 22050, 32000, 44100, 48000, 88200, 96000, 192000)
              for b in (8000, 16000, 22050, 44100, 48000)]
    seen = {check_pair(g, *p).path for p, g in zip(pairs, by_rates(run, pairs))}
    assert seen == {RC.REJECT, RC.DECIMATE3, RC.PHASE, RC.UNIFORM, RC.GLOBAL_TAPS}


def test_no_pair_could_stage_its_taps_in_lds(run):
    """MODE 1 of k_resample staged the [up][J] tap table in LDS when up > 1 and up * J <= 12288 floats, for pairs that
    do not take the phase form. up * J >= 2 hl + 1 = 20 max(up, down) + 1, so such a pair has up, down <= 614: the scan
    of all coprime pairs up to 614 is complete. Every pair in it either takes the phase form or is refused for its
    window, so no accepted launch could reach MODE 1 and it was removed. The program's path of every pair of the scan
    equals the rules restated in Python."""
    n = 614
    assert 20 * 615 + 1 > 12288 >= 20 * 614 + 1
    want, staged = [], []
    for up in range(1, n + 1):
        for down in range(1, n + 1):
            if math.gcd(up, down) != 1:
                continue
            _, _, _, J = RC.ratio(down, up)
            pl = RC.launch_plan(up, down, J)
            want.append(str(pl.path))
            if up > 1 and up * J <= 12288 and pl.path not in (RC.REJECT, RC.PHASE):
                staged.append((up, down, J))
    assert staged == []
    (got,) = run([f"scan {n}"])
    assert got[0] == "".join(want)
    assert set(got[0]) == {str(p) for p in (RC.REJECT, RC.DECIMATE3, RC.PHASE, RC.UNIFORM)}  # no MODE 0 this small
