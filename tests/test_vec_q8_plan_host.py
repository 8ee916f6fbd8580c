"""Host-side checks of audio-ident_amd/csrc/aidfp_vector_q8.h (compiled with g++, no GPU): the int8 tile layout, the
candidate count R and the bound eps of spec/FPSPEC.md 9.1. One stand-alone program with its own main reads cases and
prints what the header computes; the expected values are restated here or come from tests/vec_q8_ref.py, none from the
program's output. The same cases run a second time through a build with -fsanitize=address,undefined (the sanitizer's
runtime linked statically into the program): `fill` writes a whole catalog through the layout index into a buffer of
exactly rows * dim bytes, so an index out of range is a heap overflow there."""

import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import vec_q8_ref as Q

ROOT = Path(__file__).resolve().parent.parent
SRC = r"""
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>
#include "aidfp_vector_q8.h"
using namespace aid;
int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "idx") {
            long long row;
            int k, dim;
            std::cin >> row >> k >> dim;
            std::printf("idx %zu\n", vec_q8_layout_index(row, k, dim));
        } else if (cmd == "fill") {  // every (row, k) of a [rows][dim] catalog lands on its own byte of rows * dim
            int rows, dim;
            std::cin >> rows >> dim;
            std::vector<unsigned char> seen((size_t)rows * dim, 0);
            long long twice = 0;
            for (int r = 0; r < rows; ++r)
                for (int k = 0; k < dim; ++k) twice += seen[vec_q8_layout_index(r, k, dim)]++;
            long long empty = 0;
            for (unsigned char c : seen) empty += c == 0;
            std::printf("fill %lld %lld\n", twice, empty);
        } else if (cmd == "lane") {  // the 16 bytes of lane (i, h), k-step st, tile t: one aligned run
            long long t;
            int st, i, h, dim;
            std::cin >> t >> st >> i >> h >> dim;
            const size_t first = vec_q8_layout_index(t * 32 + i, st * 32 + h * 16, dim);
            int ok = first % 16 == 0;
            for (int j = 0; j < 16; ++j) ok = ok && vec_q8_layout_index(t * 32 + i, st * 32 + h * 16 + j, dim) == first + j;
            std::printf("lane %zu %d\n", first, ok);
        } else if (cmd == "cand") {
            int limit, over;
            std::cin >> limit >> over;
            std::printf("cand %d\n", vec_q8_candidates(limit, over));
        } else if (cmd == "eps") {
            float eq, E;
            int dim;
            std::cin >> eq >> E >> dim;
            std::printf("eps %a\n", vec_q8_eps(eq, E, dim));
        } else {
            return 3;
        }
    }
    std::printf("consts %d %d %d\n", kVecQ8MaxR, kVecQ8MaxOversample, kVecQ8Stats);
    return 0;
}
"""


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def run(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("vec_q8_plan_" + request.param)
    (d / "q8_check.cpp").write_text(SRC)
    exe = d / "q8_check"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off",
                    *(san if request.param == "sanitized" else []),
                    "-I", str(ROOT / "audio-ident_amd" / "csrc"), str(d / "q8_check.cpp"), "-o", str(exe)], check=True)

    def run_(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        rows = out.stdout.strip().split("\n")
        assert rows[-1] == "consts 1024 64 6"
        assert len(rows) == len(lines) + 1
        return [r.split()[1:] for r in rows[:-1]]

    return run_


def layout_index(row, k, dim):
    """FPSPEC 9.1's layout, restated: tile, k-step of 32, half of 16, row, byte."""
    return (row // 32) * 32 * dim + (k // 32) * 1024 + ((k // 16) % 2) * 512 + (row % 32) * 16 + k % 16


def test_layout_index_known_answers(run):
    cases = [(0, 0, 32), (0, 15, 32), (0, 16, 32), (1, 0, 32), (31, 31, 32), (32, 0, 32), (33, 17, 64), (299, 511, 512),
             (499_999, 1023, 1024), (2**32 - 3, 511, 512)]  # the last: the byte offset is past 2^40
    rows = run([f"idx {r} {k} {d}" for r, k, d in cases])
    assert [int(x[0]) for x in rows] == [layout_index(*c) for c in cases]
    assert layout_index(2**32 - 3, 511, 512) > 2**40


@pytest.mark.parametrize("dim", [32, 64, 96, 512, 1024])
def test_layout_is_a_bijection_onto_the_buffer(run, dim):
    assert run([f"fill 64 {dim}", f"fill 32 {dim}"]) == [["0", "0"], ["0", "0"]]


def test_a_lane_reads_sixteen_aligned_bytes_and_a_wave_one_kilobyte(run):
    dim = 512
    lines, want = [], []
    for t, st in ((0, 0), (3, 15), (15624, 7)):
        for i, h in ((0, 0), (31, 0), (0, 1), (17, 1)):
            lines.append(f"lane {t} {st} {i} {h} {dim}")
            want.append([str(t * 32 * dim + st * 1024 + (h * 32 + i) * 16), "1"])  # lane h * 32 + i of the wave
    assert run(lines) == want


def test_candidate_count(run):
    cases = [(1, 1), (1, 64), (50, 4), (300, 4), (1024, 1), (1024, 64), (5, 64), (17, 60), (16, 64), (17, 61)]
    got = [int(r[0]) for r in run([f"cand {a} {b}" for a, b in cases])]
    assert got == [min(1024, max(a, a * b)) for a, b in cases] == [Q.candidates(a, b) for a, b in cases]


def test_eps_is_the_oracles(run):
    rng = np.random.default_rng(9)
    cases = [(0.0, 0.0, 32), (0.0, 0.0, 1024), (1.0, 1.0, 512), (0.0078125, 0.0078125, 512)]
    cases += [(float(np.float32(a)), float(np.float32(b)), int(d)) for a, b, d in
              zip(rng.uniform(0, 0.1, 40), rng.uniform(0, 0.1, 40), rng.choice([32, 64, 512, 1024], 40))]
    rows = run([f"eps {a!r} {b!r} {d}" for a, b, d in cases])  # a float32's value, printed exactly, reads back to it
    for (a, b, d), row in zip(cases, rows):
        assert float.fromhex(row[0]) == float(Q.eps(np.float32(a), np.float32(b), d)), (a, b, d)
    assert float.fromhex(rows[0][0]) == 32 * 2.0**-21 and float.fromhex(rows[2][0]) == 3 * (1 + 2.0**-10) + 512 * 2.0**-21
