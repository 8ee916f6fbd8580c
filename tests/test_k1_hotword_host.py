"""Host-side checks of audio-ident_amd/csrc/aidfp_hotword.h (compiled with g++, no GPU): how K1 reduces the 16
ballots of a power row, and bin 512's, to the row's hot word and to its 16 store guards. A stand-alone program runs
the header's packed composition with the portable restatement of the two scalar instructions, exactly as stft.hip
calls it (level-1 words, pairs in the kernel's register order 0, 4, 1, 5, ..., then hot_word and hot_stores), and the
per-register form it replaced. Both are compared with each other and with the hot word worked out here from the
definition alone (aidfp_layout.h hot_bit: chunk c = bins 16 c .. 16 c + 15, bit c below 32, else 95 - c)."""

import random
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = r"""
#include <cinttypes>
#include <cstdio>
#define __host__
#define __device__
#include "aidfp_hotword.h"
using namespace aid;
int main() {
    uint64_t d[8], m[9];
    for (;;) {
        for (int i = 0; i < 8; ++i) if (std::scanf("%" SCNx64, &d[i]) != 1) return 0;
        for (int i = 0; i < 9; ++i) if (std::scanf("%" SCNx64, &m[i]) != 1) return 2;
        uint32_t qd[8], qm[8], pd[4], pq[4], m0[9];
        for (int ii = 0; ii < 8; ++ii) {  // the kernel's order
            const int i = (ii >> 1) + 4 * (ii & 1);
            qd[i] = hot_quads<HotOpsPortable>(d[i]);
            qm[i] = hot_quads_mirror<HotOpsPortable>(m[i]);
            m0[i] = (uint32_t)m[i];
            if (i & 1) {
                pd[i >> 1] = hot_pair<HotOpsPortable>(qd[i - 1], qd[i]);
                pq[i >> 1] = hot_pair<HotOpsPortable>(qm[i - 1], qm[i]);
            }
        }
        m0[8] = (uint32_t)m[8];
        const uint64_t w = hot_word<HotOpsPortable>(pd, pq, m0);
        std::printf("%016" PRIx64 " %016" PRIx64 " %05x\n", w, hot_word_per_register<HotOpsPortable>(d, m),
                    hot_stores<HotOpsPortable>(w));
    }
}
"""


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("k1_hotword")
    (d / "hotword_check.cpp").write_text(SRC)
    exe = d / "hotword_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(ROOT / "audio-ident_amd" / "csrc"),
                    str(d / "hotword_check.cpp"), "-o", str(exe)], check=True)

    def run_(cases):
        text = "\n".join(" ".join(f"{v:x}" for v in dd + mm) for dd, mm in cases) + "\n"
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        rows = [r.split() for r in out.stdout.strip().split("\n")]
        assert len(rows) == len(cases)
        return [(int(a, 16), int(b, 16), int(c, 16)) for a, b, c in rows]

    return run_


# ---- the definition, restated
def hot_bit(c):
    return c if c < 32 else 95 - c


def hot_bins(dd, mm):
    """The bins a case calls hot: lane l of direct register i is bin 64 i + l, of mirror register i bin 1024 - 64 i - l
    (bin 1024, lane 0 of register 0, does not exist); every lane of ballot mm[8] is bin 512."""
    bins = set()
    for i in range(8):
        for l in range(64):
            if dd[i] >> l & 1:
                bins.add(64 * i + l)
            if mm[i] >> l & 1 and (i, l) != (0, 0):
                bins.add(1024 - 64 * i - l)
    if mm[8] & 1:
        bins.add(512)
    return bins


def want_word(bins):
    w = 0
    for b in bins:
        w |= 1 << hot_bit(b >> 4)
    return w


def want_stores(bins):
    """Bit 1 + i: direct store i writes bins 64 i .. 64 i + 63; bit 9 + i: mirror store i writes bins 1024 - 64 i - 63 ..
    1024 - 64 i (without bin 1024). A store is wanted when a chunk it writes into is hot (K2 reads whole hot chunks)."""
    chunks = {b >> 4 for b in bins}
    s = 0
    for i in range(8):
        if chunks & {(64 * i + l) >> 4 for l in range(64)}:
            s |= 2 << i
        if chunks & {(1024 - 64 * i - l) >> 4 for l in range(64) if (i, l) != (0, 0)}:
            s |= 0x200 << i
    return s


def check(run, cases):
    for (dd, mm), (packed, per_reg, stores) in zip(cases, run(cases)):
        bins = hot_bins(dd, mm)
        what = f"direct {[hex(v) for v in dd]} mirror {[hex(v) for v in mm]}"
        assert per_reg == want_word(bins), f"per-register form: {what}"
        assert packed == want_word(bins), f"packed form: {what}"
        assert stores == want_stores(bins), f"store guards: {what}"


def test_single_lanes(run):
    """Every single lane of every register alone (each decides one chunk bit and one store by itself), bin 512 alone,
    nothing at all, and everything."""
    cases = []
    for i in range(8):
        for l in range(64):
            cases.append(([1 << l if j == i else 0 for j in range(8)], [0] * 9))
            cases.append(([0] * 8, [1 << l if j == i else 0 for j in range(9)]))
    cases.append(([0] * 8, [0] * 8 + [(1 << 64) - 1]))
    cases.append(([0] * 8, [0] * 9))
    cases.append(([(1 << 64) - 1] * 8, [(1 << 64) - 1] * 9))
    check(run, cases)


def test_mirror_lane0(run):
    """Lane 0 of mirror register i is bin 1024 - 64 i: the last bin of chunk 64 - 4 i, whose other bins are lanes
    49 .. 63 of register i - 1. Alone, beside its neighbours in either register, and with everything but it; register
    0's lane 0 (no bin) must change nothing, whatever else is set."""
    full = (1 << 64) - 1
    cases = []
    for i in range(8):
        for other in (0, 2, 1 << 63, full & ~1):
            m = [0] * 9
            m[i] = 1 | other
            cases.append(([0] * 8, m))
            m = [full & ~1] * 8 + [0]
            m[i] = other
            cases.append(([0] * 8, m))
    cases.append(([0] * 8, [1] * 8 + [0]))
    cases.append(([0] * 8, [1] + [0] * 8))
    cases.append(([full] * 8, [full & ~1] * 8 + [0]))  # all but bins 512 and the lane-0 bins
    # bits of bin 512's ballot above lane 0 are other lanes' copies of the same bin: lane 0 decides
    cases.append(([0] * 8, [0] * 8 + [full & ~1]))
    check(run, cases)


def test_random(run):
    rng = random.Random(20261021)
    cases = []
    for n in range(600):
        dens = rng.choice([1, 2, 4, 16, 32, 60])  # expected set lanes per ballot
        word = lambda: sum(1 << l for l in range(64) if rng.randrange(64) < dens) if rng.random() < 0.7 else 0
        cases.append(([word() for _ in range(8)], [word() for _ in range(8)] + [rng.choice([0, (1 << 64) - 1])]))
    check(run, cases)
