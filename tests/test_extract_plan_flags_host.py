"""Host-side check of the row-flag layout in audio-ident_amd/csrc/aidfp_extract_plan.h (g++, no GPU): the flag base
and strip length plan_extract puts into every ClipDesc, the groups' bases and the call's total, over the plan cases of
test_extract_plan_host.py. Expected values are restated here from csrc/aidfp_layout.h's comment: a strip of length L
takes 4 * ceil(L / 32) words, strips lie in order within a group, groups in order within the call."""

import shutil
import subprocess
from pathlib import Path

import pytest

from test_extract_plan_host import DEVICE, PLANE_ROWS, SLOTS, ceil_div, num_frames, plan_cases, plan_line, strip_len

ROOT = Path(__file__).resolve().parent.parent
SRC = r"""
#include <cstdio>
#include <iostream>
#include <string>
#define __host__
#define __device__
#include "aidfp_extract_plan.h"
using namespace aid;
int main() {
    static_assert(sizeof(ClipDesc) == 80, "ten int64 fields, no padding: desc_differ compares whole bytes");
    ExtractPlan p;
    std::string cmd;
    while (std::cin >> cmd) {
        int hop, loc, keep, width, n, has_ends;
        int64_t rows, slots;
        double mult;
        std::cin >> hop >> loc >> rows >> keep >> slots >> mult >> width >> n >> has_ends;
        std::vector<int64_t> off(n + 1), ends(has_ends ? n : 0);
        for (auto &x : off) std::cin >> x;
        for (auto &x : ends) std::cin >> x;
        plan_extract(p, off.data(), has_ends ? ends.data() : nullptr, n, loc, hop, rows, keep != 0, slots, mult, width);
        std::printf("%lld %zu", (long long)p.flag_words, p.groups.size());
        for (const ClipGroup &g : p.groups)
            std::printf(" %d %d %d %lld", g.first, g.n, g.strip_len, (long long)g.flag_base);
        for (int c = 0; c < n; ++c)
            std::printf(" %lld %lld", (long long)p.desc[c].flag_base, (long long)p.desc[c].strip_len);
        std::printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("extract_plan_flags")
    (d / "flags_check.cpp").write_text(SRC)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(ROOT / "audio-ident_amd" / "csrc"),
                    str(d / "flags_check.cpp"), "-o", str(d / "flags_check")], check=True)
    return d / "flags_check"


def test_flag_layout(exe):
    cases = [dict(dict(ends=None, loc=DEVICE, hop=512, rows=0, keep=0, slots=SLOTS, mult=1.0, width=4), **c)
             for c in plan_cases()]
    out = subprocess.run([str(exe)], input="\n".join(plan_line(**c) for c in cases) + "\n", capture_output=True,
                         text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().split("\n")
    assert len(lines) == len(cases)
    multi = 0
    for c, line in zip(cases, lines):
        v = [int(t) for t in line.split()]
        n = len(c["offsets"]) - 1
        end = [c["ends"][i] if c["ends"] else c["offsets"][i + 1] for i in range(n)]
        F = [num_frames(end[i] - c["offsets"][i], c["hop"]) for i in range(n)]
        total, ng = v[0], v[1]
        groups = [v[2 + 4 * g:6 + 4 * g] for g in range(ng)]
        desc = [v[2 + 4 * ng + 2 * i:4 + 4 * ng + 2 * i] for i in range(n)]
        words = 0
        for first, cnt, L, base in groups:
            assert L == strip_len(F[first:first + cnt], max(1, int(c["slots"] * c["mult"])))
            assert base == words and base % 4 == 0  # 16-byte units
            per = 4 * ceil_div(L, 32)
            for i in range(first, first + cnt):
                assert desc[i] == [words, L]
                words += ceil_div(F[i], L) * per
        assert total == words
        multi += ng > 1 and len({g[2] for g in groups}) > 1
    assert multi > 0  # some case has groups of different strip lengths
    assert PLANE_ROWS == 3 << 18
