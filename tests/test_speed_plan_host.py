"""Host-side checks of audio-ident_amd/csrc/aidfp_speed_plan.h (compiled with g++, no GPU): the planning half of the
speed fan-out (spec/FPSPEC.md 8.2). One stand-alone program reads cases and prints what the header computes: the
ResamplePlan of a speed, variant lengths, the packed offsets, block prefix sums and clip groups of a call, the pair
speed_find_pair gives every block id, and the status of what the plan rejects. Every expected value is restated here
in Python from the spec (rate pair (sr_in * 1000, sr_e * (1000 + pm)), gcd reduction, hl = 10 * max(up, down),
J = ceil((2 hl + 1) / up), n_out = ceil(n up / down)) or comes from the CPU oracle's resample_ratio; none is taken
from the program's output. The same cases run a second time through a build with -fsanitize=address,undefined (the
sanitizer's runtime linked statically into the program, which has its own main)."""

import math
import random
import shutil
import subprocess
from pathlib import Path

import pytest

import oracle as O

ROOT = Path(__file__).resolve().parent.parent
SRC = r"""
#include <cstdio>
#include <iostream>
#include <string>
#include "aidfp_speed_plan.h"
using namespace aid;
int main() {
    SpeedPlan p;  // reused by every plan case, as the engine reuses its own
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "var") {
            int sr_in, sr_e, pm;
            std::cin >> sr_in >> sr_e >> pm;
            ResamplePlan r;
            const int st = speed_variant(sr_in, sr_e, pm, r);
            std::printf("var %d %d %d %d %d\n", st, r.up, r.down, r.hl, r.J);
        } else if (cmd == "len") {
            long long n;
            int sr_in, sr_e, pm;
            std::cin >> n >> sr_in >> sr_e >> pm;
            ResamplePlan r;
            if (speed_variant(sr_in, sr_e, pm, r)) return 4;
            std::printf("len %lld\n", (long long)speed_len(n, r));
        } else if (cmd == "plan") {
            int sr_in, sr_e, ns, nc;
            long long budget;
            std::cin >> sr_in >> sr_e >> budget >> ns;
            std::vector<int32_t> pm(ns > 0 ? ns : 0);
            for (auto &x : pm) std::cin >> x;
            std::cin >> nc;
            std::vector<int64_t> off(nc + 1);
            for (auto &x : off) std::cin >> x;
            const int st = plan_speeds(p, off.data(), nc, sr_in, sr_e, pm.data(), ns, budget);
            std::printf("plan %d", st);
            if (st == kSpeedOk) {
                const size_t np = (size_t)nc * ns;
                if (p.dst_off.size() != np + 1 || p.blk_first.size() != np + 1 || p.clip_off.size() != (size_t)nc + 1 ||
                    p.var.size() != (size_t)ns)
                    return 2;
                std::printf(" %lld %lld %lld %zu", (long long)p.total(), (long long)p.blocks(), (long long)p.lds_floats,
                            p.groups.size());
                for (const SpeedGroup &g : p.groups) std::printf(" %d %d %lld", g.first, g.n, (long long)g.floats);
                for (int64_t x : p.clip_off) std::printf(" %lld", (long long)x);
                for (int64_t x : p.dst_off) std::printf(" %lld", (long long)x);
                for (int64_t x : p.blk_first) std::printf(" %lld", (long long)x);
                // the pair of every block id, found as K6s finds it
                for (int64_t b = 0; b < p.blocks(); ++b)
                    std::printf(" %d", speed_find_pair(p.blk_first.data(), (int)np, b));
            }
            std::printf("\n");
        } else {
            return 3;
        }
    }
    std::printf("consts %d %d %d %d %lld %lld %lld\n", kSpeedMin, kSpeedMax, kSpeedMaxVariants, kSpeedBlock,
                (long long)kSpeedGroupFloats, (long long)kSpeedMaxLds, (long long)kSpeedMaxTaps);
    return 0;
}
"""

OK, BAD_RATES, BAD_COUNT, BAD_SPEED, BAD_WINDOW, BAD_TAPS, BAD_CLIPS = range(7)  # SpeedStatus
BLOCK = 1024  # outputs of one K6s workgroup
GROUP_FLOATS = 1 << 28  # 1 GiB of variant PCM per clip group
SR_E = 16000
SPEEDS = (-500, -40, -1, 0, 1, 7, 13, 40, 1000)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def run(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("speed_plan_" + request.param)
    (d / "speed_check.cpp").write_text(SRC)
    exe = d / "speed_check"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *(san if request.param == "sanitized" else []),
                    "-I", str(ROOT / "audio-ident_amd" / "csrc"), str(d / "speed_check.cpp"), "-o", str(exe)],
                   check=True)

    def run_(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        rows = out.stdout.strip().split("\n")
        assert rows[-1] == f"consts -500 1000 256 {BLOCK} {GROUP_FLOATS} 65536 {1 << 24}"
        assert len(rows) == len(lines) + 1
        return [r.split()[1:] for r in rows[:-1]]

    return run_


# ---- the rules, restated
def ceil_div(a, b):
    return -(-a // b)


def rates(sr_in, sr_e, pm):  # FPSPEC 8.2
    return sr_in * 1000, sr_e * (1000 + pm)


def ratio(sr_in, sr_e, pm):  # FPSPEC 8: gcd reduction, hl = 10 max(up, down), J = ceil((2 hl + 1) / up)
    a, b = rates(sr_in, sr_e, pm)
    g = math.gcd(a, b)
    up, down = b // g, a // g
    hl = 10 * max(up, down)
    return up, down, hl, ceil_div(2 * hl + 1, up)


def variant_len(n, up, down):
    return ceil_div(n * up, down) if n > 0 else 0


def window_floats(up, down, J):  # input samples of 1,024 consecutive outputs, + 2
    return (BLOCK - 1) * down // up + J + 2


def test_variants_equal_the_oracle_ratio(run):
    cases = [(sr_in, pm) for sr_in in (16000, 44100, 48000) for pm in SPEEDS]
    out = run([f"var {sr_in} {SR_E} {pm}" for sr_in, pm in cases])
    for (sr_in, pm), tok in zip(cases, out):
        got = [int(t) for t in tok]
        a, b = rates(sr_in, SR_E, pm)
        assert got[0] == OK, (sr_in, pm)
        assert tuple(got[1:]) == O.resample_ratio(a, b) == ratio(sr_in, SR_E, pm), (sr_in, pm)
    assert ratio(44100, SR_E, 7)[0] == 4028  # the large-up path: above the phase-major kernels' 1,024
    assert ratio(16000, SR_E, 0)[:2] == (1, 1)  # up == down


def test_lengths(run):
    cases = []
    for sr_in in (16000, 44100, 48000):
        for pm in SPEEDS:
            up, down, _, J = ratio(sr_in, SR_E, pm)
            cases += [(n, sr_in, pm, up, down) for n in (0, 1, J - 1, 1023, 1024, 1025, 80000)]
    out = run([f"len {n} {sr_in} {SR_E} {pm}" for n, sr_in, pm, _, _ in cases])
    for (n, sr_in, pm, up, down), tok in zip(cases, out):
        assert int(tok[0]) == variant_len(n, up, down), (n, sr_in, pm)
    # a 5 s clip: its -40 variant is 4.8 s long (sub-window mode), its +40 variant 5.2 s (the lane's whole-clip mode)
    assert variant_len(80000, *ratio(16000, SR_E, -40)[:2]) == 76800
    assert variant_len(80000, *ratio(16000, SR_E, 40)[:2]) == 83200


def plan_line(sr_in, sr_e, budget, speeds, offsets):
    return " ".join(map(str, ["plan", sr_in, sr_e, budget, len(speeds), *speeds, len(offsets) - 1, *offsets]))


def parse_plan(tok, nc, ns):
    v = [int(t) for t in tok]
    if v[0] != OK:
        assert len(v) == 1
        return {"status": v[0]}
    ng, np_ = v[4], nc * ns
    k = 5 + 3 * ng
    res = {"status": OK, "total": v[1], "blocks": v[2], "lds": v[3], "groups": [v[5 + 3 * g:8 + 3 * g] for g in range(ng)],
           "clip_off": v[k:k + nc + 1], "dst_off": v[k + nc + 1:k + nc + 1 + np_ + 1],
           "blk_first": v[k + nc + np_ + 2:k + nc + 2 * np_ + 3], "pair_of": v[k + nc + 2 * np_ + 3:]}
    assert len(res["pair_of"]) == res["blocks"]
    return res


def check_plan(got, sr_in, sr_e, budget, speeds, offsets):
    nc, ns = len(offsets) - 1, len(speeds)
    var = [ratio(sr_in, sr_e, pm) for pm in speeds]
    lens = [offsets[c + 1] - offsets[c] for c in range(nc)]
    n_out = [variant_len(lens[c], *var[v][:2]) for c in range(nc) for v in range(ns)]  # pair = clip * n_speeds + v
    assert got["status"] == OK
    assert got["clip_off"] == [o - offsets[0] for o in offsets]
    # offsets packed and monotone, the last equals the total
    assert got["dst_off"][0] == 0 and got["dst_off"][-1] == got["total"] == sum(n_out)
    assert [b - a for a, b in zip(got["dst_off"], got["dst_off"][1:])] == n_out
    assert got["blk_first"][0] == 0 and got["blk_first"][-1] == got["blocks"]
    assert [b - a for a, b in zip(got["blk_first"], got["blk_first"][1:])] == [ceil_div(m, BLOCK) for m in n_out]
    assert got["lds"] == max(window_floats(up, down, J) for up, down, _, J in var)
    # every block id maps back to exactly one pair and one in-range output block
    want_pairs = [p for p, m in enumerate(n_out) for _ in range(ceil_div(m, BLOCK))]
    assert got["pair_of"] == want_pairs
    for b, p in enumerate(got["pair_of"]):
        first_out = (b - got["blk_first"][p]) * BLOCK
        assert 0 <= first_out < n_out[p]
    # groups partition the clips in order, never split a clip, and exceed the budget only as a single clip
    cap = budget or GROUP_FLOATS
    per_clip = [sum(n_out[c * ns:(c + 1) * ns]) for c in range(nc)]
    groups, cur = [], []
    for c in range(nc):
        if cur and sum(per_clip[i] for i in cur) + per_clip[c] > cap:
            groups.append(cur)
            cur = []
        cur.append(c)
    groups.append(cur)
    assert got["groups"] == [[g[0] if g else 0, len(g), sum(per_clip[i] for i in g)] for g in groups]
    assert sum(g[1] for g in got["groups"]) == nc
    for g in got["groups"]:
        assert g[2] <= cap or g[1] == 1


def layout(lens, first=0):
    offs = [first]
    for n in lens:
        offs.append(offs[-1] + n)
    return offs


def plan_cases():
    grid = (-30, -20, -2, 0, 2, 12, 14, 20, 22)
    lens = [1, 60, 1023, 1024, 1025, 16001]
    cases = [dict(sr_in=48000, speeds=(-40, -1, 0, 1, 7, 40), offsets=layout(lens, 5)),
             dict(sr_in=16000, speeds=(-40, -1, 0, 1, 7, 40), offsets=layout(lens)),
             dict(sr_in=44100, speeds=(7,), offsets=layout(lens)),
             dict(sr_in=48000, speeds=(0,), offsets=layout([4000])),
             dict(sr_in=48000, speeds=grid, offsets=[3]),  # no clip
             dict(sr_in=48000, speeds=grid, offsets=layout([0, 0, 0])),  # no frames at all
             dict(sr_in=48000, speeds=grid, offsets=layout([0, 5000, 0, 7000, 0])),
             dict(sr_in=48000, speeds=(2, 2, -2, 2), offsets=layout([3000, 100])),  # a duplicated speed
             dict(sr_in=16000, speeds=SPEEDS, offsets=layout([2500, 1, 999]))]
    # groups: budgets around the clips' own variant totals, a one-clip group over budget, budget 1
    for budget in (1, 20000, 47000, 47500, 100000, 10 ** 9):
        cases.append(dict(sr_in=48000, speeds=grid, offsets=layout([15000, 16000, 200000, 300, 0, 15000, 15000]),
                          budget=budget))
    rng = random.Random(5)
    for _ in range(40):
        ns = rng.randrange(1, 7)
        cases.append(dict(sr_in=rng.choice((16000, 44100, 48000)),
                          speeds=tuple(rng.randrange(-60, 61) for _ in range(ns)),
                          offsets=layout([rng.choice((0, 1, 59, 1024, rng.randrange(0, 9000))) for _ in
                                          range(rng.randrange(0, 9))], rng.randrange(0, 5)),
                          budget=rng.choice((0, 1, 3000, 30000))))
    return [dict(dict(sr_e=SR_E, budget=0), **c) for c in cases]


def test_plans(run):
    cases = plan_cases()
    out = run([plan_line(**c) for c in cases])
    for c, tok in zip(cases, out):
        check_plan(parse_plan(tok, len(c["offsets"]) - 1, len(c["speeds"])), **c)


def test_groups_named(run):
    """The shapes the groups exist for, spelled out: three clips of 10,000 variant samples each (one speed, same rate)."""
    offs = layout([10000, 10000, 10000])
    line = lambda budget: plan_line(16000, SR_E, budget, (0,), offs)
    out = run([line(0), line(30000), line(29999), line(10000), line(9999), line(1)])
    groups = [parse_plan(t, 3, 1)["groups"] for t in out]
    assert groups[0] == groups[1] == [[0, 3, 30000]]
    assert groups[2] == [[0, 2, 20000], [2, 1, 10000]]
    assert groups[3] == groups[4] == groups[5] == [[0, 1, 10000], [1, 1, 10000], [2, 1, 10000]]  # over budget: allowed


def test_rejections(run):
    lines = [
        plan_line(48000, SR_E, 0, (), [0, 100]),  # n_speeds 0
        plan_line(48000, SR_E, 0, tuple(range(257)), [0, 100]),  # n_speeds 257
        plan_line(48000, SR_E, 0, tuple(range(-128, 128)), [0, 100]),  # 256: allowed
        plan_line(48000, SR_E, 0, (0, -501), [0, 100]),
        plan_line(48000, SR_E, 0, (1001,), [0, 100]),
        plan_line(48000, SR_E, 0, (-500, 1000), [0, 100]),  # the ends of the range: allowed
        plan_line(0, SR_E, 0, (0,), [0, 100]),
        plan_line(48000, -1, 0, (0,), [0, 100]),
        plan_line(2147484, SR_E, 0, (0,), [0, 100]),  # sr_in * 1000 = 2^31 + 352: beyond int32
        plan_line(2147483, SR_E, 0, (0,), [0, 0]),  # 2,147,483,000 fits; its tap table does not (below)
        plan_line(48000, 1073742, 0, (1000,), [0, 100]),  # sr_e * 2000 beyond int32
        plan_line(384000, SR_E, 0, (-500,), [0, 100]),  # 48 : 1 -> a window of 50,067 floats
        plan_line(2000003, 384000, 0, (1,), [0, 100]),  # up 384,384, down 2,000,003: 20 * 2,000,003 + 1 taps > 2^24
        plan_line(48000, SR_E, 0, (0,), [0, 100, 50]),  # offsets decrease
    ]
    st = [int(t[0]) for t in run(lines)]
    assert st == [BAD_COUNT, BAD_COUNT, OK, BAD_SPEED, BAD_SPEED, OK, BAD_RATES, BAD_RATES, BAD_RATES, BAD_TAPS,
                  BAD_RATES, BAD_WINDOW, BAD_TAPS, BAD_CLIPS]
    # the same, restated: the window and the table of the two rejected rate pairs
    up, down, _, J = ratio(384000, SR_E, -500)
    assert (up, down) == (1, 48) and window_floats(up, down, J) * 4 > 65536 and up * J <= 1 << 24
    up, down, _, J = ratio(2000003, 384000, 1)
    assert up * J > 1 << 24 and window_floats(up, down, J) * 4 <= 65536
    out = run(["var 384000 16000 -500", "var 48000 16000 -501", "var 48000 16000 2"])
    assert [int(t[0]) for t in out] == [BAD_WINDOW, BAD_SPEED, OK]
