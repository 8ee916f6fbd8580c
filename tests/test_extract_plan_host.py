"""Host-side checks of audio-ident_amd/csrc/aidfp_extract_plan.h (compiled with g++, no GPU): the planning half of
extraction. One stand-alone program reads cases and prints what the header computes: plan_extract's descriptors,
clip groups, totals and K3 flags; K2Policy's width and strips-per-slot multiplier over a trace of counter words;
desc_differ, the descriptor cache's criterion. Every expected value is restated here in Python from spec/FPSPEC.md
(frame and record counts), DESIGN.md (clip groups, strips, the cache) and the policy's comment in the header; none
is taken from the program's output."""

import random
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = r"""
#include <cstdio>
#include <iostream>
#include <string>
#define __host__
#define __device__
#include "aidfp_extract_plan.h"
using namespace aid;
static std::vector<int64_t> read_vec(int n) { std::vector<int64_t> v(n); for (auto &x : v) std::cin >> x; return v; }
static std::vector<ClipDesc> read_desc(int n) {
    std::vector<ClipDesc> d(n);
    for (auto &x : d) std::cin >> x.pcm_off >> x.frames >> x.frame_base >> x.strip_base >> x.chunk_base >> x.hash_base
                               >> x.hash_cap >> x.stft_base;
    return d;
}
int main() {
    ExtractPlan p;  // reused by every plan case, as the engine reuses its own
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "plan") {
            int hop, loc, keep, width, n, has_ends;
            int64_t rows, slots;
            double mult;
            std::cin >> hop >> loc >> rows >> keep >> slots >> mult >> width >> n >> has_ends;
            std::vector<int64_t> off = read_vec(n + 1), ends = read_vec(has_ends ? n : 0);
            plan_extract(p, off.data(), has_ends ? ends.data() : nullptr, n, loc, hop, rows, keep != 0, slots, mult, width);
            std::printf("plan %d %d %zu %lld %lld %lld %lld %lld %d %d %d", p.n_clips, p.width, p.groups.size(),
                        (long long)p.total_frames, (long long)p.strips, (long long)p.chunks, (long long)p.records,
                        (long long)p.staged, (int)p.empty_clip, (int)p.multi_chunk, (int)p.one_chunk_each);
            for (const ClipGroup &g : p.groups)
                std::printf(" %d %d %lld %lld %lld %d %lld", g.first, g.n, (long long)g.frame0, (long long)g.frames,
                            (long long)g.strips, g.strip_len, (long long)g.k1_strips);
            if (p.desc.size() != (size_t)n || p.frames.size() != (size_t)n || p.hash_base.size() != (size_t)n) return 2;
            for (int c = 0; c < n; ++c) {
                const ClipDesc &d = p.desc[c];
                std::printf(" %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", (long long)d.pcm_off, (long long)d.frames,
                            (long long)d.frame_base, (long long)d.strip_base, (long long)d.chunk_base,
                            (long long)d.hash_base, (long long)d.hash_cap, (long long)d.stft_base,
                            (long long)p.frames[c], (long long)p.hash_base[c]);
            }
            std::printf("\n");
        } else if (cmd == "policy") {  // steps of (force_width, force_strips_x100, cw, sw) on one fresh policy
            int n;
            std::cin >> n;
            K2Policy k;
            std::printf("policy %d %d", k.width, k.hold);
            for (int i = 0; i < n; ++i) {
                int fw, fx;
                uint64_t cw, sw;
                std::cin >> fw >> fx >> cw >> sw;
                k.force_width = fw;
                k.force_slots_x = fx / 100.0;
                const K2Choice ch = k.choose(cw, sw);
                std::printf(" %d %.4f %d", ch.width, ch.slots_x, k.width);
            }
            std::printf("\n");
        } else if (cmd == "differ") {
            int na, nb;
            std::cin >> na >> nb;
            std::vector<ClipDesc> a = read_desc(na), b = read_desc(nb);
            std::printf("differ %d\n", (int)desc_differ(a.data(), a.size(), b.data(), b.size()));
        } else {
            return 3;
        }
    }
    std::printf("kPlaneRows %lld kK2Hold %d\n", (long long)kPlaneRows, kK2Hold);
    return 0;
}
"""

HOST, DEVICE = 0, 1  # AID_PCM_HOST, AID_PCM_DEVICE (include/aidfp.h)
PLANE_ROWS = 3 << 18  # 786,432 power rows, 3 GB of plane
SLOTS = 1024  # 256 CUs x 4 resident K2 workgroups: the order of the real device's


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("extract_plan")
    (d / "plan_check.cpp").write_text(SRC)
    exe = d / "plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(ROOT / "audio-ident_amd" / "csrc"),
                    str(d / "plan_check.cpp"), "-o", str(exe)], check=True)

    def run_(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        rows = out.stdout.strip().split("\n")
        assert rows[-1] == f"kPlaneRows {PLANE_ROWS} kK2Hold 64"
        assert len(rows) == len(lines) + 1
        return [r.split()[1:] for r in rows[:-1]]

    return run_


# ---- the rules, restated
def num_frames(n, hop):  # FPSPEC 1: frames of 2048 samples every hop samples, none for a shorter clip
    return 0 if n < 2048 else 1 + (n - 2048) // hop


def ceil_div(a, b):
    return -(-a // b)


def hash_capacity(F):  # 10 targets per anchor, 64 peaks per 8 frames
    return 10 * 64 * ceil_div(F, 8)


def strip_len(frames, slots):
    """The smallest L >= 16 at which the clips' strips fit the slots; when none does, the longest clip (one strip per
    clip), at least 16 and at most 65536 (aidfp_layout.h peak_strip_len)."""
    hi = min(max([16] + frames), 65536)
    for L in range(16, hi):
        if sum(ceil_div(F, L) for F in frames) <= slots:
            return L
    return hi


def model(offsets, ends, loc, hop, rows, keep, slots, mult):
    n = len(offsets) - 1
    end = [ends[c] if ends else offsets[c + 1] for c in range(n)]
    F = [num_frames(end[c] - offsets[c], hop) for c in range(n)]
    cap = rows if rows > 0 else PLANE_ROWS
    groups, cur = [], []
    for c in range(n):  # consecutive clips while their frames fit the cap; keep-power: one group
        if not keep and cur and sum(F[i] for i in cur) > 0 and sum(F[i] for i in cur) + F[c] > cap:
            groups.append(cur)
            cur = []
        cur.append(c)
    groups.append(cur)
    per_slot = max(1, int(slots * mult))
    chunks = [ceil_div(f, 1024) for f in F]
    k1 = [ceil_div(f, 16) for f in F]
    desc, gout = [None] * n, []
    for g in groups:
        L = strip_len([F[c] for c in g], per_slot)
        first = g[0] if g else n
        gout.append([first, len(g), sum(F[:first]), sum(F[c] for c in g), sum(ceil_div(F[c], L) for c in g), L,
                     sum(k1[c] for c in g)])
        for c in g:
            desc[c] = [offsets[c] if loc == DEVICE else offsets[c] - offsets[0], F[c], sum(F[:c]),
                       sum(ceil_div(F[i], L) for i in g if i < c), sum(chunks[:c]),
                       sum(hash_capacity(f) for f in F[:c]), hash_capacity(F[c]), sum(k1[:c])]
    return {
        "groups": gout, "desc": desc, "frames": F,
        "totals": [sum(F), sum(g[4] for g in gout), sum(chunks), sum(hash_capacity(f) for f in F),
                   end[-1] - offsets[0] if loc == HOST and n else 0],
        "flags": [int(any(f == 0 for f in F)), int(any(k > 1 for k in chunks)), int(n > 0 and all(k == 1 for k in chunks))],
    }


def plan_line(offsets, ends=None, loc=DEVICE, hop=512, rows=0, keep=0, slots=SLOTS, mult=1.0, width=4):
    n = len(offsets) - 1
    return " ".join(map(str, ["plan", hop, loc, rows, keep, slots, repr(float(mult)), width, n, int(ends is not None),
                              *offsets, *(ends or [])]))


def parse_plan(tok, n):
    v = [int(t) for t in tok]
    ng = v[2]
    return {"n": v[0], "width": v[1], "totals": v[3:8], "flags": v[8:11],
            "groups": [v[11 + 7 * g:18 + 7 * g] for g in range(ng)],
            "desc": [v[11 + 7 * ng + 10 * c:19 + 7 * ng + 10 * c] for c in range(n)],
            "frames": [v[19 + 7 * ng + 10 * c] for c in range(n)],
            "hash_base": [v[20 + 7 * ng + 10 * c] for c in range(n)]}


def check_plan(got, offsets, ends, loc, hop, rows, keep, slots, mult, width):
    n = len(offsets) - 1
    want = model(offsets, ends, loc, hop, rows, keep, slots, mult)
    F = want["frames"]
    assert (got["n"], got["width"]) == (n, width)
    # groups partition the clips in order; one exceeds the cap only as a single clip (clips without a frame take no
    # row and do not count: [100 samples, a clip above the cap] is one group, as the engine has always formed it)
    assert got["groups"][0][0] == 0 and sum(g[1] for g in got["groups"]) == n
    for a, b in zip(got["groups"], got["groups"][1:]):
        assert b[0] == a[0] + a[1] and a[1] > 0
    for g in got["groups"]:
        assert keep or g[3] <= (rows or PLANE_ROWS) or sum(f > 0 for f in F[g[0]:g[0] + g[1]]) == 1
        assert g[5] == strip_len(F[g[0]:g[0] + g[1]], max(1, int(slots * mult)))
        sb = 0
        for c in range(g[0], g[0] + g[1]):  # strip_base: a prefix sum within the group at its strip length
            assert got["desc"][c][3] == sb
            sb += ceil_div(F[c], g[5])
    for c in range(n):  # frame, chunk, record and K1-strip bases: prefix sums over the call
        d = got["desc"][c]
        assert [d[2], d[4], d[5], d[7]] == [sum(F[:c]), sum(ceil_div(f, 1024) for f in F[:c]),
                                            sum(hash_capacity(f) for f in F[:c]), sum(ceil_div(f, 16) for f in F[:c])]
        assert (got["frames"][c], got["hash_base"][c]) == (d[1], d[5])
    assert got["groups"] == want["groups"]
    assert got["desc"] == want["desc"]
    assert got["totals"] == want["totals"]
    assert got["flags"] == want["flags"]


def layout(lens, first=0):
    offs = [first]
    for n in lens:
        offs.append(offs[-1] + n)
    return offs


GROUP_LENS = [44100 * 4 + 313 * t for t in range(9)] + [44100 * 40, 100, 44100 * 3]  # test_clip_groups_bit_exact's


def plan_cases():
    cases = []
    for hop in (128, 512):
        two_chunk = 2048 + hop * 1024  # 1025 frames: two K3 chunks
        cases += [dict(offsets=[0], hop=hop), dict(offsets=[0], hop=hop, loc=HOST),
                  dict(offsets=[7, 7 + 2047], hop=hop),
                  dict(offsets=layout([1000, two_chunk]), hop=hop), dict(offsets=layout([two_chunk, 1000]), hop=hop)]
        for rows in (0, 1, 700, 2000):
            for loc in (HOST, DEVICE):
                cases.append(dict(offsets=layout(GROUP_LENS, 3), hop=hop, rows=rows, loc=loc))
        cases.append(dict(offsets=layout(GROUP_LENS), hop=hop, rows=1, keep=1))
        # overlapping clips given by ends (the exact lane's sub-windows), several groups
        starts = [0, 4000, 8000, 12001, 50000]
        cases.append(dict(offsets=starts + [50000], ends=[s + 2048 + 40 * hop + 13 * i for i, s in enumerate(starts)],
                          hop=hop, rows=90))
        for mult, width, slots in ((1.25, 4, SLOTS), (1.5, 4, SLOTS), (3.0, 4, 7), (1.0, 2, 2 * SLOTS), (0.01, 4, 3)):
            cases.append(dict(offsets=layout(GROUP_LENS, 1), hop=hop, mult=mult, width=width, slots=slots, rows=2000))
    rng = random.Random(11)
    for _ in range(60):
        hop = rng.choice((128, 512))
        lens = [rng.choice((0, 100, 2047, 2048, 2048 + hop, rng.randrange(2048, 2048 + hop * 1100),
                            rng.randrange(0, 6000))) for _ in range(rng.randrange(1, 14))]
        cases.append(dict(offsets=layout(lens, rng.randrange(0, 9)), hop=hop, loc=rng.choice((HOST, DEVICE)),
                          rows=rng.choice((0, 1, 50, 700, 1500)), keep=rng.choice((0, 0, 1)),
                          slots=rng.choice((1, 5, 64, SLOTS)), mult=rng.choice((1.0, 1.25, 1.5, 3.0)),
                          width=rng.choice((2, 4))))
    return cases


def test_plans(run):
    cases = plan_cases()
    full = [dict(dict(ends=None, loc=DEVICE, hop=512, rows=0, keep=0, slots=SLOTS, mult=1.0, width=4), **c) for c in cases]
    out = run([plan_line(**c) for c in full])
    for c, tok in zip(full, out):
        check_plan(parse_plan(tok, len(c["offsets"]) - 1), **c)


def test_plan_named_shapes(run):
    """The shapes the flags and groups exist for, spelled out."""
    two = 2048 + 512 * 1024
    out = run([plan_line([0]), plan_line([5, 5 + 2047]), plan_line(layout([1000, two])), plan_line(layout([two, 1000])),
               plan_line(layout(GROUP_LENS), rows=1, keep=1), plan_line(layout(GROUP_LENS), rows=1),
               plan_line(layout(GROUP_LENS, 2), loc=HOST), plan_line(layout(GROUP_LENS, 2), loc=DEVICE)])
    none, short, ab, ba, keep, per_clip, host, dev = (parse_plan(t, n) for t, n in zip(out, (0, 1, 2, 2, 12, 12, 12, 12)))
    assert none["totals"] == [0, 0, 0, 0, 0] and none["flags"] == [0, 0, 0] and len(none["groups"]) == 1
    assert short["totals"][0] == 0 and short["flags"] == [1, 0, 0]
    for p in (ab, ba):  # two chunks, two clips: yet not one chunk each
        assert p["totals"][2] == 2 and p["flags"] == [1, 1, 0]
    assert len(keep["groups"]) == 1
    assert len(per_clip["groups"]) == 11 and per_clip["groups"][-1][:2] == [10, 2]  # the frameless clip opens the last
    # host PCM is staged from offsets[0] on; device PCM is read in place and nothing is staged
    assert host["totals"][4] == sum(GROUP_LENS) and dev["totals"][4] == 0
    assert [d[0] for d in host["desc"]] == layout(GROUP_LENS)[:-1] and [d[0] for d in dev["desc"]] == layout(GROUP_LENS, 2)[:-1]
    assert [d[1:] for d in host["desc"]] == [d[1:] for d in dev["desc"]]


# ---- K2Policy. A word pair of a counted K2 launch: cw = cold waves | waves << 32, sw = twice-walked | strips << 32
def words(width, strips, cold=0, twice=0):
    return (cold | (width * strips) << 32, twice | strips << 32)


def policy_model(steps):
    """The header's comment: start at 4; 4 -> 2 on a width-4 count with half the waves or more cold and no hold
    pending; 2 -> 4 on a width-2 count with a strip walked twice, then 64 held calls; counts of another width and an
    empty history change nothing; a forced width is taken and stays; 1 / 1.25 / 1.5 strips per slot at cold fractions
    below 0.3 / from 0.3 / from 0.45 of a width-4 count at width 4; a forced multiplier wins."""
    width, hold, out = 4, 0, []
    for fw, fx, cw, sw in steps:
        waves, cold, strips, twice = cw >> 32, cw & 0xFFFFFFFF, sw >> 32, sw & 0xFFFFFFFF
        seen = waves // strips if strips else 0
        if fw:
            width = fw
        elif width == 4:
            if hold:
                hold -= 1
            elif seen == 4 and 2 * cold >= waves:
                width = 2
        elif seen == 2 and twice > 0:
            width, hold = 4, 64
        mult = 1.0
        if fx:
            mult = fx / 100
        elif width == 4 and seen == 4:
            frac = min(1.0, cold / waves)
            mult = 1.5 if frac >= 0.45 else 1.25 if frac >= 0.3 else 1.0
        out.append((width, mult))
    return out


def run_policy(run, traces):
    outs = run([" ".join(map(str, ["policy", len(t)] + [x for s in t for x in s])) for t in traces])
    res = []
    for t, tok in zip(traces, outs):
        assert tok[:2] == ["4", "0"]  # a fresh policy starts at width 4 with no hold
        got = [(int(tok[2 + 3 * i]), float(tok[3 + 3 * i])) for i in range(len(t))]
        assert [int(tok[4 + 3 * i]) for i in range(len(t))] == [w for w, _ in got]  # `width` is the call's width
        assert got == policy_model(t)
        res.append(got)
    return res


def test_policy(run):
    S = 1000  # strips of the counted launches
    cold4 = lambda frac: (0, 0, *words(4, S, cold=round(frac * 4 * S)))
    none = (0, 0, 0, 0)
    traces = {
        "start": [none, none],
        "half_cold": [cold4(0.5), none, none],
        "under_half": [(0, 0, *words(4, S, cold=2 * S - 1)), none],
        # at width 2: a clean width-2 count stays; one strip walked twice -> 4, 64 held calls, the 65th may move
        "fallback": [cold4(0.5), (0, 0, *words(2, S)), (0, 0, *words(2, S, twice=1))] + [cold4(0.9)] * 66,
        # counts of a launch at another width than the one in use, and an empty history
        "other_width": [(0, 0, *words(2, S, twice=5)), cold4(0.6), (0, 0, *words(4, S, cold=4 * S)), none,
                        (0, 0, 7, 3)],
        "forced": [(2, 0, 0, 0), none, (4, 0, *words(2, S)), none, cold4(0.6), (4, 0, *words(4, S, cold=4 * S)), none],
        "mult": [cold4(0.29), cold4(0.30), cold4(0.44), cold4(0.45), (0, 0, *words(2, S, twice=1))],
        "forced_mult": [(0, 300, 0, 0), (0, 300, *cold4(0.45)[2:]), (2, 300, 0, 0), (0, 0, 0, 0)],
    }
    got = dict(zip(traces, run_policy(run, list(traces.values()))))
    # the same facts spelled out, so that a slip in the model above cannot hide one in the header
    assert got["start"] == [(4, 1.0), (4, 1.0)]
    assert [w for w, _ in got["half_cold"]] == [2, 2, 2]
    assert [w for w, _ in got["under_half"]] == [4, 4]
    fb = [w for w, _ in got["fallback"]]
    assert fb[:3] == [2, 2, 4] and fb[3:3 + 64] == [4] * 64 and fb[3 + 64] == 2
    assert [w for w, _ in got["other_width"]] == [4, 2, 2, 2, 2]
    assert [w for w, _ in got["forced"]] == [2, 2, 4, 4, 2, 4, 4]
    assert [m for _, m in got["mult"]] == [1.0, 1.25, 1.25, 1.5, 1.0]
    assert [m for _, m in got["forced_mult"]] == [3.0, 3.0, 3.0, 1.0]


# ---- the descriptor cache's criterion
def test_desc_differ(run):
    a = [[2, 858, 0, 0, 0, 0, 69120, 0], [440002, 0, 858, 54, 1, 69120, 0, 54], [440102, 1030, 858, 54, 1, 69120, 82560, 54]]
    flat = lambda d: " ".join(str(x) for row in d for x in row)
    cases, want = [("differ 3 3 " + flat(a) + " " + flat(a))], [0]
    for c in range(3):
        for f in range(8):  # any single field
            b = [row[:] for row in a]
            b[c][f] += 1
            cases.append(f"differ 3 3 {flat(a)} {flat(b)}")
            want.append(1)
    cases += [f"differ 3 2 {flat(a)} {flat(a[:2])}", f"differ 2 3 {flat(a[:2])} {flat(a)}", "differ 0 0",
              f"differ 0 1 {flat(a[:1])}"]
    want += [1, 1, 0, 1]
    assert [int(t[0]) for t in run(cases)] == want
