"""Host-side checks of audio-ident_amd/csrc/aidfp_vector_filter.h (compiled with g++, no GPU): validation of a call's
filters, the grouping of a batch's queries by identical filter, the unfiltered verdict and the bitmap geometry of
spec/FPSPEC.md 9.2. One stand-alone program with its own main reads cases and prints what the header computes; the
expected values are restated here or come from tests/vec_filter_ref.py, none from the program's output. The same cases
run a second time through a build with -fsanitize=address,undefined (the sanitizer's runtime linked statically into
the program): `bits` sets one bit per entry through the geometry into a buffer of exactly the words it promises, so
a word index out of range is a heap overflow there, and `plan` reads its filters from a heap array of exactly nb."""

import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import vec_filter_ref as R
from vec_filter_ref import Filt

ROOT = Path(__file__).resolve().parent.parent
SRC = r"""
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>
#include "aidfp_vector_filter.h"
using namespace aid;
static aid_vec_filter read_filter() {
    aid_vec_filter f;
    unsigned n;
    std::cin >> f.any_of >> f.all_of >> f.none_of >> n;
    f.n_exclude = n;
    for (unsigned i = 0; i < n; ++i) {
        unsigned t;
        std::cin >> t;
        if (i < AID_VEC_MAX_EXCLUDE) f.exclude[i] = t;
    }
    for (unsigned i = n; i < AID_VEC_MAX_EXCLUDE; ++i) f.exclude[i] = 0xDEADBEEFu;  // not read
    return f;
}
int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "words") {
            long long n;
            std::cin >> n;
            std::printf("words %lld\n", (long long)vec_allow_words(n));
        } else if (cmd == "bits") {  // every entry sets its own bit of a buffer of exactly vec_allow_words(n) words
            long long n;
            std::cin >> n;
            std::vector<uint64_t> bm((size_t)vec_allow_words(n), 0);
            long long twice = 0;
            for (long long e = 0; e < n; ++e) {
                uint64_t &w = bm[(size_t)vec_allow_word(e)];
                twice += (w >> vec_allow_bit(e)) & 1;
                w |= (uint64_t)1 << vec_allow_bit(e);
            }
            long long set = 0, last = -1;
            for (size_t i = 0; i < bm.size(); ++i) {
                set += __builtin_popcountll(bm[i]);
                if (bm[i]) last = (long long)i;
            }
            // the same bytes read as the selection kernels do: bit e & 31 of 32-bit word e >> 5
            const uint32_t *b32 = reinterpret_cast<const uint32_t *>(bm.data());
            long long ok32 = 0;
            for (long long e = 0; e < n; ++e) ok32 += (b32[e >> 5] >> (e & 31)) & 1;
            std::printf("bits %lld %lld %lld %lld %d\n", twice, set, last, ok32, (int)((bm.size() * 8) % 64));
        } else if (cmd == "valid") {
            int nq;
            std::cin >> nq;
            std::vector<aid_vec_filter> f;
            for (int q = 0; q < nq; ++q) f.push_back(read_filter());
            std::printf("valid %d\n", vec_filters_invalid(f.data(), nq));
        } else if (cmd == "plan") {
            int nb;
            std::cin >> nb;
            std::vector<aid_vec_filter> f;
            for (int q = 0; q < nb; ++q) f.push_back(read_filter());
            f.shrink_to_fit();
            VecFilterPlan p;
            vec_filter_plan(f.data(), nb, p);
            std::printf("plan %d %d", p.n_distinct, (int)p.filtered);
            for (int q = 0; q < nb; ++q) std::printf(" %d", p.fmap[q]);
            for (int d = 0; d < p.n_distinct; ++d) {
                const aid_vec_filter &g = p.distinct[d];
                std::printf(" | %llu %llu %llu %u", (unsigned long long)g.any_of, (unsigned long long)g.all_of,
                            (unsigned long long)g.none_of, g.n_exclude);
                for (int i = 0; i < AID_VEC_MAX_EXCLUDE; ++i) std::printf(" %u", g.exclude[i]);
            }
            std::printf("\n");
        } else if (cmd == "pass") {
            aid_vec_filter f = read_filter();
            int live;
            unsigned long long tags;
            unsigned track;
            std::cin >> live >> tags >> track;
            std::printf("pass %d %d\n", (int)vec_filter_passes(f, live != 0, tags, track),
                        (int)vec_filter_passes(vec_filter_normal(f), live != 0, tags, track));
        } else {
            return 3;
        }
    }
    std::printf("consts %d %d %zu\n", kVecFilterBatch, AID_VEC_MAX_EXCLUDE, sizeof(aid_vec_filter));
    return 0;
}
"""


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def run(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("vec_filter_plan_" + request.param)
    (d / "filter_check.cpp").write_text(SRC)
    exe = d / "filter_check"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off",
                    *(san if request.param == "sanitized" else []),
                    "-I", str(ROOT / "audio-ident_amd" / "csrc"), str(d / "filter_check.cpp"), "-o", str(exe)], check=True)

    def run_(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        rows = out.stdout.strip().split("\n")
        assert rows[-1] == "consts 64 8 64"
        assert len(rows) == len(lines) + 1
        return [r.split()[1:] for r in rows[:-1]]

    return run_


def fl(f):
    f = R.ZERO if f is None else f
    return " ".join(str(x) for x in (f.any_of, f.all_of, f.none_of, len(f.exclude), *f.exclude))


def plan(run, filters):
    """(n_distinct, filtered, fmap, [distinct as (any, all, none, n_exclude, slots)])"""
    row = " ".join(run([f"plan {len(filters)} " + " ".join(fl(f) for f in filters)])[0])
    head, *groups = row.split(" | ")
    head = [int(x) for x in head.split()]
    distinct = []
    for g in groups:
        v = [int(x) for x in g.split()]
        distinct.append((v[0], v[1], v[2], v[3], tuple(v[4:])))
    assert len(distinct) == head[0]
    return head[0], bool(head[1]), head[2:], distinct


NO_TRACK = 0xFFFFFFFF


def test_bitmap_geometry(run):
    ns = [1, 31, 32, 33, 63, 64, 65, 300, 511, 512, 513, 500_000]
    assert [int(r[0]) for r in run([f"words {n}" for n in ns])] == [R.allow_words(n) for n in ns]
    assert [R.allow_words(n) for n in (1, 31, 32, 33, 63, 64, 65, 300)] == [8] * 8  # at least one 64-byte line
    for n, row in zip(ns, run([f"bits {n}" for n in ns])):
        twice, nset, last, ok32, misalign = (int(x) for x in row)
        assert (twice, nset, last, ok32, misalign) == (0, n, (n - 1) // 64, n, 0), n


def test_equal_filters_share_a_bitmap(run):
    a = Filt(any_of=3, exclude=(7, 2, 9))
    same = [Filt(any_of=3, exclude=(9, 7, 2)), Filt(any_of=3, exclude=(2, 2, 7, 9, 9, 7)), Filt(any_of=3, exclude=(2, 7, 9, NO_TRACK))]
    other = [Filt(any_of=3, exclude=(7, 2)), Filt(any_of=3, all_of=1, exclude=(7, 2, 9)), Filt(all_of=3, exclude=(7, 2, 9)),
             Filt(none_of=3, exclude=(7, 2, 9)), None]
    nd, filtered, fmap, distinct = plan(run, [a, *same, *other, a, None])
    assert filtered and nd == 1 + len(other)
    assert fmap == [0, 0, 0, 0, 1, 2, 3, 4, 5, 0, 5]
    assert distinct[0] == (3, 0, 0, 3, (2, 7, 9) + (NO_TRACK,) * 5)  # sorted, no duplicates, unused slots reserved
    assert distinct[5] == (0, 0, 0, 0, (NO_TRACK,) * 8)              # the zero filter among filtered ones: a bitmap too
    for d, f in zip(distinct, [a, *other]):
        assert (d[0], d[1], d[2], d[4][: d[3]]) == R.normal(f)


def test_sixty_four_distinct_filters_stay_distinct(run):
    filters = [Filt(any_of=q % 15 + 1, none_of=(1 << 63) if q % 2 else 0, exclude=(q % 40, (7 * q + 1) % 40)) for q in range(64)]
    assert len({R.normal(f) for f in filters}) == 64
    nd, filtered, fmap, distinct = plan(run, filters)
    assert (nd, filtered, fmap) == (64, True, list(range(64)))
    assert [(d[0], d[1], d[2], d[4][: d[3]]) for d in distinct] == [R.normal(f) for f in filters]
    # bit 63 and 8 exclusions survive the trip
    nd, _, _, distinct = plan(run, [Filt(any_of=1 << 63, all_of=(1 << 64) - 1, exclude=tuple(range(100, 92, -1)))])
    assert distinct == [(1 << 63, (1 << 64) - 1, 0, 8, tuple(range(93, 101)))]


def test_unfiltered_verdict(run):
    assert plan(run, [None] * 64)[:3] == (1, False, [0] * 64)
    assert plan(run, [None])[:3] == (1, False, [0])
    # exclusions that name only the reserved id exclude nothing
    assert plan(run, [None, Filt(exclude=(NO_TRACK, NO_TRACK))])[:3] == (1, False, [0, 0])
    for f in (Filt(any_of=1), Filt(all_of=1 << 63), Filt(none_of=2), Filt(exclude=(0,))):
        nd, filtered, fmap, _ = plan(run, [None] * 63 + [f])
        assert (nd, filtered, fmap) == (2, True, [0] * 63 + [1])


def test_validation(run):
    ok = fl(Filt(any_of=1, exclude=tuple(range(8))))
    nine = "1 0 0 9 " + " ".join(str(i) for i in range(9))
    assert run(["valid 0", f"valid 1 {ok}", f"valid 3 {ok} {fl(None)} {ok}"]) == [["0"], ["0"], ["0"]]
    # the answer is the first offender, counted from 1
    assert run([f"valid 1 {nine}", f"valid 3 {ok} {ok} {nine}", f"valid 2 {nine} {nine}", f"valid 2 {ok} {nine}"]) \
        == [["1"], ["3"], ["1"], ["2"]]


def test_passes_agrees_with_the_oracle(run):
    rng = np.random.default_rng(4)
    lines, want = [], []
    for _ in range(300):
        f = Filt(any_of=int(rng.integers(0, 16)) if rng.random() < 0.5 else 0,
                 all_of=int(rng.integers(0, 4)) if rng.random() < 0.4 else 0,
                 none_of=int(rng.integers(0, 16)) if rng.random() < 0.3 else 0,
                 exclude=tuple(int(x) for x in rng.integers(0, 6, size=rng.choice([0, 0, 1, 2, 8]))))
        live, tags, track = int(rng.random() < 0.9), int(rng.integers(0, 16)), int(rng.integers(0, 6))
        if rng.random() < 0.2:
            f, tags = f._replace(any_of=1 << 63), tags | (int(rng.integers(0, 2)) << 63)
        lines.append(f"pass {fl(f)} {live} {tags} {track}")
        w = int(R.passes(np.array([tags], np.uint64), np.array([track]), np.array([bool(live)]), f)[0])
        want.append([str(w), str(w)])
    assert run(lines) == want
    assert 60 < sum(int(w[0]) for w in want) < 240
