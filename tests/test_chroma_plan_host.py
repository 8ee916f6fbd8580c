"""Host-side checks of audio-ident_amd/csrc/aidfp_chroma_plan.h (compiled with g++, no GPU): the planning half of the
content fingerprint (spec/FPSPEC.md 11). One stand-alone program with its own main reads cases and prints what the
header computes: frame and word counts, the offsets of a batch, K11a's and K11b's workgroup lists, the note table and
its runs, the classifiers with their thresholds and rectangles. Expected values are restated here from the spec or
read from the committed note table (tests/golden/chroma_notes.bin); none is taken from the program's output. The same
cases run a second time through a build with -fsanitize=address,undefined (the sanitizer's runtime linked statically
into the program)."""

import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import chroma_ref as R

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
SRC = r"""
#include <cstdio>
#include <iostream>
#include <string>
#include "aidfp_chroma_plan.h"
using namespace aid;
int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "len") {
            long long n;
            std::cin >> n;
            std::printf("len %lld %lld\n", (long long)chroma_frames(n), (long long)chroma_words(n));
        } else if (cmd == "batch") {
            int nc;
            std::cin >> nc;
            std::vector<int64_t> len(nc), off(nc + 1, 0), fo(nc + 1, -1), wo(nc + 1, -1);
            for (auto &x : len) std::cin >> x;
            const int st = chroma_offsets(len.data(), nc, fo.data(), wo.data());
            std::printf("batch %d", st);
            if (st == kChromaOk) {
                for (int c = 0; c <= nc; ++c) std::printf(" %lld %lld", (long long)fo[c], (long long)wo[c]);
                for (int c = 0; c < nc; ++c) off[c + 1] = off[c] + len[c];
                std::vector<ChromaRowBlock> rb;
                std::vector<ChromaItemBlock> ib;
                chroma_row_blocks(off.data(), fo.data(), nc, 0, rb);
                chroma_item_blocks(fo.data(), wo.data(), nc, ib);
                std::printf(" | %zu", rb.size());
                for (const auto &b : rb) std::printf(" %lld %lld %d", (long long)b.src, (long long)b.row, b.nfr);
                std::printf(" | %zu", ib.size());
                for (const auto &b : ib) std::printf(" %lld %lld %d", (long long)b.row, (long long)b.word, b.n);
            }
            std::printf("\n");
        } else if (cmd == "notes") {
            std::printf("notes");
            for (int k = kChromaBinLo; k < kChromaBinHi; ++k) std::printf(" %d", chroma_note(k));
            std::printf("\n");
        } else if (cmd == "runs") {
            const auto r = chroma_runs();
            std::printf("runs %zu", r.size());
            for (const auto &x : r) std::printf(" %d %d %d", x.lo, x.len, x.note);
            std::printf("\n");
        } else if (cmd == "cls") {
            std::printf("cls");
            for (int j = 0; j < kChromaClassifiers; ++j) {
                const ChromaClassifier c = chroma_classifier(j);
                std::printf(" %d %d %d %d %a %a %a %a %a %a %d %d", c.type, c.y, c.h, c.w, (double)c.t[0], (double)c.t[1],
                            (double)c.t[2], (double)c.E[0], (double)c.E[1], (double)c.E[2], c.na, c.nb);
                for (int i = 0; i < c.na; ++i) std::printf(" %d %d %d %d", c.a[i].x0, c.a[i].x1, c.a[i].y0, c.a[i].y1);
                for (int i = 0; i < c.nb; ++i) std::printf(" %d %d %d %d", c.b[i].x0, c.b[i].x1, c.b[i].y0, c.b[i].y1);
            }
            std::printf("\n");
        } else {
            return 3;
        }
    }
    std::printf("consts %d %d %d %d %d %d %d %d %d %d %u\n", kChromaRate, kChromaN, kChromaHop, kChromaBinLo, kChromaBinHi,
                kChromaBands, kChromaItemRows, kChromaRun, kChromaStage, kChromaItems, kChromaZeroWord);
    return 0;
}
"""

OK, BAD_LENGTH, OVERFLOW = range(3)  # ChromaStatus
RUN, ITEMS = 4, 240


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def run(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("chroma_plan_" + request.param)
    (d / "chroma_check.cpp").write_text(SRC)
    exe = d / "chroma_check"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"]
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                    *(san if request.param == "sanitized" else []),
                    "-I", str(ROOT / "audio-ident_amd" / "csrc"), str(d / "chroma_check.cpp"), "-o", str(exe)], check=True)

    def run_(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        rows = out.stdout.strip().split("\n")
        assert rows[-1] == f"consts 11025 4096 1365 10 1308 12 20 {RUN} {(RUN - 1) * 1365 + 4096} {ITEMS} 627964279"
        assert len(rows) == len(lines) + 1
        return [r.split()[1:] for r in rows[:-1]]

    return run_


def test_frame_and_word_counts(run):
    ns = [0, 4095, 4096, 30030, 30031, 31395, 31396, 30 * 60 * 11025, -1]
    want = [(0, 0), (0, 0), (1, 0), (19, 0), (20, 1), (20, 1), (21, 2), (14536, 14517), (0, 0)]
    # the 30-minute track: 19,845,000 samples, 1 + (19845000 - 4096) // 1365 frames
    assert 1 + (19845000 - 4096) // 1365 == 14536
    rows = run([f"len {n}" for n in ns])
    assert [(int(r[0]), int(r[1])) for r in rows] == want
    assert [(R.n_frames(n), R.n_words(n)) for n in ns[:-1]] == want[:-1]  # the oracle counts the same


def _batch(row):
    st = int(row[0])
    if st != OK:
        return st, None, None, None
    a = row[1:].index("|")
    offs = [int(v) for v in row[1:1 + a]]
    rest = row[2 + a:]
    b = rest.index("|")
    nrb = int(rest[0])
    rb = [tuple(int(v) for v in rest[1 + 3 * i:4 + 3 * i]) for i in range(nrb)]
    tail = rest[b + 1:]
    ib = [tuple(int(v) for v in tail[1 + 3 * i:4 + 3 * i]) for i in range(int(tail[0]))]
    assert len(rest[1:b]) == 3 * nrb and len(tail[1:]) == 3 * len(ib)
    return st, list(zip(offs[0::2], offs[1::2])), rb, ib


def test_offsets_and_blocks_of_a_mixed_batch(run):
    lens = [4096, 0, 30031, 15017, 4095, 4096 + 1365 * 300]
    st, offs, rb, ib = _batch(run(["batch " + " ".join(map(str, [len(lens)] + lens))])[0])
    frames = [1, 0, 20, 9, 0, 301]
    words = [0, 0, 1, 0, 0, 282]
    assert st == OK
    assert offs == list(zip(np.concatenate([[0], np.cumsum(frames)]).tolist(),
                            np.concatenate([[0], np.cumsum(words)]).tolist()))
    # K11a: runs of RUN frames per clip, the last one short; a block's samples end inside its clip
    starts = np.concatenate([[0], np.cumsum(lens)])
    want_rb = []
    for c, T in enumerate(frames):
        for t in range(0, T, RUN):
            want_rb.append((int(starts[c]) + 1365 * t, sum(frames[:c]) + t, min(RUN, T - t)))
    assert rb == want_rb
    for src, row, nfr in rb:
        c = int(np.searchsorted(starts, src, side="right")) - 1
        assert src + (nfr - 1) * 1365 + 4096 <= starts[c + 1]
    # K11b: blocks of at most ITEMS words, each inside one clip's rows
    assert ib == [(1, 0, 1), (30, 1, ITEMS), (30 + ITEMS, 1 + ITEMS, 282 - ITEMS)]
    for row, word, n in ib:
        c = max(i for i in range(len(lens)) if offs[i][0] <= row and frames[i] > 0)
        assert row + n - 1 + 20 <= offs[c + 1][0]


def test_bad_lengths_and_overflow(run):
    big = 2**63 - 1  # 6.7e15 frames each; 48 bytes a frame fit an int64 up to 1.9e17 frames
    rows = run(["batch 2 4096 -1", "batch 40 " + " ".join([str(big)] * 40), "batch 0"])
    assert int(rows[0][0]) == BAD_LENGTH and int(rows[1][0]) == OVERFLOW
    st, offs, rb, ib = _batch(rows[2])
    assert st == OK and offs == [(0, 0)] and rb == [] and ib == []


def test_note_table_equals_fixture(run):
    gold = np.frombuffer((GOLD / "chroma_notes.bin").read_bytes(), dtype=np.uint8)
    assert len(gold) == 1298 and gold.min() == 0 and gold.max() == 11
    notes, runs = run(["notes", "runs"])
    assert np.array_equal(np.array(notes, dtype=np.int64), gold)
    assert np.array_equal(R.note_table(), gold)  # the oracle's table too
    # bin 10 is 26.9 Hz, just below A0 = 27.5 Hz: note 11; bin 41 is the first at or above 110 Hz (A2): note 0
    assert gold[0] == 11 and gold[41 - 10] == 0 and gold[40 - 10] == 11
    n = int(runs[0])
    got = [tuple(int(v) for v in runs[1 + 3 * i:4 + 3 * i]) for i in range(n)]
    assert n == 83 and max(g[1] for g in got) == 73
    want = []
    for i, v in enumerate(gold):
        if want and want[-1][2] == int(v):
            want[-1][1] += 1
        else:
            want.append([10 + i, 1, int(v)])
    assert got == [tuple(w) for w in want] == R.runs()
    assert sum(g[1] for g in got) == 1298 and got[0][0] == 10 and got[-1][0] + got[-1][1] == 1308


def test_classifiers_thresholds_and_rectangles(run):
    f = run(["cls"])[0]
    pos = 0
    for j, (typ, y, h, w, *t) in enumerate(R.CLASSIFIERS):
        head = f[pos:pos + 12]
        assert [int(v) for v in head[:4]] == [typ, y, h, w], j
        ts = [float.fromhex(v) for v in head[4:7]]
        Es = [float.fromhex(v) for v in head[7:10]]
        assert ts == [float(np.float32(v)) for v in t], j
        assert ts[0] < ts[1] < ts[2] and Es[0] < Es[1] < Es[2], j
        assert Es == [float(np.float32(np.exp(np.float64(np.float32(v))))) for v in t], j
        na, nb = int(head[10]), int(head[11])
        rs = [tuple(int(v) for v in f[pos + 12 + 4 * i:pos + 16 + 4 * i]) for i in range(na + nb)]
        pos += 12 + 4 * (na + nb)
        ra, rb = R.rects(j)
        assert rs[:na] == ra and rs[na:] == rb, j
        assert (na, nb) == {0: (1, 0), 1: (1, 1), 2: (1, 1), 3: (2, 2), 4: (1, 2), 5: (1, 2)}[typ]
        cells = set()
        for x0, x1, y0, y1 in rs:  # inside the 16 x 12 image, non-empty, disjoint, together the whole classifier
            assert 0 <= x0 < x1 <= 16 and 0 <= y0 < y1 <= 12, (j, rs)
            new = {(x, yy) for x in range(x0, x1) for yy in range(y0, y1)}
            assert not (cells & new)
            cells |= new
        assert cells == {(x, yy) for x in range(w) for yy in range(y, y + h)}, j
    assert pos == len(f)
    # the known answer: zero features give A = B = 1, q_j = #{t_i <= 0}
    v = 0
    for c in R.CLASSIFIERS:
        v = (v << 2) | [0, 1, 3, 2][sum(t <= 0 for t in c[4:])]
    assert v == 627964279 == 0x256DF977
