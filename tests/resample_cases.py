"""The K6 `resample` case table shared by tests/test_resample_plan_host.py (CPU: every row takes the kernel form it
names) and tests/test_gpu_resample_paths.py (GPU: every row equals the oracle bit for bit), and the rules of
audio-ident_amd/csrc/aidfp_resample_plan.h restated in Python. Imports no GPU code.

Rates are plain positive integers to the ABI, so small made-up rates reach exact (up, down) pairs."""

import math
from typing import NamedTuple

REJECT, DECIMATE3, PHASE, UNIFORM, GLOBAL_TAPS = range(5)  # ResPath
OK, BAD_WINDOW, BAD_TAPS = range(3)  # ResStatus
PATH_NAMES = {REJECT: "reject", DECIMATE3: "decimate3", PHASE: "phase", UNIFORM: "mode2", GLOBAL_TAPS: "mode0"}

RES_BLOCK = 1024  # outputs of a k_resample workgroup: 256 threads x 4
RES_R = 16  # outputs per thread of k_resample_phase
DEC_BLOCK = 1024  # outputs of a k_decimate workgroup: 256 threads x 4
MAX_PHASE_UP = 1024
MAX_PHASE_WINDOW = 12288  # floats
MAX_LDS = 65536  # bytes
MAX_TAPS = 1 << 24  # floats


def ratio(sr_in, sr_out):
    """FPSPEC 8: gcd reduction, hl = 10 max(up, down), J = ceil((2 hl + 1) / up)."""
    g = math.gcd(sr_in, sr_out)
    up, down = sr_out // g, sr_in // g
    hl = 10 * max(up, down)
    return up, down, hl, -(-(2 * hl + 1) // up)


def phase_window(up, down, J):  # floats of input of up * 16 consecutive outputs, + 2
    return (up * RES_R - 1) * down // up + J + 2


def use_phase(up, down, J):
    return 1 < up <= MAX_PHASE_UP and phase_window(up, down, J) <= MAX_PHASE_WINDOW


def window_floats(up, down, J):
    return phase_window(up, down, J) if use_phase(up, down, J) else (RES_BLOCK - 1) * down // up + J + 2


class Launch(NamedTuple):
    path: int
    status: int
    block: int  # outputs of one workgroup
    threads: int
    lds_floats: int


def launch_plan(up, down, J):
    """What resample_launch_plan must give, from the rules of the issue's table."""
    w = window_floats(up, down, J)
    if w * 4 > MAX_LDS:
        return Launch(REJECT, BAD_WINDOW, 0, 0, 0)
    if up * J > MAX_TAPS:
        return Launch(REJECT, BAD_TAPS, 0, 0, 0)
    if use_phase(up, down, J):
        return Launch(PHASE, OK, up * RES_R, min(256, (up + 63) // 64 * 64), w)
    if (up, down, J) == (1, 3, 61):
        return Launch(DECIMATE3, OK, DEC_BLOCK, 256, (DEC_BLOCK - 1) * 3 + 61 + 4)
    return Launch(UNIFORM if up == 1 else GLOBAL_TAPS, OK, RES_BLOCK, 256, w)


class Case(NamedTuple):
    sr_in: int
    sr_out: int
    up: int
    down: int
    J: int
    path: int
    why: str

    @property
    def id(self):
        return f"{self.sr_in}to{self.sr_out}"


CASES = [
    Case(2, 1, 1, 2, 41, UNIFORM, "smallest generic decimation"),
    Case(32000, 16000, 1, 2, 41, UNIFORM, "the same pair from real rates"),
    Case(96000, 16000, 1, 6, 121, UNIFORM, "a real ingest rate"),
    Case(15, 1, 1, 15, 301, UNIFORM, "largest accepted window (62.6 KB of LDS)"),
    Case(48000, 16000, 1, 3, 61, DECIMATE3, "block-exact counts and dst alignment"),
    Case(1, 2, 2, 1, 21, PHASE, "64-thread block, 2 active lanes"),
    Case(64, 65, 65, 64, 21, PHASE, "block of 128 with one lane in wave 1"),
    Case(65, 64, 64, 65, 21, PHASE, "exactly one full wave"),
    Case(256, 257, 257, 256, 21, PHASE, "second trip of the t loop with one thread"),
    Case(695, 1024, 1024, 695, 21, PHASE, "largest up, 4 trips"),
    Case(765, 1024, 1024, 765, 21, PHASE, "near-largest window at the largest up"),
    Case(471, 2, 2, 471, 4711, PHASE, "a long filter with J % 8 == 7"),
    Case(481, 2, 2, 481, 4811, PHASE, "largest phase window with a long filter (12,268 floats), J % 8 == 3"),
    Case(767, 1024, 1024, 767, 21, GLOBAL_TAPS, "just past use_phase by window"),
    Case(1, 1025, 1025, 1, 21, GLOBAL_TAPS, "just past use_phase by up; 5 input samples already give 6 blocks"),
    Case(1031, 1025, 1025, 1031, 21, GLOBAL_TAPS, "down > up"),
    Case(44101, 48000, 48000, 44101, 21, GLOBAL_TAPS, "s16 and stereo on a large table"),
]
BY_ID = {c.id: c for c in CASES}

# what aid_resample refuses (sr_in, sr_out, status), each beside its accepted neighbour(s)
REFUSED = [(16, 1, BAD_WINDOW), (483, 2, BAD_WINDOW), (1, 1000000, BAD_TAPS)]
ACCEPTED_NEIGHBOURS = [(15, 1), (471, 2), (473, 2), (481, 2)]
