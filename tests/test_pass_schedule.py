"""The pass schedule of the render host loop (vermilion_amd/csrc/pass_schedule.h), CPU only: the stand-alone program
tests/cpp/pass_schedule_test.cpp runs scripted passes through plan_pass and pass_form and prints (S, lead, form) per pass.
Every expected line is worked out by hand from the rule as the header's comments state it.

The frames have 64 samples per pixel: kmax 64, quarter 16, nmin 8, so the early-stop rule can fire from sample 9 on and 3
strata follow the first.  A pass line of a script is `pass <n_active> <cap, 0: none> <pixels of it that stopped a stratum>`,
a job line `job <smax> <smax_alloc> <n_pad_max> <pipeline> <nee> <ragged>` (see the program's head)."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 1 << 20
_exe = {}


def host_program(sanitize=False):
    if sanitize not in _exe:
        if shutil.which("g++") is None:
            pytest.skip("no g++")
        exe = os.path.join(tempfile.mkdtemp(prefix="pass_schedule_"), "pass_schedule_test")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", os.path.join(ROOT, "vermilion_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "pass_schedule_test.cpp"), "-o", exe], check=True)
        _exe[sanitize] = exe
    return _exe[sanitize]


def run(script, sanitize=False):
    out = subprocess.run([host_program(sanitize)], input=script, capture_output=True, text=True, check=True)
    return out.stdout.split("\n")[:-1]


# (script, expected lines).  768 active pixels = 32 x 24: the passes are far below kHybridPaths, so form 0 runs them fused.
FIXED = [
    # smax 64: one pass of all 64, then the frame is finished
    ("frame 64 0\njob 64 64 768 0 0 0\npass 768 0 0\npass 768 0 0\n", ["64 0 fused", "finished"]),
    # smax 24: 24, 24, the 16 left, finished
    ("frame 64 0\njob 24 24 768 0 0 0\n" + "pass 768 0 0\n" * 4, ["24 0 fused", "24 0 fused", "16 0 fused", "finished"]),
    # a per-call cap of 10: six passes of 10, the 4 left, finished
    ("frame 64 0\njob 64 64 768 0 0 0\n" + "pass 768 10 0\n" * 8, ["10 0 fused"] * 6 + ["4 0 fused", "finished"]),
    # the cap may change between calls: 10, then 30, then uncapped takes the 24 left
    ("frame 64 0\njob 64 64 768 0 0 0\npass 768 10 0\npass 768 30 0\npass 768 0 0\npass 768 0 0\n",
     ["10 0 fused", "30 0 fused", "24 0 fused", "finished"]),
]

UNIFORM = [
    # smax 64: the nmin + 1 = 9 samples before the rule can fire, and the first samples of the 3 later strata ride along
    ("frame 64 1\njob 64 64 768 0 0 0\npass 768 0 0\n", ["12 9 fused"]),
    # exactly room for the group: smax 12
    ("frame 64 1\njob 12 12 768 0 0 0\npass 768 0 0\n", ["12 9 fused"]),
    # smax 11: no room for the 3 that would ride along
    ("frame 64 1\njob 11 11 768 0 0 0\npass 768 0 0\n", ["9 0 fused"]),
    ("frame 64 1\njob 9 9 768 0 0 0\npass 768 0 0\n", ["9 0 fused"]),
    # smax 4: 4, 4, the 1 left of the 9; then the speculative phase — every pixel stopped (768 of 768), so 3 per pixel by the
    # first rule, but 768 pixels are "few" (768 * 2 * 1024 <= 16 M): min(16 M / (2 * 768) = 10922, 1024) = 1024, clipped to
    # the buffers' 768 * 4 / 768 = 4
    ("frame 64 1\njob 4 4 768 0 0 0\n" + "pass 768 0 768\n" * 4, ["4 0 fused", "4 0 fused", "1 0 fused", "4 0 fused"]),
    # a cap below 12 suppresses the lead: 11 leaves room for the 9 alone, 5 splits them 5 + 4
    ("frame 64 1\njob 64 64 768 0 0 0\npass 768 11 0\n", ["9 0 fused"]),
    ("frame 64 1\njob 64 64 768 0 0 0\npass 768 5 0\npass 768 5 0\n", ["5 0 fused", "4 0 fused"]),
    # ... and 12 does not
    ("frame 64 1\njob 64 64 768 0 0 0\npass 768 12 0\n", ["12 9 fused"]),
    # a frame of 4 samples (kmax 4, quarter 1, nmin 2): 3 uniform samples, more than a stratum holds, so nothing rides along
    ("frame 4 1\njob 64 64 768 0 0 0\npass 768 0 0\n", ["3 0 fused"]),
]

# the speculative phase: `state 9 0 <pixels> <breaks>` puts the schedule past the uniform samples with that feedback.
# n_pad_max 1,000,000 (a multiple of 64) and smax_alloc 12: the buffers hold 12 M paths.
SPECULATIVE = [
    # 100,000 active, 12,500 = one in eight of them stopped: 64 / 16 - 1 = 3 per pixel
    ("frame 64 1\njob 12 12 1000000 4 0 0\nstate 9 0 100000 12500\npass 100000 0 0\n", ["3 0 split"]),
    # 12,499: fewer than one in eight: min(16 M / (2 * 100,000) = 83, 1024); the clip is 12 M / 100,032 = 119
    ("frame 64 1\njob 12 12 1000000 4 0 0\nstate 9 0 100000 12499\npass 100000 0 0\n", ["83 0 split"]),
    # no feedback yet (the first speculative pass of a resumed handle): not "fewer than one in eight"
    ("frame 64 1\njob 12 12 1000000 4 0 0\nstate 9 0 0 0\npass 100000 0 0\n", ["3 0 split"]),
    # few pixels left, 8192 * 2 * 1024 = 16 M: min(16 M / 16,384, 1024) = 1024 whatever the share that stopped (here all)
    ("frame 64 1\njob 12 12 1000000 4 0 0\nstate 9 0 8192 8192\npass 8192 0 0\n", ["1024 0 split"]),
    ("frame 64 1\njob 12 12 1000000 4 0 0\nstate 9 0 100 100\npass 100 0 0\n", ["1024 0 split"]),
    # 8193 are not few
    ("frame 64 1\njob 12 12 1000000 4 0 0\nstate 9 0 8193 8193\npass 8193 0 0\n", ["3 0 split"]),
    # 20,000 pixels that keep sampling: 16 M / 40,000 = 419
    ("frame 64 1\njob 12 12 1000000 4 0 0\nstate 9 0 20000 0\npass 20000 0 0\n", ["419 0 split"]),
    # the clip n_pad_max * smax_alloc / n_pad: 8192 * 12 / 8192 = 12; 8192 * 1 / 8192 = 1; 100 pixels pad to 128: 8192 * 12 / 128 = 768
    ("frame 64 1\njob 12 12 8192 4 0 0\nstate 9 0 8192 0\npass 8192 0 0\n", ["12 0 split"]),
    ("frame 64 1\njob 1 1 8192 4 0 0\nstate 9 0 8192 0\npass 8192 0 0\n", ["1 0 split"]),
    ("frame 64 1\njob 12 12 8192 4 0 0\nstate 9 0 100 0\npass 100 0 0\n", ["768 0 split"]),
    # the clip applies to the 3 as well: buffers of 2 per pixel
    ("frame 64 1\njob 2 2 100032 4 0 0\nstate 9 0 100000 100000\npass 100000 0 0\n", ["2 0 split"]),
    # never above the cap, never 0
    ("frame 64 1\njob 12 12 1000000 4 0 0\nstate 9 0 8192 0\npass 8192 5 0\n", ["5 0 split"]),
    ("frame 64 1\njob 12 12 1000000 4 0 0\nstate 9 0 100000 100000\npass 100000 1 0\n", ["1 0 split"]),
    # the feedback a pass files is what the next one reads: 100,000 active and 12,499 stopped, then 87,501 active
    ("frame 64 1\njob 12 12 1000000 4 0 0\nstate 9 0 100000 50000\npass 100000 0 12499\npass 87501 0 0\n",
     ["3 0 split", "95 0 split"]),  # 16 M / 175,002 = 95
]

RAGGED = [
    ("frame 64 0\njob 12 12 768 0 0 1\npass 768 0 0\npass 700 5 0\npass 3 0 0\n", ["12 0 fused", "5 0 fused", "12 0 fused"]),
    # k_fixed means nothing any more: a ragged handle is never "finished" by it
    ("frame 64 0\njob 12 12 768 0 0 1\nstate 0 64 0 0\npass 768 0 0\n", ["12 0 fused"]),
]

FORMS = [
    # pipeline 0: fused below kHybridPaths = 4 M path slots, split from there on
    ("form 0 0 %d 0 0\nform 0 0 %d 0 0\n" % (4 * M - 1, 4 * M), ["fused", "split"]),
    # ... on the first pass of an early-stop frame too, and on every pass of a fixed-count frame
    ("form 0 0 %d 1 0\nform 0 0 %d 1 0\nform 0 0 %d 0 3\nform 0 0 %d 0 3\n" % (4 * M - 1, 4 * M, 4 * M - 1, 4 * M),
     ["fused", "split", "fused", "split"]),
    # a later pass of an early-stop frame: the boundary is kHybridLeftover = 32 M
    ("form 0 0 %d 1 1\nform 0 0 %d 1 1\nform 0 0 %d 1 1\n" % (4 * M, 32 * M - 1, 32 * M), ["fused", "fused", "split"]),
    # pipelines 1 and 4 never depend on the size; 2 and 3 are the first-generation kernels
    ("form 0 1 1 0 0\nform 0 1 %d 0 0\nform 0 1 %d 1 2\nform 0 4 1 0 0\nform 0 4 %d 1 2\nform 0 4 64 1 0\n" % (1 << 40, 1 << 40, 1 << 40),
     ["fused", "fused", "fused", "split", "split", "split"]),
    ("form 0 2 1 0 0\nform 0 3 %d 1 1\n" % (1 << 40), ["firstgen", "firstgen"]),
    # light sampling wins over all of them
    ("".join("form 1 %d %d %d %d\n" % (p, s, e, n) for p in (0, 1, 2, 3, 4) for s, e, n in ((1, 0, 0), (1 << 40, 1, 2))), ["nee"] * 10),
    # through a pass: 65,536 pixels x 64 samples = 4 M slots split, 65,472 x 64 fused; a light-sampled job's pass is k_nee's
    ("frame 64 0\njob 64 64 65536 0 0 0\npass 65536 0 0\nframe 64 0\njob 64 64 65536 0 0 0\npass 65472 0 0\n"
     "frame 64 0\njob 64 64 65536 4 1 0\npass 65536 0 0\n", ["64 0 split", "64 0 fused", "64 0 nee"]),
    # the second pass of an early-stop frame counts as a later pass: 2 M pixels x 3 = 6 M slots, fused below 32 M
    ("frame 64 1\njob 12 12 2097152 0 0 0\npass 2097152 0 2000000\npass 2097152 0 0\n", ["12 9 split", "3 0 fused"]),
]


@pytest.mark.parametrize("script,want", FIXED + UNIFORM + SPECULATIVE + RAGGED + FORMS)
def test_schedule(script, want):
    assert run(script) == want, script


def test_host_program_under_sanitizers():
    """the stand-alone program built with -fsanitize=address,undefined, over every script"""
    for script, want in FIXED + UNIFORM + SPECULATIVE + RAGGED + FORMS:
        assert run(script, sanitize=True) == want, script
