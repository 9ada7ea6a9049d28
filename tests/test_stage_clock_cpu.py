"""The stage clock of a step (impact_amd/csrc/stage_clock.hpp) compiled host-only — no HIP runtime, no GPU — and checked against scenarios
written out by hand in tools/stage_clock_check.cpp: every slot timed on the fused path (seven words, each shared between neighbours), a mask
with gaps (no sharing across an untimed slot), a slot without a launch (0, and a word it armed itself is given back), two enqueues before one
collect, the word budget exhausted (the call falls to events as a whole), and the calls that may not stamp. The same program, run as
`random N`, drives the clock against a transcription of the macros it replaced (profiles/step_unit/stage_clock_check.txt)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_clock_scenarios(tmp_path):
    exe = str(tmp_path / "stage_clock_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tools", "stage_clock_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, "scenarios"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "stage clock scenarios: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
