"""The solver launcher's plan (impact_amd/csrc/solve_plan.hpp) compiled host-only — no HIP runtime, no GPU — and checked by
tools/solve_plan_check.cpp: `table` holds inputs with the expected solve form, workgroups, LDS bytes and exact step sequence written out by hand
(every branch of the selection, every shape of sequence: one phase or both, replay on and off, the fork and its absence, forced group counts
against the occupancy fit, 47 / 48 levels, widest 256 / 257, one chain too many, the body counts around the LDS limit, no dynamic bodies,
tracing); `random N` draws inputs, compares the choice with a transcription of the functions the plan replaced and asserts the invariants of the
sequence (a fork has its join-record and join-wait and the side stream is used only between them, no pass 2 without a replay, k_kin_prefix
between the passes, at most 16 steps). The same program once more under the address and undefined-behaviour sanitizers, stand-alone (their
runtimes linked statically: the program then asks nothing of the order libraries are loaded in)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "solve_plan_check.cpp")


SANITIZED = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


@pytest.mark.parametrize("sanitize", [[], SANITIZED], ids=["plain", "sanitized"])
def test_solve_plan(tmp_path, sanitize):
    exe = str(tmp_path / "solve_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + sanitize + [SRC, "-o", exe], check=True)
    r = subprocess.run([exe, "table"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "solve plan table: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([exe, "random", "100000"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "solve plan random: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
