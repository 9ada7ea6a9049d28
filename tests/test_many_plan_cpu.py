"""The launch recorder's flush plan (impact_amd/csrc/many_plan.hpp) compiled host-only — no HIP runtime, no GPU — and checked by
tools/many_plan_check.cpp: `table` holds recorded batches with the expected launches, their members and running block counts, the totals and
every offset of the staging block written out by hand (an empty batch, one object, identical chains, an object that skips a stage in the middle
or at the front, the same kernel twice in a row, range operations in a row and across objects, uploads of 4 / 12 / 16 / 20 bytes ahead of
everything else, entries without blocks, a first object that recorded nothing or finishes first); `random N` draws batches over the real kernel
ids (up to 64 objects, chains of 0-12 entries, 0-300 blocks, payloads of 0-4096 bytes), compares the plan with a transcription of the loops it
replaced and asserts the invariants (every entry a member exactly once, of a launch of its kernel; an object's entries in launches that do not
go back, and go forward unless the kernel is a range operation; 16-byte boundaries, pieces apart and inside the block; totals and running
counts as the twin's search expects them). The same program once more under the address and undefined-behaviour sanitizers, stand-alone (their
runtimes linked statically: the program then asks nothing of the order libraries are loaded in)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "many_plan_check.cpp")


SANITIZED = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


@pytest.mark.parametrize("sanitize", [[], SANITIZED], ids=["plain", "sanitized"])
def test_many_plan(tmp_path, sanitize):
    exe = str(tmp_path / "many_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + sanitize + [SRC, "-o", exe], check=True)
    r = subprocess.run([exe, "table"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "many plan table: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([exe, "random", "100000"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "many plan random: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
