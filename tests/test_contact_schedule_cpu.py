"""The world's host bookkeeping (impact_amd/csrc/contact_schedule.hpp) compiled host-only — no HIP runtime, no GPU — and checked against scenarios
written out by hand in tools/contact_schedule_check.cpp: two bodies and one contact, a manifold of five on one pair (chains 4 + 1), three bodies
in a row, an id leaving from the middle of four, 33 independent chains (two tiles), a kinematic body with two positional passes, zero iterations
of either kind, the empty list after a full one, and lists that are refused. The same program, run as `random N`, drives the struct against a
transcription of the code it replaced (profiles/world_unit/schedule_check.txt)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_contact_schedule_scenarios(tmp_path):
    exe = str(tmp_path / "contact_schedule_check")
    srcs = [os.path.join(ROOT, "tools", "contact_schedule_check.cpp"), os.path.join(ROOT, "impact_amd", "csrc", "contact_schedule.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + srcs + ["-o", exe], check=True)
    r = subprocess.run([exe, "scenarios"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "contact schedule scenarios: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
