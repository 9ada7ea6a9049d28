"""The one host statement of the reference's voxel_ranges_touching_aab (impact_amd/csrc/voxel_ranges.hpp: clamped_ranges, then chunk_box)
compiled host-only — no HIP runtime, no GPU — by tools/voxel_ranges_check.cpp. `scenarios`: boxes inside, outside and straddling the occupied
ranges, bounds exactly on a voxel and on a chunk boundary, negative bounds, -0.0, NaN, +-inf and bounds above 2e9, an empty range on the first,
the middle or the last axis, for the saturating form (edits, mutual forms) and the plain one (collidables; below 2^62 only). `random N`: random
spheres, capsules and occupied ranges through the header and through a transcription of the loop the edit's enqueue spelt out before it called
the header: the same hit, and on a hit the same voxel ranges and chunk box."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("voxel_ranges") / "voxel_ranges_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tools", "voxel_ranges_check.cpp"), "-o", path], check=True)
    return path


def test_voxel_ranges_scenarios(exe):
    r = subprocess.run([exe, "scenarios"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "voxel ranges scenarios: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_voxel_ranges_random(exe):
    r = subprocess.run([exe, "random", "200000"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "voxel ranges random: ok (200000 absorbers" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
