"""Detailed drag, the host-only exports (no GPU): the direction samples, the cell indices of the equirectangular map, the force and torque
on one body from a map, and the layouts of the two records — against the numpy restatement in drag_ref.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import drag_ref as dr
from impact_amd import capi, drag

H = np.pi / 6.0  # half a cell of a map with three theta coordinates


@pytest.mark.parametrize("n", [1, 2, 200, 5000])
def test_directions_match_the_f32_formula(n):
    """the azimuth product rounds the same way in numpy f32 and in the library; sinf / cosf differ by ulps"""
    got = drag.uniformly_distributed_radial_directions(n)
    want = dr.directions_f32(n)
    assert got.shape == (n, 3) and got.dtype == np.float32
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    unit = float(np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1.0).max())
    print(f"n = {n}: max component difference {err:.3g}, max | |d| - 1 | {unit:.3g}")
    assert err <= 2e-6
    assert unit <= 1e-6
    if n > 1:  # from the north pole to the south pole
        assert got[0, 2] == 1.0 and got[-1, 2] == -1.0


def test_zero_directions_is_an_error():
    out = np.zeros((1, 3), dtype=np.float32)
    assert capi.lib().ivx_drag_directions(0, capi.ptr(out)) == capi.IVX_ERR_INVALID
    assert b"zero" in capi.lib().ivx_last_error()


def indices(n_theta, phi, theta):
    pi, ti = C.c_uint32(99), C.c_uint32(99)
    capi.check(capi.lib().ivx_drag_map_indices(n_theta, phi, theta, C.byref(pi), C.byref(ti)))
    return int(pi.value), int(ti.value)


@pytest.mark.parametrize("phi,want", [(H, 0), (3 * H, 1), (-H, 5), (2 * np.pi + H, 0)])
def test_phi_index_known_answers(phi, want):
    assert indices(3, phi, H)[0] == want


@pytest.mark.parametrize("theta,want", [(H, 0), (-H, 0), (3 * H, 1), (np.pi - H, 2), (np.pi + H, 2)])
def test_theta_index_known_answers(theta, want):
    assert indices(3, H, theta)[1] == want


def test_indices_stay_inside_the_map_at_the_seams():
    for phi in (0.0, 2.0 * np.pi, float(np.float32(2.0 * np.pi)), -1e-9, float(np.nextafter(np.float32(0.0), np.float32(-1.0)))):
        assert indices(3, phi, H)[0] < 6, phi
    for theta in (0.0, np.pi, float(np.float32(np.pi)), -1e-9, 2.0 * np.pi):
        assert indices(3, H, theta)[1] < 3, theta
    for n_theta in (1, 7, 64):  # a tiny negative azimuth: its remainder rounds to 2 pi itself
        pi_, ti_ = indices(n_theta, -1e-30, np.pi)
        assert pi_ == 2 * n_theta - 1 and ti_ == n_theta - 1
    pi, ti = C.c_uint32(), C.c_uint32()
    assert capi.lib().ivx_drag_map_indices(0, 0.0, 0.0, C.byref(pi), C.byref(ti)) == capi.IVX_ERR_INVALID
    assert capi.lib().ivx_drag_map_indices(3, float("nan"), 0.0, C.byref(pi), C.byref(ti)) == capi.IVX_ERR_INVALID


def indices_agree_with_restatement_case(n_theta, rng):
    phi, theta = rng.uniform(-10.0, 10.0), rng.uniform(-10.0, 10.0)
    cell = np.pi / n_theta
    a, b = dr.rem_euclid(phi, dr.TWO_PI) / cell, float(dr.folded_theta(theta)) / cell
    if min(a - np.floor(a), np.ceil(a) - a, b - np.floor(b), np.ceil(b) - b) < 1e-3:
        return  # decided within f32 rounding of the angle
    assert indices(n_theta, phi, theta) == (int(dr.phi_index(phi, n_theta)), int(dr.theta_index(theta, n_theta)))


def test_indices_agree_with_the_restatement():
    rng = np.random.default_rng(11)
    for n_theta in (1, 3, 8, 64):
        for _ in range(200):
            indices_agree_with_restatement_case(n_theta, rng)


def seeded_map(n_theta, seed):
    rng = np.random.default_rng(seed)
    m = np.zeros((n_theta, 2 * n_theta), dtype=capi.DRAG_LOAD_DTYPE)
    m["force"] = rng.normal(size=(n_theta, 2 * n_theta, 3)).astype(np.float32)
    m["torque"] = rng.normal(size=(n_theta, 2 * n_theta, 3)).astype(np.float32)
    return m


def seeded_body(n_theta, seed):
    """a body whose direction of motion relative to the medium lies at least 0.1 cell from every cell edge of the map"""
    rng = np.random.default_rng(seed)
    cell = np.pi / n_theta
    while True:
        b = np.zeros(1, dtype=capi.RIGID_BODY_DTYPE)
        b["mass"] = rng.uniform(0.5, 20.0)
        q = rng.normal(size=4)
        b["orientation"] = (q / np.linalg.norm(q)).astype(np.float32)
        b["momentum"] = rng.normal(size=3) * 10.0
        b["angular_momentum"] = rng.normal(size=3)
        b["position"] = rng.normal(size=3)
        b["total_force"] = rng.normal(size=3)
        b["total_torque"] = rng.normal(size=3)
        medium = rng.normal(size=3).astype(np.float32)
        d, _ = dr.body_space_direction(b[0], medium)
        a = dr.rem_euclid(np.arctan2(d[1], d[0]), dr.TWO_PI) / cell
        t = np.arccos(np.clip(d[2], -1.0, 1.0)) / cell
        if min(a - np.floor(a), np.ceil(a) - a, t - np.floor(t), np.ceil(t) - t) >= 0.1:
            return b, medium


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_force_and_torque_match_the_restatement(seed):
    n_theta = (3, 8, 64)[seed - 1]
    m = seeded_map(n_theta, 100 + seed)
    body, medium = seeded_body(n_theta, seed)
    density, cd, scaling = 1.2 + seed, 0.47 * seed, 0.5 + 0.75 * seed
    want_f, want_t = dr.force_and_torque(m, body[0], medium, density, cd, scaling)
    before = body.copy()
    out = drag.DetailedDragForce(drag.DragLoadMap(m), cd, scaling).apply(body, (medium, density))
    assert out is not None and np.shares_memory(out, body)  # in place
    got_f = body[0]["total_force"].astype(np.float64) - before[0]["total_force"].astype(np.float64)
    got_t = body[0]["total_torque"].astype(np.float64) - before[0]["total_torque"].astype(np.float64)
    # what is compared is the sum the library stored: the body's prior total is part of the f32 rounding
    tol_f = 1e-5 * (np.linalg.norm(want_f) + np.linalg.norm(before[0]["total_force"]))
    tol_t = 1e-5 * (np.linalg.norm(want_t) + np.linalg.norm(before[0]["total_torque"]))
    print(f"seed {seed}: |dF| {np.abs(got_f - want_f).max():.3g} of |F| {np.linalg.norm(want_f):.3g}; |dT| {np.abs(got_t - want_t).max():.3g} of |T| {np.linalg.norm(want_t):.3g}")
    assert np.linalg.norm(got_f - want_f) <= tol_f
    assert np.linalg.norm(got_t - want_t) <= tol_t
    for f in ("mass", "inertia", "inv_inertia", "position", "orientation", "momentum", "angular_momentum"):
        np.testing.assert_array_equal(body[f], before[f])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_force_alone_meets_the_rigid_body_tolerance(seed):
    """the same from zero totals: 1e-5 relative to |F| and to |T|"""
    n_theta = (3, 8, 64)[seed - 1]
    m = seeded_map(n_theta, 100 + seed)
    body, medium = seeded_body(n_theta, seed)
    body["total_force"] = 0.0
    body["total_torque"] = 0.0
    density, cd, scaling = 1.2 + seed, 0.47 * seed, 0.5 + 0.75 * seed
    want_f, want_t = dr.force_and_torque(m, body[0], medium, density, cd, scaling)
    drag.DetailedDragForce(drag.DragLoadMap(m), cd, scaling).apply(body, (medium, density))
    ef = np.linalg.norm(body[0]["total_force"].astype(np.float64) - want_f) / np.linalg.norm(want_f)
    et = np.linalg.norm(body[0]["total_torque"].astype(np.float64) - want_t) / np.linalg.norm(want_t)
    print(f"seed {seed}: relative force error {ef:.3g}, relative torque error {et:.3g}")
    assert ef <= 1e-5 and et <= 1e-5


def test_a_body_at_rest_in_the_medium_is_left_untouched():
    m = seeded_map(8, 5)
    body, _ = seeded_body(8, 5)
    body["mass"] = 2.0
    body["momentum"] = (2.0, 4.0, -6.0)
    medium = np.array([1.0, 2.0, -3.0], dtype=np.float32)
    before = body.copy()
    drag.DetailedDragForce(drag.DragLoadMap(m), 0.5, 1.0).apply(body, (medium, 1.0))
    assert body.tobytes() == before.tobytes()


def test_force_and_torque_reject_bad_arguments():
    m = seeded_map(3, 1)
    body, medium = seeded_body(3, 1)
    L = capi.lib()
    assert L.ivx_drag_force_and_torque(None, 3, capi.ptr(body), capi.ptr(medium), 1.0, 1.0, 1.0) == capi.IVX_ERR_INVALID
    assert L.ivx_drag_force_and_torque(capi.ptr(m), 0, capi.ptr(body), capi.ptr(medium), 1.0, 1.0, 1.0) == capi.IVX_ERR_INVALID


def test_config_default():
    c = drag.DragLoadMapConfig()
    assert (c.n_direction_samples, c.n_theta_coords, c.smoothness) == (5000, 64, 2.0)
    assert abs(c.angular_interpolation_distance() - 2.0 * np.sqrt(4.0 * np.pi / 5000.0)) < 1e-7
    r = np.full(1, 0xFF, dtype=np.uint8).repeat(16).view(capi.DRAG_MAP_CONFIG_DTYPE)
    capi.lib().ivx_drag_map_config_default(capi.ptr(r))
    assert r[0]["reserved"] == 0 and r.tobytes() == c.as_record().tobytes()


def test_drag_struct_sizes_match_the_c_compiler(tmp_path):
    """the numpy mirrors of the two drag records against `sizeof` as gcc lays the header's structs out"""
    pairs = {"ivx_drag_load": (capi.DRAG_LOAD_DTYPE, 24), "ivx_drag_map_config": (capi.DRAG_MAP_CONFIG_DTYPE, 16)}
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "impact_voxel_hip.h"\nint main(void) {\n' +
                   "".join(f'    printf("{n} %zu\\n", sizeof({n}));\n' for n in pairs) + "    return 0;\n}\n")
    exe = tmp_path / "sizes"
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.run(["gcc", "-I", inc, str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for n, (dt, size) in pairs.items():
        assert int(got[n]) == dt.itemsize == size, f"{n}: the header's struct is {got[n]} bytes, its numpy mirror {dt.itemsize}"
    assert capi.DRAG_LOAD_DTYPE.fields["torque"][1] == 12 and capi.DRAG_MAP_CONFIG_DTYPE.fields["smoothness"][1] == 8


def test_device_entry_points_fail_loudly_without_a_context():
    """argument checks that need no device: null handles and bad counts are IVX_ERR_INVALID with a message, never a quiet result"""
    L = capi.lib()
    d = np.zeros((1, 3), dtype=np.float32)
    out = np.zeros(1, dtype=capi.DRAG_LOAD_DTYPE)
    assert L.ivx_drag_loads_triangles(None, None, 0, None, 0, capi.ptr(d[0]), capi.ptr(d), 1, capi.ptr(out)) == capi.IVX_ERR_INVALID
    assert L.ivx_drag_loads(None, capi.ptr(d[0]), capi.ptr(d), 1, capi.ptr(out)) == capi.IVX_ERR_INVALID
    assert L.ivx_drag_load_map_from_samples(None, capi.ptr(d), capi.ptr(out), 1, 1, 0.5, capi.ptr(out)) == capi.IVX_ERR_INVALID
    assert L.ivx_drag_load_map(None, capi.ptr(d[0]), None, capi.ptr(out)) == capi.IVX_ERR_INVALID
    assert L.ivx_last_error()
