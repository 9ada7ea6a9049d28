"""Host-side checks of the motion drivers (impact_amd/csrc/motion.hip): `ivx_md_eval` — the function the kernel runs — against the numpy
restatement (tests/motion_ref.py) byte for byte, the float32 restatement against its float64 version, the reference's own property tests re-typed,
`ivx_md_apply_host` against the restatement's composition, the validation errors and the record's layout. No kernels are launched here."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import motion_ref as mr
from impact_amd import capi, motion

f32, f64 = np.float32, np.float64
N_SEEDED, SEED = 2000, 1
# The largest error of the float32 restatement against the float64 one over the seeded drivers, relative to the scene's scale (motion_ref.scales:
# lengths against max(|centre| components, extent), speeds against the trajectory's top speed), as measured and recorded in DESIGN.md §4.15; the
# tests allow four times these. Constant rotation: the largest absolute difference of a quaternion component.
MEASURED = {mr.CIRCULAR: (2.2e-5, 6.8e-5), mr.CONSTANT_ACCELERATION: (9.7e-8, 1.3e-7), mr.HARMONIC: (3.7e-5, 5.3e-5), mr.ORBITAL: (3.7e-5, 1.4e-4),
            mr.CONSTANT_ROTATION: (5.7e-5, 0.0)}
ALLOW = 4.0


def lib_eval(kind, p, t):
    d, out = mr.records(kind, p), np.zeros((len(p), 10), dtype=f32)
    lib = capi.lib()
    for i in range(len(p)):
        capi.check(lib.ivx_md_eval(capi.ptr(d[i : i + 1]), float(t[i]), capi.ptr(out[i])))
    return out


@functools.lru_cache(maxsize=None)
def seeded_case(kind):
    """(p, t, float32 restatement, its diagnostics, float64 restatement, its diagnostics): computed once, shared, never written"""
    p, t = mr.seeded(kind, N_SEEDED, SEED)
    d32, d64 = {}, {}
    r32 = mr.evaluate(kind, p, t, d32)
    r64 = mr.evaluate(kind, p.astype(f64), t.astype(f64), d64)
    for a in (p, t, r32, r64):
        a.setflags(write=False)
    return p, t, r32, d32, r64, d64


def assert_bytes_equal(got, want, what):
    bad = np.flatnonzero((np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)).reshape(len(got), -1).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(got)} cases differ, first {bad[:5]}: got {got[bad[0]]}, want {want[bad[0]]}"


# ---- byte equality with the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", range(5), ids=mr.KIND_NAMES)
def test_eval_equals_the_restatement_on_seeded_drivers(kind):
    p, t, r32, d32, _, _ = seeded_case(kind)
    assert_bytes_equal(lib_eval(kind, p, t), r32, mr.KIND_NAMES[kind])


def test_seeded_sets_contain_the_branches():
    _, _, _, d, _, _ = seeded_case(mr.ORBITAL)
    assert (d["sin_v"] > 0).sum() > 100 and (d["sin_v"] < 0).sum() > 100, "both signs of sin v"
    assert (d["iterations"] >= 3).sum() > 100, "orbits that need three Newton iterations or more"
    assert (d["mean_anomaly"] < 0).sum() > 100 and (d["mean_anomaly"] > 0).sum() > 100, "fmod results of both signs (orbital)"
    assert ((d["mean_anomaly"] < 0) & (d["sin_v"] > 0)).sum() > 100, "a time before the periapsis takes the positive root"
    _, _, _, d, _, _ = seeded_case(mr.CIRCULAR)
    assert (d["angle"] < 0).sum() > 100 and (d["angle"] > 0).sum() > 100, "fmod results of both signs (circular)"


def hand_made():
    ident, z3 = [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0]
    tilt = mr.random_orientations(np.random.default_rng(5), 1)[0]
    def orb(t0, q, focus, a, e, period):
        return np.asarray(motion.orbital(0, t0, q, focus, a, e, period)["p"])
    cases = []
    cases.append(("negative mean anomaly", mr.ORBITAL, orb(2.0, tilt, [1, 2, 3], 5.0, 0.3, 4.0), 1.0))
    cases.append(("eccentric anomaly just below pi", mr.ORBITAL, orb(0.0, tilt, z3, 5.0, 0.5, 4.0), 1.99))
    cases.append(("eccentric anomaly just above pi", mr.ORBITAL, orb(0.0, tilt, z3, 5.0, 0.5, 4.0), 2.01))
    cases.append(("eccentricity zero", mr.ORBITAL, orb(0.5, tilt, [3, 2, 1], 2.0, 0.0, 3.0), 1.7))
    cases.append(("several Newton steps", mr.ORBITAL, orb(0.0, ident, z3, 1.0, 0.89, 10.0), 0.4))
    cases.append(("orbit at the periapsis time", mr.ORBITAL, orb(1.5, tilt, z3, 1.0, 0.2, 10.0), 1.5))
    cases.append(("zero angular speed", mr.CONSTANT_ROTATION, np.asarray(motion.constant_rotation(0, 0.0, tilt, [0, 1, 0], 0.0)["p"]), 3.0))
    cases.append(("rotation at the initial time", mr.CONSTANT_ROTATION, np.asarray(motion.constant_rotation(0, 2.5, tilt, [0, 0, 1], 7.0)["p"]), 2.5))
    cases.append(("negative angular speed", mr.CONSTANT_ROTATION, np.asarray(motion.constant_rotation(0, 1.0, tilt, [1, 0, 0], -3.0)["p"]), 2.0))
    cases.append(("circle at the initial time", mr.CIRCULAR, np.asarray(motion.circular(0, 1.25, tilt, [1, 2, 3], 2.0, 3.0)["p"]), 1.25))
    cases.append(("circle with a negative period", mr.CIRCULAR, np.asarray(motion.circular(0, 0.0, tilt, [1, 2, 3], 2.0, -3.0)["p"]), 1.0))
    cases.append(("oscillator at the centre time", mr.HARMONIC, np.asarray(motion.harmonic_oscillator(0, 0.5, [1, 2, 3], [0, 0, 1], 2.0, 3.0)["p"]), 0.5))
    cases.append(("constant acceleration at the initial time", mr.CONSTANT_ACCELERATION, np.asarray(motion.constant_acceleration(0, 0.5, [1, 2, 3], [4, 5, 6], [7, 8, 9])["p"]), 0.5))
    return cases


@pytest.mark.parametrize("name,kind,p,t", hand_made(), ids=[c[0] for c in hand_made()])
def test_eval_equals_the_restatement_on_hand_made_cases(name, kind, p, t):
    p, t = p[None].astype(f32), np.array([t], dtype=f32)
    diag = {}
    want = mr.evaluate(kind, p, t, diag)
    assert_bytes_equal(lib_eval(kind, p, t), want, name)
    if name == "negative mean anomaly":
        assert diag["mean_anomaly"][0] < 0 and diag["sin_v"][0] > 0
    if name.startswith("eccentric anomaly just"):
        below = "below" in name
        assert (diag["eccentric_anomaly"][0] <= mr.PI32) == below and (diag["sin_v"][0] > 0) == below
        assert abs(float(diag["eccentric_anomaly"][0]) - math.pi) < 0.05
    if name == "several Newton steps":
        assert diag["iterations"][0] >= 3
    if name == "eccentricity zero":
        assert diag["iterations"][0] == 1 and diag["eccentric_anomaly"][0] == diag["mean_anomaly"][0]  # (the first step already moves by zero)
    if name in ("zero angular speed", "rotation at the initial time"):
        np.testing.assert_allclose(want[0, 0:4], p[0, 1:5], atol=1e-6)


# ---- the float32 restatement against float64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", range(5), ids=mr.KIND_NAMES)
def test_float32_restatement_against_float64(kind):
    p, t, r32, d32, r64, d64 = seeded_case(kind)
    bound_a, bound_b = MEASURED[kind]
    if kind == mr.CONSTANT_ROTATION:
        # (q and -q are the same orientation; the two precisions never land on opposite signs here, as the figure shows)
        err = np.abs(r32[:, 0:4].astype(f64) - r64[:, 0:4]).max()
        print(f"{mr.KIND_NAMES[kind]}: largest quaternion component error {err:.3e} (recorded {bound_a:.1e})")
        assert err <= ALLOW * bound_a
        return
    length, speed = mr.scales(kind, p, t)
    keep = np.ones(len(p), dtype=bool)
    if kind == mr.ORBITAL:
        # left out of THIS comparison only: an eccentric anomaly within the bound of pi (the sign of sin v may differ between the precisions), a
        # different number of Newton iterations
        keep = (np.abs(d64["eccentric_anomaly"] - math.pi) > ALLOW * bound_a) & (d32["iterations"] == d64["iterations"])
        share = 1.0 - keep.mean()
        print(f"orbital: {np.count_nonzero(~keep)} of {len(p)} cases left out ({100 * share:.2f} %)")
        assert share <= 0.01
    err_pos = (np.abs(r32[:, 0:3].astype(f64) - r64[:, 0:3]).max(axis=1) / length)[keep].max()
    err_vel = (np.abs(r32[:, 3:6].astype(f64) - r64[:, 3:6]).max(axis=1) / speed)[keep].max()
    print(f"{mr.KIND_NAMES[kind]}: position {err_pos:.3e} (recorded {bound_a:.1e}), velocity {err_vel:.3e} (recorded {bound_b:.1e})")
    assert err_pos <= ALLOW * bound_a and err_vel <= ALLOW * bound_b


# ---- the reference's property tests, against ivx_md_eval, with the reference's epsilons and its uniform ranges -----------------------------------------
N_PROP = 256


def one(kind, p, t):
    return lib_eval(kind, np.asarray(p, dtype=f32)[None], np.array([t], dtype=f32))[0]


def unit(v):
    return v / np.linalg.norm(v)


def orbital_cases(seed):
    rng = np.random.default_rng(seed)
    q = mr.random_orientations(rng, N_PROP)
    for i in range(N_PROP):
        yield (f32(rng.uniform(-10, 10)), q[i], rng.uniform(-100, 100, 3).astype(f32), f32(rng.uniform(1e-2, 1e2)), f32(rng.uniform(0.0, 0.9)),
               f32(rng.uniform(1e-1, 1e2)), int(rng.integers(0, 20)), f32(rng.uniform(-10, 10)))


def test_orbit_periapsis_and_apoapsis_at_whole_and_half_periods():
    """orbit.rs: should_get_periapsis_and_apoapsis_position_at_whole_and_half_periods_from_periapsis_time,
    should_get_velocities_normal_to_displacement_at_periapsis_and_apoapsis"""
    for t0, q, focus, a, e, period, n, _ in orbital_cases(11):
        p = motion.orbital(0, t0, q, focus, a, e, period)["p"]
        t_peri = f32(t0 + f32(n) * period)
        t_apo = f32(t_peri + f32(0.5) * period)
        d_peri = a * (f32(1) - e * e) / (f32(1) + e)
        d_apo = a * (f32(1) - e * e) / (f32(1) - e)
        peri, apo = one(mr.ORBITAL, p, t_peri), one(mr.ORBITAL, p, t_apo)
        want_peri = focus + mr.qrot(q, np.array([d_peri, 0, 0], dtype=f32))
        want_apo = focus + mr.qrot(q, np.array([-d_apo, 0, 0], dtype=f32))
        assert np.abs(peri[0:3] - want_peri).max() <= 1e-3 * a and np.abs(apo[0:3] - want_apo).max() <= 1e-3 * a
        assert abs(np.dot(unit(peri[3:6]), unit(peri[0:3] - focus))) <= 1e-2
        assert abs(np.dot(unit(apo[3:6]), unit(apo[0:3] - focus))) <= 1e-2


def test_orbit_with_zero_eccentricity_is_circular():
    """orbit.rs: should_get_circular_position_and_velocity_with_zero_eccentricity"""
    for t0, q, center, radius, _, period, _, t in orbital_cases(12):
        o = one(mr.ORBITAL, motion.orbital(0, t0, q, center, radius, 0.0, period)["p"], t)
        displacement, velocity = o[0:3] - center, o[3:6]
        assert abs(np.linalg.norm(displacement) - radius) <= 1e-3 * radius
        assert abs(np.linalg.norm(velocity) - mr.TWO_PI32 * radius / period) <= 1e-3 * radius / period
        assert abs(np.dot(unit(velocity), unit(displacement))) <= 1e-3


def harmonic_cases(seed):
    rng = np.random.default_rng(seed)
    d = mr.random_directions(rng, N_PROP)
    for i in range(N_PROP):
        yield (f32(rng.uniform(-10, 10)), rng.uniform(-100, 100, 3).astype(f32), d[i], f32(rng.uniform(-100, 100)), f32(rng.uniform(1e-1, 1e2)), int(rng.integers(0, 20)))


def test_oscillator_centre_at_half_periods_and_peaks_at_quarter_periods():
    """harmonic_oscillation.rs: should_get_center_position_at_half_periods_from_center_time,
    should_get_peak_position_and_zero_velocity_at_quarter_periods_from_center_time"""
    for t0, center, direction, amplitude, period, n in harmonic_cases(13):
        p = motion.harmonic_oscillator(0, t0, center, direction, amplitude, period)["p"]
        o = one(mr.HARMONIC, p, f32(t0 + f32(n) * f32(0.5) * period))
        assert np.abs(o[0:3] - center).max() <= 1e-3 * np.abs(center).max()
        tc = f32(t0 + f32(n) * period)
        for sign in (1, -1):
            o = one(mr.HARMONIC, p, f32(tc + f32(sign) * f32(0.25) * period))
            peak = center + f32(sign) * amplitude * direction
            assert np.abs(o[0:3] - peak).max() <= 1e-3 * np.abs(peak).max()
            assert np.abs(o[3:6]).max() <= 5e-1


def test_rotation_gives_the_initial_orientation_at_the_initial_time():
    """constant_rotation.rs: should_get_initial_orientation_at_initial_time, should_get_initial_orientation_for_zero_angular_velocity,
    should_get_different_orientation_for_nonzero_angular_velocity"""
    rng = np.random.default_rng(14)
    q, axis = mr.random_orientations(rng, N_PROP), mr.random_directions(rng, N_PROP)
    for i in range(N_PROP):
        t = f32(rng.uniform(-100, 100))
        o = one(mr.CONSTANT_ROTATION, motion.constant_rotation(0, t, q[i], axis[i], rng.uniform(-100, 100))["p"], t)
        assert np.abs(o[0:4] - q[i]).max() <= 1e-6
    ident = np.array([0, 0, 0, 1], dtype=f32)
    assert np.abs(one(mr.CONSTANT_ROTATION, motion.constant_rotation(0, 0.0, ident, [0, 1, 0], 0.0)["p"], 1.0)[0:4] - ident).max() <= 1e-6
    assert np.abs(one(mr.CONSTANT_ROTATION, motion.constant_rotation(0, 0.0, ident, [0, 1, 0], 1.0)["p"], 1.0)[0:4] - ident).max() > 1e-6


# ---- the composition -------------------------------------------------------------------------------------------------------------------------
def random_bodies(rng, n):
    k = np.zeros(n, dtype=capi.KINEMATIC_BODY_DTYPE)
    k["position"], k["velocity"] = rng.uniform(-10, 10, (n, 3)), rng.uniform(-10, 10, (n, 3))
    k["orientation"], k["angular_axis"], k["angular_speed"] = mr.random_orientations(rng, n), mr.random_directions(rng, n), rng.uniform(-3, 3, n)
    return k


def driver_of(kind, body, seed):
    p, _ = mr.seeded(kind, 1, seed)
    return mr.records(kind, p, body)[0]


def assert_bodies_equal(got, want, what=""):
    assert got.tobytes() == want.tobytes(), f"{what}: bodies differ at {np.flatnonzero([g.tobytes() != w.tobytes() for g, w in zip(got, want)])}"


def test_apply_host_equals_the_restatement():
    """bodies with 0, 1, 2 and 5 drivers, given out of order; undriven bodies keep their bytes"""
    bodies = random_bodies(np.random.default_rng(21), 9)
    drivers = np.array([driver_of(mr.CONSTANT_ROTATION, 7, 1), driver_of(mr.ORBITAL, 7, 2), driver_of(mr.HARMONIC, 3, 3), driver_of(mr.CIRCULAR, 7, 4),
                        driver_of(mr.CONSTANT_ACCELERATION, 5, 5), driver_of(mr.HARMONIC, 7, 6), driver_of(mr.CIRCULAR, 5, 7),
                        driver_of(mr.CONSTANT_ACCELERATION, 7, 8)], dtype=capi.MOTION_DRIVER_DTYPE)
    for time in (0.0, 1.37, -4.5):
        got, want = motion.apply_host(drivers, bodies, time), mr.apply(drivers, bodies, time)
        assert_bodies_equal(got, want, f"time {time}")
        for b in (0, 1, 2, 4, 6, 8):
            assert got[b].tobytes() == bodies[b].tobytes()
        assert got[7].tobytes() != bodies[7].tobytes() and got[3]["position"].tobytes() != bodies[3]["position"].tobytes()
    assert_bodies_equal(motion.apply_host(drivers[:0], bodies, 1.0), bodies, "no drivers")


def test_apply_host_adds_one_kind_in_list_order():
    """two drivers of one kind in both list orders: each result is the restatement's for that order (float32 sums do not commute with a third term)"""
    bodies = random_bodies(np.random.default_rng(22), 2)
    differ = 0
    for seed in range(40):
        a, b, c = driver_of(mr.CIRCULAR, 1, 100 + seed), driver_of(mr.CIRCULAR, 1, 200 + seed), driver_of(mr.CIRCULAR, 1, 300 + seed)
        results = []
        for order in ([a, b, c], [c, b, a]):
            d = np.array(order, dtype=capi.MOTION_DRIVER_DTYPE)
            got = motion.apply_host(d, bodies, 0.75)
            assert_bodies_equal(got, mr.apply(d, bodies, 0.75), f"seed {seed}")
            results.append(got)
        differ += results[0].tobytes() != results[1].tobytes()
    assert differ > 0, "no seeded triple distinguishes the two orders"


def test_apply_host_rotation_only_trajectory_only_and_last_rotation_wins():
    bodies = random_bodies(np.random.default_rng(23), 3)
    r1, r2 = driver_of(mr.CONSTANT_ROTATION, 0, 31), driver_of(mr.CONSTANT_ROTATION, 0, 32)
    d = np.array([r1, r2, driver_of(mr.HARMONIC, 2, 33)], dtype=capi.MOTION_DRIVER_DTYPE)
    got = motion.apply_host(d, bodies, 2.0)
    assert_bodies_equal(got, mr.apply(d, bodies, 2.0))
    for f in ("position", "velocity"):
        assert got[0][f].tobytes() == bodies[0][f].tobytes()
    for f in ("orientation", "angular_axis", "angular_speed"):
        assert got[2][f].tobytes() == bodies[2][f].tobytes()
    assert got[0]["angular_speed"] == r2["p"][8] and got[0]["angular_speed"] != r1["p"][8]
    swapped = motion.apply_host(d[[1, 0, 2]], bodies, 2.0)
    assert_bodies_equal(swapped, mr.apply(d[[1, 0, 2]], bodies, 2.0))
    assert swapped[0]["angular_speed"] == r1["p"][8]


def test_a_lone_negative_zero_contribution_comes_out_positive():
    nz = f32(-0.0)
    d = motion.constant_acceleration(0, 0.0, [nz, 1.0, 2.0], [nz, 0.0, 0.0], [nz, 0.0, 0.0])
    o = motion.evaluate(d, 1.0)
    assert o[0] == 0 and np.signbit(o[0]) and o[3] == 0 and np.signbit(o[3]), "the contribution itself is -0.0"
    bodies = random_bodies(np.random.default_rng(24), 1)
    got = motion.apply_host([d], bodies, 1.0)
    assert_bodies_equal(got, mr.apply([d], bodies, 1.0))
    assert got[0]["position"][0] == 0 and not np.signbit(got[0]["position"][0]) and not np.signbit(got[0]["velocity"][0])


# ---- validation and layout ---------------------------------------------------------------------------------------------------------------------
IDENT, ZERO3 = [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0]
EPS = float(np.finfo(f32).eps)
BAD_DRIVERS = {
    "circular radius zero": motion.circular(0, 0.0, IDENT, ZERO3, 0.0, 1.0),
    "circular radius negative": motion.circular(0, 0.0, IDENT, ZERO3, -0.1, 1.0),
    "circular radius nan": motion.circular(0, 0.0, IDENT, ZERO3, math.nan, 1.0),
    "circular period zero": motion.circular(0, 0.0, IDENT, ZERO3, 1.0, 0.0),
    "circular period epsilon": motion.circular(0, 0.0, IDENT, ZERO3, 1.0, -EPS),
    "harmonic period zero": motion.harmonic_oscillator(0, 0.0, ZERO3, [1.0, 0.0, 0.0], 1.0, 0.0),
    "orbital axis zero": motion.orbital(0, 0.0, IDENT, ZERO3, 0.0, 0.0, 1.0),
    "orbital axis negative": motion.orbital(0, 0.0, IDENT, ZERO3, -0.1, 0.0, 1.0),
    "orbital eccentricity negative": motion.orbital(0, 0.0, IDENT, ZERO3, 1.0, -0.1, 1.0),
    "orbital eccentricity one": motion.orbital(0, 0.0, IDENT, ZERO3, 1.0, 1.0, 1.0),
    "orbital period zero": motion.orbital(0, 0.0, IDENT, ZERO3, 1.0, 0.0, 0.0),
    "unknown kind": motion._driver(5, 0, 0.0),
}


@pytest.mark.parametrize("name", list(BAD_DRIVERS))
def test_validation_errors(name):
    bad = BAD_DRIVERS[name]
    with pytest.raises(capi.IvxError) as e:
        motion.evaluate(bad, 1.0)
    assert e.value.code == capi.IVX_ERR_INVALID
    good = motion.constant_velocity(0, 0.0, ZERO3, [1.0, 0.0, 0.0])
    bodies = np.zeros(1, dtype=capi.KINEMATIC_BODY_DTYPE)
    with pytest.raises(capi.IvxError) as e:
        motion.apply_host([good, bad], bodies, 1.0)
    assert e.value.code == capi.IVX_ERR_INVALID and "driver 1" in str(e.value), str(e.value)


def test_smallest_valid_period_and_body_index():
    just_above = float(np.nextafter(f32(EPS), f32(1)))
    motion.evaluate(motion.circular(0, 0.0, IDENT, ZERO3, 1.0, just_above), 0.0)
    bodies = np.zeros(2, dtype=capi.KINEMATIC_BODY_DTYPE)
    motion.apply_host([motion.constant_velocity(1, 0.0, ZERO3, ZERO3)], bodies, 1.0)
    with pytest.raises(capi.IvxError) as e:
        motion.apply_host([motion.constant_velocity(1, 0.0, ZERO3, ZERO3), motion.constant_velocity(2, 0.0, ZERO3, ZERO3)], bodies, 1.0)
    assert e.value.code == capi.IVX_ERR_INVALID and "driver 1" in str(e.value) and "body 2" in str(e.value), str(e.value)
    with pytest.raises(capi.IvxError) as e:
        capi.check(capi.lib().ivx_md_eval(None, 0.0, None))
    assert e.value.code == capi.IVX_ERR_INVALID


def test_record_layout_matches_the_c_compiler(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "impact_voxel_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu\\n", sizeof(ivx_motion_driver), offsetof(ivx_motion_driver, kind), offsetof(ivx_motion_driver, body), '
                   'offsetof(ivx_motion_driver, p));\n'
                   '    printf("%u %u %u %u %u\\n", IVX_MD_CIRCULAR, IVX_MD_CONSTANT_ACCELERATION, IVX_MD_HARMONIC, IVX_MD_ORBITAL, IVX_MD_CONSTANT_ROTATION);\n'
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.run(["gcc", "-I", inc, str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    dt = capi.MOTION_DRIVER_DTYPE
    assert [int(x) for x in lines[0].split()] == [dt.itemsize, dt.fields["kind"][1], dt.fields["body"][1], dt.fields["p"][1]] == [64, 0, 4, 8]
    assert [int(x) for x in lines[1].split()] == [capi.MD_CIRCULAR, capi.MD_CONSTANT_ACCELERATION, capi.MD_HARMONIC, capi.MD_ORBITAL, capi.MD_CONSTANT_ROTATION]
    assert capi.extra_struct_sizes()["ivx_motion_driver"] == (dt, 64)
