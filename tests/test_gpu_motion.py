"""Device checks of the motion drivers (impact_amd/csrc/motion.hip): `ivx_world_apply_motion` against `ivx_md_apply_host` over the same bodies, the
sizes around a wave and a workgroup, the world's clock, whole steps with and without contacts against the oracle world whose kinematic bodies
are driven by the numpy restatement (tests/motion_ref.py), and replacing, removing and outliving the driver set."""
import ctypes as C

import numpy as np
import pytest

import motion_ref as mr
import narrow_ref as nr
import oracle_lib as ol
import physics_util as phu
from impact_amd import capi, collision, motion
from impact_amd.physics import PhysicsWorld

pytestmark = pytest.mark.gpu

f32 = np.float32
NONE = np.zeros(0, dtype=capi.CONTACT_DTYPE)


def kinematic_bodies(n, seed):
    rng = np.random.default_rng(seed)
    k = np.zeros(n, dtype=capi.KINEMATIC_BODY_DTYPE)
    k["position"], k["velocity"] = rng.uniform(-10, 10, (n, 3)), rng.uniform(-10, 10, (n, 3))
    k["orientation"], k["angular_axis"], k["angular_speed"] = mr.random_orientations(rng, n), mr.random_directions(rng, n), rng.uniform(-3, 3, n)
    return k


def dynamic_bodies(n, seed):
    rng = np.random.default_rng(seed)
    dyn = []
    for _ in range(n):
        q = rng.normal(size=4)
        dyn.append(ol.rigid_body_new(rng.uniform(0.5, 3.0), np.diag(rng.uniform(0.5, 2.0, 3)), rng.normal(size=3), q / np.linalg.norm(q), rng.normal(size=3), rng.normal(size=3)))
    dyn = np.array(dyn)
    dyn["total_force"], dyn["total_torque"] = rng.normal(size=(n, 3)).astype(f32), rng.normal(size=(n, 3)).astype(f32)
    return dyn


def seeded_drivers(bodies, seed, kinds=range(5)):
    """one driver per entry of `bodies`, the kinds in turn, parameters from the reference's proptest ranges"""
    kinds = list(kinds)
    out = np.zeros(len(bodies), dtype=capi.MOTION_DRIVER_DTYPE)
    for i, b in enumerate(bodies):
        kind = kinds[i % len(kinds)]
        out[i] = mr.records(kind, mr.seeded(kind, 1, seed * 1000 + i)[0], b)[0]
    return out


def assert_kinematic_equal(got, want, what):
    if got.tobytes() != want.tobytes():
        bad = [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()]
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} kinematic bodies differ, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}")


def world_with(ctx, kin, drivers, dyn=None):
    w = PhysicsWorld(ctx)
    w.set_bodies(np.zeros(0, dtype=capi.RIGID_BODY_DTYPE) if dyn is None else dyn, kin)
    md = motion.MotionDrivers(w)
    md.set(drivers)
    return w, md


# ---- apply and read back ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_driven", [1, 63, 64, 65, 255, 256, 257])
def test_apply_equals_the_host_composition(ctx, n_driven):
    """a lane per driven body around a wave and a workgroup; one driver each, the five kinds in turn; two undriven bodies at the end"""
    kin = kinematic_bodies(n_driven + 2, 40 + n_driven)
    drivers = seeded_drivers(range(n_driven), n_driven)
    w, md = world_with(ctx, kin, drivers)
    for time in (0.0, 3.25):
        md.apply(time)
        got = w.bodies()[1]
        assert_kinematic_equal(got, motion.apply_host(drivers, kin, time), f"time {time}")
        assert got[n_driven:].tobytes() == kin[n_driven:].tobytes()
        w.set_bodies(np.zeros(0, dtype=capi.RIGID_BODY_DTYPE), kin)
    assert md.time == 0.0  # (the stage on its own does not touch the clock)
    w.close()


def test_every_fourth_body_driven_and_five_drivers_beside_one(ctx):
    kin = kinematic_bodies(1024, 50)
    driven = list(range(1, 1024, 4))
    drivers = seeded_drivers(driven, 51)
    rng = np.random.default_rng(52)
    w, md = world_with(ctx, kin, drivers[rng.permutation(len(drivers))])  # (the list in any order: the set is sorted by body)
    md.apply(-2.5)
    got = w.bodies()[1]
    assert_kinematic_equal(got, motion.apply_host(drivers, kin, -2.5), "every fourth")
    undriven = np.setdiff1d(np.arange(1024), driven)
    assert got[undriven].tobytes() == kin[undriven].tobytes()
    # body 5 with one driver of every kind — given rotation first — between bodies with one driver each, and a second orbit on body 5
    five = np.concatenate([seeded_drivers([5] * 5, 53, kinds=[4, 3, 2, 1, 0]), seeded_drivers([4, 6, 5], 54, kinds=[3, 0, 3])])
    w.set_bodies(np.zeros(0, dtype=capi.RIGID_BODY_DTYPE), kin[:8])
    md.set(five)
    md.apply(1.5)
    got = w.bodies()[1]
    assert_kinematic_equal(got, motion.apply_host(five, kin[:8], 1.5), "five drivers")
    assert_kinematic_equal(got, mr.apply(five, kin[:8], 1.5), "five drivers, the restatement")
    w.close()


def test_no_drivers_is_no_launch_and_no_change(ctx):
    kin = kinematic_bodies(70, 60)
    w = PhysicsWorld(ctx)
    w.set_bodies(np.zeros(0, dtype=capi.RIGID_BODY_DTYPE), kin)
    md = motion.MotionDrivers(w)
    md.apply(1.0)
    assert w.bodies()[1].tobytes() == kin.tobytes()
    md.set([])
    md.apply(1.0)
    assert w.bodies()[1].tobytes() == kin.tobytes()
    w.close()


# ---- the clock -----------------------------------------------------------------------------------------------------------------------------
def test_the_clock_is_the_float32_running_sum(ctx):
    w = PhysicsWorld(ctx)
    w.set_bodies(dynamic_bodies(3, 70), kinematic_bodies(2, 71))
    md = motion.MotionDrivers(w)
    assert md.time == 0.0
    t = f32(0)
    for k in range(10):
        if k % 2:
            w.step(0.004)
        else:
            w.step_enqueue(0.004)
        t = f32(t + f32(0.004))
        assert md.time == float(t)
    assert t != f32(0.04)  # (the running sum, not the product)
    md.time = 7.5
    t = f32(7.5)
    for _ in range(3):
        w.step(0.004)
        t = f32(t + f32(0.004))
    assert md.time == float(t)
    w.close()


# ---- whole steps -----------------------------------------------------------------------------------------------------------------------------
def drive_oracle(o, drivers, time):
    """what the step's tail does, on the oracle world: its kinematic bodies overwritten with the restatement's composition (the oracle keeps its
    constraint cache over orc_physics_set_bodies) -> (the kinematic bodies before, after)"""
    dyn, kin = o.bodies()
    driven = mr.apply(drivers, kin, time)
    ol.lib().orc_physics_set_bodies(o.h, ol._p(dyn), len(dyn), ol._p(driven), len(driven))
    return kin, driven


def test_twenty_enqueued_steps_without_contacts(ctx):
    """dynamic bodies under force and torque beside kinematic bodies: one driven by each kind, one by all five, one by two circles, one undriven"""
    dyn, kin = dynamic_bodies(8, 80), kinematic_bodies(8, 81)
    drivers = np.concatenate([seeded_drivers(range(5), 82), seeded_drivers([5] * 5, 83), seeded_drivers([6, 6], 84, kinds=[0])])
    w, md = world_with(ctx, kin, drivers, dyn)
    plain = PhysicsWorld(ctx)  # the same bodies without a driver set
    plain.set_bodies(dyn, kin)
    o = ol.OraclePhysics(dyn, kin)
    t, dt = f32(0), 0.004
    for _ in range(20):
        w.step_enqueue(dt)
        plain.step_enqueue(dt)
        o.step(NONE, dt)
        t = f32(t + f32(dt))
        advanced, _ = drive_oracle(o, drivers, t)
    got_dyn, got_kin = w.bodies()  # (the one wait)
    want_dyn, want_kin = o.bodies()
    assert md.time == float(t)
    assert got_dyn.tobytes() == plain.bodies()[0].tobytes(), "dynamic bodies never see a driver"
    differ = [f for f in phu.STATE_FIELDS if got_dyn[f].tobytes() != want_dyn[f].tobytes()]
    print("dynamic fields that differ from the oracle:", differ, [float(np.abs(got_dyn[f] - want_dyn[f]).max()) for f in differ])
    assert got_dyn.tobytes() == want_dyn.tobytes(), f"dynamic bodies against the oracle: {differ}"
    assert_kinematic_equal(got_kin, motion.apply_host(drivers, advanced, t), "kinematic bodies against ivx_md_apply_host")
    assert_kinematic_equal(got_kin, want_kin, "kinematic bodies against the driven oracle")
    assert got_kin[7]["position"].tobytes() != kin[7]["position"].tobytes()  # (the undriven body moved by its own velocity)
    w.close()
    plain.close()


def contact_scene():
    """a 3 x 3 lattice of dynamic spheres (radius 0.5, 1.05 apart, under gravity) sunk 0.02 into a kinematic plane that oscillates along y, and a
    kinematic sphere on a horizontal circle (the circle's frame turned so that its normal is +y) that reaches 0.2 into the lattice's first row once per revolution"""
    response = (0.4, 0.7, 0.5)
    dyn = np.array([ol.uniform_sphere_body(0.5, 1.0, (1.05 * i, 0.48, 1.05 * j)) for i in range(3) for j in range(3)])
    dyn["total_force"][:, 1] = f32(-9.81) * dyn["mass"]
    kin = np.concatenate([phu.static_plane(), phu.static_plane()])
    period = 0.12
    drivers = np.array([motion.harmonic_oscillator(0, 0.0, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.05, 0.4),
                        motion.circular(1, -0.5 * period, (-0.70710678, 0.0, 0.0, 0.70710678), (-1.05, 0.5, 1.05), 0.25, period)], dtype=capi.MOTION_DRIVER_DTYPE)
    kin = mr.apply(drivers, kin, 0.0)  # (the bodies start where their drivers have them at time 0)
    local = np.array([collision.sphere((0, 0, 0), 0.5, k, 1000 + k, response=response) for k in range(9)] +
                     [collision.sphere((0, 0, 0), 0.5, 1, 2000, kind=capi.BV_STATIC, response=response, kinematic=True),
                      collision.plane((0, 1, 0), 0.0, 0, 1, response=response, kinematic=True)], dtype=capi.COLLIDABLE_DTYPE)
    return dyn, kin, drivers, local


def test_thirty_frames_with_contacts_from_two_driven_bodies(ctx):
    dyn, kin, drivers, local = contact_scene()
    w, md = world_with(ctx, kin, drivers, dyn)
    o = ol.OraclePhysics(dyn, kin, (8, 0.4, 3, 0.2))
    cw = collision.CollisionWorld(w)
    cw.set_collidables(local)
    t, dt = f32(0), 0.004
    with_plane = with_sphere = 0
    cw.synchronize()
    for frame in range(30):
        contacts, deferred = cw.collide(capi.BV_DYNAMIC_PAIRS)
        # the oracle's side of the frame: the restatement's contacts over the oracle's bodies
        o_dyn, o_kin = o.bodies()
        world, boxes = nr.transform(local, *nr.body_frames(local, o_dyn, o_kin))
        want, _ = nr.collide(world, nr.broad_phase_pairs(boxes, local["kind"], capi.BV_DYNAMIC_PAIRS))
        assert len(deferred) == 0 and len(contacts) == len(want), (frame, len(contacts), len(want))
        for f in ("id", "body_a", "body_b", "flags"):
            np.testing.assert_array_equal(contacts[f], want[f], err_msg=f"frame {frame}: {f}")
        for f in ("position", "normal", "depth") if len(want) else ():
            assert np.abs(contacts[f] - want[f]).max() <= 1e-5, (frame, f, float(np.abs(contacts[f] - want[f]).max()))
        kinematic_members = set(int(b) for b in np.concatenate([contacts["body_a"], contacts["body_b"]]) if b & capi.KINEMATIC_BIT)
        with_plane += (capi.KINEMATIC_BIT | 0) in kinematic_members
        with_sphere += (capi.KINEMATIC_BIT | 1) in kinematic_members
        w.prepare_constraints(contacts)
        w.step_enqueue(dt)
        cw.synchronize()  # (right behind the enqueued step: it sees the driven bodies of the new time)
        o.step(want, dt)
        t = f32(t + f32(dt))
        drive_oracle(o, drivers, t)
        got_dyn, got_kin = w.bodies()
        phu.assert_bodies_close(got_dyn, o.bodies()[0], what=f"frame {frame}: ")
        for f in ("position", "velocity"):
            assert got_kin[f].tobytes() == o.bodies()[1][f].tobytes(), (frame, f)
    assert with_plane >= 3 and with_sphere >= 3, (with_plane, with_sphere)  # (the plane throws the lattice off after four frames; the sphere is in it for five)
    moved = w.bodies()[0]["position"] - dyn["position"]
    assert np.abs(moved[:3, 0]).max() > 1e-3, "the driven sphere pushed the first row"
    w.close()


# ---- replace, remove, outlive ------------------------------------------------------------------------------------------------------------------------
def test_replace_remove_and_fewer_bodies(ctx):
    dyn, kin = dynamic_bodies(4, 90), kinematic_bodies(6, 91)
    first, second = seeded_drivers([0, 2, 4], 92), seeded_drivers([1, 2, 2, 5], 93, kinds=[3, 4, 1, 0])
    w, md = world_with(ctx, kin, first, dyn)
    o = ol.OraclePhysics(dyn, kin)
    t, dt = f32(0), 0.01
    for drivers in (first, second, second):
        md.set(drivers)  # (the second time between two steps; the third replaces a set by itself)
        w.step_enqueue(dt)
        o.step(NONE, dt)
        t = f32(t + f32(dt))
        advanced, _ = drive_oracle(o, drivers, t)
        assert_kinematic_equal(w.bodies()[1], motion.apply_host(drivers, advanced, t), "after a step")
    # a refused set leaves the one in force
    with pytest.raises(capi.IvxError) as e:
        md.set([motion.circular(6, 0.0, (0, 0, 0, 1), (0, 0, 0), 1.0, 1.0)])
    assert e.value.code == capi.IVX_ERR_INVALID and "driver 0" in str(e.value)
    with pytest.raises(capi.IvxError) as e:
        md.set([second[0], motion.orbital(0, 0.0, (0, 0, 0, 1), (0, 0, 0), 1.0, 1.0, 1.0)])
    assert e.value.code == capi.IVX_ERR_INVALID and "driver 1" in str(e.value)
    now = w.bodies()[1]
    md.apply(2.0)
    assert_kinematic_equal(w.bodies()[1], motion.apply_host(second, now, 2.0), "after refused sets")
    # removed: a step is the step of a world that never had a set
    md.clear()
    d0, k0 = w.bodies()
    plain = PhysicsWorld(ctx)
    plain.set_bodies(d0, k0)
    w.step_enqueue(dt)
    plain.step_enqueue(dt)
    got, want = w.bodies(), plain.bodies()
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert want[1].tobytes() != k0.tobytes()
    plain.close()
    # fewer kinematic bodies than the set refers to: the next apply says so, on its own and at the end of a step
    md.set(first)
    w.set_bodies(dyn, kin[:4])
    for call in (lambda: md.apply(1.0), lambda: w.step_enqueue(dt), lambda: w.step(dt)):
        with pytest.raises(capi.IvxError) as e:
            call()
        assert e.value.code == capi.IVX_ERR_STATE, str(e.value)
    md.set(first[:2])
    md.apply(1.0)
    assert_kinematic_equal(w.bodies()[1], motion.apply_host(first[:2], kin[:4], 1.0), "a set that fits again")
    w.close()
