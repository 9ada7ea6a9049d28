"""Device checks of detailed drag inside the force stage (impact_amd/csrc/forces.hip): `ivx_world_apply_forces` with a drag set against
`ivx_fg_apply_host_drag` over the same bodies around a wave and a workgroup, a map built from a grid's resident mesh straight into a slot against
`ivx_drag_load_map` of the same grid, twenty enqueued steps against the oracle world rewritten by the restatements in the reference's order, and
replacing, removing and outliving maps, medium and set."""
import numpy as np
import pytest

import drag_stage_ref as dr
import forces_ref as fr
import oracle_lib as ol
import physics_util as phu
from impact_amd import capi, drag, forces, scenes
from impact_amd.physics import PhysicsWorld
from impact_amd.voxel import SDFVoxelGenerator, VoxelObject, VoxelObjectMesh

pytestmark = pytest.mark.gpu

f32 = np.float32
NONE = np.zeros(0, dtype=capi.CONTACT_DTYPE)
WIND = forces.UniformMedium.moving_air((1.0, 2.0, -3.0))
# velocities relative to the medium of the hand-made bodies (identity orientation, mass 2): at rest, along +z and -z, in the xy-plane on cell edges,
# phi just below zero
EDGE_VELOCITIES = [(0.0, 0.0, 0.0), (0.0, 0.0, 2.0), (0.0, 0.0, -2.0), (0.0, 4.0, 0.0), (-1.0, 0.0, 0.0), (1.0, -1e-30, 0.0)]


def assert_dynamic_equal(got, want, what):
    if got.tobytes() != want.tobytes():
        bad = [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()]
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} dynamic bodies differ, first at {bad[0]}: force {got['total_force'][bad[0]]} != {want['total_force'][bad[0]]}, "
                             f"torque {got['total_torque'][bad[0]]} != {want['total_torque'][bad[0]]}")


def seeded_maps(seed, n_thetas=(1, 3, 64)):
    rng = np.random.default_rng(seed)
    return [dr.random_map(rng, n) for n in n_thetas]


def drag_scene(n_dyn, seed, medium):
    """bodies, of which every third carries no drag generator, body 1 two of them; from 20 bodies on the hand-made edge bodies among them"""
    rng = np.random.default_rng(seed)
    dyn = fr.random_dynamic(rng, n_dyn)
    _, vm = dr.medium_of(medium)
    if n_dyn >= 20:
        for k, v in enumerate(EDGE_VELOCITIES):
            b = 3 * k + 4  # (never a multiple of three less one)
            dyn["orientation"][b], dyn["mass"][b] = (0, 0, 0, 1), 2.0
            dyn["momentum"][b] = (np.array(v, dtype=f32) + vm) * f32(2.0)
    gens = [forces.detailed_drag(b, int(rng.integers(0, 3)), rng.uniform(0.1, 2.0), rng.uniform(0.5, 2.0)) for b in range(n_dyn) if b % 3 != 2]
    if n_dyn >= 2:
        gens.append(forces.detailed_drag(1, 2, 0.7, 1.2))
    order = rng.permutation(len(gens))
    return dyn, np.array(gens, dtype=capi.DRAG_GENERATOR_DTYPE)[order]


def other_generators(n_dyn, n_kin, seed):
    """one generator on every body but each seventh, the kinds in turn (a lone body takes the kinds that need no second dynamic body)"""
    rng = np.random.default_rng(seed)
    kinds = [k for k in range(6) if n_dyn > 1 or k != fr.SPRING_DD]
    gens = []
    for i in range(n_dyn):
        if i % 7 == 6 and n_dyn >= 7:
            continue
        kind = kinds[i % len(kinds)]
        body_b = (i + 1) % n_dyn if kind == fr.SPRING_DD else int(rng.integers(0, n_kin)) if kind == fr.SPRING_DK else 0
        gens.append(fr.generators(kind, i, body_b, fr.seeded_parameters(kind, 1, rng))[0])
    return np.array(gens, dtype=capi.FORCE_GENERATOR_DTYPE)


def world_with(ctx, dyn, kin, maps=(), medium=None, drag_gens=(), generators=(), field=(), g=1.0):
    w = PhysicsWorld(ctx)
    w.set_bodies(dyn, kin)
    fg = forces.ForceGenerators(w)
    for slot, m in enumerate(maps):
        if m is not None:
            fg.set_drag_map(slot, m)
    if medium is not None:
        fg.set_medium(medium)
    if len(generators):
        fg.set(generators)
    if len(field):
        fg.set_gravity(field, g)
    if len(drag_gens):
        fg.set_drag(drag_gens)
    return w, fg


# ---- 1. device against host --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("everything", [False, True], ids=["drag-alone", "every-kind-and-a-field"])
@pytest.mark.parametrize("n_dyn", [1, 63, 64, 65, 255, 256, 257])
def test_apply_equals_the_host_stage(ctx, n_dyn, everything):
    dyn, drag_gens = drag_scene(n_dyn, 700 + n_dyn, WIND)
    rng = np.random.default_rng(800 + n_dyn)
    kin = fr.random_kinematic(rng, 3)
    maps = seeded_maps(900 + n_dyn)
    gens = other_generators(n_dyn, len(kin), 1000 + n_dyn) if everything else np.zeros(0, dtype=capi.FORCE_GENERATOR_DTYPE)
    field = rng.permutation(n_dyn)[: min(n_dyn, 5)].astype(np.uint32) if everything else np.zeros(0, dtype=np.uint32)
    w, fg = world_with(ctx, dyn, kin, maps, WIND, drag_gens, gens, field, 0.5)
    fg.apply()
    got, got_kin = w.bodies()
    want, want_loads = forces.apply_host(gens, dyn, kin, field, 0.5, drag=drag_gens, maps=maps, medium=WIND)
    assert_dynamic_equal(got, want, f"{n_dyn} bodies")
    assert got_kin.tobytes() == kin.tobytes() and fg.gravity_loads().tobytes() == want_loads.tobytes()
    for f in fr.DYNAMIC_FIELDS:
        assert got[f].tobytes() == dyn[f].tobytes(), f  # (the stage writes the totals only)
    without, _ = forces.apply_host(gens, dyn, kin, field, 0.5)
    dragged = np.unique(drag_gens["body"])
    changed = np.array([got[b].tobytes() != without[b].tobytes() for b in range(n_dyn)])
    assert changed[dragged].sum() >= len(dragged) - 1 and not changed[np.setdiff1d(np.arange(n_dyn), dragged)].any()
    if n_dyn >= 20:
        assert not changed[4], "the body at rest in the medium"
        assert_dynamic_equal(got, dr.apply(gens, dyn, kin, field, 0.5, drag_gens, maps, WIND)[0], f"{n_dyn} bodies, the restatement")
    m = fg.medium()
    assert (m.mass_density, m.velocity) == (float(f32(1.2)), (1.0, 2.0, -3.0))
    w.close()


# ---- 2. a map built from a grid --------------------------------------------------------------------------------------------------------------------
def test_map_from_grid_is_the_downloaded_map_and_follows_a_bite(ctx):
    generator = SDFVoxelGenerator(1.0, scenes.sphere_scene(14.0))
    assert generator.chunk_counts() == (2, 2, 2)  # a 32^3 grid
    g = VoxelObject.generate(ctx, generator)
    mesh = VoxelObjectMesh.create(g)
    centre = np.array([0.5 * (a + b) for a, b in g.occupied_voxel_ranges], dtype=f32)
    com = centre + np.array([0.5, -0.25, 0.75], dtype=f32)
    cfg = drag.DragLoadMapConfig(200, 8, 2.0)
    rng = np.random.default_rng(1100)
    dyn = fr.random_dynamic(rng, 70)
    drag_gens = np.array([forces.detailed_drag(b, 5, rng.uniform(0.1, 2.0), rng.uniform(0.5, 2.0)) for b in range(70)], dtype=capi.DRAG_GENERATOR_DTYPE)
    w, fg = world_with(ctx, dyn, fr.random_kinematic(rng, 0))
    fg.set_medium(WIND)
    assert fg.drag_map(5) is None
    maps = []
    for bitten in (False, True):
        if bitten:
            r = g.absorb_sphere(centre + np.array([0.0, 0.0, 14.0], dtype=f32), 7.0, 6.0)
            mesh.sync_with_voxel_object(r["invalidated"])
        fg.set_drag_map_from_grid(5, g, com, cfg)
        if not bitten:
            fg.set_drag(drag_gens)
        fg.apply()
        resident = fg.drag_map(5)
        host = drag.DragLoadMap.compute_from_voxel_object_mesh(mesh, com, 200, 8, 2.0).loads
        assert resident.shape == (8, 16) and resident.tobytes() == host.tobytes()
        assert np.abs(resident["force"]).max() > 0
        want, _ = forces.apply_host([], dyn, drag=drag_gens, maps=[None] * 5 + [resident], medium=WIND)
        assert_dynamic_equal(w.bodies()[0], want, "bitten" if bitten else "whole")
        maps.append(resident)
    assert maps[0].tobytes() != maps[1].tobytes(), "the bite did not change the map"
    stale, _ = forces.apply_host([], dyn, drag=drag_gens, maps=[None] * 5 + [maps[0]], medium=WIND)
    assert stale.tobytes() != w.bodies()[0].tobytes(), "the stage did not follow the new map"
    w.close()
    g.close()


# ---- 3. twenty enqueued steps, one wait ------------------------------------------------------------------------------------------------------------
def test_twenty_enqueued_steps_with_drag_in_the_order_of_the_reference(ctx):
    """five bodies fall under a constant acceleration through still air, each with a drag generator (body 3 with two); a damped spring between bodies 0
    and 1; bodies 2, 3, 4 a gravity field. The oracle's bodies are rewritten after every step by the restatement with the phases in the reference's
    order."""
    rng = np.random.default_rng(1200)
    dyn = fr.random_dynamic(rng, 5, spread=2.0)
    dyn["position"][2:5] = fr.spread_positions(rng, 3, 2.0, 1.0)
    kin = fr.random_kinematic(rng, 1, spread=2.0)
    gens = np.array([forces.constant_acceleration(b, (0.0, -9.81, 0.0)) for b in range(5)] +
                    [forces.spring_dynamic_dynamic(0, (0.1, 0, 0), 1, (0, 0.2, 0), forces.standard_spring(40.0, 1.5, 1.0))], dtype=capi.FORCE_GENERATOR_DTYPE)
    maps = seeded_maps(1201, (8, 3))
    drag_gens = np.array([forces.detailed_drag(b, b % 2, 0.4 + 0.1 * b, 0.3) for b in range(5)] + [forces.detailed_drag(3, 0, 0.9, 0.25)], dtype=capi.DRAG_GENERATOR_DTYPE)
    field, g, air = np.array([4, 2, 3], dtype=np.uint32), 2.0, forces.UniformMedium.still_air()
    w, fg = world_with(ctx, dyn, kin, maps, air, drag_gens, gens, field, g)
    fg.apply()
    primed, _ = dr.apply(gens, dyn, kin, field, g, drag_gens, maps, air)
    o = ol.OraclePhysics(primed, kin)
    dt = 0.004
    mattered = 0
    for _ in range(20):
        w.step_enqueue(dt)
        o.step(NONE, dt)
        o_dyn, o_kin = o.bodies()
        forced, _ = dr.apply(gens, o_dyn, o_kin, field, g, drag_gens, maps, air)
        mattered += fr.apply(gens, o_dyn, o_kin, field, g)[0].tobytes() != forced.tobytes()
        ol.lib().orc_physics_set_bodies(o.h, ol._p(forced), len(forced), ol._p(o_kin), len(o_kin))
    got_dyn, _ = w.bodies()  # (the one wait)
    want_dyn, _ = o.bodies()
    assert mattered == 20, "without the drag phase the totals would differ in every step"
    differ = [f for f in phu.STATE_FIELDS + ("total_force", "total_torque") if got_dyn[f].tobytes() != want_dyn[f].tobytes()]
    print("dynamic fields that are not byte-equal to the oracle:", differ, [float(np.abs(got_dyn[f] - want_dyn[f]).max()) for f in differ])
    phu.assert_bodies_close(got_dyn, want_dyn)
    w.close()


# ---- 4. lifetime -------------------------------------------------------------------------------------------------------------------------------------
def test_replace_remove_refuse_and_outlive(ctx):
    rng = np.random.default_rng(1300)
    dyn, kin = fr.random_dynamic(rng, 6), fr.random_kinematic(rng, 1)
    maps = seeded_maps(1301, (3, 8, 1))
    first = np.array([forces.detailed_drag(b, b % 3, 0.5, 1.0) for b in range(6)], dtype=capi.DRAG_GENERATOR_DTYPE)
    second = np.array([forces.detailed_drag(5, 0, 1.5, 0.5), forces.detailed_drag(2, 1, 0.25, 2.0), forces.detailed_drag(5, 1, 0.1, 1.0)], dtype=capi.DRAG_GENERATOR_DTYPE)
    air, water = forces.UniformMedium.still_air(), forces.UniformMedium.moving_water((0.5, 0.0, -0.25))
    w, fg = world_with(ctx, dyn, kin, maps, air, first)
    dt = 0.01
    bigger = dr.random_map(rng, 16)  # (a map that does not fit the slot's allocation: the slot grows)
    state = {"maps": list(maps), "medium": air, "set": first}

    def step_and_check(what):
        w.step_enqueue(dt)
        now, now_kin = w.bodies()
        want, _ = forces.apply_host([], now, now_kin, drag=state["set"], maps=state["maps"], medium=state["medium"])
        assert_dynamic_equal(now, want, what)  # (the totals belong to the configuration the step ended in)

    step_and_check("first set")
    state["maps"][1] = dr.random_map(rng, 8)  # the same shape: replaced in place, behind the step that read the old one
    fg.set_drag_map(1, state["maps"][1])
    step_and_check("a map replaced in place")
    state["maps"][0] = bigger
    fg.set_drag_map(0, bigger)
    step_and_check("a map replaced by a larger one")
    state["medium"] = water
    fg.set_medium(water)
    step_and_check("the medium replaced")
    state["set"] = second
    fg.set_drag(second)
    step_and_check("the set replaced")
    # refused calls leave what is in force
    for bad, says in (([second[0], forces.detailed_drag(6, 0, 1.0)], "dynamic body 6"), ([second[0], forces.detailed_drag(0, 3, 1.0)], "map slot 3"),
                      ([second[0], forces.detailed_drag(0, 70000, 1.0)], "map slot 70000")):
        with pytest.raises(capi.IvxError) as e:
            fg.set_drag(bad)
        assert e.value.code == capi.IVX_ERR_INVALID and "generator 1" in str(e.value) and says in str(e.value), str(e.value)
    with pytest.raises(capi.IvxError) as e:
        fg.set_drag_map(1, None)  # (named by the installed set)
    assert e.value.code == capi.IVX_ERR_STATE, str(e.value)
    with pytest.raises(capi.IvxError) as e:
        fg.set_drag_map(65536, maps[2])
    assert e.value.code == capi.IVX_ERR_CAPACITY, str(e.value)
    fg.set_drag_map(2, None)  # (no generator of the second set names slot 2)
    assert fg.drag_map(2) is None and fg.drag_map(1).tobytes() == state["maps"][1].tobytes()
    with pytest.raises(capi.IvxError) as e:
        fg.set_drag([forces.detailed_drag(0, 2, 1.0)])
    assert e.value.code == capi.IVX_ERR_INVALID and "holds no drag load map" in str(e.value)
    fg.n_drag = len(second)
    state["maps"][2] = None
    step_and_check("after refused calls")
    # a grid of another context, and a grid without a current mesh
    from impact_amd.voxel import Context

    other = Context(0)
    try:
        foreign = VoxelObject.generate(other, SDFVoxelGenerator(1.0, scenes.sphere_scene(6.0)))
        VoxelObjectMesh.create(foreign)
        with pytest.raises(capi.IvxError) as e:
            fg.set_drag_map_from_grid(4, foreign, (8.0, 8.0, 8.0), drag.DragLoadMapConfig(64, 4, 2.0))
        assert e.value.code == capi.IVX_ERR_INVALID and "context" in str(e.value)
        foreign.close()
    finally:
        other.close()
    bare = VoxelObject.generate(ctx, SDFVoxelGenerator(1.0, scenes.sphere_scene(6.0)))
    with pytest.raises(capi.IvxError) as e:
        fg.set_drag_map_from_grid(4, bare, (8.0, 8.0, 8.0), drag.DragLoadMapConfig(64, 4, 2.0))
    assert e.value.code == capi.IVX_ERR_STATE and fg.drag_map(4) is None
    bare.close()
    # fewer bodies than the set refers to: IVX_ERR_STATE before anything is launched; then the set over another number of bodies
    w.set_bodies(dyn[:5], kin)
    before = w.bodies()
    for call in (fg.apply, lambda: w.step_enqueue(dt), lambda: w.step(dt)):
        with pytest.raises(capi.IvxError) as e:
            call()
        assert e.value.code == capi.IVX_ERR_STATE, str(e.value)
    assert w.bodies()[0].tobytes() == before[0].tobytes(), "a refused step launched something"
    more = fr.random_dynamic(rng, 9)
    w.set_bodies(more, kin)
    fg.apply()
    assert_dynamic_equal(w.bodies()[0], forces.apply_host([], more, kin, drag=second, maps=state["maps"], medium=water)[0], "the same set over more bodies")
    # removed: a step is the step of a world that never had a set, and host-set totals persist again; the maps and the medium are still the world's
    fg.clear_drag()
    fg.apply()  # (nothing)
    d0, k0 = w.bodies()
    d0["total_force"], d0["total_torque"] = rng.normal(size=(9, 3)), rng.normal(size=(9, 3))
    w.set_bodies(d0, k0)
    plain = PhysicsWorld(ctx)
    plain.set_bodies(d0, k0)
    for _ in range(2):
        w.step_enqueue(dt)
        plain.step_enqueue(dt)
    got, want = w.bodies(), plain.bodies()
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert got[0]["total_force"].tobytes() == d0["total_force"].tobytes() and got[0]["momentum"].tobytes() != d0["momentum"].tobytes()
    plain.close()
    assert fg.drag_map(0).tobytes() == bigger.tobytes() and fg.medium().mass_density == 1e3
    fg.set_drag(second)  # ... and a drag set alone brings the stage back
    fg.apply()
    now, now_kin = w.bodies()
    assert_dynamic_equal(now, forces.apply_host([], now, now_kin, drag=second, maps=state["maps"], medium=water)[0], "the set installed again")
    w.close()
