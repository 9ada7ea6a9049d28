"""The hierarchy over a bounding-volume set on the device (impact_amd/csrc/bvh.hip). The tree: byte-equal to the library's host function over the
DOWNLOADED world boxes (which test_bvh_cpu.py holds against the restatement). The pairs: byte-equal to bvol_ref's exact upper triangle, or, where
that is too slow to restate, to the flat `ivx_bv_pairs` of the same set. The collision world: contacts and deferred pairs byte-equal between the
two broad-phase settings. No expectation comes from the tree itself, and there is no tolerance anywhere in this file.

The sort owns 1 024 words per wave and scans in rounds of 1 024 entries, the walk and the refit run a lane per leaf in workgroups of 256: the sizes
below sit one below, at and one above a wave, a workgroup and a sort tile; 65 536 leaves are 256 workgroups on every XCD, where a stale read in
the refit's hand-off can show."""
import ctypes as C

import numpy as np
import pytest

import bvh_ref as hr
import bvol_ref as br
import narrow_ref as nr
import parity_util as pu
import physics_util as phu
from impact_amd import bvol, capi, collision, scenes
from impact_amd.physics import PhysicsWorld
from impact_amd.voxel import Context

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4161]
MODES = [capi.BV_ALL_PAIRS, capi.BV_DYNAMIC_PAIRS]


def assert_pairs_equal(got, want, what=""):
    assert got.dtype == np.uint32 and got.shape == want.shape, (what, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got != want).any(axis=1))[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} pairs differ, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}")


def built(ctx, world, kinds=None):
    s = bvol.set_boxes(ctx, world, None, kinds)
    s.build_hierarchy()
    return s


def tree_cases():
    for n in SIZES:
        yield f"scene {n}", lambda n=n: br.scene(n)[0]
    yield "identical 130", lambda: hr.identical_boxes(130)
    yield "scene 65536", lambda: br.scene(65536)[0]


@pytest.mark.parametrize("name,make", list(tree_cases()), ids=[n for n, _ in tree_cases()])
def test_device_tree_equals_the_host_function(ctx, name, make):
    world = make()
    n = len(world)
    s = built(ctx, world)
    got_world, _ = s.download()
    assert got_world.tobytes() == world.tobytes()
    want_nodes, want_leaves, _ = bvol.hierarchy_host(got_world)
    nodes, leaves = s.hierarchy()
    assert leaves.tobytes() == want_leaves.tobytes(), f"{name}: leaf objects"
    if nodes.tobytes() != want_nodes.tobytes():
        bad = np.nonzero(nodes != want_nodes)[0]
        raise AssertionError(f"{name}: {len(bad)} of {len(nodes)} nodes differ, first at {bad[0]}: {nodes[bad[0]]} != {want_nodes[bad[0]]}")
    assert bool(s.device_ptr(capi.BV_PTR_NODES)) == bool(s.device_ptr(capi.BV_PTR_LEAF_OBJECTS)) == (n >= 2)
    # a second build leaves the same bytes
    s.build_hierarchy()
    again_nodes, again_leaves = s.hierarchy()
    assert again_nodes.tobytes() == nodes.tobytes() and again_leaves.tobytes() == leaves.tobytes()
    if n >= 2:
        depth, count = bvol.node_info(nodes, n)
        assert int(count[0]) == n and int(depth.max()) + 1 <= 50


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", SIZES)
def test_pairs_of_the_seeded_scene(ctx, n, mode):
    world, kinds = br.scene(n)
    s = built(ctx, world, kinds)
    want, touching = br.scene_pairs(n, mode)
    if n >= 63:  # the case can show something
        all_pairs, all_touching = br.scene_pairs(n, capi.BV_ALL_PAIRS)
        assert n <= len(all_pairs) <= n * (n - 1) // 8 and all_touching.sum() * 10 >= len(all_pairs)
        assert len(want) > 0 and (mode == capi.BV_ALL_PAIRS or len(want) < len(all_pairs))
    if n == 4161 and mode == capi.BV_ALL_PAIRS:
        assert (len(want), int(touching.sum())) == (13511, 4171)
    assert_pairs_equal(s.pairs_hierarchy(mode, capacity=len(want)), want, f"n {n} mode {mode}")


@pytest.mark.parametrize("mode", MODES)
def test_pairs_of_65536_equal_the_flat_form(ctx, mode):
    world, kinds = br.scene(65536)
    s = built(ctx, world, kinds)
    flat = s.pairs(mode)
    assert len(flat) > 65536 and (mode != capi.BV_ALL_PAIRS or len(flat) == 228064)
    tree = s.pairs_hierarchy(mode, capacity=len(flat))
    assert_pairs_equal(tree, flat, f"65536, mode {mode}")
    assert np.all(tree[:, 0] < tree[:, 1])


def hand_cases():
    for name, (world, kinds) in hr.hand_made_cases().items():
        yield name, world, kinds
    rng = np.random.default_rng(2)
    c = rng.uniform(0, 0.25, (200, 3))
    yield "all 19900 pairs of 200", bvol.boxes(c - 1.0, c + 1.0), None
    world = bvol.boxes([(0, 0, 0)] * 3, [(1, 1, 1)] * 3)
    world["upper"][1][2] = np.nan
    yield "nan of three", world, None
    for n in (4, 6):
        bodies, _ = scenes.sphere_pile_scene(n=n)
        pos, r = bodies["position"].astype(np.float32), np.float32(0.5)
        yield f"pile {n} in lattice order", bvol.boxes(pos - r, pos + r), None
        pos = pos[np.random.default_rng(n).permutation(len(pos))]
        yield f"pile {n} permuted", bvol.boxes(pos - r, pos + r), None


@pytest.mark.parametrize("name,world,kinds", list(hand_cases()), ids=[c[0] for c in hand_cases()])
def test_pairs_hand_made_cases(ctx, name, world, kinds):
    s = built(ctx, world, kinds)
    got_world, _ = s.download()
    for mode in (MODES if kinds is not None else MODES[:1]):
        with np.errstate(over="ignore", invalid="ignore"):
            want = br.pairs(got_world, kinds, mode)[0]
        if name.startswith("all 19900"):
            assert len(want) == 19900
        if name.startswith("pile"):
            n = int(name.split()[1])
            assert len(want) == ((3 * n - 2) ** 3 - n ** 3) // 2
        assert_pairs_equal(s.pairs_hierarchy(mode), want, f"{name}, mode {mode}")


def test_capacity_state_and_repetition(ctx):
    lib = capi.lib()
    world, kinds = br.scene(1025)
    want = br.scene_pairs(1025, capi.BV_ALL_PAIRS)[0]
    s = built(ctx, world, kinds)
    # one short: IVX_ERR_CAPACITY, the number found, the buffer untouched
    out = np.full((len(want), 2), 0xA5A5A5A5, dtype=np.uint32)
    found = C.c_size_t(0)
    assert lib.ivx_bv_pairs_hierarchy(ctx.h, 0, capi.ptr(out), len(want) - 1, C.byref(found)) == capi.IVX_ERR_CAPACITY
    assert found.value == len(want) and np.all(out == 0xA5A5A5A5)
    # pairs == NULL with cap == 0 leaves them on the device only
    capi.check(lib.ivx_bv_pairs_hierarchy(ctx.h, 0, None, 0, C.byref(found)))
    assert found.value == len(want) and s.device_ptr(capi.BV_PTR_PAIRS)
    # two calls leave the same bytes, and the flat form's
    first, second = s.pairs_hierarchy(0, capacity=len(want)), s.pairs_hierarchy(0, capacity=len(want) + 10)
    assert_pairs_equal(first, want, "first")
    assert first.tobytes() == second.tobytes() == s.pairs(0).tobytes()
    assert_pairs_equal(s.pairs_hierarchy(0), want, "after a flat call")  # (the flat call left the tree alone)
    # refused arguments
    assert lib.ivx_bv_pairs_hierarchy(ctx.h, 2, capi.ptr(out), 4, C.byref(found)) == capi.IVX_ERR_INVALID
    assert lib.ivx_bv_pairs_hierarchy(ctx.h, 0, None, 4, C.byref(found)) == capi.IVX_ERR_INVALID
    assert lib.ivx_bv_pairs_hierarchy(ctx.h, 0, capi.ptr(out), 4, None) == capi.IVX_ERR_INVALID
    nodes, leaves, n_nodes = np.zeros(1024, dtype=capi.BV_NODE_DTYPE), np.zeros(1025, dtype=np.uint32), C.c_size_t(0)
    assert lib.ivx_bv_hierarchy_download(ctx.h, capi.ptr(nodes), 1023, capi.ptr(leaves), 1025, C.byref(n_nodes)) == capi.IVX_ERR_CAPACITY and n_nodes.value == 1024
    assert lib.ivx_bv_hierarchy_download(ctx.h, capi.ptr(nodes), 1024, capi.ptr(leaves), 1024, C.byref(n_nodes)) == capi.IVX_ERR_CAPACITY
    assert not nodes.tobytes().strip(b"\0") and not leaves.any()
    # a smaller set after a larger one: IVX_ERR_STATE for pairs and download until the tree is rebuilt, then nothing stale
    small_world, small_kinds = br.scene(65)
    s = bvol.set_boxes(ctx, small_world, None, small_kinds)
    assert lib.ivx_bv_pairs_hierarchy(ctx.h, 0, capi.ptr(out), len(out), C.byref(found)) == capi.IVX_ERR_STATE and found.value == 0
    assert lib.ivx_bv_hierarchy_download(ctx.h, capi.ptr(nodes), 1024, capi.ptr(leaves), 1025, C.byref(n_nodes)) == capi.IVX_ERR_STATE
    assert not s.device_ptr(capi.BV_PTR_NODES)
    s.build_hierarchy()
    for mode in MODES:
        assert_pairs_equal(s.pairs_hierarchy(mode), br.scene_pairs(65, mode)[0], f"smaller set, mode {mode}")
    want_nodes, want_leaves, _ = bvol.hierarchy_host(small_world)
    got_nodes, got_leaves = s.hierarchy()
    assert got_nodes.tobytes() == want_nodes.tobytes() and got_leaves.tobytes() == want_leaves.tobytes()
    # no set at all, an empty set, one box
    fresh = Context(0)
    try:
        assert lib.ivx_bv_build_hierarchy(fresh.h) == capi.IVX_ERR_STATE
        assert lib.ivx_bv_pairs_hierarchy(fresh.h, 0, capi.ptr(out), 4, C.byref(found)) == capi.IVX_ERR_STATE
        assert lib.ivx_bv_hierarchy_download(fresh.h, None, 0, None, 0, C.byref(n_nodes)) == capi.IVX_ERR_STATE
        for n in (0, 1):
            s = built(fresh, br.scene(n)[0])
            nodes0, leaves0 = s.hierarchy()
            assert nodes0.size == 0 and leaves0.tolist() == list(range(n)) and s.pairs_hierarchy().shape == (0, 2)
    finally:
        fresh.close()


def box_object(ctx):
    g = pu.gpu_from_graph(ctx, scenes.box_scene((30.0, 30.0, 30.0)), 1.0)
    g.compute_all_derived_state()
    g.update_occupied_voxel_ranges()
    return g


def test_inside_a_bracket_behind_a_recorded_edit(ctx):
    """three config-1 voxel objects through set_grids inside an ivx_many_begin bracket, behind a recorded edit of a fourth: build and pairs issue
    the recorded launches ahead of their own, and find the one overlapping pair"""
    lib = capi.lib()
    gs = [box_object(ctx) for _ in range(3)]
    sims = bvol.similarities(3)
    sims["translation"] = np.array([(0, 0, 0), (28, 0, 0), (100, 0, 0)], dtype=np.float32)
    extra = box_object(ctx)
    extra.set_densities(np.ones(256, dtype=np.float32))
    extra.absorb_sphere(np.array([16.0, 16.0, 30.0], dtype=np.float32), 4.0, 2.0)  # (an object's first edit allocates, with waits on the stream)

    def stats():
        out = np.zeros(3, dtype=np.uint64)
        capi.check(lib.ivx_many_stats(ctx.h, capi.ptr(out)))
        return [int(x) for x in out]

    s = bvol.set_grids(gs, sims)
    capi.check(lib.ivx_many_begin(ctx.h))
    rec0, iss0, _ = stats()
    extra.absorb_sphere_enqueue(np.array([16.0, 17.0, 30.0], dtype=np.float32), 5.0, 3.0)
    assert stats()[0] > rec0, "the edit inside the bracket was not recorded"
    s.build_hierarchy()
    assert stats()[1] > iss0, "the build did not issue the recorded launches ahead of its own"
    inside = s.pairs_hierarchy()
    capi.check(lib.ivx_many_flush(ctx.h))
    assert extra.absorb_collect()["emptied_voxels"] > 0
    world, _ = s.download()
    assert inside.tolist() == [[0, 1]] == br.pairs(world)[0].tolist()
    for g in gs + [extra]:
        g.close()


@pytest.mark.parametrize("n", [60, 70, 500, 520])
def test_collision_world_under_both_broad_phases(ctx, n):
    """narrow_ref.scene(n): spheres, capsules, voxel-object boxes, three planes at the end. 60 / 70 and 500 / 520 collidables lie on both sides of a
    wave and of the flat walk's segment of 512"""
    lib = capi.lib()
    local, dyn, kin = nr.scene(n)
    assert (local["shape"][-3:] == capi.CW_PLANE).all() and (local["shape"] == capi.CW_VOXEL_OBJECT).any()
    w = PhysicsWorld(ctx)
    w.set_bodies(dyn, kin)
    cw = collision.CollisionWorld(w)
    cw.set_collidables(local)
    s = cw.synchronize()
    results = {}
    for mode in MODES:
        results["default", mode] = cw.collide(mode)
    assert not s.device_ptr(capi.BV_PTR_NODES), "the default setting built a hierarchy"
    # a bad value is refused and leaves the setting as it was
    assert lib.ivx_cw_set_broad_phase(w.h, 2) == capi.IVX_ERR_INVALID
    for mode in MODES:
        assert cw.collide(mode)[0].tobytes() == results["default", mode][0].tobytes()
    assert not s.device_ptr(capi.BV_PTR_NODES)
    cw.set_broad_phase(capi.CW_BROAD_HIERARCHY)
    for mode in MODES:
        results["tree", mode] = cw.collide(mode)
    assert s.device_ptr(capi.BV_PTR_NODES) and s.device_ptr(capi.BV_PTR_LEAF_OBJECTS)
    # switching back restores the flat form: a new set, and no tree over it
    cw.set_broad_phase(capi.CW_BROAD_FLAT)
    s = cw.synchronize()
    for mode in MODES:
        results["flat", mode] = cw.collide(mode)
    assert not s.device_ptr(capi.BV_PTR_NODES)
    for mode in MODES:
        contacts, deferred = results["default", mode]
        assert len(contacts) > n // 4 and len(deferred) > 0
        for name in ("tree", "flat"):
            assert results[name, mode][0].tobytes() == contacts.tobytes(), f"contacts, {name}, mode {mode}"
            assert results[name, mode][1].tobytes() == deferred.tobytes() and results[name, mode][1].shape == deferred.shape, f"deferred pairs, {name}, mode {mode}"
    w.close()


def test_frames_with_the_hierarchy_on(ctx):
    """the lattice of test_gpu_narrow's five-frame test, three frames of synchronize -> collide -> ivx_world_set_contacts -> step with the hierarchy
    on: every frame's contacts equal the flat setting's on the same bodies, and the bodies move"""
    bodies, _ = scenes.sphere_pile_scene(4)
    response = (0.4, 0.7, 0.5)
    local = np.array([collision.sphere((0, 0, 0), 0.5, k, 1000 + k, response=response) for k in range(len(bodies))] +
                     [collision.plane((0, 1, 0), -0.475, 0, 1, response=response, kinematic=True)], dtype=capi.COLLIDABLE_DTYPE)
    w = PhysicsWorld(ctx)
    w.set_bodies(bodies, phu.static_plane())
    cw = collision.CollisionWorld(w)
    cw.set_collidables(local)
    start = w.bodies()[0]["position"].copy()
    for frame in range(3):
        s = cw.synchronize()
        cw.set_broad_phase(capi.CW_BROAD_FLAT)
        flat = cw.collide(capi.BV_DYNAMIC_PAIRS)
        cw.set_broad_phase(capi.CW_BROAD_HIERARCHY)
        contacts, deferred = cw.collide(capi.BV_DYNAMIC_PAIRS)
        assert len(contacts) >= 144 + 16 and len(deferred) == 0, (frame, len(contacts))
        assert contacts.tobytes() == flat[0].tobytes(), frame
        assert s.device_ptr(capi.BV_PTR_NODES)
        w.perform_physics_step(contacts, 0.005)
    assert np.abs(w.bodies()[0]["position"] - start).max() > 0
    w.close()
