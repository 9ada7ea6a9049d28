"""The staged upload and the state slot of the device subsystems (impact_amd/csrc/device_common.hpp: ivx_staging_for / ivx_staging_upload /
ivx_staging_sent, ivx_state_for / ivx_state_take), where the tests of the subsystems themselves do not reach: the pinned block growing while an
upload from it is still pending, a context's states made, released with the context and made again on the next, and world-owned state leaving
and coming back. Every expectation is the library's host form or the float32 restatement the neighbouring tests use — no tolerance anywhere in
this file.

(A query of kind 4 given to the two host-only calls, ivx_bv_query_skips_boxes and ivx_bv_queries_hierarchy_host, is refused in
test_bvh_queries_cpu.py::test_refusals_and_empty_inputs.)"""
import numpy as np
import pytest

import bvol_ref as br
import cull_ref as cr
import forces_ref as fr
import instances_ref as ir
from impact_amd import bvol, capi, cull, forces, instances, motion
from impact_amd.physics import PhysicsWorld
from impact_amd.voxel import Context
from test_gpu_cull import assert_result_matches
from test_gpu_forces import assert_dynamic_equal, one_of
from test_gpu_motion import assert_kinematic_equal, kinematic_bodies, seeded_drivers
from test_instances_cpu import assert_outputs_equal

pytestmark = pytest.mark.gpu

STAGING_FLOOR = 1 << 16  # the smallest pinned block ivx_staging_for makes


def test_the_block_grows_behind_a_pending_set_of_boxes():
    """65 model boxes with similarities and kinds (an upload of a few KiB: the block is at its floor), then with no wait in between 513 queries,
    whose records are the first upload past the floor: the block is replaced while the set's upload may still be leaving it. The world boxes equal
    ivx_bv_world_aabb per object, masks and counts the restatement over them."""
    n, n_queries = 65, 513
    assert (n_queries - 1) * capi.BV_QUERY_DTYPE.itemsize <= STAGING_FLOOR < n_queries * capi.BV_QUERY_DTYPE.itemsize and n_queries <= capi.BV_MAX_QUERIES
    assert n * (capi.AABB_DTYPE.itemsize + capi.SIMILARITY_DTYPE.itemsize) + 128 * 4 + 3 * 256 <= STAGING_FLOOR
    model, kinds = br.scene(n)
    rng = np.random.default_rng(77)
    sims = bvol.similarities(n)  # (near the identity, so that the scene's queries still hit and miss)
    q = np.concatenate([0.05 * rng.normal(size=(n, 3)), np.ones((n, 1))], axis=1)
    sims["rotation"], sims["scaling"], sims["translation"] = q / np.linalg.norm(q, axis=1, keepdims=True), rng.uniform(0.9, 1.1, n), rng.uniform(-0.5, 0.5, (n, 3))
    records = br.mixed_queries(n, n_queries)
    c = Context(0)
    try:
        s = bvol.set_boxes(c, model, sims, kinds)
        masks, counts = s.query(records)
        world, _ = s.download()
    finally:
        c.close()
    assert world.tobytes() == br.host_world_boxes(model, sims).tobytes()
    want_masks, want_counts = br.queries(world, records)
    assert 0 < int(want_counts.sum()) < n * n_queries and (want_counts > 0).sum() > n_queries // 2
    assert masks.tobytes() == want_masks.tobytes() and counts.tolist() == want_counts.tolist()


def test_the_block_grows_behind_a_pending_set_of_instances():
    """Neither 65 instances (48 bytes each) nor FI_MAX_VIEWS views (72 bytes each) reach the floor of 64 KiB, so the largest legal shape instead:
    one instance, then with no wait in between 4 096 (192 KiB) — the block grows behind the first upload — and FI_MAX_VIEWS views over them. Every
    output equals the host form over the downloaded boxes and masks."""
    n, n_views, n_queries = 4096, capi.FI_MAX_VIEWS, 9
    assert max(65 * capi.FI_INSTANCE_DTYPE.itemsize, n_views * capi.FI_VIEW_DTYPE.itemsize) < STAGING_FLOOR < n * capi.FI_INSTANCE_DTYPE.itemsize
    world0, inst = ir.scene(n)
    views = ir.seeded_views(n, n_views, n_queries, 0, seed=1)
    c = Context(0)
    try:
        s = bvol.set_boxes(c, world0)
        masks, _ = s.query(br.mixed_queries(n, n_queries))
        world, _ = s.download()
        fi = instances.FrameInstances(c)
        fi.set_instances(inst[:1])
        fi.set_instances(inst)
        results = fi.views(views)
        got = fi.download()
        got.results = results
    finally:
        c.close()
    host = instances.views_host(world, inst, masks, views)
    assert 0 < int(host.offsets[-1]) < n * n_views
    assert_outputs_equal(got, (host.pairs, host.offsets, host.objects, host.transforms, host.kept, host.results), "4 096 instances behind 1")


def first_uses(c):
    """one smallest valid call of chunk culling (before any set: its count buffer is made by this enqueue), bounding volumes, the hierarchy and
    frame instances on a context that has had none -> the bytes they left, each checked against its reference"""
    rng = np.random.default_rng(9)
    tables, view = [cr.random_table(rng, 3)], np.array([cr.perspective_view()])
    res = cull.cull_submesh_tables(c, tables, np.ones(1, dtype=np.float32), view, cull.pairs(1, 1))
    out = [assert_result_matches(res, tables, view["flags"], what="first cull")[0]]
    world0, inst = bvol.boxes([(0, 0, 0), (0.5, 0.5, 0.5)], [(1, 1, 1), (2, 2, 2)]), ir.scene(2)[1]
    s = bvol.set_boxes(c, world0)
    world, _ = s.download()
    assert world.tobytes() == world0.tobytes()
    pairs = s.pairs()
    assert pairs.tolist() == [[0, 1]] == br.pairs(world)[0].tolist()
    s.build_hierarchy()
    nodes, leaves = s.hierarchy()
    want_nodes, want_leaves, _ = bvol.hierarchy_host(world)
    assert nodes.tobytes() == want_nodes.tobytes() and leaves.tobytes() == want_leaves.tobytes()
    tree_pairs = s.pairs_hierarchy()
    assert tree_pairs.tobytes() == pairs.tobytes()
    queries = bvol.query_array([bvol.box_query((-1, -1, -1), (0.25, 0.25, 0.25)), bvol.sphere_query((1.9, 1.9, 1.9), 0.2)])
    masks, counts = s.query(queries)
    want_masks, want_counts = br.queries(world, queries)
    assert masks.tobytes() == want_masks.tobytes() and counts.tolist() == want_counts.tolist() == [1, 1]
    fi = instances.FrameInstances(c)
    fi.set_instances(inst)
    views = ir.seeded_views(2, 1, 2, 0, seed=1)
    results = fi.views(views)
    got = fi.download()
    got.results = results
    host = instances.views_host(world, inst, masks, views)
    assert_outputs_equal(got, (host.pairs, host.offsets, host.objects, host.transforms, host.kept, host.results), "first views")
    return out + [a.tobytes() for a in (world, pairs, nodes, leaves, masks, counts)] + [got.tobytes()]


def test_first_use_release_and_first_use_again():
    """the states of a context are made by their first calls and leave with the context; a second fresh context makes them again and its calls
    leave the same bytes"""
    runs = []
    for _ in range(2):
        c = Context(0)
        try:
            runs.append(first_uses(c))
        finally:
            c.close()
    assert runs[0] == runs[1]


def test_motion_drivers_leave_and_return(ctx):
    """one driven body: set, set none (the world's state leaves), set again, apply -> ivx_md_apply_host"""
    kin = kinematic_bodies(2, 61)
    drivers = seeded_drivers([1], 62)
    w = PhysicsWorld(ctx)
    w.set_bodies(np.zeros(0, dtype=capi.RIGID_BODY_DTYPE), kin)
    md = motion.MotionDrivers(w)
    md.set(drivers)
    md.clear()
    md.set(drivers)
    md.apply(1.5)
    assert_kinematic_equal(w.bodies()[1], motion.apply_host(drivers, kin, 1.5), "set, none, set, apply")
    w.close()


def test_a_force_generator_leaves_and_returns(ctx):
    """one generator: set, set none (the world's state leaves), set again, apply -> ivx_fg_apply_host"""
    rng = np.random.default_rng(63)
    dyn, kin = fr.random_dynamic(rng, 2), fr.random_kinematic(rng, 1)
    gens = np.array([one_of(fr.SPRING_DK, 1, 2, 1, rng)], dtype=capi.FORCE_GENERATOR_DTYPE)
    w = PhysicsWorld(ctx)
    w.set_bodies(dyn, kin)
    fg = forces.ForceGenerators(w)
    fg.set(gens)
    fg.clear()
    fg.set(gens)
    fg.apply()
    want, _ = forces.apply_host(gens, dyn, kin)
    assert want["total_force"].tobytes() != dyn["total_force"].tobytes()
    assert_dynamic_equal(w.bodies()[0], want, "set, none, set, apply")
    w.close()
