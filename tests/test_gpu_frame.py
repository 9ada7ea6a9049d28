"""Whole collision frames with voxel bodies among the collidables, on the device against the oracle: synchronize -> pairs -> primitive contacts and
deferred voxel pairs (impact_amd/csrc/narrow.hip, bvol.hip) -> the two `_many` voxel generators (many.cpp, contacts.hip, collide.hip) ->
`ivx_world_set_contacts` -> step, all on one context. tests/frame_ref.py states the join (the float32 transform_to_object_space, the record with its
origin offset, the dispatch table, the merge order) once for both sides, and holds the oracle side of every scene: what a scene must contain is
asserted there, on the oracle's results."""
import numpy as np
import pytest

import frame_ref as fr
import narrow_ref as nr
import parity_util as pu
import physics_util as phu
import test_gpu_narrow as tn
from impact_amd import capi, collision, interaction
from impact_amd.physics import ConstraintSolverConfig, PhysicsWorld
from impact_amd.voxel import VoxelObjectInertialPropertyManager, VoxelObjectMesh

pytestmark = pytest.mark.gpu


def device_object(ctx, vb):
    """the oracle's object again on the device, meshed and with its collision probes: ranges, model box and probes equal the oracle's"""
    g = pu.gpu_from_graph(ctx, vb.graph, vb.extent)
    g.compute_all_derived_state()
    g.update_occupied_voxel_ranges()
    g.label_regions()
    g.mesh = VoxelObjectMesh.create(g)
    n = g.collision_probes_recompute()
    assert_probes_equal(g, vb, n)
    assert fr.model_aabb(g).tobytes() == fr.model_aabb(vb.o).tobytes()
    return g


def assert_probes_equal(g, vb, n):
    want_points, want_entries = vb.probes()
    got_points, got_entries = g.collision_probes()
    assert n == len(want_points) == len(got_points)
    np.testing.assert_array_equal(got_entries, want_entries)
    for e in want_entries:
        np.testing.assert_array_equal(got_points[e[3]:e[4]].view(np.uint32), want_points[e[3]:e[4]].view(np.uint32))


def single_object_manifolds(rows, mutual, voxel_bodies):
    """every row through the single-object call of its generator -> the lists, collidable rows first"""
    out = []
    for q, v in zip(rows.queries, rows.objects):
        g, ids = voxel_bodies[v].g, (int(q["collidable_id_a"]), int(q["collidable_id_b"]), int(q["body_a"]), int(q["body_b"]), q["response"])
        if q["mode"] == 0:
            out.append(g.sphere_contacts(q["rotation_xyzw"], q["translation"], q["shape3"], float(q["shape1"]), *ids))
        elif q["mode"] == 1:
            out.append(g.plane_contacts(q["rotation_xyzw"], q["translation"], q["shape3"], float(q["shape1"]), *ids))
        else:
            out.append(g.capsule_contacts(q["rotation_xyzw"], q["translation"], q["shape3"], q["shape3b"], float(q["shape1"]), *ids))
    for q, (a, b) in zip(mutual.queries, mutual.objects):
        out.append(voxel_bodies[a].g.mutual_contacts(q["rotation_a"], q["translation_a"], q["center_of_mass_a"], voxel_bodies[b].g, q["rotation_b"], q["translation_b"],
                                                     q["center_of_mass_b"], int(q["collidable_id_a"]), int(q["collidable_id_b"]), int(q["body_a"]), int(q["body_b"]),
                                                     q["response"]))
    return out


def test_static_mixed_scene_in_both_modes(ctx):
    """fr.static_scene: three voxel objects on turned dynamic bodies with their centres of mass as origin offsets, 13 spheres, 4 capsules, a plane
    last, some static or phantom. World collidables and boxes equal `ivx_cw_transform` over the world's bodies; contacts and deferred pairs equal
    narrow_ref over the downloaded records; every deferred pair's manifold from the two `_many` calls is bit-equal to the oracle generator's fed
    the same float32 rows; and every voxel pair the all-pairs broad phase did NOT defer gives an empty list from the single-object call"""
    local, dyn, kin, voxel_bodies = fr.static_scene()
    for vb in voxel_bodies.values():
        vb.g = device_object(ctx, vb)
    w, cw = tn.make_world(ctx, local, dyn, kin)
    try:
        world, boxes = tn.check_synchronized(w, cw, local, cw.synchronize())
        bodies = w.bodies()
        deferred_of, non_empty = {}, set()
        for mode in tn.MODES:  # (the generators run between the two collides: the set the world installed on the context is still its own)
            _, deferred = tn.check_collide(cw, local, world, boxes, mode)
            deferred_of[mode] = {tuple(p) for p in deferred.tolist()}
            rows, mutual = fr.dispatch(world, deferred, bodies, voxel_bodies)
            want = fr.oracle_manifolds(rows, mutual, voxel_bodies, len(deferred))
            got = fr.device_manifolds(rows, mutual, voxel_bodies, len(deferred))
            generators = fr.generator_of(rows, mutual, len(deferred))
            for g, m in zip(got, want):
                fr.assert_contacts_equal(g, m)
            # the scene, on the oracle's results: every generator at work, a pair whose boxes meet and whose shapes do not
            non_empty = {g for g, m in zip(generators, want) if len(m) > 0}
            assert non_empty == set(fr.GENERATORS), (mode, non_empty)
            assert any(len(m) == 0 for m in want), mode
            for shapes in ((nr.SPHERE, nr.VOXEL), (nr.VOXEL, nr.SPHERE), (nr.CAPSULE, nr.VOXEL), (nr.VOXEL, nr.CAPSULE), (nr.VOXEL, nr.VOXEL), (nr.VOXEL, nr.PLANE)):
                assert any((int(local["shape"][a]), int(local["shape"][b])) == shapes and len(m) > 0 for (a, b), m in zip(deferred.tolist(), want)), (mode, shapes)
        assert deferred_of[capi.BV_ALL_PAIRS] - deferred_of[capi.BV_DYNAMIC_PAIRS] and deferred_of[capi.BV_DYNAMIC_PAIRS] <= deferred_of[capi.BV_ALL_PAIRS]
        # completeness on the device: what the broad phase left out, the generators have nothing for
        others = [(min(v, c), max(v, c)) for v in voxel_bodies for c in range(len(local)) if c != v]
        left_out = sorted(set(others) - deferred_of[capi.BV_ALL_PAIRS])
        assert len(left_out) >= 10 and all(local["shape"][a] != nr.PLANE and local["shape"][b] != nr.PLANE for a, b in left_out)
        rows, mutual = fr.dispatch(world, left_out, bodies, voxel_bodies)
        lists = single_object_manifolds(rows, mutual, voxel_bodies)
        assert len(lists) == len(left_out) and all(len(m) == 0 for m in lists), [len(m) for m in lists]
    finally:
        w.close()
        for vb in voxel_bodies.values():
            vb.g.close()
            vb.g = None


class DeviceSide:
    """the falling scene on the device: the same per-frame flow as frame_ref.OracleSide, over the library's calls and its own bodies"""

    def __init__(self, ctx, oracle_side):
        self.oracle_side = oracle_side
        fresh = fr.falling_voxel_bodies()  # (oracle objects before any edit: the device objects are checked against them as they are built)
        self.local = fr.falling_scene(*fresh)[0]
        dyn, kin = oracle_side.initial_bodies
        self.voxel_bodies = {}
        for i, vb in zip((1, 3), fresh):
            self.voxel_bodies[i] = fr.DeviceBody(device_object(ctx, vb), vb.center_of_mass.copy(), vb.origin_offset.copy())
        self.densities = np.ones(256, dtype=np.float32)
        self.moments64 = VoxelObjectInertialPropertyManager.initialized_from(self.voxel_bodies[1].g, self.densities).m64.copy()
        self.w = PhysicsWorld(ctx, ConstraintSolverConfig(8, 0.4, 3, 0.2))
        self.w.set_bodies(dyn, kin)
        self.cw = collision.CollisionWorld(self.w)
        self.cw.set_collidables(self.local)
        self.synchronized = None

    def close(self):
        self.w.close()
        for b in self.voxel_bodies.values():
            b.g.close()

    def frame(self, enqueue=False):
        """synchronize -> collide -> dispatch -> generators -> merge -> step. `enqueue`: the step is only enqueued and the NEXT frame's synchronize is
        issued behind it with no wait between; the bodies are read after both"""
        bv_set = self.cw.synchronize() if self.synchronized is None else self.synchronized
        self.synchronized = None
        world, boxes = self.cw.download(), bv_set.download()[0]
        contacts, deferred = self.cw.collide(capi.BV_DYNAMIC_PAIRS)
        rows, mutual = fr.dispatch(world, deferred, self.w.bodies(), self.voxel_bodies)
        manifolds = fr.device_manifolds(rows, mutual, self.voxel_bodies, len(deferred))
        merged = fr.merge(contacts, manifolds)
        assert self.w.prepare_constraints(merged) == len(merged)
        if enqueue:
            self.w.step_enqueue(fr.DT)
            self.synchronized = self.cw.synchronize()
        else:
            self.w.step(fr.DT)
        f = {"deferred": deferred, "generators": fr.generator_of(rows, mutual, len(deferred)), "manifolds": manifolds, "merged": merged, "contacts": contacts, "boxes": boxes}
        return fr.frame_record(f, self.w.bodies()[0])

    def bite(self, oracle_edit):
        """the edit of frame_ref.OracleSide.bite through the library: absorb, mesh and probe sync, the body through
        `apply_updated_inertial_properties_to_rigid_body`, the collidable set again from the new `grid_model_aabb` and the new local centre of mass"""
        box = self.voxel_bodies[1]
        centre, influence, radius = fr.BITE
        res = box.g.absorb_sphere(np.array(centre, dtype=np.float32), influence, radius, self.densities)
        np.testing.assert_array_equal(res["invalidated"], oracle_edit["invalidated"])
        box.g.mesh.sync_with_voxel_object(res["invalidated"])
        n = box.g.collision_probes_sync(res["invalidated"])
        assert_probes_equal(box.g, self.oracle_side.box, n)
        assert fr.model_aabb(box.g).tobytes() == fr.model_aabb(self.oracle_side.box.o).tobytes()  # (the ranges followed the edit)
        self.moments64 = self.moments64 - res["removed_moments"]
        dyn, kin = self.w.bodies()
        body, new_com = interaction.apply_updated_inertial_properties_to_rigid_body(dyn[0], self.moments64, box.origin_offset)
        dyn[0] = body
        self.w.set_bodies(dyn, kin)
        box.origin_offset, box.center_of_mass = new_com.copy(), VoxelObjectInertialPropertyManager(self.moments64).derive_center_of_mass().astype(np.float32)
        self.local = fr.reseated_collidable(self.local, 1, box.g, new_com)
        self.cw.set_collidables(self.local)
        return {"body": body, "new_offset": new_com}


def assert_frames_agree(got, want, what, inertial_fields_of=None):
    """the per-frame assertions: equal deferred lists, every manifold of the same length, equal merged counts, the bodies within physics_util.RTOL"""
    assert got["deferred"].tolist() == want["deferred"].tolist(), what
    assert got["generators"] == want["generators"], what
    assert got["lengths"] == want["lengths"], (what, got["lengths"], want["lengths"])
    assert got["n_merged"] == want["n_merged"] and got["n_primitive"] == want["n_primitive"], what
    bodies = got["bodies"]
    if inertial_fields_of is not None:
        # after the edit the box's mass and inertia tensor come from float64 moments in the library and from float32 sums in the oracle (compared
        # where the edit is made, at test_gpu_interaction.py's tolerances): the exact comparison of these fields below is given the oracle's
        bodies = bodies.copy()
        for f in ("mass", "inertia", "inv_inertia", "total_force"):
            bodies[f][inertial_fields_of] = want["bodies"][f][inertial_fields_of]
    phu.assert_bodies_close(bodies, want["bodies"], what=what)


def run_frames(side, want_records, first, count, enqueue_at=None):
    for k in range(first, first + count):
        got = side.frame(enqueue=(k == enqueue_at))
        assert_frames_agree(got, want_records[k], f"frame {k}: ", inertial_fields_of=0 if k >= fr.N_FRAMES else None)


def test_frames_of_voxel_bodies_coming_to_rest(ctx):
    """fr.falling_scene, 60 frames of 4 ms, each side with its own bodies: a voxel box lands on the plane, a voxel sphere on the box, a ball on the box
    and a capsule on the sphere. One frame only enqueues its step and the next synchronize follows with no wait between"""
    run = fr.oracle_run()
    records = run["records"][:fr.N_FRAMES]
    fr.assert_run_is_physical(run["side"], records, fr.N_FRAMES)
    assert len({tuple(map(tuple, r["deferred"].tolist())) for r in records}) >= 2  # (the deferred list changes during the run)
    side = DeviceSide(ctx, run["side"])
    try:
        run_frames(side, records, 0, fr.N_FRAMES, enqueue_at=33)
    finally:
        side.close()


def test_the_same_scene_across_an_edit(ctx):
    """after the 60 frames the voxel box loses its +x end to `absorb_sphere` on both sides: mesh and probes synced, the body re-seated on the new
    inertial properties, the collidable set again from the new model box and the new local centre of mass; 15 further frames hold the same
    assertions. A record set again WITHOUT the new offset no longer holds the object (the oracle side alone shows it)"""
    run = fr.oracle_run()
    edit, records = run["edit"], run["records"]
    fr.assert_run_is_physical(run["side"], records, fr.N_FRAMES + fr.N_FRAMES_AFTER_EDIT)
    assert np.abs(edit["new_offset"] - edit["old_offset"]).max() > fr.EXTENT
    shift = (edit["old_offset"] - edit["new_offset"]).astype(np.float64)
    np.testing.assert_allclose(edit["record"]["a"] - edit["record_before"]["a"], shift, atol=1e-6)  # (the record moved by the change of the offset)
    assert records[fr.N_FRAMES]["boxes"][1].tobytes() != records[fr.N_FRAMES - 1]["boxes"][1].tobytes()  # (the world box changed)
    body = edit["body"]
    corners = fr.model_box_corners_in_world_f64(run["side"].box.o, edit["new_offset"], body["position"], body["orientation"])
    assert fr.box_contains(collision.transform(edit["record"], body["position"], body["orientation"])[1], corners)
    assert not fr.box_contains(collision.transform(edit["stale_record"], body["position"], body["orientation"])[1], corners)
    side = DeviceSide(ctx, run["side"])
    try:
        run_frames(side, records, 0, fr.N_FRAMES)
        got = side.bite(edit)
        np.testing.assert_allclose(got["new_offset"], edit["new_offset"], rtol=1e-5, atol=1e-5)
        assert abs(float(got["body"]["mass"]) - float(body["mass"])) <= 1e-5 * float(body["mass"])
        for f in ("inertia", "inv_inertia"):
            assert np.abs(got["body"][f].astype(np.float64) - body[f].astype(np.float64)).max() <= 1e-4 * float(np.abs(body[f]).max()), f
        assert side.local[1].tobytes() != fr.falling_scene(*fr.falling_voxel_bodies())[0][1].tobytes()
        run_frames(side, records, fr.N_FRAMES, fr.N_FRAMES_AFTER_EDIT)
    finally:
        side.close()
