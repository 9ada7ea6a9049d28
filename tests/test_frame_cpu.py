"""Host-side checks of the join between the collision world and the voxel contact generators (tests/frame_ref.py): the float32 derivation of a voxel
body's transform_to_object_space, the dispatch table of the deferred pairs, the record of a voxel object with its origin offset, and the completeness
of the broad phase for a real voxel object — over the oracle, narrow_ref.py and the library's host functions. No kernels are launched."""
import numpy as np
import pytest

import bvol_ref as br
import frame_ref as fr
import narrow_ref as nr
from impact_amd import capi, collision, scenes

f32 = np.float32
S, P, CAP, V = nr.SPHERE, nr.PLANE, nr.CAPSULE, nr.VOXEL
N_POSES = 2000

# The largest errors of `to_object_space_f32` measured on the 2 000 seeded poses below (seed 11; positions within +-30, origin offsets within a 16 wide
# grid), as a fraction of the scene's scale S = max(1, largest |coordinate| of the position, of the offset and of the grid's far corner):
#   TRANSLATION: |translation - translation64|_inf against the same composition in float64;
#   ROUND_TRIP:  |x' - x|_inf for every voxel centre x of a 4 x 4 x 4 grid, taken to world space in float64 and back through the float32 transform.
# The tests allow FOUR TIMES these, the margin of test_narrow_cpu.py.
MEASURED_TRANSLATION = 4.7e-7
MEASURED_ROUND_TRIP = 5.3e-7
GRID_SIZE = 16.0


def qrot64(q, v):
    return nr.qrot(np.asarray(q, dtype=np.float64), np.asarray(v, dtype=np.float64))


def seeded_poses(n=N_POSES, seed=11):
    rng = np.random.default_rng(seed)
    q = np.array([br.random_unit_quaternion(rng) for _ in range(n)], dtype=np.float32)
    return rng.uniform(-30.0, 30.0, (n, 3)).astype(np.float32), q, rng.uniform(0.0, GRID_SIZE, (n, 3)).astype(np.float32)


def test_transform_to_object_space_in_float32():
    p, q, off = seeded_poses()
    q_i, t = fr.to_object_space_f32(p, q, off)
    assert q_i.dtype == np.float32 and t.dtype == np.float32
    np.testing.assert_array_equal(q_i, np.concatenate([-q[:, :3], q[:, 3:]], axis=1))
    scale = np.maximum(1.0, np.maximum(np.abs(p).max(axis=1), GRID_SIZE)).astype(np.float64)
    # against the same composition in float64
    p64, q64, off64 = p.astype(np.float64), q.astype(np.float64), off.astype(np.float64)
    t64 = -qrot64(fr.conjugate(q64), qrot64(q64, -off64) + p64)
    translation_error = (np.abs(t.astype(np.float64) - t64).max(axis=1) / scale).max()
    # every voxel centre of a small grid at the far corner of the offsets' range: to world space in float64, back through the float32 transform
    centres = (np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), axis=-1).reshape(-1, 3) + 0.5) * 0.5 + (GRID_SIZE - 2.0)
    round_trip_error = 0.0
    for x in centres:
        x_world = qrot64(q64, x - off64) + p64
        back = qrot64(q_i, x_world) + t.astype(np.float64)
        round_trip_error = max(round_trip_error, (np.abs(back - x).max(axis=1) / scale).max())
    print(f"to_object_space_f32 over {N_POSES} poses: translation error {translation_error:.3e} S, round trip {round_trip_error:.3e} S")
    assert translation_error <= 4.0 * MEASURED_TRANSLATION, translation_error
    assert round_trip_error <= 4.0 * MEASURED_ROUND_TRIP, round_trip_error
    # the float64 composition the chain tests round once is NOT this derivation: it gives other bits (reported; that it happens at all is why this
    # restatement exists)
    differing = 0
    for i in range(N_POSES):
        q_r, t_r = fr.to_object_space_f64_rounded(q[i], p[i], off64[i])
        differing += q_r.tobytes() != q_i[i].tobytes() or t_r.tobytes() != t[i].tobytes()
    print(f"poses whose float32 derivation differs in bits from the float64 composition rounded once: {differing} of {N_POSES}")
    assert differing > 0


# generate_contact_manifold, impact_voxel/src/collidable.rs:138-215, typed row by row: (shape of a, shape of b) -> (generator, the member whose id the
# contact ids take first, the member whose body is A)
DISPATCH_TABLE = {
    (V, V): ("mutual", "a", "a"),
    (CAP, V): ("capsule", "a", "a"),
    (V, CAP): ("capsule", "b", "b"),
    (S, V): ("sphere", "a", "a"),
    (V, S): ("sphere", "b", "b"),
    (V, P): ("plane", "b", "a"),
    (P, V): ("plane", "a", "b"),
}


@pytest.fixture(scope="module")
def small_sphere():
    return fr.voxel_body(scenes.sphere_scene(12.0), 0.5)


def test_dispatch_table(small_sphere):
    """every ordered shape pair with a voxel member: generator, id order, body order, shape, transform and response of the row"""
    vb = small_sphere
    members = {S: collision.sphere((1, 2, 3), 0.5, 1, 101, response=(0.1, 0.2, 0.9)), P: collision.plane((0, 1, 0), 0.25, 0, 102, response=(0.7, 0.5, 0.3), kinematic=True),
               CAP: collision.capsule((1, 0, 0), (0, 2, 0), 0.4, 2, 103, response=(0.2, 0.8, 0.6))}
    dyn = np.array([nr.unit_body((3.0, -1.0, 2.0), br.random_unit_quaternion(np.random.default_rng(k))) for k in range(5)], dtype=capi.RIGID_BODY_DTYPE)
    kin = np.zeros(1, dtype=capi.KINEMATIC_BODY_DTYPE)
    kin["orientation"] = (0, 0, 0, 1)
    for (sa, sb), (generator, first_id, body_a) in DISPATCH_TABLE.items():
        local = np.zeros(2, dtype=capi.COLLIDABLE_DTYPE)
        voxel_bodies = {}
        for k, shape in enumerate((sa, sb)):
            if shape == V:
                local[k] = fr.voxel_collidable(vb.o, vb.origin_offset, 3 + k, 200 + k, response=(0.3 + 0.1 * k, 0.6, 0.4))
                voxel_bodies[k] = vb
            else:
                local[k] = members[shape]
        world, _ = nr.transform(local, *nr.body_frames(local, dyn, kin))
        rows, mutual = fr.dispatch(world, [(0, 1)], (dyn, kin), voxel_bodies)
        assert fr.generator_of(rows, mutual, 1) == [generator], (sa, sb)
        pick = {"a": 0, "b": 1}
        if generator == "mutual":
            assert len(rows.queries) == 0 and len(mutual.queries) == 1 and mutual.source == [0] and mutual.objects == [(0, 1)]
            q = mutual.queries[0]
            for side, k in (("a", 0), ("b", 1)):
                want_q, want_t = fr.to_object_space_f32(dyn[3 + k]["position"], dyn[3 + k]["orientation"], vb.origin_offset)
                assert q["rotation_" + side].tobytes() == want_q.tobytes() and q["translation_" + side].tobytes() == want_t.tobytes()
                assert q["center_of_mass_" + side].tobytes() == vb.center_of_mass.tobytes()
        else:
            assert len(mutual.queries) == 0 and len(rows.queries) == 1 and rows.source == [0]
            q = rows.queries[0]
            v = 0 if sa == V else 1
            c = 1 - v
            assert rows.objects == [v]
            want_q, want_t = fr.to_object_space_f32(dyn[3 + v]["position"], dyn[3 + v]["orientation"], vb.origin_offset)
            assert q["rotation_xyzw"].tobytes() == want_q.tobytes() and q["translation"].tobytes() == want_t.tobytes()
            assert q["shape3"].tobytes() == world["a"][c].tobytes() and q["shape1"] == world["s"][c]
            assert generator != "capsule" or q["shape3b"].tobytes() == world["b"][c].tobytes()
        assert int(q["collidable_id_a"]) == int(local["id"][pick[first_id]]) and int(q["collidable_id_b"]) == int(local["id"][1 - pick[first_id]]), (sa, sb)
        assert int(q["body_a"]) == int(local["body"][pick[body_a]]) and int(q["body_b"]) == int(local["body"][1 - pick[body_a]]), (sa, sb)
        r1, r2 = local["response"][0], local["response"][1]
        assert q["response"].tolist() == [max(r1[0], r2[0]), np.sqrt(r1[1] * r2[1]), np.sqrt(r1[2] * r2[2])]
    assert len(DISPATCH_TABLE) == 7


def test_world_box_of_a_voxel_object_with_an_origin_offset(small_sphere):
    """`ivx_cw_transform` of the shifted record: the world box holds the float64 image of the eight corners of the occupied model box under every
    seeded pose; the record without the shift does not (the mistake `collision.voxel_object`'s docstring used to invite)"""
    vb = small_sphere
    assert np.abs(vb.origin_offset).min() > 4.0  # (the centre of mass of a 12 wide sphere, far from the grid's origin)
    p, q, _ = seeded_poses(200, seed=12)
    shifted = fr.voxel_collidable(vb.o, vb.origin_offset, 0, 1)
    unshifted = fr.voxel_collidable(vb.o, vb.origin_offset, 0, 1, shifted=False)
    np.testing.assert_array_equal(shifted["b"] - shifted["a"], unshifted["b"] - unshifted["a"])
    unshifted_fails = 0
    for i in range(len(p)):
        corners = fr.model_box_corners_in_world_f64(vb.o, vb.origin_offset, p[i], q[i])
        assert fr.box_contains(collision.transform(shifted, p[i], q[i])[1], corners), i
        unshifted_fails += not fr.box_contains(collision.transform(unshifted, p[i], q[i])[1], corners)
    assert unshifted_fails >= 1


def test_broad_phase_is_complete_for_a_voxel_sphere(small_sphere):
    """one voxel sphere (radius 12 voxels, extent 0.5) under a rotated pose, 64 spheres and 32 capsules around it, a plane through it: a primitive whose
    float32 world box misses the object's must be one the oracle's generator finds nothing for"""
    local, dyn, kin, voxel_bodies = fr.completeness_scene(small_sphere)
    positions, orientations = nr.body_frames(local, dyn, kin)
    world, boxes = np.zeros_like(local), np.zeros(len(local), dtype=capi.AABB_DTYPE)
    for i in range(len(local)):
        world[i], boxes[i] = collision.transform(local[i], positions[i], orientations[i])
    pairs = nr.broad_phase_pairs(boxes, local["kind"], capi.BV_ALL_PAIRS)
    deferred = {int(b) for a, b in pairs if a == 0}
    everything = [(0, i) for i in range(1, len(local))]
    rows, mutual = fr.dispatch(world, everything, (dyn, kin), voxel_bodies)
    manifolds = fr.oracle_manifolds(rows, mutual, voxel_bodies, len(everything))
    generators = fr.generator_of(rows, mutual, len(everything))
    assert generators.count("sphere") == 64 and generators.count("capsule") == 32 and generators.count("plane") == 1
    empty_deferred = 0
    for (_, i), m in zip(everything, manifolds):
        assert i in deferred or len(m) == 0, (i, len(m), generators[i - 1])
        empty_deferred += i in deferred and len(m) == 0
    n = len(everything)
    assert len(deferred) >= n / 4 and n - len(deferred) >= n / 4, (len(deferred), n)
    assert empty_deferred >= 5, empty_deferred
    assert sum(len(m) > 0 for m in manifolds) >= 10 and len(manifolds[-1]) > 0  # (the plane cuts the object)


def test_static_scene_on_the_oracle_side():
    """what tests/test_gpu_frame.py's static scene must contain, without a GPU: in both modes every generator with a non-empty manifold, a deferred pair
    with an empty one, every argument order of the dispatch the scene can hold, and a pair deferred in mode 0 that mode 1 leaves out"""
    local, dyn, kin, voxel_bodies = fr.static_scene()
    assert local["shape"][-1] == P and (local["shape"][:-1] != P).all() and (local["shape"] == V).sum() == 3
    assert (local["shape"] == S).sum() == 13 and (local["shape"] == CAP).sum() == 4 and {0, 1, 2} <= set(local["kind"].tolist())
    deferred_of = {}
    for mode in (capi.BV_ALL_PAIRS, capi.BV_DYNAMIC_PAIRS):
        f = fr.oracle_frame(local, voxel_bodies, (dyn, kin), mode)
        deferred_of[mode] = {tuple(p) for p in f["deferred"].tolist()}
        assert {g for g, m in zip(f["generators"], f["manifolds"]) if len(m) > 0} == set(fr.GENERATORS), mode
        assert any(len(m) == 0 for m in f["manifolds"]), mode
        assert sum(len(m) for m in f["manifolds"]) + len(f["contacts"]) == len(f["merged"])
    assert deferred_of[capi.BV_ALL_PAIRS] - deferred_of[capi.BV_DYNAMIC_PAIRS]


def test_falling_scene_on_the_oracle_side():
    """the run tests/test_gpu_frame.py compares the device with, on the oracle alone: every generator at work in ten frames or more, nothing under the
    plane and nothing faster than free fall at the end of the 60 frames and of the 15 after the edit; the edit moves the origin offset and shrinks the
    model box, and a record set again with the OLD offset no longer holds the object"""
    run = fr.oracle_run()
    records, edit, side = run["records"], run["edit"], run["side"]
    fr.assert_run_is_physical(side, records[:fr.N_FRAMES], fr.N_FRAMES)
    fr.assert_run_is_physical(side, records, fr.N_FRAMES + fr.N_FRAMES_AFTER_EDIT)
    for generator in fr.GENERATORS:
        print(f"frames with a non-empty {generator} manifold: {fr.frames_with(records[:fr.N_FRAMES], generator)} of {fr.N_FRAMES}")
    assert np.abs(edit["new_offset"] - edit["old_offset"]).max() > fr.EXTENT
    body = edit["body"]
    corners = fr.model_box_corners_in_world_f64(side.box.o, edit["new_offset"], body["position"], body["orientation"])
    assert fr.box_contains(collision.transform(edit["record"], body["position"], body["orientation"])[1], corners)
    assert not fr.box_contains(collision.transform(edit["stale_record"], body["position"], body["orientation"])[1], corners)
    # the merged list is the primitive contacts first: every frame's count is the sum of its parts
    assert all(r["n_merged"] == r["n_primitive"] + sum(r["lengths"]) for r in records)
