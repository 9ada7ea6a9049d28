"""GPU parity of voxel contact generation (sphere collidables): `ivx_sphere_voxel_object_contacts` through the
C ABI against the oracle (pinned in tests/test_oracle_voxel.py by a brute-force sweep): the same contacts in the same order
with the same ids, geometry bit-exact; then the whole chain the reference runs every frame for a ball on a voxel body — contact
generation -> prepare constraints -> solve -> integrate — against the oracle doing the same, step by step."""
import numpy as np
import pytest

import oracle_lib as ol
import parity_util as pu
import physics_util as phu
from impact_amd import scenes
from impact_amd.capi import CONTACT_DTYPE

pytestmark = pytest.mark.gpu


def both(ctx, graph, extent):
    o = pu.oracle_from_graph(graph, extent)
    g = pu.gpu_from_graph(ctx, graph, extent)
    o.update_occupied_voxel_ranges()
    o.compute_all_derived_state()
    g.compute_all_derived_state()
    g.update_occupied_voxel_ranges()
    g.label_regions()
    return o, g


def oracle_contact_list(o, q, t, c, r, id_a, id_b, body_a, body_b, response):
    idx, pos, nrm, dep = o.sphere_contacts(q, t, c, r)
    out = np.zeros(len(idx), dtype=CONTACT_DTYPE)
    for n, (ijk, p, nn, d) in enumerate(zip(idx, pos, nrm, dep)):
        out[n]["id"] = scenes.contact_id(id_a, id_b, *[int(x) for x in ijk])
        out[n]["body_a"], out[n]["body_b"] = body_a, body_b
        out[n]["position"], out[n]["normal"], out[n]["depth"] = p, nn, d
        out[n]["restitution"], out[n]["static_friction"], out[n]["dynamic_friction"] = response
        out[n]["flags"] = 1 if n == 0 else 0
    return out


def assert_contacts_equal(got, want):
    assert len(got) == len(want)
    for f in ("id", "body_a", "body_b", "flags"):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)
    for f in ("position", "normal", "depth", "restitution", "static_friction", "dynamic_friction"):
        np.testing.assert_array_equal(got[f].view(np.uint32), want[f].view(np.uint32), err_msg=f)  # f32 bit patterns


@pytest.mark.parametrize("extent", [1.0, 0.5])
def test_sphere_against_rotated_voxel_body(ctx, extent):
    o, g = both(ctx, scenes.sphere_scene(20.0), extent)
    axis = np.array([0.3, -1.0, 0.5]) / np.linalg.norm([0.3, -1.0, 0.5])
    q = np.array([*(axis * np.sin(0.45)), np.cos(0.45)], dtype=np.float32)
    t = np.array([1.5, -2.25, 0.75], dtype=np.float32)
    ctr = np.array([0.5 * (a + b) for a, b in o.info()["occupied_voxel_ranges"]], dtype=np.float64) * extent
    resp = (0.4, 0.7, 0.5)
    for direction, depth_in in (([1, 0, 0], 1.0), ([0.6, 0.0, 0.8], 0.2), ([-0.5, 0.5, 0.7], 3.0), ([0, 1, 0], -8.0)):
        d = np.asarray(direction, dtype=np.float64)
        d /= np.linalg.norm(d)
        p_obj = ctr + d * (20.0 * extent + 4.0 - depth_in)  # ball of radius 4 pushed `depth_in` into the surface (negative: apart)
        x, y, z, w = [float(a) for a in q]
        b = np.array([-x, -y, -z])
        v = p_obj - t.astype(np.float64)
        c_world = (v * (w * w - b @ b) + b * (2 * (v @ b)) + np.cross(b, v) * (2 * w)).astype(np.float32)
        want = oracle_contact_list(o, q, t, c_world, 4.0, 77, 1234567, 0, 1, resp)
        got = g.sphere_contacts(q, t, c_world, 4.0, 77, 1234567, 0, 1, resp)
        assert (len(want) > 0) == (depth_in > -1.0)
        assert_contacts_equal(got, want)
    g.close()


def test_capacity_error_reports_the_count(ctx):
    from impact_amd.capi import IvxError

    o, g = both(ctx, scenes.sphere_scene(20.0), 1.0)
    ctr = np.array([0.5 * (a + b) for a, b in o.info()["occupied_voxel_ranges"]], dtype=np.float32)
    with pytest.raises(IvxError):
        g.sphere_contacts((0, 0, 0, 1), (0, 0, 0), ctr + np.array([22.0, 0, 0], np.float32), 6.0, 1, 2, 0, 1, capacity=3)
    g.close()


def test_ball_dropped_on_a_voxel_body_steps_like_the_oracle(ctx):
    """the per-frame chain: contacts from the voxel body's current pose -> prepare -> solve -> integrate, 60 steps; the ball
    (dynamic) lands on a heavy voxel sphere (dynamic too, at rest); GPU contacts feed the GPU solver, oracle contacts the oracle"""
    extent = 0.25
    o, g = both(ctx, scenes.sphere_scene(16.0), extent)  # radius 4.0 world units
    inf = o.info()
    ctr = np.array([0.5 * (a + b) for a, b in inf["occupied_voxel_ranges"]], dtype=np.float64) * extent  # body centre in model space
    ball_r = 0.75
    # rigid bodies: 0 = the ball, 1 = the voxel body (its body frame origin = the centre of the voxel sphere)
    ball = ol.uniform_sphere_body(ball_r, 2.0, (0.3, 4.0 + ball_r + 0.05, -0.2), (0.0, -1.0, 0.0))
    body = ol.uniform_sphere_body(4.0, 5.0, (0.0, 0.0, 0.0))
    dyn = np.array([ball, body])
    dyn["total_force"][0] = (0.0, -9.81 * float(dyn["mass"][0]), 0.0)
    w, op = phu.make_pair(ctx, dyn)
    resp = (0.2, 0.6, 0.4)
    had_contact = False
    for step in range(60):
        gd = w.bodies()[0]
        od = op.bodies()[0]
        lists = []
        for src, bodies in ((g, gd), (o, od)):
            # transform_to_object_space: world -> model space of the voxel body = translate(model centre) . inverse(body pose)
            qb = bodies["orientation"][1].astype(np.float64)
            pb = bodies["position"][1].astype(np.float64)
            qi = np.array([-qb[0], -qb[1], -qb[2], qb[3]])
            x, y, z, ww = qi
            bv = np.array([x, y, z])
            v = -pb
            tr = (v * (ww * ww - bv @ bv) + bv * (2 * (v @ bv)) + np.cross(bv, v) * (2 * ww)) + ctr
            c = bodies["position"][0]
            if src is g:
                lists.append(g.sphere_contacts(qi.astype(np.float32), tr.astype(np.float32), c, ball_r, 11, 22, 0, 1, resp))
            else:
                lists.append(oracle_contact_list(o, qi.astype(np.float32), tr.astype(np.float32), c, ball_r, 11, 22, 0, 1, resp))
        had_contact |= len(lists[1]) > 0
        assert len(lists[0]) == len(lists[1]), step
        w.perform_physics_step(lists[0], 0.004)
        op.step(lists[1], 0.004)
        phu.assert_bodies_close(w.bodies()[0], op.bodies()[0], what=f"step {step}: ")
    assert had_contact
    w.close()
    g.close()


def oracle_plane_contact_list(o, q, t, n, disp, id_a, id_b, body_a, body_b, response):
    idx, pos, nrm, dep = o.plane_contacts(q, t, n, disp)
    out = np.zeros(len(idx), dtype=CONTACT_DTYPE)
    for m, (ijk, p, nn, d) in enumerate(zip(idx, pos, nrm, dep)):
        out[m]["id"] = scenes.contact_id(id_a, id_b, *[int(x) for x in ijk])
        out[m]["body_a"], out[m]["body_b"] = body_a, body_b
        out[m]["position"], out[m]["normal"], out[m]["depth"] = p, nn, d
        out[m]["restitution"], out[m]["static_friction"], out[m]["dynamic_friction"] = response
        out[m]["flags"] = 1 if m == 0 else 0
    return out


def test_plane_against_rotated_voxel_box(ctx):
    extent = 0.5
    o, g = both(ctx, scenes.box_scene((20.0, 14.0, 18.0)), extent)
    axis = np.array([0.2, 1.0, -0.4]) / np.linalg.norm([0.2, 1.0, -0.4])
    q = np.array([*(axis * np.sin(0.3)), np.cos(0.3)], dtype=np.float32)
    t = np.array([0.5, 2.0, -1.0], dtype=np.float32)
    resp = (0.1, 0.8, 0.6)
    for normal, disp in (((0.0, 1.0, 0.0), -3.0), ((0.1, 1.0, 0.05), -4.2), ((0.0, 0.0, 1.0), -30.0), ((-0.6, 0.8, 0.0), -2.0)):
        n = np.asarray(normal, dtype=np.float64)
        n = (n / np.linalg.norm(n)).astype(np.float32)
        want = oracle_plane_contact_list(o, q, t, n, disp, 5, 9, 0, 0x80000000, resp)
        got = g.plane_contacts(q, t, n, disp, 5, 9, 0, 0x80000000, resp)
        assert_contacts_equal(got, want)
    g.close()


def test_ground_plane_through_a_box_of_343_chunks(ctx):
    """the exclusive scan over the chunks of the collidable's box takes 256 chunks a round: a solid box of 7 x 7 x 7 chunks (112 voxels a side)
    against ground planes through it. A plane restricts the touched ranges along its normal: the level plane through the middle leaves
    7 x 4 x 7 = 196 chunks (one round), the high one and the tilted one leave all 343 (two rounds), and the box's lower corner voxels, the only
    ones a plane tests, sit in chunks 0, 6, 294 and 300 of that box: two contacts take their offsets from the second round's carry"""
    o, g = both(ctx, scenes.box_scene((110.0, 110.0, 110.0)), 1.0)
    assert tuple(o.info()["chunk_counts"]) == (7, 7, 7)
    ident = (np.array([0.0, 0.0, 0.0, 1.0], dtype=np.float32), np.zeros(3, dtype=np.float32))
    axis = np.array([0.2, 1.0, -0.4]) / np.linalg.norm([0.2, 1.0, -0.4])
    turned = (np.array([*(axis * np.sin(0.3)), np.cos(0.3)], dtype=np.float32), np.array([0.5, 2.0, -1.0], dtype=np.float32))
    resp = (0.1, 0.8, 0.6)
    for (q, t), normal, disp, whole_box in ((ident, (0.0, 1.0, 0.0), 56.0, False), (ident, (0.0, 1.0, 0.0), 100.0, True), (ident, (0.3, 1.0, 0.2), None, True),
                                            (turned, (0.1, 1.0, 0.05), 60.0, False)):
        n = np.asarray(normal, dtype=np.float64)
        n = (n / np.linalg.norm(n)).astype(np.float32)
        if disp is None:
            disp = float(n.astype(np.float64) @ np.array([56.0, 56.0, 56.0]))  # through the box's centre
        want = oracle_plane_contact_list(o, q, t, n, disp, 5, 9, 0, 0x80000000, resp)
        got = g.plane_contacts(q, t, n, disp, 5, 9, 0, 0x80000000, resp)
        assert len(want) >= 2
        if whole_box:
            idx = np.asarray(o.plane_contacts(q, t, n, disp)[0]) // 16
            in_box = (idx[:, 0] * 7 + idx[:, 1]) * 7 + idx[:, 2]
            assert in_box.min() < 256 <= in_box.max()
        assert_contacts_equal(got, want)
    g.close()


def test_voxel_box_dropped_on_the_ground_steps_like_the_oracle(ctx):
    """a voxel box (dynamic body) falls onto a static plane: corner-voxel contacts -> prepare -> solve (with positional correction) ->
    integrate, 80 steps against the oracle running the same chain"""
    extent = 0.25
    o, g = both(ctx, scenes.box_scene((16.0, 12.0, 20.0)), extent)  # 4 x 3 x 5 world units
    inf = o.info()
    ctr = np.array([0.5 * (a + b) for a, b in inf["occupied_voxel_ranges"]], dtype=np.float64) * extent
    mass = 4.0 * 3.0 * 5.0
    I = np.diag([mass / 12 * (9 + 25), mass / 12 * (16 + 25), mass / 12 * (16 + 9)])
    ang = 0.15
    box = ol.rigid_body_new(mass, I, (0.0, 1.5 + 0.6, 0.0), (np.sin(ang / 2), 0.0, 0.0, np.cos(ang / 2)), (0.0, -0.5, 0.0), (0.0, 0.0, 0.1))
    dyn = np.array([box])
    dyn["total_force"][0] = (0.0, -9.81 * mass, 0.0)
    w, op = phu.make_pair(ctx, dyn, phu.static_plane())
    resp = (0.0, 0.7, 0.5)
    n = np.array([0.0, 1.0, 0.0], dtype=np.float32)
    had_contact = False
    for step in range(80):
        lists = []
        for src, bodies in ((g, w.bodies()[0]), (o, op.bodies()[0])):
            qb = bodies["orientation"][0].astype(np.float64)
            pb = bodies["position"][0].astype(np.float64)
            qi = np.array([-qb[0], -qb[1], -qb[2], qb[3]])
            bv = qi[:3]
            v = -pb
            tr = (v * (qi[3] * qi[3] - bv @ bv) + bv * (2 * (v @ bv)) + np.cross(bv, v) * (2 * qi[3])) + ctr
            if src is g:
                lists.append(g.plane_contacts(qi.astype(np.float32), tr.astype(np.float32), n, 0.0, 3, 4, 0, 0x80000000, resp))
            else:
                lists.append(oracle_plane_contact_list(o, qi.astype(np.float32), tr.astype(np.float32), n, 0.0, 3, 4, 0, 0x80000000, resp))
        had_contact |= len(lists[1]) > 0
        assert len(lists[0]) == len(lists[1]), step
        w.perform_physics_step(lists[0], 0.004)
        op.step(lists[1], 0.004)
        phu.assert_bodies_close(w.bodies()[0], op.bodies()[0], what=f"step {step}: ")
    assert had_contact
    w.close()
    g.close()


# ---- capsule collidables --------------------------------------------------------------------------------------------------------
def oracle_capsule_contact_list(o, q, t, a, v, r, id_a, id_b, body_a, body_b, response):
    idx, pos, nrm, dep = o.capsule_contacts(q, t, a, v, r)
    out = np.zeros(len(idx), dtype=CONTACT_DTYPE)
    for m, (ijk, p, nn, d) in enumerate(zip(idx, pos, nrm, dep)):
        out[m]["id"] = scenes.contact_id(id_a, id_b, *[int(x) for x in ijk])
        out[m]["body_a"], out[m]["body_b"] = body_a, body_b
        out[m]["position"], out[m]["normal"], out[m]["depth"] = p, nn, d
        out[m]["restitution"], out[m]["static_friction"], out[m]["dynamic_friction"] = response
        out[m]["flags"] = 1 if m == 0 else 0
    return out


@pytest.mark.parametrize("extent", [1.0, 0.5])
def test_capsule_against_rotated_voxel_body(ctx, extent):
    """for_each_capsule_voxel_object_contact: capsules lying on, poking into, skewering and missing a rotated + translated body;
    a zero-length capsule; a capsule whose segment passes exactly through voxel centres (the any-orthogonal-vector branch of
    determine_capsule_sphere_contact_geometry)"""
    o, g = both(ctx, scenes.sphere_scene(20.0), extent)
    axis = np.array([0.3, -1.0, 0.5]) / np.linalg.norm([0.3, -1.0, 0.5])
    q = np.array([*(axis * np.sin(0.45)), np.cos(0.45)], dtype=np.float32)
    t = np.array([1.5, -2.25, 0.75], dtype=np.float32)
    ctr = np.array([0.5 * (a + b) for a, b in o.info()["occupied_voxel_ranges"]], dtype=np.float64) * extent
    R = 20.0 * extent
    resp = (0.4, 0.7, 0.5)

    def to_world(p_obj):
        x, y, z, w = [float(a) for a in q]
        b = np.array([-x, -y, -z])
        v = p_obj - t.astype(np.float64)
        return v * (w * w - b @ b) + b * (2 * (v @ b)) + np.cross(b, v) * (2 * w)

    cases = [
        (ctr + [-0.4 * R, R + 1.0, 0.1 * R], ctr + [0.5 * R, R + 1.4, -0.2 * R], 2.0, True),  # lying on top
        (ctr + [2.0 * R, 0.3, 0.2], ctr + [0.7 * R, 0.1, -0.1], 1.0, True),  # poking in along x
        (ctr + [-2.0 * R, -2.0 * R, 0.0], ctr + [2.0 * R, 2.0 * R, 0.5], 0.75, True),  # skewer through the middle
        (ctr + [0.0, 3.0 * R, 0.0], ctr + [R, 3.0 * R, R], 2.0, False),  # miss
        (ctr + [0.0, 0.0, R + 0.5], ctr + [0.0, 0.0, R + 0.5], 2.5, True),  # zero length
    ]
    for a_obj, b_obj, rad, hits in cases:
        a_w = to_world(np.asarray(a_obj)).astype(np.float32)
        v_w = (to_world(np.asarray(b_obj)) - to_world(np.asarray(a_obj))).astype(np.float32)
        want = oracle_capsule_contact_list(o, q, t, a_w, v_w, rad, 31, 987654321, 2, 5, resp)
        got = g.capsule_contacts(q, t, a_w, v_w, rad, 31, 987654321, 2, 5, resp)
        assert (len(want) > 0) == hits
        assert_contacts_equal(got, want)
    g.close()


def test_capsule_through_voxel_centres_takes_the_degenerate_branch(ctx):
    """identity transform, a capsule along a row of voxel centres: those voxels' centres lie ON the segment (distance 0), the
    normal comes from the segment's orthogonal vector"""
    o, g = both(ctx, scenes.box_scene((20.0, 14.0, 18.0)), 1.0)
    occ = o.info()["occupied_voxel_ranges"]
    i0, j1, k0 = occ[0][0], occ[1][1] - 1, occ[2][0]
    a = np.array([i0 + 2.5, j1 + 0.5, k0 + 4.5], np.float32)  # centres of the top layer
    v = np.array([10.0, 0.0, 0.0], np.float32)
    q, t = np.array([0, 0, 0, 1], np.float32), np.zeros(3, np.float32)
    want = oracle_capsule_contact_list(o, q, t, a, v, 1.25, 3, 4, 1, 0, (0.0, 0.5, 0.5))
    got = g.capsule_contacts(q, t, a, v, 1.25, 3, 4, 1, 0, (0.0, 0.5, 0.5))
    on_segment = [c for c in want if abs(c["normal"][0]) < 1e-6 and abs(c["normal"][1]) < 1e-6 and abs(abs(c["normal"][2]) - 1.0) < 1e-6]
    assert len(on_segment) >= 5
    assert_contacts_equal(got, want)
    g.close()


@pytest.mark.parametrize("seed", pu.fuzz_seeds([51, 52, 53, 54]))
def test_random_collidables_against_random_bodies(ctx, seed):
    """random SDF bodies (tests/test_gpu_random_sdf.py's trees) under a random rigid transform, hit by random spheres, planes and
    capsules around their surface: the same contacts in the same order with the same ids, geometry bit for bit"""
    from impact_amd.sdf_graph import SDFGraph
    from impact_amd.voxel import SDFVoxelGenerator
    from test_gpu_random_sdf import random_tree

    rng = np.random.default_rng(seed)
    gr = SDFGraph()
    random_tree(gr, rng, int(rng.integers(1, 4)))
    extent = [1.0, 0.5, 0.25][seed % 3]
    if min(SDFVoxelGenerator(extent, gr, 0).chunk_counts()) == 0:
        return
    o, g = both(ctx, gr, extent)
    info = o.info()
    lo = np.array([a for a, _ in info["occupied_voxel_ranges"]], dtype=np.float64) * extent
    hi = np.array([b for _, b in info["occupied_voxel_ranges"]], dtype=np.float64) * extent
    if np.any(hi <= lo):
        g.close()
        return
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = float(rng.uniform(0, 3.1))
    q = np.array([*(axis * np.sin(0.5 * ang)), np.cos(0.5 * ang)], dtype=np.float32)
    t = rng.uniform(-5.0, 5.0, 3).astype(np.float32)
    resp = (float(rng.uniform(0, 1)), float(rng.uniform(0, 1)), float(rng.uniform(0, 1)))

    def to_world(p_obj):
        x, y, z, w = [float(a) for a in q]
        b = np.array([-x, -y, -z])
        v = np.asarray(p_obj, dtype=np.float64) - t.astype(np.float64)
        return v * (w * w - b @ b) + b * (2 * (v @ b)) + np.cross(b, v) * (2 * w)

    n_hits = 0
    for _ in range(6):
        p = rng.uniform(lo - 2.0 * extent, hi + 2.0 * extent)
        kind = int(rng.integers(0, 3))
        if kind == 0:
            r = float(rng.uniform(0.5, 6.0) * extent)
            c = to_world(p).astype(np.float32)
            want = oracle_contact_list(o, q, t, c, r, 7, 99, 0, 1, resp)
            got = g.sphere_contacts(q, t, c, r, 7, 99, 0, 1, resp)
        elif kind == 1:
            n = rng.normal(size=3)
            n = (n / np.linalg.norm(n)).astype(np.float32)
            disp = float(np.dot(n.astype(np.float64), to_world(p)))
            want = oracle_plane_contact_list(o, q, t, n, disp, 5, 9, 0, 0x80000000, resp)
            got = g.plane_contacts(q, t, n, disp, 5, 9, 0, 0x80000000, resp)
        else:
            p2 = p + rng.normal(0, 6.0 * extent, 3)
            a_w = to_world(p).astype(np.float32)
            v_w = (to_world(p2) - to_world(p)).astype(np.float32)
            r = float(rng.uniform(0.5, 3.0) * extent)
            want = oracle_capsule_contact_list(o, q, t, a_w, v_w, r, 31, 4242, 2, 5, resp)
            got = g.capsule_contacts(q, t, a_w, v_w, r, 31, 4242, 2, 5, resp)
        assert_contacts_equal(got, want)
        n_hits += len(want) > 0
    g.close()


def test_many_objects_against_a_collidable_each(ctx):
    """`ivx_voxel_object_contacts_many`: several bodies, each against its own sphere, plane or capsule — one object's box misses, one has
    no contacts at all —: object by object the very list of the single-object call (same order, ids, flags, geometry bit for bit)"""
    from impact_amd import many

    pairs = [both(ctx, scenes.sphere_scene(12.0 + 3.0 * k), 1.0) for k in range(4)] + [both(ctx, scenes.box_scene((20.0, 14.0, 18.0)), 0.5),
                                                                                   both(ctx, scenes.asteroid_scene(0.25), 1.0)]
    oracles, bodies = [p[0] for p in pairs], [p[1] for p in pairs]
    rng = np.random.default_rng(5)
    q = many.collidable_queries(len(bodies))
    want, o_want = [], []  # the single-object calls' lists and the ORACLE's (the batched form shares its device code with the former)
    for i, g in enumerate(bodies):
        occ = np.array(g.update_occupied_voxel_ranges(), dtype=np.float64) * g.voxel_extent
        lo, hi = occ[:, 0], occ[:, 1]
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ang = float(rng.uniform(0, 1.0))
        rot = np.array([*(axis * np.sin(0.5 * ang)), np.cos(0.5 * ang)], dtype=np.float32)
        t = rng.uniform(-1.0, 1.0, 3).astype(np.float32)
        resp = (0.1 * i, 0.5, 0.4)
        q[i]["rotation_xyzw"], q[i]["translation"], q[i]["response"] = rot, t, resp
        q[i]["collidable_id_a"], q[i]["collidable_id_b"], q[i]["body_a"], q[i]["body_b"] = 7 + i, 99, i, 0x80000000
        kind = i % 3
        centre = 0.5 * (lo + hi)
        top = centre.copy()
        top[1] = hi[1] if i != 3 else hi[1] + 500.0  # (object 3: a sphere far away — nothing touched)
        q[i]["mode"] = kind
        if kind == 0:
            q[i]["shape3"], q[i]["shape1"] = top.astype(np.float32), 4.0 * g.voxel_extent
            want.append(g.sphere_contacts(rot, t, q[i]["shape3"], float(q[i]["shape1"]), 7 + i, 99, i, 0x80000000, resp))
            o_want.append(oracle_contact_list(oracles[i], rot, t, q[i]["shape3"], float(q[i]["shape1"]), 7 + i, 99, i, 0x80000000, resp))
        elif kind == 1:
            n = np.array([0.05, 1.0, 0.02])
            n = (n / np.linalg.norm(n)).astype(np.float32)
            q[i]["shape3"], q[i]["shape1"] = n, float(lo[1] + 2.0 * g.voxel_extent)
            want.append(g.plane_contacts(rot, t, n, float(q[i]["shape1"]), 7 + i, 99, i, 0x80000000, resp))
            o_want.append(oracle_plane_contact_list(oracles[i], rot, t, n, float(q[i]["shape1"]), 7 + i, 99, i, 0x80000000, resp))
        else:
            q[i]["shape3"], q[i]["shape3b"], q[i]["shape1"] = top.astype(np.float32), np.array([3.0, 1.0, -2.0], dtype=np.float32), 3.0 * g.voxel_extent
            want.append(g.capsule_contacts(rot, t, q[i]["shape3"], q[i]["shape3b"], float(q[i]["shape1"]), 7 + i, 99, i, 0x80000000, resp))
            o_want.append(oracle_capsule_contact_list(oracles[i], rot, t, q[i]["shape3"], q[i]["shape3b"], float(q[i]["shape1"]), 7 + i, 99, i, 0x80000000, resp))
    got, off = many.voxel_object_contacts_many(bodies, q)
    assert int(off[-1]) == sum(len(w) for w in want) and len(want[3]) == 0 and sum(len(w) for w in want) > 50
    for i, w in enumerate(want):
        assert_contacts_equal(got[off[i]:off[i + 1]], w)
        assert_contacts_equal(got[off[i]:off[i + 1]], o_want[i])
    # one object against several collidables in one call (the reference's collision pass visits every collidable near an object): objects 0 and
    # 1 twice more each, with the other's kind of collidable swapped in — every query its own list, the oracle's
    idx = [0, 1, 0, 1, 4]
    q2 = q[idx].copy()
    lo0 = float(np.array(bodies[0].update_occupied_voxel_ranges(), dtype=np.float64)[1, 0] * bodies[0].voxel_extent)
    q2[2]["mode"], q2[2]["shape3"], q2[2]["shape1"] = q[1]["mode"], q[1]["shape3"], lo0 + 2.0 * bodies[0].voxel_extent  # the plane, two voxels into body 0
    q2[3]["mode"], q2[3]["shape3"], q2[3]["shape1"] = q[0]["mode"], q[0]["shape3"], q[0]["shape1"]  # body 0's sphere against body 1
    got2, off2 = many.voxel_object_contacts_many([bodies[k] for k in idx], q2)
    lists2 = [o_want[0], o_want[1],
              oracle_plane_contact_list(oracles[0], q2[2]["rotation_xyzw"], q2[2]["translation"], q2[2]["shape3"], float(q2[2]["shape1"]), 7, 99, 0, 0x80000000,
                                        tuple(float(x) for x in q2[2]["response"])),
              oracle_contact_list(oracles[1], q2[3]["rotation_xyzw"], q2[3]["translation"], q2[3]["shape3"], float(q2[3]["shape1"]), 8, 99, 1, 0x80000000,
                                  tuple(float(x) for x in q2[3]["response"])),
              o_want[4]]
    assert int(off2[-1]) == sum(len(w) for w in lists2) and len(lists2[2]) > 0
    for i, w in enumerate(lists2):
        assert_contacts_equal(got2[off2[i]:off2[i + 1]], w)
    # too small a capacity: the error, and the sizes it would have taken
    with pytest.raises(Exception):
        many.voxel_object_contacts_many(bodies, q, capacity=8)
    # empty list
    got0, off0 = many.voxel_object_contacts_many([], many.collidable_queries(0))
    assert len(got0) == 0 and list(off0) == [0]
    for g in bodies:
        g.close()
