"""Primitive collidables on the device (impact_amd/csrc/narrow.hip). The world-space collidables are byte-equal to the library's host function over
the bodies the world holds; every other expectation is the float32 restatement of narrow_ref.py over the DOWNLOADED world collidables and
bvol_ref.py's pairs over the downloaded boxes, and contacts and deferred pairs must equal it in content and order — no tolerance anywhere in this
file (the end-to-end test's comparison of the bodies with the oracle world is the one test_gpu_physics.py makes).

The narrow phase runs a lane per pair in workgroups of 256 and scans its per-wave counts in rounds of 256 waves (16 384 pairs): the pair counts
below sit one below, at and one above a wave, a workgroup and a round."""
import ctypes as C

import numpy as np
import pytest

import bvol_ref as br
import narrow_ref as nr
import physics_util as phu
from impact_amd import bvol, capi, collision, scenes
from impact_amd.physics import PhysicsWorld

pytestmark = pytest.mark.gpu

WAVE, GROUP, SCAN_ROUND_PAIRS = 64, 256, 256 * 64
PAIR_COUNTS = [1, WAVE - 1, WAVE, WAVE + 1, GROUP - 1, GROUP, GROUP + 1, SCAN_ROUND_PAIRS - 1, SCAN_ROUND_PAIRS, SCAN_ROUND_PAIRS + 1]
MODES = [capi.BV_ALL_PAIRS, capi.BV_DYNAMIC_PAIRS]


def make_world(ctx, local, dyn, kin):
    w = PhysicsWorld(ctx)
    w.set_bodies(dyn, kin)
    cw = collision.CollisionWorld(w)
    cw.set_collidables(local)
    return w, cw


def assert_records_equal(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero(got != want)[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} records differ, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}")


def check_synchronized(w, cw, local, bv_set):
    """the downloaded world collidables and world boxes against ivx_cw_transform over the bodies the world holds -> (world collidables, boxes)"""
    world = cw.download()
    boxes, _ = bv_set.download()
    dyn, kin = w.bodies()
    positions, orientations = nr.body_frames(local, dyn, kin)
    want_world, want_boxes = np.zeros_like(world), np.zeros_like(boxes)
    for i in range(len(local)):
        want_world[i], want_boxes[i] = collision.transform(local[i], positions[i], orientations[i])
    assert_records_equal(world, want_world, "world collidables")
    assert_records_equal(boxes, want_boxes, "world boxes")
    return world, boxes


def check_collide(cw, local, world, boxes, mode, want_pairs=None):
    pairs = nr.broad_phase_pairs(boxes, local["kind"], mode)
    assert want_pairs is None or len(pairs) == want_pairs, (len(pairs), want_pairs)
    want_contacts, want_deferred = nr.collide(world, pairs)
    got_contacts, got_deferred = cw.collide(mode, capacity=len(want_contacts), deferred_capacity=len(want_deferred))
    assert_records_equal(got_contacts, want_contacts, f"contacts, mode {mode}")
    assert got_deferred.tobytes() == want_deferred.tobytes() and got_deferred.shape == want_deferred.shape, f"deferred pairs, mode {mode}"
    return want_contacts, want_deferred


def check_scene(ctx, local, dyn, kin, modes=MODES, want_pairs=None):
    w, cw = make_world(ctx, local, dyn, kin)
    try:
        world, boxes = check_synchronized(w, cw, local, cw.synchronize())
        return [check_collide(cw, local, world, boxes, mode, want_pairs) for mode in modes]
    finally:
        w.close()


@pytest.mark.parametrize("n", [0, 1, 2, 70, 700])
def test_seeded_scene(ctx, n):
    """narrow_ref.scene(n): spheres, capsules, voxel-object boxes, three planes last, a fifth of the bodies kinematic, both modes"""
    local, dyn, kin = nr.scene(n)
    results = check_scene(ctx, local, dyn, kin)
    if n >= 70:
        for mode, (contacts, deferred) in zip(MODES, results):
            n_pairs = len(nr.scene_reference(n, mode)[2])
            assert 0.25 <= len(contacts) / n_pairs <= 0.75 and len(deferred) > 0  # (the reference side: most waves hold hits and misses)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("target", PAIR_COUNTS)
def test_pair_counts_around_a_wave_a_workgroup_and_a_scan_round(ctx, target, mode):
    n, fillers = nr.scene_with_pair_count(target, mode)
    local, dyn, kin = nr.scene(n, 7, 1, fillers)
    (contacts, deferred), = check_scene(ctx, local, dyn, kin, [mode], want_pairs=target)
    assert target < WAVE or 0.25 <= len(contacts) / target <= 0.75


def test_no_pairs_and_pairs_that_all_miss(ctx):
    # one collidable: no pair; the counts come back zero and nothing is written
    local, dyn, kin = nr.scene(1, n_planes=0)
    w, cw = make_world(ctx, local, dyn, kin)
    cw.synchronize()
    found, deferred = C.c_size_t(7), C.c_size_t(7)
    capi.check(capi.lib().ivx_cw_collide(w.h, 0, None, 0, C.byref(found), None, 0, C.byref(deferred)))
    assert (found.value, deferred.value) == (0, 0)
    w.close()
    # 70 spheres along the diagonal: neighbours' boxes overlap, the spheres do not — 69 pairs, no contact, no emit
    n = 70
    dyn = np.array([nr.unit_body((0.8 * k, 0.8 * k, 0.8 * k)) for k in range(n)], dtype=capi.RIGID_BODY_DTYPE)
    local = np.array([collision.sphere((0, 0, 0), 0.5, k, 100 + k) for k in range(n)], dtype=capi.COLLIDABLE_DTYPE)
    (contacts, deferred), = check_scene(ctx, local, dyn, None, [capi.BV_ALL_PAIRS], want_pairs=n - 1)
    assert len(contacts) == 0 and len(deferred) == 0


def test_every_branch_as_one_scene(ctx):
    """the hand-made branch cases of the CPU test, all on one body at the origin (planes last): the device takes every branch the host takes"""
    members = [m for pair in nr.hand_made_cases().values() for m in pair]
    members = [m for m in members if m["shape"] != nr.PLANE] + [m for m in members if m["shape"] == nr.PLANE]
    local = np.array(members, dtype=capi.COLLIDABLE_DTYPE)
    local["body"], local["id"] = 0, np.arange(1, len(local) + 1)
    dyn = np.array([nr.unit_body((0, 0, 0))], dtype=capi.RIGID_BODY_DTYPE)
    (contacts, deferred), = check_scene(ctx, local, dyn, None, [capi.BV_ALL_PAIRS])
    assert len(contacts) > len(local) and len(deferred) > 0


def test_capacity_state_and_repetition(ctx):
    lib = capi.lib()
    local, dyn, kin = nr.scene(300)
    w = PhysicsWorld(ctx)
    w.set_bodies(dyn, kin)
    cw = collision.CollisionWorld(w)
    found, n_deferred = C.c_size_t(0), C.c_size_t(0)
    # IVX_ERR_STATE before the collidables are set and before they are synchronized
    assert lib.ivx_cw_synchronize(w.h) == capi.IVX_ERR_STATE
    assert lib.ivx_cw_collide(w.h, 0, None, 0, C.byref(found), None, 0, C.byref(n_deferred)) == capi.IVX_ERR_STATE
    cw.set_collidables(local)
    assert lib.ivx_cw_collide(w.h, 0, None, 0, C.byref(found), None, 0, C.byref(n_deferred)) == capi.IVX_ERR_STATE
    assert lib.ivx_cw_download(w.h, None, 0) == capi.IVX_ERR_STATE
    # refused records leave the set as it was
    bad = local.copy()
    bad["shape"][5] = 4
    assert lib.ivx_cw_set_collidables(w.h, capi.ptr(bad), len(bad)) == capi.IVX_ERR_INVALID
    bad = local.copy()
    bad["body"][5] = len(dyn)
    assert lib.ivx_cw_set_collidables(w.h, capi.ptr(bad), len(bad)) == capi.IVX_ERR_INVALID
    bad["body"][5] = len(kin) | capi.KINEMATIC_BIT
    assert lib.ivx_cw_set_collidables(w.h, capi.ptr(bad), len(bad)) == capi.IVX_ERR_INVALID
    world, boxes = check_synchronized(w, cw, local, cw.synchronize())
    want_contacts, want_deferred = check_collide(cw, local, world, boxes, capi.BV_ALL_PAIRS)
    assert len(want_contacts) > 64 and len(want_deferred) > 1
    # one short: IVX_ERR_CAPACITY, the numbers found, the buffers untouched
    contacts = np.full(len(want_contacts), 0xA5, dtype=np.uint8).repeat(64).view(capi.CONTACT_DTYPE)
    deferred = np.full((len(want_deferred), 2), 0xA5A5A5A5, dtype=np.uint32)
    for cap, dcap in ((len(want_contacts) - 1, len(want_deferred)), (len(want_contacts), len(want_deferred) - 1)):
        rc = lib.ivx_cw_collide(w.h, 0, capi.ptr(contacts), cap, C.byref(found), capi.ptr(deferred), dcap, C.byref(n_deferred))
        assert rc == capi.IVX_ERR_CAPACITY and (found.value, n_deferred.value) == (len(want_contacts), len(want_deferred))
        assert np.all(contacts.view(np.uint8) == 0xA5) and np.all(deferred == 0xA5A5A5A5)
    # two calls leave the same bytes, on the host and in the world's buffers
    first = cw.collide(0, capacity=len(want_contacts), deferred_capacity=len(want_deferred))
    second = cw.collide(0, capacity=len(want_contacts) + 9, deferred_capacity=len(want_deferred) + 9)
    assert first[0].tobytes() == second[0].tobytes() == want_contacts.tobytes() and first[1].tobytes() == second[1].tobytes() == want_deferred.tobytes()
    assert cw.device_ptr(capi.CW_PTR_WORLD_COLLIDABLES) and cw.device_ptr(capi.CW_PTR_CONTACTS) and cw.device_ptr(capi.CW_PTR_DEFERRED_PAIRS)
    # the lists may stay on the device only
    capi.check(lib.ivx_cw_collide(w.h, 1, None, 0, C.byref(found), None, 0, C.byref(n_deferred)))
    assert found.value == len(nr.scene_reference(300, 1)[3]) and n_deferred.value == len(nr.scene_reference(300, 1)[4])
    # another set of bounding volumes on the context: the world's is gone until it synchronizes again
    bvol.set_boxes(ctx, br.scene(10)[0])
    assert lib.ivx_cw_collide(w.h, 0, None, 0, C.byref(found), None, 0, C.byref(n_deferred)) == capi.IVX_ERR_STATE
    cw.synchronize()
    check_collide(cw, local, world, boxes, capi.BV_DYNAMIC_PAIRS)
    w.close()


def test_the_installed_set_answers_pairs_and_queries(ctx):
    local, dyn, kin = nr.scene(500)
    w, cw = make_world(ctx, local, dyn, kin)
    s = cw.synchronize()
    world, boxes = check_synchronized(w, cw, local, s)
    for mode in MODES:
        want = nr.broad_phase_pairs(boxes, local["kind"], mode)
        got = s.pairs(mode, capacity=len(want))
        assert got.tobytes() == want.tobytes()
    records = br.mixed_queries(500, 8)
    masks, counts = s.query(records)
    with np.errstate(over="ignore", invalid="ignore"):
        want_masks, want_counts = br.queries(boxes, records)
    assert masks.tobytes() == want_masks.tobytes() and counts.tolist() == want_counts.tolist()
    assert (counts >= 3).all()  # (the three planes are in every region)
    w.close()


def test_synchronize_behind_an_enqueued_step_sees_its_bodies(ctx):
    """ivx_world_step_enqueue followed at once by ivx_cw_synchronize, no wait between: the world collidables are the transforms of the bodies AFTER
    the step"""
    local, dyn, kin = nr.scene(400)
    rng = np.random.default_rng(3)
    dyn = dyn.copy()
    dyn["momentum"], dyn["angular_momentum"] = rng.uniform(-3, 3, (len(dyn), 3)), rng.uniform(-1, 1, (len(dyn), 3))
    w, cw = make_world(ctx, local, dyn, kin)
    before = cw.synchronize()
    world_before = cw.download()
    w.step_enqueue(0.05)
    s = cw.synchronize()
    world, boxes = check_synchronized(w, cw, local, s)  # (w.bodies() waits; the bodies it returns are the stepped ones)
    moved = w.bodies()[0]
    assert np.abs(moved["position"] - dyn["position"]).max() > 0.05 and world.tobytes() != world_before.tobytes()
    check_collide(cw, local, world, boxes, capi.BV_DYNAMIC_PAIRS)
    assert before.n == s.n
    w.close()


def test_five_frames_of_a_lattice_on_a_plane(ctx):
    """a 4 x 4 x 4 lattice of spheres, 5 % overlapping, resting on a static plane: five frames of synchronize -> collide -> set_contacts -> step. Every
    frame's contacts equal the restatement's; the bodies stay within physics_util.RTOL of the oracle world stepped with the same contacts"""
    bodies, _ = scenes.sphere_pile_scene(4)
    response = (0.4, 0.7, 0.5)
    local = np.array([collision.sphere((0, 0, 0), 0.5, k, 1000 + k, response=response) for k in range(len(bodies))] +
                     [collision.plane((0, 1, 0), -0.475, 0, 1, response=response, kinematic=True)], dtype=capi.COLLIDABLE_DTYPE)
    w, o = phu.make_pair(ctx, bodies, phu.static_plane())
    cw = collision.CollisionWorld(w)
    cw.set_collidables(local)
    for frame in range(5):
        world, boxes = check_synchronized(w, cw, local, cw.synchronize())
        contacts, deferred = check_collide(cw, local, world, boxes, capi.BV_DYNAMIC_PAIRS)
        assert len(contacts) >= 144 + 16 and len(deferred) == 0, (frame, len(contacts))  # (the lattice's 144 neighbour pairs and the 16 spheres on the plane)
        phu.step_both(w, o, contacts, 0.005)
        phu.assert_bodies_close(w.bodies()[0], o.bodies()[0], what=f"frame {frame}: ")
    w.close()
