"""`ivx_cw_collide_frame` on the device (impact_amd/csrc/narrow.hip k_cw_rows, voxel_collision_api.hip): the whole collision pass of a frame in one
call, against the path the library had before it — `ivx_cw_collide`, the world and the bodies downloaded, tests/frame_ref.py's dispatch on the host,
the two `_many` generators, frame_ref's merge — and against the oracle's generators. Every comparison is of bytes; the only tolerance in this file is
`physics_util.RTOL` on the bodies of the falling scene, inside `test_gpu_frame.assert_frames_agree`."""
import ctypes as C

import numpy as np
import pytest

import frame_ref as fr
import narrow_ref as nr
import test_gpu_frame as tg
import test_gpu_narrow as tn
from impact_amd import capi, collision, scenes
from impact_amd.voxel import Context

pytestmark = pytest.mark.gpu

S, P, CAP, V = nr.SPHERE, nr.PLANE, nr.CAPSULE, nr.VOXEL
DT = 0.004


def attach(cw, voxel_bodies, only=None):
    cw.set_voxel_objects({i: (vb.g, vb.origin_offset, vb.center_of_mass) for i, vb in voxel_bodies.items() if only is None or i in only})


def device_objects(ctx, voxel_bodies):
    for vb in voxel_bodies.values():
        vb.g = tg.device_object(ctx, vb)


def close_objects(voxel_bodies):
    for vb in voxel_bodies.values():
        if vb.g is not None:
            vb.g.close()
            vb.g = None


def old_path(w, cw, local, voxel_bodies, mode, want=None):
    """what a caller had to do before: collide, download the world and the bodies, dispatch on the host, the two `_many` calls, merge. `want`: the
    contacts and deferred pairs of narrow_ref the device must return -> dict of every intermediate"""
    world = cw.download()
    bodies = w.bodies()
    contacts, deferred = cw.collide(mode)
    if want is not None:
        tn.assert_records_equal(contacts, want[0], "contacts")
        assert deferred.tobytes() == want[1].tobytes()
    rows, mutual = fr.dispatch(world, deferred, bodies, voxel_bodies)
    manifolds = fr.device_manifolds(rows, mutual, voxel_bodies, len(deferred))
    return {"world": world, "bodies": bodies, "contacts": contacts, "deferred": deferred, "rows": rows, "mutual": mutual, "manifolds": manifolds,
            "merged": fr.merge(contacts, manifolds)}


def check_frame(cw, old, voxel_bodies, mode, oracle=True):
    """`collide_frame` against the old path's results: counts, deferred list, primitive part, rows, offsets, merged list, every manifold against the
    oracle generator fed the same rows; and two calls leave the same bytes -> (merged, rows)"""
    merged, n_primitive, deferred, offsets = cw.collide_frame(mode)
    rows = cw.rows()
    nd = len(old["deferred"])
    assert n_primitive == len(old["contacts"]) and deferred.shape == (nd, 2) and deferred.tobytes() == old["deferred"].tobytes()
    tn.assert_records_equal(merged[:n_primitive], old["contacts"], "the primitive part")
    # the rows: frame_ref.dispatch over the downloaded world and bodies
    cq, c_source, mq, m_source = collision.row_queries(rows)
    assert len(rows) == nd and c_source.tolist() == old["rows"].source and m_source.tolist() == old["mutual"].source
    assert cq.tobytes() == old["rows"].queries.tobytes() and mq.tobytes() == old["mutual"].queries.tobytes()
    assert rows["voxel"][c_source].tolist() == old["rows"].objects
    assert list(zip(rows["voxel"][m_source].tolist(), rows["other"][m_source].tolist())) == old["mutual"].objects
    # the list: primitive contacts, then the manifolds in deferred-list order
    lengths = [len(m) for m in old["manifolds"]]
    assert offsets.tolist() == np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64).tolist()
    tn.assert_records_equal(merged, old["merged"], "the merged list")
    if oracle:
        want = fr.oracle_manifolds(old["rows"], old["mutual"], voxel_bodies, nd)
        for i, m in enumerate(want):
            fr.assert_contacts_equal(merged[n_primitive + offsets[i]:n_primitive + offsets[i + 1]], m)
            assert len(m) == 0 or int(m["flags"][0]) == capi.CONTACT_MANIFOLD_START
    again = cw.collide_frame(mode, capacity=len(merged) + 3, deferred_capacity=nd + 2)
    assert again[0].tobytes() == merged.tobytes() and again[1] == n_primitive and again[2].tobytes() == deferred.tobytes() and again[3].tolist() == offsets.tolist()
    assert cw.rows().tobytes() == rows.tobytes()
    assert nd == 0 or (cw.device_ptr(capi.CW_PTR_VOXEL_ROWS) and cw.device_ptr(capi.CW_PTR_FRAME_CONTACTS))
    return merged, rows


@pytest.fixture(scope="module")
def static_world(ctx):
    """fr.static_scene with its three voxel objects on the device, attached to a synchronized world"""
    local, dyn, kin, voxel_bodies = fr.static_scene()
    device_objects(ctx, voxel_bodies)
    w, cw = tn.make_world(ctx, local, dyn, kin)
    attach(cw, voxel_bodies)
    yield w, cw, local, voxel_bodies
    w.close()
    close_objects(voxel_bodies)


def reference_of_static_world(static_world, mode):
    w, cw, local, voxel_bodies = static_world
    world, boxes = tn.check_synchronized(w, cw, local, cw.synchronize())
    want = nr.collide(world, nr.broad_phase_pairs(boxes, local["kind"], mode))
    return old_path(w, cw, local, voxel_bodies, mode, want)


@pytest.mark.parametrize("broad_phase", [capi.CW_BROAD_FLAT, capi.CW_BROAD_HIERARCHY])
@pytest.mark.parametrize("mode", tn.MODES)
def test_static_scene_in_both_modes(static_world, mode, broad_phase):
    w, cw, local, voxel_bodies = static_world
    cw.set_broad_phase(broad_phase)
    try:
        old = reference_of_static_world(static_world, mode)
        generators = fr.generator_of(old["rows"], old["mutual"], len(old["deferred"]))
        assert {g for g, m in zip(generators, old["manifolds"]) if len(m) > 0} == set(fr.GENERATORS) and any(len(m) == 0 for m in old["manifolds"])
        assert len(old["contacts"]) > 0  # (primitive contacts in front of the manifolds)
        check_frame(cw, old, voxel_bodies, mode)
    finally:
        cw.set_broad_phase(capi.CW_BROAD_FLAT)


# ---- edges of the row kernel and of the merged phase -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_sphere(ctx):
    vb = fr.voxel_body(scenes.sphere_scene(12.0), 0.5)  # (the small_sphere of test_frame_cpu.py)
    vb.g = tg.device_object(ctx, vb)
    yield vb
    close_objects({0: vb})


CENTRE = np.array([3.0, -2.0, 1.5])


def sphere_scene_with(vb, points, radius, kind):
    """the voxel sphere (collidable 0) on a turned dynamic body, spheres of one radius at the given world points on a second body at the identity"""
    dyn = np.array([fr.rigid_body_of(vb, CENTRE, fr.axis_angle((0.3, -1.0, 0.5), 0.9)), nr.unit_body((0, 0, 0))], dtype=capi.RIGID_BODY_DTYPE)
    local = [fr.voxel_collidable(vb.o, vb.origin_offset, 0, 1000, response=(0.2, 0.6, 0.4))]
    local += [collision.sphere(p, radius, 1, 2000 + k, kind, response=(0.3, 0.5, 0.5)) for k, p in enumerate(points)]
    return np.array(local, dtype=capi.COLLIDABLE_DTYPE), dyn, fr.static_kinematic(), {0: vb}


def directions(k):
    """k directions spread over the sphere (a golden-angle spiral)"""
    i = np.arange(k) + 0.5
    z, phi = 1.0 - 2.0 * i / max(k, 1), i * np.pi * (3.0 - np.sqrt(5.0))
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def run_scene(ctx, local, dyn, kin, voxel_bodies, mode, n_deferred=None, n_primitive=None, oracle=True):
    w, cw = tn.make_world(ctx, local, dyn, kin)
    try:
        attach(cw, voxel_bodies)
        world, boxes = tn.check_synchronized(w, cw, local, cw.synchronize())
        want = nr.collide(world, nr.broad_phase_pairs(boxes, local["kind"], mode))
        # on narrow_ref's result, before the device is asked
        assert n_deferred is None or len(want[1]) == n_deferred, (len(want[1]), n_deferred)
        assert n_primitive is None or len(want[0]) == n_primitive, (len(want[0]), n_primitive)
        old = old_path(w, cw, local, voxel_bodies, mode, want)
        merged, rows = check_frame(cw, old, voxel_bodies, mode, oracle)
        return old, merged, rows
    finally:
        w.close()


@pytest.mark.parametrize("k", [0, 1, 63, 64, 65, 257])
def test_k_static_spheres_on_a_voxel_sphere(ctx, small_sphere, k):
    """K STATIC spheres of about a voxel's radius on the surface of the voxel sphere, in the mode that forms no static-static pair: exactly K deferred
    pairs and no primitive contact — none, one, one below / at / above a wave, and more than a workgroup of k_cw_rows (and, at 257 after 0, more rows
    than came with the counts)"""
    vb = small_sphere
    half = 0.5 * float(np.max(fr.model_aabb(vb.o)["upper"] - fr.model_aabb(vb.o)["lower"]))
    points = CENTRE + directions(k) * half
    local, dyn, kin, voxel_bodies = sphere_scene_with(vb, points, vb.extent, capi.BV_STATIC)
    old, merged, rows = run_scene(ctx, local, dyn, kin, voxel_bodies, capi.BV_DYNAMIC_PAIRS, n_deferred=k, n_primitive=0)
    assert (rows["generator"] == 0).all() and (rows["voxel"] == 0).all()
    assert k == 0 or sum(len(m) > 0 for m in old["manifolds"]) >= max(1, k // 2)  # (most of the spheres touch the surface)


def test_a_contact_buffer_that_grows_keeps_the_primitive_contacts(ctx, small_sphere):
    """257 spheres on the voxel sphere and three dynamic spheres overlapping each other far away: the world's contact buffer, sized by the pair count
    (at least 1 024 contacts), has to grow for the manifolds behind the three primitive contacts k_cw_emit wrote into it"""
    vb = small_sphere
    half = 0.5 * float(np.max(fr.model_aabb(vb.o)["upper"] - fr.model_aabb(vb.o)["lower"]))
    local, dyn, kin, voxel_bodies = sphere_scene_with(vb, CENTRE + directions(257) * half, vb.extent, capi.BV_STATIC)
    far = [collision.sphere(CENTRE + (100.0 + 0.4 * k, 0.0, 0.0), 0.5, 1, 5000 + k, response=(0.3, 0.5, 0.5)) for k in range(3)]
    local = np.concatenate([local, np.array(far, dtype=capi.COLLIDABLE_DTYPE)])
    old, merged, rows = run_scene(ctx, local, dyn, kin, voxel_bodies, capi.BV_DYNAMIC_PAIRS, n_deferred=257, n_primitive=3, oracle=False)
    assert len(merged) > 1024 + 3


def test_deferred_pairs_whose_manifolds_are_all_empty(ctx, small_sphere):
    """eight small spheres inside the voxel sphere's world box and outside the object: deferred pairs, no contact at all"""
    vb = small_sphere
    half = 0.5 * float(np.max(fr.model_aabb(vb.o)["upper"] - fr.model_aabb(vb.o)["lower"]))
    corners = np.array([[(-1.0, 1.0)[(c >> d) & 1] for d in range(3)] for c in range(8)])
    local, dyn, kin, voxel_bodies = sphere_scene_with(vb, CENTRE + corners * 0.9 * half, 0.2, capi.BV_DYNAMIC)
    old, merged, rows = run_scene(ctx, local, dyn, kin, voxel_bodies, capi.BV_DYNAMIC_PAIRS, n_deferred=8, n_primitive=0)
    assert len(merged) == 0 and all(len(m) == 0 for m in old["manifolds"])


def test_a_scene_without_voxel_collidables_equals_collide(ctx):
    local, dyn, kin = nr.scene(300)
    local = local[local["shape"] != V]
    assert (local["shape"][-3:] == P).all()
    for mode in tn.MODES:
        old, merged, rows = run_scene(ctx, local, dyn, kin, {}, mode, n_deferred=0)
        assert len(merged) == len(old["contacts"]) > 64 and len(rows) == 0


def test_two_voxel_objects_only(static_world, ctx):
    """the sphere and the box of the static scene alone: one deferred pair, a mutual row, a non-empty manifold"""
    _, _, local, voxel_bodies = static_world
    _, dyn, kin, _ = fr.static_scene()
    index = sorted(voxel_bodies)[:2]
    pair = {k: voxel_bodies[i] for k, i in enumerate(index)}
    old, merged, rows = run_scene(ctx, local[index], dyn, kin, pair, capi.BV_ALL_PAIRS, n_deferred=1, n_primitive=0)
    assert rows["generator"].tolist() == [capi.CW_ROW_MUTUAL] and (int(rows["voxel"][0]), int(rows["other"][0])) == (0, 1) and len(merged) > 0


# ---- behind an enqueued step ---------------------------------------------------------------------------------------------------------------------
def test_behind_an_enqueued_step(static_world, ctx):
    """step_enqueue, synchronize, collide_frame with no wait between: rows and list equal those of a second world that stepped, waited, and went the
    old path"""
    _, _, local, voxel_bodies = static_world
    _, dyn, kin, _ = fr.static_scene()
    rng = np.random.default_rng(3)
    dyn = dyn.copy()
    dyn["momentum"] = rng.uniform(-2.0, 2.0, (len(dyn), 3)) * dyn["mass"][:, None]
    dyn["angular_momentum"][3:] = rng.uniform(-0.5, 0.5, (len(dyn) - 3, 3))
    w, cw = tn.make_world(ctx, local, dyn, kin)
    try:
        attach(cw, voxel_bodies)
        cw.synchronize()
        unstepped = cw.collide_frame(capi.BV_DYNAMIC_PAIRS)[0], cw.rows()
        w.step_enqueue(0.05)
        cw.synchronize()
        merged, n_primitive, deferred, offsets = cw.collide_frame(capi.BV_DYNAMIC_PAIRS)
        rows = cw.rows()
        stepped = w.bodies()[0]
    finally:
        w.close()
    assert np.abs(stepped["position"] - dyn["position"]).max() > 0.05 and rows.tobytes() != unstepped[1].tobytes()
    w, cw = tn.make_world(ctx, local, dyn, kin)
    try:
        w.step_enqueue(0.05)
        assert w.bodies()[0].tobytes() == stepped.tobytes()  # (waits)
        cw.synchronize()
        old = old_path(w, cw, local, voxel_bodies, capi.BV_DYNAMIC_PAIRS)
    finally:
        w.close()
    assert len(old["deferred"]) >= 5 and sum(len(m) for m in old["manifolds"]) > 0
    assert deferred.tobytes() == old["deferred"].tobytes() and n_primitive == len(old["contacts"])
    cq, c_source, mq, m_source = collision.row_queries(rows)
    assert cq.tobytes() == old["rows"].queries.tobytes() and mq.tobytes() == old["mutual"].queries.tobytes()
    assert c_source.tolist() == old["rows"].source and m_source.tolist() == old["mutual"].source
    tn.assert_records_equal(merged, old["merged"], "the merged list behind an enqueued step")


# ---- frames ----------------------------------------------------------------------------------------------------------------------------------------
class FrameSide(tg.DeviceSide):
    """test_gpu_frame.DeviceSide with its frame replaced: synchronize -> collide_frame -> prepare_constraints -> step"""

    def __init__(self, ctx, oracle_side):
        super().__init__(ctx, oracle_side)
        self.attach()

    def attach(self):
        self.cw.set_voxel_objects({i: (b.g, b.origin_offset, b.center_of_mass) for i, b in self.voxel_bodies.items()})

    def frame(self, enqueue=False):
        bv_set = self.cw.synchronize() if self.synchronized is None else self.synchronized
        self.synchronized = None
        merged, n_primitive, deferred, offsets = self.cw.collide_frame(capi.BV_DYNAMIC_PAIRS)  # (behind an enqueued step: nothing has waited since)
        generators = [fr.GENERATORS[int(g)] for g in self.cw.rows()["generator"]]
        manifolds = [merged[n_primitive + offsets[i]:n_primitive + offsets[i + 1]] for i in range(len(deferred))]
        boxes = bv_set.download()[0]
        assert self.w.prepare_constraints(merged) == len(merged)
        if enqueue:
            self.w.step_enqueue(fr.DT)
            self.synchronized = self.cw.synchronize()
        else:
            self.w.step(fr.DT)
        f = {"deferred": deferred, "generators": generators, "manifolds": manifolds, "merged": merged, "contacts": merged[:n_primitive], "boxes": boxes}
        return fr.frame_record(f, self.w.bodies()[0])

    def bite(self, oracle_edit):
        got = super().bite(oracle_edit)  # (sets the collidables again: what was attached went with the old set)
        self.attach()
        return got


def test_frames_across_an_edit(ctx):
    """the run of test_gpu_frame.py — 60 frames of the falling scene, one of them enqueued, the bite, 15 frames more — with every frame's collision
    pass made by the one call; after the bite the objects are attached again with the new origin offset and centre of mass"""
    run = fr.oracle_run()
    records, edit = run["records"], run["edit"]
    side = FrameSide(ctx, run["side"])
    try:
        tg.run_frames(side, records, 0, fr.N_FRAMES, enqueue_at=33)
        got = side.bite(edit)
        np.testing.assert_allclose(got["new_offset"], edit["new_offset"], rtol=1e-5, atol=1e-5)
        tg.run_frames(side, records, fr.N_FRAMES, fr.N_FRAMES_AFTER_EDIT)
    finally:
        side.close()


# ---- errors and capacities -------------------------------------------------------------------------------------------------------------------------
def raw_frame(w, mode, contacts, cap, deferred, offsets, deferred_cap):
    n, n_primitive, m = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    rc = capi.lib().ivx_cw_collide_frame(w.h, mode, capi.ptr(contacts) if contacts is not None else None, cap, C.byref(n), C.byref(n_primitive),
                                         capi.ptr(deferred) if deferred is not None else None, capi.ptr(offsets) if offsets is not None else None, deferred_cap, C.byref(m))
    return rc, n.value, n_primitive.value, m.value


def test_errors_and_capacities(static_world, ctx):
    w, cw, local, voxel_bodies = static_world
    lib, mode = capi.lib(), capi.BV_ALL_PAIRS
    old = reference_of_static_world(static_world, mode)
    want, rows = check_frame(cw, old, voxel_bodies, mode, oracle=False)
    n_total, n_primitive, nd = len(want), len(old["contacts"]), len(old["deferred"])
    assert n_primitive > 0 and nd > 0 and n_total > n_primitive

    def good_call_gives_the_same_bytes():
        merged, n_prim, deferred, offsets = cw.collide_frame(mode)
        assert merged.tobytes() == want.tobytes() and n_prim == n_primitive and deferred.tobytes() == old["deferred"].tobytes()
        assert cw.rows().tobytes() == rows.tobytes()

    # one short: IVX_ERR_CAPACITY, the numbers found, nothing written
    contacts = np.full(n_total, 0xA5, dtype=np.uint8).repeat(64).view(capi.CONTACT_DTYPE)
    deferred, offsets = np.full((nd, 2), 0xA5A5A5A5, dtype=np.uint32), np.full(nd + 1, 0xA5A5A5A5, dtype=np.uint32)
    for cap, dcap in ((n_total - 1, nd), (n_total, nd - 1), (n_primitive - 1, nd)):
        assert raw_frame(w, mode, contacts, cap, deferred, offsets, dcap) == (capi.IVX_ERR_CAPACITY, n_total, n_primitive, nd)
        assert np.all(contacts.view(np.uint8) == 0xA5) and np.all(deferred == 0xA5A5A5A5) and np.all(offsets == 0xA5A5A5A5)
        good_call_gives_the_same_bytes()
    # the lists may stay on the device only
    assert raw_frame(w, mode, None, 0, None, None, 0) == (capi.IVX_OK, n_total, n_primitive, nd)
    # inside a bracket of the recorder
    capi.check(lib.ivx_many_begin(ctx.h))
    try:
        assert raw_frame(w, mode, None, 0, None, None, 0)[0] == capi.IVX_ERR_STATE
    finally:
        capi.check(lib.ivx_many_flush(ctx.h))
    good_call_gives_the_same_bytes()
    # a voxel collidable a deferred pair names has no object
    first = sorted(voxel_bodies)[0]
    attach(cw, voxel_bodies, only=set(voxel_bodies) - {first})
    assert raw_frame(w, mode, None, 0, None, None, 0)[0] == capi.IVX_ERR_STATE
    # refused attachments leave the set as it was (still one short): an index past the set, a shape that is no voxel object, a null grid, the same
    # index twice, a grid of another context
    g = voxel_bodies[first].g
    record = collision.voxel_object_record(g, voxel_bodies[first].origin_offset, voxel_bodies[first].center_of_mass)
    primitive = int(np.nonzero(local["shape"] != V)[0][0])

    def refused(index, records):
        index, records = np.array(index, dtype=np.uint32), np.array(records, dtype=capi.CW_VOXEL_OBJECT_DTYPE).reshape(-1)
        return lib.ivx_cw_set_voxel_objects(w.h, capi.ptr(index), capi.ptr(records), len(index))

    assert refused([len(local)], [record]) == capi.IVX_ERR_INVALID and refused([primitive], [record]) == capi.IVX_ERR_INVALID
    assert refused([first], [collision.voxel_object_record(None, (0, 0, 0), (0, 0, 0))]) == capi.IVX_ERR_INVALID
    assert refused([first, first], [record, record]) == capi.IVX_ERR_INVALID
    other = Context(0)
    try:
        foreign = tg.pu.gpu_from_graph(other, scenes.box_scene((8.0, 8.0, 8.0)), 1.0)
        assert refused([first], [collision.voxel_object_record(foreign, (0, 0, 0), (0, 0, 0))]) == capi.IVX_ERR_INVALID
        foreign.close()
    finally:
        other.close()
    assert raw_frame(w, mode, None, 0, None, None, 0)[0] == capi.IVX_ERR_STATE
    attach(cw, voxel_bodies)
    good_call_gives_the_same_bytes()
    # stale probes on a voxel-voxel pair: the mesh made again, the probes not yet
    a, b = old["mutual"].objects[0]
    stale = voxel_bodies[a].g
    stale.mesh.recreate()
    assert raw_frame(w, mode, None, 0, None, None, 0)[0] == capi.IVX_ERR_STATE
    assert b"probes" in lib.ivx_last_error()
    tg.assert_probes_equal(stale, voxel_bodies[a], stale.collision_probes_recompute())
    good_call_gives_the_same_bytes()
    # set_collidables drops what was attached; before synchronize
    cw.set_collidables(local)
    assert raw_frame(w, mode, None, 0, None, None, 0)[0] == capi.IVX_ERR_STATE and b"synchronize" in lib.ivx_last_error()
    cw.synchronize()
    assert raw_frame(w, mode, None, 0, None, None, 0)[0] == capi.IVX_ERR_STATE and b"attached" in lib.ivx_last_error()
    attach(cw, voxel_bodies)
    good_call_gives_the_same_bytes()
