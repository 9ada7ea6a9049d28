"""The test-side join of a whole collision frame with voxel objects among the collidables, stated once and used by both sides of every comparison:

  synchronize -> pairs -> primitive contacts + deferred voxel pairs -> voxel generators -> merged contact list -> step

`to_object_space_f32` is `VoxelObjectCollidable::new` (impact_voxel/src/collidable.rs:310-327) in the reference's operation order and precision;
`voxel_collidable` is the record a voxel body hands to the collision world (its model box seen from the body frame, whose origin is the centre of
mass); `dispatch` is the table of `generate_contact_manifold` (collidable.rs:138-215) over the deferred pairs; `merge` is the order the contacts
reach the solver in; `oracle_frame` runs all of it on the CPU over narrow_ref.py, the oracle's generators and the oracle's solver.

It also holds the oracle side of the scenes of tests/test_frame_cpu.py and tests/test_gpu_frame.py: everything a scene must satisfy is asserted on
these results, which need no GPU."""
import dataclasses
import functools

import numpy as np

import bvol_ref as br
import narrow_ref as nr
import oracle_lib as ol
import parity_util as pu
from impact_amd import bvol, capi, collision, scenes
from test_gpu_collide import oracle_contact_list as oracle_mutual_contact_list
from test_gpu_collide import world_to_object as to_object_space_f64_rounded  # (the float64 composition the three chain tests use, rounded once)
from test_gpu_contacts import assert_contacts_equal, oracle_capsule_contact_list, oracle_contact_list, oracle_plane_contact_list  # noqa: F401

f32 = np.float32
SPHERE, PLANE, CAPSULE, VOXEL = nr.SPHERE, nr.PLANE, nr.CAPSULE, nr.VOXEL
GENERATOR_OF_MODE = ("sphere", "plane", "capsule")  # `ivx_collidable_query.mode`
GENERATORS = GENERATOR_OF_MODE + ("mutual",)


# ---- the transform ---------------------------------------------------------------------------------------------------------------------------------
def conjugate(q):
    return np.concatenate([-q[..., :3], q[..., 3:]], axis=-1)


def to_object_space_f32(position, orientation_xyzw, origin_offset):
    """transform_to_object_space of a voxel body: the inverse of transform_to_world_space.applied_to_translation(-origin_offset), every operation in
    float32 and in the reference's order (isometry.rs:112-134) -> (rotation_xyzw, translation); works on arrays of cases"""
    p, q, o = (np.asarray(v, dtype=np.float32) for v in (position, orientation_xyzw, origin_offset))
    t_w = nr.qrot(q, -o) + p
    q_i = conjugate(q)
    t = -nr.qrot(q_i, t_w)
    assert q_i.dtype == np.float32 and t.dtype == np.float32
    return q_i, t


# ---- voxel bodies ----------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class VoxelBody:
    """a voxel object as a collidable: the oracle's object with its mesh and probes kept alive, the same object on the device (None on the CPU), the
    centre of mass in model space (the argument of the mutual generator) and the origin offset (the body frame's origin in model space)"""
    o: ol.OracleObject
    graph: object
    extent: float
    densities: np.ndarray
    mesh: ol.OracleMeshHandle
    probe_state: ol.OracleProbes
    center_of_mass: np.ndarray
    origin_offset: np.ndarray
    g: object = None

    def probes(self):
        return self.probe_state.get()

    def inertial_properties(self):
        return ol.derive_inertial_properties(self.o.inertia(self.densities)[0])


def voxel_body(graph, extent, density=1.0):
    o = pu.oracle_from_graph(graph, extent)
    o.update_occupied_voxel_ranges()
    o.compute_all_derived_state()
    densities = np.full(256, density, dtype=np.float32)
    mesh = ol.OracleMeshHandle(o)
    com = o.center_of_mass(densities)
    return VoxelBody(o, graph, float(extent), densities, mesh, ol.OracleProbes(mesh), com, com.copy())


def rigid_body_of(vb, position, orientation=(0, 0, 0, 1), velocity=(0, 0, 0), angular_velocity=(0, 0, 0)):
    """the dynamic body of a voxel object: mass and inertia tensor from its moments, the frame's origin at the centre of mass"""
    props = vb.inertial_properties()
    q = np.asarray(orientation, dtype=np.float64)
    return ol.rigid_body_new(props["mass"], props["inertia"].astype(np.float64), position, (q / np.linalg.norm(q)).astype(np.float32), velocity, angular_velocity)


def model_aabb(obj):
    """`ivx_grid_model_aabb`: the occupied voxel ranges times the extent, in float32; of an oracle object, or of a device object through the library"""
    if not isinstance(obj, ol.OracleObject):
        return bvol.grid_model_aabb(obj)
    extent = f32(ol.lib().orc_object_extent(obj.h))
    occ = np.array(obj.info()["occupied_voxel_ranges"], dtype=np.uint32)
    out = np.zeros((), dtype=capi.AABB_DTYPE)
    out["lower"], out["upper"] = occ[:, 0].astype(np.float32) * extent, occ[:, 1].astype(np.float32) * extent
    return out


def voxel_collidable(obj, origin_offset, body, collidable_id, kind=capi.BV_DYNAMIC, response=(0.0, 0.0, 0.0), kinematic=False, shifted=True):
    """`collision.voxel_object` over the object's model box as the BODY frame sees it: shifted by -origin_offset, in float32. `shifted=False` is the
    record of a caller that forgot the shift (what the containment tests must be able to see)"""
    box = model_aabb(obj)
    off = np.asarray(origin_offset, dtype=np.float32) if shifted else np.zeros(3, dtype=np.float32)
    return collision.voxel_object(box["lower"].astype(np.float32) - off, box["upper"].astype(np.float32) - off, body, collidable_id, kind, response, kinematic)


def model_box_corners_in_world_f64(obj, origin_offset, position, orientation_xyzw):
    """the float64 image of the eight corners of the occupied model box under the body's pose, the body frame's origin at origin_offset"""
    box = model_aabb(obj)
    lo, hi = box["lower"].astype(np.float64), box["upper"].astype(np.float64)
    corners = np.array([[(lo, hi)[(k >> d) & 1][d] for d in range(3)] for k in range(8)])
    q, p = np.asarray(orientation_xyzw, dtype=np.float64), np.asarray(position, dtype=np.float64)
    return nr.qrot(np.broadcast_to(q, (8, 4)), corners - np.asarray(origin_offset, dtype=np.float64)) + p


def box_contains(box, points):
    return bool((points >= box["lower"].astype(np.float64)).all() and (points <= box["upper"].astype(np.float64)).all())


# ---- dispatch --------------------------------------------------------------------------------------------------------------------------------------
def combined_response(r1, r2):
    """ContactResponseParameters::combined as narrow_ref.pair_contacts states it, float32"""
    r1, r2 = np.asarray(r1, dtype=np.float32), np.asarray(r2, dtype=np.float32)
    return np.array([np.where(r2[0] > r1[0], r2[0], r1[0]), np.sqrt(r1[1] * r2[1]), np.sqrt(r1[2] * r2[2])], dtype=np.float32)


@dataclasses.dataclass
class DeviceBody:
    """the same voxel object on the device, with the centre of mass and origin offset its own side of a run holds"""
    g: object
    center_of_mass: np.ndarray
    origin_offset: np.ndarray


@dataclasses.dataclass
class CollidableRows:
    """rows of `many.voxel_object_contacts_many`: the query records, the collidable index of each row's voxel object, the deferred position it came from"""
    queries: np.ndarray
    objects: list
    source: list


@dataclasses.dataclass
class MutualRows:
    """rows of `many.mutual_voxel_object_contacts_many` (handles a / b left zero: `mutual_queries_for` fills them), the collidable indices of A and B,
    the deferred position each row came from"""
    queries: np.ndarray
    objects: list
    source: list


def dispatch(world, deferred_pairs, bodies, voxel_bodies, transform=to_object_space_f32):
    """generate_contact_manifold's table over the deferred pairs. `world`: the world-space collidables (shape, id, body, response and the primitive
    shapes in world space); `bodies`: (dynamic, kinematic) records the voxel objects' transforms are derived from; `voxel_bodies`: collidable index ->
    VoxelBody -> (CollidableRows, MutualRows)"""
    dyn, kin = bodies
    deferred_pairs = np.asarray(deferred_pairs, dtype=np.uint32).reshape(-1, 2)

    def to_object(i):
        ref = int(world["body"][i])
        b = kin[ref & 0x7FFFFFFF] if ref & capi.KINEMATIC_BIT else dyn[ref]
        return transform(b["position"], b["orientation"], voxel_bodies[i].origin_offset)

    rows, row_objects, row_source, mutual, mutual_objects, mutual_source = [], [], [], [], [], []
    for n, (a, b) in enumerate(deferred_pairs.tolist()):
        sa, sb = int(world["shape"][a]), int(world["shape"][b])
        assert VOXEL in (sa, sb), (a, b)
        if sa == VOXEL and sb == VOXEL:  # Original: A is a
            q = np.zeros((), dtype=capi.MUTUAL_QUERY_DTYPE)
            (q["rotation_a"], q["translation_a"]), (q["rotation_b"], q["translation_b"]) = to_object(a), to_object(b)
            q["center_of_mass_a"], q["center_of_mass_b"] = voxel_bodies[a].center_of_mass, voxel_bodies[b].center_of_mass
            q["collidable_id_a"], q["collidable_id_b"], q["body_a"], q["body_b"] = world["id"][a], world["id"][b], world["body"][a], world["body"][b]
            q["response"] = combined_response(world["response"][a], world["response"][b])
            mutual.append(q)
            mutual_objects.append((a, b))
            mutual_source.append(n)
            continue
        v, c = (a, b) if sa == VOXEL else (b, a)  # the voxel object and the other member
        q = np.zeros((), dtype=capi.COLLIDABLE_QUERY_DTYPE)
        q["rotation_xyzw"], q["translation"] = to_object(v)
        shape = int(world["shape"][c])
        if shape == PLANE:  # the voxel object is A; the id hash takes the plane first
            q["mode"], q["shape3"], q["shape1"] = 1, world["a"][c], world["s"][c]
            q["body_a"], q["body_b"] = world["body"][v], world["body"][c]
            q["response"] = combined_response(world["response"][v], world["response"][c])
        else:  # the sphere or capsule is A and its id comes first
            q["mode"], q["shape3"], q["shape1"] = (0 if shape == SPHERE else 2), world["a"][c], world["s"][c]
            if shape == CAPSULE:
                q["shape3b"] = world["b"][c]
            q["body_a"], q["body_b"] = world["body"][c], world["body"][v]
            q["response"] = combined_response(world["response"][c], world["response"][v])
        q["collidable_id_a"], q["collidable_id_b"] = world["id"][c], world["id"][v]
        rows.append(q)
        row_objects.append(v)
        row_source.append(n)
    return (CollidableRows(np.array(rows, dtype=capi.COLLIDABLE_QUERY_DTYPE).reshape(-1), row_objects, row_source),
            MutualRows(np.array(mutual, dtype=capi.MUTUAL_QUERY_DTYPE).reshape(-1), mutual_objects, mutual_source))


def _response(q):
    return tuple(q["response"])  # (np.float32 scalars: the record fields they are assigned to take them as they are)


def oracle_collidable_manifold(vb, q):
    """one `ivx_collidable_query` row through the oracle's generator"""
    ids = (int(q["collidable_id_a"]), int(q["collidable_id_b"]), int(q["body_a"]), int(q["body_b"]), _response(q))
    if q["mode"] == 0:
        return oracle_contact_list(vb.o, q["rotation_xyzw"], q["translation"], q["shape3"], float(q["shape1"]), *ids)
    if q["mode"] == 1:
        return oracle_plane_contact_list(vb.o, q["rotation_xyzw"], q["translation"], q["shape3"], float(q["shape1"]), *ids)
    return oracle_capsule_contact_list(vb.o, q["rotation_xyzw"], q["translation"], q["shape3"], q["shape3b"], float(q["shape1"]), *ids)


def oracle_mutual_manifold(va, vb, q):
    return oracle_mutual_contact_list(va.o, va.probes(), q["center_of_mass_a"], q["rotation_a"], q["translation_a"], vb.o, vb.probes(), q["center_of_mass_b"],
                                      q["rotation_b"], q["translation_b"], int(q["collidable_id_a"]), int(q["collidable_id_b"]), int(q["body_a"]),
                                      int(q["body_b"]), _response(q))[0]


def oracle_manifolds(rows, mutual, voxel_bodies, n_deferred):
    """the manifold of every deferred pair, in deferred-list order, from the oracle's generators"""
    out = [None] * n_deferred
    for q, v, n in zip(rows.queries, rows.objects, rows.source):
        out[n] = oracle_collidable_manifold(voxel_bodies[v], q)
    for q, (a, b), n in zip(mutual.queries, mutual.objects, mutual.source):
        out[n] = oracle_mutual_manifold(voxel_bodies[a], voxel_bodies[b], q)
    assert all(m is not None for m in out)
    return out


def mutual_queries_for(mutual, voxel_bodies):
    """the `ivx_mutual_query` records with the device objects' handles filled in"""
    q = mutual.queries.copy()
    for i, (a, b) in enumerate(mutual.objects):
        q[i]["a"], q[i]["b"] = voxel_bodies[a].g.h.value, voxel_bodies[b].g.h.value
    return q


def device_manifolds(rows, mutual, voxel_bodies, n_deferred):
    """the same list from the two `_many` calls of the library"""
    from impact_amd import many

    out = [None] * n_deferred
    got, off = many.voxel_object_contacts_many([voxel_bodies[v].g for v in rows.objects], rows.queries)
    for i, n in enumerate(rows.source):
        out[n] = got[off[i]:off[i + 1]]
    got, off = many.mutual_voxel_object_contacts_many(mutual_queries_for(mutual, voxel_bodies))
    for i, n in enumerate(mutual.source):
        out[n] = got[off[i]:off[i + 1]]
    assert all(m is not None for m in out)
    return out


def generator_of(rows, mutual, n_deferred):
    """the generator of every deferred pair, in deferred-list order"""
    out = [None] * n_deferred
    for q, n in zip(rows.queries, rows.source):
        out[n] = GENERATOR_OF_MODE[int(q["mode"])]
    for n in mutual.source:
        out[n] = "mutual"
    return out


def merge(primitive_contacts, voxel_manifolds):
    """the contact list of a frame: the primitive contacts as `ivx_cw_collide` returns them, then the voxel manifolds in deferred-list order"""
    return np.concatenate([np.ascontiguousarray(primitive_contacts, dtype=capi.CONTACT_DTYPE)] +
                          [np.ascontiguousarray(m, dtype=capi.CONTACT_DTYPE) for m in voxel_manifolds])


# ---- the frame on the CPU --------------------------------------------------------------------------------------------------------------------------
def oracle_frame(local, voxel_bodies, bodies, mode=capi.BV_DYNAMIC_PAIRS, physics=None, dt=None, transform=to_object_space_f32):
    """one frame over the given bodies (dynamic, kinematic): narrow_ref for boxes, pairs, primitive contacts and deferred pairs, the oracle's generators
    for the voxel pairs, and — given the oracle's world and a step duration — its step over the merged list -> dict of every intermediate"""
    dyn, kin = bodies
    world, boxes = nr.transform(local, *nr.body_frames(local, dyn, kin))
    pairs = nr.broad_phase_pairs(boxes, local["kind"], mode)
    contacts, deferred = nr.collide(world, pairs)
    rows, mutual = dispatch(world, deferred, bodies, voxel_bodies, transform)
    manifolds = oracle_manifolds(rows, mutual, voxel_bodies, len(deferred))
    merged = merge(contacts, manifolds)
    if physics is not None:
        physics.step(merged, dt)
    return {"world": world, "boxes": boxes, "pairs": pairs, "contacts": contacts, "deferred": deferred, "rows": rows, "mutual": mutual,
            "generators": generator_of(rows, mutual, len(deferred)), "manifolds": manifolds, "merged": merged}


# ---- scenes (oracle side) --------------------------------------------------------------------------------------------------------------------------
def axis_angle(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    return np.array([*(axis / np.linalg.norm(axis) * np.sin(0.5 * angle)), np.cos(0.5 * angle)], dtype=np.float32)


def static_kinematic(n=1):
    k = np.zeros(n, dtype=capi.KINEMATIC_BODY_DTYPE)
    k["orientation"], k["angular_axis"] = (0, 0, 0, 1), (0, 1, 0)
    return k


def completeness_scene(vb, seed=31):
    """one voxel object (collidable 0) on a rotated dynamic body, 64 spheres and 32 capsules (on a second body, at the identity) scattered from well
    inside its world box to well outside, a plane through it listed last -> (local collidables, dynamic bodies, kinematic bodies, voxel bodies)"""
    rng = np.random.default_rng(seed)
    centre = np.array([3.0, -2.0, 1.5])
    dyn = np.array([rigid_body_of(vb, centre, axis_angle((0.3, -1.0, 0.5), 0.9)), nr.unit_body((0, 0, 0))], dtype=capi.RIGID_BODY_DTYPE)
    kin = static_kinematic()
    half = 0.5 * float(np.max(model_aabb(vb.o)["upper"] - model_aabb(vb.o)["lower"]))
    local = [voxel_collidable(vb.o, vb.origin_offset, 0, 1000, response=(0.2, 0.6, 0.4))]
    for k in range(96):
        direction = rng.normal(size=3)
        direction /= np.linalg.norm(direction)
        at = centre + direction * rng.uniform(0.9, 3.4) * half
        radius = rng.uniform(0.2, 0.8)
        if k < 64:
            local.append(collision.sphere(at, radius, 1, 1001 + k, response=(0.3, 0.5, 0.5)))
        else:
            v = rng.normal(size=3)
            v *= rng.uniform(0.3, 2.0) / np.linalg.norm(v)
            local.append(collision.capsule(at - 0.5 * v, v, radius, 1, 1001 + k, response=(0.1, 0.7, 0.3)))
    local.append(collision.plane((0, 1, 0), centre[1] - 0.5 * half, 0, 2000, response=(0.0, 0.8, 0.6), kinematic=True))
    return np.array(local, dtype=capi.COLLIDABLE_DTYPE), dyn, kin, {0: vb}


def _attached(body, world_point):
    """a world-space point in the frame of a body record (float64, rounded when the record is filled)"""
    q = body["orientation"].astype(np.float64)
    return nr.qrot(conjugate(q), np.asarray(world_point, dtype=np.float64) - body["position"].astype(np.float64))


def _attached_vector(body, world_vector):
    return nr.qrot(conjugate(body["orientation"].astype(np.float64)), np.asarray(world_vector, dtype=np.float64))


@functools.lru_cache(maxsize=None)
def static_scene(seed=5):
    """three voxel objects — a sphere (41 voxels across, extent 0.25), a box (32 x 20 x 28, extent 0.25) under it and overlapping it, a two-sphere body
    (32 x 18 x 18, extent 0.5, a STATIC collidable) beside them — on dynamic bodies with orientations of their own and their centres of mass as
    origin offsets; 13 spheres and 4 capsules on four carrier bodies scattered about the surfaces of the three, some listed before the voxel objects
    and some after, two of the spheres static and one a phantom; one plane on a turned kinematic body through the box's underside, listed last
    -> (local collidables, dynamic bodies, kinematic bodies, voxel bodies by collidable index)"""
    rng = np.random.default_rng(seed)
    va, vb, vc = voxel_body(scenes.sphere_scene(20.0), 0.25), voxel_body(scenes.box_scene((32.0, 20.0, 28.0)), 0.25), voxel_body(scenes.two_spheres_scene(9.0, 14.0), 0.5)
    centres = [np.array([0.5, 0.25, -0.125]), np.array([0.8, -6.6, 0.3]), np.array([11.5, -1.0, 0.6])]
    dyn = [rigid_body_of(va, centres[0], axis_angle((0.3, -1.0, 0.5), 0.9)), rigid_body_of(vb, centres[1], axis_angle((1.0, 0.2, -0.4), 0.25)),
           rigid_body_of(vc, centres[2], axis_angle((0.1, 0.3, 1.0), -0.5))]
    for k in range(4):
        dyn.append(nr.unit_body(rng.uniform(-3.0, 3.0, 3), br.random_unit_quaternion(rng)))
    dyn = np.array(dyn, dtype=capi.RIGID_BODY_DTYPE)
    kin = static_kinematic()
    kin["position"], kin["orientation"] = (0.0, -8.9, 0.0), axis_angle((1.0, 0.0, 0.3), 0.06)
    reach = [5.0, 3.2, 4.5]  # about the distance of each surface from its centre, towards the primitives placed below

    def primitive(k):
        target = k % 3
        direction = rng.normal(size=3)
        direction[1] = abs(direction[1]) if target == 1 else direction[1]  # (above the box: under it is the plane)
        direction /= np.linalg.norm(direction)
        radius = rng.uniform(0.4, 1.1)
        at = centres[target] + direction * (reach[target] * rng.uniform(0.95, 1.45) + 0.5 * radius)
        carrier = 3 + k % 4
        kind = {4: capi.BV_STATIC, 9: capi.BV_STATIC, 11: capi.BV_PHANTOM}.get(k, capi.BV_DYNAMIC)
        response = (0.1 + 0.05 * (k % 5), 0.5 + 0.03 * k, 0.4)
        if k < 13:
            return collision.sphere(_attached(dyn[carrier], at), radius, carrier, 500 + k, kind, response)
        v = rng.normal(size=3)
        v *= rng.uniform(1.0, 3.0) / np.linalg.norm(v)
        return collision.capsule(_attached(dyn[carrier], at - 0.5 * v), _attached_vector(dyn[carrier], v), 0.6 * radius, carrier, 500 + k, kind, response)

    prim = [primitive(k) for k in range(17)]
    voxels = [voxel_collidable(va.o, va.origin_offset, 0, 100, response=(0.2, 0.6, 0.4)), voxel_collidable(vb.o, vb.origin_offset, 1, 101, response=(0.1, 0.7, 0.5)),
              voxel_collidable(vc.o, vc.origin_offset, 2, 102, capi.BV_STATIC, response=(0.3, 0.5, 0.3))]
    plane = collision.plane((0, 1, 0), 0.0, 0, 900, response=(0.0, 0.8, 0.6), kinematic=True)
    local = prim[:3] + [prim[13]] + [voxels[0]] + prim[3:8] + [prim[14]] + [voxels[1]] + prim[8:11] + [voxels[2]] + prim[11:13] + prim[15:17] + [plane]
    local = np.array(local, dtype=capi.COLLIDABLE_DTYPE)
    voxel_index = [int(i) for i in np.nonzero(local["shape"] == VOXEL)[0]]
    return local, dyn, kin, dict(zip(voxel_index, (va, vb, vc)))


# ---- the falling scene: frames, and the same scene across an edit ----------------------------------------------------------------------------------
DT, GRAVITY = 0.004, 9.81
N_FRAMES, N_FRAMES_AFTER_EDIT = 60, 15
EXTENT = 0.25
FALLING_GRAPHS = {"box": ((40.0, 12.0, 20.0), EXTENT), "sphere": (10.0, EXTENT)}  # 10 x 3 x 5 and a radius of 2.5 in world units
# centre (voxel units, grid corner at the origin), influence radius, radius: a nearly flat cut that empties the last 13 of the box's 40 layers along x.
# The occupied ranges stay (1, 41): the reference recomputes them only when an edit removes a whole chunk, and the emptied chunks keep the non-void
# voxels of the grid's margin, which lie outside the occupied ranges and are not edited (intersection.rs:254-256). The model box is therefore the same
# on both sides before and after; what moves the record and the world box is the origin offset.
BITE = ((81.0, 7.0, 11.0), 55.0, 53.0)


def falling_voxel_bodies():
    return voxel_body(scenes.box_scene(FALLING_GRAPHS["box"][0]), EXTENT), voxel_body(scenes.sphere_scene(FALLING_GRAPHS["sphere"][0]), EXTENT)


def falling_scene(box, sphere):
    """a voxel box (dynamic, slightly turned) just above a level kinematic plane, a smaller voxel sphere just above the box, a ball above the box beside
    the sphere, a capsule above the sphere and a small ball above the first one (a primitive contact that shares a body with a voxel manifold: the
    order of the merged list matters to the solver), all moving down at 0.4 under gravity -> (local collidables, dynamic bodies, kinematic bodies,
    voxel bodies by collidable index). Listed: ball, box, capsule, sphere, small ball, plane — (sphere, voxel), (voxel, capsule), (capsule, voxel),
    (voxel, voxel), (voxel, sphere) and (voxel, plane) pairs all occur"""
    down = (0.0, -0.4, 0.0)
    dyn = np.array([rigid_body_of(box, (0.0, 1.5 + 0.03, 0.0), axis_angle((0.2, 0.0, 1.0), 0.012), down),
                    rigid_body_of(sphere, (0.3, 3.0 + 2.5 + 0.06, 0.1), axis_angle((1.0, 1.0, 0.0), 0.7), down),
                    ol.uniform_sphere_body(0.5, 2.0, (-3.6, 3.0 + 0.5 + 0.06, 0.4), down),
                    ol.rigid_body_new(1.5, np.diag([0.4, 0.1, 0.4]), (0.3, 3.0 + 5.0 + 0.4 + 0.09, 0.1), axis_angle((0.0, 1.0, 0.0), 0.3), down),
                    ol.uniform_sphere_body(0.3, 2.0, (-3.57, 3.0 + 1.0 + 0.3 + 0.09, 0.42), down)], dtype=capi.RIGID_BODY_DTYPE)
    dyn["total_force"][:, 1] = -GRAVITY * dyn["mass"]
    kin = static_kinematic()
    response = (0.0, 0.7, 0.5)
    local = np.array([collision.sphere((0, 0, 0), 0.5, 2, 11, response=response),
                      voxel_collidable(box.o, box.origin_offset, 0, 12, response=response),
                      collision.capsule((-0.8, 0.0, 0.0), (1.6, 0.0, 0.0), 0.4, 3, 13, response=response),
                      voxel_collidable(sphere.o, sphere.origin_offset, 1, 14, response=response),
                      collision.sphere((0, 0, 0), 0.3, 4, 16, response=response),
                      collision.plane((0, 1, 0), 0.0, 0, 15, response=response, kinematic=True)], dtype=capi.COLLIDABLE_DTYPE)
    return local, dyn, kin, {1: box, 3: sphere}


def frame_record(frame, bodies_after):
    return {"deferred": frame["deferred"].copy(), "generators": frame["generators"], "lengths": [len(m) for m in frame["manifolds"]], "n_merged": len(frame["merged"]),
            "n_primitive": len(frame["contacts"]), "boxes": frame["boxes"].copy(), "bodies": bodies_after}


def lowest_points(local, voxel_bodies, dyn):
    """the height of every dynamic body's lowest point over the plane y = 0 (float64): the voxel objects' model box corners, the ball's and the capsule's
    lowest points"""
    out = {}
    for i, c in enumerate(local):
        if c["shape"] == PLANE:
            continue
        b = dyn[int(c["body"])]
        if c["shape"] == VOXEL:
            out[i] = float(model_box_corners_in_world_f64(voxel_bodies[i].o, voxel_bodies[i].origin_offset, b["position"], b["orientation"])[:, 1].min())
        else:
            q, p = b["orientation"].astype(np.float64), b["position"].astype(np.float64)
            ends = [nr.qrot(q, c["a"].astype(np.float64)) + p]
            if c["shape"] == CAPSULE:
                ends.append(nr.qrot(q, (c["a"] + c["b"]).astype(np.float64)) + p)
            out[i] = min(float(e[1]) for e in ends) - float(c["s"])
    return out


def reseated_collidable(local, index, obj, origin_offset):
    """the list with voxel collidable `index` set again from the object's model box as it is now and the given origin offset"""
    out = local.copy()
    c = local[index]
    out[index] = voxel_collidable(obj, origin_offset, int(c["body"]), int(c["id"]), int(c["kind"]), tuple(c["response"]))
    return out


class OracleSide:
    """the falling scene on the CPU: the oracle's objects, narrow_ref, the oracle's generators and world"""

    def __init__(self):
        self.box, self.sphere = falling_voxel_bodies()
        self.local, dyn, kin, self.voxel_bodies = falling_scene(self.box, self.sphere)
        self.initial_bodies = (dyn.copy(), kin.copy())
        self.physics = ol.OraclePhysics(dyn, kin, (8, 0.4, 3, 0.2))

    def bodies(self):
        return self.physics.bodies()

    def frame(self):
        f = oracle_frame(self.local, self.voxel_bodies, self.bodies(), capi.BV_DYNAMIC_PAIRS, self.physics, DT)
        return frame_record(f, self.bodies()[0])

    def bite(self):
        """absorb_sphere at the box's +x end, mesh and probes synced, the body re-seated on the new inertial properties, the collidable set again from the
        new model box and the new local centre of mass -> what changed"""
        box, (dyn, kin) = self.box, self.bodies()
        centre, influence, radius = BITE
        res = box.o.absorb_sphere(np.array(centre, dtype=np.float32), influence, radius, box.densities)
        box.mesh.sync(res["invalidated"])
        box.probe_state.sync(res["invalidated"])
        old_offset = box.origin_offset.copy()
        body, new_com = ol.apply_updated_inertial_properties(dyn[0], box.o.inertia(box.densities)[0], old_offset)
        dyn[0] = body
        ol.lib().orc_physics_set_bodies(self.physics.h, ol._p(dyn), len(dyn), ol._p(kin), len(kin))
        box.origin_offset, box.center_of_mass = new_com.copy(), box.o.center_of_mass(box.densities)
        stale = reseated_collidable(self.local, 1, box.o, old_offset)  # (the new model box, the OLD offset: what a caller that forgot the inertial update sets)
        self.local = reseated_collidable(self.local, 1, box.o, new_com)
        return {"invalidated": res["invalidated"], "old_offset": old_offset, "new_offset": new_com.copy(), "body": body.copy(), "stale_record": stale[1].copy(),
                "record": self.local[1].copy()}


@functools.lru_cache(maxsize=None)
def oracle_run():
    """the oracle side of the whole run — N_FRAMES frames, the bite, N_FRAMES_AFTER_EDIT frames — once -> dict(records, edit, side)"""
    side = OracleSide()
    records = [side.frame() for _ in range(N_FRAMES)]
    record_before = side.local[1].copy()
    edit = side.bite()
    edit["record_before"] = record_before
    records += [side.frame() for _ in range(N_FRAMES_AFTER_EDIT)]
    return {"records": records, "edit": edit, "side": side}


def frames_with(records, generator):
    """the number of frames in which a manifold of the generator is non-empty"""
    return sum(any(g == generator and n > 0 for g, n in zip(r["generators"], r["lengths"])) for r in records)


def assert_run_is_physical(side, records, n_frames_elapsed):
    """on the oracle's run: every generator at work in at least ten frames; at the end nothing has sunk more than a voxel under the plane, and every
    body moves down more slowly than free fall would have it — what a swapped A / B or a flipped normal breaks"""
    for generator in GENERATORS:
        assert frames_with(records, generator) >= 10, (generator, frames_with(records, generator))
    assert sum(r["n_primitive"] > 0 for r in records) >= 10  # (and primitive contacts in front of them)
    dyn = records[-1]["bodies"]
    low = lowest_points(side.local, side.voxel_bodies, dyn)
    assert min(low.values()) >= -EXTENT, low
    v0 = -side.initial_bodies[0]["momentum"][:, 1] / side.initial_bodies[0]["mass"]
    down = -dyn["momentum"][:, 1] / dyn["mass"]
    free_fall = v0 + GRAVITY * DT * n_frames_elapsed
    assert (down < free_fall).all(), (down, free_fall)
    assert (down < 0.5).all(), down  # (nothing has gained speed worth naming over the 0.4 it started with: they have come to rest on each other)
