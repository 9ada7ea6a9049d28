"""Numpy checker of the primitive collidable calls (impact_amd/csrc/narrow.hip): the transforms, world boxes, five contact geometries, dispatch,
id hash and combined response in exactly the operation order include/impact_voxel_hip.h states. Every function works on arrays of cases and in the
precision of its inputs: handed float32 arrays every intermediate is an np.float32 array (the restatement the library must equal byte for byte),
handed float64 arrays it is the float64 version of the same geometry (what the float32 results are measured against).

It also holds the seeded scene of the device tests and the seeded pairs and hand-made branch cases of the host tests."""
import functools

import numpy as np

import bvol_ref as br
from impact_amd import capi

f32 = np.float32
SPHERE, PLANE, CAPSULE, VOXEL = capi.CW_SPHERE, capi.CW_PLANE, capi.CW_CAPSULE, capi.CW_VOXEL_OBJECT
NO_CONTACT, CONTACT, DEFERRED = 0, 1, 2
FLT_MAX = np.finfo(np.float32).max


# ---- arithmetic --------------------------------------------------------------------------------------------------------------------------
def _k(like, v):
    """the constant v in the precision of `like`"""
    return like.dtype.type(v)


def dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2], a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0], a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], axis=-1)


def scale(u, k):
    return u * np.asarray(k)[..., None]


def qrot(q, v):
    """glam Quat::mul_vec3a"""
    b, w = q[..., :3], q[..., 3]
    b2 = dot(b, b)
    return (scale(v, w * w - b2) + scale(b, dot(v, b) * _k(v, 2))) + scale(cross(b, v), w * _k(v, 2))


def max0(x):
    return np.where(x > 0, x, _k(x, 0))


def clamp01(x):
    return np.where(x < 0, _k(x, 0), np.where(x > 1, _k(x, 1), x))


def eps(like):
    return like.dtype.type(f32(1e-8))


def unit_z(like):
    z = np.zeros_like(like)
    z[..., 2] = 1
    return z


def ortho(v):
    """any_orthogonal_vector, normalized when its squared length is above EPS EPS, else unit z"""
    zero = np.zeros_like(v[..., 0])
    o = np.where((np.abs(v[..., 0]) > np.abs(v[..., 1]))[..., None], np.stack([-v[..., 2], zero, v[..., 0]], axis=-1), np.stack([zero, v[..., 2], -v[..., 1]], axis=-1))
    o2 = dot(o, o)
    with np.errstate(all="ignore"):
        n = o / np.sqrt(o2)[..., None]
    return np.where((o2 > eps(v) * eps(v))[..., None], n, unit_z(v))


# ---- the five geometries: -> (hit [m] bool, position [m, 3], normal [m, 3], depth [m]); rows that miss hold garbage -----------------------------
def sphere_sphere(c1, r1, c2, r2):
    d = c1 - c2
    d2, m = dot(d, d), r1 + r2
    dist = np.sqrt(d2)
    with np.errstate(all="ignore"):
        n = np.where((dist > eps(d2))[..., None], scale(d, _k(d2, 1) / dist), unit_z(d))
    return ~(d2 > m * m), c2 + scale(n, r2), n, max0(m - dist)


def sphere_plane(c, r, n, k):
    sd = dot(n, c) - k
    depth = r - sd
    return ~(depth < 0), c - scale(n, sd), n, depth


def capsule_sphere(a, v, rc, c, r):
    l2 = dot(v, v)
    with np.errstate(all="ignore"):
        t = np.where(l2 <= eps(l2), _k(l2, 0), clamp01(dot(v, c - a) / l2))
        d = c - (a + scale(v, t))
        d2, m = dot(d, d), r + rc
        dist = np.sqrt(d2)
        apart = dist > eps(d2)
        cn = np.where(apart[..., None], scale(d, _k(d2, 1) / dist), ortho(v))
    depth = np.where(apart, max0(m - dist), max0(m))
    n = -cn
    return ~(d2 > m * m), c + scale(n, r), n, depth


def closest_parameters(a1, v1, a2, v2, details=False):
    """parameters_of_closest_points_on_line_segments -> (s on segment 1, t on segment 2); details: also the denominator and the B parameter before it
    is clamped, as the general branch computes them"""
    l1, l2 = dot(v1, v1), dot(v2, v2)
    e, zero, one = eps(l1), _k(l1, 0), _k(l1, 1)
    r = a1 - a2
    f, c, g = dot(v2, r), dot(v1, r), dot(v1, v2)
    den = l1 * l2 - g * g
    with np.errstate(all="ignore"):
        t_point_1 = clamp01(f / l2)
        s_start = clamp01(c / (-l1))
        s_g = np.where(den != 0, clamp01((g * f - c * l2) / den), zero)
        t_g = (g * s_g + f) / l2
        neg = np.signbit(t_g)
        over = ~neg & (t_g > 1)
        s_general = np.where(neg, s_start, np.where(over, clamp01((g - c) / l1), s_g))
        t_general = np.where(neg, zero, np.where(over, one, t_g))
    p1, p2 = l1 <= e, l2 <= e
    s = np.where(p1, zero, np.where(p2, s_start, s_general))
    t = np.where(p1 & p2, zero, np.where(p1, t_point_1, np.where(p2, zero, t_general)))
    if details:
        return s.astype(l1.dtype), t.astype(l1.dtype), den, t_g
    return s.astype(l1.dtype), t.astype(l1.dtype)


def capsule_capsule(a1, v1, r1, a2, v2, r2):
    s, t = closest_parameters(a1, v1, a2, v2)
    p1, p2 = a1 + scale(v1, s), a2 + scale(v2, t)
    d = p1 - p2
    d2, m = dot(d, d), r1 + r2
    dist = np.sqrt(d2)
    apart = dist > eps(d2)
    with np.errstate(all="ignore"):
        crossing_n = ortho(v2)
        n = np.where(apart[..., None], scale(d, _k(d2, 1) / dist), crossing_n)
    w = dot(v1, crossing_n)
    shift = np.where(~np.signbit(w), (_k(w, 1) - s) * w, (-s) * w)
    depth = np.where(apart, max0(m - dist), max0(m + shift))
    return ~(d2 > m * m), p2 + scale(n, r2), n, depth


def capsule_plane(a, v, r, n, k):
    e = a + v
    d0, d1 = dot(n, a) - k, dot(n, e) - k
    first = d0 <= d1
    p, low = np.where(first[..., None], a, e), np.where(first, d0, d1)
    depth = r - low
    return ~(depth < 0), p - scale(n, low), n, depth


# ---- dispatch, id hash, combined response ---------------------------------------------------------------------------------------------------------
def splitmix(state):
    with np.errstate(over="ignore"):  # (arithmetic modulo 2^64)
        return _splitmix(state)


def _splitmix(state):
    state = (np.asarray(state, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)).astype(np.uint64)
    z = state
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def swapped_order(shape_a, shape_b):
    """where the reference answers CollidableOrder::Swapped"""
    return ((shape_a == SPHERE) & (shape_b == CAPSULE)) | ((shape_a == PLANE) & (shape_b != PLANE) & (shape_b != VOXEL))


def pair_geometry(first, second, dtype=np.float32):
    """the members AFTER the swap -> (hit, position, normal, depth) in `dtype`"""
    m = len(first)
    a1, b1, s1 = first["a"].astype(dtype), first["b"].astype(dtype), first["s"].astype(dtype)
    a2, b2, s2 = second["a"].astype(dtype), second["b"].astype(dtype), second["s"].astype(dtype)
    hit, pos, nrm, depth = np.zeros(m, dtype=bool), np.zeros((m, 3), dtype=dtype), np.zeros((m, 3), dtype=dtype), np.zeros(m, dtype=dtype)
    forms = {(CAPSULE, CAPSULE): lambda r: capsule_capsule(a1[r], b1[r], s1[r], a2[r], b2[r], s2[r]),
             (CAPSULE, SPHERE): lambda r: capsule_sphere(a1[r], b1[r], s1[r], a2[r], s2[r]),
             (CAPSULE, PLANE): lambda r: capsule_plane(a1[r], b1[r], s1[r], a2[r], s2[r]),
             (SPHERE, SPHERE): lambda r: sphere_sphere(a1[r], s1[r], a2[r], s2[r]),
             (SPHERE, PLANE): lambda r: sphere_plane(a1[r], s1[r], a2[r], s2[r])}
    for (sf, ss), form in forms.items():
        rows = np.nonzero((first["shape"] == sf) & (second["shape"] == ss))[0]
        if len(rows):
            h, p, n, d = form(rows)
            assert p.dtype == dtype and n.dtype == dtype and d.dtype == dtype, (sf, ss, p.dtype, n.dtype, d.dtype)
            hit[rows], pos[rows], nrm[rows], depth[rows] = h, p, n, d
    return hit, pos, nrm, depth


def ordered(a_world, b_world):
    """(first, second) after the swap, and the verdict so far: DEFERRED where a member is a voxel object"""
    sw = swapped_order(a_world["shape"], b_world["shape"])
    first, second = a_world.copy(), b_world.copy()
    first[sw], second[sw] = b_world[sw], a_world[sw]
    deferred = (a_world["shape"] == VOXEL) | (b_world["shape"] == VOXEL)
    return first, second, deferred


def pair_contacts(a_world, b_world):
    """`ivx_cw_contact` for m pairs of world-space collidables -> (verdict [m], contact records [m]: all-zero where the verdict is not CONTACT)"""
    a_world, b_world = np.atleast_1d(a_world), np.atleast_1d(b_world)
    first, second, deferred = ordered(a_world, b_world)
    hit, pos, nrm, depth = pair_geometry(first, second)
    hit &= ~deferred
    out = np.zeros(len(first), dtype=capi.CONTACT_DTYPE)
    out["id"] = splitmix(first["id"] ^ splitmix(second["id"]))
    out["body_a"], out["body_b"] = first["body"], second["body"]
    out["position"], out["normal"], out["depth"] = pos, nrm, depth
    r1, r2 = first["response"], second["response"]
    out["restitution"] = np.where(r2[:, 0] > r1[:, 0], r2[:, 0], r1[:, 0])
    out["static_friction"], out["dynamic_friction"] = np.sqrt(r1[:, 1] * r2[:, 1]), np.sqrt(r1[:, 2] * r2[:, 2])
    out["flags"] = capi.CONTACT_MANIFOLD_START
    out[~hit] = np.zeros((), dtype=capi.CONTACT_DTYPE)
    return np.where(deferred, DEFERRED, np.where(hit, CONTACT, NO_CONTACT)), out


def collide(world, pairs):
    """`ivx_cw_collide` over world-space collidables and the broad phase's pairs -> (contacts, deferred pairs), both in pair order"""
    pairs = np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)
    verdict, contacts = pair_contacts(world[pairs[:, 0]], world[pairs[:, 1]])
    return contacts[verdict == CONTACT], pairs[verdict == DEFERRED]


def decision_margin(first, second):
    """float64: how far the pair (after the swap) is from the hit / miss decision — the sum of the radii minus the distance of the segments (a sphere
    is a segment of length zero), or the radius minus the lowest signed distance to the plane; a hit when >= 0"""
    a1, a2 = first["a"].astype(np.float64), second["a"].astype(np.float64)
    v1 = np.where((first["shape"] == CAPSULE)[:, None], first["b"].astype(np.float64), 0.0)
    v2 = np.where((second["shape"] == CAPSULE)[:, None], second["b"].astype(np.float64), 0.0)
    s1, s2 = first["s"].astype(np.float64), second["s"].astype(np.float64)
    s, t = closest_parameters(a1, v1, a2, v2)
    d = (a1 + scale(v1, s)) - (a2 + scale(v2, t))
    segments = (s1 + s2) - np.sqrt(dot(d, d))
    against_plane = s1 - np.minimum(dot(a2, a1) - s2, dot(a2, a1 + v1) - s2)
    return np.where(second["shape"] == PLANE, against_plane, segments)


# ---- transforms and world boxes --------------------------------------------------------------------------------------------------------------------
def world_aabb_f32(lower, upper, q, p):
    """ivx_bv_world_aabb with scaling 1, the header's order"""
    c, h = f32(0.5) * (lower + upper), f32(0.5) * (upper - lower)
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    xx, yy, zz, ww = x * x, y * y, z * z, w * w
    n2 = ((xx + yy) + zz) + ww
    xy, xz, yz, wx, wy, wz = x * y, x * z, y * z, w * x, w * y, w * z
    rows = [[((ww + xx) - yy) - zz, f32(2) * (xy - wz), f32(2) * (xz + wy)], [f32(2) * (xy + wz), ((ww - xx) + yy) - zz, f32(2) * (yz - wx)],
            [f32(2) * (xz - wy), f32(2) * (yz + wx), ((ww - xx) - yy) + zz]]
    lo, hi = np.zeros_like(lower), np.zeros_like(lower)
    for i in range(3):
        m0, m1, m2 = (f32(1) * (rows[i][j] / n2) for j in range(3))
        ct = ((m0 * c[:, 0] + m1 * c[:, 1]) + m2 * c[:, 2]) + p[:, i]
        ht = (np.abs(m0) * h[:, 0] + np.abs(m1) * h[:, 1]) + np.abs(m2) * h[:, 2]
        lo[:, i], hi[:, i] = ct - ht, ct + ht
    return lo, hi


def transform(local, positions, orientations):
    """`ivx_cw_transform` for n collidables under their bodies' positions [n, 3] and orientations [n, 4] (float32) -> (world records, world boxes)"""
    local = np.atleast_1d(local)
    p, q = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3), np.ascontiguousarray(orientations, dtype=np.float32).reshape(-1, 4)
    world, boxes = local.copy(), np.zeros(len(local), dtype=capi.AABB_DTYPE)
    a, b, s, shape = local["a"], local["b"], local["s"], local["shape"]
    ta = qrot(q, a) + p
    assert ta.dtype == np.float32
    sp = np.nonzero(shape == SPHERE)[0]
    world["a"][sp] = ta[sp]
    boxes["lower"][sp], boxes["upper"][sp] = ta[sp] - s[sp, None], ta[sp] + s[sp, None]
    cp = np.nonzero(shape == CAPSULE)[0]
    tv = qrot(q, b)
    e = ta + tv
    world["a"][cp], world["b"][cp] = ta[cp], tv[cp]
    lo_a, lo_e, hi_a, hi_e = ta - s[:, None], e - s[:, None], ta + s[:, None], e + s[:, None]
    boxes["lower"][cp], boxes["upper"][cp] = np.where(lo_e < lo_a, lo_e, lo_a)[cp], np.where(hi_e > hi_a, hi_e, hi_a)[cp]
    pl = np.nonzero(shape == PLANE)[0]
    tn = qrot(q, a)
    tp = qrot(q, scale(a, s)) + p
    world["a"][pl], world["s"][pl] = tn[pl], dot(tn, tp)[pl]
    boxes["lower"][pl], boxes["upper"][pl] = -FLT_MAX, FLT_MAX
    vo = np.nonzero(shape == VOXEL)[0]
    lo, hi = world_aabb_f32(a, b, q, p)
    m = np.where(np.abs(b) > np.abs(a), np.abs(b), np.abs(a))  # widened by (((m_0 + m_1) + m_2) + |p_k|) 2^-19, the header's order
    pad = (((m[:, 0] + m[:, 1]) + m[:, 2])[:, None] + np.abs(p)) * f32(2.0 ** -19)
    lo, hi = lo - pad, hi + pad
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    world["a"][vo], world["b"][vo] = lo[vo], hi[vo]
    boxes["lower"][vo], boxes["upper"][vo] = lo[vo], hi[vo]
    return world, boxes


def broad_phase_pairs(boxes, kinds, mode):
    """bvol_ref's pairs (a plane's box against its like overflows to +inf in the face differences, which is the intersection it should be)"""
    with np.errstate(over="ignore"):
        return br.pairs(boxes, kinds, mode)[0]


def body_frames(local, dyn, kin):
    """position and orientation of every collidable's body"""
    body = local["body"] & np.uint32(0x7FFFFFFF)
    kinematic = (local["body"] & np.uint32(capi.KINEMATIC_BIT)) != 0
    p, q = np.zeros((len(local), 3), dtype=np.float32), np.zeros((len(local), 4), dtype=np.float32)
    if (~kinematic).any():
        p[~kinematic], q[~kinematic] = dyn["position"][body[~kinematic]], dyn["orientation"][body[~kinematic]]
    if kinematic.any():
        p[kinematic], q[kinematic] = kin["position"][body[kinematic]], kin["orientation"][body[kinematic]]
    return p, q


# ---- the seeded scene ------------------------------------------------------------------------------------------------------------------------------
def unit_body(position, orientation=(0.0, 0.0, 0.0, 1.0)):
    b = np.zeros((), dtype=capi.RIGID_BODY_DTYPE)
    b["mass"], b["inertia"], b["inv_inertia"] = 1.0, np.eye(3).reshape(-1), np.eye(3).reshape(-1)
    b["position"], b["orientation"] = position, orientation
    return b


def scene_extent(n):
    return max(2.0, 0.95 * n ** (1.0 / 3.0))


@functools.lru_cache(maxsize=None)
def _scene(n, seed, n_planes, fillers):
    rng, filler_rng = np.random.default_rng(seed), np.random.default_rng(seed + 1000)  # (the fillers leave the scene they are added to as it is)
    n_planes = min(n_planes, n)
    m = n - n_planes
    t = m + fillers
    ext = scene_extent(m)
    kinematic = np.concatenate([rng.random(m) < 0.2, np.zeros(fillers, dtype=bool)])
    positions = np.concatenate([rng.uniform(0.0, ext, (m, 3)), np.zeros((fillers, 3))])
    orientations = np.array([br.random_unit_quaternion(rng) for _ in range(m)] + [br.random_unit_quaternion(filler_rng) for _ in range(fillers)], dtype=np.float32).reshape(-1, 4)
    shapes = np.concatenate([rng.choice(np.array([SPHERE, CAPSULE, VOXEL], dtype=np.uint32), size=m, p=[0.55, 0.38, 0.07]), np.full(fillers, SPHERE, dtype=np.uint32)])
    kinds = np.concatenate([rng.choice(np.array([0, 1, 2], dtype=np.uint32), size=m, p=[0.6, 0.3, 0.1]), np.full(fillers, capi.BV_DYNAMIC, dtype=np.uint32)])
    offsets = np.concatenate([rng.uniform(-0.1, 0.1, (m, 3)), np.zeros((fillers, 3))])
    direction = np.concatenate([rng.normal(size=(m, 3)), np.ones((fillers, 3))])
    lengths = np.concatenate([rng.uniform(0.2, 0.9, (m, 1)), np.ones((fillers, 1))])
    radii = np.concatenate([rng.uniform(0.3, 0.6, m), filler_rng.uniform(0.3, 0.6, fillers)])
    box_lower, box_upper = -rng.uniform(0.2, 0.5, (m, 3)), rng.uniform(0.2, 0.5, (m, 3))
    plane_orientation = br.random_unit_quaternion(rng)
    rotation = br.rotation_matrix_f64(plane_orientation)  # the fillers: 10 apart along the first plane (normal x in its body's frame), within 1 of it
    positions[m:] = 0.5 * ext + np.outer(ext + 10.0 * (1 + np.arange(fillers)), rotation[:, 1]) + np.outer(filler_rng.uniform(-1.0, 1.0, fillers), rotation[:, 0])
    n_kin_bodies = int(kinematic.sum())
    dyn = np.array([unit_body(positions[i], orientations[i]) for i in np.nonzero(~kinematic)[0]], dtype=capi.RIGID_BODY_DTYPE).reshape(-1)
    kin = np.zeros(n_kin_bodies + 1, dtype=capi.KINEMATIC_BODY_DTYPE)  # (the last one carries the planes)
    kin["angular_axis"] = (0.0, 1.0, 0.0)
    kin["position"][:n_kin_bodies], kin["orientation"][:n_kin_bodies] = positions[kinematic], orientations[kinematic]
    kin["position"][-1], kin["orientation"][-1] = (0.5 * ext, 0.5 * ext, 0.5 * ext), plane_orientation
    index = np.zeros(t, dtype=np.uint32)
    index[~kinematic], index[kinematic] = np.arange((~kinematic).sum()), np.arange(n_kin_bodies)
    local = np.zeros(t + n_planes, dtype=capi.COLLIDABLE_DTYPE)
    o = slice(0, t)
    local["shape"][o], local["kind"][o] = shapes, kinds
    local["body"][o] = index | np.where(kinematic, np.uint32(capi.KINEMATIC_BIT), np.uint32(0))
    local["a"][o], local["s"][o] = offsets, radii
    local["b"][o] = direction / np.linalg.norm(direction, axis=1, keepdims=True) * lengths
    vo = np.nonzero(local["shape"][:m] == VOXEL)[0]
    local["a"][vo], local["b"][vo], local["s"][vo] = box_lower[vo], box_upper[vo], 0.0
    for k in range(n_planes):  # through the middle of the scene (the body's position), three different normals
        local[t + k] = (PLANE, capi.BV_STATIC, n_kin_bodies | capi.KINEMATIC_BIT, 0, 0, np.eye(3)[k % 3], (0, 0, 0), 0.05 * k, (0, 0, 0))
    id_rng = np.random.default_rng(seed + 2000)
    local["id"] = id_rng.integers(1, 2 ** 63, len(local), dtype=np.uint64)
    local["response"] = id_rng.uniform(0.0, 1.0, (len(local), 3))
    for arr in (local, dyn, kin):
        arr.setflags(write=False)
    return local, dyn, kin


def scene(n, seed=7, n_planes=3, fillers=0):
    """n collidables — spheres, capsules and a few voxel-object boxes (55 / 38 / 7 %) with radii 0.3 .. 0.6, each on a body of its own placed uniformly
    in [0, L]^3, L = max(2, 0.95 n^(1/3)), under a random orientation, a fifth of the bodies kinematic, kinds drawn 60 / 30 / 10 % dynamic / static /
    phantom, and up to three static planes through the middle of the scene LISTED LAST —, then `fillers` isolated dynamic spheres (in front of the
    planes) that meet nothing but the planes -> (local collidables, dynamic bodies, kinematic bodies); cached and read-only"""
    return _scene(int(n), int(seed), int(n_planes), int(fillers))


@functools.lru_cache(maxsize=None)
def scene_reference(n, mode, seed=7, n_planes=3, fillers=0):
    """the restatement's results for the scene -> (world collidables, world boxes, pairs, contacts, deferred pairs); cached and read-only"""
    local, dyn, kin = scene(n, seed, n_planes, fillers)
    world, boxes = transform(local, *body_frames(local, dyn, kin))
    pairs = broad_phase_pairs(boxes, local["kind"], mode)
    contacts, deferred = collide(world, pairs)
    for arr in (world, boxes, pairs, contacts, deferred):
        arr.setflags(write=False)
    return world, boxes, pairs, contacts, deferred


@functools.lru_cache(maxsize=None)
def scene_with_pair_count(target, mode, seed=7):
    """(n, fillers) of a one-plane scene whose broad phase finds exactly `target` pairs under `mode`: the largest n of a short descent whose own pairs do
    not exceed the target, and one isolated sphere (one pair, with the plane) for each pair still missing"""
    n = max(2, min(int(target / 4.0), 500))
    found = len(scene_reference(n, mode, seed, 1, 0)[2])
    n = max(2, int((0.97 if n < 500 else 0.92) * n * target / max(found, 1)))  # (the pair count is close to proportional to n)
    while True:
        found = len(scene_reference(n, mode, seed, 1, 0)[2])
        if found <= target:
            return n, target - found
        n = max(1, min(n - 1, int(n * 0.97)))


# ---- seeded pairs and hand-made cases of the host tests -----------------------------------------------------------------------------------------------
def _world_collidable(shape, a, b=(0, 0, 0), s=0.0, body=0, cid=1, response=(0.5, 0.5, 0.5)):
    c = np.zeros((), dtype=capi.COLLIDABLE_DTYPE)
    c["shape"], c["a"], c["b"], c["s"], c["body"], c["id"], c["response"] = shape, a, b, s, body, cid, response
    return c


def seeded_pairs(shape_a, shape_b, n=2000, seed=5):
    """n world-space pairs of the two shapes around the decision: the second member near the origin, the first at a distance drawn around the sum of
    the two sizes -> (A records, B records)"""
    rng = np.random.default_rng(seed + 16 * shape_a + shape_b)

    def member(shape, centre, k):
        c = np.zeros(k, dtype=capi.COLLIDABLE_DTYPE)
        c["shape"], c["s"] = shape, rng.uniform(0.2, 0.7, k)
        c["id"], c["body"] = rng.integers(1, 2 ** 63, k, dtype=np.uint64), rng.integers(0, 1000, k)
        c["response"] = rng.uniform(0.0, 1.0, (k, 3))
        if shape == PLANE:
            normal = rng.normal(size=(k, 3))
            normal /= np.linalg.norm(normal, axis=1, keepdims=True)
            c["a"] = normal
            c["s"] = (normal * centre).sum(axis=1) + rng.uniform(-0.8, 0.8, k)
        elif shape == CAPSULE:
            v = rng.normal(size=(k, 3))
            v *= rng.uniform(0.1, 1.5, (k, 1)) / np.linalg.norm(v, axis=1, keepdims=True)
            c["a"], c["b"] = centre - 0.5 * v, v
        else:
            c["a"] = centre
        return c

    direction = rng.normal(size=(n, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    second_centre = rng.uniform(-2.0, 2.0, (n, 3))
    return member(shape_a, second_centre + direction * rng.uniform(0.0, 2.2, (n, 1)), n), member(shape_b, second_centre, n)


def hand_made_cases():
    """name -> (A, B) world-space collidables, one for every branch of the five geometries and of the dispatch"""
    S, P, C = SPHERE, PLANE, CAPSULE
    w = _world_collidable
    cases = {
        "coincident sphere centres": (w(S, (1, 2, 3), s=0.5, cid=3), w(S, (1, 2, 3), s=0.25, cid=4)),
        "spheres touching exactly": (w(S, (0, 0, 0), s=0.5, cid=3), w(S, (1, 0, 0), s=0.5, cid=4)),
        "spheres apart": (w(S, (0, 0, 0), s=0.5), w(S, (1.5, 0, 0), s=0.5)),
        "sphere centre on a capsule's segment": (w(C, (0, 0, 0), (2, 0, 0), 0.25, cid=5), w(S, (1, 0, 0), s=0.5, cid=6)),
        "sphere centre on a capsule's segment along y": (w(S, (0, 1, 0), s=0.5, cid=6), w(C, (0, 0, 0), (0, 2, 0), 0.25, cid=5)),
        "sphere on a zero-length capsule": (w(C, (1, 1, 1), (0, 0, 0), 0.25), w(S, (1, 1, 1), s=0.5)),
        "sphere past a capsule's end": (w(C, (0, 0, 0), (1, 0, 0), 0.25), w(S, (1.5, 0.25, 0), s=0.5)),
        "sphere before a capsule's start": (w(S, (-0.5, 0.25, 0), s=0.5), w(C, (0, 0, 0), (1, 0, 0), 0.25)),
        "crossing capsules, A against the normal": (w(C, (0, -0.5, 0.5), (0, 2, -2), 0.25, cid=7), w(C, (-1, 0, 0), (2, 0, 0), 0.25, cid=8)),
        "crossing capsules, A along the normal": (w(C, (0, -0.5, -0.5), (0, 2, 2), 0.25, cid=7), w(C, (-1, 0, 0), (2, 0, 0), 0.25, cid=8)),
        "crossing capsules, A normal to the normal": (w(C, (-1, 0, 0), (2, 0, 0), 0.25), w(C, (0, -1, 0), (0, 2, 0), 0.25)),
        "parallel capsules": (w(C, (0, 0, 0), (1, 0, 0), 0.3), w(C, (0.25, 0, 0.5), (1, 0, 0), 0.3)),
        "antiparallel capsules": (w(C, (0, 0, 0), (1, 0, 0), 0.3), w(C, (1.5, 0, 0.5), (-1, 0, 0), 0.3)),
        "capsules, both segments points": (w(C, (0, 0, 0), (0, 0, 0), 0.3), w(C, (0.25, 0.25, 0), (0, 0, 0), 0.3)),
        "capsules, both segments points, coincident": (w(C, (1, 1, 1), (0, 0, 0), 0.3), w(C, (1, 1, 1), (0, 0, 0), 0.3)),
        "capsules, A's segment a point": (w(C, (1, 0, 0), (0, 0, 0), 0.3), w(C, (0, -1, 0), (0, 2, 0), 0.8)),
        "capsules, B's segment a point": (w(C, (0, 0, 0), (2, 0, 0), 0.3), w(C, (1, 1, 0), (0, 0, 0), 0.8)),
        "capsules, B parameter below 0": (w(C, (0, 0, 0), (1, 0, 0), 0.4), w(C, (0.5, 0.5, 0), (0, 1, 0), 0.4)),
        "capsules, B parameter minus zero": (w(C, (0, 0, 0), (1, 0, 0), 0.4), w(C, (-0.5, 0.0, -0.5), (-0.0, -1, -0.0), 0.4)),
        "capsules, B parameter above 1": (w(C, (0, 0, 0), (1, 0, 0), 0.4), w(C, (0, 2, 0), (0, -1, 0), 0.8)),
        "skew capsules": (w(C, (0, 0, 0), (1, 0, 0), 0.6), w(C, (0.5, 0, 1), (0, 1, 0), 0.6)),
        "capsules touching exactly": (w(C, (0, 0, 0), (1, 0, 0), 0.5), w(C, (0.5, -1, 1), (0, 2, 0), 0.5)),
        "capsules apart": (w(C, (0, 0, 0), (1, 0, 0), 0.25), w(C, (0, 0, 2), (1, 0, 0), 0.25)),
        "sphere on a plane, touching exactly": (w(S, (0, 0, 0.5), s=0.5, cid=9), w(P, (0, 0, 1), s=0.0, cid=10)),
        "sphere just clear of a plane": (w(S, (0, 0, np.nextafter(f32(0.5), f32(1))), s=0.5), w(P, (0, 0, 1), s=0.0)),
        "plane under a sphere (swapped)": (w(P, (0, 0, 1), s=0.25, cid=10), w(S, (3, 4, 0.5), s=0.5, cid=9)),
        "capsule on a plane, start lower": (w(C, (0, 0, 0.25), (1, 0, 1), 0.5), w(P, (0, 0, 1), s=0.0)),
        "capsule on a plane, end lower": (w(C, (0, 0, 1.25), (1, 0, -1), 0.5), w(P, (0, 0, 1), s=0.0)),
        "capsule level on a plane": (w(C, (0, 0, 0.25), (1, 0, 0), 0.5), w(P, (0, 0, 1), s=0.0)),
        "capsule on a plane, touching exactly": (w(C, (0, 0, 0.5), (1, 0, 1), 0.5), w(P, (0, 0, 1), s=0.0)),
        "capsule just clear of a plane": (w(C, (0, 0, np.nextafter(f32(0.5), f32(1))), (1, 0, 1), 0.5), w(P, (0, 0, 1), s=0.0)),
        "plane under a capsule (swapped)": (w(P, (0, 0, 1), s=0.0, cid=11), w(C, (0, 0, 0.25), (1, 0, 1), 0.5, cid=12)),
        "plane against plane": (w(P, (0, 0, 1), s=0.0), w(P, (0, 1, 0), s=0.0)),
        "voxel object against a sphere": (w(VOXEL, (0, 0, 0), (1, 1, 1)), w(S, (0.5, 0.5, 0.5), s=0.5)),
        "plane against a voxel object": (w(P, (0, 0, 1), s=0.0), w(VOXEL, (0, 0, 0), (1, 1, 1))),
    }
    return {name: (np.array(a, dtype=capi.COLLIDABLE_DTYPE), np.array(b, dtype=capi.COLLIDABLE_DTYPE)) for name, (a, b) in cases.items()}
