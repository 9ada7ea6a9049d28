"""Numpy checker of the force generators and dynamic gravity (impact_amd/csrc/forces.hip): the `apply` functions of the reference's force module and
the composition of `ForceGeneratorManager::apply_forces_and_torques`, in exactly the operation order include/impact_voxel_hip.h states. The
evaluation of a phase works on arrays of generators and in the precision it is asked for: with float32 every intermediate is an np.float32 array
(the restatement the library must equal byte for byte), with float64 it is the float64 version of the same formulas (what the float32 results
are measured against). The sums are made one generator after the other in the reference's order: reset, the phases, the caller's list order
inside a phase, and for gravity the reference's own double loop over the pairs.

acos of a float32 is the C library's double-precision function rounded once, as the library computes it.

It also holds the seeded scenes and the hand-made branch cases of the tests."""
import math

import numpy as np

import motion_ref as mr
from impact_amd import capi, forces
from motion_ref import cross, dot, qrot, scale

f32, f64 = np.float32, np.float64
(CONSTANT_ACCELERATION, LOCAL_FORCE, SPRING_DD, SPRING_DK, ALIGNMENT_FIXED, ALIGNMENT_GRAVITY) = (
    capi.FG_CONSTANT_ACCELERATION, capi.FG_LOCAL_FORCE, capi.FG_SPRING_DYNAMIC_DYNAMIC, capi.FG_SPRING_DYNAMIC_KINEMATIC, capi.FG_ALIGNMENT_FIXED,
    capi.FG_ALIGNMENT_GRAVITY)
KIND_NAMES = ["constant_acceleration", "local_force", "spring_dynamic_dynamic", "spring_dynamic_kinematic", "alignment_fixed", "alignment_gravity"]
EPSILON = f32(np.finfo(f32).eps)
EPS2 = EPSILON * EPSILON                 # normalized_from_and_norm_if_above(.., f32::EPSILON): min_norm.powi(2)
ROTATION_AXIS_MIN2 = f32(1e-8) * f32(1e-8)
GRAVITY_DIRECTION_MIN2 = f32(1e-9) * f32(1e-9)
GRAVITY_EPS = f32(1e-6)
DYNAMIC_FIELDS = ("mass", "inertia", "inv_inertia", "position", "orientation", "momentum", "angular_momentum")
KINEMATIC_FIELDS = ("position", "orientation", "velocity", "angular_axis", "angular_speed")


# ---- arithmetic --------------------------------------------------------------------------------------------------------------------------
def _k(like, v):
    return like.dtype.type(v)


def acos(x):
    return mr._libm(math.acos, x)


def mat_vec(m, v):
    """glam Mat3A::mul_vec3a over column-major [.., 9] matrices"""
    return (scale(m[..., 0:3], v[..., 0]) + scale(m[..., 3:6], v[..., 1])) + scale(m[..., 6:9], v[..., 2])


def mat_mul(a, b):
    return np.concatenate([mat_vec(a, b[..., 0:3]), mat_vec(a, b[..., 3:6]), mat_vec(a, b[..., 6:9])], axis=-1)


def transpose(m):
    return m[..., [0, 3, 6, 1, 4, 7, 2, 5, 8]]


def m3_from_quat(q):
    """glam Mat3A::from_quat, column-major"""
    x, y, z, w = (q[..., i] for i in range(4))
    one = _k(q, 1)
    x2, y2, z2 = x + x, y + y, z + z
    xx, xy, xz, yy, yz, zz, wx, wy, wz = x * x2, x * y2, x * z2, y * y2, y * z2, z * z2, w * x2, w * y2, w * z2
    return np.stack([one - (yy + zz), xy + wz, xz - wy, xy - wz, one - (xx + zz), yz + wx, xz + wy, yz - wx, one - (xx + yy)], axis=-1)


def rotated(m, q):
    """R M R^T (inertia.rs:401-404)"""
    r = m3_from_quat(q)
    return mat_mul(mat_mul(r, m), transpose(r))


def div_recip(v, s):
    return scale(v, _k(v, 1) / s)


def angular_velocity(b):
    """DynamicRigidBody::compute_angular_velocity().as_vector()"""
    w0 = mat_vec(rotated(b["inv_inertia"], b["orientation"]), b["angular_momentum"])
    n2 = dot(w0, w0)
    above = n2 > _k(w0, EPS2)
    n = np.sqrt(np.where(above, n2, _k(w0, 1)))
    return np.where(above[..., None], scale(w0 / n[..., None], n), _k(w0, 0))


def as_arrays(bodies, fields, dtype):
    return {f: np.asarray(bodies[f]).astype(dtype) for f in fields}


def take(b, idx):
    return {f: v[idx] for f, v in b.items()}


# ---- the kinds: b a dict of [m, ..] arrays, p [m, 13] -------------------------------------------------------------------------------------------
def constant_acceleration(b, p):
    return scale(p[:, 0:3], b["mass"])


def force_at(position, force, at):
    """apply_force -> (force, torque about the centre of mass)"""
    return force, cross(at - position, force)


def local_force(b, p):
    q = b["orientation"]
    return force_at(b["position"], qrot(q, p[:, 0:3]), b["position"] + qrot(q, p[:, 3:6]))


def spring(b1, b2, second_is_kinematic, p, diag=None):
    """-> (applies, force_on_2, attachment point 1, attachment point 2)"""
    stiffness, damping, rest_length, slack_length = p[:, 6], p[:, 7], p[:, 8], p[:, 9]
    a1 = b1["position"] + qrot(b1["orientation"], p[:, 0:3])
    a2 = b2["position"] + qrot(b2["orientation"], p[:, 3:6])
    d = a2 - a1
    n2 = dot(d, d)
    applies = n2 > _k(p, EPS2)
    length = np.sqrt(n2)
    direction = d / np.where(applies, length, _k(p, 1))[:, None]
    damped = ~(np.abs(damping) <= _k(p, EPSILON))
    v1 = div_recip(b1["momentum"], b1["mass"]) + cross(angular_velocity(b1), a1 - b1["position"])
    if second_is_kinematic:
        v2 = b2["velocity"] + cross(scale(b2["angular_axis"], b2["angular_speed"]), a2 - b2["position"])
    else:
        v2 = div_recip(b2["momentum"], b2["mass"]) + cross(angular_velocity(b2), a2 - b2["position"])
    rate = np.where(damped, dot(v2, direction) - dot(v1, direction), _k(p, 0))
    slack = length <= slack_length
    scalar = np.where(slack, _k(p, 0), (-stiffness) * (length - rest_length) + (-damping) * rate)
    if diag is not None:
        speed = np.sqrt(dot(v1, v1)) + np.sqrt(dot(v2, v2))
        diag.update(coincident=~applies, undamped=applies & ~damped, slack=applies & slack, plain=applies & damped & ~slack,
                    force_scale=np.abs(stiffness) * (length + np.abs(rest_length)) + np.abs(damping) * speed,
                    arm_1=np.sqrt(dot(a1 - b1["position"], a1 - b1["position"])), arm_2=np.sqrt(dot(a2 - b2["position"], a2 - b2["position"])))
    return applies, scale(direction, scalar), a1, a2


def any_orthonormal(v):
    """glam Vec3A::any_orthonormal_vector"""
    sign = np.copysign(_k(v, 1), v[..., 2])
    a = _k(v, -1) / (sign + v[..., 2])
    b = (v[..., 0] * v[..., 1]) * a
    return np.stack([b, sign + (v[..., 1] * v[..., 1]) * a, -v[..., 1]], axis=-1)


def alignment(b, p, direction, diag=None):
    """the torque towards `direction`"""
    settling_time = p[:, 6]
    spin_frequency, precession_frequency = p[:, 7] / settling_time, p[:, 8] / settling_time
    q = b["orientation"]
    axis = qrot(q, p[:, 0:3])
    c = cross(direction, axis)
    c2 = dot(c, c)
    shortest_arc = c2 > _k(p, ROTATION_AXIS_MIN2)
    rotation_axis = np.where(shortest_arc[:, None], c / np.sqrt(np.where(shortest_arc, c2, _k(p, 1)))[:, None], any_orthonormal(axis))
    inertia = rotated(b["inertia"], q)
    momentum = b["angular_momentum"]
    w = angular_velocity(b)
    speed_rotation = dot(w, rotation_axis)
    w_rotation = scale(rotation_axis, speed_rotation)
    speed_axis = dot(w, axis)
    w_axis = scale(axis, speed_axis)
    w_precession = (w - w_rotation) - w_axis
    cosine = dot(direction, axis)
    angle = acos(np.where(cosine < _k(p, -1), _k(p, -1), np.where(cosine > _k(p, 1), _k(p, 1), cosine)))
    time_constant = _k(p, 0.25) * settling_time
    natural_frequency = _k(p, 1) / time_constant
    critical_damping = _k(p, 2) * natural_frequency
    acceleration_rotation = (-(natural_frequency * natural_frequency)) * angle - critical_damping * speed_rotation
    acceleration = (scale(rotation_axis, acceleration_rotation) - scale(w_axis, spin_frequency)) - scale(w_precession, precession_frequency)
    if diag is not None:
        speed = np.sqrt(dot(w, w))
        diag.update(fallback=~shortest_arc, cosine=cosine,
                    torque_scale=np.abs(inertia).max(axis=1) * (natural_frequency * natural_frequency * math.pi + (critical_damping + np.abs(spin_frequency)
                                                                + np.abs(precession_frequency)) * speed) + speed * np.sqrt(dot(momentum, momentum)))
    return mat_vec(inertia, acceleration) + cross(w, momentum)


def gravity_pair(g, bi, bj):
    """compute_gravitational_force_and_torques (dynamic_gravity.rs:188-231) over arrays of pairs of GravitationalBody (mass, inertia in world space,
    position) -> force_i, torque_i, torque_j"""
    m_i, m_j, imat_i, imat_j = bi["mass"], bj["mass"], bi["inertia"], bj["inertia"]
    eps = _k(m_i, GRAVITY_EPS)
    r_vec = bj["position"] - bi["position"]
    r_squared = dot(r_vec, r_vec)
    r = np.sqrt(r_squared)
    r_cubed = r_squared * r
    r_to_fifth = r_cubed * r_squared
    force_mono = scale(r_vec, ((g * m_i) * m_j) / (r_cubed + eps))
    quad_scale = (_k(m_i, 1.5) * g) / (r_to_fifth + eps)
    a = scale(mat_vec(imat_i, r_vec), m_j)
    b = scale(mat_vec(imat_j, r_vec), m_i)
    s = a + b
    trace_i, trace_j = (imat_i[..., 0] + imat_i[..., 4]) + imat_i[..., 8], (imat_j[..., 0] + imat_j[..., 4]) + imat_j[..., 8]
    radial = (m_j * trace_i + m_i * trace_j) - (_k(m_i, 5) * dot(r_vec, s)) / (r_squared + eps)
    force_quad = scale(scale(r_vec, radial) + scale(s, _k(m_i, 2)), quad_scale)
    torque_scale = _k(m_i, 2) * quad_scale
    return force_mono + force_quad, scale(cross(r_vec, a), torque_scale), scale(cross(r_vec, b), torque_scale)


def gravity_loads(b, g, diag=None):
    """synchronize_bodies + compute_loads (dynamic_gravity.rs:125-159): the reference's double loop over the field's bodies `b` -> [n, 6]"""
    n = len(b["mass"])
    dtype = b["mass"].dtype
    g = dtype.type(f32(g))
    loads = np.zeros((n, 6), dtype=dtype)
    magnitudes = np.zeros((n, 2), dtype=f64)
    if n < 2:
        return loads
    records = {"mass": b["mass"], "inertia": rotated(b["inertia"], b["orientation"]), "position": b["position"]}
    for i in range(n - 1):
        later = np.arange(i + 1, n)
        force_i, torque_i, torque_j = gravity_pair(g, take(records, np.full(n - 1 - i, i)), take(records, later))
        for k in range(n - 1 - i):  # (load_i: one addition after the other)
            loads[i, 0:3] = loads[i, 0:3] + force_i[k]
            loads[i, 3:6] = loads[i, 3:6] + torque_i[k]
        loads[later, 0:3] = loads[later, 0:3] - force_i
        loads[later, 3:6] = loads[later, 3:6] + torque_j
        if diag is not None:
            fm, ti, tj = (np.sqrt(dot(v, v).astype(f64)) for v in (force_i, torque_i, torque_j))
            magnitudes[i] += (fm.sum(), ti.sum())
            magnitudes[later, 0] += fm
            magnitudes[later, 1] += tj
    if diag is not None:
        diag.update(pair_force_sum=magnitudes[:, 0], pair_torque_sum=magnitudes[:, 1])
    return loads


# ---- the composition ---------------------------------------------------------------------------------------------------------------------------
def apply(generators, dynamic, kinematic=(), gravity_bodies=(), gravitational_constant=1.0, dtype=f32, diag=None):
    """ForceGeneratorManager::apply_forces_and_torques (force.rs:130-159) with this library's order inside a phase (the caller's list order) ->
    (a copy of `dynamic` with the new totals, the gravity loads [n_gravity, 6]); with dtype float64 everything is computed in float64 and the
    totals are also returned unrounded in diag["force"], diag["torque"]"""
    gens = np.asarray(generators, dtype=capi.FORCE_GENERATOR_DTYPE).reshape(-1)
    out = np.array(dynamic, dtype=capi.RIGID_BODY_DTYPE, copy=True).reshape(-1)
    kin = np.asarray(kinematic, dtype=capi.KINEMATIC_BODY_DTYPE).reshape(-1) if len(kinematic) else np.zeros(0, dtype=capi.KINEMATIC_BODY_DTYPE)
    field = np.asarray(gravity_bodies, dtype=np.int64).reshape(-1)
    b, k = as_arrays(out, DYNAMIC_FIELDS, dtype), as_arrays(kin, KINEMATIC_FIELDS, dtype)
    n = len(out)
    F, T = np.zeros((n, 3), dtype=dtype), np.zeros((n, 3), dtype=dtype)  # reset_all_forces_and_torques
    diag = {} if diag is None else diag

    def of(kind):
        idx = np.flatnonzero(gens["kind"] == kind)
        return idx, gens["body"][idx].astype(np.int64), gens["body_b"][idx].astype(np.int64), gens["p"][idx].astype(dtype)

    idx, body, _, p = of(CONSTANT_ACCELERATION)
    if idx.size:
        contribution = constant_acceleration(take(b, body), p)
        for j, at in enumerate(body):
            F[at] = F[at] + contribution[j]
    idx, body, _, p = of(LOCAL_FORCE)
    if idx.size:
        force, torque = local_force(take(b, body), p)
        for j, at in enumerate(body):
            F[at], T[at] = F[at] + force[j], T[at] + torque[j]
    for kind in (SPRING_DD, SPRING_DK):
        idx, body, body_b, p = of(kind)
        if not idx.size:
            continue
        b1 = take(b, body)
        b2 = take(k, body_b) if kind == SPRING_DK else take(b, body_b)
        d = diag.setdefault(kind, {})
        applies, force_on_2, a1, a2 = spring(b1, b2, kind == SPRING_DK, p, d)
        f1, t1 = force_at(b1["position"], -force_on_2, a1)
        f2, t2 = force_at(b2["position"], force_on_2, a2)
        for j, at in enumerate(body):
            if applies[j]:
                F[at], T[at] = F[at] + f1[j], T[at] + t1[j]
                if kind == SPRING_DD:
                    F[body_b[j]], T[body_b[j]] = F[body_b[j]] + f2[j], T[body_b[j]] + t2[j]
    loads = gravity_loads(take(b, field), gravitational_constant, diag.setdefault("gravity", {}))
    if field.size >= 2:  # apply_loads
        F[field], T[field] = F[field] + loads[:, 0:3], T[field] + loads[:, 3:6]
    alignments = np.flatnonzero(gens["kind"] >= ALIGNMENT_FIXED)
    if alignments.size:
        body, p = gens["body"][alignments].astype(np.int64), gens["p"][alignments].astype(dtype)
        rank = np.full(n, -1, dtype=np.int64)
        rank[field] = np.arange(field.size)
        fixed = gens["kind"][alignments] == ALIGNMENT_FIXED
        in_field = rank[body] >= 0
        padded = np.concatenate([loads[:, 0:3], np.zeros((1, 3), dtype=dtype)])  # (row -1: a body outside the field)
        load = padded[rank[body]]
        n2 = (load[:, 0] * load[:, 0] + load[:, 1] * load[:, 1]) + load[:, 2] * load[:, 2]
        strong = n2 > _k(p, GRAVITY_DIRECTION_MIN2)
        applies = fixed | (in_field & strong)
        direction = np.where(fixed[:, None], p[:, 3:6], div_recip(load, np.sqrt(np.where(strong, n2, _k(p, 1)))))
        direction = np.where(applies[:, None], direction, np.array([0, 1, 0], dtype=dtype))  # (evaluated and thrown away)
        d = diag.setdefault("alignment", {})
        torque = alignment(take(b, body), p, direction, d)
        d.update(fixed=fixed, not_in_field=~fixed & ~in_field, weak_load=~fixed & in_field & ~strong, applies=applies, generator=alignments)
        for j, at in enumerate(body):
            if applies[j]:
                T[at] = T[at] + torque[j]
    diag.update(force=F.copy(), torque=T.copy())
    out["total_force"], out["total_torque"] = F, T
    return out, loads.astype(f32)


# ---- seeded scenes -------------------------------------------------------------------------------------------------------------------------------
def random_dynamic(rng, n, spread=10.0):
    """n dynamic bodies: masses 0.5-3, a full symmetric inertia tensor with principal moments 0.5-2 in a seeded frame, positions within +-spread,
    momenta and angular momenta within +-3"""
    d = np.zeros(n, dtype=capi.RIGID_BODY_DTYPE)
    d["mass"] = rng.uniform(0.5, 3.0, n)
    frames = m3_from_quat(mr.random_orientations(rng, n).astype(f64)).reshape(n, 3, 3)
    moments = rng.uniform(0.5, 2.0, (n, 3))
    inertia = np.einsum("nij,nj,nkj->nik", frames, moments, frames)
    d["inertia"] = inertia.reshape(n, 9)  # (symmetric: row- and column-major agree)
    d["inv_inertia"] = np.linalg.inv(inertia).reshape(n, 9)
    d["position"], d["orientation"] = rng.uniform(-spread, spread, (n, 3)), mr.random_orientations(rng, n)
    d["momentum"], d["angular_momentum"] = rng.uniform(-3, 3, (n, 3)), rng.uniform(-3, 3, (n, 3))
    d["total_force"], d["total_torque"] = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))  # (host-set totals the stage must overwrite)
    return d


def random_kinematic(rng, n, spread=10.0):
    k = np.zeros(n, dtype=capi.KINEMATIC_BODY_DTYPE)
    k["position"], k["velocity"] = rng.uniform(-spread, spread, (n, 3)), rng.uniform(-10, 10, (n, 3))
    k["orientation"], k["angular_axis"], k["angular_speed"] = mr.random_orientations(rng, n), mr.random_directions(rng, n), rng.uniform(-3, 3, n)
    return k


def spread_positions(rng, n, spread, min_distance):
    """n positions within +-spread, no two closer than min_distance (closer draws are rejected)"""
    out = np.zeros((0, 3))
    while len(out) < n:
        c = rng.uniform(-spread, spread, 3)
        if len(out) == 0 or np.linalg.norm(out - c, axis=1).min() >= min_distance:
            out = np.vstack([out, c])
    return out


def generators(kind, body, body_b, p):
    g = np.zeros(len(p), dtype=capi.FORCE_GENERATOR_DTYPE)
    g["kind"], g["body"], g["body_b"] = kind, body, body_b
    g["p"][:, : p.shape[1]] = p
    return g


def seeded_parameters(kind, m, rng):
    """[m, 13] float32: accelerations and forces within +-20, points within +-2, stiffness 0.1-1000 and damping 0.01-10 (log-uniform; a tenth
    undamped), rest lengths 0-5 (a sixth slack: an elastic band longer than the bodies are apart), settling times 0.05-5, dampings 0-2"""
    p = np.zeros((m, 13), dtype=f32)
    if kind == CONSTANT_ACCELERATION:
        p[:, 0:3] = rng.uniform(-20, 20, (m, 3))
    elif kind == LOCAL_FORCE:
        p[:, 0:3], p[:, 3:6] = rng.uniform(-20, 20, (m, 3)), rng.uniform(-2, 2, (m, 3))
    elif kind in (SPRING_DD, SPRING_DK):
        p[:, 0:3], p[:, 3:6] = rng.uniform(-2, 2, (m, 3)), rng.uniform(-2, 2, (m, 3))
        p[:, 6], p[:, 7] = np.exp(rng.uniform(math.log(0.1), math.log(1000), m)), np.exp(rng.uniform(math.log(0.01), math.log(10), m))
        p[:, 8] = rng.uniform(0, 5, m)
        p[rng.random(m) < 0.1, 7] = 0.0
        band = rng.random(m) < 1 / 6
        p[band, 8] = p[band, 9] = 100.0
    else:
        p[:, 0:3], p[:, 3:6] = mr.random_directions(rng, m), mr.random_directions(rng, m)
        p[:, 6], p[:, 7], p[:, 8] = np.exp(rng.uniform(math.log(0.05), math.log(5), m)), rng.uniform(0, 2, m), rng.uniform(0, 2, m)
        if kind == ALIGNMENT_GRAVITY:
            p[:, 3:6] = 0
    return p


def seeded_scene(kind, m, seed):
    """m generators of `kind`, one per dynamic body (a dynamic-dynamic spring: bodies 2 i and 2 i + 1), with the branches of the kind seeded in:
    a twelfth of the springs between coincident attachment points; an eighth of the fixed alignments with the axis already along the direction
    and an eighth against it. -> dict(generators, dynamic, kinematic)"""
    assert kind != ALIGNMENT_GRAVITY
    rng = np.random.default_rng(seed * 16 + kind)
    n_dyn = 2 * m if kind == SPRING_DD else m
    dyn, kin = random_dynamic(rng, n_dyn), random_kinematic(rng, m if kind == SPRING_DK else 0)
    p = seeded_parameters(kind, m, rng)
    body, body_b = np.arange(m), np.zeros(m, dtype=np.int64)
    if kind == SPRING_DD:
        body, body_b = 2 * np.arange(m), 2 * np.arange(m) + 1
    if kind in (SPRING_DD, SPRING_DK):
        coincide = np.flatnonzero(rng.random(m) < 1 / 12)
        other = kin if kind == SPRING_DK else dyn
        at_b = coincide if kind == SPRING_DK else body_b[coincide]
        other["position"][at_b], other["orientation"][at_b] = dyn["position"][body[coincide]], dyn["orientation"][body[coincide]]
        p[coincide, 3:6] = p[coincide, 0:3]
        if kind == SPRING_DK:
            body_b = np.arange(m)
    if kind == ALIGNMENT_FIXED:
        u = rng.random(m)
        axis = qrot(dyn["orientation"], p[:, 0:3])  # (float32, the library's own arithmetic: the cross product is exactly zero)
        p[u < 1 / 8, 3:6] = axis[u < 1 / 8]
        p[u > 7 / 8, 3:6] = -axis[u > 7 / 8]
    return {"generators": generators(kind, body, body_b, p), "dynamic": dyn, "kinematic": kin, "field": np.zeros(0, dtype=np.uint32), "g": 1.0}


def seeded_gravity_alignment_scenes(m, seed, group=50, members=40):
    """m gravity-alignment generators in scenes of `group` bodies each, one generator per body: `members` of them form the field (shuffled), the
    rest are outside it; every fourth scene has a gravitational constant of 1e-13, which leaves every load below the 1e-9 the reference asks
    of a direction"""
    rng = np.random.default_rng(seed * 16 + ALIGNMENT_GRAVITY)
    scenes = []
    for s in range(m // group):
        dyn = random_dynamic(rng, group)
        dyn["position"] = spread_positions(rng, group, 10.0, 1.0)
        p = seeded_parameters(ALIGNMENT_GRAVITY, group, rng)
        field = rng.permutation(group)[:members].astype(np.uint32)
        scenes.append({"generators": generators(ALIGNMENT_GRAVITY, np.arange(group), 0, p), "dynamic": dyn, "kinematic": random_kinematic(rng, 0), "field": field,
                       "g": 1e-13 if s % 4 == 3 else 1.0})
    return scenes


def gravity_scene(n, seed, every=1):
    """a field of n bodies in a box that keeps the number density (about one body per 2^3), no two closer than 1: the members are every
    `every`-th dynamic body, in shuffled order when `every` > 1"""
    rng = np.random.default_rng(seed * 1000 + n)
    dyn = random_dynamic(rng, n * every)
    dyn["position"] = spread_positions(rng, n * every, max(2.0, (n * every) ** (1 / 3)), 1.0)
    field = np.arange(0, n * every, every, dtype=np.uint32)
    if every > 1:
        field = rng.permutation(field).astype(np.uint32)
    return {"generators": np.zeros(0, dtype=capi.FORCE_GENERATOR_DTYPE), "dynamic": dyn, "kinematic": random_kinematic(rng, 0), "field": field, "g": 0.75}


def run(scene, dtype=f32, diag=None):
    return apply(scene["generators"], scene["dynamic"], scene["kinematic"], scene["field"], scene["g"], dtype, diag)


def run_host(scene):
    return forces.apply_host(scene["generators"], scene["dynamic"], scene["kinematic"], scene["field"], scene["g"])


# ---- hand-made branch cases ------------------------------------------------------------------------------------------------------------------------
def hand_made():
    """(name, scene, what the restatement's diagnostics must show) for every branch the header names"""
    rng = np.random.default_rng(7)
    dyn, kin = random_dynamic(rng, 3, spread=3.0), random_kinematic(rng, 1, spread=3.0)
    z3, pt = [0.0, 0.0, 0.0], [0.3, -0.2, 0.5]
    cases = []

    def case(name, gens, d=dyn, k=kin, field=(), g=1.0):
        cases.append((name, {"generators": np.array(gens, dtype=capi.FORCE_GENERATOR_DTYPE).reshape(-1), "dynamic": d, "kinematic": k,
                             "field": np.asarray(field, dtype=np.uint32), "g": g}))

    same = dyn.copy()
    same["position"][1], same["orientation"][1] = same["position"][0], same["orientation"][0]
    same_kin = kin.copy()
    same_kin["position"][0], same_kin["orientation"][0] = dyn["position"][0], dyn["orientation"][0]
    case("spring dd between coincident points", [forces.spring_dynamic_dynamic(0, pt, 1, pt, forces.standard_spring(5.0, 0.5, 1.0))], d=same)
    case("spring dk between coincident points", [forces.spring_dynamic_kinematic(0, pt, 0, pt, forces.standard_spring(5.0, 0.5, 1.0))], k=same_kin)
    case("spring dd undamped", [forces.spring_dynamic_dynamic(0, pt, 1, z3, forces.standard_spring(5.0, 0.0, 1.0))])
    case("spring dd damping at epsilon", [forces.spring_dynamic_dynamic(0, pt, 1, z3, forces.standard_spring(5.0, float(EPSILON), 1.0))])
    case("spring dd damping just above epsilon", [forces.spring_dynamic_dynamic(0, pt, 1, z3, forces.standard_spring(5.0, float(np.nextafter(EPSILON, f32(1))), 1.0))])
    case("spring dk undamped", [forces.spring_dynamic_kinematic(2, pt, 0, z3, forces.standard_spring(5.0, 0.0, 1.0))])
    case("spring dd slack band", [forces.spring_dynamic_dynamic(0, pt, 1, z3, forces.elastic_band(5.0, 0.5, 50.0))])
    case("spring dk slack band", [forces.spring_dynamic_kinematic(0, pt, 0, z3, forces.elastic_band(5.0, 0.5, 50.0))])
    case("spring dd taut band", [forces.spring_dynamic_dynamic(0, pt, 1, z3, forces.elastic_band(5.0, 0.5, 0.01))])
    case("spring dk damped", [forces.spring_dynamic_kinematic(1, pt, 0, pt, forces.standard_spring(50.0, 2.0, 0.5))])
    local_axis = mr.random_directions(rng, 1)[0]
    axis = qrot(dyn["orientation"][0:1], local_axis[None])[0]
    case("alignment parallel fallback", [forces.alignment_fixed(0, local_axis, axis, 0.5, 0.3, 0.2)])
    case("alignment antiparallel fallback", [forces.alignment_fixed(0, local_axis, -axis, 0.5, 0.3, 0.2)])
    ident = dyn.copy()
    ident["orientation"][0] = (0, 0, 0, 1)
    case("alignment fallback about -z", [forces.alignment_fixed(0, [0, 0, -1], [0, 0, 1], 0.5, 0.3, 0.2)], d=ident)
    case("alignment plain", [forces.alignment_fixed(0, local_axis, mr.random_directions(rng, 1)[0], 0.5, 0.3, 0.2)])
    case("gravity alignment outside the field", [forces.alignment_gravity(2, local_axis, 0.5, 0.3, 0.2)], field=[0, 1])
    case("gravity alignment in the field", [forces.alignment_gravity(1, local_axis, 0.5, 0.3, 0.2)], field=[0, 1, 2])
    case("gravity alignment under a negligible load", [forces.alignment_gravity(1, local_axis, 0.5, 0.3, 0.2)], field=[0, 1, 2], g=1e-13)
    case("gravity alignment in a field of one", [forces.alignment_gravity(1, local_axis, 0.5, 0.3, 0.2)], field=[1])
    case("gravity alignment without a field", [forces.alignment_gravity(1, local_axis, 0.5, 0.3, 0.2)])
    case("coincident gravity bodies", [], d=same, field=[0, 1, 2])
    case("gravity field of one", [forces.constant_acceleration(1, [0, -9.81, 0])], field=[1])
    case("gravity field of two", [], field=[2, 0])
    case("every kind on one body in reverse phase order", [
        forces.alignment_gravity(1, local_axis, 0.7, 0.1, 0.4), forces.alignment_fixed(1, local_axis, [0, 1, 0], 0.5, 0.3, 0.2),
        forces.spring_dynamic_kinematic(1, pt, 0, z3, forces.standard_spring(3.0, 0.2, 0.5)), forces.spring_dynamic_dynamic(0, pt, 1, z3, forces.standard_spring(5.0, 0.5, 1.0)),
        forces.local_force(1, [1, 2, 3], pt), forces.constant_acceleration(1, [0, -9.81, 0]), forces.spring_dynamic_dynamic(1, z3, 2, pt, forces.elastic_band(4.0, 0.0, 0.2))],
        field=[2, 1, 0])
    return cases
