"""Numpy checker of the motion drivers (impact_amd/csrc/motion.hip): the five `compute_*` functions of the reference's driven_motion module and
the composition rule of `MotionDriverManager::apply_motion`, in exactly the operation order include/impact_voxel_hip.h states. Every function
works on arrays of cases ([m, 14] parameters, [m] times) and in the precision of its inputs: handed float32 arrays every intermediate is an
np.float32 array (the restatement the library must equal byte for byte), handed float64 arrays it is the float64 version of the same
trajectory with the exact 2 pi and pi (what the float32 results are measured against).

sin, cos and tan of a float32 are the C library's double-precision functions rounded once, as the library computes them; the float64 version
calls the same functions. `%` is fmod (exact in either precision).

It also holds the seeded drivers and the hand-made branch cases of the tests."""
import math

import numpy as np

from impact_amd import capi

f32, f64 = np.float32, np.float64
CIRCULAR, CONSTANT_ACCELERATION, HARMONIC, ORBITAL, CONSTANT_ROTATION = (capi.MD_CIRCULAR, capi.MD_CONSTANT_ACCELERATION, capi.MD_HARMONIC, capi.MD_ORBITAL,
                                                                         capi.MD_CONSTANT_ROTATION)
KIND_NAMES = ["circular", "constant_acceleration", "harmonic", "orbital", "constant_rotation"]
TWO_PI32, PI32 = f32(6.2831855), f32(3.1415927)


# ---- arithmetic --------------------------------------------------------------------------------------------------------------------------
def _k(like, v):
    """the constant v in the precision of `like`"""
    return like.dtype.type(v)


def two_pi(like):
    return TWO_PI32 if like.dtype == f32 else f64(2.0 * math.pi)


def pi(like):
    return PI32 if like.dtype == f32 else f64(math.pi)


def _libm(fn, x):
    """the C library's double-precision fn of every element, rounded once to the precision of x"""
    flat = np.asarray(x).reshape(-1)
    return np.array([fn(float(v)) for v in flat], dtype=f64).reshape(np.shape(x)).astype(x.dtype)


def sin(x):
    return _libm(math.sin, x)


def cos(x):
    return _libm(math.cos, x)


def tan(x):
    return _libm(math.tan, x)


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


def qmul(a, b):
    """glam Quat::mul_quat (xyzw)"""
    ax, ay, az, aw = (a[..., i] for i in range(4))
    bx, by, bz, bw = (b[..., i] for i in range(4))
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def vec(x, y):
    return np.stack([x, y, np.zeros_like(x)], axis=-1)


# ---- the five kinds: p [m, 14], t [m] ----------------------------------------------------------------------------------------------------------
def circular(p, t, diag=None):
    """circular.rs:134-194 -> position, velocity"""
    q, center, radius, period = p[:, 1:5], p[:, 5:8], p[:, 8], p[:, 9]
    w = two_pi(p) / period
    angle = np.fmod(w * (t - p[:, 0]), two_pi(p))
    s, c = sin(angle), cos(angle)
    position = center + qrot(q, vec(radius * c, radius * s))
    v = radius * w
    if diag is not None:
        diag["angle"] = angle
    return position, qrot(q, vec(-v * s, v * c))


def constant_acceleration(p, t, diag=None):
    """constant_acceleration.rs:143-157"""
    dt = t - p[:, 0]
    p0, v0, acc = p[:, 1:4], p[:, 4:7], p[:, 7:10]
    return (p0 + scale(v0, dt)) + scale(acc, _k(p, 0.5) * (dt * dt)), v0 + scale(acc, dt)


def harmonic(p, t, diag=None):
    """harmonic_oscillation.rs:139-159"""
    dt = t - p[:, 0]
    center, direction, amplitude = p[:, 1:4], p[:, 4:7], p[:, 7]
    w = two_pi(p) / p[:, 8]
    return center + scale(direction, amplitude * sin(w * dt)), scale(direction, (amplitude * w) * cos(w * dt))


def eccentric_anomaly(e, mean_anomaly):
    """orbit.rs:243-269 -> (E, Newton iterations)"""
    ecc = mean_anomaly.copy()
    error = np.full_like(ecc, np.inf)
    iterations = np.zeros(ecc.shape, dtype=np.int64)
    for _ in range(100):
        live = error > _k(ecc, f32(1e-4))
        if not live.any():
            break
        x, ee, m = ecc[live], e[live], mean_anomaly[live]
        nxt = x - ((x - ee * sin(x)) - m) / (_k(x, 1) - ee * cos(x))
        error[live] = np.abs(nxt - x)
        ecc[live] = nxt
        iterations[live] += 1
    return ecc, iterations


def orbital(p, t, diag=None):
    """orbit.rs:149-365"""
    one = _k(p, 1)
    q, focus, a, e, period = p[:, 1:5], p[:, 5:8], p[:, 8], p[:, 9], p[:, 10]
    n = two_pi(p) / period
    mean_anomaly = np.fmod(n * (t - p[:, 0]), two_pi(p))
    ecc, iterations = eccentric_anomaly(e, mean_anomaly)
    f2 = (one + e) / (one - e)
    f = np.sqrt(f2)
    th = tan(_k(p, 0.5) * ecc)
    th2 = th * th
    tv2 = f2 * th2
    k = one / (one + tv2)
    cos_v = (one - tv2) * k
    dv_de = (f * (one + th2)) * k
    r = (a * (one - e * e)) / (one + e * cos_v)
    root = np.sqrt(one - cos_v * cos_v)
    sin_v = np.where(ecc <= pi(p), root, -root)
    position = focus + qrot(q, vec(r * cos_v, r * sin_v))
    dv = (n * dv_de) / (one - e * cos(ecc))
    den = one + e * cos_v
    vr = ((((dv * e) * a) * (one - e * e)) * sin_v) / (den * den)
    vt = r * dv
    if diag is not None:
        diag.update(mean_anomaly=mean_anomaly, eccentric_anomaly=ecc, iterations=iterations, sin_v=sin_v)
    return position, qrot(q, vec(vr * cos_v - vt * sin_v, vr * sin_v + vt * cos_v))


def advance_orientation(q, axis, speed, duration):
    """rigid_body.rs:1020-1034"""
    angle = speed * duration
    s, co = sin(_k(q, 0.5) * angle), cos(_k(q, 0.5) * angle)
    im = scale(axis, s)
    r = qmul(np.concatenate([im, co[..., None]], axis=-1), q)
    length = np.sqrt(((r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]) + r[..., 3] * r[..., 3])
    return r / length[..., None]


def constant_rotation(p, t, diag=None):
    """constant_rotation.rs:111-120 -> orientation, axis, angular speed"""
    axis, speed = p[:, 5:8], p[:, 8]
    return advance_orientation(p[:, 1:5], axis, speed, t - p[:, 0]), axis, speed


TRAJECTORIES = {CIRCULAR: circular, CONSTANT_ACCELERATION: constant_acceleration, HARMONIC: harmonic, ORBITAL: orbital}


def evaluate(kind, p, t, diag=None):
    """`ivx_md_eval` over m drivers of one kind -> [m, 10] in the precision of p"""
    p, t = np.atleast_2d(p), np.atleast_1d(t).astype(np.asarray(p).dtype)
    out = np.zeros((p.shape[0], 10), dtype=p.dtype)
    if kind == CONSTANT_ROTATION:
        q, axis, speed = constant_rotation(p, t, diag)
        out[:, 0:4], out[:, 4:7], out[:, 7] = q, axis, speed
    else:
        out[:, 0:3], out[:, 3:6] = TRAJECTORIES[kind](p, t, diag)
    return out


def apply(drivers, bodies, time, dtype=f32):
    """MotionDriverManager::apply_motion (driven_motion.rs:50-82) with this library's order inside a kind (the caller's list order) -> a copy of
    `bodies` (KINEMATIC_BODY_DTYPE; with dtype float64 the sums are made in float64 and rounded at the end)"""
    drivers = np.asarray(drivers, dtype=capi.MOTION_DRIVER_DTYPE).reshape(-1)
    out = np.array(bodies, dtype=capi.KINEMATIC_BODY_DTYPE, copy=True).reshape(-1)
    t = np.array([time], dtype=dtype)
    trajectory_kinds = (CIRCULAR, CONSTANT_ACCELERATION, HARMONIC, ORBITAL)
    for b in sorted(set(int(x) for x in drivers["body"][np.isin(drivers["kind"], trajectory_kinds)])):
        position, velocity = np.zeros(3, dtype=dtype), np.zeros(3, dtype=dtype)
        for kind in trajectory_kinds:
            for d in drivers[(drivers["body"] == b) & (drivers["kind"] == kind)]:
                o = evaluate(kind, d["p"].astype(dtype)[None], t)[0]
                position, velocity = position + o[0:3], velocity + o[3:6]
        out["position"][b], out["velocity"][b] = position, velocity
    for d in drivers[drivers["kind"] == CONSTANT_ROTATION]:
        o = evaluate(CONSTANT_ROTATION, d["p"].astype(dtype)[None], t)[0]
        b = int(d["body"])
        out["orientation"][b], out["angular_axis"][b], out["angular_speed"][b] = o[0:4], o[4:7], o[7]
    return out


# ---- seeded drivers: the reference's own proptest ranges -------------------------------------------------------------------------------------------
def random_orientations(rng, m):
    """orientation_strategy: extrinsic Euler angles y in [0, 2 pi), x in [-pi/2, pi/2), z in [0, 2 pi), as a unit quaternion in float32"""
    def axis_angle(axis, angle):
        q = np.zeros((m, 4))
        q[:, axis], q[:, 3] = np.sin(0.5 * angle), np.cos(0.5 * angle)
        return q
    qy, qx, qz = axis_angle(1, rng.uniform(0, 2 * math.pi, m)), axis_angle(0, rng.uniform(-math.pi / 2, math.pi / 2, m)), axis_angle(2, rng.uniform(0, 2 * math.pi, m))
    q = qmul(qz, qmul(qx, qy))
    return (q / np.linalg.norm(q, axis=1)[:, None]).astype(f32)


def random_directions(rng, m):
    """direction_strategy: phi in [0, 2 pi), theta in [0, pi), normalised in float32"""
    phi, theta = rng.uniform(0, 2 * math.pi, m), rng.uniform(0, math.pi, m)
    d = np.stack([np.cos(phi) * np.sin(theta), np.sin(phi) * np.sin(theta), np.cos(theta)], axis=-1).astype(f32)
    return d / np.sqrt(dot(d, d))[:, None]


def seeded(kind, m, seed):
    """m drivers of `kind` and a time for each: times within +-10, periods 0.1-100, radii and axes 0.01-100, eccentricities 0-0.9, positions within
    +-100 (log-uniform where a range spans decades) -> (p [m, 14] float32, t [m] float32)"""
    rng = np.random.default_rng(seed * 16 + kind)
    p = np.zeros((m, 14), dtype=f32)
    def log_uniform(lo, hi):
        return np.exp(rng.uniform(math.log(lo), math.log(hi), m))
    p[:, 0] = rng.uniform(-10, 10, m)
    t = rng.uniform(-10, 10, m).astype(f32)
    if kind == CIRCULAR:
        p[:, 1:5], p[:, 5:8], p[:, 8], p[:, 9] = random_orientations(rng, m), rng.uniform(-100, 100, (m, 3)), log_uniform(0.01, 100), log_uniform(0.1, 100)
    elif kind == CONSTANT_ACCELERATION:
        p[:, 1:4], p[:, 4:7], p[:, 7:10] = rng.uniform(-100, 100, (m, 3)), rng.uniform(-100, 100, (m, 3)), rng.uniform(-100, 100, (m, 3))
    elif kind == HARMONIC:
        p[:, 1:4], p[:, 4:7], p[:, 7], p[:, 8] = rng.uniform(-100, 100, (m, 3)), random_directions(rng, m), rng.uniform(-100, 100, m), log_uniform(0.1, 100)
    elif kind == ORBITAL:
        p[:, 1:5], p[:, 5:8], p[:, 8] = random_orientations(rng, m), rng.uniform(-100, 100, (m, 3)), log_uniform(0.01, 100)
        p[:, 9], p[:, 10] = rng.uniform(0, 0.9, m), log_uniform(0.1, 100)
    else:
        p[:, 1:5], p[:, 5:8], p[:, 8] = random_orientations(rng, m), random_directions(rng, m), rng.uniform(-100, 100, m)
    return p, t


def records(kind, p, body=0):
    d = np.zeros(len(p), dtype=capi.MOTION_DRIVER_DTYPE)
    d["kind"], d["body"], d["p"] = kind, body, p
    return d


def scales(kind, p, t):
    """the scene's scale of every case, in float64: (length, speed) the errors of position and velocity are measured against"""
    p, t = p.astype(f64), t.astype(f64)
    if kind == CIRCULAR:
        return np.maximum(np.abs(p[:, 5:8]).max(axis=1), p[:, 8]), p[:, 8] * 2 * math.pi / np.abs(p[:, 9])
    if kind == CONSTANT_ACCELERATION:
        dt = np.abs(t - p[:, 0])
        speed = np.abs(p[:, 4:7]).max(axis=1) + dt * np.abs(p[:, 7:10]).max(axis=1)
        return np.abs(p[:, 1:4]).max(axis=1) + dt * speed, speed
    if kind == HARMONIC:
        return np.maximum(np.abs(p[:, 1:4]).max(axis=1), np.abs(p[:, 7])), np.abs(p[:, 7]) * 2 * math.pi / np.abs(p[:, 8])
    if kind == ORBITAL:
        a, e = p[:, 8], p[:, 9]
        return np.maximum(np.abs(p[:, 5:8]).max(axis=1), a * (1 + e)), a * (2 * math.pi / np.abs(p[:, 10])) * np.sqrt((1 + e) / (1 - e))
    return np.ones(len(p)), np.ones(len(p))
