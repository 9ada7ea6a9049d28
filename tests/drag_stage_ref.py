"""Numpy checker of the drag phase of the force stage (impact_amd/csrc/forces.hip, fg_drag): `DetailedDragForce::apply` with
`DragLoad::compute_world_space_drag_force_and_torque` in exactly the operation order include/impact_voxel_hip.h states, over arrays of generators
and in the precision it is asked for — with float32 every intermediate is an np.float32 (the restatement the library must equal byte for byte),
with float64 it is the float64 version of the same formulas. The composition calls forces_ref.py for the phases ahead of drag and for the
evaluation of gravity and the alignment torques, and puts the drag phase where the reference has it: behind the dynamic-kinematic springs, ahead
of dynamic gravity.

atan2 and acos of a float32 are the C library's double-precision functions rounded once, as the library computes them.

It also holds the seeded scenes with the hand-made edge bodies of the tests."""
import math

import numpy as np

import forces_ref as fr
from impact_amd import capi, forces
from motion_ref import dot, qrot, scale

f32, f64 = np.float32, np.float64
PI32, TWO_PI32 = f32(3.14159265358979323846), f32(6.28318530717958647692)  # PI_F, TWO_PI_F of drag_internal.hpp


def _k(like, v):
    return like.dtype.type(v)


def atan2(y, x):
    flat_y, flat_x = np.asarray(y, dtype=f64).reshape(-1), np.asarray(x, dtype=f64).reshape(-1)
    return np.array([math.atan2(a, b) for a, b in zip(flat_y, flat_x)], dtype=f64).reshape(np.shape(y)).astype(y.dtype)


def random_map(rng, n_theta):
    m = np.zeros((n_theta, 2 * n_theta), dtype=capi.DRAG_LOAD_DTYPE)
    m["force"], m["torque"] = rng.normal(size=(n_theta, 2 * n_theta, 3)), rng.normal(size=(n_theta, 2 * n_theta, 3))
    return m


def medium_of(medium):
    """-> (mass density, velocity[3]) as float32 from a forces.UniformMedium, a record or None (the vacuum)"""
    r = forces._medium_record(medium)[0]
    return f32(r["mass_density"]), np.array(r["velocity"], dtype=f32)


# ---- the phase: b a dict of [m, ..] arrays (the body of every generator), gens [m] DRAG_GENERATOR_DTYPE ---------------------------------------------
def drag(b, gens, maps, medium, diag=None):
    """-> (applies [m], force [m, 3], torque [m, 3]) in the dtype of `b`"""
    like = b["mass"]
    rho32, vm32 = medium_of(medium)
    rho, vm = like.dtype.type(rho32), vm32.astype(like.dtype)
    coefficient, scaling = gens["drag_coefficient"].astype(like.dtype), gens["scaling"].astype(like.dtype)
    pi, two_pi = (PI32, TWO_PI32) if like.dtype == f32 else (f64(math.pi), f64(2.0 * math.pi))
    v_rel = fr.div_recip(b["momentum"], b["mass"]) - vm
    s2 = dot(v_rel, v_rel)
    moving = s2 > _k(like, 0)
    q = b["orientation"]
    conjugate = q * np.array([-1, -1, -1, 1], dtype=like.dtype)
    d = fr.div_recip(qrot(conjugate, v_rel), np.sqrt(np.where(moving, s2, _k(like, 1))))
    applies = moving & np.isfinite(d).all(axis=1)
    d = np.where(applies[:, None], d, np.array([1, 0, 0], dtype=like.dtype))  # (evaluated and thrown away)
    phi = atan2(d[:, 1], d[:, 0])
    z = d[:, 2]
    theta = fr.acos(np.where(z < _k(like, -1), _k(like, -1), np.where(z > _k(like, 1), _k(like, 1), z)))
    n_theta = np.array([maps[s].shape[0] for s in gens["map"]], dtype=np.int64)
    cell = pi / n_theta.astype(like.dtype)
    inv_cell = _k(like, 1) / cell
    # phi_idx_of / theta_idx_of
    rem = np.fmod(phi, two_pi)
    wrapped = rem < _k(like, 0)
    rem = np.where(wrapped, rem + two_pi, rem)
    phi_cells = rem * inv_cell
    t = np.fmod(theta, two_pi)
    t = np.where(t < _k(like, 0), t + two_pi, t)
    folded = t > pi
    t = np.where(folded, two_pi - t, t)
    theta_cells = t * inv_cell

    def index(cells, n):
        f = np.floor(cells)
        return np.minimum(np.where(f > 0, f, 0).astype(np.int64), n - 1), f > (n - 1)

    phi_idx, phi_clamped = index(phi_cells, 2 * n_theta)
    theta_idx, theta_clamped = index(theta_cells, n_theta)
    load_force = np.array([maps[s]["force"][ti, pj] for s, ti, pj in zip(gens["map"], theta_idx, phi_idx)], dtype=f32).reshape(-1, 3).astype(like.dtype)
    load_torque = np.array([maps[s]["torque"][ti, pj] for s, ti, pj in zip(gens["map"], theta_idx, phi_idx)], dtype=f32).reshape(-1, 3).astype(like.dtype)
    fs = (((scaling * scaling) * rho) * coefficient) * s2
    ts = scaling * fs
    force, torque = scale(qrot(q, load_force), fs), scale(qrot(q, load_torque), ts)
    if diag is not None:
        diag.update(moving=moving, at_rest=s2 == 0, applies=applies, wrapped=applies & wrapped, folded=applies & folded, phi_clamped=applies & phi_clamped,
                    theta_clamped=applies & theta_clamped, phi_cells=phi_cells, theta_cells=theta_cells, phi_idx=phi_idx, theta_idx=theta_idx, n_theta=n_theta,
                    force_scale=np.abs(fs) * np.sqrt(dot(load_force, load_force)), torque_scale=np.abs(ts) * np.sqrt(dot(load_torque, load_torque)),
                    force=force, torque=torque)
    return applies, force, torque


# ---- the composition ---------------------------------------------------------------------------------------------------------------------------
def apply(generators, dynamic, kinematic=(), gravity_bodies=(), gravitational_constant=1.0, drag_generators=(), maps=(), medium=None, dtype=f32, diag=None,
          drag_after_gravity=False):
    """ForceGeneratorManager::apply_forces_and_torques with the drag phase -> (a copy of `dynamic` with the new totals, the gravity loads). With dtype
    float64 the totals are also returned unrounded in diag["force"], diag["torque"]. drag_after_gravity: the WRONG order, for the test that tells
    the two apart."""
    gens = forces._records(generators)
    dg = forces._drag_records(drag_generators)
    field = np.asarray(gravity_bodies, dtype=np.int64).reshape(-1)
    diag = {} if diag is None else diag
    # reset, constant accelerations, local forces, both springs: forces_ref's composition over the generators of those kinds
    head = {}
    out, _ = fr.apply(gens[gens["kind"] < fr.ALIGNMENT_FIXED], dynamic, kinematic, (), gravitational_constant, dtype, head)
    F, T = head["force"], head["torque"]
    b = fr.as_arrays(out, fr.DYNAMIC_FIELDS, dtype)
    n = len(out)

    def drag_phase():
        if not dg.size:
            return
        body = dg["body"].astype(np.int64)
        d = diag.setdefault("drag", {})
        applies, force, torque = drag(fr.take(b, body), dg, maps, medium, d)
        for j, at in enumerate(body):  # (list order; several generators may name one body)
            if applies[j]:
                F[at], T[at] = F[at] + force[j], T[at] + torque[j]

    if not drag_after_gravity:
        drag_phase()
    loads = fr.gravity_loads(fr.take(b, field), gravitational_constant, diag.setdefault("gravity", {}))
    if field.size >= 2:  # apply_loads
        F[field], T[field] = F[field] + loads[:, 0:3], T[field] + loads[:, 3:6]
    if drag_after_gravity:
        drag_phase()
    alignments = np.flatnonzero(gens["kind"] >= fr.ALIGNMENT_FIXED)
    if alignments.size:  # (forces_ref.apply's own tail)
        body, p = gens["body"][alignments].astype(np.int64), gens["p"][alignments].astype(dtype)
        rank = np.full(n, -1, dtype=np.int64)
        rank[field] = np.arange(field.size)
        fixed = gens["kind"][alignments] == fr.ALIGNMENT_FIXED
        in_field = rank[body] >= 0
        padded = np.concatenate([loads[:, 0:3], np.zeros((1, 3), dtype=dtype)])
        load = padded[rank[body]]
        n2 = (load[:, 0] * load[:, 0] + load[:, 1] * load[:, 1]) + load[:, 2] * load[:, 2]
        strong = n2 > _k(p, fr.GRAVITY_DIRECTION_MIN2)
        applies = fixed | (in_field & strong)
        direction = np.where(fixed[:, None], p[:, 3:6], fr.div_recip(load, np.sqrt(np.where(strong, n2, _k(p, 1)))))
        direction = np.where(applies[:, None], direction, np.array([0, 1, 0], dtype=dtype))
        torque = fr.alignment(fr.take(b, body), p, direction)
        for j, at in enumerate(body):
            if applies[j]:
                T[at] = T[at] + torque[j]
    diag.update(force=F.copy(), torque=T.copy())
    out["total_force"], out["total_torque"] = F, T
    return out, loads.astype(f32)


# ---- seeded scenes -------------------------------------------------------------------------------------------------------------------------------
N_EDGE = 120  # bodies of every hand-made kind in a seeded scene
SLOTS = (0, 2, 3)  # (slot 1 of the table stays empty)


def seeded_scene(n_theta, medium, seed, m=2000):
    """m detailed-drag generators over maps of n_theta rows in three slots of a table of four, in shuffled list order. The bodies: seeded random
    ones, and with identity orientation and a power of two as mass, so that their velocity relative to `medium` is exact, N_EDGE each of
      at rest in the medium                     momentum = mass * medium velocity
      moving along +z and along -z              (theta 0 and pi: the last row is reached by the clamp)
      in the xy-plane at multiples of the cell  phi = j * cell, j = 0 .. 2 n_theta - 1 in turn
      phi just below zero                       v_rel = (1, -1e-30, 0): the remainder rounds to 2 pi, the index is clamped
    Every 25th of the random bodies carries two generators. -> dict(drag, dynamic, maps, medium, random: mask over the generators)"""
    rng = np.random.default_rng(seed * 1000 + n_theta)
    _, vm = medium_of(medium)
    n_random = (m - 5 * N_EDGE) * 25 // 26
    n_dyn = n_random + 5 * N_EDGE
    dyn = fr.random_dynamic(rng, n_dyn)
    edge = slice(n_random, n_dyn)
    dyn["orientation"][edge] = (0, 0, 0, 1)
    mass = f32(2.0) ** rng.integers(-1, 3, 5 * N_EDGE).astype(f32)
    cell = PI32 / f32(n_theta)
    j = np.arange(N_EDGE) % (2 * n_theta)
    speed = f32(2.0) ** rng.integers(-1, 3, N_EDGE).astype(f32)
    v_edge = np.zeros((5 * N_EDGE, 3), dtype=f32)
    v_edge[1 * N_EDGE:2 * N_EDGE, 2] = speed
    v_edge[2 * N_EDGE:3 * N_EDGE, 2] = -speed
    v_edge[3 * N_EDGE:4 * N_EDGE, 0], v_edge[3 * N_EDGE:4 * N_EDGE, 1] = speed * np.cos(j * cell, dtype=f32), speed * np.sin(j * cell, dtype=f32)
    v_edge[4 * N_EDGE:5 * N_EDGE] = (1.0, -1e-30, 0.0)
    exact = np.r_[0:3 * N_EDGE, 4 * N_EDGE:5 * N_EDGE]
    v = v_edge.copy()
    v[exact] = v_edge[exact] + vm  # (small integers and powers of two: exact; the tiny y of the last kind survives only in a medium at rest along y)
    v[3 * N_EDGE:4 * N_EDGE] = v_edge[3 * N_EDGE:4 * N_EDGE] + vm
    dyn["mass"][edge] = mass
    dyn["momentum"][edge] = v * mass[:, None]
    maps = [random_map(rng, n_theta), None, random_map(rng, n_theta), random_map(rng, n_theta)]
    body = np.concatenate([np.arange(n_dyn), rng.choice(n_random, m - n_dyn, replace=False)])
    order = rng.permutation(m)
    body = body[order]
    gens = np.zeros(m, dtype=capi.DRAG_GENERATOR_DTYPE)
    gens["body"], gens["map"] = body, rng.choice(SLOTS, m)
    gens["drag_coefficient"], gens["scaling"] = rng.uniform(0.1, 2.0, m), rng.uniform(0.5, 2.0, m)
    return {"drag": gens, "dynamic": dyn, "maps": maps, "medium": medium, "random": body < n_random}


def run(scene, dtype=f32, diag=None, generators=(), kinematic=(), field=(), g=1.0):
    return apply(generators, scene["dynamic"], kinematic, field, g, scene["drag"], scene["maps"], scene["medium"], dtype, diag)


def run_host(scene, generators=(), kinematic=(), field=(), g=1.0):
    return forces.apply_host(generators, scene["dynamic"], kinematic, field, g, drag=scene["drag"], maps=scene["maps"], medium=scene["medium"])
