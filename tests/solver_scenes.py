"""Scenes of turned anisotropic bodies for the contact-solver tests (test_solver_ref_cpu.py, test_gpu_solver_bodies.py): every body comes
from `physics_util.anisotropic_body` (full body-frame inertia, random orientation, angular velocity of order 1 rad/s). A scene is a dict:
dyn, kin (or None), config, dt, frames (one contact list per step, fixed in space: computed from the bodies' initial positions)."""
import numpy as np

import physics_util as pu
import solver_ref
from impact_amd.capi import CONTACT_DTYPE, KINEMATIC_BIT, KINEMATIC_BODY_DTYPE

f32 = np.float32
DEFAULT = (8, 0.4, 3, 0.2)
# the small graphs that are also held to the float64 restatement: 8-14 bodies, manifolds of 1-9 contacts; seeds picked on the CPU out of
# 0..499 for at least 12 contacts in every frame and the margin rule of test_solver_ref_cpu.py with room to spare (6 seeds qualified)
SMALL_GRAPH = dict(n_range=(8, 14), longest_manifold=9)
SMALL_GRAPH_SEEDS = [207, 360, 391, 398]
PULL = 40.0 # acceleration per unit distance towards the origin that keeps the bodies of the larger scenes in contact from frame to frame


def contact(cid, a, b, position, normal, depth, restitution, mu_s=0.0, mu_d=0.0, first=True):
    c = np.zeros((), dtype=CONTACT_DTYPE)
    c["id"], c["body_a"], c["body_b"] = cid, a, b
    c["position"], c["normal"], c["depth"] = position, normal, depth
    c["restitution"], c["static_friction"], c["dynamic_friction"] = restitution, mu_s, mu_d
    c["flags"] = 1 if first else 0
    return c


def _unit(v):
    return v / np.linalg.norm(v)


def _omega(body):
    """angular velocity of a dynamic body record: R I^-1 R^T L"""
    inverse = solver_ref.rotated(solver_ref.column_major(body["inv_inertia"]), body["orientation"].astype(np.float64))
    return inverse @ body["angular_momentum"].astype(np.float64)


def _point_velocity(body, point, kinematic=False):
    disp = np.asarray(point, dtype=np.float64) - body["position"].astype(np.float64)
    if kinematic:
        return body["velocity"].astype(np.float64) + np.cross(float(body["angular_speed"]) * body["angular_axis"].astype(np.float64), disp)
    return body["momentum"].astype(np.float64) / float(body["mass"]) + np.cross(_omega(body), disp)


def _set_point_velocity(body, point, velocity):
    """the momentum that gives the dynamic body's material point at `point` the velocity `velocity` (its spin stays)"""
    disp = np.asarray(point, dtype=np.float64) - body["position"].astype(np.float64)
    body["momentum"] = ((velocity - np.cross(_omega(body), disp)) * float(body["mass"])).astype(f32)


def _tilted_normal(rng, about=(0.0, 1.0, 0.0), tilt=0.3):
    return _unit(np.asarray(about) + rng.normal(0, tilt, 3)).astype(f32)


def _tangent(rng, n):
    t = np.cross(n.astype(np.float64), rng.normal(size=3))
    return _unit(t)


def moving_kinematic(rng, position=(0.0, -0.6, 0.0)):
    """a kinematic body that is turned, moves and spins"""
    k = np.zeros(1, dtype=KINEMATIC_BODY_DTYPE)
    k["position"] = position
    k["orientation"] = _unit(rng.normal(size=4)).astype(f32)
    k["velocity"] = (0.3, 0.1, -0.2)
    k["angular_axis"] = _unit(rng.normal(size=3)).astype(f32)
    k["angular_speed"] = 0.8
    return k


def pair_scene(seed, approach, slide=0.0, restitution=0.0, mu=(0.0, 0.0), depth=0.01, n_contacts=1, push=8.0, frames=2, config=DEFAULT,
               kinematic=None):
    """Body A above body B, `n_contacts` contacts of one manifold between them at a tilted normal, off the line of centres. A's momentum is
    set so that at the (first) contact point A closes in on B at `approach` along the normal and slips at `slide` along a random tangent;
    a constant force of `push` * mass presses A against B (0: none; 100: enough to close the contact again in the frame after a bounce).
    kinematic = "b": B is a moving, spinning kinematic body; "a": the same pair given in the other order (the kinematic body is body A of
    the contact, the normal turned round)."""
    rng = np.random.default_rng(seed)
    top = pu.anisotropic_body(rng, (0.0, 0.6, 0.0))
    n = _tilted_normal(rng)
    points = [np.array([rng.uniform(-0.25, 0.25), rng.uniform(-0.05, 0.05), rng.uniform(-0.25, 0.25)]).astype(f32) for _ in range(n_contacts)]
    if kinematic:
        kin = moving_kinematic(rng)
        dyn = np.array([top])
        under = _point_velocity(kin[0], points[0], kinematic=True)
    else:
        kin = None
        bottom = pu.anisotropic_body(rng, (0.0, -0.6, 0.0), velocity=rng.normal(0, 0.2, 3))
        dyn = np.array([top, bottom])
        under = _point_velocity(bottom, points[0])
    _set_point_velocity(dyn[0], points[0], under - approach * n.astype(np.float64) + slide * _tangent(rng, n))
    dyn["total_force"][0] = (-push * float(dyn[0]["mass"]) * n.astype(np.float64)).astype(f32)
    a, b, normal = (0, 1, n) if not kinematic else (0, KINEMATIC_BIT | 0, n) if kinematic == "b" else (KINEMATIC_BIT | 0, 0, -n)
    cs = np.array([contact(100 + j, a, b, points[j], normal, f32(depth * (1.0 - 0.2 * j)), restitution, mu[0], mu[1], first=(j == 0))
                   for j in range(n_contacts)])
    return {"dyn": dyn, "kin": kin, "config": config, "dt": 0.004, "frames": [cs] * frames}


def chain_scene(seed, frames=3):
    """three bodies in a row, the middle one in both contacts (once as body B, once as body A), friction on one of them"""
    rng = np.random.default_rng(seed)
    dyn = np.array([pu.anisotropic_body(rng, (0.0, y, 0.0), velocity=rng.normal(0, 0.2, 3)) for y in (1.2, 0.0, -1.2)])
    cs = []
    for k, (a, b, y) in enumerate(((0, 1, 0.6), (1, 2, -0.6))):
        n = _tilted_normal(rng)
        p = np.array([rng.uniform(-0.2, 0.2), y, rng.uniform(-0.2, 0.2)]).astype(f32)
        mover, other, sign = (a, b, 1.0) if k == 0 else (b, a, -1.0)  # the outer body closes in on the middle one
        rel = -1.0 * n.astype(np.float64) + 0.3 * _tangent(rng, n)
        _set_point_velocity(dyn[mover], p, _point_velocity(dyn[other], p) + sign * rel)
        dyn["total_force"][mover] = (-sign * 100.0 * float(dyn[mover]["mass"]) * n.astype(np.float64)).astype(f32)
        cs.append(contact(200 + k, a, b, p, n, f32(0.02), 0.3, 0.7 * k, 0.5 * k))
    return {"dyn": dyn, "kin": None, "config": DEFAULT, "dt": 0.004, "frames": [np.array(cs)] * frames}


def closed_scenes():
    """section (a): two or three bodies, a few contacts each; name -> scene (seeds picked so that every decision of the float64 restatement
    keeps the margin test_solver_ref_cpu.py asserts)"""
    return {
        "bounce": pair_scene(101, approach=1.5, restitution=0.6),                        # above the restitution threshold
        "rest": pair_scene(102, approach=0.2, restitution=0.6),                          # below it: the target velocity is 0
        "separating": pair_scene(103, approach=-2.0, restitution=0.5, depth=-0.01, push=0.0),  # zero impulse, nothing to correct
        "stick": pair_scene(104, approach=2.0, slide=0.3, mu=(1.0, 0.9), frames=3),      # inside the friction circle; static from frame 2
        "slide": pair_scene(105, approach=0.5, slide=2.0, mu=(0.3, 0.2)),                # on the friction circle
        "manifold": pair_scene(124, approach=1.0, slide=0.5, restitution=0.3, mu=(0.7, 0.5), n_contacts=4, frames=3, push=100.0),
        "chain": chain_scene(107),
        "kinematic_b": pair_scene(108, approach=1.0, slide=0.4, restitution=0.3, mu=(0.7, 0.5), kinematic="b", frames=3, push=100.0),
        "kinematic_a": pair_scene(109, approach=1.0, slide=0.4, restitution=0.3, mu=(0.7, 0.5), kinematic="a", frames=3, push=100.0),
        "deep": pair_scene(110, approach=0.5, mu=(0.7, 0.5), depth=0.4),                 # positional correction turns the bodies
    }


def random_graph_scene(seed, n_range=(8, 60), longest_manifold=9, frames=5):
    """section (b): the generator of test_gpu_physics_random.test_random_graphs_on_several_workgroups with anisotropic bodies in place of
    the spheres: irregular chains, manifolds of 1..`longest_manifold` contacts, pairs in either order, a kinematic plane that is turned, moves
    and spins, contact sets that change from frame to frame. `groups` is the workgroup count the seed draws for the tile kernel."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(n_range[0], n_range[1], endpoint=True))
    pos = rng.uniform(-3.0, 3.0, (n, 3)).astype(f32)
    dyn = np.array([pu.anisotropic_body(rng, pos[i], velocity=rng.normal(0, 0.3, 3)) for i in range(n)])
    dyn["total_force"] = (-PULL * dyn["mass"][:, None] * pos).astype(f32)
    plane = moving_kinematic(rng, (0.0, 0.0, 0.0))
    plane["angular_speed"], plane["velocity"] = 0.3, (0.05, 0.0, -0.02)
    groups = int(rng.integers(2, 17))
    n_pairs = int(rng.integers(4, 3 * n))
    pairs = []
    for k in range(n_pairs):
        a = int(rng.integers(0, n))
        b = (KINEMATIC_BIT | 0) if rng.random() < 0.2 else int(rng.integers(0, n))
        if b == a:
            b = KINEMATIC_BIT | 0
        if rng.random() < 0.3 and not (b & KINEMATIC_BIT):
            a, b = b, a
        pairs.append((a, b, int(rng.integers(1, longest_manifold + 1)), rng.random() < 0.5))
    alive = rng.random(n_pairs) < 0.8
    lists = []
    for frame in range(frames):
        cs = []
        for k in rng.permutation(n_pairs):
            if not alive[k]:
                continue
            a, b, m, frictional = pairs[k]
            pa = pos[a].astype(np.float64)
            pb = np.array([pa[0], 0.0, pa[2]]) if (b & KINEMATIC_BIT) else pos[b].astype(np.float64)
            nrm = pa - pb
            nrm = nrm / np.linalg.norm(nrm) if np.linalg.norm(nrm) > 1e-6 else np.array([0.0, 1.0, 0.0])
            mid = 0.5 * (pa + pb)
            for j in range(m):
                cs.append(contact(int(k) * 16 + j, a, b, (mid + rng.normal(0, 0.1, 3)).astype(f32), nrm.astype(f32), f32(rng.uniform(-0.01, 0.05)),
                                  float(rng.uniform(0, 0.8)), 0.6 if frictional else 0.0, 0.4 if frictional else 0.0, first=(j == 0)))
        lists.append(np.array(cs) if cs else np.zeros(0, dtype=CONTACT_DTYPE))
        alive = np.where(rng.random(n_pairs) < 0.25, ~alive, alive)
    return {"dyn": dyn, "kin": plane, "config": DEFAULT, "dt": 0.004, "frames": lists, "groups": groups}


def anisotropic_pile(config, seed=7):
    """section (c): the contacts of `scenes.sphere_pile_scene(3)` between 27 anisotropic bodies with perturbed momenta; three frames, the
    middle one without every other manifold"""
    from impact_amd import scenes

    rng = np.random.default_rng(seed)
    spheres, contacts = scenes.sphere_pile_scene(3)
    dyn = np.array([pu.anisotropic_body(rng, s["position"], velocity=rng.normal(0, 0.05, 3), mass=float(s["mass"])) for s in spheres])
    dyn["total_force"] = spheres["total_force"]
    manifolds = contacts.reshape(-1, 4)
    half = manifolds[::2].reshape(-1).copy()
    return {"dyn": dyn, "kin": None, "config": config, "dt": 0.004, "frames": [contacts, half, contacts]}


def sparse_scene(n_dyn, seed=3):
    """section (d): `n_dyn` dynamic and two kinematic bodies, about 20 contacts that constrain body 0, body n_dyn - 1 and kinematic body 1
    and leave most bodies free; two frames"""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-3.0, 3.0, (n_dyn, 3)).astype(f32)
    dyn = np.array([pu.anisotropic_body(rng, pos[i], velocity=rng.normal(0, 0.3, 3)) for i in range(n_dyn)])
    kin = np.concatenate([moving_kinematic(rng, (0.0, -4.0, 0.0)), moving_kinematic(rng, (0.0, 4.0, 0.0))])
    last = n_dyn - 1
    pairs = [(0, last), (0, KINEMATIC_BIT | 1), (KINEMATIC_BIT | 1, last), (last, 5), (7, 0), (11, 12), (12, KINEMATIC_BIT | 0)]
    cs = []
    for k, (a, b) in enumerate(pairs):
        pa = (kin[a & 0x7FFFFFFF] if a & KINEMATIC_BIT else dyn[a])["position"].astype(np.float64)
        pb = (kin[b & 0x7FFFFFFF] if b & KINEMATIC_BIT else dyn[b])["position"].astype(np.float64)
        nrm = _unit(pa - pb)
        for j in range(3):
            cs.append(contact(k * 16 + j, a, b, (0.5 * (pa + pb) + rng.normal(0, 0.1, 3)).astype(f32), nrm.astype(f32), f32(rng.uniform(0.0, 0.05)),
                              float(rng.uniform(0, 0.8)), 0.6 * (k % 2), 0.4 * (k % 2), first=(j == 0)))
    cs = np.array(cs)
    constrained = sorted({r for a, b in pairs for r in (a, b) if not r & KINEMATIC_BIT})
    # (forces on the constrained bodies only: the free bodies' momenta stay as they are)
    dyn["total_force"][constrained] = (-PULL * dyn["mass"][constrained, None] * pos[constrained]).astype(f32)
    return {"dyn": dyn, "kin": kin, "config": DEFAULT, "dt": 0.004, "frames": [cs, cs[3:]], "constrained": constrained}
