#!/usr/bin/env python3
"""Everything a world computes, frame by frame, into one file — to compare two builds of the library byte for byte:

    IMPACT_VOXEL_HIP_LIB=/path/to/one.so   python tools/dump_world_state.py one.bin
    IMPACT_VOXEL_HIP_LIB=/path/to/other.so python tools/dump_world_state.py other.bin && cmp one.bin other.bin

Four scenes, each at solver groups 1, 5 and 255 (the chain-stationary solve): the 4^3 pile with every second manifold, all, all, every second
(the contact arrays grow with a previous state to keep); six frames of scenes.pile_churn_frames on the 6^3 pile; an interlocked pair; a 3^3
pile whose bottom layer rests on a moving kinematic body, with positional iterations. Per frame: the dynamic and kinematic bodies, the contact
ids and accumulated impulses, and solver_info()."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from impact_amd import scenes  # noqa: E402
from impact_amd.capi import CONTACT_DTYPE, CONTACT_MANIFOLD_START, KINEMATIC_BIT, KINEMATIC_BODY_DTYPE  # noqa: E402
from impact_amd.physics import ConstraintSolverConfig, PhysicsWorld, uniform_sphere_body  # noqa: E402
from impact_amd.voxel import Context  # noqa: E402


def perturbed_pile(n, seed):
    rng = np.random.default_rng(seed)
    bodies, contacts = scenes.sphere_pile_scene(n)
    bodies["momentum"] += rng.normal(0, 0.05, bodies["momentum"].shape).astype(np.float32)
    bodies["angular_momentum"] += rng.normal(0, 0.01, bodies["angular_momentum"].shape).astype(np.float32)
    return bodies, contacts


def scene_growth():
    bodies, contacts = perturbed_pile(4, 5)
    man = contacts.reshape(-1, 4)
    full, half = np.arange(len(man)), np.arange(0, len(man), 2)
    return bodies, None, [man[k].reshape(-1) for k in (half, full, full, half)], ConstraintSolverConfig()


def scene_churn():
    bodies, contacts = perturbed_pile(6, 7)
    return bodies, None, scenes.pile_churn_frames(contacts, 6), ConstraintSolverConfig()


def scene_interlocked():
    dyn = np.array([uniform_sphere_body(0.5, 1.0, (0, 0.3, 0)), uniform_sphere_body(0.5, 1.0, (0, 0, 0))])
    pts = [(-1.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.1, 1.0), (0.0, -0.1, -1.0)]
    nrm = [(1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1)]
    cs = np.zeros(4, dtype=CONTACT_DTYPE)
    for k in range(4):
        cs[k]["id"], cs[k]["body_a"], cs[k]["body_b"] = 20 + k, 0, 1
        cs[k]["position"], cs[k]["normal"], cs[k]["depth"] = pts[k], nrm[k], 0.1
        cs[k]["restitution"], cs[k]["static_friction"], cs[k]["dynamic_friction"] = 0.5, 0.7, 0.5
        cs[k]["flags"] = CONTACT_MANIFOLD_START if k == 0 else 0
    return dyn, None, [cs, cs], ConstraintSolverConfig()


def scene_kinematic_plane():
    bodies, contacts = perturbed_pile(3, 9)
    kin = np.zeros(1, dtype=KINEMATIC_BODY_DTYPE)
    kin["position"], kin["orientation"], kin["velocity"] = (0, -1.0, 0), (0, 0, 0, 1), (0.05, 0.1, 0)
    kin["angular_axis"], kin["angular_speed"] = (0, 1, 0), 0.2
    lowest = float(bodies["position"][:, 1].min())
    floor = []
    for b in np.flatnonzero(bodies["position"][:, 1] == lowest):
        c = np.zeros(1, dtype=CONTACT_DTYPE)
        c["id"], c["body_a"], c["body_b"] = 1_000_000 + int(b), int(b), KINEMATIC_BIT | 0
        c["position"], c["normal"], c["depth"] = bodies["position"][b] - np.float32([0, 0.5, 0]), (0, 1, 0), 0.02
        c["restitution"], c["static_friction"], c["dynamic_friction"], c["flags"] = 0.4, 0.7, 0.5, CONTACT_MANIFOLD_START
        floor.append(c)
    cs = np.concatenate([contacts] + floor)
    man = contacts.reshape(-1, 4)
    fewer = np.concatenate([man[::2].reshape(-1)] + floor[:-2])
    return bodies, kin, [cs, cs, fewer, cs], ConstraintSolverConfig(6, 0.4, 3, 0.2)


def main(path):
    ctx = Context()
    with open(path, "wb") as f:
        for make in (scene_growth, scene_churn, scene_interlocked, scene_kinematic_plane):
            for groups in (1, 5, 255):
                bodies, kin, frames, cfg = make()
                w = PhysicsWorld(ctx, cfg)
                w.set_bodies(bodies, kin)
                w.set_solver_groups(groups)
                for cs in frames:
                    r = w.perform_physics_step(cs, 0.004)
                    dyn, k = w.bodies()
                    ids, imp = w.contact_state()
                    info = w.solver_info()
                    for a in (dyn, k, ids, imp):
                        f.write(np.ascontiguousarray(a).tobytes())
                    line = f"{make.__name__} groups {groups}: {info} n_bodies {int(r['n_bodies'])} n_levels {[int(x) for x in r['n_levels']]}"
                    f.write(line.encode() + b"\n")
                    print(line)
                w.close()


if __name__ == "__main__":
    main(sys.argv[1])
