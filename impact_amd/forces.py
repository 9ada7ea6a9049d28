"""Host-side mirror of the force-generator calls (`ivx_world_set_force_generators`, `ivx_world_set_dynamic_gravity`, `ivx_world_apply_forces`,
`ivx_world_gravity_loads`, `ivx_fg_apply_host`; impact_amd/csrc/forces.hip): the reference's `ForceGeneratorManager`
(impact_physics/src/force.rs) for the dynamic bodies of a `PhysicsWorld`:

  ConstantAcceleration                   force/constant_acceleration.rs:96-102  (`constant_acceleration`)
  LocalForce                             force/local_force.rs:37-62             (`local_force`)
  DynamicDynamicSpringForceProperties    force/spring_force.rs:140-189          (`spring_dynamic_dynamic`, with `spring` / `standard_spring` / `elastic_band`)
  DynamicKinematicSpringForceProperties  force/spring_force.rs:191-243          (`spring_dynamic_kinematic`)
  FixedDirectionAlignmentTorque          force/alignment_torque.rs:107-241      (`alignment_fixed`)
  GravityAlignmentTorque                 the same, AlignmentDirection::GravityForce  (`alignment_gravity`)
  DynamicGravityManager                  force/dynamic_gravity.rs:103-231       (`ForceGenerators.set_gravity`, `gravity_loads`)
  apply_forces_and_torques               force.rs:130-159                       (`ForceGenerators.apply`, and the tail of every `PhysicsWorld.step`)

`body` indexes the world's dynamic bodies; an anchor is given resolved, as body index plus body-space point. With a set or a field installed every
step of the world ends with the force stage, which resets the totals of all dynamic bodies first. Nothing here computes, and nothing falls back
to the CPU.
"""
from __future__ import annotations

import numpy as np

from . import capi
from .capi import FORCE_GENERATOR_DTYPE, KINEMATIC_BODY_DTYPE, RIGID_BODY_DTYPE, check, ptr


def _generator(kind, body, body_b, fields) -> np.ndarray:
    g = np.zeros((), dtype=FORCE_GENERATOR_DTYPE)
    g["kind"], g["body"], g["body_b"] = kind, body, body_b
    for at, f in fields:
        v = np.asarray(f, dtype=np.float32).reshape(-1)
        g["p"][at : at + v.size] = v
    return g


def constant_acceleration(body, acceleration) -> np.ndarray:
    return _generator(capi.FG_CONSTANT_ACCELERATION, body, 0, [(0, acceleration)])


def local_force(body, force, point) -> np.ndarray:
    """a force fixed in the body's frame, applied at a point of that frame"""
    return _generator(capi.FG_LOCAL_FORCE, body, 0, [(0, force), (3, point)])


def spring(stiffness, damping, rest_length, slack_length):
    """`Spring::new`"""
    return (stiffness, damping, rest_length, slack_length)


def standard_spring(stiffness, damping, rest_length):
    """`Spring::standard`: no slack"""
    return spring(stiffness, damping, rest_length, 0.0)


def elastic_band(stiffness, damping, slack_length):
    """`Spring::elastic_band`: slack below its rest length"""
    return spring(stiffness, damping, slack_length, slack_length)


def spring_dynamic_dynamic(body_1, attachment_point_1, body_2, attachment_point_2, spring) -> np.ndarray:
    return _generator(capi.FG_SPRING_DYNAMIC_DYNAMIC, body_1, body_2, [(0, attachment_point_1), (3, attachment_point_2), (6, spring)])


def spring_dynamic_kinematic(body_1, attachment_point_1, kinematic_body_2, attachment_point_2, spring) -> np.ndarray:
    """`kinematic_body_2` indexes the kinematic bodies, without the IVX_KINEMATIC_BODY bit"""
    return _generator(capi.FG_SPRING_DYNAMIC_KINEMATIC, body_1, kinematic_body_2, [(0, attachment_point_1), (3, attachment_point_2), (6, spring)])


def alignment_fixed(body, axis_to_align, alignment_direction, settling_time, spin_damping, precession_damping) -> np.ndarray:
    return _generator(capi.FG_ALIGNMENT_FIXED, body, 0, [(0, axis_to_align), (3, alignment_direction), (6, (settling_time, spin_damping, precession_damping))])


def alignment_gravity(body, axis_to_align, settling_time, spin_damping, precession_damping) -> np.ndarray:
    return _generator(capi.FG_ALIGNMENT_GRAVITY, body, 0, [(0, axis_to_align), (6, (settling_time, spin_damping, precession_damping))])


def _records(generators):
    if len(generators) == 0:
        return np.zeros(0, dtype=FORCE_GENERATOR_DTYPE)
    return np.ascontiguousarray(generators, dtype=FORCE_GENERATOR_DTYPE).reshape(-1)


def _or_null(a):
    return ptr(a) if a.size else None


def apply_host(generators, dynamic_bodies, kinematic_bodies=(), gravity_bodies=(), gravitational_constant=1.0):
    """`ivx_fg_apply_host`: the whole stage over copies of host bodies, the code the kernels run -> (dynamic bodies, gravity loads [n_gravity, 6])"""
    g = _records(generators)
    d = np.array(dynamic_bodies, dtype=RIGID_BODY_DTYPE, copy=True).reshape(-1)
    k = np.ascontiguousarray(kinematic_bodies, dtype=KINEMATIC_BODY_DTYPE).reshape(-1) if len(kinematic_bodies) else np.zeros(0, dtype=KINEMATIC_BODY_DTYPE)
    field = np.ascontiguousarray(gravity_bodies, dtype=np.uint32).reshape(-1)
    loads = np.zeros((field.size, 6), dtype=np.float32)
    check(capi.lib().ivx_fg_apply_host(_or_null(g), g.size, _or_null(field), field.size, float(gravitational_constant), _or_null(d), d.size, _or_null(k), k.size,
                                       _or_null(loads)))
    return d, loads


class ForceGenerators:
    """The generator set and the gravity field of a `PhysicsWorld`."""

    def __init__(self, physics_world):
        self.world = physics_world
        self.n = 0
        self.n_gravity = 0

    def set(self, generators) -> None:
        """`ivx_world_set_force_generators`: replaces the set (an empty list removes it); call it after `PhysicsWorld.set_bodies`"""
        g = _records(generators)
        check(capi.lib().ivx_world_set_force_generators(self.world.h, _or_null(g), g.size))
        self.n = g.size

    def clear(self) -> None:
        self.set([])

    def set_gravity(self, dynamic_bodies, gravitational_constant=1.0) -> None:
        """`ivx_world_set_dynamic_gravity`: the field's members in order (an empty list removes the field)"""
        field = np.ascontiguousarray(dynamic_bodies, dtype=np.uint32).reshape(-1)
        check(capi.lib().ivx_world_set_dynamic_gravity(self.world.h, _or_null(field), field.size, float(gravitational_constant)))
        self.n_gravity = field.size

    def apply(self) -> None:
        """`ivx_world_apply_forces`: the stage on its own, enqueued (primes the totals before the first step)"""
        check(capi.lib().ivx_world_apply_forces(self.world.h))

    def gravity_loads(self) -> np.ndarray:
        """`ivx_world_gravity_loads`: [n_gravity, 6] force and torque on every field member as of the last apply; waits for the stream"""
        loads = np.zeros((self.n_gravity, 6), dtype=np.float32)
        check(capi.lib().ivx_world_gravity_loads(self.world.h, _or_null(loads), self.n_gravity))
        return loads
