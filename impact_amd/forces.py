"""Host-side mirror of the force-generator calls (`ivx_world_set_force_generators`, `ivx_world_set_dynamic_gravity`, `ivx_world_apply_forces`,
`ivx_world_gravity_loads`, `ivx_fg_apply_host`, and for detailed drag `ivx_world_set_medium`, `ivx_world_set_drag_map`, `ivx_world_set_drag_map_from_grid`,
`ivx_world_drag_map_download`, `ivx_world_set_detailed_drag`, `ivx_fg_apply_host_drag`; impact_amd/csrc/forces.hip): the reference's `ForceGeneratorManager`
(impact_physics/src/force.rs) for the dynamic bodies of a `PhysicsWorld`:

  ConstantAcceleration                   force/constant_acceleration.rs:96-102  (`constant_acceleration`)
  LocalForce                             force/local_force.rs:37-62             (`local_force`)
  DynamicDynamicSpringForceProperties    force/spring_force.rs:140-189          (`spring_dynamic_dynamic`, with `spring` / `standard_spring` / `elastic_band`)
  DynamicKinematicSpringForceProperties  force/spring_force.rs:191-243          (`spring_dynamic_kinematic`)
  FixedDirectionAlignmentTorque          force/alignment_torque.rs:107-241      (`alignment_fixed`)
  GravityAlignmentTorque                 the same, AlignmentDirection::GravityForce  (`alignment_gravity`)
  DynamicGravityManager                  force/dynamic_gravity.rs:103-231       (`ForceGenerators.set_gravity`, `gravity_loads`)
  DetailedDragForce                      force/detailed_drag.rs:200-243         (`detailed_drag`, `ForceGenerators.set_drag`, with `UniformMedium` and map slots)
  apply_forces_and_torques               force.rs:130-159                       (`ForceGenerators.apply`, and the tail of every `PhysicsWorld.step`)

`body` indexes the world's dynamic bodies; an anchor is given resolved, as body index plus body-space point. With a set or a field installed every
step of the world ends with the force stage, which resets the totals of all dynamic bodies first. Drag load maps are resident in the world, in
numbered slots (the reference's `DragLoadMapID` -> slot is the caller's mapping); a detailed-drag generator names a body and a slot. Nothing here computes, and nothing falls back
to the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import (DRAG_GENERATOR_DTYPE, DRAG_LOAD_DTYPE, DRAG_MAP_VIEW_DTYPE, FORCE_GENERATOR_DTYPE, KINEMATIC_BODY_DTYPE, RIGID_BODY_DTYPE, UNIFORM_MEDIUM_DTYPE, check,
                   ptr)


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


class UniformMedium:
    """`UniformMedium` (medium.rs:11-68): a mass density and a velocity, the same everywhere"""

    SEA_LEVEL_AIR_MASS_DENSITY = 1.2
    WATER_MASS_DENSITY = 1e3

    def __init__(self, mass_density=0.0, velocity=(0.0, 0.0, 0.0)):
        self.mass_density = float(mass_density)
        self.velocity = tuple(float(v) for v in velocity)

    @classmethod
    def vacuum(cls):
        return cls(0.0)

    @classmethod
    def still_air(cls):
        return cls.moving_air((0.0, 0.0, 0.0))

    @classmethod
    def moving_air(cls, velocity):
        return cls(cls.SEA_LEVEL_AIR_MASS_DENSITY, velocity)

    @classmethod
    def still_water(cls):
        return cls.moving_water((0.0, 0.0, 0.0))

    @classmethod
    def moving_water(cls, velocity):
        return cls(cls.WATER_MASS_DENSITY, velocity)

    def record(self) -> np.ndarray:
        r = np.zeros((), dtype=UNIFORM_MEDIUM_DTYPE)
        r["mass_density"], r["velocity"] = self.mass_density, self.velocity
        return r

    @classmethod
    def from_record(cls, r):
        return cls(float(r["mass_density"]), [float(v) for v in np.asarray(r["velocity"]).reshape(3)])


def _medium_record(medium) -> np.ndarray:
    if medium is None:
        medium = UniformMedium.vacuum()
    r = medium.record() if isinstance(medium, UniformMedium) else np.asarray(medium, dtype=UNIFORM_MEDIUM_DTYPE)
    return np.ascontiguousarray(r).reshape(1)


def detailed_drag(body, map_slot, drag_coefficient, scaling=1.0) -> np.ndarray:
    """`DetailedDragForce` on dynamic body `body`, its drag load map in slot `map_slot` of the world's table"""
    g = np.zeros((), dtype=DRAG_GENERATOR_DTYPE)
    g["body"], g["map"], g["drag_coefficient"], g["scaling"] = body, map_slot, drag_coefficient, scaling
    return g


def _drag_records(generators):
    if generators is None or len(generators) == 0:
        return np.zeros(0, dtype=DRAG_GENERATOR_DTYPE)
    return np.ascontiguousarray(generators, dtype=DRAG_GENERATOR_DTYPE).reshape(-1)


def _map_loads(m):
    """a map as [n_theta, 2 n_theta] records of DRAG_LOAD_DTYPE, from an array or a `drag.DragLoadMap`"""
    loads = np.ascontiguousarray(getattr(m, "loads", m), dtype=DRAG_LOAD_DTYPE)
    assert loads.ndim == 2 and loads.shape[1] == 2 * loads.shape[0], "a drag load map is n_theta x 2 n_theta"
    return loads


def _records(generators):
    if len(generators) == 0:
        return np.zeros(0, dtype=FORCE_GENERATOR_DTYPE)
    return np.ascontiguousarray(generators, dtype=FORCE_GENERATOR_DTYPE).reshape(-1)


def _or_null(a):
    return ptr(a) if a.size else None


def apply_host(generators, dynamic_bodies, kinematic_bodies=(), gravity_bodies=(), gravitational_constant=1.0, drag=None, maps=None, medium=None):
    """`ivx_fg_apply_host`: the whole stage over copies of host bodies, the code the kernels run -> (dynamic bodies, gravity loads [n_gravity, 6]).
    With any of `drag` (detailed-drag generators), `maps` (the slot table: a list of maps, None for an empty slot) or `medium` given it is
    `ivx_fg_apply_host_drag`, the stage with the drag phase."""
    g = _records(generators)
    d = np.array(dynamic_bodies, dtype=RIGID_BODY_DTYPE, copy=True).reshape(-1)
    k = np.ascontiguousarray(kinematic_bodies, dtype=KINEMATIC_BODY_DTYPE).reshape(-1) if len(kinematic_bodies) else np.zeros(0, dtype=KINEMATIC_BODY_DTYPE)
    field = np.ascontiguousarray(gravity_bodies, dtype=np.uint32).reshape(-1)
    loads = np.zeros((field.size, 6), dtype=np.float32)
    if drag is None and maps is None and medium is None:
        check(capi.lib().ivx_fg_apply_host(_or_null(g), g.size, _or_null(field), field.size, float(gravitational_constant), _or_null(d), d.size, _or_null(k), k.size,
                                           _or_null(loads)))
        return d, loads
    dg = _drag_records(drag)
    held = [None if m is None else _map_loads(m) for m in (maps or ())]  # (kept alive through the call)
    views = np.zeros(len(held), dtype=DRAG_MAP_VIEW_DTYPE)
    for i, m in enumerate(held):
        if m is not None:
            views[i] = (m.ctypes.data, m.shape[0], 0)
    med = _medium_record(medium)
    check(capi.lib().ivx_fg_apply_host_drag(_or_null(g), g.size, _or_null(field), field.size, float(gravitational_constant), _or_null(d), d.size, _or_null(k), k.size,
                                            _or_null(loads), _or_null(dg), dg.size, _or_null(views), views.size, ptr(med)))
    return d, loads


class ForceGenerators:
    """The generator set, the gravity field and the detailed-drag set of a `PhysicsWorld`, with the world's medium and its drag load maps."""

    def __init__(self, physics_world):
        self.world = physics_world
        self.n = 0
        self.n_gravity = 0
        self.n_drag = 0

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

    # ---- detailed drag: the medium and the maps belong to the world and outlive the sets -----------------------------------------------------
    def set_medium(self, medium) -> None:
        """`ivx_world_set_medium`: a `UniformMedium` (a new world has the vacuum); takes effect at the next apply"""
        check(capi.lib().ivx_world_set_medium(self.world.h, ptr(_medium_record(medium))))

    def medium(self) -> UniformMedium:
        r = np.zeros(1, dtype=UNIFORM_MEDIUM_DTYPE)
        check(capi.lib().ivx_world_medium(self.world.h, ptr(r)))
        return UniformMedium.from_record(r[0])

    def set_drag_map(self, slot, drag_load_map) -> None:
        """`ivx_world_set_drag_map`: a host map ([n_theta, 2 n_theta] DRAG_LOAD_DTYPE or a `drag.DragLoadMap`) into slot `slot`; None frees the slot"""
        if drag_load_map is None:
            check(capi.lib().ivx_world_set_drag_map(self.world.h, int(slot), None, 0))
            return
        loads = _map_loads(drag_load_map)
        check(capi.lib().ivx_world_set_drag_map(self.world.h, int(slot), ptr(loads), loads.shape[0]))

    def set_drag_map_from_grid(self, slot, voxel_object, center_of_mass, config=None) -> None:
        """`ivx_world_set_drag_map_from_grid`: the map of the object's resident mesh, built on the device straight into the slot; `config` a
        `drag.DragLoadMapConfig` (None: the defaults)"""
        from .drag import DragLoadMapConfig

        cfg = (config or DragLoadMapConfig()).as_record()
        com = np.ascontiguousarray(center_of_mass, dtype=np.float32).reshape(3)
        check(capi.lib().ivx_world_set_drag_map_from_grid(self.world.h, int(slot), getattr(voxel_object, "h", voxel_object), ptr(com), ptr(cfg)))

    def drag_map(self, slot):
        """`ivx_world_drag_map_download`: the slot's resident map as [n_theta, 2 n_theta] records, None for an empty slot; waits for the stream"""
        n_theta = C.c_uint32(0)
        check(capi.lib().ivx_world_drag_map_download(self.world.h, int(slot), None, 0, C.byref(n_theta)))  # (the size alone)
        n = int(n_theta.value)
        if n == 0:
            return None
        m = np.zeros((n, 2 * n), dtype=DRAG_LOAD_DTYPE)
        check(capi.lib().ivx_world_drag_map_download(self.world.h, int(slot), ptr(m), m.size, C.byref(n_theta)))
        assert n_theta.value == n
        return m

    def set_drag(self, generators) -> None:
        """`ivx_world_set_detailed_drag`: replaces the detailed-drag set (an empty list removes it); every slot it names must hold a map"""
        g = _drag_records(generators)
        check(capi.lib().ivx_world_set_detailed_drag(self.world.h, _or_null(g), g.size))
        self.n_drag = g.size

    def clear_drag(self) -> None:
        self.set_drag([])
