"""Host-side mirror of the motion-driver calls (`ivx_world_set_motion_drivers`, `ivx_world_apply_motion`, `ivx_md_*`; impact_amd/csrc/motion.hip):
the reference's `MotionDriverManager` (impact_physics/src/driven_motion.rs) for kinematic bodies of a `PhysicsWorld`:

  CircularTrajectory              driven_motion/circular.rs:52-68               (`circular`)
  ConstantAccelerationTrajectory  driven_motion/constant_acceleration.rs:52-61  (`constant_acceleration`, `constant_velocity`)
  HarmonicOscillatorTrajectory    driven_motion/harmonic_oscillation.rs:55-64   (`harmonic_oscillator`)
  OrbitalTrajectory               driven_motion/orbit.rs:52-70                  (`orbital`)
  ConstantRotation                driven_motion/constant_rotation.rs:51-59      (`constant_rotation`)
  MotionDriverManager::apply_motion  driven_motion.rs:50-82                     (`MotionDrivers.apply`, and the tail of every `PhysicsWorld.step`)

A record holds the setup struct of its kind field by field; `body` indexes the world's kinematic bodies. With a set installed every step of the
world ends by applying it at the world's new time. Nothing here computes, and nothing falls back to the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import KINEMATIC_BODY_DTYPE, MOTION_DRIVER_DTYPE, check, ptr


def _driver(kind, body, *fields):
    d = np.zeros((), dtype=MOTION_DRIVER_DTYPE)
    d["kind"], d["body"] = kind, body
    p = np.concatenate([np.asarray(f, dtype=np.float32).reshape(-1) for f in fields])
    d["p"][: p.size] = p
    return d


def circular(body, initial_time, orientation_xyzw, center_position, radius, period) -> np.ndarray:
    return _driver(capi.MD_CIRCULAR, body, initial_time, orientation_xyzw, center_position, radius, period)


def constant_acceleration(body, initial_time, initial_position, initial_velocity, acceleration) -> np.ndarray:
    return _driver(capi.MD_CONSTANT_ACCELERATION, body, initial_time, initial_position, initial_velocity, acceleration)


def constant_velocity(body, initial_time, initial_position, velocity) -> np.ndarray:
    """`ConstantAccelerationTrajectory::with_constant_velocity`"""
    return constant_acceleration(body, initial_time, initial_position, velocity, (0.0, 0.0, 0.0))


def harmonic_oscillator(body, center_time, center_position, direction, amplitude, period) -> np.ndarray:
    return _driver(capi.MD_HARMONIC, body, center_time, center_position, direction, amplitude, period)


def orbital(body, periapsis_time, orientation_xyzw, focal_position, semi_major_axis, eccentricity, period) -> np.ndarray:
    return _driver(capi.MD_ORBITAL, body, periapsis_time, orientation_xyzw, focal_position, semi_major_axis, eccentricity, period)


def constant_rotation(body, initial_time, initial_orientation_xyzw, axis, angular_speed) -> np.ndarray:
    return _driver(capi.MD_CONSTANT_ROTATION, body, initial_time, initial_orientation_xyzw, axis, angular_speed)


def _records(drivers):
    return np.ascontiguousarray(drivers, dtype=MOTION_DRIVER_DTYPE).reshape(-1)


def evaluate(driver, time) -> np.ndarray:
    """`ivx_md_eval`: one driver at `time` -> float32[10] (trajectories: position, velocity; rotation: orientation xyzw, axis, angular speed)"""
    d, out = _records(driver), np.zeros(10, dtype=np.float32)
    assert d.size == 1, d.size
    check(capi.lib().ivx_md_eval(ptr(d), float(time), ptr(out)))
    return out


def apply_host(drivers, kinematic_bodies, time) -> np.ndarray:
    """`ivx_md_apply_host`: the composition rule over a copy of host bodies, the code the kernel runs"""
    d = _records(drivers)
    k = np.array(kinematic_bodies, dtype=KINEMATIC_BODY_DTYPE, copy=True).reshape(-1)
    check(capi.lib().ivx_md_apply_host(ptr(d) if d.size else None, d.size, ptr(k) if k.size else None, k.size, float(time)))
    return k


class MotionDrivers:
    """The driver set and the simulation clock of a `PhysicsWorld`."""

    def __init__(self, physics_world):
        self.world = physics_world
        self.n = 0

    def set(self, drivers) -> None:
        """`ivx_world_set_motion_drivers`: replaces the set (an empty list removes it); call it after `PhysicsWorld.set_bodies`"""
        d = _records(drivers) if len(drivers) else np.zeros(0, dtype=MOTION_DRIVER_DTYPE)
        check(capi.lib().ivx_world_set_motion_drivers(self.world.h, ptr(d) if d.size else None, d.size))
        self.n = d.size

    def clear(self) -> None:
        self.set([])

    def apply(self, time: float) -> None:
        """`ivx_world_apply_motion`: the stage on its own, enqueued; does not touch the clock"""
        check(capi.lib().ivx_world_apply_motion(self.world.h, float(time)))

    @property
    def time(self) -> float:
        t = C.c_float(0.0)
        check(capi.lib().ivx_world_time(self.world.h, C.byref(t)))
        return t.value

    @time.setter
    def time(self, value: float) -> None:
        check(capi.lib().ivx_world_set_time(self.world.h, float(value)))
