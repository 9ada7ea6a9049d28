"""Host-side mirror of the reference's detailed drag (engine/crates/impact_physics/src/force/detailed_drag), on top of the C ABI
(`ivx_drag_*`, impact_amd/csrc/drag.hip):

  DragLoadMapConfig     detailed_drag.rs:70-90, 341-353   (the numeric fields)
  DragLoadMap           detailed_drag.rs:355-399          (compute_from_mesh; here also from a voxel object's resident mesh)
  DetailedDragForce     detailed_drag.rs:44-57, 200-243   (apply)

The loads of the directions and the smoothing into the map run in HIP kernels; nothing falls back to the CPU. The lookup of one cell
and the force on one body are host arithmetic of the library (`ivx_drag_map_indices`, `ivx_drag_force_and_torque`).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import capi
from .capi import DRAG_LOAD_DTYPE, DRAG_MAP_CONFIG_DTYPE, RIGID_BODY_DTYPE, check, ptr


class DragLoadMapConfig:
    """`DragLoadMapConfig` without the map-file settings; the defaults are the library's (`ivx_drag_map_config_default`)."""

    def __init__(self, n_direction_samples=None, n_theta_coords=None, smoothness=None):
        r = np.zeros(1, dtype=DRAG_MAP_CONFIG_DTYPE)
        capi.lib().ivx_drag_map_config_default(ptr(r))
        self.n_direction_samples = int(r[0]["n_direction_samples"]) if n_direction_samples is None else int(n_direction_samples)
        self.n_theta_coords = int(r[0]["n_theta_coords"]) if n_theta_coords is None else int(n_theta_coords)
        self.smoothness = float(r[0]["smoothness"]) if smoothness is None else float(smoothness)

    def as_record(self):
        r = np.zeros(1, dtype=DRAG_MAP_CONFIG_DTYPE)
        r[0] = (self.n_direction_samples, self.n_theta_coords, self.smoothness, 0)
        return r

    def angular_interpolation_distance(self) -> float:
        """smoothness * sqrt(4 pi / n) in f32 (compute_angular_interpolation_distance_from_smoothness, detailed_drag.rs:457-465)"""
        return float(np.float32(self.smoothness) * np.sqrt(np.float32(4.0) * np.float32(math.pi) / np.float32(self.n_direction_samples)))


def uniformly_distributed_radial_directions(n: int) -> np.ndarray:
    """`compute_uniformly_distributed_radial_directions` (impact_geometry/src/lib.rs:59-91): [n, 3] f32 unit vectors"""
    d = np.zeros((int(n), 3), dtype=np.float32)
    check(capi.lib().ivx_drag_directions(int(n), ptr(d) if n else None))
    return d


def _vec3(v):
    a = np.ascontiguousarray(v, dtype=np.float32).reshape(-1)
    assert a.size == 3
    return a


def drag_loads_for_triangles(ctx, positions, indices, center_of_mass, directions) -> np.ndarray:
    """`ivx_drag_loads_triangles`: the aggregate drag load (compute_aggregate_drag_load_for_direction, drag_load.rs:174-208) of a triangle
    list for every direction; a record array of DRAG_LOAD_DTYPE"""
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
    dirs = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
    out = np.zeros(max(1, dirs.shape[0]), dtype=DRAG_LOAD_DTYPE)
    check(capi.lib().ivx_drag_loads_triangles(ctx.h, ptr(pos), pos.shape[0], ptr(idx), idx.size, ptr(_vec3(center_of_mass)), ptr(dirs), dirs.shape[0], ptr(out)))
    return out[: dirs.shape[0]]


def drag_loads_for_voxel_object(voxel_object, center_of_mass, directions) -> np.ndarray:
    """`ivx_drag_loads`: the same over the object's resident mesh (the live submeshes)"""
    dirs = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
    out = np.zeros(max(1, dirs.shape[0]), dtype=DRAG_LOAD_DTYPE)
    check(capi.lib().ivx_drag_loads(voxel_object.h, ptr(_vec3(center_of_mass)), ptr(dirs), dirs.shape[0], ptr(out)))
    return out[: dirs.shape[0]]


class DragLoadMap:
    """`DragLoadMap`: an equirectangular map of drag loads, `loads[theta_idx, phi_idx]` (n_theta x 2 n_theta records of DRAG_LOAD_DTYPE)"""

    def __init__(self, loads: np.ndarray):
        loads = np.ascontiguousarray(loads, dtype=DRAG_LOAD_DTYPE)
        assert loads.ndim == 2 and loads.shape[1] == 2 * loads.shape[0]
        self.loads = loads

    @property
    def n_theta_coords(self) -> int:
        return self.loads.shape[0]

    @property
    def n_phi_coords(self) -> int:
        return self.loads.shape[1]

    @classmethod
    def from_samples(cls, ctx, directions, loads, n_theta_coords: int, angular_interpolation_distance: float) -> "DragLoadMap":
        """`generate_map_from_drag_loads` (detailed_drag.rs:401-447): the smoothing stage alone"""
        dirs = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
        ld = np.ascontiguousarray(loads, dtype=DRAG_LOAD_DTYPE).reshape(-1)
        assert ld.size == dirs.shape[0]
        n_theta = int(n_theta_coords)
        m = np.zeros((max(1, n_theta), 2 * max(1, n_theta)), dtype=DRAG_LOAD_DTYPE)
        check(capi.lib().ivx_drag_load_map_from_samples(ctx.h, ptr(dirs), ptr(ld), dirs.shape[0], n_theta, float(angular_interpolation_distance), ptr(m)))
        return cls(m)

    @classmethod
    def compute_from_mesh(cls, ctx, positions, indices, center_of_mass, n_direction_samples=None, n_theta_coords=None, smoothness=None) -> "DragLoadMap":
        """`DragLoadMap::compute_from_mesh` for a triangle list in host memory"""
        cfg = DragLoadMapConfig(n_direction_samples, n_theta_coords, smoothness)
        if cfg.n_direction_samples <= 0 or cfg.n_theta_coords <= 0 or not cfg.smoothness > 0.0:
            raise capi.IvxError(capi.IVX_ERR_INVALID, "DragLoadMap.compute_from_mesh: direction samples, theta coordinates and smoothness must be positive")
        dirs = uniformly_distributed_radial_directions(cfg.n_direction_samples)
        loads = drag_loads_for_triangles(ctx, positions, indices, center_of_mass, dirs)
        return cls.from_samples(ctx, dirs, loads, cfg.n_theta_coords, cfg.angular_interpolation_distance())

    @classmethod
    def compute_from_voxel_object_mesh(cls, mesh, center_of_mass, n_direction_samples=None, n_theta_coords=None, smoothness=None) -> "DragLoadMap":
        """`ivx_drag_load_map`: the map of a `VoxelObjectMesh` as it is resident on the device, in one call"""
        cfg = DragLoadMapConfig(n_direction_samples, n_theta_coords, smoothness)
        n_theta = max(1, cfg.n_theta_coords)
        m = np.zeros((n_theta, 2 * n_theta), dtype=DRAG_LOAD_DTYPE)
        check(capi.lib().ivx_drag_load_map(mesh.object.h, ptr(_vec3(center_of_mass)), ptr(cfg.as_record()), ptr(m)))
        return cls(m)

    def indices(self, phi: float, theta: float):
        """(phi_idx, theta_idx) of the cell that holds the angles (EquirectangularMap::compute_phi_idx / compute_theta_idx)"""
        pi, ti = C.c_uint32(), C.c_uint32()
        check(capi.lib().ivx_drag_map_indices(self.n_theta_coords, float(phi), float(theta), C.byref(pi), C.byref(ti)))
        return int(pi.value), int(ti.value)

    def value(self, phi: float, theta: float):
        """`EquirectangularMap::value`: the load record of the cell at azimuth phi and polar angle theta"""
        pi, ti = self.indices(phi, theta)
        return self.loads[ti, pi]


class DetailedDragForce:
    """`DetailedDragForce` (detailed_drag.rs:44-57): a map, the body's drag coefficient and the scale of its mesh"""

    def __init__(self, drag_load_map: DragLoadMap, drag_coefficient: float, scaling: float = 1.0):
        self.drag_load_map = drag_load_map
        self.drag_coefficient = float(drag_coefficient)
        self.scaling = float(scaling)

    def apply(self, body_record, medium):
        """`DetailedDragForce::apply`: adds the drag force and torque to `total_force` / `total_torque` of one RIGID_BODY_DTYPE record, in
        place when it is a contiguous array of one record; returns the record. `medium` = (velocity[3], mass_density) (UniformMedium)."""
        velocity, mass_density = medium
        body = body_record if isinstance(body_record, np.ndarray) and body_record.dtype == RIGID_BODY_DTYPE and body_record.flags["C_CONTIGUOUS"] \
            else np.ascontiguousarray(body_record, dtype=RIGID_BODY_DTYPE)
        body = body.reshape(1)
        check(capi.lib().ivx_drag_force_and_torque(ptr(self.drag_load_map.loads), self.drag_load_map.n_theta_coords, ptr(body), ptr(_vec3(velocity)),
                                                   float(mass_density), self.drag_coefficient, self.scaling))
        return body
