"""SDF queries: the value and gradient of a compiled atomic SDF program at arbitrary points, and the three placements of the reference's
meta-SDF graph that sample it (engine/crates/impact_voxel/src/generation/sdf/meta.rs):
  SDFQuery.closest      compute_translation_to_closest_point_on_surface   meta.rs:2411-2479   (MetaClosestTranslationToSurface :1620-1688)
  SDFQuery.spherecast   compute_spherecast_translation_to_surface         meta.rs:2534-2703   (MetaRayTranslationToSurface    :1690-1796)
  SDFQuery.rotation     compute_rotation_to_gradient                      meta.rs:2481-2532   (MetaRotationToGradient         :1798-1863)
  SDFQuery.distances / .gradients   compute_signed_distance (atomic.rs:1001-1010) / sample_signed_distance_with_gradient (meta.rs:2728-2770)
The three `*_instances` functions turn results into the output lists of the reference's nodes. All compute happens in libimpact_voxel_hip.so
(csrc/sdf_query.hip): on the device with a context, through the host build of the same functions with `device=False`."""
from __future__ import annotations

import ctypes as C
import sys

import numpy as np

from . import capi
from .capi import check, ptr
from .capi import SDF_QUERY_INSTANCE_DTYPE as INSTANCE_DTYPE, SDF_QUERY_RESULT_DTYPE as RESULT_DTYPE, SIMILARITY_DTYPE
from .voxel import SDFGenerator, _live_grids

f32 = np.float32
IDENTITY = np.zeros((), SIMILARITY_DTYPE)
IDENTITY["rotation"] = (0, 0, 0, 1)
IDENTITY["scaling"] = 1
# the constants the reference's nodes pass (meta.rs:1664-1665, 1737-1740)
CLOSEST_MAX_ITERATIONS, CLOSEST_MAX_DISTANCE = 5, 0.1
CAST_DIRECTION, CAST_MAX_STEPS, CAST_TOLERANCE, CAST_SAFETY_FACTOR = (0.0, 1.0, 0.0), 128, 0.1, 0.5


def similarity(translation=(0, 0, 0), rotation_xyzw=(0, 0, 0, 1), scaling=1.0):
    s = np.zeros((), SIMILARITY_DTYPE)
    s["translation"], s["rotation"], s["scaling"] = translation, rotation_xyzw, scaling
    return s


def instances(translations, rotations_xyzw=None, scalings=None, sphere_centers=None, sphere_radii=None):
    """an `ivx_sdf_query_instance` array from per-instance columns (identity rotation, unit scaling and a zero sphere by default)"""
    t = np.asarray(translations, f32).reshape(-1, 3)
    a = np.zeros(len(t), INSTANCE_DTYPE)
    a["subject_to_parent"]["translation"] = t
    a["subject_to_parent"]["rotation"] = (0, 0, 0, 1) if rotations_xyzw is None else np.asarray(rotations_xyzw, f32)
    a["subject_to_parent"]["scaling"] = 1 if scalings is None else np.asarray(scalings, f32)
    if sphere_centers is not None:
        a["sphere_center"] = np.asarray(sphere_centers, f32)
    if sphere_radii is not None:
        a["sphere_radius"] = np.asarray(sphere_radii, f32)
    return a


class SDFQuery:
    """`ivx_sdf_query` over a compiled `SDFGenerator`. `device=False` (no context needed): the host build of the functions the kernels run."""

    def __init__(self, generator: SDFGenerator, ctx=None, device: bool = True):
        if device and ctx is None:
            raise ValueError("SDFQuery on the device needs a Context (device=False runs the host build)")
        self.generator = generator
        self.ctx = ctx if device else None
        nodes = np.ascontiguousarray(generator.nodes)
        h = C.c_void_p()
        check(capi.lib().ivx_sdf_query_create(self.ctx.h if self.ctx else None, ptr(nodes) if len(nodes) else None, len(nodes),
                                              generator.required_forward_stack_size, ptr(np.ascontiguousarray(generator.domain, f32)), C.byref(h)))
        self.h = h
        if self.ctx:
            _live_grids.add(self)  # (released before the contexts at interpreter exit)

    def close(self):
        if getattr(self, "h", None):
            capi.lib().ivx_sdf_query_destroy(self.h)
            self.h = None

    def __del__(self):
        if not sys.is_finalizing():
            try:
                self.close()
            except Exception:
                pass

    def __hash__(self):
        return id(self)

    def _points(self, which, points, width):
        p = np.ascontiguousarray(np.asarray(points, f32).reshape(-1, 3))
        out = np.zeros((len(p), width) if width > 1 else len(p), f32)
        check(capi.lib().ivx_sdf_query_points(self.h, which, ptr(p), len(p), ptr(out)))
        return out

    def distances(self, points):
        """compute_signed_distance at each root-space point"""
        return self._points(0, points, 1)

    def gradients(self, points):
        """sample_signed_distance_with_gradient at each root-space point: [n, 4] = centre value, gradient"""
        return self._points(1, points, 4)

    @staticmethod
    def _args(surface_to_parent, inst):
        s = np.ascontiguousarray(np.asarray(IDENTITY if surface_to_parent is None else surface_to_parent, SIMILARITY_DTYPE).reshape(()))
        a = np.ascontiguousarray(np.asarray(inst, INSTANCE_DTYPE).reshape(-1))
        return s, a, np.zeros(len(a), RESULT_DTYPE)

    def closest(self, surface_to_parent, inst, max_iterations=CLOSEST_MAX_ITERATIONS, max_distance=CLOSEST_MAX_DISTANCE):
        s, a, r = self._args(surface_to_parent, inst)
        check(capi.lib().ivx_sdf_query_closest(self.h, ptr(s), ptr(a), len(a), int(max_iterations), float(max_distance), ptr(r)))
        return r

    def spherecast(self, surface_to_parent, inst, direction=CAST_DIRECTION, max_steps=CAST_MAX_STEPS, tolerance=CAST_TOLERANCE,
                   safety_factor=CAST_SAFETY_FACTOR):
        s, a, r = self._args(surface_to_parent, inst)
        d = np.ascontiguousarray(np.asarray(direction, f32).reshape(3))
        check(capi.lib().ivx_sdf_query_spherecast(self.h, ptr(s), ptr(a), len(a), ptr(d), int(max_steps), float(tolerance), float(safety_factor), ptr(r)))
        return r

    def rotation(self, surface_to_parent, inst):
        s, a, r = self._args(surface_to_parent, inst)
        check(capi.lib().ivx_sdf_query_rotation(self.h, ptr(s), ptr(a), len(a), ptr(r)))
        return r


# ---- the reference's output lists ---------------------------------------------------------------------------------------------------------------
def _qrot(q, v):
    """glam Quat::mul_vec3a in the library's operation order (csrc/vec3.hpp), float32, rows of v"""
    b, w = q[:3], q[3]
    b2 = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]
    vb = (v[:, 0] * b[0] + v[:, 1] * b[1]) + v[:, 2] * b[2]
    cx = b[1] * v[:, 2] - v[:, 1] * b[2]
    cy = b[2] * v[:, 0] - v[:, 2] * b[0]
    cz = b[0] * v[:, 1] - v[:, 0] * b[1]
    k, kb, kc = w * w - b2, vb * f32(2), w * f32(2)
    return np.stack([(v[:, 0] * k + b[0] * kb) + cx * kc, (v[:, 1] * k + b[1] * kb) + cy * kc, (v[:, 2] * k + b[2] * kb) + cz * kc], axis=1).astype(f32)


def _qmul(a, b):
    """glam Quat::mul_quat (xyzw), rows"""
    ax, ay, az, aw = (a[:, i] for i in range(4))
    bx, by, bz, bw = (b[:, i] for i in range(4))
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz], axis=1).astype(f32)


def translated_instances(inst, results):
    """the instances whose result is Some, in order, each `translated` by its result (similarity.rs:131-134)"""
    inst = np.asarray(inst, INSTANCE_DTYPE).reshape(-1)
    keep = results["status"] == capi.SQ_OK
    out = inst[keep].copy()
    out["subject_to_parent"]["translation"] = out["subject_to_parent"]["translation"] + results["v"][keep][:, :3]
    return out


def rotated_instances(inst, results):
    """the instances whose result is Some, in order, each `rotated` by its result (similarity.rs:138-144): the rotation turns the translation and
    multiplies the orientation from the left"""
    inst = np.asarray(inst, INSTANCE_DTYPE).reshape(-1)
    keep = results["status"] == capi.SQ_OK
    out = inst[keep].copy()
    q = np.ascontiguousarray(results["v"][keep], f32)
    t = np.ascontiguousarray(out["subject_to_parent"]["translation"], f32)
    r = np.ascontiguousarray(out["subject_to_parent"]["rotation"], f32)
    new_t = np.empty_like(t)
    for i in range(len(out)):
        new_t[i] = _qrot(q[i], t[i : i + 1])[0]
    out["subject_to_parent"]["translation"] = new_t
    out["subject_to_parent"]["rotation"] = _qmul(q, r) if len(out) else r
    return out


def closest_translation_instances(query, surface_to_parent, inst, **kw):
    """MetaClosestTranslationToSurface's output (meta.rs:1636-1686); `query` None stands for SingleSDF(None): the input comes back unchanged"""
    inst = np.asarray(inst, INSTANCE_DTYPE).reshape(-1)
    return inst.copy() if query is None else translated_instances(inst, query.closest(surface_to_parent, inst, **kw))


def ray_translation_instances(query, surface_to_parent, inst, **kw):
    """MetaRayTranslationToSurface's output (meta.rs:1706-1794)"""
    inst = np.asarray(inst, INSTANCE_DTYPE).reshape(-1)
    return inst.copy() if query is None else translated_instances(inst, query.spherecast(surface_to_parent, inst, **kw))


def rotation_to_gradient_instances(query, surface_to_parent, inst):
    """MetaRotationToGradient's output (meta.rs:1815-1861)"""
    inst = np.asarray(inst, INSTANCE_DTYPE).reshape(-1)
    return inst.copy() if query is None else rotated_instances(inst, query.rotation(surface_to_parent, inst))
