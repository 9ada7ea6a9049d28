"""Host-side mirror of the frame-instance calls (`ivx_fi_*`, impact_amd/csrc/instances.hip): what the reference's task
BufferModelInstancesAndBoundLights (engine/src/tasks.rs:779) does in per-view loops on the host, as one call per pass over the context's resident
world boxes and query masks:

  buffer_model_instances_for_rendering                                          model.rs:171-297          (`camera_view`)
  bound_omnidirectional_lights_and_buffer_shadow_casting_model_instances        light.rs:85-284, 383-450  (`omnidirectional_light_view`, `cubemap_face_view`)
  bound_unidirectional_lights_and_buffer_shadow_casting_model_instances         light.rs:465-641, 747-848 (`unidirectional_light_view`, `cascade_view`)

A frame: `bvol.set_*` / `CollisionWorld.synchronize` -> `BoundingVolumeSet.query` -> `FrameInstances.views` (camera; light culling with REACH; faces
and cascades with `and_view`) -> `FrameInstances.cull`. The pairs, the lists, the kept masks and the results stay in context-owned device buffers
(`device_ptr`). The light geometry (cascade volumes, face frusta, light-space orientation, texel snapping), material buffering, scene-graph group
transforms and `declare_visible_this_frame` stay with the caller. Nothing here computes, and nothing falls back to the CPU: `views_host` is the
library's own host form.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import (AABB_DTYPE, CULL_PAIR_DTYPE, CULL_REGION_DTYPE, CULL_VIEW_DTYPE, FI_INSTANCE_DTYPE, FI_VIEW_DTYPE, FI_VIEW_RESULT_DTYPE, SIMILARITY_DTYPE, check, ptr)
from .cull import CullResult, _objects
from .many import _handles

SHADOW_REJECT = capi.FI_ABSENT | capi.FI_HIDDEN | capi.FI_CASTS_NO_SHADOWS | capi.FI_SHADOWS_OFF_BY_DISTANCE | capi.FI_NO_SHADOW_FEATURES  # light.rs:401-417
CAMERA_REJECT = capi.FI_ABSENT | capi.FI_HIDDEN  # model.rs: no node, or hidden


def _rec(a, dtype, n=None):
    a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
    assert n is None or a.size == n, (a.size, n)
    return a


def instances(model_to_world, flags=None, entities=None) -> np.ndarray:
    """`ivx_fi_instance` records from SIMILARITY_DTYPE records, flags (None: 0) and entities (None: the object's index)"""
    s = _rec(model_to_world, SIMILARITY_DTYPE)
    out = np.zeros(s.size, dtype=FI_INSTANCE_DTYPE)
    out["model_to_world"] = s
    out["flags"] = 0 if flags is None else np.asarray(flags, dtype=np.uint32)
    out["entity"] = np.arange(s.size, dtype=np.uint32) if entities is None else np.asarray(entities, dtype=np.uint32)
    return out


def view(world_to_view, query: int, reject_flags: int = 0, exclude_entity: int = capi.FI_NONE, and_view: int = capi.FI_NONE, instance_base: int = 0, flags: int = 0,
         point=(0.0, 0.0, 0.0), squared_reach: float = 0.0) -> np.ndarray:
    """one `ivx_fi_view` record; `world_to_view` a SIMILARITY_DTYPE record"""
    v = np.zeros((), dtype=FI_VIEW_DTYPE)
    v["world_to_view"] = np.asarray(world_to_view, dtype=SIMILARITY_DTYPE).reshape(())
    v["query"], v["reject_flags"], v["exclude_entity"], v["and_view"], v["instance_base"], v["flags"] = query, reject_flags, exclude_entity, and_view, instance_base, flags
    v["point"], v["squared_reach"] = point, squared_reach
    return v


def isometry(rotation_xyzw, translation) -> np.ndarray:
    """an isometry as a SIMILARITY_DTYPE record (scaling 1)"""
    s = np.zeros((), dtype=SIMILARITY_DTYPE)
    s["rotation"], s["translation"], s["scaling"] = rotation_xyzw, translation, 1.0
    return s


def camera_view(world_to_camera, query: int, instance_base: int = 0) -> np.ndarray:
    """buffer_model_instances_for_rendering: the camera frustum's hits minus hidden and absent instances, the camera-space transforms, and the
    world- and camera-space boxes of the visible models. `world_to_camera`: an `isometry`; `query`: the row of the camera frustum."""
    return view(world_to_camera, query, CAMERA_REJECT, instance_base=instance_base, flags=capi.FI_VIEW_BOX)


def omnidirectional_light_view(world_to_camera, query: int, light_entity: int, world_space_position, max_reach: float) -> np.ndarray:
    """the culling pass of a shadowable omnidirectional light (register_primitive_in_omnidirectional_light_culling_frustum): the hits of its culling
    frustum or sphere (`query`) that can cast shadows, are not the light itself and lie within reach; the results carry the squared shadow-shell
    distances; the transforms are model_to_camera (ShadowingModel), which `cubemap_face_view` composes further on the host side of its own view"""
    reach = np.float32(max_reach)
    return view(world_to_camera, query, SHADOW_REJECT, exclude_entity=light_entity, flags=capi.FI_VIEW_REACH, point=world_space_position, squared_reach=reach * reach)


def cubemap_face_view(world_to_face, query: int, light_view: int, instance_base: int = 0) -> np.ndarray:
    """one cubemap face of that light in the NEXT call: the face frustum's hits among the light's shadowing models (`light_view`: the light's view index
    in the previous call); `world_to_face` = camera-to-face o world-to-camera, composed by the caller"""
    return view(world_to_face, query, and_view=light_view, instance_base=instance_base)


def unidirectional_light_view(world_to_light, query: int, light_entity: int) -> np.ndarray:
    """the bounding pass of a shadowable unidirectional light: the shadow casters among the hits of `query`, and their light-space box"""
    return view(world_to_light, query, SHADOW_REJECT, exclude_entity=light_entity, flags=capi.FI_VIEW_BOX)


def cascade_view(world_to_light, query: int, light_entity: int, instance_base: int = 0, light_view: int = capi.FI_NONE) -> np.ndarray:
    """one cascade of that light: the shadow casters among the hits of the cascade's oriented box (`query`), their light-space transforms and box"""
    return view(world_to_light, query, SHADOW_REJECT, exclude_entity=light_entity, and_view=light_view, instance_base=instance_base, flags=capi.FI_VIEW_BOX)


class FrameInstanceOutputs:
    """pairs [n_views, n] CULL_PAIR_DTYPE, offsets [n_views + 1], objects / transforms [offsets[-1]], kept masks [n_views, ceil(n / 64)] uint64,
    results [n_views] FI_VIEW_RESULT_DTYPE (None from `download`)"""

    def __init__(self, pairs, offsets, objects, transforms, kept, results=None):
        self.pairs, self.offsets, self.objects, self.transforms, self.kept, self.results = pairs, offsets, objects, transforms, kept, results

    def tobytes(self) -> bytes:
        return b"".join(a.tobytes() for a in (self.pairs, self.offsets, self.objects, self.transforms, self.kept) + (() if self.results is None else (self.results,)))


def views_host(world_boxes, instance_records, masks, view_records, previous_kept=None) -> FrameInstanceOutputs:
    """`ivx_fi_views_host`: the whole stage on the host with the library's own functions. `masks`: [n_queries, ceil(n / 64)] uint64;
    `previous_kept`: the kept masks of the previous call, [n_previous_views, ceil(n / 64)] (None: no previous call)"""
    w, inst, v = _rec(world_boxes, AABB_DTYPE), _rec(instance_records, FI_INSTANCE_DTYPE), _rec(view_records, FI_VIEW_DTYPE)
    n, nv, words = w.size, v.size, (w.size + 63) // 64
    assert inst.size == n, (inst.size, n)
    m = np.ascontiguousarray(masks, dtype=np.uint64).reshape(-1, words) if words else np.zeros((len(masks), 0), dtype=np.uint64)
    prev = None if previous_kept is None else (np.ascontiguousarray(previous_kept, dtype=np.uint64).reshape(-1, words) if words else np.zeros((len(previous_kept), 0), dtype=np.uint64))
    pairs, offsets = np.zeros((nv, n), dtype=CULL_PAIR_DTYPE), np.zeros(nv + 1, dtype=np.uint32)
    objects, transforms = np.zeros(max(1, nv * n), dtype=np.uint32), np.zeros(max(1, nv * n), dtype=SIMILARITY_DTYPE)
    kept, results = np.zeros((nv, words), dtype=np.uint64), np.zeros(nv, dtype=FI_VIEW_RESULT_DTYPE)
    check(capi.lib().ivx_fi_views_host(ptr(w) if n else None, n, ptr(inst) if n else None, ptr(m) if m.size else None, m.shape[0], ptr(v) if nv else None, nv,
                                       ptr(prev) if prev is not None and prev.size else None, 0 if prev is None else prev.shape[0], ptr(pairs) if pairs.size else None,
                                       ptr(offsets), ptr(objects), ptr(transforms), nv * n, ptr(kept) if kept.size else None, ptr(results) if nv else None))
    total = int(offsets[nv])
    return FrameInstanceOutputs(pairs, offsets, objects[:total], transforms[:total], kept, results)


class FrameInstances:
    """The frame-instance state of a context: the instances it holds and the outputs of its last `views` call."""

    def __init__(self, ctx):
        self.ctx, self._h = ctx, ctx.h
        self.n, self.n_views = 0, 0

    def set_instances(self, instance_records) -> None:
        """`ivx_fi_set_instances`: one per object of the context's bounding-volume set, resident until the next call"""
        inst = _rec(instance_records, FI_INSTANCE_DTYPE)
        check(capi.lib().ivx_fi_set_instances(self._h, ptr(inst) if inst.size else None, inst.size))
        self.n = inst.size

    def views(self, view_records, with_results: bool = True):
        """`ivx_fi_views` over the context's set, its last queries call and the instances -> results [n_views] (None when `with_results` is off:
        nothing waits)"""
        v = _rec(view_records, FI_VIEW_DTYPE)
        results = np.zeros(v.size, dtype=FI_VIEW_RESULT_DTYPE) if with_results else None
        check(capi.lib().ivx_fi_views(self._h, ptr(v) if v.size else None, v.size, ptr(results) if with_results and v.size else None))
        self.n_views = v.size
        return results

    def download(self) -> FrameInstanceOutputs:
        """`ivx_fi_download`: every output of the last `views` call"""
        nv, n, words = self.n_views, self.n, (self.n + 63) // 64
        pairs, offsets, kept = np.zeros((nv, n), dtype=CULL_PAIR_DTYPE), np.zeros(nv + 1, dtype=np.uint32), np.zeros((nv, words), dtype=np.uint64)
        total = C.c_size_t(0)
        lib = capi.lib()
        check(lib.ivx_fi_download(self._h, ptr(pairs) if pairs.size else None, pairs.size, ptr(offsets), offsets.size, None, None, 0, ptr(kept) if kept.size else None, kept.size,
                                  C.byref(total)))
        objects, transforms = np.zeros(max(1, total.value), dtype=np.uint32), np.zeros(max(1, total.value), dtype=SIMILARITY_DTYPE)
        check(lib.ivx_fi_download(self._h, None, 0, None, 0, ptr(objects), ptr(transforms), total.value, None, 0, None))
        return FrameInstanceOutputs(pairs, offsets, objects[: total.value], transforms[: total.value], kept)

    def device_ptr(self, which: int) -> int:
        """`ivx_fi_device_ptr`: capi.FI_PTR_INSTANCES / _PAIRS / _OFFSETS / _OBJECTS / _TRANSFORMS / _KEPT_MASKS / _RESULTS"""
        return int(capi.lib().ivx_fi_device_ptr(self._h, int(which)) or 0)

    def cull(self, voxel_objects, cull_view_records, object_indices=None, mode: int = capi.CULL_ZEROED, objects=None) -> CullResult:
        """`ivx_cull_many_resident`: `cull.cull_many(..., enqueue_only=True)` with the pair of (view, object g) taken on the device from the last
        `views` call at (view, object_indices[g]) (None: g). The counts come with `CullResult.collect`."""
        n = len(voxel_objects)
        v = _rec(cull_view_records, CULL_VIEW_DTYPE)
        idx = None if object_indices is None else np.ascontiguousarray(object_indices, dtype=np.uint32).reshape(-1)
        assert idx is None or idx.size == n, (idx.size, n)
        o = _objects(objects, n)
        layout = np.zeros(v.size, dtype=CULL_REGION_DTYPE)
        handles = _handles(voxel_objects)
        check(capi.lib().ivx_cull_many_resident(ptr(handles) if n else None, n, ptr(o) if o is not None and n else None, ptr(idx) if idx is not None and n else None,
                                                ptr(v) if v.size else None, v.size, int(mode), ptr(layout) if v.size else None))
        return CullResult(voxel_objects[0].ctx.h if n else None, layout, None, n)
