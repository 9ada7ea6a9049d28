"""Host-side mirror of the primitive collidable calls (`ivx_cw_*`, impact_amd/csrc/narrow.hip): the reference's `CollisionWorld` for sphere,
plane and capsule collidables (impact_physics/src/collision.rs, collision/collidable/basic.rs) on top of a `PhysicsWorld`:

  synchronize_collidables_with_rigid_bodies                                collision.rs:175-209   (`CollisionWorld.synchronize`)
  cache_all_collisions / for_each_non_phantom_collision_involving_dynamic  collision.rs:215-373   (`CollisionWorld.collide`, modes 0 / 1)
  generate_contact_manifold                                                basic.rs:57-151        (`contact`, host arithmetic of the library)
  Collidable::from_descriptor                                              basic.rs:42-55         (`transform`)

  VoxelObjectCollidable::new, generate_contact_manifold (voxel pairs)     impact_voxel collidable.rs:310-327, 138-215 (`to_object_space`, `voxel_row`)

A frame: `synchronize()` -> `collide()` -> `PhysicsWorld.prepare_constraints(contacts)` -> `PhysicsWorld.step(dt)`. With voxel objects among the
collidables: `set_voxel_objects()` once, then `synchronize()` -> `collide_frame()` -> `prepare_constraints(merged)` -> `step(dt)` — the deferred pairs'
manifolds come back in the same call, behind the primitive contacts. The world-space collidables, the world boxes, the pairs, the contacts, the
deferred pairs and their rows stay in device buffers. Nothing here computes, and nothing falls back to the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .bvol import BoundingVolumeSet
from .capi import (AABB_DTYPE, COLLIDABLE_DTYPE, COLLIDABLE_QUERY_DTYPE, CONTACT_DTYPE, CW_VOXEL_OBJECT_DTYPE, CW_VOXEL_ROW_DTYPE, MUTUAL_QUERY_DTYPE, check,
                   ptr)

NO_CONTACT, CONTACT, DEFERRED = 0, 1, 2  # `ivx_cw_contact`'s verdicts


def _collidable(shape, body, collidable_id, kind, response, kinematic):
    c = np.zeros((), dtype=COLLIDABLE_DTYPE)
    c["shape"], c["kind"], c["id"], c["response"] = shape, kind, collidable_id, response
    c["body"] = int(body) | (capi.KINEMATIC_BIT if kinematic else 0)
    return c


def sphere(center, radius, body, collidable_id, kind=capi.BV_DYNAMIC, response=(0.0, 0.0, 0.0), kinematic=False) -> np.ndarray:
    c = _collidable(capi.CW_SPHERE, body, collidable_id, kind, response, kinematic)
    c["a"], c["s"] = center, radius
    return c


def plane(unit_normal, displacement, body, collidable_id, kind=capi.BV_STATIC, response=(0.0, 0.0, 0.0), kinematic=False) -> np.ndarray:
    c = _collidable(capi.CW_PLANE, body, collidable_id, kind, response, kinematic)
    c["a"], c["s"] = unit_normal, displacement
    return c


def capsule(segment_start, segment_vector, radius, body, collidable_id, kind=capi.BV_DYNAMIC, response=(0.0, 0.0, 0.0), kinematic=False) -> np.ndarray:
    c = _collidable(capi.CW_CAPSULE, body, collidable_id, kind, response, kinematic)
    c["a"], c["b"], c["s"] = segment_start, segment_vector, radius
    return c


def voxel_object(model_lower, model_upper, body, collidable_id, kind=capi.BV_DYNAMIC, response=(0.0, 0.0, 0.0), kinematic=False) -> np.ndarray:
    """a voxel object's place in the broad phase; its pairs come back deferred. The box is the object's model box IN THE BODY'S FRAME, whose origin
    is the body's centre of mass and not the grid's origin: `bvol.grid_model_aabb` MINUS the origin offset (the local centre of mass, in float32),
    and again after every edit that moves the centre of mass. A record holding the model box as it is puts the world box a centre of mass away
    from the body. The reference derives the object's world -> object transform from the same offset, in float32 (collidable.rs:310-327):
    t_w = rotate(q, -origin_offset) + p;  rotation = conj(q);  translation = -rotate(rotation, t_w) — the transform the deferred pairs' generators
    take (INTEGRATION.md 2c has the table of which member is A)"""
    c = _collidable(capi.CW_VOXEL_OBJECT, body, collidable_id, kind, response, kinematic)
    c["a"], c["b"] = model_lower, model_upper
    return c


def _one(record):
    a = np.ascontiguousarray(record, dtype=COLLIDABLE_DTYPE).reshape(-1)
    assert a.size == 1, a.size
    return a


def transform(local, position, orientation_xyzw):
    """`ivx_cw_transform`: one collidable under its body's position and orientation -> (world-space collidable, world box)"""
    world, box = np.zeros(1, dtype=COLLIDABLE_DTYPE), np.zeros(1, dtype=AABB_DTYPE)
    p, q = np.ascontiguousarray(position, dtype=np.float32).reshape(3), np.ascontiguousarray(orientation_xyzw, dtype=np.float32).reshape(4)
    check(capi.lib().ivx_cw_transform(ptr(_one(local)), ptr(p), ptr(q), ptr(world), ptr(box)))
    return world[0], box[0]


def contact(a_world, b_world):
    """`ivx_cw_contact`: one pair of world-space collidables -> (verdict, the contact record when the verdict is CONTACT, else None)"""
    out, hit = np.zeros(1, dtype=CONTACT_DTYPE), C.c_int(0)
    check(capi.lib().ivx_cw_contact(ptr(_one(a_world)), ptr(_one(b_world)), ptr(out), C.byref(hit)))
    return hit.value, (out[0] if hit.value == CONTACT else None)


def to_object_space(position, orientation_xyzw, origin_offset):
    """`ivx_cw_to_object_space`: the world -> object transform of a voxel body, float32 in the reference's order -> (rotation_xyzw, translation)"""
    p, q, o = (np.ascontiguousarray(v, dtype=np.float32).reshape(k) for v, k in ((position, 3), (orientation_xyzw, 4), (origin_offset, 3)))
    rotation, translation = np.zeros(4, dtype=np.float32), np.zeros(3, dtype=np.float32)
    check(capi.lib().ivx_cw_to_object_space(ptr(p), ptr(q), ptr(o), ptr(rotation), ptr(translation)))
    return rotation, translation


def voxel_object_record(grid, origin_offset, center_of_mass) -> np.ndarray:
    """an `ivx_cw_voxel_object`: `grid` is a device object (its handle is taken), None or a raw handle"""
    r = np.zeros((), dtype=CW_VOXEL_OBJECT_DTYPE)
    handle = getattr(grid, "h", grid)
    r["grid"] = int(getattr(handle, "value", handle) or 0)
    r["origin_offset"], r["center_of_mass"] = origin_offset, center_of_mass
    return r


def voxel_row(a_world, b_world, pose_a=None, pose_b=None, voxel_a=None, voxel_b=None) -> np.ndarray:
    """`ivx_cw_voxel_row`: the dispatch of one deferred pair of world-space collidables. pose_* = (position, orientation_xyzw) of a voxel member's
    body, voxel_* its `voxel_object_record` -> one CW_VOXEL_ROW_DTYPE record (`voxel` / `other` read 0 for member a, 1 for member b)"""
    def pose(p):
        return None if p is None else np.concatenate([np.asarray(p[0], dtype=np.float32).reshape(3), np.asarray(p[1], dtype=np.float32).reshape(4)])

    def record(v):
        return None if v is None else np.ascontiguousarray(v, dtype=CW_VOXEL_OBJECT_DTYPE).reshape(1)

    pa, pb, va, vb = pose(pose_a), pose(pose_b), record(voxel_a), record(voxel_b)
    out = np.zeros(1, dtype=CW_VOXEL_ROW_DTYPE)
    check(capi.lib().ivx_cw_voxel_row(ptr(_one(a_world)), ptr(_one(b_world)), *(None if x is None else ptr(x) for x in (pa, pb, va, vb)), ptr(out)))
    return out[0]


def row_queries(rows, grid_handles=None):
    """the rows as the generators' records, by plain field copies -> (ivx_collidable_query records, their row positions, ivx_mutual_query records, their
    row positions). grid_handles: collidable index -> handle, for the mutual records' `a` / `b` (left zero without it)"""
    rows = np.ascontiguousarray(rows, dtype=CW_VOXEL_ROW_DTYPE).reshape(-1)
    is_mutual = rows["generator"] == capi.CW_ROW_MUTUAL
    r, m = rows[~is_mutual], rows[is_mutual]
    cq, mq = np.zeros(len(r), dtype=COLLIDABLE_QUERY_DTYPE), np.zeros(len(m), dtype=MUTUAL_QUERY_DTYPE)
    cq["mode"], cq["rotation_xyzw"], cq["translation"] = r["generator"], r["rotation_a"], r["translation_a"]
    for f in ("shape3", "shape3b", "shape1", "body_a", "body_b", "collidable_id_a", "collidable_id_b", "response"):
        cq[f] = r[f]
    for f in ("rotation_a", "translation_a", "center_of_mass_a", "rotation_b", "translation_b", "center_of_mass_b", "collidable_id_a", "collidable_id_b", "body_a", "body_b",
              "response"):
        mq[f] = m[f]
    if grid_handles is not None:
        mq["a"], mq["b"] = [grid_handles[int(i)] for i in m["voxel"]], [grid_handles[int(i)] for i in m["other"]]
    return cq, np.nonzero(~is_mutual)[0], mq, np.nonzero(is_mutual)[0]


class CollisionWorld:
    """The collidables of a `PhysicsWorld`. List planes last: a block of 64 consecutive collidables that holds one is never rejected as a whole."""

    def __init__(self, physics_world):
        self.world = physics_world
        self.n = 0

    def set_collidables(self, collidables) -> None:
        """`ivx_cw_set_collidables`: local records (body frame), resident until replaced"""
        c = np.ascontiguousarray(collidables, dtype=COLLIDABLE_DTYPE).reshape(-1)
        check(capi.lib().ivx_cw_set_collidables(self.world.h, ptr(c) if c.size else None, c.size))
        self.n = c.size

    def set_broad_phase(self, which: int) -> None:
        """`ivx_cw_set_broad_phase`: capi.CW_BROAD_FLAT (the default) or capi.CW_BROAD_HIERARCHY — where `collide` takes its pairs from"""
        check(capi.lib().ivx_cw_set_broad_phase(self.world.h, int(which)))

    def synchronize(self) -> BoundingVolumeSet:
        """`ivx_cw_synchronize`: enqueued behind whatever the stream holds -> the context's bounding-volume set of the world boxes"""
        check(capi.lib().ivx_cw_synchronize(self.world.h))
        return BoundingVolumeSet(self.world.ctx.h, self.n)

    def download(self) -> np.ndarray:
        """`ivx_cw_download`: the world-space collidables of the last synchronize"""
        out = np.zeros(self.n, dtype=COLLIDABLE_DTYPE)
        check(capi.lib().ivx_cw_download(self.world.h, ptr(out) if self.n else None, self.n))
        return out

    def collide(self, mode: int = capi.BV_DYNAMIC_PAIRS, capacity: int | None = None, deferred_capacity: int | None = None):
        """`ivx_cw_collide` -> (contacts [n] CONTACT_DTYPE, deferred pairs [m, 2] uint32), both in pair order. A capacity of None: sized by a first
        call that only counts."""
        lib = capi.lib()
        n, m = C.c_size_t(0), C.c_size_t(0)
        if capacity is None or deferred_capacity is None:
            check(lib.ivx_cw_collide(self.world.h, int(mode), None, 0, C.byref(n), None, 0, C.byref(m)))
            capacity = n.value if capacity is None else capacity
            deferred_capacity = m.value if deferred_capacity is None else deferred_capacity
        contacts, deferred = np.zeros(max(1, capacity), dtype=CONTACT_DTYPE), np.zeros((max(1, deferred_capacity), 2), dtype=np.uint32)
        check(lib.ivx_cw_collide(self.world.h, int(mode), ptr(contacts), capacity, C.byref(n), ptr(deferred), deferred_capacity, C.byref(m)))
        return contacts[: n.value], deferred[: m.value]

    def set_voxel_objects(self, attachments) -> None:
        """`ivx_cw_set_voxel_objects`: {collidable index: (grid, origin_offset, center_of_mass)}, replacing what was attached before. The grids' ranges
        and probes are read at every `collide_frame`: call again only when an origin offset or a centre of mass moved (or after `set_collidables`)"""
        index = np.array(sorted(attachments), dtype=np.uint32)
        records = np.array([voxel_object_record(*attachments[int(i)]) for i in index], dtype=CW_VOXEL_OBJECT_DTYPE).reshape(-1)
        check(capi.lib().ivx_cw_set_voxel_objects(self.world.h, ptr(index) if index.size else None, ptr(records) if index.size else None, index.size))

    def collide_frame(self, mode: int = capi.BV_DYNAMIC_PAIRS, capacity: int | None = None, deferred_capacity: int | None = None):
        """`ivx_cw_collide_frame` -> (merged contacts: the primitive ones, then one manifold per deferred pair in deferred-list order; n_primitive;
        deferred pairs [m, 2] uint32; manifold offsets [m + 1] uint32 counted from n_primitive). A capacity of None: sized by a first call that leaves
        the lists on the device."""
        lib = capi.lib()
        n, n_primitive, m = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        if capacity is None or deferred_capacity is None:
            check(lib.ivx_cw_collide_frame(self.world.h, int(mode), None, 0, C.byref(n), C.byref(n_primitive), None, None, 0, C.byref(m)))
            capacity = n.value if capacity is None else capacity
            deferred_capacity = m.value if deferred_capacity is None else deferred_capacity
        contacts, deferred = np.zeros(max(1, capacity), dtype=CONTACT_DTYPE), np.zeros((max(1, deferred_capacity), 2), dtype=np.uint32)
        offsets = np.zeros(deferred_capacity + 1, dtype=np.uint32)
        check(lib.ivx_cw_collide_frame(self.world.h, int(mode), ptr(contacts), capacity, C.byref(n), C.byref(n_primitive), ptr(deferred), ptr(offsets), deferred_capacity,
                                       C.byref(m)))
        return contacts[: n.value], n_primitive.value, deferred[: m.value], offsets[: m.value + 1]

    def rows(self) -> np.ndarray:
        """`ivx_cw_rows_download`: the CW_VOXEL_ROW_DTYPE records of the last `collide_frame`, in deferred-list order"""
        lib, n = capi.lib(), C.c_size_t(0)
        rc = lib.ivx_cw_rows_download(self.world.h, None, 0, C.byref(n))
        if rc != capi.IVX_ERR_CAPACITY:
            check(rc)
        out = np.zeros(max(1, n.value), dtype=CW_VOXEL_ROW_DTYPE)
        check(lib.ivx_cw_rows_download(self.world.h, ptr(out), n.value, C.byref(n)))
        return out[: n.value]

    def device_ptr(self, which: int) -> int:
        """`ivx_cw_device_ptr`: capi.CW_PTR_WORLD_COLLIDABLES / _CONTACTS / _DEFERRED_PAIRS / _FRAME_CONTACTS / _VOXEL_ROWS"""
        return int(capi.lib().ivx_cw_device_ptr(self.world.h, int(which)) or 0)
