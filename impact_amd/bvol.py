"""Host-side mirror of the bounding volume calls (`ivx_bv_*`, impact_amd/csrc/bvol.hip): what the reference's `IntersectionManager`
(impact_intersection/src/lib.rs) answers from its hierarchy, as flat exact passes over the world boxes of a frame:

  add_bounding_volume_to_hierarchy                 lib.rs:39-54            (`world_aabb`, `set_boxes`)
  sync_voxel_object_bounding_volume                interaction.rs:202-222  (`grid_model_aabb`, `set_grids`)
  for_each_intersecting_bounding_volume_pair       collision.rs:215-349    (`BoundingVolumeSet.pairs`)
  for_each_bounding_volume_in_* / _maybe_in_*      absorption.rs:474, model.rs:191, light.rs:172-543  (`BoundingVolumeSet.query`)

The pair pass has a second form that leaves the same bytes: a linear hierarchy over the set (csrc/bvh.hip; hierarchy.rs in the reference), built
on request (`BoundingVolumeSet.build_hierarchy`, `.hierarchy`, `.pairs_hierarchy`; `morton_key`, `hierarchy_host` and `node_info` on the host).
So have the region queries (`.query_hierarchy`; `queries_hierarchy_host` and `query_skips_boxes` on the host), and the masks of either form
become hit lists on the device (`.query_lists`). The flat forms are the default.

The world boxes, the pairs, the masks, the hit lists and the tree stay in context-owned device buffers (`device_ptr`). Nothing here computes,
and nothing falls back to the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import AABB_DTYPE, BV_NODE_DTYPE, BV_QUERY_DTYPE, SIMILARITY_DTYPE, check, ptr
from .many import _handles


def boxes(lower, upper) -> np.ndarray:
    """`ivx_aabb` records from [n, 3] lower and upper corners"""
    lower = np.asarray(lower, dtype=np.float32).reshape(-1, 3)
    b = np.zeros(len(lower), dtype=AABB_DTYPE)
    b["lower"], b["upper"] = lower, np.asarray(upper, dtype=np.float32).reshape(-1, 3)
    return b


def similarities(n: int) -> np.ndarray:
    """`n` identity `ivx_similarity` records"""
    s = np.zeros(n, dtype=SIMILARITY_DTYPE)
    s["rotation"][:, 3] = 1.0
    s["scaling"] = 1.0
    return s


def _rec(a, dtype, n=None):
    a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
    assert n is None or a.size == n, (a.size, n)
    return a


def world_aabb(model, similarity) -> np.ndarray:
    """`ivx_bv_world_aabb`: one box under one similarity, host arithmetic of the library"""
    out = np.zeros(1, dtype=AABB_DTYPE)
    check(capi.lib().ivx_bv_world_aabb(ptr(_rec(model, AABB_DTYPE, 1)), ptr(_rec(similarity, SIMILARITY_DTYPE, 1)), ptr(out)))
    return out[0]


def grid_model_aabb(voxel_object) -> np.ndarray:
    """`ivx_grid_model_aabb`: the model-space box of the occupied voxel ranges the object holds"""
    out = np.zeros(1, dtype=AABB_DTYPE)
    check(capi.lib().ivx_grid_model_aabb(voxel_object.h, ptr(out)))
    return out[0]


# ---- the four query kinds ----------------------------------------------------------------------------------------------------------------
def box_query(lower, upper) -> np.ndarray:
    q = np.zeros((), dtype=BV_QUERY_DTYPE)
    q["kind"], q["lower"], q["upper"] = capi.BV_QUERY_BOX, lower, upper
    return q


def sphere_query(center, radius: float) -> np.ndarray:
    q = np.zeros((), dtype=BV_QUERY_DTYPE)
    q["kind"], q["center"], q["radius"] = capi.BV_QUERY_SPHERE, center, radius
    return q


def frustum_query(planes) -> np.ndarray:
    """`ivx_bv_frustum_query`: six world-space planes (unit normal xyz, displacement); the library picks the corners"""
    q = np.zeros(1, dtype=BV_QUERY_DTYPE)
    check(capi.lib().ivx_bv_frustum_query(ptr(np.ascontiguousarray(planes, dtype=np.float32).reshape(6, 4)), ptr(q)))
    return q[0]


def oriented_box_query(center, orientation_xyzw, half_extents) -> np.ndarray:
    """an oriented box from its centre, orientation quaternion (box frame -> world) and half extents: `axes` are the rows of the rotation from
    world space into the box frame, i.e. the box's axes in world space (computed in float64, rounded once)"""
    x, y, z, w = (float(v) for v in orientation_xyzw)
    r = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    q = np.zeros((), dtype=BV_QUERY_DTYPE)
    q["kind"], q["axes"], q["box_center"], q["half_extents"] = capi.BV_QUERY_ORIENTED_BOX, r.T, center, half_extents
    return q


def query_array(records) -> np.ndarray:
    """several query records as one contiguous BV_QUERY_DTYPE array, copied as bytes (the dtype's fields overlap: numpy would otherwise copy
    field by field)"""
    if isinstance(records, np.ndarray) and records.dtype == BV_QUERY_DTYPE:
        return np.ascontiguousarray(records).reshape(-1)
    out = np.zeros(len(records), dtype=BV_QUERY_DTYPE)
    raw = out.view(np.uint8).reshape(len(records), BV_QUERY_DTYPE.itemsize)
    for i, r in enumerate(records):
        r = np.asarray(r)
        assert r.dtype == BV_QUERY_DTYPE and r.size == 1
        raw[i] = np.frombuffer(r.tobytes(), dtype=np.uint8)
    return out


def mask_indices(masks: np.ndarray, n: int):
    """a [n_queries, ceil(n / 64)] mask array as one sorted index array per query"""
    masks = np.ascontiguousarray(masks, dtype="<u8").reshape(masks.shape[0], -1)
    bits = np.unpackbits(masks.view(np.uint8), axis=1, bitorder="little")[:, :n] if masks.shape[1] else np.zeros((masks.shape[0], 0), dtype=np.uint8)
    return [np.nonzero(row)[0].astype(np.uint32) for row in bits]


class BoundingVolumeSet:
    """The set of world boxes a context holds after `set_boxes` / `set_grids`; valid until the context's next set."""

    def __init__(self, ctx_handle, n: int):
        self._h, self.n = ctx_handle, n

    def download(self):
        """`ivx_bv_download` -> (world boxes [n], the box around all of them)"""
        world, total = np.zeros(self.n, dtype=AABB_DTYPE), np.zeros(1, dtype=AABB_DTYPE)
        check(capi.lib().ivx_bv_download(self._h, ptr(world) if self.n else None, self.n, ptr(total)))
        return world, total[0]

    def pairs(self, mode: int = capi.BV_ALL_PAIRS, capacity: int | None = None) -> np.ndarray:
        """`ivx_bv_pairs` -> [n_pairs, 2] uint32, sorted by (a, b). `capacity` None: sized by a first call that only counts"""
        found = C.c_size_t(0)
        if capacity is None:
            rc = capi.lib().ivx_bv_pairs(self._h, int(mode), ptr(np.zeros((1, 2), dtype=np.uint32)), 0, C.byref(found))
            if rc != capi.IVX_ERR_CAPACITY:
                check(rc)
                return np.zeros((0, 2), dtype=np.uint32)
            capacity = found.value
        out = np.zeros((max(1, capacity), 2), dtype=np.uint32)
        check(capi.lib().ivx_bv_pairs(self._h, int(mode), ptr(out), capacity, C.byref(found)))
        return out[: found.value]

    def query(self, queries):
        """`ivx_bv_queries` -> (masks [n_queries, ceil(n / 64)] uint64, counts [n_queries] uint32)"""
        q = query_array(queries)
        words = (self.n + 63) // 64
        masks, counts = np.zeros((q.size, words), dtype=np.uint64), np.zeros(q.size, dtype=np.uint32)
        check(capi.lib().ivx_bv_queries(self._h, ptr(q) if q.size else None, q.size, ptr(masks) if masks.size else None, ptr(counts) if q.size else None))
        return masks, counts

    def query_hierarchy(self, queries):
        """`ivx_bv_queries_hierarchy` -> what `query` returns, found through the tree (`build_hierarchy` first)"""
        q = query_array(queries)
        words = (self.n + 63) // 64
        masks, counts = np.zeros((q.size, words), dtype=np.uint64), np.zeros(q.size, dtype=np.uint32)
        check(capi.lib().ivx_bv_queries_hierarchy(self._h, ptr(q) if q.size else None, q.size, ptr(masks) if masks.size else None, ptr(counts) if q.size else None))
        return masks, counts

    def query_lists(self, capacity: int | None = None):
        """`ivx_bv_query_lists`: the hits of the last `query` / `query_hierarchy` as lists made on the device -> (offsets [n_queries + 1] uint32,
        objects [offsets[-1]] uint32; query q's objects are objects[offsets[q]:offsets[q + 1]], ascending). `capacity` None: sized by a first call
        that leaves the lists on the device only"""
        found = C.c_size_t(0)
        if capacity is None:
            check(capi.lib().ivx_bv_query_lists(self._h, None, None, 0, C.byref(found)))
            capacity = found.value
        # (the call knows how many queries the context's last call had; an offset never reaches 2^32 - 1, so what it wrote can be told)
        offsets, objects = np.full(capi.BV_MAX_QUERIES + 1, 0xFFFFFFFF, dtype=np.uint32), np.zeros(max(1, capacity), dtype=np.uint32)
        check(capi.lib().ivx_bv_query_lists(self._h, ptr(offsets), ptr(objects), capacity, C.byref(found)))
        return offsets[: int(np.count_nonzero(offsets != 0xFFFFFFFF))].copy(), objects[: found.value]

    def device_ptr(self, which: int) -> int:
        """`ivx_bv_device_ptr`: capi.BV_PTR_WORLD_BOXES / _PAIRS / _MASKS / _NODES / _LEAF_OBJECTS / _HIT_OFFSETS / _HIT_OBJECTS"""
        return int(capi.lib().ivx_bv_device_ptr(self._h, int(which)) or 0)

    def build_hierarchy(self) -> None:
        """`ivx_bv_build_hierarchy`: the linear BVH over this set, enqueued on the context's stream"""
        check(capi.lib().ivx_bv_build_hierarchy(self._h))

    def hierarchy(self):
        """`ivx_bv_hierarchy_download` -> (nodes [max(n - 1, 0)] BV_NODE_DTYPE, leaf objects [n] uint32 in Morton order)"""
        nodes, leaves = np.zeros(max(self.n - 1, 0), dtype=BV_NODE_DTYPE), np.zeros(self.n, dtype=np.uint32)
        found = C.c_size_t(0)
        check(capi.lib().ivx_bv_hierarchy_download(self._h, ptr(nodes) if nodes.size else None, nodes.size, ptr(leaves) if self.n else None, self.n, C.byref(found)))
        assert found.value == nodes.size, (found.value, nodes.size)
        return nodes, leaves

    def pairs_hierarchy(self, mode: int = capi.BV_ALL_PAIRS, capacity: int | None = None) -> np.ndarray:
        """`ivx_bv_pairs_hierarchy` -> what `pairs` returns, found through the tree. `capacity` None: sized by a first call that only counts"""
        found = C.c_size_t(0)
        if capacity is None:
            rc = capi.lib().ivx_bv_pairs_hierarchy(self._h, int(mode), ptr(np.zeros((1, 2), dtype=np.uint32)), 0, C.byref(found))
            if rc != capi.IVX_ERR_CAPACITY:
                check(rc)
                return np.zeros((0, 2), dtype=np.uint32)
            capacity = found.value
        out = np.zeros((max(1, capacity), 2), dtype=np.uint32)
        check(capi.lib().ivx_bv_pairs_hierarchy(self._h, int(mode), ptr(out), capacity, C.byref(found)))
        return out[: found.value]


def morton_key(frame, box, index: int) -> int:
    """`ivx_bv_morton_key`: (code << 32) | index of one box in a frame, host arithmetic of the library"""
    key = C.c_uint64(0)
    check(capi.lib().ivx_bv_morton_key(ptr(_rec(frame, AABB_DTYPE, 1)), ptr(_rec(box, AABB_DTYPE, 1)), int(index), C.byref(key)))
    return int(key.value)


def hierarchy_host(world_boxes, nodes=None, leaf_objects=None):
    """`ivx_bv_hierarchy_host`: the hierarchy of n world boxes on the host -> (nodes [max(n - 1, 0)], leaf objects [n], frame). The C call takes no
    capacities, so arrays given to be filled are measured here: one that is too short raises an IvxError of IVX_ERR_CAPACITY before the call."""
    w = _rec(world_boxes, AABB_DTYPE)
    n, nn = w.size, max(w.size - 1, 0)
    nodes = np.zeros(nn, dtype=BV_NODE_DTYPE) if nodes is None else nodes
    leaf_objects = np.zeros(n, dtype=np.uint32) if leaf_objects is None else leaf_objects
    for a, dtype, need, what in ((nodes, BV_NODE_DTYPE, nn, "node"), (leaf_objects, np.dtype(np.uint32), n, "leaf object")):
        assert a.dtype == dtype and a.flags.c_contiguous, what
        if a.size < need:
            raise capi.IvxError(capi.IVX_ERR_CAPACITY, f"hierarchy_host: {need} {what}s, the array holds {a.size}")
    frame = np.zeros(1, dtype=AABB_DTYPE)
    check(capi.lib().ivx_bv_hierarchy_host(ptr(w) if n else None, n, ptr(nodes) if nn else None, ptr(leaf_objects) if n else None, ptr(frame)))
    return nodes[:nn], leaf_objects[:n], frame[0]


def queries_hierarchy_host(world_boxes, nodes, leaf_objects, queries):
    """`ivx_bv_queries_hierarchy_host`: the queries through a tree on the host (`hierarchy_host`'s, say), with the decision functions the kernels
    run -> (masks [n_queries, ceil(n / 64)] uint64, counts [n_queries] uint32). A tree that is none raises an IvxError of IVX_ERR_STATE."""
    w, q = _rec(world_boxes, AABB_DTYPE), query_array(queries)
    n, nn = w.size, max(w.size - 1, 0)
    nodes, leaf_objects = _rec(nodes, BV_NODE_DTYPE, nn), _rec(leaf_objects, np.uint32, n)
    masks, counts = np.zeros((q.size, (n + 63) // 64), dtype=np.uint64), np.zeros(q.size, dtype=np.uint32)
    check(capi.lib().ivx_bv_queries_hierarchy_host(ptr(w) if n else None, n, ptr(nodes) if nn else None, ptr(leaf_objects) if n else None, ptr(q) if q.size else None, q.size,
                                                   ptr(masks) if masks.size else None, ptr(counts) if q.size else None))
    return masks, counts


def query_skips_boxes(queries, node_boxes) -> np.ndarray:
    """`ivx_bv_query_skips_boxes`: the node decision of the queries' walk for every query and every box (AABB_DTYPE or BV_NODE_DTYPE records), host
    arithmetic of the library -> [n_queries, n_boxes] bool, True where no proper box inside the box can be hit"""
    q, b = query_array(queries), np.asarray(node_boxes)
    if b.dtype != AABB_DTYPE:
        b = boxes(b["lower"], b["upper"])
    b = _rec(b, AABB_DTYPE)
    skips = np.zeros((q.size, b.size), dtype=np.uint8)
    check(capi.lib().ivx_bv_query_skips_boxes(ptr(q) if q.size else None, q.size, ptr(b) if b.size else None, b.size, ptr(skips) if skips.size else None))
    return skips.astype(bool)


def node_info(nodes, n: int):
    """per internal node its depth (the root: 0) and the number of leaves below it — what the reference's BVHNodeInfo carries for its gizmo
    (hierarchy.rs) -> (depth [n - 1] uint32, primitive_count [n - 1] uint32). A tree deeper than 64 or with a child out of range is refused."""
    nn = max(int(n) - 1, 0)
    depth, count = np.zeros(nn, dtype=np.uint32), np.zeros(nn, dtype=np.uint32)
    if nn == 0:
        return depth, count
    left, right = nodes["left"].astype(np.int64), nodes["right"].astype(np.int64)
    order, stack = [], [(0, 0)]
    while stack:
        i, d = stack.pop()
        if not (0 <= i < nn) or d > 64 or len(order) >= nn:
            raise ValueError(f"node_info: node {i} at depth {d} is not part of a tree of {nn} nodes")
        depth[i] = d
        order.append(i)
        stack.extend((c, d + 1) for c in (int(left[i]), int(right[i])) if not c & capi.BV_LEAF)
    for i in reversed(order):  # (children come behind their parent in `order`)
        count[i] = sum(1 if c & capi.BV_LEAF else int(count[c]) for c in (int(left[i]), int(right[i])))
    return depth, count


def _kinds(kinds, n):
    if kinds is None:
        return None
    k = np.ascontiguousarray(kinds, dtype=np.uint32).reshape(-1)
    assert k.size == n, (k.size, n)
    return k


def set_boxes(ctx, model_boxes, similarity_records=None, kinds=None) -> BoundingVolumeSet:
    """`ivx_bv_set`: model boxes under their similarities (None: the boxes are world boxes already), kinds (None: all dynamic)"""
    b = _rec(model_boxes, AABB_DTYPE)
    s = None if similarity_records is None else _rec(similarity_records, SIMILARITY_DTYPE, b.size)
    k = _kinds(kinds, b.size)
    check(capi.lib().ivx_bv_set(ctx.h, ptr(b) if b.size else None, ptr(s) if s is not None and b.size else None, ptr(k) if k is not None and b.size else None, b.size))
    return BoundingVolumeSet(ctx.h, b.size)


def set_grids(voxel_objects, similarity_records=None, kinds=None) -> BoundingVolumeSet:
    """`ivx_bv_set_grids`: the same with every object's `grid_model_aabb` as its model box"""
    n = len(voxel_objects)
    s = None if similarity_records is None else _rec(similarity_records, SIMILARITY_DTYPE, n)
    k = _kinds(kinds, n)
    check(capi.lib().ivx_bv_set_grids(ptr(_handles(voxel_objects)) if n else None, n, ptr(s) if s is not None and n else None, ptr(k) if k is not None and n else None))
    return BoundingVolumeSet(voxel_objects[0].ctx.h if n else None, n)
