"""Host-side mirror of chunk culling (`ivx_cull_*`, impact_amd/csrc/cull.hip): what the reference's `VoxelChunkCullingPass` records as one compute
dispatch per object per view (impact_voxel/src/render_commands.rs:392-598, shaders/compute/voxel_chunk_culling.template.wgsl), as one call over
all objects and all views of a frame:

  CullingFrustum                                  mesh.rs:128-131, 638-696   (`culling_frustum_from_view`, CULLING_FRUSTUM_DTYPE)
  VoxelChunkCullingPass::record_*                 render_commands.rs:392-589 (`cull_many`, `cull_submesh_tables`)

The draw arguments stay in a context-owned device buffer (`device_ptr`); `CullResult` downloads regions on demand. Nothing here computes, and
nothing falls back to the CPU.
"""
from __future__ import annotations

import numpy as np

from . import capi
from .capi import (CULL_COUNT_DTYPE, CULL_OBJECT_DTYPE, CULL_PAIR_DTYPE, CULL_REGION_DTYPE, CULL_VIEW_DTYPE, CULLING_FRUSTUM_DTYPE, DRAW_ARGS_DTYPE,
                   DRAW_INDEXED_ARGS_DTYPE, SUBMESH_DTYPE, check, ptr)
from .many import _handles


def views(n: int) -> np.ndarray:
    """`n` zeroed `ivx_cull_view` records with identity box orientations"""
    v = np.zeros(n, dtype=CULL_VIEW_DTYPE)
    v["box_orientation"][:, 3] = 1.0
    return v


def pairs(n_views: int, n_objects: int) -> np.ndarray:
    """[n_views, n_objects] `ivx_cull_pair` records: identity similarities, instance index = object index"""
    p = np.zeros((n_views, n_objects), dtype=CULL_PAIR_DTYPE)
    p["rotation"][..., 3] = 1.0
    p["scaling"] = 1.0
    p["instance_idx"] = np.arange(n_objects, dtype=np.uint32)[None, :]
    return p


def _rec(a, dtype, n=None):
    a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
    assert n is None or a.size == n, (a.size, n)
    return a


def culling_frustum_from_view(view, pair, chunk_extent: float) -> np.ndarray:
    """`ivx_culling_frustum_from_view`: the record of one view and one pair, host arithmetic of the library"""
    out = np.zeros(1, dtype=CULLING_FRUSTUM_DTYPE)
    check(capi.lib().ivx_culling_frustum_from_view(ptr(_rec(view, CULL_VIEW_DTYPE, 1)), ptr(_rec(pair, CULL_PAIR_DTYPE, 1)), float(chunk_extent), ptr(out)))
    return out[0]


def cull_frusta(ctx, view_records, pair_records, chunk_extents) -> np.ndarray:
    """`ivx_cull_frusta`: the derivation stage alone on the device -> [n_views, n_objects] records"""
    v = _rec(view_records, CULL_VIEW_DTYPE)
    e = np.ascontiguousarray(chunk_extents, dtype=np.float32).reshape(-1)
    p = _rec(pair_records, CULL_PAIR_DTYPE, v.size * e.size)
    out = np.zeros((v.size, e.size), dtype=CULLING_FRUSTUM_DTYPE)
    check(capi.lib().ivx_cull_frusta(ctx.h, ptr(v), v.size, ptr(p), ptr(e), e.size, ptr(out)))
    return out


class CullResult:
    """What a cull call left on the device: `layout` (CULL_REGION_DTYPE per view), `counts` (CULL_COUNT_DTYPE per view; None after an enqueue
    until `collect`), and downloads of a view's region, count record and frustum records. Valid until the context's next cull call."""

    def __init__(self, ctx_handle, layout, counts, n_objects):
        self._h, self.layout, self.counts, self.n_objects = ctx_handle, layout, counts, n_objects

    def collect(self):
        """`ivx_cull_collect`: wait, and bring the views' counts back"""
        self.counts = np.zeros(self.layout.size, dtype=CULL_COUNT_DTYPE)
        check(capi.lib().ivx_cull_collect(self._h, ptr(self.counts) if self.layout.size else None, self.layout.size))
        return self

    def download(self, view: int):
        """`ivx_cull_download` -> (args: DRAW_ARGS_DTYPE or DRAW_INDEXED_ARGS_DTYPE per slot, count record, the view's frustum records)"""
        r = self.layout[view]
        args = np.zeros(int(r["n_slots"]), dtype=DRAW_INDEXED_ARGS_DTYPE if int(r["stride"]) == 20 else DRAW_ARGS_DTYPE)
        count = np.zeros(1, dtype=CULL_COUNT_DTYPE)
        frusta = np.zeros(max(1, self.n_objects), dtype=CULLING_FRUSTUM_DTYPE)
        check(capi.lib().ivx_cull_download(self._h, int(view), ptr(args) if args.size else None, args.nbytes, ptr(count), ptr(frusta), frusta.size))
        return args, count[0], frusta[: self.n_objects]

    def device_ptr(self, which: int) -> int:
        """`ivx_cull_device_ptr`: capi.CULL_PTR_ARGS / _COUNTS / _FRUSTA"""
        return int(capi.lib().ivx_cull_device_ptr(self._h, int(which)) or 0)


def _tables(tables):
    tabs = [np.ascontiguousarray(t, dtype=SUBMESH_DTYPE).reshape(-1) for t in tables]
    counts = np.fromiter((t.size for t in tabs), dtype=np.uint32, count=len(tabs))
    addr = np.fromiter((t.__array_interface__["data"][0] if t.size else 0 for t in tabs), dtype=np.uint64, count=len(tabs))
    return tabs, counts, addr


def _objects(objects, n):
    return None if objects is None else _rec(objects, CULL_OBJECT_DTYPE, n)


def cull_submesh_tables(ctx, tables, chunk_extents, view_records, pair_records, mode: int = capi.CULL_ZEROED, objects=None) -> CullResult:
    """`ivx_cull_submesh_tables`: host submesh tables (one SUBMESH_DTYPE array per object), uploaded for the call"""
    tabs, counts, addr = _tables(tables)
    n = len(tabs)
    v = _rec(view_records, CULL_VIEW_DTYPE)
    p = _rec(pair_records, CULL_PAIR_DTYPE, v.size * n)
    e = np.ascontiguousarray(chunk_extents, dtype=np.float32).reshape(-1)
    assert e.size == n
    o = _objects(objects, n)
    layout, cnt = np.zeros(v.size, dtype=CULL_REGION_DTYPE), np.zeros(v.size, dtype=CULL_COUNT_DTYPE)
    check(capi.lib().ivx_cull_submesh_tables(ctx.h, ptr(addr) if n else None, ptr(counts) if n else None, n, ptr(o) if o is not None and n else None, ptr(e) if n else None,
                                             ptr(v) if v.size else None, v.size, ptr(p) if p.size else None, int(mode), ptr(layout) if v.size else None,
                                             ptr(cnt) if v.size else None))
    return CullResult(ctx.h, layout, cnt, n)


def cull_submesh_tables_frusta(ctx, tables, frusta, view_flags, pair_flags=None, mode: int = capi.CULL_ZEROED, objects=None) -> CullResult:
    """`ivx_cull_submesh_tables_frusta`: the same with ready [n_views, n_objects] frustum records"""
    tabs, counts, addr = _tables(tables)
    n = len(tabs)
    vf = np.ascontiguousarray(view_flags, dtype=np.uint32).reshape(-1)
    f = _rec(frusta, CULLING_FRUSTUM_DTYPE, vf.size * n)
    pf = None if pair_flags is None else np.ascontiguousarray(pair_flags, dtype=np.uint32).reshape(-1)
    assert pf is None or pf.size == vf.size * n
    o = _objects(objects, n)
    layout, cnt = np.zeros(vf.size, dtype=CULL_REGION_DTYPE), np.zeros(vf.size, dtype=CULL_COUNT_DTYPE)
    check(capi.lib().ivx_cull_submesh_tables_frusta(ctx.h, ptr(addr) if n else None, ptr(counts) if n else None, n, ptr(o) if o is not None and n else None,
                                                    ptr(f) if f.size else None, ptr(vf) if vf.size else None, ptr(pf) if pf is not None and pf.size else None, vf.size,
                                                    int(mode), ptr(layout) if vf.size else None, ptr(cnt) if vf.size else None))
    return CullResult(ctx.h, layout, cnt, n)


def cull_many(voxel_objects, view_records, pair_records, mode: int = capi.CULL_ZEROED, objects=None, enqueue_only: bool = False) -> CullResult:
    """`ivx_cull_many` over the objects' resident submesh tables (`enqueue_only`: `ivx_cull_many_enqueue`, the counts come with
    `CullResult.collect`)"""
    n = len(voxel_objects)
    v = _rec(view_records, CULL_VIEW_DTYPE)
    p = _rec(pair_records, CULL_PAIR_DTYPE, v.size * n)
    o = _objects(objects, n)
    layout, cnt = np.zeros(v.size, dtype=CULL_REGION_DTYPE), np.zeros(v.size, dtype=CULL_COUNT_DTYPE)
    handles = _handles(voxel_objects)
    args = [ptr(handles) if n else None, n, ptr(o) if o is not None and n else None, ptr(v) if v.size else None, v.size, ptr(p) if p.size else None, int(mode),
            ptr(layout) if v.size else None]
    ctx_handle = voxel_objects[0].ctx.h if n else None  # (no objects: the call touches no context, and there is nothing to download)
    if enqueue_only:
        check(capi.lib().ivx_cull_many_enqueue(*args))
        return CullResult(ctx_handle, layout, None if n else cnt, n)
    check(capi.lib().ivx_cull_many(*args, ptr(cnt) if v.size else None))
    return CullResult(ctx_handle, layout, cnt, n)


def cull_many_frusta(voxel_objects, frusta, view_flags, pair_flags=None, mode: int = capi.CULL_ZEROED, objects=None) -> CullResult:
    """`ivx_cull_many_frusta`: resident tables, ready [n_views, n_objects] frustum records"""
    n = len(voxel_objects)
    vf = np.ascontiguousarray(view_flags, dtype=np.uint32).reshape(-1)
    f = _rec(frusta, CULLING_FRUSTUM_DTYPE, vf.size * n)
    pf = None if pair_flags is None else np.ascontiguousarray(pair_flags, dtype=np.uint32).reshape(-1)
    o = _objects(objects, n)
    layout, cnt = np.zeros(vf.size, dtype=CULL_REGION_DTYPE), np.zeros(vf.size, dtype=CULL_COUNT_DTYPE)
    check(capi.lib().ivx_cull_many_frusta(ptr(_handles(voxel_objects)) if n else None, n, ptr(o) if o is not None and n else None, ptr(f) if f.size else None,
                                          ptr(vf) if vf.size else None, ptr(pf) if pf is not None and pf.size else None, vf.size, int(mode),
                                          ptr(layout) if vf.size else None, ptr(cnt) if vf.size else None))
    return CullResult(voxel_objects[0].ctx.h if n else None, layout, cnt, n)
