"""Host-side mirror of the reference's voxel-object interface for the hot path, on top of the C ABI.

Class and method names follow engine/crates/impact_voxel so that parity tests read like the
reference's own tests:
  SDFVoxelGenerator            generation.rs:69-77, 204-258
  VoxelObject                  object.rs:45-57, 223-263, 1136-1198; split_detection.rs:186-301
  VoxelObjectMesh              mesh.rs:44-58, 267-354
  VoxelObjectInertialPropertyManager   object/inertia.rs:20-25, 113-169, 288-326
All compute happens in libimpact_voxel_hip.so (HIP, gfx950); nothing here falls back to the CPU.
"""
from __future__ import annotations

import atexit
import ctypes as C
import sys
import weakref

import numpy as np

from . import capi
from .capi import check, ptr
from .sdf_graph import PROCESSED_NODE_DTYPE, SDFGraph

CHUNK_SIZE = 16
CHUNK_VOXEL_COUNT = 4096

# Device objects must be released before the HIP runtime unloads at interpreter exit.
_live_grids: "weakref.WeakSet" = weakref.WeakSet()
_live_contexts: "weakref.WeakSet" = weakref.WeakSet()


@atexit.register
def _release_device_objects():
    for g in list(_live_grids):
        g.close()
    for c in list(_live_contexts):
        c.close()


class Context:
    """One per process and GPU (`ivx_ctx`)."""

    def __init__(self, device: int = 0, stream: int | None = None):
        h = C.c_void_p()
        check(capi.lib().ivx_init(device, C.c_void_p(stream) if stream else None, C.byref(h)))
        self.h = h
        self.device = device
        _live_contexts.add(self)

    def synchronize(self):
        check(capi.lib().ivx_synchronize(self.h))

    @property
    def stream(self) -> int:
        return capi.lib().ivx_stream(self.h) or 0

    def close(self):
        if getattr(self, "h", None):
            capi.lib().ivx_shutdown(self.h)
            self.h = None

    def __del__(self):
        if not sys.is_finalizing():
            try:
                self.close()
            except Exception:
                pass


class SDFGenerator:
    """Compiled atomic SDF graph (`SDFGenerator`, generation/sdf/atomic.rs:33-40, 228-596)."""

    def __init__(self, graph: SDFGraph):
        nodes = graph.nodes()
        cap = 4 * max(1, len(nodes)) + 64
        for _ in range(8):
            out = np.zeros(cap, dtype=PROCESSED_NODE_DTYPE)
            n_out = C.c_size_t(0)
            dom = np.zeros(6, dtype=np.float32)
            ss = C.c_uint32(0)
            rc = capi.lib().ivx_sdf_compile(ptr(nodes) if len(nodes) else None, len(nodes), graph.root_node_id, ptr(out), cap,
                                            C.byref(n_out), ptr(dom), C.byref(ss))
            if rc == capi.IVX_ERR_CAPACITY:
                cap *= 4
                continue
            check(rc)
            break
        self.nodes = np.ascontiguousarray(out[: n_out.value])
        self.domain = dom
        self.required_forward_stack_size = int(ss.value)

    def is_empty(self):
        return len(self.nodes) == 0


class SameVoxelTypeGenerator:
    """`SameVoxelTypeGenerator` (generation/voxel_type.rs:18-25, 88-96): every voxel gets the one type."""

    def __init__(self, voxel_type: int = 0):
        assert 0 <= int(voxel_type) <= 255
        self.voxel_type = int(voxel_type)

    def _noise_args(self):
        return (0, 0.0, 0.0, 0)


class GradientNoiseVoxelTypeGenerator:
    """`GradientNoiseVoxelTypeGenerator` (generation/voxel_type.rs:27-36, 97-169): a 4D gradient noise value per candidate type, the
    voxel takes the index of the greatest. The reference's list of voxel types enters by its length alone."""

    def __init__(self, n_voxel_types: int, noise_frequency: float, voxel_type_frequency: float, seed: int):
        self.n_voxel_types = int(n_voxel_types)
        self.noise_frequency = float(noise_frequency)
        self.voxel_type_frequency = float(voxel_type_frequency)
        self.seed = int(seed) & 0xFFFFFFFF
        self.voxel_type = 0  # (the sample calls' voxel_type argument, ignored under this generator)

    def _noise_args(self):
        return (self.n_voxel_types, self.noise_frequency, self.voxel_type_frequency, self.seed)


class SDFVoxelGenerator:
    """`SDFVoxelGenerator::new(voxel_extent, sdf_generator, voxel_type_generator)`; an int as the third argument stands for
    `SameVoxelTypeGenerator(voxel_type)`."""

    def __init__(self, voxel_extent: float, sdf_generator: SDFGenerator | SDFGraph,
                 voxel_type: "int | SameVoxelTypeGenerator | GradientNoiseVoxelTypeGenerator" = 0):
        assert voxel_extent > 0.0
        if isinstance(sdf_generator, SDFGraph):
            sdf_generator = SDFGenerator(sdf_generator)
        self.voxel_extent = float(voxel_extent)
        self.sdf_generator = sdf_generator
        if not isinstance(voxel_type, (SameVoxelTypeGenerator, GradientNoiseVoxelTypeGenerator)):
            voxel_type = SameVoxelTypeGenerator(int(voxel_type))
        self.voxel_type_generator = voxel_type
        self.voxel_type = voxel_type.voxel_type
        shape = np.zeros(3, dtype=np.uint32)
        centre = np.zeros(3, dtype=np.float32)
        check(capi.lib().ivx_sdf_grid_shape(ptr(sdf_generator.domain), ptr(shape), ptr(centre)))
        self._grid_shape = tuple(int(x) for x in shape)
        self.shifted_grid_center = centre

    def grid_shape(self):
        return self._grid_shape

    def chunk_counts(self):
        return tuple((s + CHUNK_SIZE - 1) // CHUNK_SIZE for s in self._grid_shape)


class VoxelObject:
    """Dense chunk-tiled voxel object living in HBM (`ivx_grid`)."""

    def __init__(self, ctx: Context, chunk_counts, voxel_extent: float, x_chunk_offset: int = 0, global_x_chunks: int = 0):
        self.ctx = ctx
        self.chunk_counts = tuple(int(c) for c in chunk_counts)
        self.voxel_extent = float(voxel_extent)
        self.x_chunk_offset = int(x_chunk_offset)
        cc = np.asarray(self.chunk_counts, dtype=np.uint32)
        h = C.c_void_p()
        check(capi.lib().ivx_grid_create(ctx.h, ptr(cc), voxel_extent, x_chunk_offset, global_x_chunks, C.byref(h)))
        self.h = h
        self.n_chunks = int(np.prod(self.chunk_counts))
        self.n_voxels = self.n_chunks * CHUNK_VOXEL_COUNT
        self.occupied_chunk_ranges = None
        self.occupied_voxel_ranges = None
        self._region_count = None
        _live_grids.add(self)

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None):
                capi.lib().ivx_grid_destroy(self.h)
            self.h = None

    def __del__(self):
        if not sys.is_finalizing():
            try:
                self.close()
            except Exception:
                pass

    # ---- generation ------------------------------------------------------------------------
    @classmethod
    def generate_without_derived_state(cls, ctx: Context, generator: SDFVoxelGenerator, x_chunk_range=None) -> "VoxelObject":
        cc = generator.chunk_counts()
        if min(cc) == 0:
            raise ValueError("empty SDF domain")
        x0, x1 = (0, cc[0]) if x_chunk_range is None else x_chunk_range
        obj = cls(ctx, (x1 - x0, cc[1], cc[2]), generator.voxel_extent, x0, cc[0])
        obj.sample(generator)
        return obj

    def set_voxel_type_generator(self, voxel_type_generator):
        """`ivx_grid_set_voxel_type_noise`: the voxel type generator of every later sample of this object"""
        n, nf, vtf, seed = voxel_type_generator._noise_args()
        check(capi.lib().ivx_grid_set_voxel_type_noise(self.h, n, nf, vtf, seed))

    def sample(self, generator: SDFVoxelGenerator):
        g = generator.sdf_generator
        self.set_voxel_type_generator(generator.voxel_type_generator)
        shape = np.asarray(generator.grid_shape(), dtype=np.uint32)
        check(capi.lib().ivx_sdf_sample(self.h, ptr(g.nodes) if len(g.nodes) else None, len(g.nodes), g.required_forward_stack_size,
                                        ptr(shape), ptr(generator.shifted_grid_center), generator.voxel_type))

    @classmethod
    def generate(cls, ctx: Context, generator: SDFVoxelGenerator) -> "VoxelObject":
        """`VoxelObject::generate` (object.rs:239-244)."""
        obj = cls.generate_without_derived_state(ctx, generator)
        obj.compute_all_derived_state()
        obj.update_occupied_voxel_ranges()
        return obj

    @classmethod
    def from_dense(cls, ctx: Context, chunk_counts, sdf_tiled, type_tiled, voxel_extent=1.0) -> "VoxelObject":
        obj = cls(ctx, chunk_counts, voxel_extent)
        s = np.ascontiguousarray(sdf_tiled, dtype=np.int8).reshape(-1)
        t = np.ascontiguousarray(type_tiled, dtype=np.uint8).reshape(-1)
        check(capi.lib().ivx_grid_upload_dense(obj.h, ptr(s), ptr(t), s.size))
        return obj

    # ---- whole step over resident inputs ----------------------------------------------------
    def set_sdf_program(self, generator: SDFVoxelGenerator):
        g = generator.sdf_generator
        self.set_voxel_type_generator(generator.voxel_type_generator)
        shape = np.asarray(generator.grid_shape(), dtype=np.uint32)
        check(capi.lib().ivx_grid_set_sdf_program(self.h, ptr(g.nodes) if len(g.nodes) else None, len(g.nodes), g.required_forward_stack_size,
                                                  ptr(shape), ptr(generator.shifted_grid_center), generator.voxel_type))

    def set_densities(self, densities):
        d = np.zeros(256, dtype=np.float32)
        src = np.asarray(densities, dtype=np.float32)
        d[: src.size] = src
        check(capi.lib().ivx_grid_set_densities(self.h, ptr(d)))

    def step(self, stages: int = capi.STAGE_ALL) -> np.ndarray:
        """one pass of the voxel hot path (`ivx_voxel_step`) over device-resident inputs"""
        out = np.zeros(1, dtype=capi.STEP_RESULT_DTYPE)
        check(capi.lib().ivx_voxel_step(self.h, stages, ptr(out)))
        if stages & capi.STAGE_REGIONS:
            self._region_count = int(out[0]["region_count"])
        return out[0]

    def set_sample_ahead(self, on: bool):
        """`ivx_grid_set_sample_ahead`: every sample stage also enqueues the next one's pre-pass on the context's second stream"""
        check(capi.lib().ivx_grid_set_sample_ahead(self.h, 1 if on else 0))

    def set_stage_timing(self, slot_mask: int = 0xFFFFFFFF):
        """which timed slots of a step are timed (`ivx_grid_set_stage_timing`): all by default, 0 = none"""
        check(capi.lib().ivx_grid_set_stage_timing(self.h, int(slot_mask) & 0xFFFFFFFF))

    def stage_ticks(self):
        """(`ivx_debug_stage_ticks`) the raw clock stamps of the last collected step, [slot, (start, end)], 0 = not stamped; the clock's rate in kHz"""
        out = np.zeros((capi.N_TIMED_STAGES, 2), dtype=np.uint64)
        khz = np.zeros(1, dtype=np.float64)
        check(capi.lib().ivx_debug_stage_ticks(self.h, ptr(out), ptr(khz)))
        return out, float(khz[0])

    def stage_counters(self):
        out = np.zeros(4, dtype=np.uint32)
        check(capi.lib().ivx_grid_stage_counters(self.h, ptr(out)))
        return {"evaluated_chunks": int(out[0]), "multi_region_chunks": int(out[1]), "meshed_chunks": int(out[2]), "chunks": int(out[3])}

    def step_enqueue(self, stages: int = capi.STAGE_ALL):
        """launch the kernels of `stages` without waiting (`ivx_voxel_step_enqueue`)"""
        if getattr(self, "_fn_enqueue", None) is None:
            self._step_buffers()
        rc = self._fn_enqueue(self.h, stages)
        if rc:
            check(rc)

    def _step_buffers(self):
        # the step pair is called once per frame: keep the foreign functions and the result record instead of looking them up and
        # allocating per call (tens of microseconds of interpreter time the GPU would sit idle for)
        lib = capi.lib()
        self._fn_enqueue, self._fn_collect = lib.ivx_voxel_step_enqueue, lib.ivx_voxel_step_collect
        self._res = np.zeros(1, dtype=capi.STEP_RESULT_DTYPE)
        self._res_ptr = ptr(self._res)

    def step_collect(self) -> np.ndarray:
        """wait once and fetch the results of everything enqueued since the last collect (`ivx_voxel_step_collect`). The record that comes
        back is this object's own buffer: it is overwritten by the next collect."""
        if getattr(self, "_fn_enqueue", None) is None:
            self._step_buffers()
        rc = self._fn_collect(self.h, self._res_ptr)
        if rc:
            check(rc)
        r = self._res[0]
        self._region_count = int(r["region_count"])
        return r

    # ---- derived state ----------------------------------------------------------------------
    def derive_state(self):
        check(capi.lib().ivx_derive_state(self.h))

    def compute_all_derived_state(self):
        """`compute_all_derived_state` (object.rs:1136-1145): adjacencies, local regions, boundary
        adjacencies, global region resolve."""
        self.derive_state()
        self.label_regions()

    def update_occupied_voxel_ranges(self):
        out = np.zeros(12, dtype=np.uint32)
        check(capi.lib().ivx_occupied_ranges(self.h, ptr(out)))
        self.occupied_chunk_ranges = [(int(out[2 * d]), int(out[2 * d + 1])) for d in range(3)]
        self.occupied_voxel_ranges = [(int(out[6 + 2 * d]), int(out[7 + 2 * d])) for d in range(3)]
        return self.occupied_voxel_ranges

    def download(self, sdf=True, types=True, flags=True, labels=True, info=True):
        n = self.n_voxels
        a_sdf = np.empty(n, dtype=np.int8) if sdf else None
        a_typ = np.empty(n, dtype=np.uint8) if types else None
        a_flg = np.empty(n, dtype=np.uint8) if flags else None
        a_lab = np.empty(n, dtype=np.uint8) if labels else None
        a_inf = np.zeros(self.n_chunks, dtype=capi.CHUNK_INFO_DTYPE) if info else None
        check(capi.lib().ivx_grid_download_dense(self.h, ptr(a_sdf), ptr(a_typ), ptr(a_flg), ptr(a_lab), ptr(a_inf), n))
        return a_sdf, a_typ, a_flg, a_lab, a_inf

    # ---- regions ------------------------------------------------------------------------------
    def label_regions(self) -> int:
        n = C.c_uint32(0)
        check(capi.lib().ivx_label_regions(self.h, C.byref(n)))
        self._region_count = int(n.value)
        return self._region_count

    def count_regions(self) -> int:
        """`VoxelObject::count_regions` (split_detection.rs:255-301)."""
        if self._region_count is None:
            self.label_regions()
        return self._region_count

    def is_effectively_empty(self) -> bool:
        """`VoxelObject::is_effectively_empty` (object.rs:803-845): fewer than NON_EMPTY_VOXEL_THRESHOLD = 8 non-empty voxels"""
        if self.count_regions() == 0:
            return True
        return int(self.describe_regions()["voxel_count"].sum()) < 8

    def region_labels(self) -> np.ndarray:
        out = np.empty(self.n_voxels, dtype=np.uint32)
        check(capi.lib().ivx_region_labels_download(self.h, ptr(out), out.size))
        return out

    def describe_regions(self, densities=None) -> np.ndarray:
        d = np.ones(256, dtype=np.float32) if densities is None else np.ascontiguousarray(densities, dtype=np.float32)
        cap = max(1, self.count_regions())
        out = np.zeros(cap, dtype=capi.REGION_DESC_DTYPE)
        n = C.c_size_t(0)
        check(capi.lib().ivx_regions_describe(self.h, ptr(d), ptr(out), cap, C.byref(n)))
        return out[: n.value]

    def find_two_disconnected_regions(self):
        """`find_two_disconnected_regions` (split_detection.rs:193-248): the first two regions in chunk
        scan order, or None."""
        if self.count_regions() < 2:
            return None
        r = self.describe_regions()
        return [(int(r[i]["root_chunk"]), int(r[i]["root_region"])) for i in range(2)]

    def _wrap_child(self, handle):
        obj = VoxelObject.__new__(VoxelObject)
        obj.ctx = self.ctx
        obj.h = handle
        obj.voxel_extent = self.voxel_extent
        obj.x_chunk_offset = 0
        ccs = np.zeros(3, dtype=np.uint32)
        check(capi.lib().ivx_grid_chunk_counts(handle, ptr(ccs)))
        obj.chunk_counts = tuple(int(x) for x in ccs)
        obj.n_chunks = int(np.prod(obj.chunk_counts))
        obj.n_voxels = obj.n_chunks * CHUNK_VOXEL_COUNT
        obj.occupied_chunk_ranges = obj.occupied_voxel_ranges = None
        obj._region_count = None
        _live_grids.add(obj)
        return obj

    def _clip(self, normalized_aabb, normalized_face_planes, copy):
        pl = np.ascontiguousarray(normalized_face_planes, dtype=np.float32).reshape(-1, 4)
        bb = np.ascontiguousarray(normalized_aabb, dtype=np.float32).reshape(6)
        child = C.c_void_p()
        origin = np.zeros(3, dtype=np.uint32)
        outcome = C.c_int(0)
        check(capi.lib().ivx_clip_polyhedron(self.h, ptr(pl), len(pl), ptr(bb), 1 if copy else 0, C.byref(child), ptr(origin), C.byref(outcome)))
        if not copy and outcome.value:
            self._region_count = None
        obj = self._wrap_child(child) if outcome.value == 1 else None
        return int(outcome.value), obj, tuple(int(x) for x in origin)

    def extract_polyhedron(self, normalized_aabb, normalized_face_planes):
        """`VoxelObject::extract_polyhedron` (object/extraction.rs:604-617): planes = n x (unit normal, displacement)"""
        return self._clip(normalized_aabb, normalized_face_planes, False)

    def copy_polyhedron(self, normalized_aabb, normalized_face_planes):
        """`VoxelObject::copy_polyhedron` (object/extraction.rs:1278-1291)"""
        return self._clip(normalized_aabb, normalized_face_planes, True)

    def copy_polyhedra(self, normalized_aabbs, plane_sets):
        """all fragments of one impact in one call (`ivx_copy_polyhedra`; FracturingProcess::execute_in_parallel, fracturing.rs:1047-1189):
        -> list of (outcome, child VoxelObject or None, origin offset) as `copy_polyhedron` returns them one by one"""
        n = len(plane_sets)
        sets = [np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 4) for p in plane_sets]
        planes = np.ascontiguousarray(np.concatenate(sets)) if n else np.zeros((0, 4), dtype=np.float32)
        counts = np.array([len(p) for p in sets], dtype=np.uint32)
        bbs = np.ascontiguousarray(np.asarray(normalized_aabbs, dtype=np.float32).reshape(-1, 6))
        children = (C.c_void_p * max(n, 1))()
        origins = np.zeros((max(n, 1), 3), dtype=np.uint32)
        outcomes = np.zeros(max(n, 1), dtype=np.int32)
        check(capi.lib().ivx_copy_polyhedra(self.h, ptr(planes), ptr(counts), ptr(bbs), n, children, ptr(origins), ptr(outcomes)))
        out = []
        for f in range(n):
            obj = self._wrap_child(C.c_void_p(children[f])) if outcomes[f] == 1 else None
            out.append((int(outcomes[f]), obj, tuple(int(x) for x in origins[f])))
        return out

    def extract_any_disconnected_region(self):
        """`VoxelObject::extract_any_disconnected_region` (object/extraction.rs:78-119). Returns
        (outcome, child VoxelObject or None, origin_offset_in_parent, descriptor of the removed region):
        outcome 0 = nothing to split, 1 = extracted, 2 = removed but too small to become an object."""
        child = C.c_void_p()
        origin = np.zeros(3, dtype=np.uint32)
        outcome = C.c_int(0)
        moved = np.zeros(1, dtype=capi.REGION_DESC_DTYPE)
        check(capi.lib().ivx_split_off_smallest_region(self.h, C.byref(child), ptr(origin), C.byref(outcome), ptr(moved)))
        self._region_count = None if outcome.value else self._region_count
        obj = None
        if outcome.value == 1:
            obj = self._wrap_child(child)
        return int(outcome.value), obj, tuple(int(x) for x in origin), moved[0]

    def extract_all_disconnected_regions(self):
        """the whole loop `while find_two_disconnected_regions { extract_disconnected_region }` (impact_voxel/src/interaction.rs:256) in one
        call (`ivx_split_off_all`): a list of (outcome, child VoxelObject or None, origin_offset_in_parent, descriptor) in the order the loop
        extracts them; the object keeps its last region"""
        n_regions = self.count_regions()
        cap = max(n_regions - 1, 0)
        if cap == 0:
            return []
        kids = (C.c_void_p * cap)()
        origins = np.zeros((cap, 3), dtype=np.uint32)
        outcomes = np.zeros(cap, dtype=np.int32)
        moved = np.zeros(cap, dtype=capi.REGION_DESC_DTYPE)
        n = C.c_size_t(0)
        check(capi.lib().ivx_split_off_all(self.h, cap, kids, ptr(origins), ptr(outcomes), ptr(moved), C.byref(n)))
        self._region_count = None
        out = []
        for k in range(n.value):
            child = self._wrap_child(C.c_void_p(kids[k])) if outcomes[k] == 1 else None
            out.append((int(outcomes[k]), child, tuple(int(x) for x in origins[k]), moved[k]))
        return out

    # ---- halos -----------------------------------------------------------------------------------
    # ---- voxel edit ops ----------------------------------------------------------------------------
    def absorb_sphere(self, center, influence_radius: float, sphere_radius: float, densities=None, want_invalidated: bool = True):
        """`apply_sphere_absorption` (interaction/absorption.rs:801-844) with the sphere in the object's normalized space (voxel
        units, lower grid corner at the origin): every voxel whose centre lies within `influence_radius` of `center` gets
        sd = max(sd, -(|p - c| - sphere_radius)). Returns a dict: removed_moments (10 f64: what the inertial property updater
        subtracts), emptied_by_type (256 counts: the absorbed-voxel tracker), invalidated (bool per chunk: the mesh chunks
        `handle_chunk_voxels_modified` registers), touched_chunks, removed_chunks. Derived state and regions are current
        afterwards; the mesh is not."""
        d = np.ones(256, dtype=np.float32) if densities is None else np.ascontiguousarray(densities, dtype=np.float32)
        c = np.ascontiguousarray(center, dtype=np.float32)
        out = np.zeros(1, dtype=capi.ABSORB_RESULT_DTYPE)
        by_type = np.zeros(256, dtype=np.uint32)
        inval = np.zeros(self.n_chunks, dtype=np.uint8) if want_invalidated else None
        check(capi.lib().ivx_absorb_sphere(self.h, ptr(c), influence_radius, sphere_radius, ptr(d), ptr(out), ptr(by_type),
                                           ptr(inval) if inval is not None else None))
        self._region_count = None
        return {"removed_moments": out[0]["removed_moments"].copy(), "emptied_by_type": by_type, "emptied_voxels": int(out[0]["emptied_voxels"]),
                "invalidated": None if inval is None else inval.astype(bool), "touched_chunks": int(out[0]["touched_chunks"]),
                "removed_chunks": int(out[0]["removed_chunks"])}

    def set_early_mesh_needs(self, on: bool = True):
        """`ivx_grid_set_early_mesh_needs`: the edits of this object deliver what their invalidated meshes need ahead of their other results, so
        that `VoxelObjectMesh.sync_enqueue(None)` can place the re-mesh while an edit is still in flight"""
        check(capi.lib().ivx_grid_set_early_mesh_needs(self.h, 1 if on else 0))

    def absorb_sphere_enqueue(self, center, influence_radius: float, sphere_radius: float, densities=None):
        """`ivx_absorb_sphere_enqueue`: the edit and everything that follows it on the stream, without waiting; `absorb_collect` delivers"""
        d = np.ones(256, dtype=np.float32) if densities is None else np.ascontiguousarray(densities, dtype=np.float32)
        c = np.ascontiguousarray(center, dtype=np.float32)
        check(capi.lib().ivx_absorb_sphere_enqueue(self.h, ptr(c), influence_radius, sphere_radius, ptr(d)))

    def absorb_collect(self, want_invalidated: bool = True):
        """`ivx_absorb_collect`: the one wait of an enqueued edit; the result dict of `absorb_sphere`"""
        out = np.zeros(1, dtype=capi.ABSORB_RESULT_DTYPE)
        by_type = np.zeros(256, dtype=np.uint32)
        inval = np.zeros(self.n_chunks, dtype=np.uint8) if want_invalidated else None
        check(capi.lib().ivx_absorb_collect(self.h, ptr(out), ptr(by_type), ptr(inval) if inval is not None else None))
        self._region_count = None
        return {"removed_moments": out[0]["removed_moments"].copy(), "emptied_by_type": by_type, "emptied_voxels": int(out[0]["emptied_voxels"]),
                "invalidated": None if inval is None else inval.astype(bool), "touched_chunks": int(out[0]["touched_chunks"]),
                "removed_chunks": int(out[0]["removed_chunks"])}

    def absorb_capsule(self, segment_start, segment_vector, influence_radius: float, capsule_radius: float, densities=None,
                       want_invalidated: bool = True):
        """`apply_capsule_absorption` (interaction/absorption.rs:846-889) with the capsule (segment start + vector) in the object's
        normalized space; the result dict of `absorb_sphere`."""
        d = np.ones(256, dtype=np.float32) if densities is None else np.ascontiguousarray(densities, dtype=np.float32)
        a = np.ascontiguousarray(segment_start, dtype=np.float32)
        v = np.ascontiguousarray(segment_vector, dtype=np.float32)
        out = np.zeros(1, dtype=capi.ABSORB_RESULT_DTYPE)
        by_type = np.zeros(256, dtype=np.uint32)
        inval = np.zeros(self.n_chunks, dtype=np.uint8) if want_invalidated else None
        check(capi.lib().ivx_absorb_capsule(self.h, ptr(a), ptr(v), influence_radius, capsule_radius, ptr(d), ptr(out), ptr(by_type),
                                            ptr(inval) if inval is not None else None))
        self._region_count = None
        return {"removed_moments": out[0]["removed_moments"].copy(), "emptied_by_type": by_type, "emptied_voxels": int(out[0]["emptied_voxels"]),
                "invalidated": None if inval is None else inval.astype(bool), "touched_chunks": int(out[0]["touched_chunks"]),
                "removed_chunks": int(out[0]["removed_chunks"])}

    def absorb_mutual(self, rotation_xyzw, translation, other: "VoxelObject", other_rotation_xyzw, other_translation, smoothness: float, densities=None,
                      other_densities=None):
        """`apply_mutual_absorption` (interaction/absorption.rs:891-1079) with self = A, other = B and world -> object transforms;
        returns the result dicts of A and B (as `absorb_sphere`, without the per-type counts)."""
        f = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
        da = np.ones(256, dtype=np.float32) if densities is None else f(densities)
        db = np.ones(256, dtype=np.float32) if other_densities is None else f(other_densities)
        oa, ob = np.zeros(1, dtype=capi.ABSORB_RESULT_DTYPE), np.zeros(1, dtype=capi.ABSORB_RESULT_DTYPE)
        ia, ib = np.zeros(self.n_chunks, dtype=np.uint8), np.zeros(other.n_chunks, dtype=np.uint8)
        check(capi.lib().ivx_absorb_mutual(self.h, ptr(f(rotation_xyzw)), ptr(f(translation)), ptr(da), other.h, ptr(f(other_rotation_xyzw)),
                                           ptr(f(other_translation)), ptr(db), smoothness, ptr(oa), ptr(ob), ptr(ia), ptr(ib)))
        self._region_count = None
        other._region_count = None
        mk = lambda o, inv: {"removed_moments": o[0]["removed_moments"].copy(), "emptied_voxels": int(o[0]["emptied_voxels"]),  # noqa: E731
                             "invalidated": inv.astype(bool), "touched_chunks": int(o[0]["touched_chunks"]), "removed_chunks": int(o[0]["removed_chunks"])}
        return mk(oa, ia), mk(ob, ib)

    # ---- contact generation ------------------------------------------------------------------------
    def sphere_contacts(self, rotation_xyzw, translation, sphere_center, sphere_radius: float, collidable_id_a: int, collidable_id_b: int, body_a: int,
                        body_b: int, response=(0.0, 0.0, 0.0), capacity: int = 65536) -> np.ndarray:
        """`for_each_sphere_voxel_object_contact` (collidable.rs:1098-1127) as a contact list for `PhysicsWorld.prepare_constraints`:
        `rotation_xyzw` + `translation` = transform_to_object_space, the sphere in world space, `response` = combined restitution,
        static and dynamic friction."""
        out = np.zeros(capacity, dtype=capi.CONTACT_DTYPE)
        n = C.c_size_t(0)
        f = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
        check(capi.lib().ivx_sphere_voxel_object_contacts(self.h, ptr(f(rotation_xyzw)), ptr(f(translation)), ptr(f(sphere_center)), sphere_radius,
                                                          collidable_id_a, collidable_id_b, body_a, body_b, ptr(f(response)), ptr(out), capacity, C.byref(n)))
        return out[: n.value]

    def plane_contacts(self, rotation_xyzw, translation, plane_unit_normal, plane_displacement: float, collidable_id_a: int, collidable_id_b: int,
                       body_a: int, body_b: int, response=(0.0, 0.0, 0.0), capacity: int = 65536) -> np.ndarray:
        """`for_each_voxel_object_plane_contact` (collidable.rs:1176-1208): ids in the reference's hash order (plane, voxel object),
        `body_a` = the voxel object's body (the contact normal is the plane's)."""
        out = np.zeros(capacity, dtype=capi.CONTACT_DTYPE)
        n = C.c_size_t(0)
        f = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
        check(capi.lib().ivx_plane_voxel_object_contacts(self.h, ptr(f(rotation_xyzw)), ptr(f(translation)), ptr(f(plane_unit_normal)), plane_displacement,
                                                         collidable_id_a, collidable_id_b, body_a, body_b, ptr(f(response)), ptr(out), capacity, C.byref(n)))
        return out[: n.value]

    def capsule_contacts(self, rotation_xyzw, translation, segment_start, segment_vector, capsule_radius: float, collidable_id_a: int,
                         collidable_id_b: int, body_a: int, body_b: int, response=(0.0, 0.0, 0.0), capacity: int = 65536) -> np.ndarray:
        """`for_each_capsule_voxel_object_contact` (collidable.rs:1257-1286): the capsule in world space, ids and bodies as for
        `sphere_contacts` (collidable first)."""
        out = np.zeros(capacity, dtype=capi.CONTACT_DTYPE)
        n = C.c_size_t(0)
        f = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
        check(capi.lib().ivx_capsule_voxel_object_contacts(self.h, ptr(f(rotation_xyzw)), ptr(f(translation)), ptr(f(segment_start)), ptr(f(segment_vector)),
                                                           capsule_radius, collidable_id_a, collidable_id_b, body_a, body_b, ptr(f(response)), ptr(out),
                                                           capacity, C.byref(n)))
        return out[: n.value]

    def collision_probes_recompute(self) -> int:
        """`VoxelObjectCollisionProbes::recompute_for_all_chunks` (collidable.rs:361-731) on the current mesh; returns the number of probes"""
        n = C.c_size_t(0)
        check(capi.lib().ivx_collision_probes_recompute(self.h, C.byref(n)))
        return int(n.value)

    def collision_probes_sync(self, invalidated) -> int:
        """`VoxelObjectCollisionProbes::sync_with_voxel_object_and_mesh` (collidable.rs:394-433): after `VoxelObjectMesh.sync_with_voxel_object`
        with the same invalidated chunks; returns the length of the point buffer"""
        inv = np.ascontiguousarray(np.asarray(invalidated).reshape(-1), dtype=np.uint8)
        n = C.c_size_t(0)
        check(capi.lib().ivx_collision_probes_sync(self.h, ptr(inv), C.byref(n)))
        return int(n.value)

    def collision_probes(self):
        """-> (points [n,3] f32, entries [m,5] u32: chunk i, j, k, first point, end point)"""
        n, m = C.c_size_t(0), C.c_size_t(0)
        check(capi.lib().ivx_collision_probes_download(self.h, None, 0, None, 0, C.byref(n), C.byref(m)))
        pts = np.zeros((max(1, n.value), 3), dtype=np.float32)
        ent = np.zeros((max(1, m.value), 5), dtype=np.uint32)
        check(capi.lib().ivx_collision_probes_download(self.h, ptr(pts), n.value, ptr(ent), m.value, C.byref(n), C.byref(m)))
        return pts[: n.value], ent[: m.value]

    def mutual_contacts(self, rotation_xyzw, translation, center_of_mass, other: "VoxelObject", other_rotation_xyzw, other_translation,
                        other_center_of_mass, collidable_id_a: int, collidable_id_b: int, body_a: int, body_b: int, response=(0.0, 0.0, 0.0),
                        capacity: int = 65536) -> np.ndarray:
        """`for_each_mutual_voxel_object_contact` (collidable.rs:859-1049) with self = A, other = B: world -> object transforms, each
        object's centre of mass (object space); the contact list for `PhysicsWorld.prepare_constraints`."""
        out = np.zeros(capacity, dtype=capi.CONTACT_DTYPE)
        n = C.c_size_t(0)
        f = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
        check(capi.lib().ivx_mutual_voxel_object_contacts(self.h, ptr(f(rotation_xyzw)), ptr(f(translation)), ptr(f(center_of_mass)), other.h,
                                                          ptr(f(other_rotation_xyzw)), ptr(f(other_translation)), ptr(f(other_center_of_mass)),
                                                          collidable_id_a, collidable_id_b, body_a, body_b, ptr(f(response)), ptr(out), capacity,
                                                          C.byref(n)))
        return out[: n.value]

    def halo_bytes(self) -> int:
        return int(capi.lib().ivx_halo_bytes(self.h))

    def halo_pack(self, side: int, device_ptr: int):
        check(capi.lib().ivx_halo_pack(self.h, side, C.c_void_p(device_ptr)))

    def halo_unpack(self, side: int, device_ptr: int):
        check(capi.lib().ivx_halo_unpack(self.h, side, C.c_void_p(device_ptr)))

    def halo_pack_enqueue(self, side: int, device_ptr: int):
        check(capi.lib().ivx_halo_pack_enqueue(self.h, side, C.c_void_p(device_ptr)))

    def halo_unpack_enqueue(self, side: int, device_ptr: int):
        check(capi.lib().ivx_halo_unpack_enqueue(self.h, side, C.c_void_p(device_ptr)))

    def halo_clear(self, side: int):
        check(capi.lib().ivx_halo_clear(self.h, side))


class VoxelObjectMesh:
    """`VoxelObjectMesh` (mesh.rs:44-58): buffers stay in HBM; accessors download on demand."""

    def __init__(self, voxel_object: VoxelObject):
        self.object = voxel_object
        self.counts = None

    @classmethod
    def create(cls, voxel_object: VoxelObject) -> "VoxelObjectMesh":
        m = cls(voxel_object)
        m.recreate()
        return m

    def recreate(self):
        c = np.zeros((), dtype=capi.MESH_COUNTS_DTYPE)
        check(capi.lib().ivx_remesh(self.object.h, ptr(c.reshape(1))))
        self.counts = c
        return self

    def sync_with_voxel_object(self, invalidated):
        """`VoxelObjectMesh::sync_with_voxel_object` (mesh.rs:355-456): re-mesh the invalidated chunks (bool / byte per chunk, as
        returned by the edit ops) in place, reusing freed buffer ranges"""
        inv = np.ascontiguousarray(np.asarray(invalidated).reshape(-1), dtype=np.uint8)
        assert inv.size == self.object.n_chunks
        c = np.zeros((), dtype=capi.MESH_COUNTS_DTYPE)
        check(capi.lib().ivx_mesh_sync(self.object.h, ptr(inv), ptr(c.reshape(1))))
        self.counts = c
        return self

    def sync_enqueue(self, invalidated=None):
        """`ivx_mesh_sync_enqueue`: place and launch the re-mesh of the invalidated chunks without waiting. `None`: the chunks of the edit that
        is in flight (`absorb_*_enqueue` without its `absorb_collect` yet) — the call waits for the edit's mesh needs, which arrive a third of
        the way down the edit's chain, places the meshes while the region stages still run and puts its launches behind them"""
        if invalidated is None:
            check(capi.lib().ivx_mesh_sync_enqueue(self.object.h, None))
            return
        inv = np.ascontiguousarray(np.asarray(invalidated).reshape(-1), dtype=np.uint8)
        assert inv.size == self.object.n_chunks
        check(capi.lib().ivx_mesh_sync_enqueue(self.object.h, ptr(inv)))

    def sync_collect(self):
        """`ivx_mesh_sync_collect`: the wait of an enqueued sync"""
        c = np.zeros((), dtype=capi.MESH_COUNTS_DTYPE)
        check(capi.lib().ivx_mesh_sync_collect(self.object.h, ptr(c.reshape(1))))
        self.counts = c
        return self

    MESH_BUFFERS = ("positions", "normals", "indices", "index_materials", "submeshes")

    def export(self, which):
        """`ivx_mesh_export`: handles of one mesh buffer (name or number, see MESH_BUFFERS) for another process / API — dict with `ipc_handle`
        (64 bytes, hipIpcOpenMemHandle), `dmabuf_fd` (-1 if the runtime makes none; the caller closes it), `bytes`, `capacity_bytes`,
        `element_bytes`, `generation`, `dmabuf_offset` / `dmabuf_bytes` (where the buffer lies inside the dma-buf object, how much the
        descriptor covers)"""
        w = self.MESH_BUFFERS.index(which) if isinstance(which, str) else int(which)
        e = np.zeros((), dtype=capi.MESH_EXPORT_DTYPE)
        check(capi.lib().ivx_mesh_export(self.object.h, w, ptr(e.reshape(1))))
        return {"ipc_handle": bytes(e["ipc_handle"].tobytes()), "dmabuf_fd": int(e["dmabuf_fd"]), "bytes": int(e["bytes"]), "capacity_bytes": int(e["capacity_bytes"]),
                "element_bytes": int(e["element_bytes"]), "generation": int(e["generation"]), "device_ptr": int(e["device_ptr"]),
                "dmabuf_offset": int(e["dmabuf_offset"]), "dmabuf_bytes": int(e["dmabuf_bytes"])}

    def generation(self) -> int:
        g = C.c_uint64()
        check(capi.lib().ivx_mesh_generation(self.object.h, C.byref(g)))
        return int(g.value)

    def mesh_modifications(self):
        """`VoxelMeshModifications` (mesh.rs:113-123): (ranges [n,4] u32: vertex start, end, index start, end of every chunk written
        since the last report, chunks_were_removed)"""
        n = C.c_size_t(0)
        removed = C.c_int(0)
        check(capi.lib().ivx_mesh_modifications(self.object.h, None, 0, C.byref(n), C.byref(removed)))
        out = np.zeros((max(1, n.value), 4), dtype=np.uint32)
        check(capi.lib().ivx_mesh_modifications(self.object.h, ptr(out), n.value, C.byref(n), C.byref(removed)))
        return out[: n.value], bool(removed.value)

    def report_gpu_resources_synchronized(self):
        check(capi.lib().ivx_mesh_report_synchronized(self.object.h))

    def n_vertices(self):
        return int(self.counts["n_vertices"])

    def n_indices(self):
        return int(self.counts["n_indices"])

    def n_chunks(self):
        return int(self.counts["n_submeshes"])

    def download(self):
        nv, ni, ns = self.n_vertices(), self.n_indices(), self.n_chunks()
        pos = np.empty((nv, 3), dtype=np.float32)
        nrm = np.empty((nv, 3), dtype=np.float32)
        idx = np.empty(ni, dtype=np.uint32)
        im = np.empty((ni, 8), dtype=np.uint8)
        sub = np.zeros(ns, dtype=capi.SUBMESH_DTYPE)
        check(capi.lib().ivx_mesh_download(self.object.h, ptr(pos), ptr(nrm), ptr(idx), ptr(im), ptr(sub)))
        return pos, nrm, idx, im, sub


class VoxelObjectInertialPropertyManager:
    """`VoxelObjectInertialPropertyManager` (object/inertia.rs:20-25)."""

    def __init__(self, moments64: np.ndarray):
        self.m64 = np.asarray(moments64, dtype=np.float64)
        m = self.m64.astype(np.float32)
        self.mass = float(m[0])
        self.moments = m[1:4]
        self.moments_of_inertia = m[4:7]
        self.products_of_inertia = m[7:10]

    @classmethod
    def initialized_from(cls, voxel_object: VoxelObject, voxel_type_densities) -> "VoxelObjectInertialPropertyManager":
        d = np.zeros(256, dtype=np.float32)
        src = np.asarray(voxel_type_densities, dtype=np.float32)
        d[: src.size] = src
        out = np.zeros((), dtype=capi.MOMENTS_DTYPE)
        check(capi.lib().ivx_inertia(voxel_object.h, ptr(d), ptr(out.reshape(1))))
        return cls(out["m64"].copy())

    def derive_center_of_mass(self):
        return self.m64[1:4] / self.m64[0]

    def derive_inertial_properties(self):
        """mass, centre of mass, inertia tensor about the centre of mass and its inverse
        (object/inertia.rs:288-326); evaluated in f64 on the host — O(1) work per object."""
        m = self.m64
        mass = m[0]
        com = m[1:4] / mass
        J = np.array([[m[4], -m[7], -m[9]], [-m[7], m[5], -m[8]], [-m[9], -m[8], m[6]]])
        sq = com * com
        delta = -mass * np.array(
            [[sq[1] + sq[2], -com[0] * com[1], -com[2] * com[0]], [-com[0] * com[1], sq[2] + sq[0], -com[1] * com[2]],
             [-com[2] * com[0], -com[1] * com[2], sq[0] + sq[1]]]
        )
        Jc = J + delta
        return {"mass": mass, "com": com, "inertia": Jc, "inverse": np.linalg.inv(Jc / mass) / mass}
