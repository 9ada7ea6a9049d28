"""Several voxel types on ANY scene, for the parity tests of everything downstream of the sampler: the sdf and type planes of the oracle's
own generator with the types of every chunk that holds a voxel with sdf < 0 replaced by the numpy restatement of the gradient-noise type
generator (voxel_type_ref.chunk_types; the rule of voxel_type_ref.restated_planes_with_noise_types without restating the SDF evaluation, so
every node kind and voxel extent works), and the conditions a typed case asserts on its oracle object before it touches the device — a
typed case that happens to put one type where a kernel looks proves nothing. No code of the library under test is in the oracle's path
but the host-side grid centre of SDFVoxelGenerator."""
from __future__ import annotations

import numpy as np

import oracle_lib as ol
import voxel_type_ref as vr

f32 = np.float32
DENSITIES = (1.0 + np.arange(256)).astype(f32)  # densities[t] = 1 + t: a stage that takes one type for all voxels shows in the moments
SPHERE60_NOISE = (4, 0.01, 1.0, 0)  # (n types, noise frequency, voxel type frequency, seed) of test_gpu_voxel_types' sphere


def sphere60():
    from impact_amd import scenes

    return scenes.sphere_scene(60.0)


_planes = {}


def typed_planes(graph, extent, noise):
    """-> (chunk counts, sdf tiled, type tiled)"""
    from impact_amd.voxel import SDFVoxelGenerator

    key = (graph.nodes().tobytes(), int(graph.root_node_id), float(extent), tuple(noise))
    if key in _planes:  # (the same scene under several drivers: the overlay is some ms per typed chunk)
        return _planes[key]
    n, nf, vtf, seed = noise
    o = ol.OracleObject.from_sdf(graph, extent, 0)
    cc = o.chunk_counts
    sdf, typ = o.export_dense()[:2]
    center = np.asarray(SDFVoxelGenerator(extent, graph).shifted_grid_center, f32)
    sdf_c, typ_c = sdf.reshape(-1, 4096), typ.reshape(-1, 4096).copy()
    for c in np.flatnonzero((sdf_c < 0).any(axis=1)):
        ci, cj, ck = c // (cc[1] * cc[2]), (c // cc[2]) % cc[1], c % cc[2]
        origin = (np.array([ci * 16, cj * 16, ck * 16], f32) - center).astype(f32)
        typ_c[c] = vr.chunk_types(origin, n, nf, vtf, seed).reshape(-1)
    sdf.setflags(write=False)
    typ = typ_c.reshape(-1)
    typ.setflags(write=False)
    _planes[key] = (cc, sdf, typ)
    return _planes[key]


def typed_oracle(graph, extent, noise, derived=True):
    cc, sdf, typ = typed_planes(graph, extent, noise)
    o = ol.OracleObject.from_dense(cc, sdf, typ, extent)
    if derived:
        o.update_occupied_voxel_ranges()
        o.compute_all_derived_state()
    return o


def noise_generator(noise):
    from impact_amd.voxel import GradientNoiseVoxelTypeGenerator

    return GradientNoiseVoxelTypeGenerator(*noise)


def typed_gpu(ctx, graph, extent, noise, derived=True):
    """the same scene sampled on the device with the noise type generator; `derived`: as parity tests' `both` leaves an object"""
    from impact_amd.voxel import SDFVoxelGenerator, VoxelObject

    g = VoxelObject.generate_without_derived_state(ctx, SDFVoxelGenerator(extent, graph, noise_generator(noise)))
    if derived:
        g.compute_all_derived_state()
        g.update_occupied_voxel_ranges()
        g.label_regions()
    return g


# ---- what a typed case must contain to show anything (asserted on the oracle object, derived state computed) ----------------------------
def types_of_non_empty(o_typ, o_flg):
    """the distinct types among non-empty voxels of (a slice of) exported planes"""
    return np.unique(o_typ[(o_flg & 1) == 0])


def cut_face_types(o: ol.OracleObject, cut):
    """the distinct types among the non-empty voxels of the two one-voxel x-planes that meet at chunk plane `cut`: (below, above)"""
    _, typ, flg, _, _ = o.export_dense()
    cc = o.chunk_counts
    typ, flg = ol.tiled_to_dense(typ, cc), ol.tiled_to_dense(flg, cc)
    x = 16 * cut
    return types_of_non_empty(typ[x - 1], flg[x - 1]), types_of_non_empty(typ[x], flg[x])


def uniform_typed_chunks_on_face_layers(o: ol.OracleObject, cut):
    """how many Uniform chunks of a non-zero type lie in the two chunk planes that meet at `cut`"""
    info = o.export_dense()[4]
    cc = o.chunk_counts
    info = info.reshape(cc)
    layers = info[cut - 1:cut + 1]
    return int(((layers["kind"] == 1) & (layers["uniform_type"] != 0)).sum())


def mixed_material_submeshes(om: ol.OracleMesh, chunk_filter=None):
    """how many submeshes (of the chunks `chunk_filter(i, j, k)` accepts) have an index range with >= 2 distinct 8-byte index-material
    rows: their quads do not all have the same materials"""
    n = 0
    for sm in om.submeshes:
        if chunk_filter is not None and not chunk_filter(int(sm[0]), int(sm[1]), int(sm[2])):
            continue
        rows = om.index_materials[int(sm[3]):int(sm[3]) + int(sm[4])]
        if len(rows) and len(np.unique(np.ascontiguousarray(rows).view(np.uint64))) >= 2:
            n += 1
    return n


def assert_slab_case_shows_types(o: ol.OracleObject, world, need_uniform):
    """the conditions of a typed slab case: at every cut both face planes hold >= 2 types among non-empty voxels and the two chunk planes
    beside it hold >= 1 submesh of mixed materials; over the cuts, >= 1 Uniform chunk of a non-zero type on a face layer (`need_uniform`:
    the scenes that have such chunks at all)"""
    from impact_amd.distributed import slab_ranges

    om = o.mesh()
    uniform = 0
    cuts = [x1 for _, x1 in slab_ranges(o.chunk_counts[0], world)[:-1]]
    for cut in cuts:
        lo, hi = cut_face_types(o, cut)
        assert len(lo) >= 2 and len(hi) >= 2, (cut, lo, hi)
        mixed = mixed_material_submeshes(om, lambda i, j, k: cut - 1 <= i <= cut)
        assert mixed >= 1, cut
        uniform += uniform_typed_chunks_on_face_layers(o, cut)
    if need_uniform:
        assert uniform >= 1, cuts
    return cuts, uniform


def edit_census(o: ol.OracleObject, edits, dens=None):
    """the oracle alone through a sequence of edits — ("s", centre, radius) or ("c", segment start, segment vector, radius), influence radius
    + 2 — with a mesh synced after each: the types that lost voxels over the sequence, how many Uniform chunks of a non-zero type were
    converted, and per edit how many submeshes of mixed materials the sync re-meshed. `o` is consumed (use a fresh typed_oracle)."""
    om = ol.OracleMeshHandle(o)
    cc = o.chunk_counts
    emptied, converted, mixed = set(), 0, []
    for e in edits:
        before = o.export_dense()[4].copy()
        if e[0] == "s":
            ro = o.absorb_sphere(e[1], float(e[2]) + 2.0, float(e[2]), dens)
        else:
            ro = o.absorb_capsule(e[1], e[2], float(e[3]) + 2.0, float(e[3]), dens)
        after = o.export_dense()[4]
        emptied |= set(np.flatnonzero(ro["emptied_by_type"]).tolist())
        converted += int(((before["kind"] == 1) & (before["uniform_type"] != 0) & (after["kind"] != 1)).sum())
        om.sync(ro["invalidated"])
        inv = ro["invalidated"].reshape(cc)
        mixed.append(mixed_material_submeshes(om.get(), lambda i, j, k: bool(inv[i, j, k])))
    return {"emptied_types": emptied, "converted_typed_uniform": converted, "mixed_remeshed": mixed}
