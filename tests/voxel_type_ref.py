"""numpy restatement of the gradient-noise voxel type generator (GradientNoiseVoxelTypeGenerator, generation/voxel_type.rs:97-169, as
SDFVoxelGenerator::generate_chunk applies it, generation.rs:293-371) over the library's own noise (noise_ref.simplex4), in the f32
operation order of impact_amd/csrc/noise.hpp (type_coord, type_argmax4)."""
from __future__ import annotations

import numpy as np

import noise_block_ref as nb
import noise_ref as nr
from impact_amd.voxel import SDFVoxelGenerator

f32 = np.float32
IDX = np.arange(16, dtype=f32)


def chunk_types(origin, n, nf, vtf, seed):
    """the 4096 types [i, j, k] of the chunk whose root-space origin is given: the first t < n whose noise value is greatest"""
    o = np.asarray(origin, dtype=f32)
    nf, vtf = f32(nf), f32(vtf)
    w = ((o[0] + IDX) * nf)[:, None, None]  # dimensions reversed, as the reference hands them to its noise builder
    z = ((o[1] + IDX) * nf)[None, :, None]
    y = ((o[2] + IDX) * nf)[None, None, :]
    w, z, y = (np.ascontiguousarray(np.broadcast_to(a, (16, 16, 16))) for a in (w, z, y))
    best = nr.simplex4(np.full((16, 16, 16), f32(0) * vtf, f32), y, z, w, seed)
    typ = np.zeros((16, 16, 16), np.uint8)
    for t in range(1, n):
        v = nr.simplex4(np.full((16, 16, 16), f32(t) * vtf, f32), y, z, w, seed)
        with np.errstate(invalid="ignore"):
            m = v > best  # strict: the first maximum stays, a NaN never wins
        best = np.where(m, v, best)
        typ[m] = t
    return typ


def restated_planes_with_noise_types(graph, n, nf, vtf, seed):
    """noise_block_ref.restated_planes with the types of every chunk that has a non-empty voxel drawn from the noise (all 4096 of them,
    the empty voxels and those beyond the generator's grid included); every other chunk keeps the dummy type"""
    cc, sdf, typ = nb.restated_planes(graph, 0)
    center = np.asarray(SDFVoxelGenerator(1.0, graph).shifted_grid_center, f32)
    sdf_c, typ_c = sdf.reshape(-1, 4096), typ.reshape(-1, 4096).copy()
    for ci in range(cc[0]):
        for cj in range(cc[1]):
            for ck in range(cc[2]):
                c = (ci * cc[1] + cj) * cc[2] + ck
                if np.any(sdf_c[c] < 0):
                    o = (np.array([ci * 16, cj * 16, ck * 16], f32) - center).astype(f32)
                    typ_c[c] = chunk_types(o, n, nf, vtf, seed).reshape(-1)
    return cc, sdf, typ_c.reshape(-1)
