"""Gradient-noise voxel types on the host: the per-voxel function of impact_amd/csrc/noise.hpp (type_argmax4, through the developer export
ivx_voxel_types_eval with a null context) against its numpy restatement (tests/voxel_type_ref.py) byte for byte, the argument checks that
need no device, and the Python mirror's generator types."""
import itertools

import numpy as np
import pytest

import voxel_type_ref as vr
from impact_amd import capi
from impact_amd.sdf_graph import SDFGraph, SDFNode
from impact_amd.voxel import GradientNoiseVoxelTypeGenerator, SameVoxelTypeGenerator, SDFVoxelGenerator

f32 = np.float32

ORIGINS = [(-40.5, -40.5, -40.5), (-8.0, 24.0, -56.0), (1e4, -1e4, 1e4), (-1e4, 16.0, -1e4 + 0.25)]
FREQUENCIES = [(0.01, 1.0), (0.02, 0.37), (0.11, 2.5)]  # (noise_frequency, voxel_type_frequency)
SEEDS = [0, 0xFFFFFFFF, 12345]


def eval_cases():
    """(n, origin, noise_frequency, voxel_type_frequency, seed): every combination for the small type counts, four for 255 types"""
    cases = [(n, o, nf, vtf, s) for n in (1, 2, 4, 7) for o, (nf, vtf), s in itertools.product(ORIGINS, FREQUENCIES, SEEDS)]
    cases += [(255, ORIGINS[q], *FREQUENCIES[q % 3], SEEDS[q % 3]) for q in range(4)]
    return cases


def types_eval(ctx_handle, n, origin, nf, vtf, seed, expect=capi.IVX_OK):
    o = np.asarray(origin, dtype=f32)
    out = np.full(4096, 0xEE, np.uint8)
    rc = capi.lib().ivx_voxel_types_eval(ctx_handle, n, nf, vtf, seed, o.ctypes.data, out.ctypes.data)
    assert rc == expect, capi.lib().ivx_last_error()
    return out.reshape(16, 16, 16)


def test_host_types_equal_restatement():
    seen = set()
    for n, o, nf, vtf, seed in eval_cases():
        got = types_eval(None, n, o, nf, vtf, seed)
        want = vr.chunk_types(o, n, nf, vtf, seed)
        np.testing.assert_array_equal(got, want, err_msg=str((n, o, nf, vtf, seed)))
        assert got.max() < n
        seen.update(np.unique(got).tolist())
    assert len(seen) > 100  # (the 255-type cases spread over the types)


def test_one_type_is_all_zeros():
    for o in ORIGINS:
        assert not types_eval(None, 1, o, 0.05, 1.0, 7).any()


def test_tie_keeps_the_first_index():
    # voxel_type_frequency = 0: every candidate type has the same noise value
    for n in (2, 7, 255):
        assert not types_eval(None, n, ORIGINS[0], 0.05, 0.0, 3).any()
        assert not vr.chunk_types(ORIGINS[0], n, 0.05, 0.0, 3).any()


def test_types_vary_within_and_between_chunks():
    a = types_eval(None, 4, (-8.0, -8.0, -8.0), 0.05, 1.0, 0)
    b = types_eval(None, 4, (8.0, -8.0, -8.0), 0.05, 1.0, 0)
    assert len(np.unique(a)) > 1 and not np.array_equal(a, b)
    # neighbouring chunks continue each other: row i = 15 of a lies one voxel from row i = 0 of b, and the same point has the same type
    c = types_eval(None, 4, (-7.0, -8.0, -8.0), 0.05, 1.0, 0)
    np.testing.assert_array_equal(c[:15], a[1:])
    np.testing.assert_array_equal(c[15], b[0])


def test_argument_checks_without_device():
    L = capi.lib()
    o = np.zeros(3, f32)
    out = np.zeros(4096, np.uint8)
    for n, nf, vtf in ((0, 0.1, 1.0), (256, 0.1, 1.0), (4, float("nan"), 1.0), (4, 0.1, float("inf"))):
        assert L.ivx_voxel_types_eval(None, n, nf, vtf, 0, o.ctypes.data, out.ctypes.data) == capi.IVX_ERR_INVALID
    assert L.ivx_voxel_types_eval(None, 4, 0.1, 1.0, 0, None, out.ctypes.data) == capi.IVX_ERR_INVALID
    assert L.ivx_voxel_types_eval(None, 4, 0.1, 1.0, 0, o.ctypes.data, None) == capi.IVX_ERR_INVALID
    assert L.ivx_grid_set_voxel_type_noise(None, 4, 0.1, 1.0, 0) == capi.IVX_ERR_INVALID
    assert not out.any()


def test_python_generator_types():
    g = SDFGraph()
    g.set_root_node(g.add_node(SDFNode.new_box([10.0, 10.0, 10.0])))
    gen = SDFVoxelGenerator(1.0, g, 3)  # an int still means SameVoxelTypeGenerator(3)
    assert isinstance(gen.voxel_type_generator, SameVoxelTypeGenerator) and gen.voxel_type == 3
    assert gen.voxel_type_generator._noise_args()[0] == 0
    assert SDFVoxelGenerator(1.0, g).voxel_type == 0
    assert SDFVoxelGenerator(1.0, g, SameVoxelTypeGenerator(9)).voxel_type == 9
    noise = GradientNoiseVoxelTypeGenerator(4, 0.02, 1.0, -1)
    gen = SDFVoxelGenerator(1.0, g, noise)
    assert gen.voxel_type_generator is noise and noise._noise_args() == (4, 0.02, 1.0, 0xFFFFFFFF)


def test_restated_planes_type_every_voxel_of_a_non_empty_chunk():
    g = SDFGraph()
    g.set_root_node(g.add_node(SDFNode.new_sphere(12.0)))
    cc, sdf, typ = vr.restated_planes_with_noise_types(g, 3, 0.1, 0.6, 5)
    sdf_c, typ_c = sdf.reshape(-1, 4096), typ.reshape(-1, 4096)
    has = (sdf_c < 0).any(axis=1)
    assert has.any() and (typ_c[has] < 3).all() and (typ_c[~has] == 255).all()
    assert (sdf_c[has] >= 0).any()  # (empty voxels of those chunks are typed as well)
    assert len(np.unique(typ_c[has])) == 3
