"""Gradient-noise voxel types (GradientNoiseVoxelTypeGenerator, generation/voxel_type.rs:97-169) on the device: the device build of the
per-voxel function against its numpy restatement, one noise type through the whole sampler against the oracle's own generator, and
multi-type objects against the restated planes (tests/voxel_type_ref.py) followed by the oracle's classification, derived state, mesh,
regions and inertia of those planes — with a density per type, so that a stage that took one type for all voxels shows."""
import numpy as np
import pytest

import oracle_lib as ol
import parity_util as pu
import voxel_type_ref as vr
from impact_amd import capi
from impact_amd.sdf_graph import SDFGraph, SDFNode
from impact_amd.voxel import GradientNoiseVoxelTypeGenerator, SDFVoxelGenerator, VoxelObject
from test_gpu_random_sdf import random_tree
from test_voxel_types_cpu import eval_cases, types_eval

pytestmark = pytest.mark.gpu
f32 = np.float32
DENSITIES = (1.0 + np.arange(256)).astype(f32)  # densities[t] = 1 + t


def test_device_types_equal_restatement(ctx):
    for n, o, nf, vtf, seed in eval_cases():
        got = types_eval(ctx.h, n, o, nf, vtf, seed)
        np.testing.assert_array_equal(got, vr.chunk_types(o, n, nf, vtf, seed), err_msg=str((n, o, nf, vtf, seed)))


@pytest.mark.parametrize("seed", [41, 42, 43, 44, 45, 46])
def test_one_noise_type_equals_the_oracle_generator(ctx, seed):
    """n = 1: every typed voxel is 0, which is what the oracle's own generator gives with voxel type 0 — no restatement in between"""
    rng = np.random.default_rng(seed)
    while True:  # (a tree whose root domain is degenerate has no grid to compare: draw again)
        graph = SDFGraph()
        random_tree(graph, rng, int(rng.integers(1, 4)))
        o = pu.oracle_from_graph(graph)
        if min(o.chunk_counts) > 0:
            break
    gen = SDFVoxelGenerator(1.0, graph, GradientNoiseVoxelTypeGenerator(1, 0.03, 0.7, seed))
    g = VoxelObject.generate_without_derived_state(ctx, gen)
    pu.assert_generated_equal(o, g)
    o.update_occupied_voxel_ranges()
    o.compute_all_derived_state()
    g.compute_all_derived_state()
    pu.assert_derived_equal(o, g)
    pu.assert_mesh_equal(o, g)
    pu.assert_regions_equal(o, g)
    g.close()


def box(half_extent):
    g = SDFGraph()
    g.set_root_node(g.add_node(SDFNode.new_box([2.0 * half_extent] * 3)))  # (new_box takes the extents)
    return g


def noisy_sphere():
    g = SDFGraph()
    s = g.add_node(SDFNode.new_sphere(30.0))
    g.set_root_node(g.add_node(SDFNode.new_multifractal_noise(s, 3, 0.05, 2.0, 0.6, 2.0, 11)))
    return g


def rotated_capsule():
    g = SDFGraph()
    c = g.add_node(SDFNode.new_capsule(30.0, 9.0))
    g.set_root_node(g.add_node(SDFNode.new_rotation_from_axis_angle(c, [0.3, 0.8, 0.5], 0.9)))
    return g


def _generated(ctx, graph, n, nf, vtf, seed):
    """the device object, the oracle object of the restated planes, and those planes' chunk view"""
    cc, sdf, typ = vr.restated_planes_with_noise_types(graph, n, nf, vtf, seed)
    gen = SDFVoxelGenerator(1.0, graph, GradientNoiseVoxelTypeGenerator(n, nf, vtf, seed))
    g = VoxelObject.generate_without_derived_state(ctx, gen)
    o = ol.OracleObject.from_dense(cc, sdf, typ)
    pu.assert_generated_equal(o, g)
    o_info, g_info = o.export_dense()[4], g.download(flags=False, labels=False)[4]
    uni = o_info["gen_kind"] == 1
    np.testing.assert_array_equal(g_info["uniform_type"][uni], o_info["uniform_type"][uni])
    return g, o, sdf.reshape(-1, 4096), typ.reshape(-1, 4096), o_info


def _check_against_restatement(ctx, graph, n, nf, vtf, seed):
    g, o, sdf_c, typ_c, o_info = _generated(ctx, graph, n, nf, vtf, seed)
    o.update_occupied_voxel_ranges()
    o.compute_all_derived_state()
    g.compute_all_derived_state()
    pu.assert_derived_equal(o, g)
    pu.assert_mesh_equal(o, g)
    pu.assert_regions_equal(o, g)
    pu.assert_inertia_equal(o, g, DENSITIES)
    g.close()
    return sdf_c, typ_c, o_info


def _census(sdf_c, typ_c, o_info):
    """fully inside chunks (every voxel -128): how many stay Uniform, how many the types demote; the type histogram"""
    inside = (sdf_c == -128).all(axis=1)
    stay = int((inside & (o_info["gen_kind"] == 1)).sum())
    demoted = int((inside & (o_info["gen_kind"] == 2)).sum())
    hist = np.bincount(typ_c.reshape(-1), minlength=256)
    print("fully inside", int(inside.sum()), "uniform", stay, "demoted", demoted, "types", hist[:4].tolist(), "dummy", int(hist[255]))
    return stay, demoted, hist


def test_box_with_four_types(ctx):
    """Box of half-extent 40, 4 types, 0.01, 1.0, seed 0. Every chunk of this object is NonUniform: the 27 chunks deep inside the box
    are the block constant -margin (atomic.rs:654-668), which quantises to -127, not -128. In 8 of them the 4096 types are equal, in 19
    mixed — planes either way. The Uniform branch of the type pass is the sphere's below."""
    sdf_c, typ_c, o_info = _check_against_restatement(ctx, box(40.0), 4, 0.01, 1.0, 0)
    stay, demoted, hist = _census(sdf_c, typ_c, o_info)
    assert hist[:4].tolist() == [279287, 236072, 189185, 180192]
    const = (sdf_c == sdf_c[:, :1]).all(axis=1)
    one_type = (typ_c == typ_c[:, :1]).all(axis=1)
    assert (int(const.sum()), int((const & one_type).sum()), int((const & ~one_type).sum())) == (27, 8, 19)
    assert (o_info["gen_kind"] == 2).all() and (stay, demoted) == (0, 0)


def test_sphere_with_four_types(ctx):
    """Sphere of radius 60, 4 types, 0.01, 1.0, seed 0: 72 chunks are maximally inside throughout (the pre-pass settles them as Uniform);
    22 of them have one type — each of the four types among them — and stay Uniform, the types demote the other 50."""
    sdf_c, typ_c, o_info = _check_against_restatement(ctx, sphere60(), 4, 0.01, 1.0, 0)
    stay, demoted, hist = _census(sdf_c, typ_c, o_info)
    # what the case must contain to show anything
    assert stay >= 1 and demoted >= 1
    assert (hist[:4] > 0).all()
    assert len(np.unique(o_info["uniform_type"][o_info["gen_kind"] == 1])) >= 2
    assert (stay, demoted) == (22, 50)


@pytest.mark.parametrize("make, params", [(noisy_sphere, (3, 0.02, 0.37, 9)), (rotated_capsule, (5, 0.04, 0.8, 0xFFFFFFFF))])
def test_noise_types_on_other_bodies(ctx, make, params):
    _, typ_c, _ = _check_against_restatement(ctx, make(), *params)
    hist = np.bincount(typ_c.reshape(-1), minlength=256)
    assert (hist[: params[0]] > 0).sum() >= 2


@pytest.mark.parametrize("half_extent, n_chunks", [(80.0, 1331), (40.0, 216)])
def test_reference_benchmark_planes(ctx, half_extent, n_chunks):
    """the type generator of generate_box_with_gradient_noise_voxel_types (benchmarks/generation.rs:105-129): 4 types, 0.02, 1.0, seed 0,
    generated planes and records only — over a box of half-extent 80 (1331 chunks), and over the benchmark's own box, whose 80 are its
    extents (216 chunks)"""
    g, o, sdf_c, typ_c, o_info = _generated(ctx, box(half_extent), 4, 0.02, 1.0, 0)
    assert g.n_chunks == n_chunks
    assert (np.bincount(typ_c.reshape(-1), minlength=256)[:4] > 0).all()
    g.close()


def sphere60():
    g = SDFGraph()
    g.set_root_node(g.add_node(SDFNode.new_sphere(60.0)))
    return g


def test_resident_program_with_noise_types(ctx):
    """the sphere of test_sphere_with_four_types under the resident-program step with sample-ahead on: the records the ahead pre-pass
    parks for its Uniform chunks are corrected (or demoted) by the type pass every step"""
    graph = sphere60()
    noise = GradientNoiseVoxelTypeGenerator(4, 0.01, 1.0, 0)
    cc, r_sdf, r_typ = vr.restated_planes_with_noise_types(graph, 4, 0.01, 1.0, 0)
    o = ol.OracleObject.from_dense(cc, r_sdf, r_typ)
    o.update_occupied_voxel_ranges()
    o.compute_all_derived_state()
    want = {}
    for key, gen in (("noise", SDFVoxelGenerator(1.0, graph, noise)), ("same", SDFVoxelGenerator(1.0, graph, 5))):
        ref = VoxelObject.generate_without_derived_state(ctx, gen)
        want[key] = ref.download(flags=False, labels=False)
        ref.close()
    assert not np.array_equal(want["noise"][1], want["same"][1])
    obj = VoxelObject(ctx, cc, 1.0)
    obj.set_sdf_program(SDFVoxelGenerator(1.0, graph, 5))  # (the resident program's own type is ignored while noise types are on)
    obj.set_voxel_type_generator(noise)
    obj.set_densities(DENSITIES)
    obj.set_sample_ahead(True)
    n = obj.n_voxels
    junk_sdf, junk_typ = np.full(n, 0x55, np.int8), np.full(n, 0x55, np.uint8)

    def step_equals(w):
        res = obj.step(capi.STAGE_ALL)
        got = obj.download(flags=False, labels=False)
        np.testing.assert_array_equal(got[0], w[0])
        np.testing.assert_array_equal(got[1], w[1])
        np.testing.assert_array_equal(got[4]["gen_kind"], w[4]["gen_kind"])
        return res

    for _ in range(3):
        res = step_equals(want["noise"])
        parity = pu.step_parity(o, obj, res, DENSITIES)  # derived state, labels, mesh with materials, regions, moments of the step itself
        assert parity["equal"], parity
        capi.check(capi.lib().ivx_grid_upload_dense(obj.h, junk_sdf.ctypes.data, junk_typ.ctypes.data, n))
    capi.check(capi.lib().ivx_grid_set_voxel_type_noise(obj.h, 0, 0.0, 0.0, 0))
    for _ in range(2):
        step_equals(want["same"])
        capi.check(capi.lib().ivx_grid_upload_dense(obj.h, junk_sdf.ctypes.data, junk_typ.ctypes.data, n))
    obj.close()


@pytest.mark.parametrize("body", ["box", "sphere"])
def test_slabs_generate_the_whole_grids_chunks(ctx, body):
    gen = SDFVoxelGenerator(1.0, box(40.0) if body == "box" else sphere60(), GradientNoiseVoxelTypeGenerator(4, 0.01, 1.0, 0))
    whole = VoxelObject.generate_without_derived_state(ctx, gen)
    w_sdf, w_typ, _, _, w_info = whole.download(flags=False, labels=False)
    cx, cy, cz = whole.chunk_counts
    assert cx >= 2
    for x0, x1 in ((0, cx // 2), (cx // 2, cx)):
        part = VoxelObject.generate_without_derived_state(ctx, gen, x_chunk_range=(x0, x1))
        p_sdf, p_typ, _, _, p_info = part.download(flags=False, labels=False)
        c0, c1 = x0 * cy * cz, x1 * cy * cz
        np.testing.assert_array_equal(p_sdf, w_sdf[c0 * 4096 : c1 * 4096])
        np.testing.assert_array_equal(p_typ, w_typ[c0 * 4096 : c1 * 4096])
        for f in ("kind", "gen_kind", "flags", "uniform_type"):
            np.testing.assert_array_equal(p_info[f], w_info[c0:c1][f], err_msg=f)
        part.close()
    whole.close()


def test_invalid_arguments_leave_the_generator_as_it_was(ctx):
    L = capi.lib()
    gen = SDFVoxelGenerator(1.0, box(20.0), GradientNoiseVoxelTypeGenerator(4, 0.05, 1.0, 3))
    g = VoxelObject.generate_without_derived_state(ctx, gen)
    before = g.download(flags=False, labels=False)
    assert len(np.unique(before[1])) >= 3
    assert L.ivx_grid_set_voxel_type_noise(g.h, 256, 0.05, 1.0, 3) == capi.IVX_ERR_INVALID
    assert L.ivx_grid_set_voxel_type_noise(g.h, 4, float("nan"), 1.0, 3) == capi.IVX_ERR_INVALID
    assert L.ivx_grid_set_voxel_type_noise(g.h, 4, 0.05, float("inf"), 3) == capi.IVX_ERR_INVALID
    sg = gen.sdf_generator
    shape = np.asarray(gen.grid_shape(), dtype=np.uint32)
    capi.check(L.ivx_sdf_sample(g.h, capi.ptr(sg.nodes), len(sg.nodes), sg.required_forward_stack_size, capi.ptr(shape),
                                capi.ptr(gen.shifted_grid_center), 0))
    after = g.download(flags=False, labels=False)
    for a, b in zip(before[:2], after[:2]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(before[4]["gen_kind"], after[4]["gen_kind"])
    g.close()
