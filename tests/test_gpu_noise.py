"""Multifractal noise SDF nodes (kind 6) on the device: the device build of the noise functions, amplitude-0 noise through the whole
sampler against the oracle, and noisy objects against a numpy restatement of the reference's block semantics (atomic.rs:633-875,
1420-1571) followed by the oracle's derived state, mesh, regions and inertia of the same planes."""
import numpy as np
import pytest

import noise_block_ref as nb
import noise_ref as nr
import oracle_lib as ol
import parity_util as pu
from impact_amd import capi
from impact_amd.sdf_graph import SDFGraph, SDFNode
from impact_amd.voxel import SDFGenerator, SDFVoxelGenerator, VoxelObject
from test_gpu_random_sdf import random_tree
from test_noise_cpu import noise_params, point_sets

pytestmark = pytest.mark.gpu
f32 = np.float32


def device_noise(ctx, which, params, pts):
    pts = np.ascontiguousarray(pts, dtype=f32)
    out = np.zeros(pts.shape[0], f32)
    capi.check(capi.lib().ivx_noise_eval(ctx.h, which, params.ctypes.data, pts.ctypes.data, pts.shape[0], out.ctypes.data))
    return out


def test_device_noise_equals_restatement(ctx):
    for pts in point_sets():
        for octaves in (0, 1, 2, 5, 8):
            for gain in (1.0, 0.6):
                got = device_noise(ctx, 0, noise_params(0.05, 2.0, gain, octaves, 77), pts[:, :3])
                want = nr.fbm3(pts[:, 0], pts[:, 1], pts[:, 2], octaves, 0.05, 2.0, gain, 77)
                np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        got = device_noise(ctx, 1, noise_params(0, 0, 0, 0, 4242), pts * f32(0.05))
        want = nr.simplex4(*(pts * f32(0.05)).T, 4242)
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def _with_noise(g_src, rng, amplitude=(0.0, 0.0)):
    """the same graph with noise nodes (amplitude drawn from the range) above random nodes"""
    nodes = g_src.nodes().copy()
    g = SDFGraph()
    remap = {}
    for i, rec in enumerate(nodes):
        rec = rec.copy()
        if rec["kind"] in (3, 4, 5, 7, 8, 9):
            rec["child1"] = remap[int(rec["child1"])]
        if rec["kind"] in (7, 8, 9):
            rec["child2"] = remap[int(rec["child2"])]
        nid = g.add_node(rec)
        if rng.random() < 0.5:
            nid = g.add_node(SDFNode.new_multifractal_noise(nid, int(rng.integers(0, 6)), float(rng.uniform(0.01, 0.2)), 2.0, 0.5,
                                                            float(rng.uniform(*amplitude)), int(rng.integers(0, 2**32))))
        remap[i] = nid
    g.set_root_node(remap[g_src.root_node_id])
    return g


@pytest.mark.parametrize("seed", [31, 32, 33, 34, 35, 36])
def test_amplitude_zero_noise_is_plumbing_only(ctx, seed):
    rng = np.random.default_rng(seed)
    while True:  # (a tree whose root domain is degenerate has no grid to compare: draw again)
        plain = SDFGraph()
        random_tree(plain, rng, int(rng.integers(1, 4)))
        o = pu.oracle_from_graph(plain)
        if min(o.chunk_counts) > 0:
            break
    noisy = _with_noise(plain, rng)
    g = pu.gpu_from_graph(ctx, noisy)
    pu.assert_generated_equal(o, g)
    o.update_occupied_voxel_ranges()
    o.compute_all_derived_state()
    g.compute_all_derived_state()
    pu.assert_derived_equal(o, g)
    pu.assert_mesh_equal(o, g)
    pu.assert_regions_equal(o, g)
    g.close()


def noisy_sphere(radius=40.0, amplitude=3.0, octaves=4, seed=7):
    g = SDFGraph()
    s = g.add_node(SDFNode.new_sphere(radius))
    g.set_root_node(g.add_node(SDFNode.new_multifractal_noise(s, octaves, 0.05, 2.0, 0.6, amplitude, seed)))
    return g


def noisy_translated_scaled_box():
    g = SDFGraph()
    b = g.add_node(SDFNode.new_box([30.0, 18.0, 24.0]))
    n = g.add_node(SDFNode.new_multifractal_noise(b, 5, 0.08, 2.0, 0.5, 2.5, 123))
    t = g.add_node(SDFNode.new_translation(n, [3.0, -2.0, 5.0]))
    g.set_root_node(g.add_node(SDFNode.new_scaling(t, 1.5)))  # (noise below a scaling: the per-voxel path, scaled origin and frequency)
    return g


def noisy_rotated_capsule():
    g = SDFGraph()
    c = g.add_node(SDFNode.new_capsule(30.0, 9.0))
    n = g.add_node(SDFNode.new_multifractal_noise(c, 3, 0.1, 2.0, 0.6, 2.0, 5))
    g.set_root_node(g.add_node(SDFNode.new_rotation_from_axis_angle(n, [0.3, 0.8, 0.5], 0.9)))
    return g


def noisy_union():
    g = SDFGraph()
    s = g.add_node(SDFNode.new_sphere(14.0))
    ns = g.add_node(SDFNode.new_multifractal_noise(s, 4, 0.1, 2.0, 0.5, 3.0, 1))
    ts = g.add_node(SDFNode.new_translation(ns, [-20.0, 0.0, 0.0]))
    b = g.add_node(SDFNode.new_box([16.0, 20.0, 12.0]))
    nb_ = g.add_node(SDFNode.new_multifractal_noise(b, 2, 0.15, 2.5, 0.7, 1.5, 2))
    rb = g.add_node(SDFNode.new_rotation_from_axis_angle(nb_, [0.0, 0.0, 1.0], 0.5))
    tb = g.add_node(SDFNode.new_translation(rb, [22.0, 4.0, -3.0]))
    g.set_root_node(g.add_node(SDFNode.new_union(ts, tb, 0.0)))
    return g


def noise_over_smooth_subtraction():
    g = SDFGraph()
    b = g.add_node(SDFNode.new_box([40.0, 30.0, 30.0]))
    s = g.add_node(SDFNode.new_sphere(14.0))
    t = g.add_node(SDFNode.new_translation(s, [12.0, 8.0, 0.0]))
    d = g.add_node(SDFNode.new_subtraction(b, t, 4.0))
    g.set_root_node(g.add_node(SDFNode.new_multifractal_noise(d, 4, 0.07, 2.0, 0.5, 3.0, 99)))
    return g


def random_noisy_program(seed):
    """a random program of test_gpu_random_sdf's generator with noise of non-zero amplitude above random nodes (some far from
    most chunks, so that their early-out decides)"""
    rng = np.random.default_rng(1000 + seed)
    while True:
        plain = SDFGraph()
        random_tree(plain, rng, int(rng.integers(1, 4)))
        g = _with_noise(plain, rng, (0.5, 3.0))
        if min(SDFVoxelGenerator(1.0, g).chunk_counts()) > 0:
            return g


def _check_against_restatement(ctx, graph):
    cc, sdf, typ = nb.restated_planes(graph)
    g = pu.gpu_from_graph(ctx, graph)
    o = ol.OracleObject.from_dense(cc, sdf, typ)
    pu.assert_generated_equal(o, g)
    o.update_occupied_voxel_ranges()
    o.compute_all_derived_state()
    g.compute_all_derived_state()
    pu.assert_derived_equal(o, g)
    pu.assert_mesh_equal(o, g)
    pu.assert_inertia_equal(o, g, np.ones(256, dtype=f32))
    pu.assert_regions_equal(o, g)
    g.close()


@pytest.mark.parametrize("make", [noisy_sphere, noisy_translated_scaled_box, noisy_rotated_capsule, noisy_union, noise_over_smooth_subtraction])
def test_noise_values_match_restatement(ctx, make):
    _check_against_restatement(ctx, make())


def test_random_noisy_programs_match_restatement(ctx):
    """40 committed seeds; together they take every branch of the noise node's block test"""
    before = dict(nb.NOISE_BRANCHES)
    for seed in range(40):
        graph = random_noisy_program(seed)
        cc, sdf, typ = nb.restated_planes(graph)
        g = pu.gpu_from_graph(ctx, graph)
        pu.assert_generated_equal(ol.OracleObject.from_dense(cc, sdf, typ), g)
        g.close()
    taken = {k: nb.NOISE_BRANCHES[k] - before[k] for k in before}
    assert all(v > 0 for v in taken.values()), taken


def test_resident_programs_alternate(ctx):
    """two noisy programs of equal chunk counts, alternated every step with sample-ahead on, planes overwritten between steps"""
    ga, gb = noisy_sphere(30.0, 2.0, 3, 11), noisy_sphere(29.0, 3.0, 4, 12)
    gen_a, gen_b = SDFVoxelGenerator(1.0, ga, 0), SDFVoxelGenerator(1.0, gb, 0)
    assert tuple(gen_a.chunk_counts()) == tuple(gen_b.chunk_counts())
    want = []
    for gen in (gen_a, gen_b):
        ref = VoxelObject.generate_without_derived_state(ctx, gen)
        want.append(ref.download(flags=False, labels=False))
        ref.close()
    obj = VoxelObject(ctx, gen_a.chunk_counts(), 1.0)
    obj.set_densities(np.ones(256, dtype=f32))
    obj.set_sample_ahead(True)
    n = int(np.prod(gen_a.chunk_counts())) * 4096
    junk_sdf, junk_typ = np.full(n, 0x55, np.int8), np.full(n, 0x55, np.uint8)
    for step in range(10):
        obj.set_sdf_program((gen_a, gen_b)[step % 2])
        obj.step(capi.STAGE_ALL)
        got = obj.download(flags=False, labels=False)
        w = want[step % 2]
        np.testing.assert_array_equal(got[0], w[0])
        np.testing.assert_array_equal(got[1], w[1])
        np.testing.assert_array_equal(got[4]["gen_kind"], w[4]["gen_kind"])
        capi.check(capi.lib().ivx_grid_upload_dense(obj.h, junk_sdf.ctypes.data, junk_typ.ctypes.data, n))
    obj.close()


def test_resident_noise_program_equals_sample(ctx):
    graph = noisy_sphere(30.0, 2.0, 3, 11)
    gen = SDFVoxelGenerator(1.0, graph, 0)
    ref = VoxelObject.generate_without_derived_state(ctx, gen)
    want = ref.download(flags=False, labels=False)
    obj = VoxelObject(ctx, gen.chunk_counts(), 1.0)
    obj.set_sdf_program(gen)
    obj.set_densities(np.ones(256, dtype=f32))
    obj.set_sample_ahead(True)
    for _ in range(3):
        obj.step(capi.STAGE_ALL)
        got = obj.download(flags=False, labels=False)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[4]["gen_kind"], want[4]["gen_kind"])
    obj.close()
    ref.close()
