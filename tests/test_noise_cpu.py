"""Multifractal noise SDF nodes (kind 6) on the host: the noise definition (impact_amd/csrc/noise.hpp) against its numpy restatement
(tests/noise_ref.py) bit for bit, its proven bounds, and the compile of noisy graphs (atomic.rs:228-596, 1364-1391)."""
import numpy as np
import pytest

import noise_ref as nr
from impact_amd import capi
from impact_amd.sdf_graph import SDFGraph, SDFNode
from impact_amd.voxel import SDFGenerator, SDFVoxelGenerator

f32 = np.float32


def noise_params(freq, lacunarity, gain, octaves, seed):
    p = np.zeros(5, f32)
    p[:3] = (freq, lacunarity, gain)
    p.view(np.uint32)[3] = octaves
    p.view(np.uint32)[4] = seed
    return p


def point_sets():
    """10^5 points in four dimensions: ordinary, negative, exact lattice points, and coordinates of +-1e4"""
    rng = np.random.default_rng(2024)
    pts = (rng.standard_normal((100000, 4)) * 40.0).astype(f32)
    pts[:20000] = -np.abs(pts[:20000])
    pts[20000:30000] = np.round(pts[20000:30000])
    pts[30000:31000] = rng.choice([-1e4, 1e4], size=(1000, 4)).astype(f32)
    pts[31000:32000] = (rng.uniform(-1e4, 1e4, (1000, 4))).astype(f32)
    return [pts]


def host_noise(which, params, pts):
    pts = np.ascontiguousarray(pts, dtype=f32)
    out = np.zeros(pts.shape[0], f32)
    capi.check(capi.lib().ivx_noise_eval(None, which, params.ctypes.data, pts.ctypes.data, pts.shape[0], out.ctypes.data))
    return out


@pytest.mark.parametrize("octaves", list(range(9)))
def test_fbm3_host_equals_restatement(octaves):
    (pts,) = point_sets()
    for gain in (1.0, 0.6):
        got = host_noise(0, noise_params(0.05, 2.0, gain, octaves, 991), pts[:, :3])
        want = nr.fbm3(pts[:, 0], pts[:, 1], pts[:, 2], octaves, 0.05, 2.0, gain, 991)
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def test_simplex4_host_equals_restatement():
    (pts,) = point_sets()
    for scale in (1.0, 0.05):
        p = (pts * f32(scale)).astype(f32)
        got = host_noise(1, noise_params(0, 0, 0, 0, 31337), p)
        want = nr.simplex4(p[:, 0], p[:, 1], p[:, 2], p[:, 3], 31337)
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def test_bounds_hold():
    rng = np.random.default_rng(5)
    m3 = m4 = 0.0
    for _ in range(10):
        p = rng.uniform(-64.0, 64.0, (1000000, 4)).astype(f32)
        m3 = max(m3, float(np.abs(host_noise(0, noise_params(1.0, 1.0, 1.0, 1, 3), p[:, :3])).max()))
        m4 = max(m4, float(np.abs(host_noise(1, noise_params(0, 0, 0, 0, 3), p)).max()))
    assert 0.5 < m3 <= nr.B3 and 0.5 < m4 <= nr.B4


def _noisy_sphere(radius, octaves, frequency, lacunarity, persistence, amplitude, seed):
    g = SDFGraph()
    s = g.add_node(SDFNode.new_sphere(radius))
    g.set_root_node(g.add_node(SDFNode.new_multifractal_noise(s, octaves, frequency, lacunarity, persistence, amplitude, seed)))
    return g


def test_compile_benchmark_sphere():
    # reference generation benchmark: sphere r = 80 with noise (8, 0.02, 2.0, 0.6, 4.0, 0)
    g = _noisy_sphere(80.0, 8, 0.02, 2.0, 0.6, 4.0, 0)
    gen = SDFGenerator(g)
    assert list(gen.domain) == [-84.0] * 3 + [84.0] * 3
    nodes = gen.nodes
    assert [int(k) for k in nodes["kind"]] == [0, 6]
    sphere, noise = nodes
    inherent = (f32(1) - f32(0.6) ** 8) / (f32(1) - f32(0.6))
    assert noise["a"] == pytest.approx(4.0 / inherent, rel=1e-6)
    assert (noise["b"], noise["c"]) == (f32(0.02), f32(2.0))
    assert noise["reserved"][0:1].view(f32)[0] == f32(0.6) and noise["reserved"][1] == 8 and noise["reserved"][2] == 0
    margin = f32(0.02) * f32(127)
    assert noise["margin"] == margin and sphere["margin"] == margin + f32(4.0)  # the child's margin grows by the amplitude
    np.testing.assert_array_equal(noise["domain_lo"], [-84.0 - margin] * 3)
    np.testing.assert_array_equal(sphere["domain_lo"], [-80.0 - (margin + f32(4.0))] * 3)
    np.testing.assert_array_equal(noise["transform"], sphere["transform"])
    assert noise["leaf_count"] == 1 and gen.required_forward_stack_size == 1
    vg = SDFVoxelGenerator(1.0, g)
    assert tuple(vg.grid_shape()) == (170, 170, 170) and tuple(vg.chunk_counts()) == (11, 11, 11)


def test_compile_noise_scale_edge_cases():
    g = _noisy_sphere(10.0, 0, 0.1, 2.0, 0.5, 3.0, 1)  # no octaves: theoretical amplitude 0 -> noise_scale 0
    assert SDFGenerator(g).nodes[-1]["a"] == 0.0
    g = _noisy_sphere(10.0, 5, 0.1, 2.0, 1.0, 3.0, 1)  # persistence 1: the amplitude is the octave count
    assert SDFGenerator(g).nodes[-1]["a"] == f32(3.0) / f32(5.0)


def test_compile_noise_under_transforms():
    g = SDFGraph()
    b = g.add_node(SDFNode.new_box([20.0, 10.0, 6.0]))
    n = g.add_node(SDFNode.new_multifractal_noise(b, 3, 0.1, 2.0, 0.5, 1.5, 9))
    t = g.add_node(SDFNode.new_translation(n, [5.0, 0.0, -3.0]))
    g.set_root_node(g.add_node(SDFNode.new_scaling(t, 2.0)))
    gen = SDFGenerator(g)
    np.testing.assert_array_equal(np.asarray(gen.domain, f32), f32([(-10 - 1.5 + 5) * 2, -6.5 * 2, (-3 - 1.5 - 3) * 2, (10 + 1.5 + 5) * 2, 6.5 * 2, (3 + 1.5 - 3) * 2]))
    box, noise = gen.nodes[0], gen.nodes[1]
    np.testing.assert_array_equal(box["transform"], noise["transform"])
    assert box["margin"] == noise["margin"] + f32(1.5)


def test_self_referencing_noise_is_rejected():
    g = SDFGraph()
    g.add_node(SDFNode.new_multifractal_noise(0, 4, 0.1, 2.0, 0.5, 1.0, 0))
    with pytest.raises(capi.IvxError):
        SDFGenerator(g)
