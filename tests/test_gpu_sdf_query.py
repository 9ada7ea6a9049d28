"""SDF queries on the device (impact_amd/csrc/sdf_query.hip): the kernels run the functions the host build runs, so every device result is
byte-equal to the host build's, with no tolerance — all five calls, over the programs of test_sdf_query_cpu.py (which ties the host build to the
restatement, the oracle and float64), instance counts around what a wave and a workgroup hold, a batch that mixes every exit inside one wave,
repetition, two objects alive, a call behind an enqueued voxel step, and the tie to `ivx_sdf_sample`."""
import numpy as np
import pytest

import sdf_query_ref as R
import test_sdf_query_cpu as cpu
from impact_amd import capi, sdf_query as sq
from impact_amd.sdf_graph import SDFGraph, SDFNode
from impact_amd.voxel import SDFGenerator, SDFVoxelGenerator, VoxelObject

pytestmark = pytest.mark.gpu

f32 = np.float32
same_bytes = cpu.same_bytes
# eight lanes to an instance and one-wave workgroups: a wave and a workgroup hold 8 instances (64 points of `distances`, a lane per point)
PER_WAVE, POINTS_PER_WAVE = 8, 64


def both(gen, ctx):
    return sq.SDFQuery(gen, ctx), sq.SDFQuery(gen, device=False)


def assert_all_calls_equal(dev, host, surface, inst, direction, cast=(40, 0.05, 0.7)):
    pts = np.ascontiguousarray(inst["subject_to_parent"]["translation"])
    assert same_bytes(dev.distances(pts), host.distances(pts))
    assert same_bytes(dev.gradients(pts), host.gradients(pts))
    assert same_bytes(dev.closest(surface, inst), host.closest(surface, inst))
    assert same_bytes(dev.rotation(surface, inst), host.rotation(surface, inst))
    got, want = dev.spherecast(surface, inst, direction, *cast), host.spherecast(surface, inst, direction, *cast)
    assert same_bytes(got, want)
    return want


@pytest.mark.parametrize("name", cpu.ALL_PROGRAMS)
def test_device_is_byte_equal_to_the_host_build(ctx, name):
    gen = cpu.generator_of(name)
    dev, host = both(gen, ctx)
    rng = np.random.default_rng(len(name) * 1000 + sum(map(ord, name)))
    inst, surface = R.shell_instances(gen, rng, 24), R.a_surface(rng)
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    assert_all_calls_equal(dev, host, surface, inst, d)
    below = inst.copy()
    below["subject_to_parent"]["translation"][:, 1] = min(float(gen.domain[1]), -1.0) - 8.0
    assert same_bytes(dev.spherecast(None, below), host.spherecast(None, below))  # (the reference's constants)
    dev.close()


COUNTS = [0, 1, PER_WAVE - 1, PER_WAVE, PER_WAVE + 1, POINTS_PER_WAVE - 1, POINTS_PER_WAVE, POINTS_PER_WAVE + 1, 37 * PER_WAVE + 3]


@pytest.fixture(scope="module")
def counted(ctx):
    gen = cpu.generator_of("random509")  # (34 nodes, four levels, noise)
    dev, host = both(gen, ctx)
    yield gen, dev, host
    dev.close()


@pytest.mark.parametrize("n", COUNTS)
def test_instance_counts_around_a_wave_and_a_workgroup(counted, n):
    gen, dev, host = counted
    rng = np.random.default_rng(n)
    inst = R.shell_instances(gen, rng, n)
    below = inst.copy()
    below["subject_to_parent"]["translation"][:, 1] = float(gen.domain[1]) - 8.0
    below["subject_to_parent"]["rotation"] = (0, 0, 0, 1)
    want = assert_all_calls_equal(dev, host, R.a_surface(rng), below, (0.0, 1.0, 0.0), cast=(128, 0.1, 0.5))
    assert len(want) == n
    if n >= POINTS_PER_WAVE:
        assert len(set(want["steps"].tolist())) > 3  # (lanes of a wave finish after different step counts)


def test_a_wave_that_mixes_every_exit(ctx):
    """eight instances, one wave: every status of the cast and both of its Some exits, each lane group finishing after its own number of steps"""
    one = lambda t, r: sq.instances([t], sphere_radii=[r])  # noqa: E731
    g = SDFGraph()
    g.add_node(SDFNode.new_sphere(10.0))
    dev, host = both(SDFGenerator(g), ctx)
    inst = np.concatenate([one((30, -30, 0), 1.0), one((0, 0, 0), 1.0), one((0, 1, 0), 1.0), one((9.5, -30, 9.5), 0.5), one((6, -30, 0), 1.0), one((0, -30, 0), 1.0),
                           one((9.99, -30, 0), 0.2), one((6, -30, 0), 0.0)])
    assert len(inst) == PER_WAVE
    want = host.spherecast(None, inst, max_steps=12)
    assert same_bytes(dev.spherecast(None, inst, max_steps=12), want)
    assert set(want["status"].tolist()) == {capi.SQ_RAY_MISSES_DOMAIN, capi.SQ_PENETRATING, capi.SQ_NO_GRADIENT_DIRECTION, capi.SQ_LEFT_INTERVAL, capi.SQ_OK, capi.SQ_MAX_STEPS}
    assert len(set(want["steps"].tolist())) >= 4
    assert same_bytes(dev.spherecast(None, inst, direction=(0, 0, 0)), host.spherecast(None, inst, direction=(0, 0, 0)))
    assert np.all(host.spherecast(None, inst, direction=(0, 0, 0))["status"] == capi.SQ_DEGENERATE_DIRECTION)
    # closest and rotation: the centre (no gradient), a first-sample convergence, longer runs, a degenerate subject
    mixed = sq.instances([(0, 0, 0), (0, 10.05, 0), (3, 25, 1), (30, -30, 0), (0, 14, 0), (1, 2, 3), (-9, 9, 9), (3, 25, 1)], scalings=[1, 1, 1, 1, 1, 1, 1, 0])
    want = host.closest(None, mixed, 3, 0.001)
    assert same_bytes(dev.closest(None, mixed, 3, 0.001), want)
    assert set(want["status"].tolist()) == {capi.SQ_OK, capi.SQ_ZERO_GRADIENT} and len(set(want["steps"].tolist())) >= 3
    want = host.rotation(None, mixed)
    assert same_bytes(dev.rotation(None, mixed), want)
    assert set(want["status"].tolist()) == {capi.SQ_OK, capi.SQ_NO_GRADIENT_DIRECTION, capi.SQ_DEGENERATE_Y_AXIS}
    dev.close()
    # the crossed exit beside the others, on the noisy sphere
    dev, host = both(cpu.generator_of("noise_block"), ctx)
    rng = np.random.default_rng(1)
    t = np.stack([rng.uniform(-8, 8, 64), np.full(64, -30.0), rng.uniform(-8, 8, 64)], axis=1)
    inst = sq.instances(np.round(t * 4) / 4, sphere_radii=np.full(64, 1.0))
    want = host.spherecast(None, inst, max_steps=4, tolerance=1e-3, safety_factor=1.0)
    assert same_bytes(dev.spherecast(None, inst, max_steps=4, tolerance=1e-3, safety_factor=1.0), want)
    first = want[:PER_WAVE]
    assert capi.SQ_MAX_STEPS in first["status"] and np.any(want["exit"] == capi.SQ_EXIT_CROSSED) and np.any((want["status"] == 0) & (want["exit"] == 0))
    dev.close()


def test_the_same_call_twice_gives_the_same_bytes(counted):
    gen, dev, _ = counted
    rng = np.random.default_rng(77)
    inst, surface = R.shell_instances(gen, rng, 100), R.a_surface(rng)
    pts = np.ascontiguousarray(inst["subject_to_parent"]["translation"])
    for call in (lambda: dev.distances(pts), lambda: dev.gradients(pts), lambda: dev.closest(surface, inst), lambda: dev.spherecast(surface, inst, (0.6, 0.0, 0.8)),
                 lambda: dev.rotation(surface, inst)):
        first = call().copy()
        assert same_bytes(first, call())


def test_two_query_objects_alive_at_once(ctx):
    gens = [cpu.generator_of("max_stack"), cpu.generator_of("noise_rotated")]
    devs = [sq.SDFQuery(g, ctx) for g in gens]
    hosts = [sq.SDFQuery(g, device=False) for g in gens]
    rng = np.random.default_rng(5)
    insts = [R.shell_instances(g, rng, 20) for g in gens]
    for _ in range(2):  # (interleaved: neither object's program or buffers serve the other's call)
        for dev, host, inst in zip(devs, hosts, insts):
            assert same_bytes(dev.closest(None, inst), host.closest(None, inst))
            assert same_bytes(dev.gradients(inst["subject_to_parent"]["translation"]), host.gradients(inst["subject_to_parent"]["translation"]))
    for dev in devs:
        dev.close()


def test_a_call_behind_an_enqueued_voxel_step(ctx, counted):
    gen, dev, host = counted
    vg = SDFVoxelGenerator(1.0, cpu.exact_position_graph(1), 0)
    obj = VoxelObject(ctx, vg.chunk_counts(), 1.0)
    obj.set_sdf_program(vg)
    obj.set_densities(np.ones(256, dtype=f32))
    alone = obj.step(capi.STAGE_ALL).copy()
    rng = np.random.default_rng(9)
    inst = R.shell_instances(gen, rng, 50)
    obj.step_enqueue(capi.STAGE_ALL)
    got = dev.spherecast(None, inst, (0.0, -1.0, 0.0))
    r = obj.step_collect()
    assert same_bytes(got, host.spherecast(None, inst, (0.0, -1.0, 0.0)))
    assert int(r["region_count"]) == int(alone["region_count"]) and same_bytes(r["mesh"], alone["mesh"]) and same_bytes(r["moments"], alone["moments"])
    obj.close()


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_distances_at_voxel_centres_are_the_samplers_voxel_bytes(ctx, variant):
    gen = SDFVoxelGenerator(1.0, cpu.exact_position_graph(variant), 0)
    assert cpu.no_block_shortcut_fires(gen)
    obj = VoxelObject.generate_without_derived_state(ctx, gen)
    sdf, _, _, _, info = obj.download(flags=False, labels=False)
    obj.close()
    dev = sq.SDFQuery(gen.sdf_generator, ctx)
    cc = gen.chunk_counts()
    checked = 0
    for ci in range(cc[0]):
        for cj in range(cc[1]):
            for ck in range(cc[2]):
                c = (ci * cc[1] + cj) * cc[2] + ck
                if info["gen_kind"][c] != 2:
                    continue
                pts, inside = cpu.chunk_points(gen, ci, cj, ck)
                np.testing.assert_array_equal(cpu.quantised(dev.distances(pts))[inside], sdf[c * 4096 : (c + 1) * 4096][inside])
                checked += int(inside.sum())
    assert checked == 8 * 4096
    dev.close()
