"""The store forms of the three big kernels of a step (device_common.hpp: plain, nt, write-through, write-through + nt; one policy per output
stream of the evaluator, the derive sweep and the mesher). What can go wrong with a store form is a range or an address: a store dropped, a
store in a neighbour's plane, a path that kept another form and now disagrees. The smallest shapes that show these, each through the C ABI
against the oracle: one chunk; a ragged grid with surface in its first and last chunks; a chunk the sweep demotes (its fresh sdf / type
planes); the planes form of the sweep after an edit; two objects that share one device block, stepped alone and in one `_many` bracket.
The sign rows and the k-face bytes have no download of their own: the step's sweep makes the flags and the labels from nothing else, and
the mesher takes its tile rims from the k-face bytes, so they are checked through the flags, labels and mesh of the step that follows."""
import numpy as np
import pytest

import oracle_lib as ol
import parity_util as pu
from impact_amd import capi, many, scenes
from impact_amd.voxel import SDFVoxelGenerator, VoxelObject
from test_gpu_clip import box_planes
from test_gpu_split import assert_objects_equal

pytestmark = pytest.mark.gpu

NO_SAMPLE = capi.STAGE_ALL & ~capi.STAGE_SAMPLE
ONES = np.ones(256, dtype=np.float32)
RAGGED_BOX = (25.0, 41.0, 73.0)  # + the border: a 27 x 43 x 75 grid, 2 x 3 x 5 chunks, no dimension a multiple of 16


def derived_oracle(graph):
    o = pu.oracle_from_graph(graph)
    o.update_occupied_voxel_ranges()
    o.compute_all_derived_state()
    return o


def sampled(ctx, graph):
    gen = SDFVoxelGenerator(1.0, graph, 0)
    obj = VoxelObject(ctx, gen.chunk_counts(), 1.0)
    obj.set_sdf_program(gen)
    obj.set_densities(ONES)
    return gen, obj


def dented_solid():
    """48^3 voxels, all maximally inside (27 chunks uploaded Uniform) but for a dent in chunk (0, 1, 1) that reaches its face towards the
    centre chunk: the centre chunk is Uniform beside a face that is not full, and the chunks on the grid's faces lack a neighbour."""
    cc = (3, 3, 3)
    sd = np.full((48, 48, 48), -128, np.int8)
    sd[12:16, 20:28, 21:27] = 127
    sd[11, 20:28, 21:27] = -30
    ty = np.full(sd.shape, 3, np.uint8)
    return cc, ol.dense_to_tiled(sd), ol.dense_to_tiled(ty)


def dented_pair(ctx):
    cc, sd_t, ty_t = dented_solid()
    o = ol.OracleObject.from_dense(cc, sd_t, ty_t, 1.0)
    g = VoxelObject.from_dense(ctx, cc, sd_t, ty_t, 1.0)
    g.set_densities(ONES)
    o.update_occupied_voxel_ranges()
    o.compute_all_derived_state()
    return o, g


def test_one_chunk(ctx):
    """A sphere inside a 1 x 1 x 1 grid: all four planes, the records and the mesh of two steps (the second starts from the first one's list)"""
    graph = scenes.sphere_scene(6.0)
    o = derived_oracle(graph)
    gen, a = sampled(ctx, graph)
    assert gen.chunk_counts() == (1, 1, 1) and int(o.export_dense()[4]["kind"][0]) == 2
    for _ in range(2):
        p = pu.step_parity(o, a, a.step(capi.STAGE_ALL))
        assert p["equal"], p
    pu.assert_derived_equal(o, a)
    a.close()


def test_ragged_grid_first_and_last_chunk(ctx):
    """2 x 3 x 5 chunks, no dimension of the grid a multiple of 16 (the evaluator's in-grid path), surface in the first chunk and in the
    last, which has the highest addresses of every plane"""
    graph = scenes.box_scene(RAGGED_BOX)
    o = derived_oracle(graph)
    gen, a = sampled(ctx, graph)
    assert gen.chunk_counts() == (2, 3, 5) and all(s % 16 for s in gen.grid_shape())
    kinds = o.export_dense()[4]["kind"]
    assert len(kinds) == 30 and int(kinds[0]) == 2 and int(kinds[-1]) == 2
    for _ in range(2):
        p = pu.step_parity(o, a, a.step(capi.STAGE_ALL))
        assert p["equal"], p
    pu.assert_derived_equal(o, a)
    a.close()


def test_demoted_chunk(ctx):
    """A solid body over 3 x 3 x 3 chunks: the centre chunk is uploaded Uniform beside a face that is not full, and the sweep gives it
    (and the chunks on the grid's faces) fresh sdf / type planes"""
    o, g = dented_pair(ctx)
    info = o.export_dense()[4]
    demoted = (info["gen_kind"] == 1) & (info["kind"] == 2)
    assert demoted.any() and bool(demoted[13])  # (13: the centre chunk)
    p = pu.step_parity(o, g, g.step(NO_SAMPLE))
    assert p["equal"], p
    g_info = g.download()[4]
    assert ((g_info["gen_kind"] == 1) & (g_info["kind"] == 2)).sum() == demoted.sum()
    pu.assert_derived_equal(o, g)
    pu.assert_mesh_equal(o, g)
    g.close()


def test_planes_form_of_the_sweep_after_a_bite(ctx):
    """The ragged body after an absorbing sphere's bite (the sign rows are no longer current: the sweep takes its planes form), then a
    full step, which samples the body anew"""
    graph = scenes.box_scene(RAGGED_BOX)
    o = derived_oracle(graph)
    _, a = sampled(ctx, graph)
    assert pu.step_parity(o, a, a.step(capi.STAGE_ALL))["equal"]
    occ = np.array(o.info()["occupied_voxel_ranges"], dtype=np.float32)
    centre = np.array([occ[0, 1] - 2.0, occ[1, 1] - 3.0, occ[2, 1] - 2.0], np.float32)  # in the last chunk
    o.absorb_sphere(centre, 9.0, 7.0, None)
    a.absorb_sphere(centre, 9.0, 7.0, None)
    r = a.step(NO_SAMPLE)
    om = o.mesh()
    assert (int(r["mesh"]["n_vertices"]), int(r["mesh"]["n_indices"])) == (om.positions.shape[0], om.indices.shape[0])
    pu.assert_edited_objects_equal(o, a, "after the bite: ")
    fresh = derived_oracle(graph)
    p = pu.step_parity(fresh, a, a.step(capi.STAGE_ALL))
    assert p["equal"], p
    a.close()


def halves(ctx):
    """the two halves of a cut of the dented solid at x = 24, copied out in one call (the children share one device block)"""
    o, g = dented_pair(ctx)
    g.step(NO_SAMPLE)
    sets = [(box_planes((-100, -100, -100), (24, 100, 100)), (-100, -100, -100, 24, 100, 100)),
            (box_planes((24, -100, -100), (100, 100, 100)), (24, -100, -100, 100, 100, 100))]
    res = g.copy_polyhedra([s[1] for s in sets], [s[0] for s in sets])
    pairs = []
    for (planes, bb), (rc, child, off) in zip(sets, res):
        rco, co, org = o.clip_polyhedron(planes, bb, copy=True)
        assert rc == rco == 1 and tuple(off) == tuple(org)
        child.set_densities(ONES)
        pairs.append((co, child))
    g.close()
    return pairs


def test_two_objects_from_one_block(ctx):
    """Each half stepped alone, and both in one `_many` bracket: a range too long on one object shows in the other's planes"""
    alone, together = halves(ctx), halves(ctx)
    for k, (o, g) in enumerate(alone):
        r = g.step(NO_SAMPLE)
        om = o.mesh()
        assert (int(r["mesh"]["n_vertices"]), int(r["mesh"]["n_indices"])) == (om.positions.shape[0], om.indices.shape[0])
    for k, (o, g) in enumerate(alone):  # (compared after BOTH were stepped: the second one's stores are in by now)
        assert_objects_equal(o, g, f"half {k} stepped alone: ")
    res = many.voxel_step_many([g for _, g in together], NO_SAMPLE)
    for k, (o, g) in enumerate(together):
        om = o.mesh()
        assert (int(res[k]["mesh"]["n_vertices"]), int(res[k]["mesh"]["n_indices"])) == (om.positions.shape[0], om.indices.shape[0])
        assert_objects_equal(o, g, f"half {k} stepped with the other: ")
        for x, y in zip(g.download(), alone[k][1].download()):
            assert np.array_equal(np.asarray(x), np.asarray(y)), k
    for _, g in alone + together:
        g.close()
