"""The mesher's single-type form (k_step_emit<true>, role_sn_emit<.., true>): a grid whose voxels all came from the sampler with one type
is meshed without its type plane. Every case here is compared bit for bit with the oracle, on both sides of the switch between the
single-type form and the general one."""
import numpy as np
import pytest

import oracle_lib as ol
import parity_util as pu
from impact_amd import capi, many, scenes
from impact_amd.voxel import SDFVoxelGenerator, VoxelObject

pytestmark = pytest.mark.gpu

NO_SAMPLE = capi.STAGE_ALL & ~capi.STAGE_SAMPLE


def sampled(ctx, graph, vtype):
    gen = SDFVoxelGenerator(1.0, graph, vtype)
    obj = VoxelObject(ctx, gen.chunk_counts(), 1.0)
    obj.set_sdf_program(gen)
    obj.set_densities(np.ones(256, dtype=np.float32))
    return gen, obj


def oracle_of(graph, vtype):
    o = pu.oracle_from_graph(graph, 1.0, vtype)
    o.update_occupied_voxel_ranges()
    o.compute_all_derived_state()
    return o


MESH_KEYS = ("index_sha", "position_sha", "normal_sha", "index_material_sha", "triangles", "vertices")


def mesh_equal(p):
    return all(p[k][0] == p[k][1] for k in MESH_KEYS)


@pytest.mark.parametrize("vtype", [0, 7])
def test_sampled_body_with_empty_and_uniform_neighbours(ctx, vtype):
    """(a) A sampled single-type body, of type 0 and of another type: its surface chunks border NonUniform chunks without a non-empty
    voxel (type 0xFF throughout) and Uniform chunks (the type of their record)."""
    graph = scenes.asteroid_scene(0.6)
    o = oracle_of(graph, vtype)
    _, obj = sampled(ctx, graph, vtype)
    for _ in range(2):
        r = obj.step(capi.STAGE_ALL)
        p = pu.step_parity(o, obj, r)
        assert p["equal"], p
    _, typ, _, _, info = obj.download()
    nonuniform = info["kind"] == 2
    assert nonuniform.any() and (info["kind"] == 1).any()
    # (the grid holds NonUniform chunks with no non-empty voxel)
    per_chunk = typ.reshape(len(info), -1)
    assert (per_chunk[nonuniform] == 0xFF).all(axis=1).any()
    obj.close()


def test_sample_edit_step_resample_step(ctx):
    """(b) The mesher alternates between its two forms: sampled (single type), edited (the general form: the edit rewrote voxels), sampled
    again with ANOTHER type (single type), stepped without sampling (still single type), each against the oracle."""
    graph = scenes.asteroid_scene(0.5)
    gen_a, obj = sampled(ctx, graph, 2)
    o = oracle_of(graph, 2)
    r = obj.step(capi.STAGE_ALL)
    assert pu.step_parity(o, obj, r)["equal"]
    centre = np.array([0.5 * (a + b) for a, b in o.info()["occupied_voxel_ranges"]], np.float32)
    centre = centre + np.float32(40.0) * np.array([0.6, 0.0, 0.8], np.float32)
    o.absorb_sphere(centre, 15.0, 13.0, None)
    obj.absorb_sphere(centre, 15.0, 13.0, None)
    r = obj.step(NO_SAMPLE)  # (the edit rewrote voxels: the general form)
    p = pu.step_parity(o, obj, r)
    assert mesh_equal(p), p
    pu.assert_edited_objects_equal(o, obj, "after the edit: ")
    gen_b = SDFVoxelGenerator(1.0, graph, 5)
    assert gen_b.chunk_counts() == gen_a.chunk_counts()
    obj.set_sdf_program(gen_b)
    o5 = oracle_of(graph, 5)
    r = obj.step(capi.STAGE_ALL)
    p = pu.step_parity(o5, obj, r)
    assert p["equal"], p
    r = obj.step(NO_SAMPLE)
    p = pu.step_parity(o5, obj, r)
    assert p["equal"], p
    obj.close()


def uploaded_two_types(ctx, seed):
    rng = np.random.default_rng(seed)
    cc = (3, 2, 3)
    blobs = rng.random((cc[0] * 16, cc[1] * 16, cc[2] * 16))
    for ax in range(3):
        blobs = 0.5 * blobs + 0.25 * (np.roll(blobs, 1, ax) + np.roll(blobs, -1, ax))
    sd = np.where(blobs > 0.55, -128, np.where(blobs > 0.52, rng.integers(-60, -1, blobs.shape), rng.integers(0, 127, blobs.shape))).astype(np.int8)
    sd[16:32, :, 0:16] = -128  # a Uniform chunk
    ty = np.where(np.arange(cc[0] * 16)[:, None, None] < 24, 1, 4) * np.ones(blobs.shape, np.uint8)
    ty = ty.astype(np.uint8)
    sd_t, ty_t = ol.dense_to_tiled(sd), ol.dense_to_tiled(ty)
    o = ol.OracleObject.from_dense(cc, sd_t, ty_t, 1.0)
    g = VoxelObject.from_dense(ctx, cc, sd_t, ty_t, 1.0)
    g.set_densities(np.ones(256, dtype=np.float32))
    o.update_occupied_voxel_ranges()
    o.compute_all_derived_state()
    return o, g


def test_upload_with_two_types(ctx):
    """(c) Planes uploaded with two voxel types: the step's mesher takes the general form, and its mesh (index materials included) is the
    oracle's."""
    o, g = uploaded_two_types(ctx, 11)
    r = g.step(NO_SAMPLE)
    p = pu.step_parity(o, g, r)
    assert p["equal"], p
    pu.assert_mesh_equal(o, g)
    g.close()


def test_many_batch_of_a_sampled_and_an_uploaded_grid(ctx):
    """(d) One `_many` step over a sampled single-type grid and an uploaded two-type grid: each equals its oracle, and equals the same
    object stepped alone."""
    graph = scenes.asteroid_scene(0.4)
    os_ = oracle_of(graph, 3)
    _, gs = sampled(ctx, graph, 3)
    gs.step(capi.STAGE_ALL)  # (sampled, single type from here on)
    ou, gu = uploaded_two_types(ctx, 12)
    res = many.voxel_step_many([gs, gu], NO_SAMPLE)
    p = pu.step_parity(os_, gs, res[0])
    assert p["equal"], p
    p = pu.step_parity(ou, gu, res[1])
    assert p["equal"], p
    # the sampled grid stepped alone (the single-type form) leaves the same mesh as the batch (the general form)
    r = gs.step(NO_SAMPLE)
    p = pu.step_parity(os_, gs, r)
    assert p["equal"], p
    gs.close()
    gu.close()
