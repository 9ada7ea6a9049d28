"""GPU parity of splitting disconnected regions off a voxel object (a11: `extract_any_disconnected_region`,
object/extraction.rs:78-596, 1901-2123, driven in a loop like `handle_voxel_object_after_removing_voxels`,
interaction.rs:256) against the oracle: the same regions leave in the same order, the child's chunk grid and origin
offset agree, voxel bytes / chunk kinds / flags of non-empty voxels / local labels / meshes / moments of parent and
children agree after every extraction."""
import numpy as np
import pytest

import moments_ref as mr
import oracle_lib as ol
import parity_util as pu
from impact_amd import scenes
from impact_amd.sdf_graph import SDFGraph, SDFNode
from impact_amd.voxel import VoxelObject

pytestmark = pytest.mark.gpu


def assert_objects_equal(o, g, what=""):
    o_sdf, o_typ, o_flg, o_lab, o_info = o.export_dense()
    g_sdf, g_typ, g_flg, g_lab, g_info = g.download()
    assert o.chunk_counts == g.chunk_counts, what
    np.testing.assert_array_equal(g_sdf, o_sdf, err_msg=what + "sdf")
    ne = (o_flg & 1) == 0
    np.testing.assert_array_equal((g_flg & 1) == 0, ne, err_msg=what + "emptiness")
    np.testing.assert_array_equal(g_typ[ne], o_typ[ne], err_msg=what + "types of non-empty voxels")
    # adjacency bits of EMPTY voxels are history artefacts in the reference (oracle/src/orc_split.cpp header)
    np.testing.assert_array_equal(g_flg[ne], o_flg[ne], err_msg=what + "flags of non-empty voxels")
    np.testing.assert_array_equal(g_lab, o_lab, err_msg=what + "local labels")
    for f in ("kind", "flags", "face_dist", "region_count", "boundary_region_count"):
        np.testing.assert_array_equal(g_info[f], o_info[f], err_msg=what + f)
    pu.assert_regions_equal(o, g)
    pu.assert_mesh_equal(o, g)
    pu.assert_inertia_equal(o, g)


def split_all(ctx, o, g, expect):
    children = 0
    outcomes = []
    for it in range(64):
        before = o.export_dense()[1:3]  # (type and flag planes ahead of the split: the moved moments are sums over what leaves)
        rc_o, co, org_o = o.split_off_smallest_region()
        rc_g, cg, org_g, moved = g.extract_any_disconnected_region()
        assert rc_g == rc_o, f"iteration {it}"
        outcomes.append(rc_o)
        if rc_o == 0:
            break
        assert_objects_equal(o, g, f"parent after split {it}: ")
        if rc_o == 1:
            assert org_g == org_o
            assert_objects_equal(co, cg, f"child {it}: ")
            # the descriptor of the moved region carries its moments (PropertyTransferrer)
            _, c64 = co.inertia()
            # child moments are about the child's origin; shift check via mass only + voxel count
            assert abs(moved["moments"][0] - c64[0]) <= 1e-9 * max(c64[0], 1.0)
            # all ten, in the parent's frame: the exact restatement over the oracle's voxels that were non-empty before and are empty after
            mr.assert_moments(moved["moments"], *mr.emptied_exact(before[1], before[0], o, None, g.voxel_extent), f"moved by split {it}")
            assert int(moved["voxel_count"]) == int(np.count_nonzero((co.export_dense()[2] & 1) == 0))
            cg.close()
            children += 1
    assert outcomes[-1] == 0
    assert children == expect, outcomes
    assert g.count_regions() <= 1


def build(ctx, graph, extent=1.0):
    o = pu.oracle_from_graph(graph, extent)
    g = pu.gpu_from_graph(ctx, graph, extent)
    o.update_occupied_voxel_ranges()
    o.compute_all_derived_state()
    g.compute_all_derived_state()
    pu.assert_derived_equal(o, g)
    return o, g


def test_two_spheres(ctx):
    """extraction.rs:2587-2624 scene: two r=25 spheres 60 apart -> one split, then nothing"""
    o, g = build(ctx, scenes.two_spheres_scene())
    split_all(ctx, o, g, 1)


def test_config3_fracture_into_8(ctx):
    """BASELINE config 3: seven successive split-offs leave 8 objects"""
    o, g = build(ctx, scenes.fracture_scene())
    split_all(ctx, o, g, 7)


def test_small_fragments_repack_and_discard(ctx):
    """a body with small satellites: a 5-voxel-wide blob (repacked into a single chunk when it straddles chunks),
    and a 1-voxel crumb (fewer than 8 voxels: removed, no object)"""
    g = SDFGraph()
    body = g.add_node(SDFNode.new_box((20.0, 20.0, 20.0)))
    acc = body
    for pos, r in (((17.0, 3.0, 2.0), 3.0), ((-17.5, -4.0, 9.0), 2.2), ((2.0, 16.5, -3.0), 0.8)):
        s = g.add_node(SDFNode.new_sphere(r))
        t = g.add_node(SDFNode.new_translation(s, pos))
        acc = g.add_node(SDFNode.new_union(acc, t, 0.0))
    o, gg = build(ctx, g)
    n_o, _ = o.region_labels(False)
    assert n_o == 4
    split_all(ctx, o, gg, 2)


@pytest.mark.parametrize("seed", [0, 1])
def test_random_blobs(ctx, seed):
    """ragged random blobs: many small regions per chunk (exercises the exact local numbering, shared chunks,
    discards and repacks) until a single region is left"""
    rng = np.random.default_rng(seed)
    cc = (2, 2, 3)
    blobs = rng.random((32, 32, 48))
    for ax in range(3):
        blobs = 0.5 * blobs + 0.25 * (np.roll(blobs, 1, ax) + np.roll(blobs, -1, ax))
    sd = np.where(blobs > 0.53, -128, np.where(blobs > 0.5, -40, 60)).astype(np.int8)
    sd[:, :, 22:26] = 90  # a gap that cuts the grid in two
    ty = rng.integers(0, 3, blobs.shape).astype(np.uint8)
    sd_t, ty_t = ol.dense_to_tiled(sd), ol.dense_to_tiled(ty)
    o = ol.OracleObject.from_dense(cc, sd_t, ty_t, 0.5)
    g = VoxelObject.from_dense(ctx, cc, sd_t, ty_t, 0.5)
    o.update_occupied_voxel_ranges()
    o.compute_all_derived_state()
    g.compute_all_derived_state()
    pu.assert_derived_equal(o, g)
    children = 0
    for it in range(400):
        rc_o, co, org_o = o.split_off_smallest_region()
        rc_g, cg, org_g, _ = g.extract_any_disconnected_region()
        assert rc_g == rc_o, it
        if rc_o == 0:
            break
        if rc_o == 1:
            assert org_g == org_o
            if children < 6:
                assert_objects_equal(co, cg, f"child {it}: ")
            children += 1
            cg.close()
    assert_objects_equal(o, g, "final parent: ")
    assert children >= 2


def split_all_at_once(ctx, o, g, expect):
    """`ivx_split_off_all` against the oracle's loop: the same objects in the same order, parent included"""
    want = []
    while True:
        rc_o, co, org_o = o.split_off_smallest_region()
        if rc_o == 0:
            break
        want.append((rc_o, co, org_o))
    got = g.extract_all_disconnected_regions()
    assert [w[0] for w in want] == [x[0] for x in got]
    assert sum(1 for w in want if w[0] == 1) == expect
    assert_objects_equal(o, g, "parent after all split-offs: ")
    for k, ((rc_o, co, org_o), (rc_g, cg, org_g, moved)) in enumerate(zip(want, got)):
        if rc_o == 1:
            assert org_g == org_o, k
            assert_objects_equal(co, cg, f"child {k}: ")
            assert int(moved["voxel_count"]) == int(np.count_nonzero((co.export_dense()[2] & 1) == 0))
            cg.close()
    assert g.count_regions() <= 1
    assert g.extract_all_disconnected_regions() == []


def test_all_split_offs_in_one_call(ctx):
    """config 3 (seven split-offs leave 8 objects), two spheres, and the body with satellites (a repacked blob, a discarded crumb)"""
    o, g = build(ctx, scenes.fracture_scene())
    split_all_at_once(ctx, o, g, 7)
    g.close()
    o, g = build(ctx, scenes.two_spheres_scene())
    split_all_at_once(ctx, o, g, 1)
    g.close()
    gr = SDFGraph()
    acc = gr.add_node(SDFNode.new_box((20.0, 20.0, 20.0)))
    for pos, r in (((17.0, 3.0, 2.0), 3.0), ((-17.5, -4.0, 9.0), 2.2), ((2.0, 16.5, -3.0), 0.8)):
        t = gr.add_node(SDFNode.new_translation(gr.add_node(SDFNode.new_sphere(r)), pos))
        acc = gr.add_node(SDFNode.new_union(acc, t, 0.0))
    o, g = build(ctx, gr)
    split_all_at_once(ctx, o, g, 2)
    g.close()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_all_split_offs_of_random_blobs(ctx, seed):
    """ragged random blobs — many small regions per chunk, chunks shared by several regions that all leave, discards and repacks — in one call"""
    rng = np.random.default_rng(100 + seed)
    cc = (2, 2, 3)
    blobs = rng.random((32, 32, 48))
    for ax in range(3):
        blobs = 0.5 * blobs + 0.25 * (np.roll(blobs, 1, ax) + np.roll(blobs, -1, ax))
    sd = np.where(blobs > 0.53, -128, np.where(blobs > 0.5, -40, 60)).astype(np.int8)
    sd[:, :, 22:26] = 90
    ty = rng.integers(0, 3, blobs.shape).astype(np.uint8)
    sd_t, ty_t = ol.dense_to_tiled(sd), ol.dense_to_tiled(ty)
    o = ol.OracleObject.from_dense(cc, sd_t, ty_t, 0.5)
    g = VoxelObject.from_dense(ctx, cc, sd_t, ty_t, 0.5)
    o.update_occupied_voxel_ranges()
    o.compute_all_derived_state()
    g.compute_all_derived_state()
    n_regions, _ = o.region_labels(False)
    want = []
    while True:
        rc_o, co, org_o = o.split_off_smallest_region()
        if rc_o == 0:
            break
        want.append((rc_o, co, org_o))
    assert len(want) == n_regions - 1
    got = g.extract_all_disconnected_regions()
    assert [w[0] for w in want] == [x[0] for x in got]
    assert_objects_equal(o, g, f"seed {seed} parent: ")
    for k, ((rc_o, co, org_o), (rc_g, cg, org_g, _)) in enumerate(zip(want, got)):
        if rc_o == 1:
            assert org_g == org_o, k
            assert_objects_equal(co, cg, f"seed {seed} child {k}: ")
            cg.close()
    g.close()
