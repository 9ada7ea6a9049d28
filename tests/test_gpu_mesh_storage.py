"""Where the mesh arrays live and how they grow (csrc/mesh_api.hip), as a renderer sees it through `VoxelObjectMesh.export`: the capacities after a
full rebuild (`create`, the step, the pooled first mesh of objects stepped together) and after a sync that outgrew them, the parts of a pooled
block, and the state of a sync in flight on an object that was never edited.

The two growth rules, written out: a rebuild gives a group max(2 n + slack, 2 cap) elements, a growth that keeps the mesh max(n + n // 2 + slack,
2 cap); slack 4096 per vertex, 24576 per index, 64 per submesh. Bytes per element: positions 12, normals 12, indices 4, index materials 8,
submeshes `SUBMESH_DTYPE.itemsize` (and 16 of scratch per vertex, which nobody exports)."""
import os

import numpy as np
import pytest

import oracle_lib as ol
import parity_util as pu
from impact_amd import capi, many, scenes
from impact_amd.voxel import VoxelObjectMesh
from test_gpu_mesh_sync import assert_synced_meshes_equal, both

pytestmark = pytest.mark.gpu

BUFFERS = VoxelObjectMesh.MESH_BUFFERS
ELEM = {"positions": 12, "normals": 12, "indices": 4, "index_materials": 8, "submeshes": capi.SUBMESH_DTYPE.itemsize}
GROUP = {"positions": 0, "normals": 0, "indices": 1, "index_materials": 1, "submeshes": 2}  # counted per vertex, per index, per submesh
SLACK = (4096, 24576, 64)
SCRATCH_PER_VERTEX = 16
NO_SAMPLE = capi.STAGE_ALL & ~capi.STAGE_SAMPLE


def rebuilt(n, cap=(0, 0, 0)):
    return [max(2 * n[k] + SLACK[k], 2 * cap[k]) for k in range(3)]


def grown_keeping(n, cap):
    return [max(n[k] + n[k] // 2 + SLACK[k], 2 * cap[k]) for k in range(3)]


def counts(gm):
    return [gm.n_vertices(), gm.n_indices(), gm.n_chunks()]


def exported(gm):
    """name -> (capacity in bytes, device address) of the five buffers"""
    out = {}
    for name in BUFFERS:
        e = gm.export(name)
        if e["dmabuf_fd"] >= 0:
            os.close(e["dmabuf_fd"])
        assert e["element_bytes"] == ELEM[name]
        out[name] = (e["capacity_bytes"], e["device_ptr"])
    return out


def capacities(ex):
    """elements per group from what `exported` returned (the two arrays of a group agree)"""
    assert ex["positions"][0] // 12 == ex["normals"][0] // 12 and ex["indices"][0] // 4 == ex["index_materials"][0] // 8
    return [ex["positions"][0] // 12, ex["indices"][0] // 4, ex["submeshes"][0] // ELEM["submeshes"]]


def assert_capacities(ex, cap, what=""):
    for name in BUFFERS:
        print(f"{what}{name}: capacity_bytes {ex[name][0]}, expected {cap[GROUP[name]] * ELEM[name]}")
        assert ex[name][0] == cap[GROUP[name]] * ELEM[name], (what, name)


def assert_meshes_identical(a, b, what=""):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8), err_msg=what)


def mesh_of_step(g, res):
    gm = VoxelObjectMesh(g)
    gm.counts = res["mesh"].copy()
    return gm


SPHERE_32 = scenes.sphere_scene(14.0)  # 2 x 2 x 2 chunks
# 1, 1 x 2 x 3, 8 and 27 chunks; the last is the solid box of the keep test: 48 voxels of grid, the surface at voxels 1 and 41
POOLED = [scenes.box_scene((10.0, 10.0, 10.0)), scenes.box_scene((12.0, 28.0, 44.0)), SPHERE_32, scenes.box_scene((40.0, 40.0, 40.0))]
POOLED_CHUNKS = [(1, 1, 1), (1, 2, 3), (2, 2, 2), (3, 3, 3)]
BOX = 3  # its place in POOLED
# Cavities about the box's centre, each wider than the one before: every sync re-meshes the chunks around the cavity, whose meshes no longer fit
# the ranges they had and go to the end of the buffers. The oracle's buffer lengths along this sequence (n0 = 10 586 vertices, 57 600 indices
# after the rebuild, so 25 268 and 139 776 of capacity): 12 307 / 66 240, 16 427 / 78 696, 19 156 / 96 666, 21 495 / 108 732, 23 157 / 117 336,
# 23 752 / 123 522, 25 565 / 132 978 (the vertices outgrow), 26 298 / 146 814 (the indices outgrow). Radius 16 + 2 of influence about voxel 21
# stays inside the surface at voxels 1 and 41.
CAVITY_CENTER = (21.0, 21.0, 21.0)
CAVITY_RADII = (6.0, 8.0, 10.0, 12.0, 13.0, 14.0, 15.0, 16.0)


def test_rebuild_rule_and_a_rebuild_that_fits(ctx):
    g = pu.gpu_from_graph(ctx, SPHERE_32)
    assert g.chunk_counts == (2, 2, 2)
    g.compute_all_derived_state()
    gm = VoxelObjectMesh.create(g)
    ex = exported(gm)
    assert_capacities(ex, rebuilt(counts(gm)), "create: ")
    gen, first = gm.generation(), gm.download()
    gm.recreate()
    assert gm.generation() == gen
    assert exported(gm) == ex
    assert_meshes_identical(gm.download(), first)
    g.close()


def test_step_path_gives_the_same_capacities_and_mesh(ctx):
    twin = pu.gpu_from_graph(ctx, SPHERE_32)
    twin.compute_all_derived_state()
    want = VoxelObjectMesh.create(twin)
    g = pu.gpu_from_graph(ctx, SPHERE_32)
    gm = mesh_of_step(g, g.step(capi.STAGE_DERIVE | capi.STAGE_OCCUPIED | capi.STAGE_REGIONS | capi.STAGE_REMESH))
    assert counts(gm) == counts(want)
    assert_capacities(exported(gm), rebuilt(counts(gm)), "step: ")
    assert capacities(exported(gm)) == capacities(exported(want))
    assert_meshes_identical(gm.download(), want.download())
    g.close()
    twin.close()


def pooled_first_meshes(ctx):
    """the POOLED objects through one `voxel_step_many` from no mesh: (objects, meshes)"""
    gs = [pu.gpu_from_graph(ctx, graph) for graph in POOLED]
    assert [g.chunk_counts for g in gs] == POOLED_CHUNKS
    for g in gs:
        g.set_densities(np.ones(256, dtype=np.float32))
    res = many.voxel_step_many(gs, NO_SAMPLE)
    return gs, [mesh_of_step(g, r) for g, r in zip(gs, res)]


def test_pooled_first_mesh(ctx):
    gs, gms = pooled_first_meshes(ctx)
    ranges, meshes = [], []
    for k, (graph, gm) in enumerate(zip(POOLED, gms)):
        ex = exported(gm)
        cap = rebuilt(counts(gm))
        assert_capacities(ex, cap, f"object {k}: ")
        for name in BUFFERS:
            assert ex[name][1] % 256 == 0, (k, name)
            ranges.append((ex[name][1], ex[name][1] + ex[name][0], k, name))
        # the vertex scratch has no handle: its part lies between the normals and the indices
        scratch = ex["normals"][1] + ((ex["normals"][0] + 255) & ~255)
        ranges.append((scratch, scratch + cap[0] * SCRATCH_PER_VERTEX, k, "vertex scratch"))
        twin = pu.gpu_from_graph(ctx, graph)
        twin.compute_all_derived_state()
        assert_meshes_identical(gm.download(), VoxelObjectMesh.create(twin).download(), f"object {k}")
        twin.close()
        meshes.append(gm.download())
    assert len(ranges) == 24
    ranges.sort()
    for a, b in zip(ranges, ranges[1:]):
        assert a[1] <= b[0], (a, b)
    # one block: the parts in the order positions, normals, vertex scratch, indices, index materials, submeshes, object after object
    assert [(r[2], r[3]) for r in ranges] == [(k, name) for k in range(4) for name in ("positions", "normals", "vertex scratch", "indices", "index_materials", "submeshes")]
    assert ranges[-1][1] - ranges[0][0] < sum(((r[1] - r[0] + 255) & ~255) for r in ranges) + 256
    gs[0].close()
    gs[2].close()
    for k in (1, 3):  # the block outlives its first holders
        assert_meshes_identical(gms[k].download(), meshes[k], f"object {k} after two of four are gone")
    gs[1].close()
    gs[3].close()


def carve_until_outgrown(o, g, om, gm, stop_at_first=False):
    """the cavity sequence, edit -> sync -> compare with the oracle -> check the capacities; returns the groups that grew, per sync"""
    grew_at = []
    for radius in CAVITY_RADII:
        before, gen = exported(gm), gm.generation()
        cap = capacities(before)
        c = np.asarray(CAVITY_CENTER, dtype=np.float32)
        ro, rg = o.absorb_sphere(c, radius + 2.0, radius), g.absorb_sphere(c, radius + 2.0, radius)
        np.testing.assert_array_equal(rg["invalidated"], ro["invalidated"])
        om.sync(ro["invalidated"])
        gm.sync_with_voxel_object(rg["invalidated"])
        assert_synced_meshes_equal(om.get(), gm.download())
        n, after = counts(gm), exported(gm)
        grew = [n[k] > cap[k] for k in range(3)]
        kept = grown_keeping(n, cap)
        print(f"radius {radius}: counts {n}, capacities {cap} -> {capacities(after)}, generation {gen} -> {gm.generation()}")
        assert_capacities(after, [kept[k] if grew[k] else cap[k] for k in range(3)], f"radius {radius}: ")
        for name in BUFFERS:
            if not grew[GROUP[name]]:
                assert after[name] == before[name], (radius, name)
        assert (gm.generation() != gen) == any(grew)
        grew_at.append(grew)
        if stop_at_first and any(grew):
            break
    return grew_at


def test_growth_that_keeps(ctx):
    o, g = both(ctx, POOLED[BOX])
    om, gm = ol.OracleMeshHandle(o), VoxelObjectMesh.create(g)
    first = om.get()
    n0 = [len(first.positions), len(first.indices), len(first.submeshes)]
    assert n0[:2] == [10586, 57600]
    assert capacities(exported(gm)) == rebuilt(n0)
    grew_at = carve_until_outgrown(o, g, om, gm)
    last = om.get()  # (the oracle's own lengths: the sequence passes both bounds whatever the code under test does)
    assert len(last.positions) > 2 * n0[0] + SLACK[0] and len(last.indices) > 2 * n0[1] + SLACK[1]
    assert any(w[0] for w in grew_at) and any(w[1] for w in grew_at) and not any(w[2] for w in grew_at)
    g.close()
    # the same on the object that shares a pooled block: its vertex group moves out, the other parts and the siblings stay
    gs, gms = pooled_first_meshes(ctx)
    siblings = [k for k in range(4) if k != BOX]
    before = {k: (exported(gms[k]), gms[k].download()) for k in siblings}
    o = pu.oracle_from_graph(POOLED[BOX])
    o.update_occupied_voxel_ranges()
    o.compute_all_derived_state()
    grew_at = carve_until_outgrown(o, gs[BOX], ol.OracleMeshHandle(o), gms[BOX], stop_at_first=True)
    assert grew_at[-1] == [True, False, False]
    for k in siblings:
        assert exported(gms[k]) == before[k][0]
        assert_meshes_identical(gms[k].download(), before[k][1], f"sibling {k}")
    for k in (BOX, 0, 2, 1):
        gs[k].close()
    ctx.synchronize()


def test_sync_state_without_an_edit(ctx):
    o, g = both(ctx, SPHERE_32)
    om, gm = ol.OracleMeshHandle(o), VoxelObjectMesh.create(g)
    with pytest.raises(capi.IvxError, match="ivx_mesh_sync_collect: no sync of this object is in flight") as e:
        gm.sync_collect()  # never edited, never synced
    assert e.value.code == capi.IVX_ERR_STATE
    inv = np.zeros(g.n_chunks, dtype=np.uint8)
    inv[3] = 1
    gm.sync_enqueue(inv)
    with pytest.raises(capi.IvxError, match=r"ivx_mesh_sync_enqueue: a sync of this object is in flight \(ivx_mesh_sync_collect first\)") as e:
        gm.sync_enqueue(inv)
    assert e.value.code == capi.IVX_ERR_STATE
    gm.sync_collect()
    om.sync(inv.astype(bool))
    assert_synced_meshes_equal(om.get(), gm.download())
    g.close()
    # a batched sync that fails in the middle (an object without a mesh): the objects enqueued before it are not left in flight
    pairs = [both(ctx, scenes.sphere_scene(10.0 + 2.0 * k)) for k in range(4)]
    oms = [ol.OracleMeshHandle(po) for po, _ in pairs]
    gms = [VoxelObjectMesh.create(pg) if k != 2 else VoxelObjectMesh(pg) for k, (_, pg) in enumerate(pairs)]
    invs = []
    for _, pg in pairs:
        a = np.zeros(pg.n_chunks, dtype=np.uint8)
        a[0] = 1
        invs.append(a)
    with pytest.raises(capi.IvxError, match="there is no mesh to synchronise"):
        many.mesh_sync_many(gms, invs)
    for k in (0, 1):  # their syncs ran before the call failed
        oms[k].sync(invs[k].astype(bool))
    for k in (0, 1, 3):
        gms[k].sync_enqueue(invs[k])
        gms[k].sync_collect()
        oms[k].sync(invs[k].astype(bool))
        assert_synced_meshes_equal(oms[k].get(), gms[k].download())
    # ... and the same behind a batched edit that fails in the middle
    gs = [pg for _, pg in pairs]
    ctr = [np.array([0.5 * (lo + hi) for lo, hi in po.info()["occupied_voxel_ranges"]], dtype=np.float32) for po, _ in pairs]
    with pytest.raises(capi.IvxError):
        many.absorb_sphere_many(gs, ctr, [5.0, 5.0, -1.0, 5.0], [3.0] * 4)
    for k in (0, 1):  # (their edits, cavities about the centre, ran before the call failed; the results were discarded)
        pairs[k][0].absorb_sphere(ctr[k], 5.0, 3.0)
    for k in (0, 1, 3):
        gms[k].sync_enqueue(invs[k])
        gms[k].sync_collect()
        oms[k].sync(invs[k].astype(bool))
        assert_synced_meshes_equal(oms[k].get(), gms[k].download())
    for pg in gs:
        pg.close()
