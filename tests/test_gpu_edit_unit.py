"""The host state of an object's edits (csrc/edit_api.hip) across edits, which the parity tests of single edits do not see: the two blocks an
edit's results go through — the accumulators on the device, their host-mapped copy — growing between a small edit and a larger one, a density
table that is not the resident one riding in the device block without ever being read as a later edit's touched words, and a many-object edit
refused in the middle because one of its objects still has an edit in flight. Every case compares an object with a twin that took the same edits
by a route that avoids what the case is about; the edits themselves are checked against the oracle in test_gpu_edit.py.

The blocks are 64 KiB at least and an edit needs 1 120 bytes, 4 per chunk of its box and 16 (the host-mapped copy with early delivery: 32) per
chunk of that box grown by one chunk each way: they grow past the floor only for a box of more than 3 166 chunks, hence the one object of
15 x 15 x 15 chunks here."""
import numpy as np
import pytest

import parity_util as pu
from impact_amd import capi, many, scenes
from impact_amd.voxel import VoxelObject

pytestmark = pytest.mark.gpu

RESULT_FIELDS = ("removed_moments", "emptied_by_type", "emptied_voxels", "touched_chunks", "removed_chunks", "invalidated")


def derived(ctx, graph):
    g = pu.gpu_from_graph(ctx, graph)
    g.compute_all_derived_state()
    g.update_occupied_voxel_ranges()
    return g


def assert_results_equal(a, b, what, fields=RESULT_FIELDS):
    for f in fields:
        if f in a or f in b:
            np.testing.assert_array_equal(np.asarray(a[f]), np.asarray(b[f]), err_msg=f"{what}: {f}")


def assert_voxels_equal(a, b, what):
    for x, y, plane in zip(a.download(flags=False, labels=False, info=False), b.download(flags=False, labels=False, info=False), ("sdf", "types")):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {plane}")


@pytest.mark.parametrize("early", [False, True])
def test_blocks_grow_between_a_small_edit_and_a_larger_one(ctx, early):
    """`twin`: first an edit whose influence covers all 3 375 chunks from 500 voxels outside (sphere radius 0: no voxel leaves, the distances
    in its influence are quantised again), so that its blocks have their final sizes. `g`: a new object with the twin's voxels as they are then,
    and no edit behind it. Both then take a bite that touches a few chunks (g's blocks at their floor) and a cavity whose influence covers
    every chunk (g's blocks both outgrown): the same results, the same voxels."""
    twin = derived(ctx, scenes.box_scene((232.0, 232.0, 232.0)))
    assert twin.chunk_counts == (15, 15, 15)
    r0 = twin.absorb_sphere((-500.0, 120.0, 120.0), 2000.0, 0.0)
    assert r0["emptied_voxels"] == 0 and r0["removed_chunks"] == 0 and r0["touched_chunks"] == 3375
    sdf, types = twin.download(flags=False, labels=False, info=False)[:2]
    g = VoxelObject.from_dense(ctx, twin.chunk_counts, sdf, types)
    g.compute_all_derived_state()
    g.update_occupied_voxel_ranges()
    assert g.occupied_voxel_ranges == twin.update_occupied_voxel_ranges()
    for o in (g, twin):
        o.set_early_mesh_needs(early)
    bite = ((30.0, 30.0, 30.5), 7.0, 5.0)
    cavity = ((120.0, 119.5, 120.0), 400.0, 50.0)
    # (the bite with a density table that is not g's resident one: it rides in the last kilobyte of the block that the cavity then outgrows;
    # the twin has it as its resident table for the bite)
    foreign = np.linspace(0.5, 3.0, 256, dtype=np.float32)
    g.set_densities(np.ones(256, dtype=np.float32))
    twin.set_densities(foreign)
    small, small_twin = g.absorb_sphere(*bite, densities=foreign), twin.absorb_sphere(*bite, densities=foreign)
    twin.set_densities(np.ones(256, dtype=np.float32))
    assert 0 < small["emptied_voxels"] < 1000 and 0 < np.count_nonzero(small["invalidated"]) <= 8
    assert_results_equal(small, small_twin, "bite")
    large, large_twin = g.absorb_sphere(*cavity), twin.absorb_sphere(*cavity)
    assert large["emptied_voxels"] > 400000 and large["touched_chunks"] == 3375
    assert_results_equal(large, large_twin, "cavity")
    assert_voxels_equal(g, twin, "after the cavity")
    assert g.count_regions() == twin.count_regions() == 1
    g.close()
    twin.close()


def test_a_foreign_density_table_is_never_a_later_edits_touched_words(ctx):
    """An edit with a density table that is not the resident one puts it into the device block; a later, larger edit of the same object must
    not find its floats where the touched words of its chunks go (1.0f reads as "touched": chunks invalidated for nothing). The sizes: the
    bite's box is one chunk, its grown box eight, so its results end at byte 1 264 and a table "right behind them" would lie at bytes 1 280 to
    2 304; the hollow's box holds all 64 chunks of the object, touched words at bytes 1 120 to 1 376, the last 24 of them — the chunks
    (2, 2..3, *) and (3, *, *) — where the table's first floats would be; its influence (18 voxels about the middle) reaches neither
    the chunks at the corners nor those along the edges. The twin takes the same edits with the same tables, each made the resident one
    first, and so never puts a table into the block."""
    rng = np.random.default_rng(11)
    resident, foreign = np.ones(256, dtype=np.float32), rng.uniform(0.5, 3.0, 256).astype(np.float32)
    foreign[:64] = 1.0  # (the floats that would read as touched words)
    graph = scenes.box_scene((56.0, 56.0, 56.0))
    g, twin = derived(ctx, graph), derived(ctx, graph)
    assert g.chunk_counts == (4, 4, 4)
    g.set_densities(resident)
    bite = ((8.0, 8.0, 8.5), 6.0, 4.0)         # one chunk, the lowest corner
    hollow = ((32.0, 32.0, 32.5), 18.0, 16.0)  # all 64 chunks in its box; the corners and the edges outside its influence
    twin.set_densities(foreign)
    small, small_twin = g.absorb_sphere(*bite, densities=foreign), twin.absorb_sphere(*bite, densities=foreign)
    assert small["emptied_voxels"] > 0 and small["touched_chunks"] == 1
    assert_results_equal(small, small_twin, "bite with a foreign table")
    twin.set_densities(resident)
    large, large_twin = g.absorb_sphere(*hollow, densities=resident), twin.absorb_sphere(*hollow, densities=resident)
    inv = large["invalidated"].reshape(4, 4, 4)
    print(f"hollow: touched {large['touched_chunks']}, invalidated {np.count_nonzero(inv)} (twin {np.count_nonzero(large_twin['invalidated'])})")
    assert large["emptied_voxels"] > 0 and 8 <= large["touched_chunks"] < 64 and not inv[::3, ::3, ::3].any()
    assert_results_equal(large, large_twin, "hollow behind a foreign table")
    assert_voxels_equal(g, twin, "after the hollow")
    g.close()
    twin.close()


def test_a_batch_refused_for_an_edit_in_flight_leaves_every_object_usable(ctx):
    """`ivx_absorb_sphere_many` over four objects, the third with an edit of its own still in flight: the call fails with that object's message;
    the edits of the two objects before it ran and their results were discarded, the one in flight was collected the same way. Afterwards every
    object takes and completes a single edit; its results and voxels are those of a twin that took the same edits one call at a time."""
    graphs = [scenes.sphere_scene(12.0 + 2.0 * k) for k in range(4)]  # 2 x 2 x 2 and 3 x 3 x 3 chunks
    gs, twins = [derived(ctx, gr) for gr in graphs], [derived(ctx, gr) for gr in graphs]
    ctr = [np.array([0.5 * (lo + hi) for lo, hi in g.occupied_voxel_ranges], dtype=np.float32) for g in gs]
    top = [c + np.array([0.0, 0.5 * (g.occupied_voxel_ranges[1][1] - g.occupied_voxel_ranges[1][0]), 0.0], dtype=np.float32) for c, g in zip(ctr, gs)]
    gs[2].absorb_sphere_enqueue(top[2], 6.0, 4.0)
    with pytest.raises(capi.IvxError, match=r"ivx_absorb_sphere_many: an edit of this object is in flight \(ivx_absorb_collect first\)") as e:
        many.absorb_sphere_many(gs, ctr, [5.0] * 4, [3.0] * 4)
    assert e.value.code == capi.IVX_ERR_STATE
    with pytest.raises(capi.IvxError, match="ivx_absorb_collect: no edit of this object is in flight"):
        gs[2].absorb_collect()  # (given up with the batch)
    for k in (0, 1):
        twins[k].absorb_sphere(ctr[k], 5.0, 3.0)
    twins[2].absorb_sphere(top[2], 6.0, 4.0)
    for k, (g, twin) in enumerate(zip(gs, twins)):
        g.absorb_sphere_enqueue(top[k], 7.0, 5.0)
        r, want = g.absorb_collect(), twin.absorb_sphere(top[k], 7.0, 5.0)
        assert r["emptied_voxels"] > 0
        assert_results_equal(r, want, f"object {k} after the failed batch")
        assert_voxels_equal(g, twin, f"object {k} after the failed batch")
        assert g.count_regions() == twin.count_regions()
    for o in gs + twins:
        o.close()
