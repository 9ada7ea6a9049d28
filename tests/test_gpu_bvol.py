"""Bounding volumes on the device (impact_amd/csrc/bvol.hip). The derivation: device world boxes byte-equal to the library's host function. The
decisions: every expectation is the float32 restatement of bvol_ref.py over the DOWNLOADED world boxes, and pair lists (content and order),
masks, zero tail bits and counts must be equal to it — no tolerance anywhere in this file.

The pair walk owns 64 rows x one segment of 512 columns per wave, and its scan runs in rounds of 1 024 rows: the sizes below sit one below, at and
one above each."""
import ctypes as C

import numpy as np
import pytest

import bvol_ref as br
import parity_util as pu
from impact_amd import bvol, capi, many, scenes
from impact_amd.voxel import Context, VoxelObjectMesh

pytestmark = pytest.mark.gpu

SEGMENT_WIDTH, SCAN_ROUND = 512, 1024
SIZES = [0, 1, 2, 3, 63, 64, 65, 200, SEGMENT_WIDTH - 1, SEGMENT_WIDTH, SEGMENT_WIDTH + 1, SCAN_ROUND - 1, SCAN_ROUND, 1025, 4161]
assert SCAN_ROUND + 1 == 1025


def assert_pairs_equal(got, want, what=""):
    assert got.dtype == np.uint32 and got.shape == want.shape, (what, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got != want).any(axis=1))[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} pairs differ, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}")


def test_device_world_boxes_equal_the_host_function(ctx):
    """the CPU test's 400 seeded cases: byte-equal to ivx_bv_world_aabb's; boxes given without similarities come back as the given bytes, a NaN
    and signed zeros included; the total is the box around them"""
    boxes, sims = br.seeded_derivation_cases(400, 21)
    s = bvol.set_boxes(ctx, boxes, sims)
    world, total = s.download()
    want = br.host_world_boxes(boxes, sims)
    assert world.tobytes() == want.tobytes()
    assert total["lower"].tolist() == want["lower"].min(axis=0).tolist() and total["upper"].tolist() == want["upper"].max(axis=0).tolist()
    given = boxes.copy()
    given["lower"][5], given["upper"][6] = (-0.0, 0.0, -0.0), (np.nan, 1.0, 2.0)
    world, total = bvol.set_boxes(ctx, given).download()
    assert world.tobytes() == given.tobytes()
    sound = np.delete(given, 6)  # (a box with a NaN bound intersects nothing and stays out of the total)
    assert total["lower"].tolist() == sound["lower"].min(axis=0).tolist() and total["upper"].tolist() == sound["upper"].max(axis=0).tolist()
    assert s.device_ptr(capi.BV_PTR_WORLD_BOXES)


@pytest.mark.parametrize("mode", [capi.BV_ALL_PAIRS, capi.BV_DYNAMIC_PAIRS])
@pytest.mark.parametrize("n", SIZES)
def test_pairs_of_the_seeded_scene(ctx, n, mode):
    """bvol_ref.scene(n), seed 11, kinds drawn 60 / 30 / 10 %: the pair list equals the restatement's over the downloaded boxes in content and order"""
    world, kinds = br.scene(n)
    s = bvol.set_boxes(ctx, world, None, kinds)
    got_world, _ = s.download()
    assert got_world.tobytes() == world.tobytes()
    want, touching = br.scene_pairs(n, mode)
    if n >= 63:  # the case can show something
        all_pairs, all_touching = br.scene_pairs(n, capi.BV_ALL_PAIRS)
        assert n <= len(all_pairs) <= n * (n - 1) // 8 and all_touching.sum() * 10 >= len(all_pairs)
        assert len(want) > 0 and (mode == capi.BV_ALL_PAIRS or len(want) < len(all_pairs))
    got = s.pairs(mode, capacity=len(want))
    assert_pairs_equal(got, want, f"n {n} mode {mode}")


def test_pairs_hand_made_cases(ctx):
    # the sign bit of the difference: a.upper = -0.0 against b.lower = +0.0 is outside, +0.0 against +0.0 intersects
    for upper, expected in ((-0.0, []), (0.0, [[0, 1]])):
        world = bvol.boxes([(-1, 0, 0), (0.0, 0, 0)], [(upper, 1, 1), (1, 1, 1)])
        s = bvol.set_boxes(ctx, world)
        assert np.signbit(s.download()[0]["upper"][0][0]) == np.signbit(np.float32(upper))
        assert s.pairs().tolist() == expected == br.pairs(world)[0].tolist()
    # identical boxes: every pair
    n = 70
    world = bvol.boxes([(1, 2, 3)] * n, [(2, 3, 4)] * n)
    assert_pairs_equal(bvol.set_boxes(ctx, world).pairs(), br.pairs(world)[0], "identical")
    # one box containing all the others, which are disjoint: a full row, at the front, in the middle and at the end
    rng = np.random.default_rng(2)
    n = 150
    small = np.stack([np.arange(n) * 2.0, rng.uniform(0, 5, n), rng.uniform(0, 5, n)], axis=1)
    for at in (0, 77, n - 1):
        world = bvol.boxes(small, small + 1.0)
        world["lower"][at], world["upper"][at] = (-1, -1, -1), (2 * n + 1, 7, 7)
        want = br.pairs(world)[0]
        assert len(want) == n - 1
        assert_pairs_equal(bvol.set_boxes(ctx, world).pairs(), want, f"full row {at}")
    # all disjoint: no pair (and no emit)
    world = bvol.boxes(small, small + 1.0)
    found = C.c_size_t(5)
    bvol.set_boxes(ctx, world)
    capi.check(capi.lib().ivx_bv_pairs(ctx.h, 0, None, 0, C.byref(found)))
    assert found.value == 0
    # 200 boxes, every pair intersecting
    n = 200
    c = rng.uniform(0, 0.25, (n, 3))
    world = bvol.boxes(c - 1.0, c + 1.0)
    got = bvol.set_boxes(ctx, world).pairs()
    assert len(got) == 19900
    assert_pairs_equal(got, np.array([(a, b) for a in range(n) for b in range(a + 1, n)], dtype=np.uint32), "all pairs")
    # a box with a NaN bound intersects nothing, by the restatement and on the device
    world = bvol.boxes([(0, 0, 0)] * 3, [(1, 1, 1)] * 3)
    world["upper"][1][2] = np.nan
    assert bvol.set_boxes(ctx, world).pairs().tolist() == [[0, 2]] == br.pairs(world)[0].tolist()


def test_pairs_capacity_and_repetition(ctx):
    lib = capi.lib()
    world, kinds = br.scene(1025)
    want = br.scene_pairs(1025, capi.BV_ALL_PAIRS)[0]
    s = bvol.set_boxes(ctx, world, None, kinds)
    # one short: IVX_ERR_CAPACITY, the number found, the buffer untouched
    out = np.full((len(want), 2), 0xA5A5A5A5, dtype=np.uint32)
    found = C.c_size_t(0)
    assert lib.ivx_bv_pairs(ctx.h, 0, capi.ptr(out), len(want) - 1, C.byref(found)) == capi.IVX_ERR_CAPACITY
    assert found.value == len(want) and np.all(out == 0xA5A5A5A5)
    # two calls leave the same bytes
    first, second = s.pairs(0, capacity=len(want)), s.pairs(0, capacity=len(want) + 10)
    assert_pairs_equal(first, want, "first")
    assert first.tobytes() == second.tobytes()
    assert s.device_ptr(capi.BV_PTR_PAIRS)
    # a smaller set after a larger one: nothing stale
    small_world, small_kinds = br.scene(65)
    s = bvol.set_boxes(ctx, small_world, None, small_kinds)
    for mode in (0, 1):
        assert_pairs_equal(s.pairs(mode), br.scene_pairs(65, mode)[0], f"smaller set, mode {mode}")
    assert s.download()[0].tobytes() == small_world.tobytes()


@pytest.mark.parametrize("n", [4, 6])
def test_pairs_of_the_pile_in_lattice_order(ctx, n):
    """scenes.sphere_pile_scene: the spheres' boxes in the scene's own (coherent) order — the pair count is the lattice's 26-neighbour half count,
    and the pairs whose centres are closer than 2 r are the scene's 6-neighbour pair list, in the scene's own (a, b) order"""
    bodies, contacts = scenes.sphere_pile_scene(n=n)
    pos, r = bodies["position"].astype(np.float32), np.float32(0.5)
    s = bvol.set_boxes(ctx, bvol.boxes(pos - r, pos + r))
    world, _ = s.download()
    got = s.pairs()
    assert len(got) == ((3 * n - 2) ** 3 - n ** 3) // 2
    assert_pairs_equal(got, br.pairs(world)[0], f"pile {n}")
    d = np.linalg.norm(pos[got[:, 0]].astype(np.float64) - pos[got[:, 1]].astype(np.float64), axis=1)
    scene_pairs = np.stack([contacts["body_a"][::4], contacts["body_b"][::4]], axis=1).astype(np.uint32)
    assert len(scene_pairs) == 3 * n * n * (n - 1)
    assert_pairs_equal(np.ascontiguousarray(got[d < 2.0 * 0.5]), scene_pairs, "6-neighbours")


def boundary_queries(world):
    """one query of each kind with a face of object 0's box exactly on its boundary (the scene's coordinates are multiples of 1/8: exact)"""
    lo, hi = world["lower"][0].astype(np.float64), world["upper"][0].astype(np.float64)
    mid = 0.5 * (lo + hi)
    far = [[0, 1, 0, -1000], [0, -1, 0, -1000], [0, 0, 1, -1000], [0, 0, -1, -1000], [-1, 0, 0, -1000]]
    return bvol.query_array([bvol.box_query((hi[0], lo[1], lo[2]), (hi[0] + 1.0, hi[1], hi[2])),
                             bvol.sphere_query((hi[0] + 0.5, mid[1], mid[2]), 0.5),
                             bvol.frustum_query([[1, 0, 0, hi[0]]] + far),
                             bvol.oriented_box_query((hi[0] + 0.75, mid[1], mid[2]), (0, 0, 0, 1), (0.75, 0.125, 0.125))])


@pytest.mark.parametrize("n_queries", [1, 2, 67])
@pytest.mark.parametrize("n", [1, 64, 65, 1025])
def test_queries_of_mixed_kinds(ctx, n, n_queries):
    """the seeded scene against bvol_ref.mixed_queries (kind = index % 4): masks, zero tail bits and counts equal the restatement's over the
    downloaded boxes. From 64 objects on every query hits at least a tenth of the objects and misses a tenth (one object can only be hit or missed)"""
    world, kinds = br.scene(n)
    s = bvol.set_boxes(ctx, world, None, kinds)
    got_world, _ = s.download()
    records = br.mixed_queries(n, n_queries)
    want_masks, want_counts = br.queries(got_world, records)
    if n >= 64:
        assert np.all(want_counts >= 0.1 * n) and np.all(want_counts <= 0.9 * n), want_counts
    masks, counts = s.query(records)
    assert masks.shape == (n_queries, (n + 63) // 64) and masks.tobytes() == want_masks.tobytes()
    assert counts.tolist() == want_counts.tolist()
    if n % 64:
        assert not (masks[:, -1] >> np.uint64(n % 64)).any()
    assert [m.tolist() for m in bvol.mask_indices(masks, n)] == [np.nonzero(br.query_hits(got_world, q))[0].tolist() for q in records]


def test_queries_touching_their_boundary_and_repetition(ctx):
    world, kinds = br.scene(65)
    s = bvol.set_boxes(ctx, world, None, kinds)
    records = boundary_queries(world)
    assert records["kind"].tolist() == [0, 1, 2, 3]
    want_masks, want_counts = br.queries(world, records)
    assert np.all(want_masks[:, 0] & np.uint64(1)), "the restatement counts a touching face as a hit"
    masks, counts = s.query(records)
    assert masks.tobytes() == want_masks.tobytes() and counts.tolist() == want_counts.tolist()
    assert np.all(masks[:, 0] & np.uint64(1))
    again = s.query(records)
    assert again[0].tobytes() == masks.tobytes() and again[1].tobytes() == counts.tobytes()
    assert s.device_ptr(capi.BV_PTR_MASKS)
    # NaN: a miss for the box, the frustum and the oriented box, a hit for the sphere (its comparisons are false)
    nan_world = bvol.boxes([(0, 0, 0), (np.nan, 0, 0)], [(1, 1, 1), (1, 1, 1)])
    s = bvol.set_boxes(ctx, nan_world)
    everything = bvol.query_array([bvol.box_query((-9, -9, -9), (9, 9, 9)), bvol.sphere_query((0.5, 0.5, 0.5), 0.25),
                                   bvol.frustum_query([[1, 0, 0, -9], [-1, 0, 0, -9], [0, 1, 0, -9], [0, -1, 0, -9], [0, 0, 1, -9], [0, 0, -1, -9]]),
                                   bvol.oriented_box_query((0, 0, 0), (0, 0, 0, 1), (9, 9, 9))])
    masks, counts = s.query(everything)
    assert masks[:, 0].tolist() == [1, 3, 1, 1] == br.queries(nan_world, everything)[0][:, 0].tolist() and counts.tolist() == [1, 2, 1, 1]


def box_object(ctx, extents=(30.0, 30.0, 30.0), voxel_extent=1.0, probes=True):
    g = pu.gpu_from_graph(ctx, scenes.box_scene(extents), voxel_extent)
    g.compute_all_derived_state()
    g.update_occupied_voxel_ranges()
    if probes:
        g.mesh = VoxelObjectMesh.create(g)
        g.collision_probes_recompute()
    return g


def expected_model_box(g):
    ranges = g.update_occupied_voxel_ranges()
    e = np.float32(g.voxel_extent)
    return [np.float32(r[0]) * e for r in ranges], [np.float32(r[1]) * e for r in ranges]


def test_voxel_objects(ctx):
    """three config-1 boxes (32^3 grids), two overlapping and one apart: set_grids -> pairs gives exactly the overlapping pair, whose mutual
    contacts exist while the pair not found has none; ivx_grid_model_aabb follows the occupied ranges through a clip and an absorbing sphere; the
    same set inside an ivx_many_begin bracket behind a recorded edit"""
    lib = capi.lib()
    gs = [box_object(ctx) for _ in range(3)]
    assert all(g.chunk_counts == (2, 2, 2) for g in gs)
    offsets = np.array([(0, 0, 0), (28, 0, 0), (100, 0, 0)], dtype=np.float32)
    sims = bvol.similarities(3)
    sims["translation"] = offsets
    for g in gs:
        box = bvol.grid_model_aabb(g)
        lo, hi = expected_model_box(g)
        assert box["lower"].tolist() == lo and box["upper"].tolist() == hi
        assert 0.0 <= lo[0] <= 2.0 and 30.0 <= hi[0] <= 32.0  # (a 30^3 box in a 32^3 grid)
    lo, hi = np.array(lo, dtype=np.float32), np.array(hi, dtype=np.float32)
    s = bvol.set_grids(gs, sims)
    world, total = s.download()
    assert world["lower"].tolist() == (offsets + lo).tolist() and world["upper"].tolist() == (offsets + hi).tolist()  # (small integers: exact)
    assert total["lower"].tolist() == lo.tolist() and total["upper"].tolist() == (offsets[2] + hi).tolist()
    plain = s.pairs()
    assert plain.tolist() == [[0, 1]] == br.pairs(world)[0].tolist()

    def mutual(a, b):
        com = np.array([16.0, 16.0, 16.0], dtype=np.float32)
        ident = np.array([0, 0, 0, 1], dtype=np.float32)
        q = many.mutual_queries([dict(a=gs[a], b=gs[b], rotation_a=ident, translation_a=-offsets[a], center_of_mass_a=com, rotation_b=ident,
                                      translation_b=-offsets[b], center_of_mass_b=com, collidable_id_a=10 + a, collidable_id_b=10 + b, body_a=a, body_b=b)])
        return many.mutual_voxel_object_contacts_many(q)[0]

    assert len(mutual(*plain[0])) >= 1
    assert len(mutual(1, 2)) == 0 and len(mutual(0, 2)) == 0
    # the same set inside a bracket, behind a recorded edit of a fourth object: the recorded launches are issued ahead of the set's own
    extra = box_object(ctx, probes=False)
    extra.set_densities(np.ones(256, dtype=np.float32))
    extra.absorb_sphere(np.array([16.0, 16.0, 30.0], dtype=np.float32), 4.0, 2.0)  # (an object's first edit allocates, with waits on the stream)

    def stats():
        out = np.zeros(3, dtype=np.uint64)
        capi.check(lib.ivx_many_stats(ctx.h, capi.ptr(out)))
        return [int(x) for x in out]

    capi.check(lib.ivx_many_begin(ctx.h))
    rec0, iss0, _ = stats()
    extra.absorb_sphere_enqueue(np.array([16.0, 17.0, 30.0], dtype=np.float32), 5.0, 3.0)
    rec1, _, _ = stats()
    assert rec1 > rec0, "the edit inside the bracket was not recorded"
    inside = bvol.set_grids(gs, sims)
    rec2, iss2, _ = stats()
    assert rec2 == rec1 and iss2 > iss0, "the set did not issue the recorded launches ahead of its own"
    inside_pairs = inside.pairs()
    capi.check(lib.ivx_many_flush(ctx.h))
    assert stats()[1] == iss2, "recorded launches were still waiting behind the set"
    assert extra.absorb_collect()["emptied_voxels"] > 0
    assert inside_pairs.tolist() == [[0, 1]] and inside.download()[0].tobytes() == world.tobytes()
    extra.close()
    # a clip that shortens the object (voxel extent 0.5): the box follows the ranges the clip left
    g = box_object(ctx, (40.0, 40.0, 40.0), 0.5, probes=False)
    before = bvol.grid_model_aabb(g)
    lo, hi = expected_model_box(g)
    assert before["lower"].tolist() == lo and before["upper"].tolist() == hi
    planes = []
    for d in range(3):
        for sgn, disp in ((1.0, 21.0 if d == 0 else 100.0), (-1.0, 100.0)):
            nrm = [0.0, 0.0, 0.0]
            nrm[d] = sgn
            planes.append((*nrm, disp))
    outcome, child, _ = g.extract_polyhedron((-100, -100, -100, 21, 100, 100), np.array(planes, dtype=np.float32))
    assert outcome == 1
    after = bvol.grid_model_aabb(g)  # (before anything asks for the ranges again: a clip refreshes them itself)
    lo, hi = expected_model_box(g)
    assert after["lower"].tolist() == lo and after["upper"].tolist() == hi
    assert after["lower"][0] > before["lower"][0] and after["upper"].tolist() == before["upper"].tolist()
    child.close()
    g.close()
    # a grid emptied by an absorbing sphere. The edit touches the occupied ranges only, so the rim voxels around the box keep their small positive
    # distances: no chunk becomes Void, and the object, like the reference's (intersection.rs:387-389), goes on holding the ranges it held — the
    # box is still the old one. The next update of the ranges finds no voxel: the all-zero box, and no pair
    held = bvol.grid_model_aabb(gs[1])
    r = gs[1].absorb_sphere(np.array([16.0, 16.0, 16.0], dtype=np.float32), 60.0, 58.0)
    assert r["emptied_voxels"] == 30 ** 3 and r["removed_chunks"] == 0
    assert bvol.grid_model_aabb(gs[1]).tobytes() == held.tobytes()
    assert [tuple(x) for x in gs[1].update_occupied_voxel_ranges()] == [(0, 0)] * 3
    empty = bvol.grid_model_aabb(gs[1])
    assert not empty.tobytes().strip(b"\0")
    s = bvol.set_grids(gs, sims)
    world, _ = s.download()
    assert world["lower"][1].tolist() == world["upper"][1].tolist() == offsets[1].tolist()
    assert s.pairs().tolist() == br.pairs(world)[0].tolist() == []
    for g in gs:
        g.close()


def test_state_and_refusals(ctx):
    lib = capi.lib()
    fresh = Context(0)
    try:
        box = np.zeros(1, dtype=capi.AABB_DTYPE)
        found = C.c_size_t(9)
        out = np.zeros((1, 2), dtype=np.uint32)
        q = bvol.query_array([bvol.box_query((0, 0, 0), (1, 1, 1))])
        masks, counts = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint32)
        # no set on the context yet
        assert lib.ivx_bv_download(fresh.h, capi.ptr(box), 1, capi.ptr(box)) == capi.IVX_ERR_STATE
        assert lib.ivx_bv_pairs(fresh.h, 0, capi.ptr(out), 1, C.byref(found)) == capi.IVX_ERR_STATE and found.value == 0
        assert lib.ivx_bv_queries(fresh.h, capi.ptr(q), 1, capi.ptr(masks), capi.ptr(counts)) == capi.IVX_ERR_STATE
        assert not lib.ivx_bv_device_ptr(fresh.h, capi.BV_PTR_WORLD_BOXES)
        # an empty set is a set: empty results, the all-zero total
        s = bvol.set_boxes(fresh, np.zeros(0, dtype=capi.AABB_DTYPE))
        world, total = s.download()
        assert world.size == 0 and not total.tobytes().strip(b"\0")
        assert s.pairs().shape == (0, 2)
        masks0, counts0 = s.query(q)
        assert masks0.shape == (1, 0) and counts0.tolist() == [0]
        # one box: no pair; no queries: nothing
        s = bvol.set_boxes(fresh, bvol.boxes([(0, 0, 0)], [(1, 1, 1)]))
        assert s.pairs().shape == (0, 2)
        assert lib.ivx_bv_queries(fresh.h, None, 0, None, None) == capi.IVX_OK
        masks1, counts1 = s.query(q)
        assert masks1.tolist() == [[1]] and counts1.tolist() == [1]
    finally:
        fresh.close()
    # refusals leave the context's set as it was
    world, kinds = br.scene(65)
    s = bvol.set_boxes(ctx, world, None, kinds)
    sims = bvol.similarities(65)
    for scaling in (0.0, -1.0, float("nan")):
        bad = sims.copy()
        bad["scaling"][64] = scaling
        assert lib.ivx_bv_set(ctx.h, capi.ptr(world), capi.ptr(bad), None, 65) == capi.IVX_ERR_INVALID
    bad_kinds = kinds.copy()
    bad_kinds[3] = 3
    assert lib.ivx_bv_set(ctx.h, capi.ptr(world), None, capi.ptr(bad_kinds), 65) == capi.IVX_ERR_INVALID
    assert lib.ivx_bv_set(ctx.h, None, None, None, 65) == capi.IVX_ERR_INVALID
    assert lib.ivx_bv_set(ctx.h, capi.ptr(world), None, None, capi.BV_MAX_OBJECTS + 1) == capi.IVX_ERR_CAPACITY
    found = C.c_size_t(0)
    out = np.zeros((4, 2), dtype=np.uint32)
    assert lib.ivx_bv_pairs(ctx.h, 2, capi.ptr(out), 4, C.byref(found)) == capi.IVX_ERR_INVALID
    assert lib.ivx_bv_pairs(ctx.h, 0, None, 4, C.byref(found)) == capi.IVX_ERR_INVALID
    assert lib.ivx_bv_pairs(ctx.h, 0, capi.ptr(out), 4, None) == capi.IVX_ERR_INVALID
    assert lib.ivx_bv_download(ctx.h, capi.ptr(np.zeros(64, dtype=capi.AABB_DTYPE)), 64, None) == capi.IVX_ERR_CAPACITY
    q = np.zeros(capi.BV_MAX_QUERIES + 1, dtype=capi.BV_QUERY_DTYPE)
    masks, counts = np.zeros((len(q), 2), dtype=np.uint64), np.zeros(len(q), dtype=np.uint32)
    assert lib.ivx_bv_queries(ctx.h, capi.ptr(q), len(q), capi.ptr(masks), capi.ptr(counts)) == capi.IVX_ERR_CAPACITY
    q["kind"][1] = 4
    assert lib.ivx_bv_queries(ctx.h, capi.ptr(q), 2, capi.ptr(masks), capi.ptr(counts)) == capi.IVX_ERR_INVALID
    assert lib.ivx_bv_queries(ctx.h, None, 2, capi.ptr(masks), capi.ptr(counts)) == capi.IVX_ERR_INVALID
    q["kind"][1] = 0
    assert lib.ivx_bv_queries(ctx.h, capi.ptr(q), 2, None, capi.ptr(counts)) == capi.IVX_ERR_INVALID
    assert_pairs_equal(s.pairs(1), br.scene_pairs(65, 1)[0], "after the refusals")
    # a grid that holds no ranges yet
    g = pu.gpu_from_graph(ctx, scenes.box_scene())
    assert lib.ivx_grid_model_aabb(g.h, capi.ptr(np.zeros(1, dtype=capi.AABB_DTYPE))) == capi.IVX_ERR_STATE
    with pytest.raises(capi.IvxError) as e:
        bvol.set_grids([g])
    assert e.value.code == capi.IVX_ERR_STATE
    assert_pairs_equal(s.pairs(1), br.scene_pairs(65, 1)[0], "after the refused set_grids")
    g.close()
