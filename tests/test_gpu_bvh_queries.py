"""Region queries through the hierarchy on the device (`ivx_bv_queries_hierarchy`, impact_amd/csrc/bvh.hip) and the hit lists made from the resident
masks (`ivx_bv_query_lists`, bvol.hip). The masks and counts: byte-equal to the flat `ivx_bv_queries` of the same set and to the library's host
form over the host tree (which test_bvh_queries_cpu.py holds against bvol_ref's restatement). The lists: `bvol.mask_indices` of the masks.
No expectation comes from the tree itself, and there is no tolerance anywhere in this file.

A query's workgroup expands the top of the tree until it holds 256 subtrees: the sizes lie on both sides of that, of a mask word and of the
lists' 256-word launches; 25 000 boxes under 1 000 boxes of up to half the scene is the reference's own benchmark shape."""
import ctypes as C

import numpy as np
import pytest

import bvh_query_cases as qc
import bvol_ref as br
import narrow_ref as nr
import parity_util as pu
from impact_amd import bvol, capi, collision, scenes
from impact_amd.physics import PhysicsWorld
from impact_amd.voxel import Context

pytestmark = pytest.mark.gpu


def built(ctx, world):
    s = bvol.set_boxes(ctx, world)
    s.build_hierarchy()
    return s


def assert_same(got, want, what):
    assert got[0].dtype == np.uint64 and got[0].shape == want[0].shape, what
    if got[0].tobytes() != want[0].tobytes():
        q, w = (int(x[0]) for x in np.nonzero(got[0] != want[0]))
        raise AssertionError(f"{what}: query {q}, word {w}: {int(got[0][q, w]):#x} != {int(want[0][q, w]):#x}")
    assert got[1].tobytes() == want[1].tobytes(), what


def assert_lists(s, masks, what):
    offsets, objects = s.query_lists()
    want = bvol.mask_indices(masks, s.n)
    want_offsets = np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.uint32)
    assert offsets.tobytes() == want_offsets.tobytes(), what
    assert objects.tobytes() == (np.concatenate(want) if want else np.zeros(0, dtype=np.uint32)).astype(np.uint32).tobytes(), what
    return offsets, objects


def check_all(ctx, world, queries, what):
    s = built(ctx, world)
    tree = s.query_hierarchy(queries)
    if len(queries) and len(world):
        assert_lists(s, tree[0], f"{what}: lists after the tree form")
    again = s.query_hierarchy(queries)
    assert again[0].tobytes() == tree[0].tobytes() and again[1].tobytes() == tree[1].tobytes(), f"{what}: two calls differ"
    flat = s.query(queries)
    assert_same(tree, flat, f"{what}: tree against flat")
    if len(queries) and len(world):
        assert_lists(s, flat[0], f"{what}: lists after the flat form")
    got_world, _ = s.download()
    nodes, leaves = s.hierarchy()
    assert_same(tree, bvol.queries_hierarchy_host(got_world, nodes, leaves, queries), f"{what}: device against host form")
    return tree


@pytest.mark.parametrize("n_queries", qc.QUERY_COUNTS)
@pytest.mark.parametrize("n", qc.SIZES)
def test_seeded_scene_with_mixed_queries(ctx, n, n_queries):
    masks, counts = check_all(ctx, br.scene(n)[0], br.mixed_queries(n, n_queries), f"n {n}, {n_queries} queries")
    if n >= 63:
        assert all(0 < int(counts[k]) < n for k in range(min(4, n_queries)))


@pytest.mark.parametrize("name", list(qc.hand_made_sets()))
def test_hand_made_sets(ctx, name):
    world = qc.hand_made_sets()[name]
    check_all(ctx, world, qc.queries_over(world, 32, 40), name)


@pytest.mark.parametrize("name", list(qc.adversarial_cases()))
def test_adversarial_sets(ctx, name):
    world, queries = qc.adversarial_cases()[name]
    masks, counts = check_all(ctx, world, queries, name)
    assert int(counts.sum()) > 0


def test_the_reference_benchmark_shape(ctx):
    """25 000 boxes of the seeded recipe under 1 000 box queries whose half extent runs from 0.5 to half the scene: queries that hit thousands of
    leaves, each spread over the lanes of its workgroup"""
    n, n_queries = 25000, 1000
    world = br.scene(n)[0]
    ext = br.scene_extent(n)
    rng = np.random.default_rng(4)
    queries = []
    for i in range(n_queries):
        half = 0.5 + (0.5 * ext - 0.5) * i / (n_queries - 1)
        centre = rng.uniform(0, ext, 3) if i + 1 < n_queries else np.full(3, 0.5 * ext)  # (the last one covers the scene: its stack fills up)
        queries.append(bvol.box_query(centre - half, centre + half))
    queries = bvol.query_array(queries)
    s = built(ctx, world)
    tree, flat = s.query_hierarchy(queries), s.query(queries)
    assert_same(tree, flat, "25 000 x 1 000")
    assert int(flat[1][-1]) == n and int(flat[1].min()) < 50
    offsets, objects = assert_lists(s, flat[0], "25 000 x 1 000: lists")
    assert len(objects) == int(flat[1].astype(np.int64).sum()) > 10 ** 6


def test_several_workgroups_a_query(ctx):
    """65 536 boxes: a query's front is shared among four workgroups, which OR into the same mask words"""
    n = 65536
    world, queries = br.scene(n)[0], br.mixed_queries(n, 64)
    s = built(ctx, world)
    tree, flat = s.query_hierarchy(queries), s.query(queries)
    assert_same(tree, flat, "65 536 x 64")
    assert all(n // 20 < int(c) < n for c in flat[1])
    assert s.query_hierarchy(queries)[0].tobytes() == tree[0].tobytes()
    assert_lists(s, tree[0], "65 536 x 64: lists")


def test_lists_capacity_residency_and_pointers(ctx):
    lib = capi.lib()
    world = br.scene(1000)[0]
    queries = br.mixed_queries(1000, 7)
    s = bvol.set_boxes(ctx, world)
    found = C.c_size_t(77)
    offsets, objects = np.full(8, 0xA5A5A5A5, dtype=np.uint32), np.full(7000, 0xA5A5A5A5, dtype=np.uint32)
    # no queries call since the set: IVX_ERR_STATE, and no resident lists
    assert lib.ivx_bv_query_lists(ctx.h, capi.ptr(offsets), capi.ptr(objects), 7000, C.byref(found)) == capi.IVX_ERR_STATE and found.value == 0
    assert not s.device_ptr(capi.BV_PTR_HIT_OFFSETS) and not s.device_ptr(capi.BV_PTR_HIT_OBJECTS)
    masks, counts = s.query(queries)
    total = int(counts.sum())
    assert 7 < total < 7000
    # one short: IVX_ERR_CAPACITY, the number found, nothing written
    assert lib.ivx_bv_query_lists(ctx.h, capi.ptr(offsets), capi.ptr(objects), total - 1, C.byref(found)) == capi.IVX_ERR_CAPACITY
    assert found.value == total and np.all(offsets == 0xA5A5A5A5) and np.all(objects == 0xA5A5A5A5)
    # objects == NULL with cap == 0 leaves them on the device only
    capi.check(lib.ivx_bv_query_lists(ctx.h, None, None, 0, C.byref(found)))
    assert found.value == total and np.all(objects == 0xA5A5A5A5)
    d_offsets, d_objects = s.device_ptr(capi.BV_PTR_HIT_OFFSETS), s.device_ptr(capi.BV_PTR_HIT_OBJECTS)
    assert d_offsets and d_objects and s.device_ptr(capi.BV_PTR_MASKS)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipDeviceSynchronize() == 0  # (the resident-only call leaves its last launch on the context's stream)
    want = bvol.mask_indices(masks, 1000)
    for address, count, expect in ((d_offsets, 8, np.concatenate([[0], np.cumsum([len(w) for w in want])])), (d_objects, total, np.concatenate(want))):
        resident = np.zeros(count, dtype=np.uint32)
        assert hip.hipMemcpy(resident.ctypes.data_as(C.c_void_p), C.c_void_p(address), resident.nbytes, 2) == 0  # (device to host)
        assert resident.tobytes() == expect.astype(np.uint32).tobytes()
    capi.check(lib.ivx_bv_query_lists(ctx.h, capi.ptr(offsets), capi.ptr(objects), 7000, C.byref(found)))
    assert offsets[7] == total == found.value and np.all(objects[total:] == 0xA5A5A5A5)
    # refused arguments
    assert lib.ivx_bv_query_lists(ctx.h, capi.ptr(offsets), None, 4, C.byref(found)) == capi.IVX_ERR_INVALID
    assert lib.ivx_bv_query_lists(ctx.h, capi.ptr(offsets), capi.ptr(objects), 7000, None) == capi.IVX_ERR_INVALID
    # a new queries call, and a new set, take the resident lists away
    s.query(queries[:3])
    assert not s.device_ptr(capi.BV_PTR_HIT_OFFSETS)
    assert_lists(s, masks[:3], "three queries")
    s = bvol.set_boxes(ctx, world[:100])
    assert not s.device_ptr(capi.BV_PTR_HIT_OFFSETS)
    assert lib.ivx_bv_query_lists(ctx.h, capi.ptr(offsets), capi.ptr(objects), 7000, C.byref(found)) == capi.IVX_ERR_STATE


def test_state_refusals_and_small_sets(ctx):
    lib = capi.lib()
    world = br.scene(1025)[0]
    queries = br.mixed_queries(1025, 8)
    masks, counts = np.zeros((8, 17), dtype=np.uint64), np.zeros(8, dtype=np.uint32)
    call = lambda h=None, q=queries, nq=8, m=masks: lib.ivx_bv_queries_hierarchy(ctx.h if h is None else h, capi.ptr(q) if q is not None else None, nq,
                                                                                    capi.ptr(m) if m is not None else None, capi.ptr(counts))
    # before a build: IVX_ERR_STATE; after it the flat form's bytes; after a new set IVX_ERR_STATE again until the tree is rebuilt
    s = bvol.set_boxes(ctx, world)
    assert call() == capi.IVX_ERR_STATE
    s.build_hierarchy()
    assert call() == capi.IVX_OK
    flat = s.query(queries)
    assert masks.tobytes() == flat[0].tobytes() and counts.tobytes() == flat[1].tobytes()
    # the flat form's refusals
    assert call(nq=capi.BV_MAX_QUERIES + 1) == capi.IVX_ERR_CAPACITY and call(q=None) == capi.IVX_ERR_INVALID and call(m=None) == capi.IVX_ERR_INVALID
    bad = queries.copy()
    bad["kind"][5] = 4
    assert call(q=bad) == capi.IVX_ERR_INVALID
    masks[:] = 7
    assert call(nq=0) == capi.IVX_OK and (masks == 7).all()
    small = br.scene(65)[0]
    s = bvol.set_boxes(ctx, small)
    assert call() == capi.IVX_ERR_STATE
    s.build_hierarchy()
    small_queries = br.mixed_queries(65, 8)
    assert_same(s.query_hierarchy(small_queries), qc.reference(small, small_queries), "a smaller set after a larger one")
    # no set at all, an empty set, one box
    fresh = Context(0)
    try:
        assert call(h=fresh.h) == capi.IVX_ERR_STATE
        s = built(fresh, br.scene(0)[0])
        got = s.query_hierarchy(small_queries)
        assert got[0].shape == (8, 0) and not got[1].any()
        found = C.c_size_t(0)
        assert lib.ivx_bv_query_lists(fresh.h, None, None, 0, C.byref(found)) == capi.IVX_ERR_STATE  # (that call had n == 0)
        one = bvol.boxes([(1, 1, 1)], [(2, 2, 2)])
        s = built(fresh, one)
        some = bvol.query_array([bvol.box_query((0, 0, 0), (1, 1, 1)), bvol.box_query((3, 3, 3), (4, 4, 4)), bvol.sphere_query((0, 0, 0), 1.8), bvol.sphere_query((0, 0, 0), 1.7)])
        got = s.query_hierarchy(some)
        assert got[0].tolist() == [[1], [0], [1], [0]] and got[1].tolist() == [1, 0, 1, 0]
        assert_same(got, s.query(some), "one box")
        offsets, objects = s.query_lists()
        assert offsets.tolist() == [0, 1, 1, 2, 2] and objects.tolist() == [0, 0]
    finally:
        fresh.close()


def test_inside_a_bracket_behind_a_recorded_edit(ctx):
    """inside an ivx_many_begin bracket, behind a recorded edit: the queries issue the recorded launches ahead of their own"""
    lib = capi.lib()
    g = pu.gpu_from_graph(ctx, scenes.box_scene((30.0, 30.0, 30.0)), 1.0)
    g.compute_all_derived_state()
    g.update_occupied_voxel_ranges()
    g.set_densities(np.ones(256, dtype=np.float32))
    g.absorb_sphere(np.array([16.0, 16.0, 30.0], dtype=np.float32), 4.0, 2.0)  # (an object's first edit allocates, with waits on the stream)

    def stats():
        out = np.zeros(3, dtype=np.uint64)
        capi.check(lib.ivx_many_stats(ctx.h, capi.ptr(out)))
        return [int(x) for x in out]

    world = br.scene(257)[0]
    queries = br.mixed_queries(257, 7)
    s = built(ctx, world)
    capi.check(lib.ivx_many_begin(ctx.h))
    recorded, issued, _ = stats()
    g.absorb_sphere_enqueue(np.array([16.0, 17.0, 30.0], dtype=np.float32), 5.0, 3.0)
    assert stats()[0] > recorded, "the edit inside the bracket was not recorded"
    inside = s.query_hierarchy(queries)
    assert stats()[1] > issued, "the queries did not issue the recorded launches ahead of their own"
    capi.check(lib.ivx_many_flush(ctx.h))
    assert g.absorb_collect()["emptied_voxels"] > 0
    assert_same(inside, qc.reference(world, queries), "inside the bracket")
    g.close()


def test_the_set_of_a_collision_world(ctx):
    """through ivx_cw_synchronize: narrow_ref.scene(70) ends in three planes, whose world boxes are unbounded"""
    local, dyn, kin = nr.scene(70)
    assert (local["shape"][-3:] == capi.CW_PLANE).all()
    w = PhysicsWorld(ctx)
    w.set_bodies(dyn, kin)
    cw = collision.CollisionWorld(w)
    cw.set_collidables(local)
    s = cw.synchronize()
    world, _ = s.download()
    assert (np.abs(world["lower"][-3:]) >= 1e30).any()
    queries = bvol.query_array(list(qc.queries_over(world, 32, 41)) + list(qc.frusta_over(world, 16, 42)))
    assert lib_state(ctx, queries) == capi.IVX_ERR_STATE  # (the new set has no tree yet)
    s.build_hierarchy()
    tree, flat = s.query_hierarchy(queries), s.query(queries)
    assert_same(tree, flat, "collision world")
    assert flat[0][:, -1].any() and int(flat[1].sum()) > 48  # (planes are hit)
    assert_lists(s, flat[0], "collision world: lists")
    w.close()


def lib_state(ctx, queries):
    masks, counts = np.zeros((len(queries), 2), dtype=np.uint64), np.zeros(len(queries), dtype=np.uint32)
    return capi.lib().ivx_bv_queries_hierarchy(ctx.h, capi.ptr(queries), len(queries), capi.ptr(masks), capi.ptr(counts))
