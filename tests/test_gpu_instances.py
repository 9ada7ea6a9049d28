"""Frame instances on the device (impact_amd/csrc/instances.hip). Every expectation is the library's host form (`ivx_fi_views_host`, which the CPU
tests hold against the float32 restatement) over the context's DOWNLOADED world boxes and masks, or the existing cull call fed the downloaded
pairs: pairs, lists, kept masks and results must be byte-equal — no tolerance anywhere in this file.

The partitions of the kernels and the sizes that sit on each side of them: the decide kernel reduces 64 objects per wave and a REDUCTION TILE of
256 objects per workgroup (n = 63, 64, 65 and 255, 256, 257); the EMIT BLOCK is 256 consecutive (view, object) pairs (one view of 255, 256 and
257 objects: one block short, one block full, a second block of one pair; 11 views of 65 objects: blocks that straddle views); the SCAN ROUND of
the per-view prefix is 1 024 kept words, 65 536 objects (n = 65 536: one full round; 65 537: a second round of one word)."""
import numpy as np
import pytest

import bvol_ref as br
import cull_ref as cr
import instances_ref as ir
import parity_util as pu
from impact_amd import bvol, capi, collision, cull, instances, scenes
from impact_amd.physics import PhysicsWorld
from impact_amd.voxel import Context, VoxelObjectMesh
from test_instances_cpu import assert_outputs_equal

pytestmark = pytest.mark.gpu

N_QUERIES = 9
REDUCTION_TILE, EMIT_BLOCK, SCAN_ROUND_OBJECTS = 256, 256, 1024 * 64
CASES = [(1, 1, False), (63, 11, False), (64, 64, False), (65, 11, True), (REDUCTION_TILE - 1, 1, False), (REDUCTION_TILE, 1, True), (REDUCTION_TILE + 1, 1, False),
         (1000, 11, False), (SCAN_ROUND_OBJECTS, 2, False), (SCAN_ROUND_OBJECTS + 1, 2, True)]
assert REDUCTION_TILE == EMIT_BLOCK  # (one view of n objects is n pairs: the same three sizes sit around both)


def want_of(host):
    return (host.pairs, host.offsets, host.objects, host.transforms, host.kept, host.results)


def run_chain(fi, world, inst, masks, chain):
    """the device calls of `chain` (view arrays, each call's and_view naming the one before) -> per call (downloaded outputs with the results, the
    host form's outputs over the same inputs)"""
    out, prev = [], None
    for views in chain:
        results = fi.views(views)
        got = fi.download()
        got.results = results
        host = instances.views_host(world, inst, masks, views, prev)
        out.append((got, host))
        prev = host.kept
    return out


@pytest.mark.parametrize("n,n_views,hierarchy", CASES)
def test_device_equals_the_host_form(ctx, n, n_views, hierarchy):
    """the seeded scene, its nine seeded queries through the flat or the hierarchy form, then two calls (the second takes and_view from the first;
    REACH and BOX cycle through their four combinations): every output of both equals the host form over the downloaded boxes and masks, and a
    second run of the chain leaves the same bytes"""
    world0, inst = ir.scene(n)
    s = bvol.set_boxes(ctx, world0)
    queries = br.mixed_queries(n, N_QUERIES)
    if hierarchy:
        s.build_hierarchy()
        masks, _ = s.query_hierarchy(queries)
    else:
        masks, _ = s.query(queries)
    world, _ = s.download()
    fi = instances.FrameInstances(ctx)
    fi.set_instances(inst)
    chain = [ir.seeded_views(n, min(n_views, 5), N_QUERIES, 0, seed=1), ir.seeded_views(n, n_views, N_QUERIES, min(n_views, 5), seed=2)]
    first = run_chain(fi, world, inst, masks, chain)
    for k, (got, host) in enumerate(first):
        assert_outputs_equal(got, want_of(host), f"n {n} x {len(chain[k])} views, call {k}")
    if n >= 63:  # the case can show something
        got = first[1][0]
        assert 0 < int(got.offsets[-1]) < n * n_views and (got.pairs["flags"] == capi.CULL_PAIR_SKIP).any() and (got.pairs["flags"] == 0).any()
    again = run_chain(fi, world, inst, masks, chain)
    assert [g.tobytes() for g, _ in again] == [g.tobytes() for g, _ in first]
    assert all(fi.device_ptr(w) for w in range(7))


def test_and_view_sees_the_previous_call_only(ctx):
    """three calls over 300 objects: the second takes and_view from the first (5 views), the third from the second (2 views) — a view index that
    only the first call had is refused, and the refused call leaves the second call's outputs in place"""
    n = 300
    world0, inst = ir.scene(n)
    s = bvol.set_boxes(ctx, world0)
    masks, _ = s.query(br.mixed_queries(n, N_QUERIES))
    world, _ = s.download()
    fi = instances.FrameInstances(ctx)
    fi.set_instances(inst)
    a, b = ir.seeded_views(n, 5, N_QUERIES, 0, seed=1), ir.seeded_views(n, 2, N_QUERIES, 0, seed=2)
    b["and_view"] = (4, 3)
    c = ir.seeded_views(n, 11, N_QUERIES, 2, seed=3)
    assert (c["and_view"] != capi.FI_NONE).any()
    runs = run_chain(fi, world, inst, masks, [a, b, c])
    for k, (got, host) in enumerate(runs):
        assert_outputs_equal(got, want_of(host), f"call {k}")
    c_first = instances.views_host(world, inst, masks, c[c["and_view"] != capi.FI_NONE][:1], runs[0][1].kept)
    c_second = instances.views_host(world, inst, masks, c[c["and_view"] != capi.FI_NONE][:1], runs[1][1].kept)
    assert c_first.kept.tobytes() != c_second.kept.tobytes(), "the case cannot tell the first call's kept sets from the second's"
    run_chain(fi, world, inst, masks, [a, b])
    stale = c.copy()
    stale["and_view"][1] = 3  # (the first call had a view 3, the second has not)
    with pytest.raises(capi.IvxError) as e:
        fi.views(stale)
    assert e.value.code == capi.IVX_ERR_INVALID
    fi.n_views = 2
    assert_outputs_equal(fi.download(), want_of(runs[1][1])[:5] + (None,), "after the refused call")
    # nothing waits without results, and the outputs are the same
    assert fi.views(c, with_results=False) is None
    assert_outputs_equal(fi.download(), want_of(runs[2][1])[:5] + (None,), "without results")


def expect_state(call):
    with pytest.raises(capi.IvxError) as e:
        call()
    assert e.value.code == capi.IVX_ERR_STATE, e.value


def test_state_refusals_and_empty_calls():
    c = Context(0)
    try:
        fi = instances.FrameInstances(c)
        world, inst = ir.scene(65)
        views = ir.seeded_views(65, 3, N_QUERIES, 0, seed=1)
        queries = br.mixed_queries(65, N_QUERIES)
        expect_state(lambda: fi.views(views))  # before a set
        expect_state(fi.download)
        s = bvol.set_boxes(c, world)
        expect_state(lambda: fi.views(views))  # no queries call since the set
        masks, _ = s.query(queries)
        expect_state(lambda: fi.views(views))  # no instances
        fi.set_instances(inst[:64])
        expect_state(lambda: fi.views(views))  # 64 instances, 65 objects
        fi.set_instances(inst)
        results = fi.views(views)
        host = instances.views_host(world, inst, masks, views)
        assert results.tobytes() == host.results.tobytes()
        with pytest.raises(capi.IvxError) as e:  # a refused set of instances leaves the instances as they were
            bad = inst.copy()
            bad["flags"][3] = 64
            fi.set_instances(bad)
        assert e.value.code == capi.IVX_ERR_INVALID
        fi.n = 65
        assert fi.views(views).tobytes() == host.results.tobytes()
        s = bvol.set_boxes(c, world)  # a new set: its queries have not run
        expect_state(lambda: fi.views(views))
        s.query(queries)
        chained = views.copy()
        chained["and_view"][0] = 0
        with pytest.raises(capi.IvxError) as e:  # ... and the kept masks of the old set are gone
            fi.views(chained)
        assert e.value.code == capi.IVX_ERR_INVALID
        # no views, and no objects: empty outputs
        assert fi.views(views[:0]).size == 0
        out = fi.download()
        assert out.pairs.shape == (0, 65) and out.offsets.tolist() == [0]
        s = bvol.set_boxes(c, world[:0])
        s.query(queries)
        fi.set_instances(inst[:0])
        empty = fi.views(views[:2])
        assert empty.tobytes() == b"".join(ir.empty_result().tobytes() for _ in range(2))
        out = fi.download()
        assert out.pairs.shape == (2, 0) and out.offsets.tolist() == [0, 0, 0] and out.objects.size == 0
    finally:
        c.close()


def sphere_object(ctx, radius):
    g = pu.gpu_from_graph(ctx, scenes.sphere_scene(radius))
    g.compute_all_derived_state()
    g.update_occupied_voxel_ranges()
    g.label_regions()
    return g


def frame_views(centre):
    """1 camera + 6 cubemap faces + 4 cascades: (frame-instance world_to_view similarities, cull views)"""
    rng = np.random.default_rng(17)
    sims, cull_views = [], []
    for v in range(11):
        direction = rng.normal(size=3) if v else np.array([-60.0, -45.0, -150.0])
        q = cr.look_rotation(direction)
        eye = np.asarray(centre, dtype=np.float64) - 180.0 * direction / np.linalg.norm(direction)
        rotation = cr.q_conj(q)
        sims.append(instances.isometry(rotation, -cr.q_rot(rotation, eye)))
        cull_views.append(cr.perspective_view(24.0, 24.0, 1.0, 500.0, indexed=v > 0) if v < 7 else cr.orthographic_view(40.0, 40.0, 1.0, 500.0))
    return np.array(sims), np.array(cull_views)


@pytest.fixture(scope="module")
def voxel_frame(ctx):
    """three small voxel spheres with current meshes among seven bounding volumes (objects 5, 1 and 3 of the set), and the frame's records"""
    gs = [sphere_object(ctx, r) for r in (22.0, 12.0, 16.0)]
    meshes = [VoxelObjectMesh.create(g) for g in gs]
    index = np.array([5, 1, 3], dtype=np.uint32)
    rng = np.random.default_rng(23)
    models = bvol.boxes(rng.uniform(-4.0, 0.0, (7, 3)), rng.uniform(1.0, 5.0, (7, 3)))
    sims = bvol.similarities(7)
    sims["translation"] = rng.uniform(-30.0, 30.0, (7, 3))
    for g, o in zip(gs, index):
        models[o] = bvol.grid_model_aabb(g)
    inst = instances.instances(sims, flags=[0, 0, capi.FI_HIDDEN, 0, 0, 0, capi.FI_CASTS_NO_SHADOWS], entities=np.arange(7) + 50)
    world_to_view, cull_views = frame_views(sims["translation"][5] + 8.0 * np.asarray(gs[0].chunk_counts))
    queries = [bvol.box_query((-200, -200, -200), (200, 200, 200))] * 5 + [bvol.sphere_query(sims["translation"][int(index[v % 3])], 30.0) for v in range(6)]
    views = np.array([instances.camera_view(world_to_view[0], 0, instance_base=100)] +
                     [instances.cubemap_face_view(world_to_view[v], v, capi.FI_NONE, instance_base=1000 * v) for v in range(1, 7)] +
                     [instances.cascade_view(world_to_view[v], v, light_entity=51 if v == 8 else capi.FI_NONE, instance_base=1000 * v) for v in range(7, 11)])
    yield gs, index, models, sims, inst, bvol.query_array(queries), views, cull_views
    for g in gs:
        g.close()


def regions_of(res, n_views):
    got = [res.download(v) for v in range(n_views)]
    return b"".join(g[0].tobytes() for g in got), np.array([g[1] for g in got]), np.stack([g[2] for g in got])


@pytest.mark.parametrize("mode", [capi.CULL_ZEROED, capi.CULL_COMPACTED])
def test_resident_cull_equals_the_cull_of_the_downloaded_pairs(ctx, voxel_frame, mode):
    """ivx_cull_many_resident over objects 5, 1, 3 of seven under 1 camera + 6 faces + 4 cascades: its argument regions, counts and frustum records
    are the bytes of ivx_cull_many fed the downloaded frame-instance pairs gathered on the host"""
    gs, index, models, sims, inst, queries, views, cull_views = voxel_frame
    s = bvol.set_boxes(ctx, models, sims)
    s.query(queries)
    fi = instances.FrameInstances(ctx)
    fi.set_instances(inst)
    fi.views(views, with_results=False)
    res = fi.cull(gs, cull_views, index, mode).collect()
    pairs = fi.download().pairs
    gathered = np.ascontiguousarray(pairs[:, index])
    assert (gathered["flags"] == 0).any() and (gathered["flags"] == capi.CULL_PAIR_SKIP).any(), "the case needs kept and skipped pairs among the voxel objects"
    got = regions_of(res, 11)
    want_res = cull.cull_many(gs, cull_views, gathered, mode)
    want = regions_of(want_res, 11)
    assert res.layout.tobytes() == want_res.layout.tobytes() and res.counts.tobytes() == want_res.counts.tobytes()
    assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
    assert int(res.counts["draws"].sum()) > 0
    # the identity when no indices are given: the first three instances
    fi.views(views, with_results=False)
    plain = fi.cull(gs, cull_views, None, mode).collect()
    want_plain = cull.cull_many(gs, cull_views, np.ascontiguousarray(pairs[:, :3]), mode)
    assert regions_of(plain, 11)[0] == regions_of(want_plain, 11)[0] and plain.counts.tobytes() == want_plain.counts.tobytes()
    # refusals: another number of views than the last ivx_fi_views call; an index past its n
    fi.views(views, with_results=False)
    with pytest.raises(capi.IvxError) as e:
        fi.cull(gs, cull_views[:10], index, mode)
    assert e.value.code == capi.IVX_ERR_STATE
    with pytest.raises(capi.IvxError) as e:
        fi.cull(gs, cull_views, [5, 7, 3], mode)
    assert e.value.code == capi.IVX_ERR_INVALID
    none = fi.cull([], cull_views, None, mode)  # (a frame without voxel objects touches no context)
    assert none.layout["n_slots"].tolist() == [0] * 11


def test_one_frame_through_the_collision_world(ctx, voxel_frame):
    """synchronize -> queries -> instances -> cull on the context's stream, the three voxel objects as collidables 5, 1, 3 of seven: the frame reads
    back the results and the draw counts only (the query call's own masks are not used). Afterwards everything is downloaded and held against the
    host form and the existing cull call."""
    gs, index, models, sims, inst, queries, views, cull_views = voxel_frame
    dyn = np.zeros(7, dtype=capi.RIGID_BODY_DTYPE)
    dyn["mass"], dyn["orientation"][:, 3], dyn["position"] = 1.0, 1.0, sims["translation"]
    dyn["inertia"][:, [0, 4, 8]], dyn["inv_inertia"][:, [0, 4, 8]] = 1.0, 1.0
    w = PhysicsWorld(ctx)
    w.set_bodies(dyn)
    cw = collision.CollisionWorld(w)
    cw.set_collidables(np.array([collision.voxel_object(models["lower"][o], models["upper"][o], o, 100 + o) if o in index else collision.sphere((0, 0, 0), 3.0, o, 100 + o)
                                 for o in range(7)], dtype=capi.COLLIDABLE_DTYPE))
    fi = instances.FrameInstances(ctx)
    fi.set_instances(inst)
    # the frame
    s = cw.synchronize()
    s.query(queries)
    results = fi.views(views)
    res = fi.cull(gs, cull_views, index, capi.CULL_COMPACTED).collect()
    # ... and its check
    world, _ = s.download()
    masks, _ = s.query(queries)
    host = instances.views_host(world, inst, masks, views)
    got = fi.download()
    got.results = results
    assert_outputs_equal(got, want_of(host), "the frame")
    assert int(results["count"][0]) >= 3 and int(res.counts["draws"].sum()) > 0
    want = cull.cull_many(gs, cull_views, np.ascontiguousarray(got.pairs[:, index]), capi.CULL_COMPACTED)
    assert res.counts.tobytes() == want.counts.tobytes() and regions_of(res, 11)[0] == regions_of(want, 11)[0]
    w.close()
