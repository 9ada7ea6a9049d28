"""Chunk culling on the device (impact_amd/csrc/cull.hip). The derivation: device records byte-equal to the library's host function. The
decision: every expectation is the float32 restatement of cull_ref.py over the DOWNLOADED device records, and arguments, counts and zero tails
must be byte-equal to it — no tolerance anywhere in this file."""
import numpy as np
import pytest

import cull_ref as cr
import parity_util as pu
from impact_amd import capi, cull, many, scenes
from impact_amd.voxel import VoxelObjectMesh
from test_cull_cpu import seeded_case

pytestmark = pytest.mark.gpu


def assert_result_matches(res, tables, view_flags, pair_flags=None, objects=None, mode=0, what=""):
    """download every view, restate from the downloaded records, compare bytes; -> (the regions' bytes, the device records)"""
    n_views = len(view_flags)
    got = [res.download(v) for v in range(n_views)]
    frusta = np.stack([g[2] for g in got]) if n_views else np.zeros((0, len(tables)), dtype=capi.CULLING_FRUSTUM_DTYPE)
    want = cr.expected(tables, frusta, view_flags, pair_flags, objects, mode)
    total = sum(len(t) for t in tables)
    for v, ((args, count, _), (w_args, w_count)) in enumerate(zip(got, want)):
        stride = 20 if int(view_flags[v]) & capi.CULL_VIEW_INDEXED else 16
        assert int(res.layout[v]["stride"]) == stride and int(res.layout[v]["n_slots"]) == total, (what, v)
        assert args.dtype == w_args.dtype and (int(count["draws"]), int(count["indices"])) == w_count, (what, v, count, w_count)
        assert (int(res.counts[v]["draws"]), int(res.counts[v]["indices"])) == w_count, (what, v)
        if args.tobytes() != w_args.tobytes():
            bad = np.nonzero(args != w_args)[0]
            raise AssertionError(f"{what} view {v} mode {mode}: {len(bad)} of {total} slots differ, first {bad[0]}: {args[bad[0]]} != {w_args[bad[0]]}")
        if mode == 1:
            assert not args[w_count[0]:].tobytes().strip(b"\0"), (what, v)
    offs = [int(r["offset"]) for r in res.layout]
    ends = [int(r["offset"]) + int(r["n_slots"]) * int(r["stride"]) for r in res.layout]
    assert all(a <= b for a, b in zip(ends[:-1], offs[1:])), "regions overlap"
    return b"".join(g[0].tobytes() for g in got), frusta


def test_device_derivation_equals_the_host_function(ctx):
    """the CPU test's seeded inputs (both kinds) and an unrotated orthographic box, whose negated axes carry -0.0: the records of
    ivx_cull_frusta are byte-equal to ivx_culling_frustum_from_view's"""
    rng0, rng1 = np.random.default_rng(100), np.random.default_rng(101)
    cases = [seeded_case(rng0, 0) for _ in range(20)] + [seeded_case(rng1, 1) for _ in range(20)]
    views = np.array([c[0] for c in cases] + [cr.orthographic_view(4.0, 4.0, 1.0, 9.0)])
    extents = np.array([c[2] for c in cases[:7]], dtype=np.float32)
    pairs = np.zeros((len(views), len(extents)), dtype=capi.CULL_PAIR_DTYPE)
    for v in range(len(views)):
        for o in range(len(extents)):
            pairs[v, o] = cases[(v + 3 * o) % len(cases)][1]
    pairs[-1] = cull.pairs(1, len(extents))[0]
    got = cull.cull_frusta(ctx, views, pairs, extents)
    want = cr.host_frusta(views, pairs, extents)
    assert got.tobytes() == want.tobytes()
    assert int(got[-1, 0]["most_inside_corners"][1]) == 0 and np.signbit(got[-1, 0]["planes"][1][1])


OBJECT_SETS = {"mixed": (0, 1, 63, 64, 65, 200), "alone": (200,), "130x1": (1,) * 130, "scan": (64 * 65 + 1,)}


@pytest.mark.parametrize("n_views", [1, 2, 11, 64])
@pytest.mark.parametrize("objects", list(OBJECT_SETS))
def test_culling_where_the_tiling_can_go_wrong(ctx, objects, n_views):
    """seeded random tables (chunk indices 0..40, every obscuredness entry set with probability 1/2): objects of 0, 1, 63, 64, 65 and 200
    submeshes in one call, one object alone, 130 objects of one submesh, one object of 64 x 65 + 1 submeshes (the scan's second round of 64
    tiles) x 1, 2, 11 and 64 views of mixed kinds and `indexed` bits, both modes"""
    tables, extents, views, pairs = cr.tiling_scene(OBJECT_SETS[objects], n_views, 11)
    rng = np.random.default_rng(5)
    objs = np.zeros(len(tables), dtype=capi.CULL_OBJECT_DTYPE)
    objs["first_index_base"], objs["base_vertex"] = rng.integers(0, 1 << 20, len(tables)), rng.integers(-1000, 1 << 20, len(tables))
    regions = {}
    for mode in (capi.CULL_ZEROED, capi.CULL_COMPACTED):
        res = cull.cull_submesh_tables(ctx, tables, extents, views, pairs, mode, objs)
        regions[mode], frusta = assert_result_matches(res, tables, views["flags"], pairs["flags"], objs, mode, f"{objects} x {n_views}")
        # the case shows what it is there for: per view a tenth of the slots frustum-culled and not obscured, a tenth obscured and inside, a tenth drawn
        c = cr.census(tables, frusta, n_views)
        assert c.min() >= 0.1, c.min(axis=0)
    assert regions[0] != regions[1]


def test_more_than_64_views_and_bad_arguments_are_refused(ctx):
    tables, extents, views, pairs = cr.tiling_scene((5,), 1, 11)
    many_views, many_pairs = np.repeat(views, 65), np.repeat(pairs, 65, axis=0)
    with pytest.raises(capi.IvxError) as e:
        cull.cull_submesh_tables(ctx, tables, extents, many_views, many_pairs)
    assert e.value.code == capi.IVX_ERR_INVALID
    cull.cull_submesh_tables(ctx, tables, extents, many_views[:64], many_pairs[:64])
    for field, value, where in (("kind", 2, "view"), ("scaling", 0.0, "pair"), ("scaling", -1.0, "pair"), ("scaling", float("nan"), "pair")):
        v, p = views.copy(), pairs.copy()
        (v if where == "view" else p)[field] = value
        with pytest.raises(capi.IvxError) as e:
            cull.cull_submesh_tables(ctx, tables, extents, v, p)
        assert e.value.code == capi.IVX_ERR_INVALID, (field, value)
    for extent in (0.0, -2.0):
        with pytest.raises(capi.IvxError) as e:
            cull.cull_submesh_tables(ctx, tables, [extent], views, pairs)
        assert e.value.code == capi.IVX_ERR_INVALID
    with pytest.raises(capi.IvxError) as e:
        cull.cull_submesh_tables(ctx, tables, extents, views, pairs, mode=2)
    assert e.value.code == capi.IVX_ERR_INVALID
    lib = capi.lib()
    layout, counts = np.zeros(1, dtype=capi.CULL_REGION_DTYPE), np.zeros(1, dtype=capi.CULL_COUNT_DTYPE)
    assert lib.ivx_cull_submesh_tables(ctx.h, None, None, 1, None, None, capi.ptr(views), 1, capi.ptr(pairs), 0, capi.ptr(layout), capi.ptr(counts)) == capi.IVX_ERR_INVALID
    assert lib.ivx_cull_submesh_tables(None, None, None, 0, None, None, None, 0, None, 0, None, None) == capi.IVX_ERR_INVALID
    assert lib.ivx_cull_many(None, 3, None, capi.ptr(views), 1, capi.ptr(pairs), 0, capi.ptr(layout), capi.ptr(counts)) == capi.IVX_ERR_INVALID
    # no objects, or no views: empty regions
    res = cull.cull_submesh_tables(ctx, [], [], views, np.zeros((1, 0), dtype=capi.CULL_PAIR_DTYPE))
    assert int(res.layout[0]["n_slots"]) == 0 and (int(res.counts[0]["draws"]), int(res.counts[0]["indices"])) == (0, 0)
    assert res.download(0)[0].size == 0
    res = cull.cull_submesh_tables(ctx, tables, extents, views[:0], pairs[:0])
    assert res.layout.size == 0


def plane_record(normal, d, corner=None):
    """a record whose first plane is (normal, d) and whose other planes cull nothing (zero normal, displacement -1)"""
    r = np.zeros((), dtype=capi.CULLING_FRUSTUM_DTYPE)
    r["planes"][:, 3] = -1.0
    r["planes"][0] = (normal[0], normal[1], normal[2], d)
    r["most_inside_corners"][0] = cr.corner_of(normal) if corner is None else corner
    r["apex"] = (-50.0, -50.0, -50.0)
    return r


def test_the_threshold_in_float32(ctx):
    """normal (1, 0, 0) and chunk 0 (most inside corner at x = 1), d stepping through the adjacent float32 values around 1.05: the outcome
    flips exactly where 1 - d < -0.05f does in float32; -0.05f exactly (normal (-1, 0, 0), lower corner, d = 0.05f) draws; a NaN plane draws; a
    normal of -0.0 components with the lower corner as the derivation would choose it reads the lower corner"""
    table = np.zeros(1, dtype=capi.SUBMESH_DTYPE)
    table["index_count"], table["index_offset"] = 30, 60
    d0 = np.float32(1.05)
    ds = [d0]
    for _ in range(20):
        ds.append(np.nextafter(ds[-1], np.float32(2.0)))
    for _ in range(20):
        ds.insert(0, np.nextafter(ds[0], np.float32(0.0)))
    recs = [plane_record((1.0, 0.0, 0.0), d) for d in ds]
    want = [bool((np.float32(1.0) - d) < np.float32(-0.05)) for d in ds]
    assert want[0] is False and want[-1] is True and sum(a != b for a, b in zip(want[:-1], want[1:])) == 1
    recs.append(plane_record((-1.0, 0.0, 0.0), np.float32(0.05)))
    want.append(False)  # -0.05f < -0.05f is false: equality draws
    recs.append(plane_record((-1.0, 0.0, 0.0), np.nextafter(np.float32(0.05), np.float32(1.0))))
    want.append(True)
    recs.append(plane_record((np.nan, np.nan, np.nan), np.nan))
    want.append(False)
    recs.append(plane_record((np.nan, 0.0, 0.0), 5.0, corner=0))
    want.append(False)
    # (-0.0, -0.0, -1): corner 0, the chunk's lower corner z = 0 -> distance -0.0 - 0.01, drawn; read at the upper corner it would be -1.01
    recs.append(plane_record((np.float32(-0.0), np.float32(-0.0), -1.0), 0.01))
    want.append(False)
    assert int(recs[-1]["most_inside_corners"][0]) == 0
    frusta = np.array(recs).reshape(len(recs), 1)
    flags = np.arange(len(recs)) % 2
    for mode in (0, 1):
        res = cull.cull_submesh_tables_frusta(ctx, [table], frusta, flags, None, mode)
        assert_result_matches(res, [table], flags, None, None, mode, "threshold")
        assert [int(c) == 0 for c in res.counts["draws"]] == want, (mode, res.counts["draws"].tolist())


def test_skip_flag_instance_indices_and_arena_offsets(ctx):
    tables, extents, views, pairs = cr.tiling_scene((70, 3, 40), 4, 11)
    pairs = pairs.copy()
    pairs["instance_idx"] = np.arange(12).reshape(4, 3) * 1000 + 17
    pairs["flags"][1, 0] = pairs["flags"][1, 2] = pairs["flags"][2, 1] = capi.CULL_PAIR_SKIP
    pairs["flags"][3, :] = capi.CULL_PAIR_SKIP
    objs = np.array([(1 << 30, -7), (12345, 1 << 29), (0, 0)], dtype=capi.CULL_OBJECT_DTYPE)
    bases = [0, 70, 73, 113]
    for mode in (0, 1):
        res = cull.cull_submesh_tables(ctx, tables, extents, views, pairs, mode, objs)
        assert_result_matches(res, tables, views["flags"], pairs["flags"], objs, mode, "skip")
        assert int(res.counts[3]["draws"]) == 0 and not res.download(3)[0]["index_count"].any()
        for v in range(4):
            args = res.download(v)[0]
            if mode == 0:
                for o in range(3):
                    a = args[bases[o]:bases[o + 1]]
                    assert np.all(a["first_instance"] == pairs["instance_idx"][v, o])
                    assert np.all(a["first_index"] == tables[o]["index_offset"] + objs[o]["first_index_base"])
                    if "base_vertex" in a.dtype.names:
                        assert np.all(a["base_vertex"] == objs[o]["base_vertex"])
                    if pairs["flags"][v, o]:
                        assert not a["index_count"].any() and not a["instance_count"].any()
            else:
                drawn = args[: int(res.counts[v]["draws"])]
                skipped = [int(pairs["instance_idx"][v, o]) for o in range(3) if pairs["flags"][v, o]]
                assert not np.isin(drawn["first_instance"], skipped).any() and np.all(drawn["instance_count"] == 1)
                assert not args[len(drawn):].tobytes().strip(b"\0")


def test_compacted_is_zeroed_in_place_without_the_culled_slots(ctx):
    tables, extents, views, pairs = cr.tiling_scene(OBJECT_SETS["mixed"], 11, 11)
    zeroed = cull.cull_submesh_tables(ctx, tables, extents, views, pairs, capi.CULL_ZEROED)
    z = [zeroed.download(v)[0] for v in range(11)]
    compacted = cull.cull_submesh_tables(ctx, tables, extents, views, pairs, capi.CULL_COMPACTED)
    assert compacted.counts.tobytes() == zeroed.counts.tobytes()
    for v in range(11):
        c, n = compacted.download(v)[0], int(compacted.counts[v]["draws"])
        kept = z[v][z[v]["instance_count"] > 0]
        assert len(kept) == n and c[:n].tobytes() == kept.tobytes() and not c[n:].tobytes().strip(b"\0")
        assert int(compacted.counts[v]["indices"]) == int(kept["index_count"].sum())


def camera_views_and_pairs(objects, offsets=None):
    """a narrow perspective camera outside the bodies and an orthographic view from the same place, looking at the first object's centre"""
    centre = 8.0 * np.asarray(objects[0].chunk_counts, dtype=np.float64)
    cam = centre + np.array([60.0, 45.0, 150.0])
    vq = cr.look_rotation(centre - cam)
    views = np.array([cr.perspective_view(16.0, 16.0, 1.0, 400.0), cr.orthographic_view(30.0, 30.0, 1.0, 400.0)])
    pairs = np.zeros((2, len(objects)), dtype=capi.CULL_PAIR_DTYPE)
    for v in range(2):
        for o in range(len(objects)):
            pairs[v, o] = cr.pair_record(vq, cam, (0, 0, 0, 1), (0, 0, 0) if offsets is None else offsets[o], 1.0, 10 * v + o)
    return views, pairs


def sphere_object(ctx, radius):
    g = pu.gpu_from_graph(ctx, scenes.sphere_scene(radius))
    g.compute_all_derived_state()
    g.update_occupied_voxel_ranges()
    g.label_regions()
    return g


def test_resident_mesh_before_and_after_an_edit(ctx):
    """a solid sphere of radius 40 — the smallest on a 6^3-chunk grid for which the CPU oracle leaves a chunk that lies inside this camera's
    frustum and is culled by obscuredness alone — through the normal step; culled under a perspective camera outside the body and under an
    orthographic view, again after a bite and ivx_mesh_sync; byte-equal to the restatement over ivx_mesh_download's table both times"""
    g = sphere_object(ctx, 40.0)
    assert g.chunk_counts == (6, 6, 6)
    mesh = VoxelObjectMesh.create(g)
    views, pairs = camera_views_and_pairs([g])
    for edited in (False, True):
        if edited:
            r = g.absorb_sphere(np.array([49.0, 47.0, 80.0], dtype=np.float32), 14.0, 12.0)
            assert r["invalidated"].any()
            mesh.sync_with_voxel_object(r["invalidated"])
        sub = mesh.download()[4]
        assert len(sub) > 64 and (sub["is_obscured_from_direction"].reshape(len(sub), -1) > 0).any()
        for mode in (0, 1):
            res = cull.cull_many([g], views, pairs, mode)
            _, frusta = assert_result_matches(res, [sub], views["flags"], pairs["flags"], None, mode, f"sphere, edited {edited}")
            outside, obscured = cr.classify(sub, frusta[0, 0])
            assert outside.any() and (~outside & ~obscured).any()
            assert (obscured & ~outside).any(), "no chunk inside the frustum is culled by obscuredness alone"
            live = np.zeros(int(mesh.counts["n_indices"]) + 1, dtype=np.int32)
            for s in sub:
                live[int(s["index_offset"]):int(s["index_offset"]) + int(s["index_count"])] += 1
            assert live.max() == 1
            for v in range(2):
                args = res.download(v)[0]
                ranges = {(int(s["index_offset"]), int(s["index_count"])) for s in sub}
                for a in args[args["instance_count"] > 0]:
                    assert (int(a["first_index"]), int(a["index_count"])) in ranges
    g.close()


def test_several_objects_brackets_halves_and_refusals(ctx):
    """ivx_cull_many over three grids of different chunk counts, one of them with a current but empty mesh: plainly; inside an ivx_many_begin
    bracket right after ivx_mesh_sync_many; as enqueue + collect; twice in a row; and what it refuses"""
    lib = capi.lib()
    gs = [sphere_object(ctx, 40.0), sphere_object(ctx, 12.0), sphere_object(ctx, 22.0)]
    assert len({g.chunk_counts for g in gs}) == 3
    meshes = [VoxelObjectMesh.create(g) for g in gs]
    # the middle one is eaten whole: its mesh stays current and has no submesh
    r = gs[1].absorb_sphere(8.0 * np.asarray(gs[1].chunk_counts, dtype=np.float32), 40.0, 38.0)
    meshes[1].sync_with_voxel_object(r["invalidated"])
    assert meshes[1].n_chunks() == 0
    offsets = [(0, 0, 0), (10, 0, 0), (40, 30, -20)]
    views, pairs = camera_views_and_pairs(gs, offsets)
    objs = np.array([(0, 0), (5000, 300), (90000, 7000)], dtype=capi.CULL_OBJECT_DTYPE)

    def tables():
        return [m.download()[4] for m in meshes]

    for mode in (0, 1):
        res = cull.cull_many(gs, views, pairs, mode, objs)
        plain, _ = assert_result_matches(res, tables(), views["flags"], pairs["flags"], objs, mode, "three objects")
        again = cull.cull_many(gs, views, pairs, mode, objs)
        assert b"".join(again.download(v)[0].tobytes() for v in range(2)) == plain and again.counts.tobytes() == res.counts.tobytes()
        halves = cull.cull_many(gs, views, pairs, mode, objs, enqueue_only=True)
        assert halves.counts is None
        halves.collect()
        assert b"".join(halves.download(v)[0].tobytes() for v in range(2)) == plain and halves.counts.tobytes() == res.counts.tobytes()
        assert res.device_ptr(capi.CULL_PTR_ARGS) and res.device_ptr(capi.CULL_PTR_COUNTS) and res.device_ptr(capi.CULL_PTR_FRUSTA)
    # edits, then the sync and the cull inside one bracket; the same cull outside afterwards
    rs = [gs[0].absorb_sphere(np.array([49.0, 47.0, 80.0], dtype=np.float32), 14.0, 12.0), None,
          gs[2].absorb_sphere(np.array([25.0, 24.0, 44.0], dtype=np.float32), 9.0, 7.0)]
    inval = [rs[0]["invalidated"], np.zeros(gs[1].n_chunks, dtype=np.uint8), rs[2]["invalidated"]]
    many.mesh_sync_many(meshes, inval)
    # inside the bracket an edit of a fourth object is RECORDED first (a twinned launch chain, nothing issued): the cull, whose launches have no
    # twin, must put what has been recorded on the stream before its own work — the launches are issued while it is enqueued, none is left for the flush
    extra = sphere_object(ctx, 16.0)
    extra.set_densities(np.ones(256, dtype=np.float32))
    extra.absorb_sphere(np.array([17.0, 17.0, 30.0], dtype=np.float32), 4.0, 2.0)  # (an object's first edit allocates, with waits on the stream)

    def stats():
        out = np.zeros(3, dtype=np.uint64)
        capi.check(lib.ivx_many_stats(ctx.h, capi.ptr(out)))
        return [int(x) for x in out]

    capi.check(lib.ivx_many_begin(ctx.h))
    rec0, iss0, fl0 = stats()
    extra.absorb_sphere_enqueue(np.array([17.0, 18.0, 31.0], dtype=np.float32), 5.0, 3.0)
    rec1, iss1, _ = stats()
    assert rec1 > rec0, "the edit inside the bracket was not recorded"
    inside = cull.cull_many(gs, views, pairs, capi.CULL_COMPACTED, objs, enqueue_only=True)
    rec2, iss2, _ = stats()
    assert rec2 == rec1 and iss2 > iss0, "the cull did not issue the recorded launches ahead of its own"
    capi.check(lib.ivx_many_flush(ctx.h))
    assert stats()[1] == iss2, "recorded launches were still waiting behind the cull: it went onto the stream ahead of them"
    assert extra.absorb_collect()["emptied_voxels"] > 0
    inside.collect()
    in_bytes, _ = assert_result_matches(inside, tables(), views["flags"], pairs["flags"], objs, 1, "inside the bracket")
    outside = cull.cull_many(gs, views, pairs, capi.CULL_COMPACTED, objs)
    out_bytes, _ = assert_result_matches(outside, tables(), views["flags"], pairs["flags"], objs, 1, "outside the bracket")
    assert in_bytes == out_bytes and inside.counts.tobytes() == outside.counts.tobytes()
    # the ready-records form over the resident tables
    frusta = np.stack([outside.download(v)[2] for v in range(2)])
    ready = cull.cull_many_frusta(gs, frusta, views["flags"], pairs["flags"], capi.CULL_COMPACTED, objs)
    assert b"".join(ready.download(v)[0].tobytes() for v in range(2)) == out_bytes
    # no objects (a frame without voxel objects), and no views: success with empty regions
    for mode in (0, 1):
        none = cull.cull_many([], views, np.zeros((2, 0), dtype=capi.CULL_PAIR_DTYPE), mode)
        assert none.layout["n_slots"].tolist() == [0, 0] and none.layout["offset"].tolist() == [0, 0]
        assert none.layout["stride"].tolist() == [20 if f & capi.CULL_VIEW_INDEXED else 16 for f in views["flags"].tolist()]
        assert none.counts["draws"].tolist() == [0, 0] and none.counts["indices"].tolist() == [0, 0]
        none = cull.cull_many([], views, np.zeros((2, 0), dtype=capi.CULL_PAIR_DTYPE), mode, enqueue_only=True)
        assert none.layout["n_slots"].tolist() == [0, 0]
        no_views = cull.cull_many(gs, views[:0], pairs[:0], mode, objs)
        assert no_views.layout.size == 0 and no_views.counts.size == 0
        no_views = cull.cull_many(gs, views[:0], pairs[:0], mode, objs, enqueue_only=True).collect()
        assert no_views.counts.size == 0
    none = cull.cull_many_frusta([], np.zeros((2, 0), dtype=capi.CULLING_FRUSTUM_DTYPE), views["flags"])
    assert none.layout["n_slots"].tolist() == [0, 0] and none.counts["draws"].tolist() == [0, 0]
    handles0 = many._handles(gs[:1])
    assert lib.ivx_cull_many(capi.ptr(handles0), 0, None, None, 0, None, 0, None, None) == capi.IVX_OK
    # refusals
    fresh = sphere_object(ctx, 12.0)  # never meshed
    with pytest.raises(capi.IvxError) as e:
        cull.cull_many([gs[0], fresh], views, pairs[:, :2])
    assert e.value.code == capi.IVX_ERR_STATE
    with pytest.raises(capi.IvxError) as e:
        cull.cull_many(gs, np.repeat(views, 33), np.repeat(pairs, 33, axis=0))
    assert e.value.code == capi.IVX_ERR_INVALID
    for field, value, where in (("kind", 7, "view"), ("scaling", 0.0, "pair")):
        v, p = views.copy(), pairs.copy()
        (v if where == "view" else p)[field] = value
        with pytest.raises(capi.IvxError) as e:
            cull.cull_many(gs, v, p)
        assert e.value.code == capi.IVX_ERR_INVALID
    layout, counts = np.zeros(2, dtype=capi.CULL_REGION_DTYPE), np.zeros(2, dtype=capi.CULL_COUNT_DTYPE)
    handles = many._handles(gs)
    assert lib.ivx_cull_many(capi.ptr(handles), 3, None, None, 2, capi.ptr(pairs), 0, capi.ptr(layout), capi.ptr(counts)) == capi.IVX_ERR_INVALID
    assert lib.ivx_cull_many(capi.ptr(handles), 3, None, capi.ptr(views), 2, None, 0, capi.ptr(layout), capi.ptr(counts)) == capi.IVX_ERR_INVALID
    assert lib.ivx_cull_many(capi.ptr(handles), 3, None, capi.ptr(views), 2, capi.ptr(pairs), 0, None, capi.ptr(counts)) == capi.IVX_ERR_INVALID
    assert lib.ivx_cull_many(capi.ptr(handles), 3, None, capi.ptr(views), 2, capi.ptr(pairs), 3, capi.ptr(layout), capi.ptr(counts)) == capi.IVX_ERR_INVALID
    assert lib.ivx_cull_collect(ctx.h, capi.ptr(counts), 5) == capi.IVX_ERR_INVALID
    for g in gs + [fresh, extra]:
        g.close()
