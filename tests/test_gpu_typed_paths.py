"""Several voxel types through everything downstream of the sampler. Type 0 is what a zero-filled or never-written buffer holds, so a parity
test on a type-0 body cannot see a kernel that drops, misplaces or never writes a type byte. Here the bodies are sampled on the device with
the gradient-noise type generator and compared with the oracle built from the oracle generator's own planes overlaid with the restated
noise types (tests/typed_util.py): the incremental remesh (mixed-material quads inside the re-meshed ranges), edits (Uniform chunks of a
non-zero type spread over a plane, per-type emptied counts), clips, batched copies, fragments and split-offs (the children's type planes),
and `_many` batches that mix a typed and a same-type object. Densities are 1 + t per type, so a stage that takes one type for all voxels
shows in the moments too. Every case first asserts ON THE ORACLE that it holds what it is meant to show. (The x-slab protocol with types:
tests/test_gpu_slabs.py, tests/test_gpu_slabs_ipc.py; random operation mixes: tests/test_gpu_random_mix.py.)"""
import numpy as np
import pytest

import oracle_lib as ol
import parity_util as pu
import typed_util as tu
from impact_amd import capi, many, scenes
from impact_amd import fracturing as fr
from impact_amd.sdf_graph import SDFGraph, SDFNode
from impact_amd.voxel import SDFVoxelGenerator, VoxelObject, VoxelObjectMesh
from test_gpu_clip import rotated_box
from test_gpu_mesh_sync import SYNC_CASES, assert_synced_meshes_equal, edit_sequence, sync_after_edits

pytestmark = pytest.mark.gpu
f32 = np.float32
DENS = tu.DENSITIES
NO_SAMPLE = capi.STAGE_ALL & ~capi.STAGE_SAMPLE
# (graph, sphere radius, noise): the sphere of test_gpu_voxel_types (22 Uniform chunks of all four types), and a small sphere whose types
# change every few voxels, so that nearly every surface chunk holds quads of mixed materials
BODIES = {
    "sphere60": (tu.sphere60, 60.0, tu.SPHERE60_NOISE),
    "sphere30_fine": (lambda: scenes.sphere_scene(30.0), 30.0, (4, 0.05, 1.0, 3)),
}


def both(ctx, graph, extent, noise):
    o = tu.typed_oracle(graph, extent, noise)
    g = tu.typed_gpu(ctx, graph, extent, noise)
    return o, g


def centre_of(o):
    return np.array([0.5 * (a + b) for a, b in o.info()["occupied_voxel_ranges"]], dtype=f32)


def assert_typed_objects_equal(o, g, what="", with_mesh=True):
    """parity_util.assert_edited_objects_equal with the per-type densities, plus the type of every Uniform chunk's record; -> the types among
    the object's non-empty voxels"""
    pu.assert_edited_objects_equal(o, g, what, densities=DENS, with_mesh=with_mesh)
    _, o_typ, o_flg, _, o_info = o.export_dense()
    g_info = g.download(sdf=False, types=False, flags=False, labels=False)[4]
    uni = o_info["kind"] == 1
    np.testing.assert_array_equal(g_info["uniform_type"][uni], o_info["uniform_type"][uni], err_msg=what + "uniform_type")
    return tu.types_of_non_empty(o_typ, o_flg)


# ---- b. incremental remesh -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SYNC_CASES)
@pytest.mark.parametrize("body", list(BODIES))
def test_sync_after_edits_of_a_typed_body(ctx, body, case):
    """the four edit sequences of test_gpu_mesh_sync.test_sync_after_edits, scaled to the body: every sync re-meshes chunks whose quads have
    mixed materials (the mesher's general pass and its hard-edge hand-over inside a sync). The fine-grained body takes its sphere edits in
    the enqueue / collect form with the early mesh needs on. (`eaten_whole` leaves no submesh to hold materials: there the chunks that LOSE
    their submeshes are the mixed ones, and the census before the edit says so.)"""
    make, radius, noise = BODIES[body]
    graph = make()
    probe = tu.typed_oracle(graph, 1.0, noise)
    assert tu.mixed_material_submeshes(probe.mesh()) >= 50
    census = tu.edit_census(probe, edit_sequence(case, centre_of(probe), radius), DENS)
    assert len(census["emptied_types"]) >= 2
    if case != "eaten_whole":
        assert all(m >= 1 for m in census["mixed_remeshed"]), census
    if body == "sphere60":  # (the fine-grained body has no Uniform chunk)
        assert census["converted_typed_uniform"] >= 1
    o, g = both(ctx, graph, 1.0, noise)
    sync_after_edits(o, g, case, radius, DENS, overlapped=body == "sphere30_fine")


def test_mesh_sync_many_over_two_typed_bodies(ctx):
    """`ivx_absorb_sphere_many` + `ivx_mesh_sync_many` over both bodies, three rounds: every object's synced mesh against its oracle's"""
    specs = [BODIES["sphere60"], BODIES["sphere30_fine"]]
    rounds = [((0.0, 0.0, 1.0), 7.0 / 30.0), ((0.6, 0.0, 0.8), 11.0 / 30.0), ((0.0, -1.0, 0.0), 12.0 / 30.0)]

    def edits_of(o, radius):
        c = centre_of(o)
        return [("s", c + f32(radius) * np.asarray(d, f32), float(f32(k * radius))) for d, k in rounds]

    for make, radius, noise in specs:
        probe = tu.typed_oracle(make(), 1.0, noise)
        census = tu.edit_census(probe, edits_of(probe, radius), DENS)
        assert len(census["emptied_types"]) >= 2 and all(m >= 1 for m in census["mixed_remeshed"]), census
    pairs = [both(ctx, make(), 1.0, noise) for make, _, noise in specs]
    os_, gs = [p[0] for p in pairs], [p[1] for p in pairs]
    oms = [ol.OracleMeshHandle(o) for o in os_]
    gms = [VoxelObjectMesh.create(g) for g in gs]
    seqs = [edits_of(o, radius) for o, (_, radius, _) in zip(os_, specs)]
    for rnd in range(len(rounds)):
        es = [s[rnd] for s in seqs]
        ros = [o.absorb_sphere(e[1], e[2] + 2.0, e[2], DENS) for o, e in zip(os_, es)]
        rgs = many.absorb_sphere_many(gs, [e[1] for e in es], [e[2] + 2.0 for e in es], [e[2] for e in es], DENS)
        for k, (ro, rg) in enumerate(zip(ros, rgs)):
            np.testing.assert_array_equal(rg["invalidated"], ro["invalidated"], err_msg=f"object {k}, round {rnd}")
            assert rg["emptied_voxels"] == int(ro["emptied_by_type"].sum())
            scale = np.maximum(np.abs(ro["removed64"]), 1e-300)
            assert np.all(np.abs(rg["removed_moments"] - ro["removed64"]) <= 1e-5 * scale + 1e-9), (k, rnd)
            om = oms[k]
            om.sync(ro["invalidated"])
        many.mesh_sync_many(gms, [rg["invalidated"] for rg in rgs])
        for k in range(len(gs)):
            assert_synced_meshes_equal(oms[k].get(), gms[k].download())
            assert_typed_objects_equal(os_[k], gs[k], f"object {k}, round {rnd}: ", with_mesh=False)
    for g in gs:
        g.close()


# ---- c. edits of sampled typed objects -------------------------------------------------------------------------------------------------
SPHERE_BITES = [("s", (0.0, 0.0, 60.0), 20.0), ("s", (36.0, 0.0, 48.0), 25.0), ("s", (0.0, -30.0, 0.0), 12.0)]
CAPSULES = [("c", (-70.0, 5.0, 10.0), (140.0, -10.0, 6.0), 8.0), ("c", (3.0, -2.0, -70.0), (1e-9, 4.0, 140.0), 10.0)]


def placed(edits, ctr):
    return [(e[0], ctr + np.asarray(e[1], f32), *[np.asarray(x, f32) if isinstance(x, tuple) else x for x in e[2:]]) for e in edits]


@pytest.mark.parametrize("tool", ["sphere", "capsule"])
def test_edits_of_the_sampled_typed_sphere(ctx, tool):
    """three bites off the typed sphere of radius 60 (they empty types {3}, {0, 2, 3} and {1} and convert 2, 2 and 7 Uniform chunks, of types
    3, 0 and 1), and two capsules through it (5 Uniform chunks of type 0, then 2 of type 3): a converted Uniform chunk spreads the type of
    its record over a plane; per-type emptied counts, removed moments with a density per type, the edited object and its mesh"""
    graph = tu.sphere60()
    probe = tu.typed_oracle(graph, 1.0, tu.SPHERE60_NOISE)
    edits = placed(SPHERE_BITES if tool == "sphere" else CAPSULES, centre_of(probe))
    census = tu.edit_census(probe, edits, DENS)
    assert len(census["emptied_types"]) >= 2 and census["converted_typed_uniform"] >= 1, census
    o, g = both(ctx, graph, 1.0, tu.SPHERE60_NOISE)
    for k, e in enumerate(edits):
        if e[0] == "s":
            ro, rg = o.absorb_sphere(e[1], e[2] + 2.0, e[2], DENS), g.absorb_sphere(e[1], e[2] + 2.0, e[2], DENS)
        else:
            ro, rg = o.absorb_capsule(e[1], e[2], e[3] + 2.0, e[3], DENS), g.absorb_capsule(e[1], e[2], e[3] + 2.0, e[3], DENS)
        assert (rg["touched_chunks"], rg["removed_chunks"]) == (ro["touched_chunks"], ro["removed_chunks"])
        np.testing.assert_array_equal(rg["emptied_by_type"], ro["emptied_by_type"])
        np.testing.assert_array_equal(rg["invalidated"], ro["invalidated"])
        scale = np.maximum(np.abs(ro["removed64"]), 1e-300)
        assert np.all(np.abs(rg["removed_moments"] - ro["removed64"]) <= 1e-5 * scale + 1e-9), (rg["removed_moments"], ro["removed64"])
        assert_typed_objects_equal(o, g, f"{tool} edit {k}: ")
    g.close()


def test_edit_many_over_a_typed_and_an_untyped_object(ctx):
    """`ivx_absorb_sphere_many` and `ivx_absorb_capsule_many` over the typed sphere and the same sphere with type 0 in one batch"""
    graph = tu.sphere60()
    probe = tu.typed_oracle(graph, 1.0, tu.SPHERE60_NOISE)
    ctr = centre_of(probe)
    spheres, capsules = placed(SPHERE_BITES, ctr), placed(CAPSULES, ctr)
    census = tu.edit_census(probe, spheres + capsules, DENS)
    assert len(census["emptied_types"]) >= 2 and census["converted_typed_uniform"] >= 1, census
    ot, gt = both(ctx, graph, 1.0, tu.SPHERE60_NOISE)
    ou = pu.oracle_from_graph(graph)
    ou.update_occupied_voxel_ranges()
    ou.compute_all_derived_state()
    gu = pu.gpu_from_graph(ctx, graph)
    gu.compute_all_derived_state()
    gu.update_occupied_voxel_ranges()
    gu.label_regions()
    os_, gs = [ot, ou], [gt, gu]
    for k, e in enumerate(spheres + capsules):
        if e[0] == "s":
            ros = [o.absorb_sphere(e[1], e[2] + 2.0, e[2], DENS) for o in os_]
            rgs = many.absorb_sphere_many(gs, [e[1]] * 2, [e[2] + 2.0] * 2, [e[2]] * 2, DENS)
        else:
            ros = [o.absorb_capsule(e[1], e[2], e[3] + 2.0, e[3], DENS) for o in os_]
            rgs = many.absorb_capsule_many(gs, [e[1]] * 2, [e[2]] * 2, [e[3] + 2.0] * 2, [e[3]] * 2, DENS)
        for j, (ro, rg) in enumerate(zip(ros, rgs)):
            np.testing.assert_array_equal(rg["invalidated"], ro["invalidated"], err_msg=f"edit {k}, object {j}")
            assert (rg["touched_chunks"], rg["removed_chunks"], rg["emptied_voxels"]) == (ro["touched_chunks"], ro["removed_chunks"], int(ro["emptied_by_type"].sum()))
            scale = np.maximum(np.abs(ro["removed64"]), 1e-300)
            assert np.all(np.abs(rg["removed_moments"] - ro["removed64"]) <= 1e-5 * scale + 1e-9), (k, j)
            assert_typed_objects_equal(os_[j], gs[j], f"edit {k}, object {j}: ")
    gt.close()
    gu.close()


# ---- d. clip, batched copies, fragments, split-offs -------------------------------------------------------------------------------------
CLIP_NOISE = (4, 0.03, 1.0, 1)


def clip_sphere():
    g = SDFGraph()
    g.add_node(SDFNode.new_sphere(26.0))
    return g


@pytest.mark.parametrize("copy", [True, False])
def test_oriented_box_through_a_typed_sphere(ctx, copy):
    """the oriented box of test_gpu_clip.test_oriented_box_through_sphere through a sphere of four types (extent 0.5): the 4 x 3 x 4-chunk
    child holds all four, and all four stay in the parent"""
    planes, aabb = rotated_box((30.0, 24.0, 31.0), np.array([14.0, 9.0, 30.0]), (1.0, 2.0, 0.5), 0.6)
    probe = tu.typed_oracle(clip_sphere(), 0.5, CLIP_NOISE)
    rc, child, _ = probe.clip_polyhedron(planes, aabb, copy=copy)
    assert rc == 1 and child.chunk_counts == (4, 3, 4)
    for obj in (child, probe):
        _, typ, flg, _, _ = obj.export_dense()
        assert len(tu.types_of_non_empty(typ, flg)) >= 2
    o, g = both(ctx, clip_sphere(), 0.5, CLIP_NOISE)
    rc_o, co, org_o = o.clip_polyhedron(planes, aabb, copy=copy)
    rc_g, cg, org_g = (g.copy_polyhedron if copy else g.extract_polyhedron)(aabb, planes)
    assert rc_g == rc_o == 1 and org_g == org_o
    assert len(assert_typed_objects_equal(co, cg, "polyhedron: ")) == 4
    assert len(assert_typed_objects_equal(o, g, "parent: ")) == 4
    cg.close()
    g.close()


def test_batched_copies_and_first_many_step_of_typed_fragments(ctx):
    """`ivx_copy_polyhedra` on the typed sphere of radius 60 — the eight Voronoi cells of a jittered 2^3 lattice and an oriented box —
    against the looped copies and the oracle's, then the fragments' first step, all in one `ivx_voxel_step_many`: every child's type plane,
    its mesh with materials and its moments under the per-type densities"""
    graph = tu.sphere60()
    o, g = both(ctx, graph, 1.0, tu.SPHERE60_NOISE)
    cc = np.asarray(o.chunk_counts, dtype=f32) * f32(16.0)
    rng = np.random.default_rng(7)
    ax = [(np.arange(2) + 0.5) * (c / 2) for c in cc]
    pts = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3) + rng.uniform(-3.0, 3.0, (8, 3))
    sets, tets = fr.fragment_plane_sets(pts.astype(f32), np.array([0, 0, 0, cc[0], cc[1], cc[2]], dtype=f32))
    tets.close()
    sets = [(s[1], s[2]) for s in sets] + [rotated_box((60.0, 70.0, 62.0), np.array([30.0, 22.0, 41.0]), (1.0, 2.0, 0.5), 0.6)]
    want = [o.clip_polyhedron(planes, bb, copy=True) for planes, bb in sets]
    assert [w[0] for w in want] == [1] * 9
    for _, co, _ in want:  # (on the oracle, before the device: several types in every child, mixed-material submeshes in its mesh)
        _, typ, flg, _, _ = co.export_dense()
        assert len(tu.types_of_non_empty(typ, flg)) >= 2
        assert tu.mixed_material_submeshes(co.mesh()) >= 1
    batched = g.copy_polyhedra([s[1] for s in sets], [s[0] for s in sets])
    kids = []
    for k, ((planes, bb), (rc_o, co, org_o), (rc_b, child_b, org_b)) in enumerate(zip(sets, want, batched)):
        rc_l, child_l, org_l = g.copy_polyhedron(bb, planes)
        assert rc_b == rc_o == rc_l and org_b == org_o == org_l
        assert_typed_objects_equal(co, child_b, f"batched child {k}: ")
        for x, y in zip(child_b.download(), child_l.download()):
            np.testing.assert_array_equal(x, y)
        child_l.close()
        kids.append(child_b)
    assert_typed_objects_equal(o, g, "parent untouched: ")
    for child in kids:
        child.set_densities(DENS)
    res = many.voxel_step_many(kids, NO_SAMPLE)
    for k, ((_, co, _), child) in enumerate(zip(want, kids)):
        assert_typed_objects_equal(co, child, f"fragment {k} after the step of all: ", with_mesh=False)
        om = co.mesh()
        gm = VoxelObjectMesh(child)
        gm.counts = res[k]["mesh"].copy()
        pos, nrm, idx, im, sub = gm.download()
        np.testing.assert_array_equal(idx, om.indices)
        np.testing.assert_array_equal(pos.view(np.uint32), om.positions.view(np.uint32))
        np.testing.assert_array_equal(nrm.view(np.uint32), om.normals.view(np.uint32))
        np.testing.assert_array_equal(im, om.index_materials)
        _, o64 = co.inertia(DENS)
        g64 = np.asarray(res[k]["moments"]["m64"], dtype=np.float64)
        assert np.all(np.abs(g64 - o64) <= 1e-5 * np.maximum(np.abs(o64), 1e-300) + 1e-12), k
        assert int(res[k]["region_count"]) == co.region_labels(False)[0]
        child.close()
    g.close()


SPLIT_NOISE = (5, 0.02, 1.0, 7)


@pytest.mark.parametrize("entry", ["any", "all"])
def test_split_off_of_typed_two_spheres(ctx, entry):
    """`extract_any_disconnected_region` / `extract_all_disconnected_regions` on two spheres of five types (extent 0.5): the child's and the
    parent's type planes"""
    graph = scenes.two_spheres_scene(25.0, 60.0)
    probe = tu.typed_oracle(graph, 0.5, SPLIT_NOISE)
    rc, child, _ = probe.split_off_smallest_region()
    assert rc == 1
    for obj in (child, probe):
        _, typ, flg, _, _ = obj.export_dense()
        assert len(tu.types_of_non_empty(typ, flg)) >= 2
    o, g = both(ctx, graph, 0.5, SPLIT_NOISE)
    rc_o, co, org_o = o.split_off_smallest_region()
    if entry == "any":
        rc_g, cg, org_g, moved = g.extract_any_disconnected_region()
    else:
        got = g.extract_all_disconnected_regions()
        assert len(got) == 1
        rc_g, cg, org_g, moved = got[0]
    assert rc_g == rc_o == 1 and tuple(int(x) for x in org_g) == tuple(org_o)
    assert len(assert_typed_objects_equal(co, cg, "child: ")) >= 2
    assert len(assert_typed_objects_equal(o, g, "parent: ")) >= 2
    assert int(moved["voxel_count"]) == int(np.count_nonzero((co.export_dense()[2] & 1) == 0))
    assert o.split_off_smallest_region()[0] == 0 and g.extract_any_disconnected_region()[0] == 0
    cg.close()
    g.close()


# ---- e. `_many` step with the sample stage ---------------------------------------------------------------------------------------------
def test_step_many_samples_a_typed_and_a_same_type_program(ctx):
    """`ivx_voxel_step_many` with IVX_STAGE_SAMPLE over a resident program with noise types and one with a single type (5) in one batch, then
    batches without the sample stage: each object against its oracle, and against the same object stepped alone"""
    graph = tu.sphere60()
    oracles = [tu.typed_oracle(graph, 1.0, tu.SPHERE60_NOISE), pu.oracle_from_graph(scenes.asteroid_scene(0.4), 1.0, 5)]
    oracles[1].update_occupied_voxel_ranges()
    oracles[1].compute_all_derived_state()
    _, typ, flg, _, info = oracles[0].export_dense()
    assert len(tu.types_of_non_empty(typ, flg)) == 4 and ((info["kind"] == 1) & (info["uniform_type"] != 0)).any()
    assert tu.mixed_material_submeshes(oracles[0].mesh()) >= 1
    gens = [SDFVoxelGenerator(1.0, graph, tu.noise_generator(tu.SPHERE60_NOISE)), SDFVoxelGenerator(1.0, scenes.asteroid_scene(0.4), 5)]

    def resident():
        objs = []
        for gen in gens:
            obj = VoxelObject(ctx, gen.chunk_counts(), 1.0)
            obj.set_sdf_program(gen)
            obj.set_densities(DENS)
            objs.append(obj)
        return objs

    batch, alone = resident(), resident()
    for stages in (capi.STAGE_ALL, NO_SAMPLE, NO_SAMPLE, capi.STAGE_ALL):
        res = many.voxel_step_many(batch, stages)
        for k, (o, g, a) in enumerate(zip(oracles, batch, alone)):
            parity = pu.step_parity(o, g, res[k], DENS)
            assert parity["equal"], (k, stages, parity)
            ra = a.step(stages)
            assert pu.step_parity(o, a, ra, DENS)["equal"]
            for x, y in zip(g.download(), a.download()):
                np.testing.assert_array_equal(x, y)
            ma, mb = VoxelObjectMesh(g), VoxelObjectMesh(a)
            ma.counts, mb.counts = res[k]["mesh"].copy(), ra["mesh"].copy()
            for x, y in zip(ma.download(), mb.download()):
                np.testing.assert_array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    for g in batch + alone:
        g.close()
