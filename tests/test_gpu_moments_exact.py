"""Every producer of the ten mass moments against the exact restatement (tests/moments_ref.py) over the voxel bytes downloaded from the
device: the stand-alone chain (loop form, closed forms of Uniform chunks), the object's own step (wave form; the step's copies of the closed
forms), the workgroup form of the derive sweep (byte-table form and loop form, chosen per wave), the slab protocol with its x offset and its
host sum, the removed moments of edits and of mutual absorption (f64 atomics), the dense-moments batch, the per-region moments and the moved
moments of a split. The gate is `assert_moments`: bit for bit (2^-52 on the 1/3 terms) where every intermediate is an integer below 2^53,
(n + 64) 2^-53 relative otherwise — one dropped voxel of any of these grids is orders of magnitude above either.

Every case runs with integer and with fractional densities, at extents 1.0 and 0.3, and twice: the kernels that sum in a fixed order must give
the same bits both times, the ones that add chunks by f64 atomics must do so in the exact case (otherwise the test prints whether they did)."""
import numpy as np
import pytest

import moments_ref as mr
import oracle_lib as ol
from fractions import Fraction
from impact_amd import capi, many, scenes
from impact_amd.voxel import GradientNoiseVoxelTypeGenerator, SDFVoxelGenerator, VoxelObject, VoxelObjectInertialPropertyManager

pytestmark = pytest.mark.gpu

NO_SAMPLE = capi.STAGE_ALL & ~capi.STAGE_SAMPLE
EXTENTS = [1.0, 0.3]
_sums = {}


def sums_of(flags, types, cc, mask=None, x_off=0):
    """integer_sums, kept per set of bytes: one set of voxels serves both density tables and both extents"""
    import hashlib

    h = hashlib.sha1(np.ascontiguousarray(flags).view(np.uint8)).digest() + hashlib.sha1(np.ascontiguousarray(types).view(np.uint8)).digest()
    if mask is not None:
        h += hashlib.sha1(np.ascontiguousarray(mask).view(np.uint8)).digest()
    key = (h, tuple(cc), int(x_off))
    if key not in _sums:
        _sums[key] = mr.integer_sums(flags, types, cc, mask, x_off)
    return _sums[key]


def planes(g):
    _, typ, flg, _, _ = g.download(sdf=False, labels=False, info=False)
    return flg, typ


def exact_of(g, dens, mask=None, bytes_=None):
    flg, typ = planes(g) if bytes_ is None else bytes_
    return mr.moments_of_sums(sums_of(flg, typ, g.chunk_counts, mask, g.x_chunk_offset), dens, g.voxel_extent)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64).copy()


def check(got, ex, what, parts=1):
    m, n, exact = ex
    print("%s: n_terms %d exact_case %s rel err %.3e" % (what, n, exact, mr.rel_err(got, m)))
    mr.assert_moments(got, m, n, exact, what, parts)


def same_bits(a, b, what):
    assert np.array_equal(bits(a), bits(b)), (what, np.asarray(a), np.asarray(b))


def kinds(g):
    return g.download(sdf=False, types=False, flags=False, labels=False)[4]["kind"]


def standalone(g, dens):
    return VoxelObjectInertialPropertyManager.initialized_from(g, dens).m64


def generated(ctx, graph, extent, vtype=0):
    g = VoxelObject.generate_without_derived_state(ctx, SDFVoxelGenerator(extent, graph, vtype))
    g.compute_all_derived_state()
    return g


def uploaded(ctx, cc, sd, ty, extent):
    g = VoxelObject.from_dense(ctx, cc, sd, ty, extent)
    g.compute_all_derived_state()
    return g


def sampled(ctx, graph, extent, vtype):
    gen = SDFVoxelGenerator(extent, graph, vtype)
    obj = VoxelObject(ctx, gen.chunk_counts(), extent)
    obj.set_sdf_program(gen)
    return obj


# ---- a. the stand-alone chain: k_inertia_dense -> k_inertia_sum -> k_inertia_final ----------------------------------------------------------
def _rod(thick):
    """the box rod of test_long_thin_rod_more_than_64_chunks along x, or a capsule of radius 20 and the same length along x"""
    from impact_amd.sdf_graph import SDFGraph, SDFNode
    from test_gpu_parity import _boxes_along

    if not thick:
        return _boxes_along(0, [0.0], long_half=550.0)
    g = SDFGraph()
    c = g.add_node(SDFNode.new_capsule(1060.0, 20.0))
    g.add_node(SDFNode.new_rotation_from_axis_angle(c, (0.0, 0.0, 1.0), 1.5707963267948966))  # capsule axis y -> x
    return g


@pytest.mark.parametrize("extent", EXTENTS)
@pytest.mark.parametrize("grid", ["upload", "sphere", "rod", "thick_rod"])
def test_standalone_chain(ctx, grid, extent):
    """upload: five types per voxel, the loop form (no Uniform chunk but the solid one). sphere: Uniform chunks, the closed forms. rod: the
    rod of test_long_thin_rod_more_than_64_chunks along x — 69 chunks, I up to 1100, but 10 voxels thick: no Uniform chunk (nor has a box
    of any thickness: deep inside a box the sampler leaves -127, not the -128 of a Uniform chunk); thick_rod: a capsule of radius 20 and the
    same length along x, whose middle column is 67 Uniform chunks: the closed forms at large I."""
    if grid == "upload":
        cc, sd, ty = mr.random_upload_grid(0, 0.5)
        g = uploaded(ctx, cc, sd, ty, extent)
        assert len(np.unique(planes(g)[1][(planes(g)[0] & 1) == 0])) == 5
    else:
        g = generated(ctx, {"sphere": lambda: scenes.sphere_scene(30.0), "rod": lambda: _rod(False), "thick_rod": lambda: _rod(True)}[grid](), extent)
        n_uniform = int(np.count_nonzero(kinds(g) == 1))
        if grid == "sphere":
            assert n_uniform >= 1
        if grid == "rod":
            assert g.chunk_counts == (69, 1, 1)
        if grid == "thick_rod":
            assert g.chunk_counts == (69, 3, 3) and n_uniform >= 60
    for kind, dens in mr.DENSITY_SETS.items():
        m1 = standalone(g, dens)
        m2 = standalone(g, dens)
        same_bits(m1, m2, (grid, kind))
        check(m1, exact_of(g, dens), "standalone %s %s %g" % (grid, kind, extent))
    g.close()


# ---- b. the object's own step ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent", EXTENTS)
@pytest.mark.parametrize("types", ["type3", "type0", "noise"])
def test_own_step(ctx, types, extent):
    """asteroid_scene(0.5) (32 Uniform, 245 NonUniform chunks) stepped by `ivx_voxel_step(STAGE_ALL)`, twice (the second step starts from the
    first one's list). One type (3, then 0): the sweep is k_derive_wave, whose moments are moments_row_sums_one_type + moments_rows_wave with
    the type from the sampler or the chunk record. Gradient-noise types: the types are in the type plane alone, the sweep is k_derive<false>
    (from the planes, a chunk per workgroup), whose moments are chunk_moments_rows_tab — table form or loop form per wave. Either way the
    chunk slots are summed by role_inertia_sum / role_inertia_final, the step's copies of the closed forms."""
    vtype = {"type3": 3, "type0": 0, "noise": GradientNoiseVoxelTypeGenerator(4, 0.02, 1.0, 0)}[types]
    obj = sampled(ctx, scenes.asteroid_scene(0.5), extent, vtype)
    for kind, dens in mr.DENSITY_SETS.items():
        obj.set_densities(dens)
        got = [np.array(obj.step(capi.STAGE_ALL)["moments"]["m64"], dtype=np.float64) for _ in range(2)]
        same_bits(got[0], got[1], (types, kind))
        flg, typ = planes(obj)
        present = np.unique(typ[(flg & 1) == 0])
        if types == "noise":
            assert len(present) >= 2
        else:
            assert present.tolist() == [int(vtype)]
        k = kinds(obj)
        assert np.count_nonzero(k == 1) >= 1 and np.count_nonzero(k == 2) >= 100
        check(got[0], exact_of(obj, dens, bytes_=(flg, typ)), "own step %s %s %g" % (types, kind, extent))
    obj.close()


# ---- c. the workgroup form of the sweep: a `_many` step of uploaded grids --------------------------------------------------------------------
def random_sign_grid(seed, plane):
    """2 x 2 x 2 chunks of independent random signs (every chunk NonUniform, some tens of regions each), and a type plane: "ij" a type per
    row (i, j), "voxel" a type per voxel, "one_byte" as ij with one differing byte in one row per chunk, "empty_rows" as ij with three rows per
    chunk emptied and given type 0xFF -> (cc, sdf tiled, type tiled, row masks [32, 32, 2])"""
    rng = np.random.default_rng(seed)
    sd = np.where(rng.random((32, 32, 32)) < 0.5, -40, 40).astype(np.int8)
    ty = np.broadcast_to(rng.integers(0, 200, (32, 32, 1)), sd.shape).astype(np.uint8)
    if plane == "voxel":
        ty = rng.integers(0, 200, sd.shape).astype(np.uint8)
    for ci in range(2):
        for cj in range(2):
            for ck in range(2):
                i, j, k = 16 * ci + 5 + ck, 16 * cj + 9 - ci, 16 * ck
                if plane == "one_byte":
                    sd[i, j, k + 6] = -40  # (a non-empty voxel, so that the byte counts)
                    ty[i, j, k + 6] = 201
                if plane == "empty_rows":
                    for r in range(3):
                        sd[i + r, j + 2 * r, k:k + 16] = 40
                        ty[i + r, j + 2 * r, k:k + 16] = 0xFF
    masks = ((sd < 0).astype(np.int64).reshape(32, 32, 2, 16) << np.arange(16)).sum(-1)
    return (2, 2, 2), ol.dense_to_tiled(sd), ol.dense_to_tiled(ty), masks


@pytest.mark.parametrize("extent", EXTENTS)
@pytest.mark.parametrize("plane", ["ij", "voxel", "one_byte", "empty_rows"])
def test_workgroup_form(ctx, plane, extent):
    """k_derive's moments (chunk_moments_rows_tab) through a `_many` step of two uploaded grids without the sample stage. ij: every row has one
    type, every wave takes the byte-table form — and the result equals the stand-alone chain's (the loop form) bit for bit in the exact
    case, the code's own claim. voxel: every wave takes the loop form. one_byte: one wave per chunk takes the loop beside table waves.
    empty_rows: all-empty rows of type 0xFF with densities[255] = 1e30 — a zero mask times any density is zero. The low and the high bytes of
    the row masks take all 256 values in every grid: every entry of the byte table is read."""
    grids = []
    for seed in (11, 13):
        cc, sd, ty, masks = random_sign_grid(seed, plane)
        assert len(np.unique(masks & 255)) == 256 and len(np.unique(masks >> 8)) == 256
        if plane == "empty_rows":
            assert np.count_nonzero(masks == 0) >= 24
        grids.append(VoxelObject.from_dense(ctx, cc, sd, ty, extent))
    for kind, dens in mr.DENSITY_SETS.items():
        if plane == "empty_rows":
            dens = dens.copy()
            dens[255] = np.float32(1e30)
        for g in grids:
            g.set_densities(dens)
        res = [many.voxel_step_many(grids, NO_SAMPLE) for _ in range(2)]
        for q, g in enumerate(grids):
            got = np.array(res[0][q]["moments"]["m64"], dtype=np.float64)
            same_bits(got, res[1][q]["moments"]["m64"], (plane, kind, q))
            assert np.all(kinds(g) == 2)
            ex = exact_of(g, dens)
            check(got, ex, "workgroup form %s %s %g grid %d" % (plane, kind, extent, q))
            if plane == "ij" and ex[2]:
                same_bits(got, standalone(g, dens), "table form against the loop form")
    for g in grids:
        g.close()


# ---- d. slabs ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent", EXTENTS)
@pytest.mark.parametrize("world", [2, 3])
def test_slabs(ctx, world, extent):
    """The type-3 asteroid of test_own_step in x-slabs, in process. Python driver: every slab's own moments (words 18..27 of its record)
    against the restatement of its voxels at their global x. Native driver: the host sum of the slabs' moments (slab_comm.cpp) against the
    whole object — a sum of `world` separately scaled results, hence `parts=world`."""
    import torch

    from impact_amd.distributed import NativeComm, NativeSlabStepper, SlabStepper, native_step, run_slabs_in_process

    graph = scenes.asteroid_scene(0.5)
    for kind, dens in mr.DENSITY_SETS.items():
        # python driver: per-slab records
        steppers = [SlabStepper(ctx, graph, dens, r, world, torch, extent, 3) for r in range(world)]
        try:
            recs = []
            for _ in range(2):
                results = run_slabs_in_process(steppers)
                recs.append([s.record.t[18:28].cpu().numpy().view(np.float64).copy() for s in steppers])
            total, n_total, exact_all = [Fraction(0)] * 10, 0, True
            for r, s in enumerate(steppers):
                assert s.obj.x_chunk_offset == s.x_range[0]
                same_bits(recs[0][r], recs[1][r], (kind, r))
                ex = exact_of(s.obj, dens)
                check(recs[0][r], ex, "slab %d of %d %s %g" % (r, world, kind, extent))
                total = [a + b for a, b in zip(total, ex[0])]
                n_total += ex[1]
                exact_all = exact_all and ex[2]
            assert n_total > 400000
            check(results[0].moments, (total, n_total, exact_all), "python sum of %d slabs %s %g" % (world, kind, extent), parts=world)
        finally:
            for s in steppers:
                s.close()
        # native driver: the library's host sum
        comm = NativeComm(ctx, world, local=True)
        steppers = [NativeSlabStepper(ctx, comm, graph, dens, r, extent, 3) for r in range(world)]
        try:
            sums = [np.array(native_step(steppers)[0].moments, dtype=np.float64) for _ in range(2)]
            same_bits(sums[0], sums[1], (kind, "native"))
            check(sums[0], (total, n_total, exact_all), "native sum of %d slabs %s %g" % (world, kind, extent), parts=world)
        finally:
            for s in steppers:
                s.close()
            comm.close()


# ---- e. edits ----------------------------------------------------------------------------------------------------------------------------------
def prepared(g):
    """as the edit tests' `both` leaves an object"""
    g.update_occupied_voxel_ranges()
    g.label_regions()
    return g


def centre_of(g):
    return np.array([0.5 * (a + b) for a, b in g.update_occupied_voxel_ranges()], dtype=np.float32)


def edit_and_check(make, edit, dens, what, expect):
    """`make()` -> a fresh prepared object, `edit(g)` -> the result dict of an absorb call. Twice; -> nothing"""
    runs = []
    for _ in range(2):
        g = make()
        flg0, typ0 = planes(g)
        info0 = kinds(g).copy()
        before = standalone(g, dens)
        ex0 = exact_of(g, dens, bytes_=(flg0, typ0))
        check(before, ex0, what + " before")
        r = edit(g)
        flg1, typ1 = planes(g)
        emptied = ((flg0 & 1) == 0) & ((flg1 & 1) != 0)
        assert int(emptied.sum()) == r["emptied_voxels"]
        exr = exact_of(g, dens, mask=emptied, bytes_=(flg0, typ0))
        removed = r["removed_moments"]
        if expect == "miss":
            assert r["emptied_voxels"] == 0 and r["touched_chunks"] == 0
            assert np.array_equal(bits(removed), bits(np.zeros(10))), removed  # ten +0.0
        else:
            assert r["emptied_voxels"] > 300
            chunks = np.unique(np.flatnonzero(emptied) >> 12)
            if expect == "corner":
                assert len(chunks) >= 8 and len(np.unique(typ0[emptied])) >= 3
            if expect == "uniform":
                assert np.any(info0[chunks] == 1)
        check(removed, exr, what + " removed")
        after = standalone(g, dens)
        ex1 = exact_of(g, dens, bytes_=(flg1, typ1))
        check(after, ex1, what + " after")
        # conservation in Fractions: before - after = removed within the three bounds added
        for q in range(10):
            lim = sum(mr.bound(e[0][q], e[1], e[2], q) for e in (ex0, ex1, exr))
            assert abs(Fraction(float(before[q])) - Fraction(float(after[q])) - Fraction(float(removed[q]))) <= lim, (what, q)
        runs.append((np.array(removed), exr[2]))
        g.close()
    differ = not np.array_equal(bits(runs[0][0]), bits(runs[1][0]))
    print("%s: removed moments of two runs %s" % (what, "DIFFER" if differ else "equal bit for bit"))
    if runs[0][1]:
        assert not differ, what


@pytest.mark.parametrize("extent", EXTENTS)
@pytest.mark.parametrize("tool", ["sphere", "capsule"])
@pytest.mark.parametrize("case", ["corner", "uniform", "miss"])
def test_edit_removed_moments(ctx, case, tool, extent):
    """removed_moments of absorb_sphere / absorb_capsule (k_absorb: chunk_moments_rows over the `emptied` masks, chunks added by f64 atomics)
    against the restatement over (non-empty before) & (empty after) with the types from before: a bite across the chunk corner (16, 16, 16)
    of the five-type upload, a bite into a Uniform chunk of the sphere, and a miss."""
    if case == "corner":
        cc, sd, ty = mr.random_upload_grid(0, 0.5)
        make = lambda: prepared(uploaded(ctx, cc, sd, ty, extent))  # noqa: E731
        c, off = np.array([16.5, 15.0, 17.0], np.float32), np.zeros(3, np.float32)
    else:
        make = lambda: prepared(generated(ctx, scenes.sphere_scene(30.0), extent))  # noqa: E731
        g0 = make()
        c = centre_of(g0)
        g0.close()
        off = np.array([200.0, 0.0, 0.0], np.float32) if case == "miss" else np.array([3.25, -2.5, 1.75], np.float32)
    for kind, dens in mr.DENSITY_SETS.items():
        if tool == "sphere":
            edit = lambda g: g.absorb_sphere(c + off, 11.0, 9.0, dens)  # noqa: E731
        else:
            edit = lambda g: g.absorb_capsule(c + off - np.array([3.0, 2.0, 1.0], np.float32), np.array([6.0, 4.0, 2.0], np.float32), 9.0, 7.0, dens)  # noqa: E731
        edit_and_check(make, edit, dens, "%s %s %s %g" % (tool, case, kind, extent), case)


@pytest.mark.parametrize("extent", EXTENTS)
def test_mutual_absorption_removed_moments(ctx, extent):
    """mutual absorption's removed moments (voxel_collision_api.hip) of both objects, at a pose of test_gpu_mutual_sequences' harness: a box and
    a sphere, both turned, the centres 0.7 (ra + rb) apart"""
    import test_gpu_collide as tc
    from test_gpu_mutual_sequences import random_quaternion

    rng = np.random.default_rng(101)
    qa, qb = random_quaternion(rng, 3), random_quaternion(rng, 2)
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    for kind, dens in mr.DENSITY_SETS.items():
        runs = []
        for _ in range(2):
            GA = prepared(generated(ctx, scenes.box_scene((44.0, 20.0, 30.0)), extent, 2))
            GB = prepared(generated(ctx, scenes.sphere_scene(16.0), extent, 5))
            occ_a, occ_b = GA.update_occupied_voxel_ranges(), GB.update_occupied_voxel_ranges()
            ca = (np.array([0.5 * (a + b) for a, b in occ_a]) * extent).astype(np.float32)
            cb = (np.array([0.5 * (a + b) for a, b in occ_b]) * extent).astype(np.float32)
            ra = 0.5 * min(b - a for a, b in occ_a) * extent
            rb = 0.5 * min(b - a for a, b in occ_b) * extent
            ta = tc.placed(ca, qa, [0.0, 0.0, 0.0])
            tb = tc.placed(cb, qb, d * (ra + rb) * 0.7)
            before = [planes(GA), planes(GB)]
            res = GA.absorb_mutual(qa, ta, GB, qb, tb, 1.0, dens, dens[::-1].copy())
            out = []
            for g, r, b0, dd, name in ((GA, res[0], before[0], dens, "A"), (GB, res[1], before[1], dens[::-1].copy(), "B")):
                flg1, _ = planes(g)
                emptied = ((b0[0] & 1) == 0) & ((flg1 & 1) != 0)
                assert int(emptied.sum()) == r["emptied_voxels"] > 50
                ex = exact_of(g, dd, mask=emptied, bytes_=b0)
                check(r["removed_moments"], ex, "mutual %s %s %g" % (name, kind, extent))
                out.append((np.array(r["removed_moments"]), ex[2]))
            runs.append(out)
            GA.close()
            GB.close()
        for q in range(2):
            differ = not np.array_equal(bits(runs[0][q][0]), bits(runs[1][q][0]))
            print("mutual %s %s %g: two runs %s" % ("AB"[q], kind, extent, "DIFFER" if differ else "equal bit for bit"))
            if runs[0][q][1]:
                assert not differ


# ---- f. the dense-moments batch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent", EXTENTS)
def test_dense_moments_batch(ctx, extent):
    """k_inertia_dense_many: `ivx_voxel_step_many(STAGE_INERTIA)` over three grids of 18, 27 and 8 chunks, each bit for bit what the same grid
    gives alone (k_inertia_dense)"""
    cc, sd, ty = mr.random_upload_grid(0, 0.5)
    gs = [VoxelObject.from_dense(ctx, cc, sd, ty, extent), sampled(ctx, scenes.sphere_scene(20.0), extent, 4), sampled(ctx, scenes.box_scene(), extent, 1)]
    assert len({g.n_chunks for g in gs}) == 3
    for kind, dens in mr.DENSITY_SETS.items():
        for q, g in enumerate(gs):
            g.set_densities(dens)
            g.step(NO_SAMPLE if q == 0 else capi.STAGE_ALL)
        res = [many.voxel_step_many(gs, capi.STAGE_INERTIA) for _ in range(2)]
        for q, g in enumerate(gs):
            got = np.array(res[0][q]["moments"]["m64"], dtype=np.float64)
            same_bits(got, res[1][q]["moments"]["m64"], (kind, q))
            same_bits(got, g.step(capi.STAGE_INERTIA)["moments"]["m64"], ("alone", kind, q))
            check(got, exact_of(g, dens), "batch grid %d %s %g" % (q, kind, extent))
    for g in gs:
        g.close()


# ---- g. regions and split ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent", EXTENTS)
def test_region_moments(ctx, extent):
    """k_region_stats (per-region f64 atomics) on the many-regions scene: every region's ten moments and voxel count against the restatement
    over its mask from region_labels(), and the sum over the regions (in Fractions) against the whole within the regions' bounds added"""
    from test_gpu_derive_wave import many_regions_scene

    g = generated(ctx, many_regions_scene(), extent, 6)
    lab = g.region_labels()
    flg, typ = planes(g)
    n = g.count_regions()
    assert n > 20 and set(np.unique(lab).tolist()) == set(range(n)) | {0xFFFFFFFF}
    assert np.array_equal(lab != 0xFFFFFFFF, (flg & 1) == 0)
    for kind, dens in mr.DENSITY_SETS.items():
        runs = [g.describe_regions(dens) for _ in range(2)]
        desc = runs[0]
        assert len(desc) == n
        total, lim, exact_all = [Fraction(0)] * 10, [Fraction(0)] * 10, True
        for r in range(n):
            ex = exact_of(g, dens, mask=lab == r, bytes_=(flg, typ))
            assert int(desc[r]["voxel_count"]) == ex[1] > 0
            mr.assert_moments(desc[r]["moments"], ex[0], ex[1], ex[2], "region %d %s %g" % (r, kind, extent))
            total = [t + Fraction(float(v)) for t, v in zip(total, desc[r]["moments"])]
            lim = [l + mr.bound(ex[0][q], ex[1], ex[2], q) for q, l in enumerate(lim)]
            exact_all = exact_all and ex[2]
        whole = exact_of(g, dens, bytes_=(flg, typ))
        for q in range(10):
            assert abs(total[q] - whole[0][q]) <= lim[q], (kind, q)
        differ = not np.array_equal(bits(runs[0]["moments"]), bits(runs[1]["moments"]))
        print("regions %s %g: %d regions, two runs %s" % (kind, extent, n, "DIFFER" if differ else "equal bit for bit"))
        if exact_all:
            assert not differ
    g.close()


@pytest.mark.parametrize("extent", EXTENTS)
def test_split_moments(ctx, extent):
    """the split case of test_gpu_split (two spheres): all ten moved moments over the region's mask in the parent's frame — the voxels that
    were non-empty before and are empty after —, the child's own moments over its downloaded grid, and the parent's remainder"""
    for kind, dens in mr.DENSITY_SETS.items():
        runs = []
        for _ in range(2):
            g = generated(ctx, scenes.two_spheres_scene(), extent, 2)
            g.set_densities(dens)
            assert g.count_regions() == 2
            b0 = planes(g)
            rc, child, origin, moved = g.extract_any_disconnected_region()
            assert rc == 1
            flg1, typ1 = planes(g)
            gone = ((b0[0] & 1) == 0) & ((flg1 & 1) != 0)
            ex = exact_of(g, dens, mask=gone, bytes_=b0)
            assert int(moved["voxel_count"]) == ex[1] > 10000
            check(moved["moments"], ex, "moved %s %g" % (kind, extent))
            check(standalone(child, dens), exact_of(child, dens), "child %s %g" % (kind, extent))
            check(standalone(g, dens), exact_of(g, dens, bytes_=(flg1, typ1)), "remainder %s %g" % (kind, extent))
            runs.append((np.array(moved["moments"]), ex[2]))
            child.close()
            g.close()
        differ = not np.array_equal(bits(runs[0][0]), bits(runs[1][0]))
        print("split %s %g: two runs %s" % (kind, extent, "DIFFER" if differ else "equal bit for bit"))
        if runs[0][1]:
            assert not differ
