"""The launch recorder's merge rule and its twins on the smallest objects on which every twinned stage has work (csrc/many.hpp, many_plan.hpp):
spheres of radius 6 and 12 voxels, 1x1x1 and 2x2x2 chunks. The expected launch counts follow from the rule — objects whose chains hold the same
kernels at the same positions share every launch, a chain that ends early takes part as far as it goes — not from a measurement; the results
are held, byte for byte, to those of the unbatched calls (but for an edit's removed moments, atomic sums of doubles whose order no call
fixes: those to the relative 1e-5 that test_gpu_many.py holds them to). A twin launched with another thread count than its body was written for (the two
64-thread ones, the step's and the probes' gathers, beside the 256-thread ones of every file) would show here as wrong bytes."""
import numpy as np
import pytest

import parity_util as pu
from impact_amd import capi, many, scenes
from impact_amd.voxel import VoxelObjectMesh

pytestmark = pytest.mark.gpu

DENS = np.linspace(0.5, 2.0, 256).astype(np.float32)
STAGES = capi.STAGE_DERIVE | capi.STAGE_REGIONS | capi.STAGE_REMESH | capi.STAGE_INERTIA
IDENT, ZERO, RESP = np.array([0, 0, 0, 1], dtype=np.float32), np.zeros(3, dtype=np.float32), (0.25, 0.6, 0.4)


def fresh(ctx, radius):
    """a sphere stepped once on its own (the first step allocates — mesh arrays, result block — with waits that are not the recorder's business),
    no stage slot timed: a recorded step cannot stamp, and the event records it would take instead are stream operations without a twin, each
    of which sends out what has been recorded (as `ivx_voxel_step_many` steps: step_enqueue_untimed)"""
    g = pu.gpu_from_graph(ctx, scenes.sphere_scene(radius))
    assert g.chunk_counts == ((1, 1, 1) if radius == 6.0 else (2, 2, 2))
    g.set_densities(DENS)
    g.set_stage_timing(0)
    g.step(STAGES)
    return g


def prepared(ctx, radius):
    """a sphere with derived state, occupied ranges, regions and a mesh: what the contact, probe and sync calls ask of an object"""
    g = pu.gpu_from_graph(ctx, scenes.sphere_scene(radius))
    g.compute_all_derived_state()
    g.update_occupied_voxel_ranges()
    g.label_regions()
    g.mesh = VoxelObjectMesh.create(g)
    return g


def placed(com, world_pos):
    """world -> object translation that puts the centre of mass of an object that is not turned at `world_pos`"""
    return (com.astype(np.float64) - np.asarray(world_pos, dtype=np.float64)).astype(np.float32)


def state(g, res, stages):
    """what a step of `stages` leaves: the dense planes and chunk records, and per stage the mesh, the moments, the regions — as bytes"""
    out = [np.ascontiguousarray(a).tobytes() for a in g.download()]
    if stages & capi.STAGE_REMESH:
        m = VoxelObjectMesh(g)
        m.counts = res["mesh"].copy()
        out += [np.ascontiguousarray(a).tobytes() for a in m.download()]
    if stages & capi.STAGE_INERTIA:
        out.append(np.asarray(res["moments"]["m64"], dtype=np.float64).tobytes())
    if stages & capi.STAGE_REGIONS:
        out += [int(res["region_count"]), g.region_labels().tobytes()]
    return out


def stats(ctx):
    out = np.zeros(3, dtype=np.uint64)
    capi.check(capi.lib().ivx_many_stats(ctx.h, capi.ptr(out)))
    return [int(x) for x in out]


def bracket(ctx, objs, stages):
    """the objects' steps enqueued inside one bare bracket -> launches recorded, merged launches issued, flushes, the steps' results"""
    lib = capi.lib()
    s0 = stats(ctx)
    capi.check(lib.ivx_many_begin(ctx.h))
    for g, st in zip(objs, stages):
        g.step_enqueue(st)
    capi.check(lib.ivx_many_flush(ctx.h))
    s1 = stats(ctx)
    return [b - a for a, b in zip(s0, s1)], [g.step_collect().copy() for g in objs]


@pytest.mark.parametrize("radius", [6.0, 12.0])
def test_identical_objects_share_every_launch(ctx, radius):
    """one object alone in a bracket, then four like it in one bracket: four times the launches recorded, the same number issued"""
    ref, one, four = fresh(ctx, radius), fresh(ctx, radius), [fresh(ctx, radius) for _ in range(4)]
    want = state(ref, ref.step(STAGES), STAGES)
    (rec1, iss1, fl1), res1 = bracket(ctx, [one], [STAGES])
    (rec4, iss4, fl4), res4 = bracket(ctx, four, [STAGES] * 4)
    print(f"radius {radius}: alone {rec1} recorded, {iss1} issued, {fl1} flushes; four {rec4} recorded, {iss4} issued, {fl4} flushes")
    assert rec1 > 0 and 0 < iss1 <= rec1
    assert rec4 == 4 * rec1
    assert iss4 == iss1
    assert state(one, res1[0], STAGES) == want
    for k, (g, r) in enumerate(zip(four, res4)):
        assert state(g, r, STAGES) == want, f"object {k} of four"
    for g in [ref, one] + four:
        g.close()


def test_a_shorter_chain_takes_part_as_far_as_it_goes(ctx):
    """three objects of two sizes in one bracket, the middle one asked for the derive sweep and the moments only: no more launches issued than
    for the longest chain alone"""
    radii, stages = [12.0, 6.0, 12.0], [STAGES, capi.STAGE_DERIVE | capi.STAGE_INERTIA, STAGES]
    refs, objs, alone = [fresh(ctx, r) for r in radii], [fresh(ctx, r) for r in radii], fresh(ctx, 12.0)
    want = [state(g, g.step(st), st) for g, st in zip(refs, stages)]
    (rec_l, iss_l, fl_l), _ = bracket(ctx, [alone], [STAGES])
    (rec, iss, fl), res = bracket(ctx, objs, stages)
    print(f"longest chain alone {rec_l} recorded, {iss_l} issued, {fl_l} flushes; the three {rec} recorded, {iss} issued, {fl} flushes")
    assert rec_l < rec < 3 * rec_l
    assert iss == iss_l
    for k, (g, r, st) in enumerate(zip(objs, res, stages)):
        assert state(g, r, st) == want[k], f"object {k}"
    for g in refs + objs + [alone]:
        g.close()


def test_twins_of_every_file_against_the_single_object_calls(ctx):
    """batches of two and three of the same small objects through the calls that record the twins of each file — clip (split.hip), the
    collidable contacts (contacts.hip), the mutual contacts and the probe sync with its 64-thread gather (collide.hip), the absorbing sphere
    (edit.hip), the mesh sync (surface_nets.hip), the moment sweep (inertia.hip) and the whole step with its 64-thread gather (derive.hip,
    step_fused.hip) — next to the same objects through the single-object calls"""
    radii = [6.0, 12.0, 12.0]
    objs, refs = [prepared(ctx, r) for r in radii], [prepared(ctx, r) for r in radii]
    for g in objs + refs:
        g.set_densities(DENS)
        g.collision_probes_recompute()
    # clip: the two halves of the larger sphere, copied out together and one by one
    box = np.array([0, 0, 0, 32, 32, 32], dtype=np.float32)
    halves = [np.array([[1, 0, 0, 16]], dtype=np.float32), np.array([[-1, 0, 0, -16]], dtype=np.float32)]
    together, singly = objs[1].copy_polyhedra([box, box], halves), [refs[1].copy_polyhedron(box, h) for h in halves]
    for k, ((rc_t, child_t, off_t), (rc_s, child_s, off_s)) in enumerate(zip(together, singly)):
        assert rc_t == rc_s == 1 and off_t == off_s, f"half {k}"
        for x, y in zip(child_t.download(), child_s.download()):
            np.testing.assert_array_equal(x, y, err_msg=f"half {k}")
        child_t.close()
        child_s.close()
    # a ball at every object's +x face
    qs = many.collidable_queries(3)
    qs["mode"], qs["shape1"], qs["response"], qs["rotation_xyzw"] = 0, 3.0, RESP, IDENT
    qs["collidable_id_a"], qs["collidable_id_b"], qs["body_a"], qs["body_b"] = (40, 41, 42), 7, (0, 1, 2), 0x80000000
    coms = []
    for k, g in enumerate(objs):
        occ = np.array(g.update_occupied_voxel_ranges(), dtype=np.float64)
        centre, half = 0.5 * (occ[:, 0] + occ[:, 1]), 0.5 * (occ[:, 1] - occ[:, 0])
        qs["shape3"][k] = (centre + [half[0] + 1.0, 0.0, 0.0]).astype(np.float32)
        coms.append(centre.astype(np.float32))
    got, off = many.voxel_object_contacts_many(objs, qs)
    for k, g in enumerate(refs):
        single = g.sphere_contacts(IDENT, ZERO, qs["shape3"][k], 3.0, 40 + k, 7, k, 0x80000000, RESP)
        assert len(single) > 0 and got[off[k]:off[k + 1]].tobytes() == single.tobytes(), f"collidable of object {k}"
    # the two larger spheres 0.8 diameters apart, each probing the other
    d, pairs, singles = 2.0 * 12.0, [], []
    for a, b in ((1, 2), (2, 1)):
        ta, tb = placed(coms[a], [0.0, 0.0, 0.0]), placed(coms[b], [0.8 * d, 0.0, 0.0])
        pairs.append(dict(a=objs[a], b=objs[b], rotation_a=IDENT, translation_a=ta, center_of_mass_a=coms[a], rotation_b=IDENT, translation_b=tb,
                          center_of_mass_b=coms[b], collidable_id_a=100 + a, collidable_id_b=100 + b, body_a=a, body_b=b, response=RESP))
        singles.append(refs[a].mutual_contacts(IDENT, ta, coms[a], refs[b], IDENT, tb, coms[b], 100 + a, 100 + b, a, b, RESP))
    got, off = many.mutual_voxel_object_contacts_many(many.mutual_queries(pairs))
    for k, single in enumerate(singles):
        assert len(single) > 0 and got[off[k]:off[k + 1]].tobytes() == single.tobytes(), f"pair {k}"
    # a bite off every object's +x face; mesh and probes of all synced in one call each
    centres = [q.copy() for q in qs["shape3"]]
    edits = many.absorb_sphere_many(objs, centres, [5.0] * 3, [3.0] * 3, DENS)
    for k, (g, r, e) in enumerate(zip(objs, refs, edits)):
        single = r.absorb_sphere(centres[k], 5.0, 3.0, DENS)
        assert single["invalidated"].any(), k
        np.testing.assert_array_equal(e["invalidated"], single["invalidated"], err_msg=f"object {k}")
        assert (e["emptied_voxels"], e["touched_chunks"], e["removed_chunks"]) == (single["emptied_voxels"], single["touched_chunks"], single["removed_chunks"]), k
        # (sums of doubles in the order the workgroups arrive: the bound test_gpu_many.py holds them to against the oracle's)
        assert np.all(np.abs(e["removed_moments"] - single["removed_moments"]) <= 1e-5 * np.abs(single["removed_moments"]) + 1e-9), f"object {k}"
        for x, y in zip(g.download(), r.download()):
            np.testing.assert_array_equal(x, y, err_msg=f"object {k} after the bite")
        r.mesh.sync_with_voxel_object(single["invalidated"])
        r.collision_probes_sync(single["invalidated"])
    inv = [e["invalidated"] for e in edits]
    many.mesh_sync_many([g.mesh for g in objs], inv)
    ns = many.collision_probes_sync_many(objs, inv)
    for k, (g, r) in enumerate(zip(objs, refs)):
        (gpos, gnrm, gidx, gim, gsub), (rpos, rnrm, ridx, rim, rsub) = g.mesh.download(), r.mesh.download()
        assert gsub.tobytes() == rsub.tobytes() and len(gsub) > 0, f"submeshes of object {k} after the sync"
        for sm in rsub:  # (the data of every live range: what a freed range still holds is nobody's)
            i0, i1 = int(sm["index_offset"]), int(sm["index_offset"]) + int(sm["index_count"])
            v0, v1 = int(sm["vertex_offset"]), int(sm["vertex_offset"]) + int(sm["vertex_count"])
            assert gpos[v0:v1].tobytes() == rpos[v0:v1].tobytes() and gnrm[v0:v1].tobytes() == rnrm[v0:v1].tobytes(), f"vertices of object {k} after the sync"
            assert gidx[i0:i1].tobytes() == ridx[i0:i1].tobytes() and gim[i0:i1].tobytes() == rim[i0:i1].tobytes(), f"indices of object {k} after the sync"
        (gp, ge), (rp, re_) = g.collision_probes(), r.collision_probes()
        assert int(ns[k]) == len(rp) == len(gp) > 0, k
        np.testing.assert_array_equal(ge, re_)
        for e in re_:
            np.testing.assert_array_equal(gp[e[3]:e[4]].view(np.uint32), rp[e[3]:e[4]].view(np.uint32))
    # the moment sweep on its own, then the whole step: all objects per call, their gathers as one launch
    for stages in (capi.STAGE_INERTIA, STAGES):
        res = many.voxel_step_many(objs, stages)
        for k, (g, r) in enumerate(zip(objs, refs)):
            assert state(g, res[k], stages) == state(r, r.step(stages), stages), f"object {k}, stages {stages}"
    for g in objs + refs:
        g.close()
