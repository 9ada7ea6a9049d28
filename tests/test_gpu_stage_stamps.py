"""Stage times from in-kernel clock stamps (`ivx_grid_set_stage_timing`, step_enqueue in csrc/step_api.hip): on the step's fused path a timed
slot is the distance between two clock words that the first workgroup of two launches writes on entry, not a pair of event records on the
queue. The bodies here are a few chunks a side, so every kernel sits at the launch floor and no test compares durations with each other:
they check that timing never changes what a step computes, which slots report, and that the stamps are ordered and bounded by the host's
clock. The paths that keep their event records (slab protocol, calls that run the stand-alone per-chunk kernels) must still time."""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

import parity_util as pu
import stage_stamps_worker as w
from impact_amd import capi, scenes
from impact_amd.voxel import VoxelObjectMesh

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
USED = range(6)  # slots 0..5 are the step's; 6..9 are unused
ALL = 0xFFFFFFFF

_untimed = {}


def untimed(ctx, body):
    """the reference of a body — its step with timing off —, made once"""
    if body not in _untimed:
        _untimed[body] = w.stepped_snapshot(ctx, body, 0)
    return _untimed[body]


def assert_same_bytes(got, want, what):
    assert sorted(got) == sorted(want)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")


def assert_slots(ms, on, off, what=""):
    for i in range(capi.N_TIMED_STAGES):
        if i in on:
            assert ms[i] > 0.0, (what, i, list(ms))
        elif i in off:
            assert ms[i] == 0.0, (what, i, list(ms))


def timed_wall(obj, calls):
    """`calls` (stage masks) enqueued back to back, one collect: the step record, the host's wall time in ms from the first enqueue to the collect"""
    t0 = time.perf_counter()
    for st in calls:
        obj.step_enqueue(st)
    res = obj.step_collect().copy()
    return res, 1e3 * (time.perf_counter() - t0)


def assert_bounded(ms, wall_ms):
    assert all(ms[i] <= wall_ms for i in range(capi.N_TIMED_STAGES)), (list(ms), wall_ms)
    assert float(np.sum(ms)) <= wall_ms, (list(ms), wall_ms)


@pytest.fixture(scope="module")
def events_child():
    """every body stepped in ONE fresh process with IVX_STAGE_TIMING_EVENTS=1 (the switch is read when the library is loaded)"""
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([sys.executable, os.path.join(HERE, "stage_stamps_worker.py"), tmp] + list(w.BODIES), env=dict(os.environ, IVX_STAGE_TIMING_EVENTS="1"),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-3000:]
        yield {b: dict(np.load(os.path.join(tmp, b + ".npz"))) for b in w.BODIES}


@pytest.mark.parametrize("body", list(w.BODIES))
def test_same_bytes_under_every_timing_mask(ctx, body, events_child):
    """planes, chunk records, region labels, mesh buffers and the step record with one slot timed, with all of them, and with the event
    records forced, against the step with timing off"""
    want, ms0 = untimed(ctx, body)
    assert not np.any(ms0)
    assert int(want["mesh_counts"][0]) > 0 and int(want["region_count"][0]) >= 1
    for mask in [1 << k for k in USED] + [ALL]:
        got, ms = w.stepped_snapshot(ctx, body, mask)
        assert_same_bytes(got, want, f"mask {mask:#x}")
        assert_slots(ms, [i for i in USED if (mask >> i) & 1], [i for i in range(capi.N_TIMED_STAGES) if not (mask >> i) & 1], f"mask {mask:#x}")
    child = events_child[body]
    ms = child.pop("stage_ms")
    assert_same_bytes(child, want, "IVX_STAGE_TIMING_EVENTS=1")
    assert_slots(ms, USED, range(6, capi.N_TIMED_STAGES), "IVX_STAGE_TIMING_EVENTS=1")


@pytest.mark.parametrize("body", ["sphere4", "sphere2"])
def test_which_slots_report(ctx, body):
    obj = w.resident_object(ctx, body)
    obj.step(capi.STAGE_ALL)
    for mask in (0, 0b000101, 0b101010, ALL):
        obj.set_stage_timing(mask)
        ms = obj.step(capi.STAGE_ALL)["stage_ms"]
        assert_slots(ms, [i for i in USED if (mask >> i) & 1], [i for i in range(capi.N_TIMED_STAGES) if not (mask >> i) & 1], f"mask {mask:#x}")
        ticks, khz = obj.stage_ticks()
        assert khz > 0
        for i in range(capi.N_TIMED_STAGES):  # (the fused path: a timed slot's stamps are there, and stage_ms is their distance)
            if (mask >> i) & 1 and i in USED:
                assert 0 < ticks[i, 0] < ticks[i, 1]
                assert ms[i] == np.float32((int(ticks[i, 1]) - int(ticks[i, 0])) / khz)
            else:
                assert ticks[i, 0] == 0 and ticks[i, 1] == 0
    obj.set_stage_timing(ALL)
    # stages whose slots have no launch in the call report 0
    assert_slots(obj.step(capi.STAGE_SAMPLE | capi.STAGE_DERIVE)["stage_ms"], [0, 1], range(2, capi.N_TIMED_STAGES), "sample + derive")
    assert_slots(obj.step(capi.STAGE_DERIVE | capi.STAGE_OCCUPIED)["stage_ms"], [1, 2, 3], [0] + list(range(4, capi.N_TIMED_STAGES)), "derive + occupied")
    assert_slots(obj.step(capi.STAGE_ALL)["stage_ms"], USED, range(6, capi.N_TIMED_STAGES), "all")
    # a call without the derive stage (the moments' stand-alone kernel runs ahead of k_step_post1: the event path); no regions, so no assign
    ms = obj.step(capi.STAGE_REMESH | capi.STAGE_INERTIA)["stage_ms"]
    assert_slots(ms, [2, 3, 4], [0, 1] + list(range(5, capi.N_TIMED_STAGES)), "remesh + inertia")
    assert not np.any(obj.stage_ticks()[0])
    obj.close()


@pytest.mark.parametrize("body", list(w.BODIES))
def test_stamps_are_ordered_and_bounded_by_the_host_clock(ctx, body):
    obj = w.resident_object(ctx, body)
    obj.set_stage_timing(ALL)
    obj.step(capi.STAGE_ALL)
    for _ in range(3):
        res, wall_ms = timed_wall(obj, [capi.STAGE_ALL])
        ms = res["stage_ms"]
        assert_slots(ms, USED, range(6, capi.N_TIMED_STAGES))
        assert_bounded(ms, wall_ms)
        ticks, _ = obj.stage_ticks()
        flat = [int(t) for i in USED for t in ticks[i]]
        assert all(t > 0 for t in flat) and flat == sorted(flat), flat
        for i in range(5):  # adjacent timed slots share the stamp between them
            assert ticks[i, 1] == ticks[i + 1, 0]
    obj.close()


def test_sample_ahead_on_and_off_report_the_same_slots(ctx):
    """with the pre-pass a step ahead slot 0 starts at the first evaluator launch, without it at the pre-pass: timed either way"""
    seen = {}
    for ahead in (True, False):
        obj = w.resident_object(ctx, "asteroid5", ahead)
        obj.set_stage_timing(ALL)
        rows = []
        for _ in range(3):
            res, wall_ms = timed_wall(obj, [capi.STAGE_ALL])
            ms = res["stage_ms"]
            assert ms[0] > 0.0
            assert_bounded(ms, wall_ms)
            flat = [int(t) for i in USED for t in obj.stage_ticks()[0][i]]
            assert all(t > 0 for t in flat) and flat == sorted(flat), flat
            rows.append([bool(v > 0.0) for v in ms])
        seen[ahead] = rows
        obj.close()
    assert seen[True] == seen[False]
    assert all(r == [True] * 6 + [False] * 4 for r in seen[True])


@pytest.mark.parametrize("body", ["sphere4", "sphere2"])
def test_two_enqueues_before_one_collect(ctx, body):
    obj = w.resident_object(ctx, body)
    obj.set_stage_timing(ALL)
    whole = obj.step(capi.STAGE_ALL).copy()
    rest = capi.STAGE_ALL & ~(capi.STAGE_SAMPLE | capi.STAGE_DERIVE)
    # derive alone, then the rest (which, without the derive stage, runs the stand-alone region and moment kernels: events for that call)
    res, wall_ms = timed_wall(obj, [capi.STAGE_DERIVE, rest])
    assert_slots(res["stage_ms"], [1, 2, 3, 4, 5], [0] + list(range(6, capi.N_TIMED_STAGES)), "derive | rest")
    assert_bounded(res["stage_ms"], wall_ms)
    for k in ("mesh", "region_count"):
        assert res[k] == whole[k]
    np.testing.assert_array_equal(res["occupied"], whole["occupied"])
    np.testing.assert_allclose(res["moments"]["m64"], whole["moments"]["m64"], rtol=1e-5)  # (the stand-alone moment kernel sums in another order)
    # the derive sweep with its fused parts, then the launches behind it: every call on the fused path, one word shared across the two calls
    res, wall_ms = timed_wall(obj, [capi.STAGE_DERIVE | capi.STAGE_REGIONS | capi.STAGE_INERTIA, capi.STAGE_DERIVE | rest])
    assert_slots(res["stage_ms"], [1, 2, 3, 4, 5], [0] + list(range(6, capi.N_TIMED_STAGES)), "derive+ | derive + rest")
    assert_bounded(res["stage_ms"], wall_ms)
    ticks, khz = obj.stage_ticks()
    flat = [int(t) for i in range(1, 6) for t in ticks[i]]
    assert all(t > 0 for t in flat) and flat == sorted(flat), flat
    assert res["stage_ms"][1] == np.float32((int(ticks[1, 1]) - int(ticks[1, 0])) / khz)  # (slot 1 was enqueued twice: the second sweep's stamps)
    for k in ("mesh", "region_count"):
        assert res[k] == whole[k]
    # ... and a step of its own afterwards is whole again
    assert_slots(obj.step(capi.STAGE_ALL)["stage_ms"], USED, range(6, capi.N_TIMED_STAGES), "all")
    obj.close()


def test_slab_of_a_world_of_one_still_times(ctx):
    """the slab protocol keeps its event records (its step ends in the slab's record, not in the gather)"""
    from impact_amd.distributed import NativeComm, NativeSlabStepper, native_step

    comm = NativeComm(ctx, 1, local=True)
    st = NativeSlabStepper(ctx, comm, w.BODIES["sphere4"](), w.DENSITIES, 0)
    try:
        for _ in range(2):
            r = native_step([st])[0]
            assert_slots(r.stage_ms, USED, range(6, capi.N_TIMED_STAGES), "slab")
        assert not np.any(st.obj.stage_ticks()[0])
        want, _ = untimed(ctx, "sphere4")
        assert r.mesh_counts == tuple(int(v) for v in want["mesh_counts"]) and r.region_count == int(want["region_count"][0])
    finally:
        st.close()
        comm.close()


def test_steps_after_an_edit_and_a_mesh_sync_still_time(ctx):
    """an edit leaves planes that the sampler's sign rows no longer describe (the general forms of the sweep and the mesher run), and a step
    without the derive stage takes the stand-alone kernels and the event records"""
    g = pu.gpu_from_graph(ctx, scenes.sphere_scene(30.0))
    g.compute_all_derived_state()
    g.update_occupied_voxel_ranges()
    g.set_densities(w.DENSITIES)
    gm = VoxelObjectMesh.create(g)
    ctr = np.array([0.5 * (lo + hi) for lo, hi in g.occupied_voxel_ranges], dtype=np.float32)
    c = ctr + np.float32(30.0) * np.array([0.0, 0.0, 1.0], np.float32)  # (a bite out of the top)
    rg = g.absorb_sphere(c, 9.0, 7.0)
    assert np.any(rg["invalidated"])
    gm.sync_with_voxel_object(rg["invalidated"])
    g.set_stage_timing(ALL)
    a = g.step(capi.STAGE_ALL & ~(capi.STAGE_SAMPLE | capi.STAGE_DERIVE)).copy()
    assert_slots(a["stage_ms"], [2, 3, 4, 5], [0, 1] + list(range(6, capi.N_TIMED_STAGES)), "events")
    assert not np.any(g.stage_ticks()[0])
    b = g.step(capi.STAGE_ALL & ~capi.STAGE_SAMPLE).copy()
    assert_slots(b["stage_ms"], [1, 2, 3, 4, 5], [0] + list(range(6, capi.N_TIMED_STAGES)), "stamps")
    assert np.all(g.stage_ticks()[0][1:6] > 0)
    assert a["mesh"] == b["mesh"] and a["region_count"] == b["region_count"] and int(a["mesh"]["n_vertices"]) > 0
    np.testing.assert_allclose(a["moments"]["m64"], b["moments"]["m64"], rtol=1e-5)  # (stand-alone moment kernel against the sweep's fused part)
    g.close()
