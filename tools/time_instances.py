#!/usr/bin/env python3
"""Times the frame-instance stage (`ivx_fi_views`, impact_amd/csrc/instances.hip) and the frame leg it closes, at two shapes:

  small   1 000 objects x 11 views: 1 000 copies of config 1's 32^3 box on a 10 x 10 x 10 lattice (the cull tool's shape), every one a voxel object
  large   25 000 objects x 64 views: the seeded boxes of tests/bvol_ref.py; 1 000 of them (every 25th) are the voxel objects above

Per shape, in one process, host clock around prepared ctypes calls that end in a wait (`--calls` calls after `--warmup` calls):

  views_ms          ivx_fi_views with its results (one wait)
  views_enqueue_ms  ivx_fi_views without results (nothing waits; one synchronize behind the timed calls)
  host_form_ms      ivx_fi_views_host over the same inputs, one thread
  frame_ms          ivx_bv_set -> ivx_bv_queries -> ivx_fi_views (results) -> ivx_cull_many_resident -> ivx_cull_collect
  old_frame_ms      ivx_bv_set -> ivx_bv_queries -> ivx_bv_query_lists (lists downloaded) -> ivx_fi_views_host -> ivx_cull_many_enqueue with the
                    voxel objects' pairs uploaded -> ivx_cull_collect: what a caller did before this stage existed

  python tools/time_instances.py            both shapes, each in a child process under its own time limit"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = {"small": (1000, 11), "large": (25000, 64)}


def workload(shape, calls, warmup):
    import ctypes as C

    import numpy as np
    import torch

    import bvol_ref as br
    import instances_ref as ir
    from impact_amd import bvol, capi, instances, scenes
    from impact_amd.many import _handles
    from impact_amd.voxel import Context, SDFVoxelGenerator, VoxelObject, VoxelObjectMesh
    from time_cull import frame_views_and_pairs

    n, n_views = SHAPES[shape]
    stream = torch.cuda.Stream()
    ctx = Context(0, stream.cuda_stream)
    lib = capi.lib()
    gen = SDFVoxelGenerator(1.0, scenes.box_scene())
    objects = [VoxelObject.generate(ctx, gen) for _ in range(1000)]
    meshes = [VoxelObjectMesh.create(o) for o in objects]
    index = (np.arange(1000) * (n // 1000)).astype(np.uint32)
    world, inst = ir.scene(n)
    world, inst = world.copy(), inst.copy()
    positions = np.array([(48.0 * i, 48.0 * j, 48.0 * k) for i in range(10) for j in range(10) for k in range(10)])
    if shape == "small":  # the voxel objects' own boxes on the lattice, unrotated and unscaled
        model = bvol.grid_model_aabb(objects[0])
        world["lower"], world["upper"] = positions + model["lower"], positions + model["upper"]
        inst["model_to_world"] = bvol.similarities(n)
        inst["model_to_world"]["translation"] = positions
    cull_views, _ = frame_views_and_pairs(positions, 480.0)
    cull_views = np.ascontiguousarray(np.resize(cull_views, n_views))
    ext = br.scene_extent(n) if shape == "large" else 480.0
    rng = np.random.default_rng(3)
    queries = bvol.query_array([bvol.sphere_query(rng.uniform(0.2 * ext, 0.8 * ext, 3), rng.uniform(0.3, 0.6) * ext) for _ in range(n_views)])
    views = ir.seeded_views(n, n_views, n_views, 0, seed=1)
    views["point"], views["squared_reach"] = rng.uniform(0.0, ext, (n_views, 3)), (0.6 * ext) ** 2
    inst["flags"] = np.where(rng.random(n) < 0.9, 0, inst["flags"])
    words = (n + 63) // 64
    masks, counts = np.zeros((n_views, words), dtype=np.uint64), np.zeros(n_views, dtype=np.uint32)
    results = np.zeros(n_views, dtype=capi.FI_VIEW_RESULT_DTYPE)
    layout, cull_counts = np.zeros(n_views, dtype=capi.CULL_REGION_DTYPE), np.zeros(n_views, dtype=capi.CULL_COUNT_DTYPE)
    host_pairs = np.zeros((n_views, n), dtype=capi.CULL_PAIR_DTYPE)
    handles = _handles(objects)
    offsets, hit_objects, found = np.zeros(n_views + 1, dtype=np.uint32), np.zeros(n_views * n, dtype=np.uint32), C.c_size_t(0)

    def ok(rc):
        if rc:
            capi.check(rc)

    def set_and_query():
        ok(lib.ivx_bv_set(ctx.h, world.ctypes.data, None, None, n))
        ok(lib.ivx_bv_queries(ctx.h, queries.ctypes.data, n_views, masks.ctypes.data, counts.ctypes.data))

    def fi_views():
        ok(lib.ivx_fi_views(ctx.h, views.ctypes.data, n_views, results.ctypes.data))

    def fi_views_enqueue():
        ok(lib.ivx_fi_views(ctx.h, views.ctypes.data, n_views, None))

    def host_form():
        ok(lib.ivx_fi_views_host(world.ctypes.data, n, inst.ctypes.data, masks.ctypes.data, n_views, views.ctypes.data, n_views, None, 0, host_pairs.ctypes.data, None, None, None, 0,
                                 None, results.ctypes.data))

    def frame():
        set_and_query()
        fi_views()
        ok(lib.ivx_cull_many_resident(handles.ctypes.data, 1000, None, index.ctypes.data, cull_views.ctypes.data, n_views, capi.CULL_COMPACTED, layout.ctypes.data))
        ok(lib.ivx_cull_collect(ctx.h, cull_counts.ctypes.data, n_views))

    def old_frame():
        set_and_query()
        ok(lib.ivx_bv_query_lists(ctx.h, offsets.ctypes.data, hit_objects.ctypes.data, hit_objects.size, C.byref(found)))
        host_form()
        gathered = np.ascontiguousarray(host_pairs[:, index])
        ok(lib.ivx_cull_many_enqueue(handles.ctypes.data, 1000, None, cull_views.ctypes.data, n_views, gathered.ctypes.data, capi.CULL_COMPACTED, layout.ctypes.data))
        ok(lib.ivx_cull_collect(ctx.h, cull_counts.ctypes.data, n_views))

    def timed(fn, sync_after=False):
        for _ in range(warmup):
            fn()
        ok(lib.ivx_synchronize(ctx.h))
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        if sync_after:
            ok(lib.ivx_synchronize(ctx.h))
        return (time.perf_counter() - t0) * 1e3 / calls

    ok(lib.ivx_fi_set_instances(ctx.h, inst.ctypes.data, n))
    set_and_query()
    out = {"shape": shape, "objects": n, "views": n_views, "voxel_objects": 1000, "calls": calls, "warmup": warmup}
    out["views_ms"] = timed(fi_views)
    out["kept_pairs"] = int(results["count"].sum())
    device_results = results.copy()
    out["views_enqueue_ms"] = timed(fi_views_enqueue, sync_after=True)
    out["host_form_ms"] = timed(host_form)
    out["host_form_equals_device"] = bool(results.tobytes() == device_results.tobytes())
    out["frame_ms"] = timed(frame)
    frame_draws = cull_counts["draws"].copy()
    out["old_frame_ms"] = timed(old_frame)
    out["old_frame_draws_equal"] = bool((frame_draws == cull_counts["draws"]).all())
    out["draws"] = int(frame_draws.sum())
    del meshes
    for o in objects:
        o.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", choices=["small", "large", "both"], default="both")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="time limit of each child process in seconds")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(workload(args.shape, args.calls, args.warmup)))
        return
    me = [sys.executable, os.path.abspath(__file__), "--child", "--calls", str(args.calls), "--warmup", str(args.warmup)]
    for shape in (["small", "large"] if args.shape == "both" else [args.shape]):
        # (a child that fails or runs out of time ends the run: nothing more is started on the device)
        done = subprocess.run(me + ["--shape", shape], stdout=subprocess.PIPE, text=True, timeout=args.limit, check=True)
        print(done.stdout.strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
