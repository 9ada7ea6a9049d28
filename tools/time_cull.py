#!/usr/bin/env python3
"""Times chunk culling (`ivx_cull_many`, impact_amd/csrc/cull.hip) on two scenes under the 11 views of the reference's stress scene
(docs/voxel_gpu_buffer_pooling.md): 1 perspective camera (non-indexed), 6 cubemap faces (perspective, indexed), 4 cascades (orthographic, indexed).

  small   1 000 copies of config 1's 32^3 box on a 10 x 10 x 10 lattice
  large   the 512^3 headline grid (scenes.asteroid_scene(2.05)), one object

Each scene three ways: the batched call in mode 0 (zeroed in place) and mode 1 (compacted), and a loop of `n = 1, n_views = 1` calls of
`ivx_cull_many_enqueue` over every (object, view) — the reference's dispatch structure, the baseline. Device events over `--calls` calls after
`--warmup` calls, on a stream the events know; all timed calls are prepared ctypes calls, so the host side is the library's, not numpy's.
The batched call is timed whole (with its collect's wait) and as its enqueue half alone.

  python tools/time_cull.py            both scenes, each in a child process under its own time limit
  python tools/time_cull.py --trace    also the batched calls once more under `rocprofv3 --kernel-trace --stats` (a run of its own) and the
                                       average time of every culling kernel"""
import argparse
import json
import os
import shutil
import sqlite3
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def frame_views_and_pairs(positions, extent_of_scene):
    """the 11 views of a frame looking at the scene's centre, and the pairs of objects placed (unrotated, unscaled) at `positions`"""
    import numpy as np

    import cull_ref as cr
    from impact_amd import capi

    centre = 0.5 * (positions.min(axis=0) + positions.max(axis=0)) + 16.0
    size = float(extent_of_scene)
    cameras = [(cr.perspective_view(70.0, 50.0, 0.1, 4.0 * size, indexed=False), centre + np.array([0.3, 0.2, 1.0]) * size, None)]
    light = centre + np.array([0.1, 0.45, 0.05]) * size
    for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        cameras.append((cr.perspective_view(90.0, 90.0, 0.1, 2.0 * size, indexed=True), light, np.array(d, dtype=np.float64)))
    sun = centre + np.array([0.4, 1.5, 0.3]) * size
    for k in range(4):
        half = size * 0.08 * 2.2 ** k
        cameras.append((cr.orthographic_view(half, half, 0.0, 4.0 * size, indexed=True), sun, None))
    views = np.array([c[0] for c in cameras])
    pairs = np.zeros((len(cameras), len(positions)), dtype=capi.CULL_PAIR_DTYPE)
    for v, (_, position, direction) in enumerate(cameras):
        vq = cr.look_rotation(centre - position if direction is None else direction)
        pairs[v]["rotation"] = cr.q_conj(vq)
        for o in range(len(positions)):
            pairs[v, o]["translation"] = cr.q_rot(cr.q_conj(vq), positions[o] - position)
        pairs[v]["scaling"] = 1.0
        pairs[v]["instance_idx"] = np.arange(len(positions))
    return views, pairs


def workload(scene, calls, warmup, with_loop):
    import numpy as np
    import torch

    from impact_amd import capi, scenes
    from impact_amd.many import _handles
    from impact_amd.voxel import Context, SDFVoxelGenerator, VoxelObject, VoxelObjectMesh

    stream = torch.cuda.Stream()
    ctx = Context(0, stream.cuda_stream)
    if scene == "small":
        gen = SDFVoxelGenerator(1.0, scenes.box_scene())
        objects = [VoxelObject.generate(ctx, gen) for _ in range(1000)]
        positions = np.array([(48.0 * i, 48.0 * j, 48.0 * k) for i in range(10) for j in range(10) for k in range(10)])
        size = 480.0
    else:
        objects = [VoxelObject.generate(ctx, SDFVoxelGenerator(1.0, scenes.asteroid_scene(2.05)))]
        positions = np.zeros((1, 3))
        size = 512.0
    meshes = [VoxelObjectMesh.create(o) for o in objects]
    views, pairs = frame_views_and_pairs(positions, size)
    n, n_views = len(objects), len(views)

    def timed(fn, calls, warmup):
        for _ in range(warmup):
            fn()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            start.record(stream)
            for _ in range(calls):
                fn()
            stop.record(stream)
        stop.synchronize()
        return start.elapsed_time(stop) / calls

    out = {"scene": scene, "objects": n, "views": n_views, "submeshes": int(sum(m.n_chunks() for m in meshes)), "calls": calls, "warmup": warmup}
    # every timed call is a prepared ctypes call (arrays built once): the host side is the library's in all three ways
    lib = capi.lib()
    handles = _handles(objects)
    views_c, pairs_c = np.ascontiguousarray(views), np.ascontiguousarray(pairs)
    layout_all = np.zeros(n_views, dtype=capi.CULL_REGION_DTYPE)
    counts_all = np.zeros(n_views, dtype=capi.CULL_COUNT_DTYPE)
    for mode, name in ((capi.CULL_ZEROED, "batched_zeroed_ms"), (capi.CULL_COMPACTED, "batched_compacted_ms")):
        call = (handles.ctypes.data, n, None, views_c.ctypes.data, n_views, pairs_c.ctypes.data, mode, layout_all.ctypes.data, counts_all.ctypes.data)

        def batched(call=call):
            rc = lib.ivx_cull_many(*call)
            if rc:
                capi.check(rc)

        out[name] = timed(batched, calls, warmup)
        out[name.replace("_ms", "_draws")] = [int(d) for d in counts_all["draws"]]
        enqueue = call[:-1]

        def enqueued(enqueue=enqueue):  # the enqueue half alone, one collect behind the timed calls' last
            rc = lib.ivx_cull_many_enqueue(*enqueue)
            if rc:
                capi.check(rc)

        out[name.replace("_ms", "_enqueue_only_ms")] = timed(enqueued, calls, warmup)
        capi.check(lib.ivx_cull_collect(ctx.h, counts_all.ctypes.data, n_views))
    if with_loop:
        layout = np.zeros(1, dtype=capi.CULL_REGION_DTYPE)
        counts = np.zeros(1, dtype=capi.CULL_COUNT_DTYPE)
        prepared = [(handles[o:o + 1].ctypes.data, 1, None, views[v:v + 1].ctypes.data, 1, pairs[v, o:o + 1].ctypes.data, 0, layout.ctypes.data)
                    for v in range(n_views) for o in range(n)]

        def loop():
            for a in prepared:
                rc = lib.ivx_cull_many_enqueue(*a)
                if rc:
                    capi.check(rc)
            capi.check(lib.ivx_cull_collect(ctx.h, counts.ctypes.data, 1))

        out["loop_calls_per_frame"] = len(prepared)
        out["loop_ms"] = timed(loop, calls, warmup)
        out["loop_over_batched_zeroed"] = out["loop_ms"] / out["batched_zeroed_ms"]
    for o in objects:
        o.close()
    ctx.close()
    return out


def kernel_times(db_path):
    db = sqlite3.connect(db_path)
    rows = db.execute("select name, count(*), avg(end-start) from kernels where name like '%k_cull_%' group by name order by 3 desc")
    return {name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: (int(n), float(avg_ns)) for name, n, avg_ns in rows}


def run_limited(cmd, limit, quiet=False):
    """run `cmd` in a process group of its own; a time limit ends the whole group (rocprofv3 and the program below it)"""
    import signal

    p = subprocess.Popen(cmd, stdout=subprocess.DEVNULL if quiet else subprocess.PIPE, stderr=subprocess.DEVNULL if quiet else None, text=True, start_new_session=True)
    try:
        stdout, _ = p.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        p.wait()
        raise
    if p.returncode:
        raise subprocess.CalledProcessError(p.returncode, cmd)
    return stdout


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", choices=["small", "large", "both"], default="both")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", action="store_true", help="also run the batched calls under rocprofv3 --kernel-trace --stats and report the kernel times")
    ap.add_argument("--limit", type=int, default=300, help="time limit of each child process in seconds")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-loop", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(workload(args.scene, args.calls, args.warmup, not args.no_loop)))
        return
    me = [sys.executable, os.path.abspath(__file__), "--child", "--calls", str(args.calls), "--warmup", str(args.warmup)]
    for scene in (["small", "large"] if args.scene == "both" else [args.scene]):
        # (a step that fails or runs out of time ends the run: nothing more is started on the device)
        out = json.loads(run_limited(me + ["--scene", scene], args.limit).strip().splitlines()[-1])
        if args.trace:
            tmp = tempfile.mkdtemp(prefix="time_cull_")
            try:
                run_limited(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "trace", "--"] + me + ["--scene", scene, "--no-loop"], args.limit, quiet=True)
                dbs = [os.path.join(d, f) for d, _, fs in os.walk(tmp) for f in fs if f.endswith(".db")]
                times = kernel_times(sorted(dbs)[-1])
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
            out["kernel_us"] = {k: round(v[1] / 1e3, 2) for k, v in times.items()}
            out["kernel_calls"] = {k: v[0] for k, v in times.items()}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
