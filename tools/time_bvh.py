#!/usr/bin/env python3
"""Times the two forms of the pair pass — the hierarchy (`ivx_bv_build_hierarchy`, `ivx_bv_pairs_hierarchy`, impact_amd/csrc/bvh.hip) and the flat
upper triangle (`ivx_bv_pairs`, bvol.hip) — in the same process, alternating, on the four scenes of tools/time_bvol.py and one more:

  pile      the 4 096 spheres of scenes.sphere_pile_scene(16), boxes in the scene's lattice order
  shuffled  the same boxes in a seeded random order
  boxes     1 000 copies of config 1's 32^3 box on a 10 x 10 x 10 lattice (ivx_bv_set_grids)
  seeded    65 536 boxes of the seeded recipe of tests/bvol_ref.py
  fullrow   the pile with its first box replaced by one box around the 4 095 others: one lane of the tree walk visits most of the tree

Per scene, from device events over `--calls` calls after `--warmup` calls (all timed calls are prepared ctypes calls): build, tree pairs, flat
pairs, and set + pairs + download for both forms (the tree form's includes its build). The two forms must return the same bytes, or the scene fails.
`--sizes` adds the seeded recipe at the given sizes, to find where the tree form first wins.

  python tools/time_bvh.py            all scenes, each in a child process under its own time limit, one child at a time
  python tools/time_bvh.py --trace    also each scene once more under `rocprofv3 --kernel-trace --stats` (a run of its own) and the average
                                      time of every k_bv_ / k_bvh_ kernel"""
import argparse
import json
import os
import shutil
import sqlite3
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SCENES = ["pile", "shuffled", "boxes", "seeded", "fullrow"]


def workload(scene, calls, warmup):
    import ctypes as C

    import numpy as np
    import torch

    import bvol_ref as br
    from impact_amd import bvol, capi, scenes
    from impact_amd.many import _handles
    from impact_amd.voxel import Context, SDFVoxelGenerator, VoxelObject

    stream = torch.cuda.Stream()
    ctx = Context(0, stream.cuda_stream)
    lib = capi.lib()
    objects = []
    if scene in ("pile", "shuffled", "fullrow"):
        bodies, _ = scenes.sphere_pile_scene(16, points_per_pair=1)
        pos = bodies["position"].astype(np.float32)
        if scene == "shuffled":
            pos = pos[np.random.default_rng(1).permutation(len(pos))]
        boxes = bvol.boxes(pos - np.float32(0.5), pos + np.float32(0.5))
        if scene == "fullrow":
            boxes["lower"][0], boxes["upper"][0] = boxes["lower"][1:].min(axis=0) - 1.0, boxes["upper"][1:].max(axis=0) + 1.0
    elif scene.startswith("seeded"):
        boxes = np.array(br.scene(int(scene[6:] or 65536))[0])
    else:
        gen = SDFVoxelGenerator(1.0, scenes.box_scene())
        objects = [VoxelObject.generate(ctx, gen) for _ in range(1000)]
        for o in objects:
            o.update_occupied_voxel_ranges()
        sims = bvol.similarities(1000)
        sims["translation"] = np.array([(48.0 * i, 48.0 * j, 48.0 * k) for i in range(10) for j in range(10) for k in range(10)], dtype=np.float32)
        handles = _handles(objects)
    n = len(objects) if objects else len(boxes)
    found = C.c_size_t(0)

    def ok(rc):
        if rc:
            capi.check(rc)

    def set_call():
        ok(lib.ivx_bv_set_grids(handles.ctypes.data, n, sims.ctypes.data, None) if objects else lib.ivx_bv_set(ctx.h, boxes.ctypes.data, None, None, n))

    set_call()
    ok(lib.ivx_bv_pairs(ctx.h, 0, None, 0, C.byref(found)))
    cap = found.value
    flat_out, tree_out = np.zeros((max(1, cap), 2), dtype=np.uint32), np.zeros((max(1, cap), 2), dtype=np.uint32)
    world, total = np.zeros(n, dtype=capi.AABB_DTYPE), np.zeros(1, dtype=capi.AABB_DTYPE)
    build_call = lambda: ok(lib.ivx_bv_build_hierarchy(ctx.h))
    tree_pairs = lambda: ok(lib.ivx_bv_pairs_hierarchy(ctx.h, 0, tree_out.ctypes.data, cap, C.byref(found)))
    flat_pairs = lambda: ok(lib.ivx_bv_pairs(ctx.h, 0, flat_out.ctypes.data, cap, C.byref(found)))
    download_call = lambda: ok(lib.ivx_bv_download(ctx.h, world.ctypes.data, n, total.ctypes.data))

    def tree_frame():
        set_call(), build_call(), tree_pairs(), download_call()

    def flat_frame():
        set_call(), flat_pairs(), download_call()

    def timed(fn):
        for _ in range(warmup):
            fn()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            start.record(stream)
            for _ in range(calls):
                fn()
            stop.record(stream)
        stop.synchronize()
        return round(start.elapsed_time(stop) / calls, 4)

    out = {"scene": scene, "objects": n, "calls": calls, "warmup": warmup}
    build_call()
    # the two forms alternate: frame, frame, then the parts
    out["tree_set_build_pairs_download_ms"], out["flat_set_pairs_download_ms"] = timed(tree_frame), timed(flat_frame)
    out["build_ms"], out["tree_pairs_ms"], out["flat_pairs_ms"] = timed(build_call), timed(tree_pairs), timed(flat_pairs)
    out["pairs"] = int(found.value)
    if tree_out.tobytes() != flat_out.tobytes():
        raise SystemExit(f"{scene}: the two forms returned different pairs")
    for o in objects:
        o.close()
    ctx.close()
    return out


def kernel_times(db_path):
    db = sqlite3.connect(db_path)
    rows = db.execute("select name, count(*), avg(end-start) from kernels where name like '%k_bv%' group by name order by 3 desc")
    return {name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: (int(n), float(avg_ns)) for name, n, avg_ns in rows}


def main():
    from time_bvol import run_limited

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="all", help="one of " + ", ".join(SCENES) + ", seeded<n>, or all")
    ap.add_argument("--sizes", type=int, nargs="*", default=[], help="also the seeded recipe at these sizes")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", action="store_true", help="also run each scene under rocprofv3 --kernel-trace --stats and report the kernel times")
    ap.add_argument("--limit", type=int, default=240, help="time limit of each child process in seconds")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(workload(args.scene, args.calls, args.warmup)))
        return
    me = [sys.executable, os.path.abspath(__file__), "--child", "--calls", str(args.calls), "--warmup", str(args.warmup)]
    for scene in (SCENES if args.scene == "all" else [args.scene]) + [f"seeded{n}" for n in args.sizes]:
        # (a step that fails or runs out of time ends the run: nothing more is started on the device)
        out = json.loads(run_limited(me + ["--scene", scene], args.limit).strip().splitlines()[-1])
        if args.trace:
            tmp = tempfile.mkdtemp(prefix="time_bvh_")
            try:
                run_limited(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "trace", "--"] + me + ["--scene", scene], args.limit, quiet=True)
                dbs = [os.path.join(d, f) for d, _, fs in os.walk(tmp) for f in fs if f.endswith(".db")]
                times = kernel_times(sorted(dbs)[-1])
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
            out["kernel_us"] = {k: round(v[1] / 1e3, 2) for k, v in times.items()}
            out["kernel_calls"] = {k: v[0] for k, v in times.items()}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
