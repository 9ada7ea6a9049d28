#!/usr/bin/env python3
"""Times the bounding volume calls (`ivx_bv_*`, impact_amd/csrc/bvol.hip) on four scenes:

  pile      the 4 096 spheres of scenes.sphere_pile_scene(16), boxes in the scene's lattice order
  shuffled  the same boxes in a seeded random order (no coherence for the block test to use)
  boxes     1 000 copies of config 1's 32^3 box on a 10 x 10 x 10 lattice (ivx_bv_set_grids) with 11 frustum queries, the views of a frame
  seeded    65 536 boxes of the seeded recipe of tests/bvol_ref.py

Per scene: set + pairs + download per call (device events over `--calls` calls after `--warmup` calls, on a stream the events know; all timed
calls are prepared ctypes calls), the pairs found, and the share of the pair walk's (row block, column block) tiles at or right of the diagonal
that the block-box test removes — restated in numpy from the downloaded boxes, in the kernel's own order.

  python tools/time_bvol.py            all scenes, each in a child process under its own time limit
  python tools/time_bvol.py --trace    also each scene once more under `rocprofv3 --kernel-trace --stats` (a run of its own) and the average
                                       time of every k_bv_ kernel"""
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

SCENES = ["pile", "shuffled", "boxes", "seeded"]


def skipped_tile_share(world):
    """of the tiles (row block, column block >= row block) of 64 x 64 objects: the share whose two block boxes lie outside each other"""
    import numpy as np

    import bvol_ref as br

    n = len(world)
    nb = (n + 63) // 64
    lo = np.full((nb * 64, 3), np.inf, dtype=np.float32)
    hi = np.full((nb * 64, 3), -np.inf, dtype=np.float32)
    lo[:n], hi[:n] = world["lower"], world["upper"]
    blo, bhi = lo.reshape(nb, 64, 3).min(axis=1), hi.reshape(nb, 64, 3).max(axis=1)
    skipped = tiles = 0
    for rb in range(nb):
        hit = br.boxes_intersect(blo[rb], bhi[rb], blo[rb:], bhi[rb:])
        tiles += nb - rb
        skipped += int((~hit).sum())
    return skipped / tiles, tiles


def frustum_planes(position, direction, fov_degrees, near, far):
    """the six world-space planes (unit normal, displacement; inside where n . p - d >= 0) of a square perspective frustum"""
    import numpy as np

    f = np.asarray(direction, dtype=np.float64)
    f /= np.linalg.norm(f)
    up = np.array([0.0, 1.0, 0.0]) if abs(f[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    t = np.tan(np.radians(fov_degrees) / 2)
    normals = [(r + t * f), (-r + t * f), (u + t * f), (-u + t * f)]
    planes = []
    p = np.asarray(position, dtype=np.float64)
    for nrm in normals:
        nrm = nrm / np.linalg.norm(nrm)
        planes.append((*nrm, float(nrm @ p)))
    planes.append((*f, float(f @ p) + near))
    planes.append((*(-f), float(-f @ p) - far))
    return np.array(planes, dtype=np.float32)


def workload(scene, calls, warmup):
    import numpy as np
    import torch

    import bvol_ref as br
    from impact_amd import bvol, capi, scenes
    from impact_amd.many import _handles
    from impact_amd.voxel import Context, SDFVoxelGenerator, VoxelObject

    stream = torch.cuda.Stream()
    ctx = Context(0, stream.cuda_stream)
    lib = capi.lib()
    objects, queries = [], None
    if scene in ("pile", "shuffled"):
        bodies, _ = scenes.sphere_pile_scene(16, points_per_pair=1)
        pos = bodies["position"].astype(np.float32)
        if scene == "shuffled":
            pos = pos[np.random.default_rng(1).permutation(len(pos))]
        boxes = bvol.boxes(pos - np.float32(0.5), pos + np.float32(0.5))
    elif scene == "seeded":
        boxes = np.array(br.scene(65536)[0])
    else:
        gen = SDFVoxelGenerator(1.0, scenes.box_scene())
        objects = [VoxelObject.generate(ctx, gen) for _ in range(1000)]
        for o in objects:
            o.update_occupied_voxel_ranges()
        positions = np.array([(48.0 * i, 48.0 * j, 48.0 * k) for i in range(10) for j in range(10) for k in range(10)], dtype=np.float32)
        sims = bvol.similarities(1000)
        sims["translation"] = positions
        centre, size = positions.mean(axis=0) + 16.0, 480.0
        views = [frustum_planes(centre + np.array([0.3, 0.2, 1.0]) * size, -np.array([0.3, 0.2, 1.0]), 60.0, 0.1, 4 * size)]
        light = centre + np.array([0.1, 0.45, 0.05]) * size
        views += [frustum_planes(light, d, 90.0, 0.1, 2 * size) for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
        sun = centre + np.array([0.4, 1.5, 0.3]) * size
        views += [frustum_planes(sun, centre - sun, 4.0 * 2.2 ** k, 0.0, 4 * size) for k in range(4)]
        queries = bvol.query_array([bvol.frustum_query(v) for v in views])
        handles = _handles(objects)
    n = len(objects) if objects else len(boxes)

    def set_call():
        rc = lib.ivx_bv_set_grids(handles.ctypes.data, n, sims.ctypes.data, None) if objects else lib.ivx_bv_set(ctx.h, boxes.ctypes.data, None, None, n)
        if rc:
            capi.check(rc)

    import ctypes as C

    found = C.c_size_t(0)
    set_call()
    rc = lib.ivx_bv_pairs(ctx.h, 0, None, 0, C.byref(found))
    if rc:
        capi.check(rc)
    cap = found.value
    pair_out = np.zeros((max(1, cap), 2), dtype=np.uint32)
    world, total = np.zeros(n, dtype=capi.AABB_DTYPE), np.zeros(1, dtype=capi.AABB_DTYPE)

    def pairs_call():
        rc = lib.ivx_bv_pairs(ctx.h, 0, pair_out.ctypes.data, cap, C.byref(found))
        if rc:
            capi.check(rc)

    def download_call():
        rc = lib.ivx_bv_download(ctx.h, world.ctypes.data, n, total.ctypes.data)
        if rc:
            capi.check(rc)

    def frame():
        set_call()
        pairs_call()
        download_call()

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
        return start.elapsed_time(stop) / calls

    out = {"scene": scene, "objects": n, "calls": calls, "warmup": warmup}
    out["set_pairs_download_ms"] = timed(frame)
    out["set_ms"], out["pairs_ms"], out["download_ms"] = timed(set_call), timed(pairs_call), timed(download_call)
    out["pairs"] = int(found.value)
    share, tiles = skipped_tile_share(world)
    out["tiles"], out["tiles_skipped_share"] = tiles, round(share, 4)
    if queries is not None:
        masks, counts = np.zeros((len(queries), (n + 63) // 64), dtype=np.uint64), np.zeros(len(queries), dtype=np.uint32)

        def query_call():
            rc = lib.ivx_bv_queries(ctx.h, queries.ctypes.data, len(queries), masks.ctypes.data, counts.ctypes.data)
            if rc:
                capi.check(rc)

        out["queries"], out["queries_ms"], out["query_counts"] = len(queries), timed(query_call), counts.tolist()
    for o in objects:
        o.close()
    ctx.close()
    return out


def kernel_times(db_path):
    db = sqlite3.connect(db_path)
    rows = db.execute("select name, count(*), avg(end-start) from kernels where name like '%k_bv_%' group by name order by 3 desc")
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
    ap.add_argument("--scene", choices=SCENES + ["all"], default="all")
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
    for scene in (SCENES if args.scene == "all" else [args.scene]):
        # (a step that fails or runs out of time ends the run: nothing more is started on the device)
        out = json.loads(run_limited(me + ["--scene", scene], args.limit).strip().splitlines()[-1])
        if args.trace:
            tmp = tempfile.mkdtemp(prefix="time_bvol_")
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
