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
  python tools/time_bvh.py --leg queries
                                      the region queries instead (`ivx_bv_queries_hierarchy` against `ivx_bv_queries`, and `ivx_bv_query_lists`):
                                      refbench, the shape of the reference's own benchmark (25 000 stratified boxes under 1 000 box queries of half
                                      extent 0.5 to half the scene), and small<n> (64 absorber-sized boxes and 11 frusta) over 4 096, 65 536 and
                                      2^20 stratified boxes. Per workload: both forms, twice each, alternating; the masks' download on its own
                                      (the calls always download: `_without_download_ms` is the better call less that copy); the build; the
                                      list expansion with its results left on the device and downloaded
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


QUERY_WORKLOADS = ["refbench", "small4096", "small65536", "small1048576"]


def stratified_boxes(n, seed=1):
    """the shape of the reference benchmark's set: one box per cell of a cubic lattice of cell size 2, its centre offset by up to 1 per axis in
    steps of 1/256, its half extent 0.25 .. 0.75 in steps of 1/512 (seeded here; the reference hashes the index)"""
    import numpy as np

    from impact_amd import bvol

    rng = np.random.default_rng(seed)
    per_axis = int(np.ceil(np.cbrt(n)))
    i = np.arange(n)
    cell = np.stack([i % per_axis, (i // per_axis) % per_axis, i // (per_axis * per_axis)], axis=1).astype(np.float64)
    centre = 2.0 * cell + rng.integers(0, 256, (n, 3)) / 256.0
    half = (0.25 + rng.integers(0, 256, n) / 512.0)[:, None]
    return bvol.boxes(centre - half, centre + half)


def query_records(name, boxes, seed=2):
    """refbench: 1 000 box queries centred anywhere in the set's extent, half extent 0.5 .. 0.5 + half the largest extent. small<n>: 64
    absorber-sized boxes (half extent 1 .. 3) and 11 frusta (a camera, six cube faces and four cascades' worth: boxes of a tenth to a half of the
    extent under rotations uniform on the sphere)"""
    import numpy as np

    import bvh_query_cases as qc
    from impact_amd import bvol

    rng = np.random.default_rng(seed)
    lo, hi = boxes["lower"].min(axis=0).astype(np.float64), boxes["upper"].max(axis=0).astype(np.float64)
    out = []
    if name == "refbench":
        for _ in range(1000):
            centre, half = rng.uniform(lo, hi), 0.5 + rng.integers(0, 256) / 255.0 * float((hi - lo).max()) * 0.5
            out.append(bvol.box_query(centre - half, centre + half))
        return bvol.query_array(out)
    for _ in range(64):
        centre, half = rng.uniform(lo, hi), rng.uniform(1.0, 3.0, 3)
        out.append(bvol.box_query(centre - half, centre + half))
    for _ in range(11):
        half = rng.uniform(0.1, 0.5) * (hi - lo) * 0.5
        out.append(bvol.frustum_query(qc.box_planes(rng.uniform(lo, hi), qc.random_rotation(rng), half)))
    return bvol.query_array(out)


def query_workload(name, calls, warmup):
    """one workload of the queries leg: both forms in the same process, alternating; the masks' download timed on its own (the calls always
    download: `without` is the call less that copy), and the list expansion on its own"""
    import ctypes as C

    import numpy as np
    import torch

    from impact_amd import capi
    from impact_amd.voxel import Context

    stream = torch.cuda.Stream()
    ctx = Context(0, stream.cuda_stream)
    lib = capi.lib()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    n = 25000 if name == "refbench" else int(name[5:])
    boxes = stratified_boxes(n)
    queries = query_records(name, boxes)
    nq, words = len(queries), (n + 63) // 64
    found = C.c_size_t(0)

    def ok(rc):
        if rc:
            capi.check(rc)

    ok(lib.ivx_bv_set(ctx.h, boxes.ctypes.data, None, None, n))
    ok(lib.ivx_bv_build_hierarchy(ctx.h))
    flat_masks, tree_masks = np.zeros((nq, words), dtype=np.uint64), np.zeros((nq, words), dtype=np.uint64)
    flat_counts, tree_counts = np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.uint32)
    flat_call = lambda: ok(lib.ivx_bv_queries(ctx.h, queries.ctypes.data, nq, flat_masks.ctypes.data, flat_counts.ctypes.data))
    tree_call = lambda: ok(lib.ivx_bv_queries_hierarchy(ctx.h, queries.ctypes.data, nq, tree_masks.ctypes.data, tree_counts.ctypes.data))
    build_call = lambda: ok(lib.ivx_bv_build_hierarchy(ctx.h))
    flat_call()
    d_masks = lib.ivx_bv_device_ptr(ctx.h, capi.BV_PTR_MASKS)
    copy = np.zeros((nq, words), dtype=np.uint64)

    def download_call():
        assert hip.hipMemcpyAsync(copy.ctypes.data, d_masks, copy.nbytes, 2, stream.cuda_stream) == 0
        stream.synchronize()

    ok(lib.ivx_bv_query_lists(ctx.h, None, None, 0, C.byref(found)))
    total = found.value
    offsets, objects = np.zeros(nq + 1, dtype=np.uint32), np.zeros(max(1, total), dtype=np.uint32)
    lists_resident = lambda: ok(lib.ivx_bv_query_lists(ctx.h, None, None, 0, C.byref(found)))
    lists_download = lambda: ok(lib.ivx_bv_query_lists(ctx.h, offsets.ctypes.data, objects.ctypes.data, total, C.byref(found)))

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

    out = {"workload": name, "objects": n, "queries": nq, "calls": calls, "warmup": warmup}
    out["tree_queries_ms"], out["flat_queries_ms"] = timed(tree_call), timed(flat_call)
    out["tree_queries_again_ms"], out["flat_queries_again_ms"] = timed(tree_call), timed(flat_call)
    out["mask_download_ms"], out["build_ms"] = timed(download_call), timed(build_call)
    for form in ("tree", "flat"):
        out[f"{form}_without_download_ms"] = round(min(out[f"{form}_queries_ms"], out[f"{form}_queries_again_ms"]) - out["mask_download_ms"], 4)
    out["lists_resident_ms"], out["lists_download_ms"] = timed(lists_resident), timed(lists_download)
    out["hits"], out["mask_bytes"] = int(total), int(copy.nbytes)
    if tree_masks.tobytes() != flat_masks.tobytes() or tree_counts.tobytes() != flat_counts.tobytes():
        raise SystemExit(f"{name}: the two forms returned different masks")
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
    ap.add_argument("--leg", choices=["pairs", "queries"], default="pairs", help="queries: the region queries through both forms, --scene one of " + ", ".join(QUERY_WORKLOADS))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps((query_workload if args.leg == "queries" else workload)(args.scene, args.calls, args.warmup)))
        return
    me = [sys.executable, os.path.abspath(__file__), "--child", "--leg", args.leg, "--calls", str(args.calls), "--warmup", str(args.warmup)]
    scenes_of_leg = QUERY_WORKLOADS if args.leg == "queries" else SCENES
    for scene in (scenes_of_leg if args.scene == "all" else [args.scene]) + [f"seeded{n}" for n in args.sizes]:
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
