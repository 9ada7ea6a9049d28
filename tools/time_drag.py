#!/usr/bin/env python3
"""Times the drag load map of the config-2 asteroid (256^3, scenes.asteroid_scene(1.0)) at the default map configuration.

  python tools/time_drag.py            device-event times: `ivx_drag_load_map` (whole call: kernels, the map's copy back, the wait) and one
                                       `ivx_drag_loads` call for a single direction, after a warm-up
  python tools/time_drag.py --trace    the same workload once more in a child process under `rocprofv3 --kernel-trace --stats` (a run of its
                                       own: the trace slows the host side), then the average time of every drag kernel, the pairs/s of the
                                       load pass and its share of the FP32 vector peak

A (direction, triangle) pair is counted as 18 flops: the dot product (5), the max (1) and six multiply-adds (12); the peak is the MI355X
specification's 157.3 TFLOP/s. Pairs are counted over the triangle slots the pass walks (the index buffer's, freed ranges included)."""
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

FLOPS_PER_PAIR = 18.0
FP32_VECTOR_PEAK = 157.3e12


def workload(calls, warmup):
    import numpy as np
    import torch

    from impact_amd import drag, scenes
    from impact_amd.voxel import Context, SDFVoxelGenerator, VoxelObject, VoxelObjectInertialPropertyManager, VoxelObjectMesh

    stream = torch.cuda.Stream()
    ctx = Context(0, stream.cuda_stream)  # the library works on a stream torch knows, so torch's events time it
    obj = VoxelObject.generate(ctx, SDFVoxelGenerator(1.0, scenes.asteroid_scene(1.0)))
    mesh = VoxelObjectMesh.create(obj)
    com = np.asarray(VoxelObjectInertialPropertyManager.initialized_from(obj, np.ones(256, dtype=np.float32)).derive_center_of_mass(), dtype=np.float32)
    cfg = drag.DragLoadMapConfig()
    one_direction = drag.uniformly_distributed_radial_directions(3)[1:2]

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

    map_ms = timed(lambda: drag.DragLoadMap.compute_from_voxel_object_mesh(mesh, com, cfg.n_direction_samples, cfg.n_theta_coords, cfg.smoothness))
    one_ms = timed(lambda: drag.drag_loads_for_voxel_object(obj, com, one_direction))
    out = {"triangle_slots": mesh.n_indices() // 3, "submeshes": mesh.n_chunks(), "n_direction_samples": cfg.n_direction_samples, "n_theta_coords": cfg.n_theta_coords,
           "smoothness": cfg.smoothness, "drag_load_map_ms": map_ms, "drag_loads_one_direction_ms": one_ms, "calls": calls, "warmup": warmup}
    obj.close()
    ctx.close()
    return out


def kernel_times(db_path):
    db = sqlite3.connect(db_path)
    rows = db.execute("select name, count(*), avg(end-start) from kernels where name like '%k_drag_%' group by name order by 3 desc")
    return {name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: (int(n), float(avg_ns)) for name, n, avg_ns in rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", action="store_true", help="also run the workload under rocprofv3 --kernel-trace --stats and report the kernel times")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(workload(args.calls, args.warmup)))
        return
    out = workload(args.calls, args.warmup)
    if args.trace:
        tmp = tempfile.mkdtemp(prefix="time_drag_")
        try:
            subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "trace", "--", sys.executable, os.path.abspath(__file__), "--child", "--calls",
                            str(args.calls), "--warmup", str(args.warmup)], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
            dbs = [os.path.join(d, f) for d, _, fs in os.walk(tmp) for f in fs if f.endswith(".db")]
            times = kernel_times(sorted(dbs)[-1])
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        out["kernel_us"] = {k: round(v[1] / 1e3, 2) for k, v in times.items()}
        out["kernel_calls"] = {k: v[0] for k, v in times.items()}
        # the map's load pass is the four-directions-to-a-lane form of the kernel; the single direction runs the other one
        loads = times.get("k_drag_loads<4u>")
        if loads:
            out["load_pass_pairs_per_s"] = out["triangle_slots"] * out["n_direction_samples"] / (loads[1] * 1e-9)
            out["load_pass_share_of_fp32_vector_peak"] = out["load_pass_pairs_per_s"] * FLOPS_PER_PAIR / FP32_VECTOR_PEAK
    print(json.dumps(out))


if __name__ == "__main__":
    main()
