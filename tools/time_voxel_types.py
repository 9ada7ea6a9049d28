#!/usr/bin/env python3
"""Sample stage of a box with gradient-noise voxel types against the same box with SameVoxelTypeGenerator (the path without the type pass).

The object is the reference's generation benchmark generate_box_with_gradient_noise_voxel_types (4 types, noise frequency 0.02, voxel type
frequency 1.0, seed 0) over a box of half-extent 80: 11^3 = 1331 chunks. Each run is the sample stage of the resident-program step alone,
timed by the stage slot's own hipEvents (ivx_step_result::stage_ms[0]): warm-up steps, then --reps steps; min, median and max. The type
pass's time is the difference of the medians (the evaluator launches are the same in both runs), and the simplex4 rate is the typed
voxels times the type count over that time.

    python tools/time_voxel_types.py [--half-extent 80] [--types 4] [--reps 30] [--out profiles/voxel_types/timing.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from impact_amd import capi  # noqa: E402
from impact_amd.sdf_graph import SDFGraph, SDFNode  # noqa: E402
from impact_amd.voxel import Context, GradientNoiseVoxelTypeGenerator, SDFVoxelGenerator, VoxelObject  # noqa: E402


def stats(ms):
    return {"min_ms": float(np.min(ms)), "median_ms": float(np.median(ms)), "max_ms": float(np.max(ms)), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--half-extent", type=float, default=80.0)
    ap.add_argument("--types", type=int, default=4)
    ap.add_argument("--noise-frequency", type=float, default=0.02)
    ap.add_argument("--voxel-type-frequency", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 20

    graph = SDFGraph()
    graph.set_root_node(graph.add_node(SDFNode.new_box([2.0 * a.half_extent] * 3)))
    noise = GradientNoiseVoxelTypeGenerator(a.types, a.noise_frequency, a.voxel_type_frequency, a.seed)
    ctx = Context(0)
    out = {"half_extent": a.half_extent, "types": a.types, "noise_frequency": a.noise_frequency, "voxel_type_frequency": a.voxel_type_frequency,
           "seed": a.seed}
    runs = {}
    for key, types in (("same_voxel_type", 0), ("gradient_noise", noise), ("same_voxel_type_again", 0)):
        gen = SDFVoxelGenerator(1.0, graph, types)
        obj = VoxelObject(ctx, gen.chunk_counts(), 1.0)
        obj.set_sdf_program(gen)
        obj.set_stage_timing(1)  # the sample slot alone
        for _ in range(a.warmup):
            obj.step(capi.STAGE_SAMPLE)
        ms = [float(obj.step(capi.STAGE_SAMPLE)["stage_ms"][0]) for _ in range(a.reps)]
        runs[key] = stats(ms)
        if key == "gradient_noise":
            info = obj.download(sdf=False, types=False, flags=False, labels=False)[4]
            typed = (info["kind"] != 0) & ~((info["kind"] == 2) & ((info["flags"] & 0x40) != 0))
            out["chunks"] = int(obj.n_chunks)
            out["typed_chunks"] = int(typed.sum())
        obj.close()
    ctx.close()
    out["runs"] = runs
    base = min(runs["same_voxel_type"]["median_ms"], runs["same_voxel_type_again"]["median_ms"])
    diff = runs["gradient_noise"]["median_ms"] - base
    evals = out["typed_chunks"] * 4096 * a.types
    out["type_pass_ms"] = diff
    out["simplex4_evaluations"] = evals
    out["simplex4_evaluations_per_second"] = evals / (diff * 1e-3) if diff > 0 else None
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
