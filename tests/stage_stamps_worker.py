"""What tests/test_gpu_stage_stamps.py shares with its child process: the small resident bodies, and the snapshot of everything a step leaves
behind (planes, chunk records, region labels, mesh buffers, step record). Run as a program — `stage_stamps_worker.py OUT_DIR BODY...` —
it steps every BODY twice with every slot timed and writes its snapshot and stage times to OUT_DIR/BODY.npz: the test starts it with IVX_STAGE_TIMING_EVENTS=1,
which the library reads once when it is loaded."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np

from impact_amd import capi, scenes
from impact_amd.voxel import SDFVoxelGenerator, VoxelObject, VoxelObjectMesh

# 5^3, 4^3 and 2^3 chunks (the last: k_step_post2 / k_step_assign at their smallest grids)
BODIES = {"asteroid5": lambda: scenes.asteroid_scene(0.25), "sphere4": lambda: scenes.sphere_scene(30.0), "sphere2": lambda: scenes.sphere_scene(12.0)}
DENSITIES = np.linspace(0.5, 2.0, 256).astype(np.float32)


def resident_object(ctx, body, ahead=False):
    gen = SDFVoxelGenerator(1.0, BODIES[body](), 0)
    obj = VoxelObject(ctx, gen.chunk_counts(), 1.0)
    obj.set_sdf_program(gen)
    obj.set_densities(DENSITIES)
    obj.set_sample_ahead(ahead)
    return obj


def snapshot(obj, res):
    """every byte the step left: name -> array"""
    sdf, typ, flg, lab, info = obj.download()
    mesh = VoxelObjectMesh(obj)
    mesh.counts = res["mesh"]
    pos, nrm, idx, im, sub = mesh.download()
    return {
        "sdf": sdf, "type": typ, "flags": flg, "labels": lab, "info": info.view(np.uint8), "region_labels": obj.region_labels(),
        "positions": pos.view(np.uint32), "normals": nrm.view(np.uint32), "indices": idx, "index_materials": np.ascontiguousarray(im).view(np.uint8),
        "submeshes": np.ascontiguousarray(sub).view(np.uint8),
        "mesh_counts": np.array([int(res["mesh"][k]) for k in ("n_vertices", "n_indices", "n_submeshes")], dtype=np.uint64),
        "region_count": np.array([int(res["region_count"])], dtype=np.uint64),
        "occupied": np.array(res["occupied"], dtype=np.uint32),
        "moments_m64": np.array(res["moments"]["m64"], dtype=np.float64).view(np.uint64),
        "moments_m32": np.array(res["moments"]["m32"], dtype=np.float32).view(np.uint32),
    }


def stepped_snapshot(ctx, body, mask):
    """BODY stepped twice under timing mask `mask` (the second step finds the mesh buffers and scratch words of the first): snapshot, stage_ms"""
    obj = resident_object(ctx, body)
    obj.set_stage_timing(mask)
    obj.step(capi.STAGE_ALL)
    res = obj.step(capi.STAGE_ALL).copy()
    snap = snapshot(obj, res)
    obj.close()
    return snap, np.array(res["stage_ms"], dtype=np.float64)


if __name__ == "__main__":  # stage_stamps_worker.py OUT_DIR BODY...
    from impact_amd.voxel import Context

    c = Context(0)
    try:
        for body in sys.argv[2:]:
            s, ms = stepped_snapshot(c, body, 0xFFFFFFFF)
            np.savez(os.path.join(sys.argv[1], body + ".npz"), stage_ms=ms, **s)
    finally:
        c.close()
