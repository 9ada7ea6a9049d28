#!/usr/bin/env python3
"""Times the collision pass of a frame with voxel objects among the collidables, the way it had to be made before `ivx_cw_collide_frame` and with
that call, in one run and on the same scenes:

  old   cw.collide -> cw.download -> bodies -> the dispatch on the host (tests/frame_ref.py) -> the two `_many` generators -> concatenate
  new   cw.collide_frame

  falling  tests/frame_ref.py's falling scene as it stands after 40 frames (two voxel objects, a ball, a capsule, a plane)
  static   tests/frame_ref.py's static scene (three voxel objects, 17 primitives, a plane)
  stress   the reference's stress shape: 1 000 small voxel boxes on a plane with a ball resting on each, >= 2 000 deferred pairs

Both paths end in a wait for the device, so a host clock around a call measures it. The two are timed alternately, `--calls` times each after
`--warmup` untimed rounds, and the medians are reported with the spread (min, max). The old path's time is given in two parts: the library calls
with their waits, and the host dispatch, which here is Python (a C caller's would be shorter; it is reported so that it is not mistaken for library
time). The wait counts are those of the calls made: collide 2, download 1, bodies 1, each `_many` call that has rows 2; collide_frame 2 with no
deferred pair, 3 with empty manifolds only, else 4. The merged lists of the two paths are compared byte for byte before anything is timed.

  python tools/time_cw_frame.py            all scenes, each in a child process under its own time limit"""
import argparse
import json
import os
import signal
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SCENES = ["falling", "static", "stress"]


def stress_scene(ctx, n_side):
    """n_side^2 voxel boxes (12 voxels of 0.25 across, an object each) resting on the plane y = 0, a ball of radius 0.5 resting on each"""
    import numpy as np

    import frame_ref as fr
    import narrow_ref as nr
    import parity_util as pu
    from impact_amd import capi, collision, scenes
    from impact_amd.voxel import VoxelObjectInertialPropertyManager, VoxelObjectMesh

    extent, graph = 0.25, scenes.box_scene((12.0, 12.0, 12.0))
    bodies, local, voxel_bodies = [], [], {}
    com = None
    for k in range(n_side * n_side):
        g = pu.gpu_from_graph(ctx, graph, extent)
        g.compute_all_derived_state()
        g.update_occupied_voxel_ranges()
        g.label_regions()
        g.mesh = VoxelObjectMesh.create(g)
        g.collision_probes_recompute()
        if com is None:
            com = VoxelObjectInertialPropertyManager.initialized_from(g, np.ones(256, dtype=np.float32)).derive_center_of_mass().astype(np.float32)
        x, z = 6.0 * (k % n_side), 6.0 * (k // n_side)
        bodies.append(nr.unit_body((x, 1.5 - 0.03, z), fr.axis_angle((0.2, 1.0, 0.1), 0.01 * (k % 7))))
        bodies.append(nr.unit_body((x + 0.1, 3.0 + 0.5 - 0.06, z - 0.1)))
        voxel_bodies[2 * k] = fr.DeviceBody(g, com.copy(), com.copy())
        local.append(fr.voxel_collidable(g, com, 2 * k, 10 + 2 * k, response=(0.0, 0.7, 0.5)))
        local.append(collision.sphere((0, 0, 0), 0.5, 2 * k + 1, 11 + 2 * k, response=(0.0, 0.7, 0.5)))
    local.append(collision.plane((0, 1, 0), 0.0, 0, 1, response=(0.0, 0.7, 0.5), kinematic=True))
    return np.array(local, dtype=capi.COLLIDABLE_DTYPE), np.array(bodies, dtype=capi.RIGID_BODY_DTYPE), fr.static_kinematic(), voxel_bodies


def workload(scene, calls, warmup, n_side):
    import numpy as np
    import torch

    import frame_ref as fr
    import test_gpu_frame as tg
    from impact_amd import capi, collision
    from impact_amd.physics import PhysicsWorld
    from impact_amd.voxel import Context

    stream = torch.cuda.Stream()
    ctx = Context(0, stream.cuda_stream)
    mode = capi.BV_DYNAMIC_PAIRS
    if scene == "stress":
        local, dyn, kin, voxel_bodies = stress_scene(ctx, n_side)
    else:
        if scene == "static":
            local, dyn, kin, made = fr.static_scene()
        else:
            local, _, kin, made = fr.falling_scene(*fr.falling_voxel_bodies())
            dyn = fr.oracle_run()["records"][39]["bodies"]
        voxel_bodies = {i: fr.DeviceBody(tg.device_object(ctx, vb), vb.center_of_mass.copy(), vb.origin_offset.copy()) for i, vb in made.items()}
    w = PhysicsWorld(ctx)
    w.set_bodies(dyn, kin)
    cw = collision.CollisionWorld(w)
    cw.set_collidables(local)
    cw.set_voxel_objects({i: (b.g, b.origin_offset, b.center_of_mass) for i, b in voxel_bodies.items()})
    cw.synchronize()
    parts = {}

    def old():
        t0 = time.perf_counter()
        contacts, deferred = cw.collide(mode, capacity=parts.get("cap"), deferred_capacity=parts.get("dcap"))
        world = cw.download()
        bodies = w.bodies()
        t1 = time.perf_counter()
        rows, mutual = fr.dispatch(world, deferred, bodies, voxel_bodies)
        t2 = time.perf_counter()
        manifolds = fr.device_manifolds(rows, mutual, voxel_bodies, len(deferred))
        merged = fr.merge(contacts, manifolds)
        t3 = time.perf_counter()
        parts.update(cap=len(contacts), dcap=len(deferred), waits=4 + 2 * (len(rows.queries) > 0) + 2 * (len(mutual.queries) > 0))
        return merged, (t1 - t0) + (t3 - t2), t2 - t1

    def new():
        t0 = time.perf_counter()
        merged, n_primitive, deferred, offsets = cw.collide_frame(mode, capacity=parts.get("total"), deferred_capacity=parts.get("dcap"))
        t1 = time.perf_counter()
        parts.update(total=len(merged), new_waits=2 if len(deferred) == 0 else (3 if len(merged) == n_primitive else 4), n_primitive=n_primitive)
        return merged, t1 - t0

    want, got = old()[0], new()[0]
    assert got.tobytes() == want.tobytes(), "the two paths disagree"
    for _ in range(warmup):
        old(), new()
    t_old, t_dispatch, t_new = [], [], []
    for _ in range(calls):  # (alternating: whatever else the machine is doing falls on both)
        _, calls_s, dispatch_s = old()
        t_old.append(calls_s), t_dispatch.append(dispatch_s)
        t_new.append(new()[1])

    def ms(values):
        return {"median": round(1e3 * statistics.median(values), 4), "min": round(1e3 * min(values), 4), "max": round(1e3 * max(values), 4)}

    out = {"scene": scene, "collidables": len(local), "voxel_objects": len(voxel_bodies), "deferred_pairs": parts["dcap"], "primitive_contacts": parts["n_primitive"],
           "contacts": parts["total"], "calls": calls, "warmup": warmup, "old_library_calls_ms": ms(t_old), "old_host_dispatch_python_ms": ms(t_dispatch),
           "new_collide_frame_ms": ms(t_new), "old_waits": parts["waits"], "new_waits": parts["new_waits"]}
    w.close()
    for b in voxel_bodies.values():
        b.g.close()
    ctx.close()
    return out


def run_limited(cmd, limit):
    """run `cmd` in a process group of its own; a time limit ends the whole group"""
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, start_new_session=True)
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
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--side", type=int, default=32, help="the stress scene holds side^2 voxel objects (32: 1 024)")
    ap.add_argument("--limit", type=int, default=240, help="time limit of each child process in seconds")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(workload(args.scene, args.calls, args.warmup, args.side)))
        return
    me = [sys.executable, os.path.abspath(__file__), "--child", "--calls", str(args.calls), "--warmup", str(args.warmup), "--side", str(args.side)]
    for scene in (SCENES if args.scene == "all" else [args.scene]):
        # (a step that fails or runs out of time ends the run: nothing more is started on the device)
        print(run_limited(me + ["--scene", scene], args.limit).strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
