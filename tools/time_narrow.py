#!/usr/bin/env python3
"""Times the primitive collidable calls (`ivx_cw_*`, impact_amd/csrc/narrow.hip) on three scenes:

  pile      the 4 096 spheres of scenes.sphere_pile_scene(16) on a static plane, collidables in the scene's lattice order
  shuffled  the same collidables in a seeded random order (no coherence for the pair pass's block test to use), the plane still last
  mixed     65 536 collidables of the seeded recipe of tests/narrow_ref.py: spheres, capsules, voxel-object boxes, three planes last

Per scene: synchronize + collide per call (device events over `--calls` calls after `--warmup` calls, on a stream the events know; all timed
calls are prepared ctypes calls), each of the two alone, and the pairs, contacts and deferred pairs found.

  python tools/time_narrow.py            all scenes, each in a child process under its own time limit
  python tools/time_narrow.py --trace    also each scene once more under `rocprofv3 --kernel-trace --stats` (a run of its own) and the average
                                         time of every k_cw_ and k_bv_ kernel"""
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

SCENES = ["pile", "shuffled", "mixed"]


def workload(scene, calls, warmup):
    import ctypes as C

    import numpy as np
    import torch

    import narrow_ref as nr
    from impact_amd import capi, collision, scenes
    from impact_amd.physics import PhysicsWorld
    from impact_amd.voxel import Context

    stream = torch.cuda.Stream()
    ctx = Context(0, stream.cuda_stream)
    lib = capi.lib()
    if scene in ("pile", "shuffled"):
        dyn, _ = scenes.sphere_pile_scene(16, points_per_pair=1)
        kin = np.zeros(1, dtype=capi.KINEMATIC_BODY_DTYPE)
        kin["orientation"], kin["angular_axis"] = (0, 0, 0, 1), (0, 1, 0)
        order = np.random.default_rng(1).permutation(len(dyn)) if scene == "shuffled" else np.arange(len(dyn))
        response = (0.4, 0.7, 0.5)
        local = np.array([collision.sphere((0, 0, 0), 0.5, int(k), 1000 + int(k), response=response) for k in order] +
                         [collision.plane((0, 1, 0), -0.475, 0, 1, response=response, kinematic=True)], dtype=capi.COLLIDABLE_DTYPE)
    else:
        local, dyn, kin = (np.array(a) for a in nr.scene(65536))
    w = PhysicsWorld(ctx)
    w.set_bodies(dyn, kin)
    cw = collision.CollisionWorld(w)
    cw.set_collidables(local)
    n = len(local)
    found, deferred_found = C.c_size_t(0), C.c_size_t(0)

    def synchronize_call():
        rc = lib.ivx_cw_synchronize(w.h)
        if rc:
            capi.check(rc)

    synchronize_call()
    rc = lib.ivx_cw_collide(w.h, capi.BV_DYNAMIC_PAIRS, None, 0, C.byref(found), None, 0, C.byref(deferred_found))
    if rc:
        capi.check(rc)
    cap, dcap = found.value, deferred_found.value
    contacts, deferred = np.zeros(max(1, cap), dtype=capi.CONTACT_DTYPE), np.zeros((max(1, dcap), 2), dtype=np.uint32)

    def collide_call():
        rc = lib.ivx_cw_collide(w.h, capi.BV_DYNAMIC_PAIRS, contacts.ctypes.data, cap, C.byref(found), deferred.ctypes.data, dcap, C.byref(deferred_found))
        if rc:
            capi.check(rc)

    def frame():
        synchronize_call()
        collide_call()

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

    out = {"scene": scene, "collidables": n, "calls": calls, "warmup": warmup}
    out["synchronize_collide_ms"] = timed(frame)
    out["synchronize_ms"], out["collide_ms"] = timed(synchronize_call), timed(collide_call)
    pairs = C.c_size_t(0)
    rc = lib.ivx_bv_pairs(ctx.h, capi.BV_DYNAMIC_PAIRS, None, 0, C.byref(pairs))
    if rc:
        capi.check(rc)
    out["pairs"], out["contacts"], out["deferred_pairs"] = int(pairs.value), int(found.value), int(deferred_found.value)
    w.close()
    ctx.close()
    return out


def kernel_times(db_path):
    db = sqlite3.connect(db_path)
    rows = db.execute("select name, count(*), avg(end-start) from kernels where name like '%k_cw_%' or name like '%k_bv_%' group by name order by 3 desc")
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
            tmp = tempfile.mkdtemp(prefix="time_narrow_")
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
