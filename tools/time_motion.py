#!/usr/bin/env python3
"""Times a free step (`ivx_world_step_enqueue` without contacts: one launch, plus the motion drivers' launch when a set is installed;
impact_amd/csrc/motion.hip) of a world of kinematic bodies under three driver sets:

  orbital   one orbital driver on every body (the dearest kind: Newton's iteration with two double-precision calls per round)
  mixed     one driver on every body, the five kinds in turn (what a wave of 64 lanes then holds)
  removed   the mixed set installed and removed again: the step a world without drivers takes

for 4 096 and for 65 536 kinematic bodies. Per case: milliseconds per step by device events over `--calls` steps after `--warmup` steps, on a
stream the events know; the timed calls are prepared ctypes calls. Each case runs in a child process under its own time limit.

  python tools/time_motion.py"""
import argparse
import json
import os
import signal
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = ["orbital", "mixed", "removed"]
SIZES = [4096, 65536]


def workload(case, n, calls, warmup):
    import numpy as np
    import torch

    import motion_ref as mr
    from impact_amd import capi, motion
    from impact_amd.physics import PhysicsWorld
    from impact_amd.voxel import Context

    stream = torch.cuda.Stream()
    ctx = Context(0, stream.cuda_stream)
    lib = capi.lib()
    rng = np.random.default_rng(1)
    kin = np.zeros(n, dtype=capi.KINEMATIC_BODY_DTYPE)
    kin["position"], kin["velocity"] = rng.uniform(-10, 10, (n, 3)), rng.uniform(-1, 1, (n, 3))
    kin["orientation"], kin["angular_axis"], kin["angular_speed"] = mr.random_orientations(rng, n), mr.random_directions(rng, n), rng.uniform(-3, 3, n)
    drivers = np.zeros(n, dtype=capi.MOTION_DRIVER_DTYPE)
    kinds = [mr.ORBITAL] if case == "orbital" else list(range(5))
    for j, kind in enumerate(kinds):
        rows = np.arange(j, n, len(kinds))
        drivers[rows] = mr.records(kind, mr.seeded(kind, len(rows), 7)[0])
    drivers["body"] = np.arange(n)
    w = PhysicsWorld(ctx)
    w.set_bodies(np.zeros(0, dtype=capi.RIGID_BODY_DTYPE), kin)
    md = motion.MotionDrivers(w)
    md.set(drivers)
    if case == "removed":
        md.clear()

    def step():
        rc = lib.ivx_world_step_enqueue(w.h, 0.004)
        if rc:
            capi.check(rc)

    for _ in range(warmup):
        step()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        start.record(stream)
        for _ in range(calls):
            step()
        stop.record(stream)
    stop.synchronize()
    out = {"case": case, "kinematic_bodies": n, "drivers": 0 if case == "removed" else n, "calls": calls, "warmup": warmup,
           "step_ms": start.elapsed_time(stop) / calls, "time": md.time}
    w.close()
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
    ap.add_argument("--case", choices=CASES + ["all"], default="all")
    ap.add_argument("--bodies", type=int, default=0, help="kinematic bodies (default: 4096 and 65536)")
    ap.add_argument("--calls", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--limit", type=int, default=120, help="time limit of each child process in seconds")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(workload(args.case, args.bodies, args.calls, args.warmup)))
        return
    me = [sys.executable, os.path.abspath(__file__), "--child", "--calls", str(args.calls), "--warmup", str(args.warmup)]
    for n in ([args.bodies] if args.bodies else SIZES):
        for case in (CASES if args.case == "all" else [args.case]):
            # (a case that fails or runs out of time ends the run: nothing more is started on the device)
            print(run_limited(me + ["--case", case, "--bodies", str(n)], args.limit).strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
