#!/usr/bin/env python3
"""Times a free step (`ivx_world_step_enqueue` without contacts: one launch, plus the launches of the force stage when a set is installed;
impact_amd/csrc/forces.hip) of a world of dynamic bodies:

  none          no set: the step a world without force generators takes (this case uses nothing of the force stage, so the same file times the
                commit before it)
  acceleration  a constant acceleration on every body
  springs       the same and a damped spring between every body and the next
  removed       the acceleration set installed and removed again
  gravity       every body a member of the gravity field, no generators

`none`, `acceleration`, `springs` and `removed` for 4 096 and 65 536 dynamic bodies, `gravity` for fields of 64, 512 and 4 096. The gravity
kernel is serial per lane (a lane walks all partners of its body), so its time grows with the field, not with the field squared over the
lanes. Per case: milliseconds per step by device events over `--calls` steps (a quarter of them for a 512-body field, a fortieth for a
4 096-body field) after `--warmup` steps, on a stream the events know; the timed calls are prepared ctypes calls. Each case runs in a child
process under its own time limit.

  python tools/time_forces.py"""
import argparse
import json
import os
import signal
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEP_CASES = ["none", "acceleration", "springs", "removed"]
STEP_SIZES = [4096, 65536]
GRAVITY_SIZES = [64, 512, 4096]


def random_bodies(n):
    """n dynamic bodies on a lattice of spacing 2 (no two gravity partners closer than that), seeded orientations and momenta"""
    import numpy as np

    from impact_amd import capi

    rng = np.random.default_rng(1)
    d = np.zeros(n, dtype=capi.RIGID_BODY_DTYPE)
    d["mass"] = rng.uniform(0.5, 3.0, n)
    moments = rng.uniform(0.5, 2.0, (n, 3))
    for k in range(3):
        d["inertia"][:, 4 * k], d["inv_inertia"][:, 4 * k] = moments[:, k], 1.0 / moments[:, k]
    side = int(np.ceil(n ** (1 / 3)))
    i = np.arange(n)
    d["position"] = 2.0 * np.stack([i % side, (i // side) % side, i // (side * side)], axis=1)
    q = rng.normal(size=(n, 4))
    d["orientation"] = q / np.linalg.norm(q, axis=1)[:, None]
    d["momentum"], d["angular_momentum"] = rng.uniform(-1, 1, (n, 3)), rng.uniform(-1, 1, (n, 3))
    return d


def workload(case, n, calls, warmup):
    import numpy as np
    import torch

    from impact_amd import capi
    from impact_amd.physics import PhysicsWorld
    from impact_amd.voxel import Context

    stream = torch.cuda.Stream()
    ctx = Context(0, stream.cuda_stream)
    lib = capi.lib()
    w = PhysicsWorld(ctx)
    w.set_bodies(random_bodies(n), np.zeros(0, dtype=capi.KINEMATIC_BODY_DTYPE))
    n_generators = 0
    if case != "none":
        from impact_amd import forces

        fg = forces.ForceGenerators(w)
        if case == "gravity":
            fg.set_gravity(np.arange(n), 1.0)
            calls = max(50, calls // (1 if n <= 64 else 4 if n <= 512 else 40))
        else:
            gens = np.zeros(n, dtype=capi.FORCE_GENERATOR_DTYPE)
            gens["kind"], gens["body"] = capi.FG_CONSTANT_ACCELERATION, np.arange(n)
            gens["p"][:, 1] = -9.81
            if case == "springs":
                springs = np.zeros(n - 1, dtype=capi.FORCE_GENERATOR_DTYPE)
                springs["kind"], springs["body"], springs["body_b"] = capi.FG_SPRING_DYNAMIC_DYNAMIC, np.arange(n - 1), np.arange(1, n)
                springs["p"][:, 6:10] = (20.0, 0.5, 2.0, 0.0)
                gens = np.concatenate([gens, springs])
            fg.set(gens)
            n_generators = len(gens)
            if case == "removed":
                fg.clear()
                n_generators = 0

    def step():
        rc = lib.ivx_world_step_enqueue(w.h, 0.0001)
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
    out = {"case": case, "dynamic_bodies": n, "generators": n_generators, "calls": calls, "warmup": warmup, "step_ms": start.elapsed_time(stop) / calls}
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
    ap.add_argument("--case", choices=STEP_CASES + ["gravity", "all"], default="all")
    ap.add_argument("--bodies", type=int, default=0, help="dynamic bodies (default: 4096 and 65536; gravity: 64, 512 and 4096)")
    ap.add_argument("--calls", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--limit", type=int, default=120, help="time limit of each child process in seconds")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(workload(args.case, args.bodies, args.calls, args.warmup)))
        return
    me = [sys.executable, os.path.abspath(__file__), "--child", "--calls", str(args.calls), "--warmup", str(args.warmup)]
    for case in (STEP_CASES + ["gravity"] if args.case == "all" else [args.case]):
        for n in ([args.bodies] if args.bodies else GRAVITY_SIZES if case == "gravity" else STEP_SIZES):
            # (a case that fails or runs out of time ends the run: nothing more is started on the device)
            print(run_limited(me + ["--case", case, "--bodies", str(n)], args.limit).strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
