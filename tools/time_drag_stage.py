#!/usr/bin/env python3
"""Times a free step (`ivx_world_step_enqueue` without contacts: one launch, plus the launches of the force stage when a set is installed;
impact_amd/csrc/forces.hip) of a world of dynamic bodies with and without detailed drag:

  none          no set: the step a world without a force stage takes
  acceleration  a constant acceleration on every body
  drag          a detailed-drag generator on every body, all of them on ONE shared 64 x 128 map, in still air
  drag64        the same over 64 maps of 64 x 128, body b on map b % 64
  both          `acceleration` and `drag` together

`none` and `acceleration` use nothing of the drag phase, so the same file times the commit before it (copy it there): the two must not move,
since the path without a drag set runs the same instructions plus one uniform branch. Every case for 4 096 and 65 536 dynamic bodies. Per case:
milliseconds per step by device events over `--calls` steps after `--warmup` steps, on a stream the events know; the timed calls are prepared
ctypes calls. Each case runs in a child process under its own time limit.

  python tools/time_drag_stage.py"""
import argparse
import json
import os
import signal
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ["none", "acceleration", "drag", "drag64", "both"]
SIZES = [4096, 65536]
MAP_N_THETA = 64


def random_bodies(n):
    """n dynamic bodies on a lattice of spacing 2, seeded orientations and momenta"""
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
    n_generators = n_drag = n_maps = 0
    if case != "none":
        from impact_amd import forces

        fg = forces.ForceGenerators(w)
        if case in ("acceleration", "both"):
            gens = np.zeros(n, dtype=capi.FORCE_GENERATOR_DTYPE)
            gens["kind"], gens["body"] = capi.FG_CONSTANT_ACCELERATION, np.arange(n)
            gens["p"][:, 1] = -9.81
            fg.set(gens)
            n_generators = n
        if case in ("drag", "drag64", "both"):
            rng = np.random.default_rng(2)
            n_maps = 64 if case == "drag64" else 1
            for slot in range(n_maps):
                m = np.zeros((MAP_N_THETA, 2 * MAP_N_THETA), dtype=capi.DRAG_LOAD_DTYPE)
                m["force"], m["torque"] = rng.normal(size=m.shape + (3,)), rng.normal(size=m.shape + (3,))
                fg.set_drag_map(slot, m)
            fg.set_medium(forces.UniformMedium.still_air())
            dg = np.zeros(n, dtype=capi.DRAG_GENERATOR_DTYPE)
            dg["body"], dg["map"], dg["drag_coefficient"], dg["scaling"] = np.arange(n), np.arange(n) % n_maps, 0.5, 1e-3
            fg.set_drag(dg)
            n_drag = n

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
    out = {"case": case, "dynamic_bodies": n, "generators": n_generators, "drag_generators": n_drag, "maps": n_maps, "calls": calls, "warmup": warmup,
           "step_ms": start.elapsed_time(stop) / calls}
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
    ap.add_argument("--case", choices=CASES + ["all", "before"], default="all", help="`before`: the two cases the commit before the drag phase can run")
    ap.add_argument("--bodies", type=int, default=0, help="dynamic bodies (default: 4096 and 65536)")
    ap.add_argument("--calls", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=1, help="runs of every case (the run-to-run spread)")
    ap.add_argument("--limit", type=int, default=120, help="time limit of each child process in seconds")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(workload(args.case, args.bodies, args.calls, args.warmup)))
        return
    me = [sys.executable, os.path.abspath(__file__), "--child", "--calls", str(args.calls), "--warmup", str(args.warmup)]
    cases = CASES if args.case == "all" else ["none", "acceleration"] if args.case == "before" else [args.case]
    for case in cases:
        for n in ([args.bodies] if args.bodies else SIZES):
            for _ in range(args.repeat):
                # (a case that fails or runs out of time ends the run: nothing more is started on the device)
                print(run_limited(me + ["--case", case, "--bodies", str(n)], args.limit).strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
