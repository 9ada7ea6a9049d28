#!/usr/bin/env python3
"""Times the SDF queries (`ivx_sdf_query_*`, impact_amd/csrc/sdf_query.hip): the sphere cast, `closest` and `points` (distance with gradient) at
64, 512 and 4 096 instances on three programs:

  leaf    one sphere
  union64 a smooth union of 64 leaves (190 nodes, two stack levels)
  noisy   a sphere under a multifractal noise node of three octaves

Per program, call and size: the whole call on the device (upload, kernel, download and wait: a host clock around a call that ends in a stream
synchronise; the median and the least of `--calls` calls after `--warmup` calls) and the same call through the host build (`ctx = NULL`, one
thread; the least of `--host-calls`) on the same machine, and that the two leave the same bytes. The cast runs with the reference's constants
(128 steps, tolerance 0.1, safety factor 0.5) from below the body; its mean step count is reported, since the work is proportional to it.

  python tools/time_sdf_query.py            all programs, each in a child process under its own time limit"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PROGRAMS = ["leaf", "union64", "noisy"]
SIZES = [64, 512, 4096]


def graph_of(program):
    import numpy as np

    from impact_amd.sdf_graph import SDFGraph, SDFNode

    g = SDFGraph()
    if program == "leaf":
        g.add_node(SDFNode.new_sphere(16.0))
    elif program == "noisy":
        g.add_node(SDFNode.new_multifractal_noise(g.add_node(SDFNode.new_sphere(16.0)), 3, 0.05, 2.0, 0.5, 1.0, 11))
    else:
        rng = np.random.default_rng(64)
        node = None
        for i in range(64):
            leaf = g.add_node(SDFNode.new_sphere(float(rng.uniform(3.0, 7.0))) if i % 2 else SDFNode.new_box([float(x) for x in rng.uniform(4.0, 10.0, 3)]))
            leaf = g.add_node(SDFNode.new_translation(leaf, [float(x) for x in rng.uniform(-14.0, 14.0, 3)]))
            node = leaf if node is None else g.add_node(SDFNode.new_union(node, leaf, 2.0))
    return g


def workload(program, calls, warmup, host_calls):
    import numpy as np

    import sdf_query_ref as R
    from impact_amd import sdf_query as sq
    from impact_amd.voxel import Context, SDFGenerator

    gen = SDFGenerator(graph_of(program))
    ctx = Context(0)
    dev, host = sq.SDFQuery(gen, ctx), sq.SDFQuery(gen, device=False)
    out = {"program": program, "nodes": len(gen.nodes), "stack_size": gen.required_forward_stack_size, "calls": calls, "warmup": warmup, "host_calls": host_calls}

    def clocked(fn, repeats, warm):
        for _ in range(warm):
            fn()
        times = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            r = fn()
            times.append((time.perf_counter() - t0) * 1e3)
        return r, float(np.median(times)), float(min(times))

    for n in SIZES:
        rng = np.random.default_rng(n)
        shells = R.shell_instances(gen, rng, n, spread=1.5)
        below = shells.copy()
        below["subject_to_parent"]["translation"][:, 1] = float(gen.domain[1]) - 6.0
        below["subject_to_parent"]["translation"][:, [0, 2]] *= np.float32(0.6)
        below["subject_to_parent"]["rotation"] = (0, 0, 0, 1)
        pts = np.ascontiguousarray(shells["subject_to_parent"]["translation"])
        for name, on in (("cast", lambda q: q.spherecast(None, below)), ("closest", lambda q: q.closest(None, shells)), ("points", lambda q: q.gradients(pts))):
            got, median_ms, least_ms = clocked(lambda: on(dev), calls, warmup)
            want, _, host_ms = clocked(lambda: on(host), host_calls, 0)
            rec = {"device_ms_median": round(median_ms, 4), "device_ms_least": round(least_ms, 4), "host_ms_least": round(host_ms, 3),
                   "same_bytes": bool(np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)))}
            if name != "points":
                rec["mean_steps"] = round(float(want["steps"].mean()), 2)
                rec["found"] = int((want["status"] == 0).sum())
            out[f"{name}_{n}"] = rec
    dev.close()
    ctx.close()
    return out


def run_limited(cmd, limit):
    """run `cmd` in a process group of its own; a time limit ends the whole group"""
    import signal

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
    ap.add_argument("--program", choices=PROGRAMS + ["all"], default="all")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="time limit of each child process in seconds")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(workload(args.program, args.calls, args.warmup, args.host_calls)))
        return
    me = [sys.executable, os.path.abspath(__file__), "--child", "--calls", str(args.calls), "--warmup", str(args.warmup), "--host-calls", str(args.host_calls)]
    for program in (PROGRAMS if args.program == "all" else [args.program]):
        # (a step that fails or runs out of time ends the run: nothing more is started on the device)
        print(run_limited(me + ["--program", program], args.limit).strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
