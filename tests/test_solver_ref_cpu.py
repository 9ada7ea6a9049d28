"""The float64 restatement of a contact step (solver_ref.py, written from the reference's text) against the C++ oracle (written line by line
from the same text, in f32), on the scenes the device tests use: no GPU needed. Two independent readings of the reference have to agree
on turned anisotropic bodies before either is used to judge the kernels.

Bars: body state through `assert_bodies_close` (1e-5), accumulated impulses at the 1e-4 of `compare_contact_state`. Every scene also asserts
the margin rule: the smallest relative margin by which the restatement took any decision (solver_ref.MARGIN_KINDS) is at least 100 times the
largest relative error observed between oracle and restatement in that scene (state and impulses, every frame) — so no decision of the
scene can fall differently in f32 and f64, and a disagreement would be a misreading, not rounding."""
import numpy as np
import pytest

import oracle_lib as ol
import physics_util as pu
import solver_ref
import solver_scenes

from solver_scenes import SMALL_GRAPH, SMALL_GRAPH_SEEDS

CLOSED = solver_scenes.closed_scenes()


def run_scene(scene, what):
    """every frame through oracle and restatement; returns (largest error, smallest margin with its kind, restatement)"""
    o = ol.OraclePhysics(scene["dyn"], scene["kin"], scene["config"])
    ref = solver_ref.RefWorld(scene["dyn"], scene["kin"], scene["config"])
    worst, tightest, ref.largest_impulse, ref.history = 0.0, (np.inf, None), 0.0, []
    for frame, cs in enumerate(scene["frames"]):
        n = o.step(cs, scene["dt"])
        assert n == len(cs), "an interlocked manifold: the restatement leaves those out"
        margins = ref.step(cs, o.contact_order(), scene["dt"])
        ref.history.append(dict(ref.counts, turn=ref.largest_turn, carrying=int((ref.impulses[:, 0] > 0.0).sum())))
        kind = min(margins, key=margins.get)
        tightest = min(tightest, (margins[kind], kind))
        od, ok = o.bodies()
        state_err, impulse_err = pu.body_state_error(ref.state64(), od), pu.impulse_error(ref.impulses, o.accumulated_impulses())
        err = max(state_err, impulse_err)
        worst = max(worst, err)
        ref.largest_impulse = max(ref.largest_impulse, float(ref.impulses[:, 0].max(initial=0.0)))
        print(f"{what} frame {frame}: {len(cs)} contacts, state error {state_err:.2e}, impulse error {impulse_err:.2e}, "
              f"tightest margin {margins[kind]:.2e} ({kind})")
        pu.assert_bodies_close(ref.bodies()[0], od, what=f"{what} frame {frame}: ")
        assert impulse_err <= 1e-4
        rk = ref.bodies()[1]
        for f in ("position", "orientation", "velocity", "angular_axis", "angular_speed"):
            np.testing.assert_allclose(rk[f], ok[f], rtol=1e-6, atol=1e-7, err_msg=f"{what} frame {frame} kinematic {f}")
    return worst, tightest, ref


@pytest.mark.parametrize("name", list(CLOSED))
def test_closed_scenes(name):
    """Measured oracle-to-restatement error (state or impulses, worst frame; the state alone stays below 2.5e-6) and tightest decision margin:
    bounce 2.6e-7 / 1.0e-2, rest 4.3e-6 / 1.0e-2, separating 3.6e-7 / 1.0e-2, stick 9.2e-6 / 1.0e-2, slide 1.0e-6 / 1.0e-2,
    manifold 3.6e-6 / 7.4e-3, chain 2.5e-6 / 1.0e-2, kinematic_b 2.7e-6 / 1.0e-2, kinematic_a 2.0e-6 / 1.0e-2, deep 3.9e-6 / 1.0e-2
    (1.0e-2: the warm-start dot products, 1 against 1 - 1e-2; the deep contact turns its bodies by 0.095 rad)."""
    worst, (margin, kind), ref = run_scene(CLOSED[name], name)
    assert margin >= 100.0 * worst, f"{name}: margin {margin:.2e} ({kind}) against an error of {worst:.2e}"
    # the scene is what its name says
    first, last = ref.history[0], ref.history[-1]
    print(name, ref.history)
    if name == "separating":
        assert ref.largest_impulse == 0.0 and not ref.impulses.any()
    else:
        assert first["carrying"] > 0
    if name == "bounce":
        assert first["bounce"] == 1
    if name == "rest":
        assert first["bounce"] == 0 and last["carrying"] == 1
    if name == "stick":  # slipping when prepared (dynamic coefficient), held inside the circle; at rest a frame later (static coefficient)
        assert first["dynamic_friction"] == 1 and first["inside_circle"] == 1
        assert last["static_friction"] == 1 and last["inside_circle"] == 1 and last["carrying"] == 1
    if name == "slide":
        assert first["on_circle"] == 1
    if name in ("chain", "kinematic_a", "kinematic_b"):  # still (or again) in contact after the first frame: warm starts count
        assert first["carrying"] == len(CLOSED[name]["frames"][0]) and last["carrying"] == first["carrying"]
    if name == "manifold":  # (a body that lands on four points while it spins rarely loads all four)
        assert all(h["carrying"] >= 2 for h in ref.history)
    if name == "deep":  # the corrected orientation differs measurably from the one the step started with
        assert first["turn"] > 1e-3, first["turn"]


@pytest.mark.parametrize("seed", SMALL_GRAPH_SEEDS)
def test_small_random_graphs(seed):
    """8-14 bodies, manifolds of 1-9 contacts, five frames of 14-49 contacts of which 2-14 carry an impulse. Measured error / tightest
    margin: seed 207 2.1e-6 / 5.8e-4 (bounce), 360 2.7e-6 / 5.7e-4 (depth), 391 4.0e-6 / 1.2e-3 (slip), 398 3.5e-6 / 9.2e-4 (normal clamp).
    Few seeds keep the rule: with dozens of contacts and eight sweeps a step takes thousands of clamp decisions, and one within 1e-4 of
    its threshold is common."""
    worst, (margin, kind), _ = run_scene(solver_scenes.random_graph_scene(seed, **SMALL_GRAPH), f"graph {seed}")
    assert margin >= 100.0 * worst, f"seed {seed}: margin {margin:.2e} ({kind}) against an error of {worst:.2e}"
