"""The contact solver on bodies whose rotation matters: every body has a full symmetric positive definite inertia tensor in its body frame, a
random orientation and an angular velocity of order 1 rad/s (`physics_util.anisotropic_body`), so R I^-1 R^T is no multiple of the identity and
a transposed rotation, a misplaced or dropped tensor element or a write-back at the wrong orientation changes the result.

Every case runs on the kernel under test — `one_workgroup` (k_solve), `tile_dataflow` (k_solve_mg on 2..16 workgroups), `chain_stationary`
(k_solve_cs) — and asserts: `solver_info()` reports that kernel; its state and accumulated impulses equal the one-workgroup world's word for
word; it agrees with the oracle (`assert_bodies_close` 1e-5, `compare_contact_state` 1e-4); and, where the float64 restatement
(solver_ref.py) applies, with that at the same bars. The scenes are those of test_solver_ref_cpu.py, which pins oracle and restatement
against each other without a GPU."""
import numpy as np
import pytest

import oracle_lib as ol
import parity_util
import physics_util as pu
import solver_ref
import solver_scenes
from impact_amd.capi import CONTACT_DTYPE
from impact_amd.physics import ConstraintSolverConfig, PhysicsWorld
from solver_scenes import SMALL_GRAPH, SMALL_GRAPH_SEEDS

pytestmark = pytest.mark.gpu
KERNELS = ("one_workgroup", "tile_dataflow", "chain_stationary")
CLOSED = solver_scenes.closed_scenes()


def make_world(ctx, scene, kernel, groups):
    w = PhysicsWorld(ctx, ConstraintSolverConfig(*scene["config"]))
    w.set_bodies(scene["dyn"], scene["kin"])
    w.set_solver_groups({"one_workgroup": 1, "tile_dataflow": groups, "chain_stationary": 255}[kernel])
    return w


def assert_kernel(w, kernel, groups):
    info = w.solver_info()
    assert info["kernel"] == kernel, info
    if kernel != "chain_stationary":
        assert info["workgroups"] == (1 if kernel == "one_workgroup" else groups), info


def assert_same_words(w, w1, what):
    d, d1 = w.bodies(), w1.bodies()
    for f in pu.STATE_FIELDS:
        np.testing.assert_array_equal(d[0][f].view(np.uint32), d1[0][f].view(np.uint32), err_msg=f"{what} {f}")
    for f in ("position", "orientation", "velocity", "angular_axis", "angular_speed"):
        np.testing.assert_array_equal(np.atleast_1d(d[1][f]).view(np.uint32), np.atleast_1d(d1[1][f]).view(np.uint32), err_msg=f"{what} kinematic {f}")
    a, a1 = w.contact_state(), w1.contact_state()
    np.testing.assert_array_equal(a[0], a1[0], err_msg=f"{what} contact order")
    np.testing.assert_array_equal(a[1].view(np.uint32), a1[1].view(np.uint32), err_msg=f"{what} impulses")


def differing_words(w, o):
    (d, k), (od, ok) = w.bodies(), o.bodies()
    n = sum(int((d[f].view(np.uint32) != od[f].view(np.uint32)).sum()) for f in pu.STATE_FIELDS)
    return n + sum(int((np.atleast_1d(k[f]).view(np.uint32) != np.atleast_1d(ok[f]).view(np.uint32)).sum())
                   for f in ("position", "orientation", "velocity", "angular_axis", "angular_speed"))


def run_scene(ctx, scene, kernel, what, groups=3, restatement=True):
    """every frame of the scene on the kernel under test (and on one workgroup beside it), against the oracle and the restatement; returns
    the restatement and the number of state words that differed from the oracle's"""
    w = make_world(ctx, scene, kernel, groups)
    w1 = make_world(ctx, scene, "one_workgroup", groups) if kernel != "one_workgroup" else None
    o = ol.OraclePhysics(scene["dyn"], scene["kin"], scene["config"])
    ref = solver_ref.RefWorld(scene["dyn"], scene["kin"], scene["config"]) if restatement else None
    differing, turns = 0, []
    for frame, cs in enumerate(scene["frames"]):
        at = f"{what} [{kernel}] frame {frame}:"
        pu.step_both(w, o, cs, scene["dt"])
        if len(cs):
            assert_kernel(w, kernel, groups)
        if w1 is not None:
            w1.perform_physics_step(cs, scene["dt"])
            assert_same_words(w, w1, at)
        (d, k), (od, ok) = w.bodies(), o.bodies()
        pu.assert_bodies_close(d, od, what=at + " ")
        for f in ("position", "orientation", "velocity", "angular_axis", "angular_speed"):
            np.testing.assert_allclose(k[f], ok[f], rtol=1e-6, atol=1e-7, err_msg=f"{at} kinematic {f}")
        if len(cs):
            pu.compare_contact_state(w, o)
        differing += differing_words(w, o)
        if ref is not None:
            ref.step(cs, o.contact_order(), scene["dt"])
            turns.append(ref.largest_turn)
            pu.assert_bodies_close(d, ref.bodies()[0], what=at + " restatement: ")
            if len(cs):
                err = pu.impulse_error(w.contact_state()[1], ref.impulses)
                assert err <= 1e-4, f"{at} impulses against the restatement: {err:.2e}"
    w.close()
    if w1 is not None:
        w1.close()
    if ref is not None:
        ref.turns = turns  # per frame: the largest angle positional correction turned a dynamic body by
    return ref, differing


# ---- a. closed scenes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", list(CLOSED))
def test_closed_scenes(ctx, name, kernel):
    """two or three bodies, a few contacts: a contact that bounces, one that rests, one that separates, friction inside and on its circle, a
    four-contact manifold, a chain of three, a moving and spinning kinematic body as body B and as body A, a deep penetration"""
    ref, differing = run_scene(ctx, CLOSED[name], kernel, name)
    if name == "separating":  # no impulse, no correction: the state changes by the write-back round trip alone, and that is the oracle's to the bit
        assert not ref.impulses.any() and differing == 0
    if name == "deep":  # positional correction turned a body measurably, so writing L = R I R^T w at the corrected orientation matters
        assert ref.turns[0] > 1e-3


# ---- b. random contact graphs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("seed", parity_util.fuzz_seeds([51, 52, 53, 54]))
def test_random_graphs(ctx, seed, kernel):
    """8-60 bodies, manifolds of 1-9 contacts, a turned kinematic plane that moves and spins, five frames with contacts coming and going"""
    scene = solver_scenes.random_graph_scene(seed)
    _, differing = run_scene(ctx, scene, kernel, f"graph {seed}", groups=scene["groups"], restatement=False)
    # counted and printed, not required (the bar is 1e-5): 0 on the build and libm this was written on
    print(f"graph {seed} [{kernel}]: {differing} words of body state differ from the oracle's over {len(scene['frames'])} frames")


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("seed", SMALL_GRAPH_SEEDS)
def test_small_random_graphs_also_against_the_restatement(ctx, seed, kernel):
    """the small graphs whose every decision keeps the margin test_solver_ref_cpu.py asserts: held to the float64 restatement too"""
    scene = solver_scenes.random_graph_scene(seed, **SMALL_GRAPH)
    run_scene(ctx, scene, kernel, f"small graph {seed}", groups=scene["groups"])


# ---- c. configurations ----------------------------------------------------------------------------------------------------------------
CONFIGS = [(0, .4, 0, .2), (0, .4, 3, .2), (1, 0, 0, .2), (1, 1, 1, 1), (8, .4, 0, .2), (20, .4, 10, .5), (8, .4, 3, 0)]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: "-".join(str(v) for v in c))
def test_configurations(ctx, config, kernel):
    """warm start only, no positional phase (an empty second phase of the schedule), warm-start weight 0 and 1, correction factor 0 and 1,
    other iteration counts than 8 + 3: a 27-body pile, three frames, the middle one without half the manifolds"""
    run_scene(ctx, solver_scenes.anisotropic_pile(config), kernel, f"config {config}", groups=4, restatement=False)


# ---- d. sizes around the per-body kernels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n_dyn", [63, 64, 65, 255, 256, 257])
def test_body_counts_around_the_block_size(ctx, n_dyn, kernel):
    """k_prepare_bodies / k_pre_solve / k_post_solve run 256 bodies per block, dynamic then kinematic: the first, the last dynamic and the last
    kinematic body constrained, most bodies free; those keep momentum and angular momentum to the bit"""
    scene = solver_scenes.sparse_scene(n_dyn)
    free = np.setdiff1d(np.arange(n_dyn), scene["constrained"])
    assert len(free) > n_dyn // 2 and 0 in scene["constrained"] and n_dyn - 1 in scene["constrained"]
    w = make_world(ctx, scene, kernel, 2)
    w1 = make_world(ctx, scene, "one_workgroup", 2)
    o = ol.OraclePhysics(scene["dyn"], scene["kin"], scene["config"])
    for frame, cs in enumerate(scene["frames"]):
        pu.step_both(w, o, cs, scene["dt"])
        assert_kernel(w, kernel, 2)
        w1.perform_physics_step(cs, scene["dt"])
        assert_kernel(w1, "one_workgroup", 2)
        assert_same_words(w, w1, f"n_dyn {n_dyn} [{kernel}] frame {frame}:")
        (d, k), (od, ok) = w.bodies(), o.bodies()
        pu.assert_bodies_close(d, od, what=f"n_dyn {n_dyn} frame {frame}: ")
        pu.compare_contact_state(w, o)
        for f in ("position", "orientation", "velocity", "angular_axis", "angular_speed"):
            np.testing.assert_allclose(k[f], ok[f], rtol=1e-6, atol=1e-7, err_msg=f"n_dyn {n_dyn} frame {frame} kinematic {f}")
        for f in ("momentum", "angular_momentum"):
            np.testing.assert_array_equal(d[f][free].view(np.uint32), scene["dyn"][f][free].view(np.uint32), err_msg=f"free bodies' {f}")
    w.close()
    w1.close()


# ---- e. the stages one by one ----------------------------------------------------------------------------------------------------------
def staged_step(w, contacts, dt):
    """the order include/impact_voxel_hip.h gives for ivx_world_step; contacts = None: prepare again over the resident list"""
    if contacts is None:
        w.prepare_constraints_again()
    else:
        w.prepare_constraints(np.ascontiguousarray(contacts, dtype=CONTACT_DTYPE))
    w.advance_dynamic_rigid_body_momenta(dt)
    w.compute_and_apply_constrained_state()
    w.advance_rigid_body_configurations(dt)


@pytest.mark.parametrize("kernel", KERNELS)
def test_stages_one_by_one_are_the_step(ctx, kernel):
    """ivx_world_prepare / _advance_momenta / _solve / _advance_configurations (k_prepare_bodies, k_pre_solve, k_post_solve as launches of
    their own) against ivx_world_step on a second world: byte-equal over four frames of a random graph, then a frame that prepares the resident
    list again on both"""
    scene = solver_scenes.random_graph_scene(52)
    ws, wf = (make_world(ctx, scene, kernel, scene["groups"]) for _ in range(2))
    for frame, cs in enumerate(scene["frames"][:4]):
        staged_step(ws, cs, scene["dt"])
        wf.perform_physics_step(cs, scene["dt"])
        assert_kernel(ws, kernel, scene["groups"])
        assert_same_words(ws, wf, f"staged [{kernel}] frame {frame}:")
    staged_step(ws, None, scene["dt"])
    wf.step(scene["dt"])
    assert_same_words(ws, wf, f"staged [{kernel}] resident frame:")
    for w in (ws, wf):
        w.close()


def test_stages_without_contacts_are_the_free_step(ctx):
    """an empty contact list: the stages (three launches) against the fused free step (k_free_step) and the oracle"""
    scene = solver_scenes.sparse_scene(257)
    scene["dyn"]["total_force"] = np.random.default_rng(9).normal(0, 1.0, (257, 3)).astype(np.float32)
    scene["dyn"]["total_torque"] = np.random.default_rng(10).normal(0, 0.3, (257, 3)).astype(np.float32)
    ws, wf = (make_world(ctx, scene, "one_workgroup", 1) for _ in range(2))
    o = ol.OraclePhysics(scene["dyn"], scene["kin"], scene["config"])
    none = np.zeros(0, dtype=CONTACT_DTYPE)
    for frame in range(3):
        staged_step(ws, none if frame == 0 else None, scene["dt"])
        wf.step(scene["dt"])  # (no contact list ever set: the single-launch path)
        o.step(none, scene["dt"])
        assert_same_words(ws, wf, f"free frame {frame}:")
        pu.assert_bodies_close(ws.bodies()[0], o.bodies()[0], what=f"free frame {frame}: ")
    for w in (ws, wf):
        w.close()


# ---- f. body counts around the one-workgroup kernel's LDS limit -------------------------------------------------------------------------
@pytest.mark.parametrize("n_dyn", [5120, 5121, 5973, 5974])
def test_body_counts_around_the_lds_limit(ctx, n_dyn):
    """k_solve keeps a phase's mutable body state in LDS while it fits 143 360 bytes, at 24 bytes a body in the velocity phase and 28 in the
    positional phase (solve_plan.hpp): 5120 is the last count with both phases in LDS, 5121 the first with the positional phase in global
    memory (k_solve<false, 1>, both passes of a replay), 5973 the last with the velocity phase in LDS, 5974 the first with both in global
    memory (k_solve<false, 0>). Section (d)'s scene and asserts on one workgroup, word for word against a chain-stationary world"""
    scene = solver_scenes.sparse_scene(n_dyn)
    free = np.setdiff1d(np.arange(n_dyn), scene["constrained"])
    assert len(free) > n_dyn // 2 and 0 in scene["constrained"] and n_dyn - 1 in scene["constrained"]
    w = make_world(ctx, scene, "one_workgroup", 1)
    w2 = make_world(ctx, scene, "chain_stationary", 1)
    o = ol.OraclePhysics(scene["dyn"], scene["kin"], scene["config"])
    for frame, cs in enumerate(scene["frames"]):
        pu.step_both(w, o, cs, scene["dt"])
        assert_kernel(w, "one_workgroup", 1)
        w2.perform_physics_step(cs, scene["dt"])
        assert_kernel(w2, "chain_stationary", 1)
        assert_same_words(w, w2, f"n_dyn {n_dyn} frame {frame}:")
        (d, k), (od, ok) = w.bodies(), o.bodies()
        pu.assert_bodies_close(d, od, what=f"n_dyn {n_dyn} frame {frame}: ")
        pu.compare_contact_state(w, o)
        for f in ("position", "orientation", "velocity", "angular_axis", "angular_speed"):
            np.testing.assert_allclose(k[f], ok[f], rtol=1e-6, atol=1e-7, err_msg=f"n_dyn {n_dyn} frame {frame} kinematic {f}")
        for f in ("momentum", "angular_momentum"):
            np.testing.assert_array_equal(d[f][free].view(np.uint32), scene["dyn"][f][free].view(np.uint32), err_msg=f"free bodies' {f}")
    w.close()
    w2.close()
