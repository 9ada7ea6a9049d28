"""Host-side checks of the drag phase of the force stage (impact_amd/csrc/forces.hip): `ivx_fg_apply_host_drag` — the code the kernel runs — against
the numpy restatement (tests/drag_stage_ref.py) byte for byte, the float32 restatement against its float64 version, the place of the phase in the
composition, a stage without a drag set against `ivx_fg_apply_host`, the validation errors, the layouts of the three records and the C++ setup
structs of include/impact_voxel.hpp against the Python constructors. No kernels are launched here."""
import functools
import os
import subprocess

import numpy as np
import pytest

import drag_stage_ref as dr
import forces_ref as fr
from impact_amd import capi, drag, forces

f32, f64 = np.float32, np.float64
N_THETAS = (1, 3, 8, 64)
SEED = 1
MEDIA = {"still air": forces.UniformMedium.still_air(), "moving water": forces.UniformMedium.moving_water((1.0, 2.0, -3.0))}
# The largest error of the float32 restatement against the float64 one over the seeded random bodies (both media, every n_theta), force relative to
# fs |load.force|, torque relative to ts |load.torque|, as measured and recorded in DESIGN.md (Detailed drag in the force stage); the test allows
# four times these.
MEASURED = (3.9e-7, 5.5e-7)
ALLOW = 4.0
EDGE_MARGIN = 1e-3  # cases whose float64 phi / cell or theta / cell lies this close to a cell edge are left out of THAT comparison only
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


@functools.lru_cache(maxsize=None)
def seeded_case(n_theta, medium_name):
    """a seeded scene with its float32 and float64 restatements: computed once, shared, never written"""
    scene = dr.seeded_scene(n_theta, MEDIA[medium_name], SEED)
    for v in [scene["drag"], scene["dynamic"], scene["random"]] + [m for m in scene["maps"] if m is not None]:
        v.setflags(write=False)
    d32, d64 = {}, {}
    return scene, dr.run(scene, f32, d32), d32, dr.run(scene, f64, d64), d64


def assert_same_bytes(got, want, what):
    bad = [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()]
    assert not bad, (f"{what}: {len(bad)} of {len(want)} bodies differ, first at {bad[0]}: force {got['total_force'][bad[0]]} != {want['total_force'][bad[0]]}, "
                     f"torque {got['total_torque'][bad[0]]} != {want['total_torque'][bad[0]]}")


# ---- 1. byte equality with the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("medium_name", list(MEDIA))
@pytest.mark.parametrize("n_theta", N_THETAS)
def test_apply_host_drag_equals_the_restatement_on_seeded_generators(n_theta, medium_name):
    scene, r32, d32, _, _ = seeded_case(n_theta, medium_name)
    assert len(scene["drag"]) == 2000 and len(set(scene["drag"]["map"])) == 3
    got, _ = dr.run_host(scene)
    assert_same_bytes(got, r32[0], f"n_theta {n_theta}, {medium_name}")
    d = d32["drag"]
    body = scene["drag"]["body"]
    at_rest = body[d["at_rest"]]
    zero3 = np.zeros(3, dtype=f32).tobytes()
    for b in at_rest:  # a body at rest in the medium carries no other generator here: its totals are the reset's +0.0
        assert got["total_force"][b].tobytes() == zero3 and got["total_torque"][b].tobytes() == zero3
    counts = np.bincount(body, minlength=len(scene["dynamic"]))
    assert (counts == 2).sum() >= 50 and counts.min() == 1, "two generators on one body"
    assert np.abs(got["total_force"][body[d["applies"]]]).max() > 0


def test_a_body_at_rest_in_the_medium_keeps_the_bytes_of_its_totals():
    """mass 2, momentum (2, 4, -6), medium (1, 2, -3): s2 == 0, and the totals another generator has made stay as they are"""
    rng = np.random.default_rng(3)
    dyn = fr.random_dynamic(rng, 1)
    dyn["mass"], dyn["momentum"] = 2.0, (2.0, 4.0, -6.0)
    maps, medium = [dr.random_map(rng, 8)], forces.UniformMedium.moving_air((1.0, 2.0, -3.0))
    other = [forces.local_force(0, (1.0, -2.0, 0.5), (0.3, 0.1, -0.2))]
    with_drag, _ = forces.apply_host(other, dyn, drag=[forces.detailed_drag(0, 0, 1.3, 2.0)], maps=maps, medium=medium)
    without, _ = forces.apply_host(other, dyn)
    assert with_drag.tobytes() == without.tobytes() and np.abs(without["total_torque"]).max() > 0
    moving = dyn.copy()
    moving["momentum"] = (2.0, 4.0, -5.0)
    assert forces.apply_host(other, moving, drag=[forces.detailed_drag(0, 0, 1.3, 2.0)], maps=maps, medium=medium)[0].tobytes() != forces.apply_host(other, moving)[0].tobytes()


def test_seeded_sets_contain_the_branches():
    """s2 > 0, s2 == 0, a negative phi wrapped, an index clamped. The fold of theta (theta_idx_of: a remainder above pi) is in the shared index
    function for the maps' region walk; the stage cannot reach it — theta is acos of a clamped argument rounded once, whose largest value is
    float32(pi) itself, which is not above it — and the restatement shows that it never does."""
    for n_theta in N_THETAS:
        for medium_name in MEDIA:
            d = seeded_case(n_theta, medium_name)[2]["drag"]
            counts = {k: int(d[k].sum()) for k in ("moving", "at_rest", "wrapped", "folded", "phi_clamped", "theta_clamped")}
            print(n_theta, medium_name, counts)
            assert counts["moving"] >= 100 and counts["at_rest"] >= 100 and counts["wrapped"] >= 100, counts
            assert int((d["phi_clamped"] | d["theta_clamped"]).sum()) >= 100, counts
            assert counts["folded"] == 0, counts


# ---- 2. the float32 restatement against float64 --------------------------------------------------------------------------------------------------------
def near_an_edge(d64):
    """float64 phi / cell within the margin of any cell edge (the row wraps), theta / cell within it of an interior edge"""
    n_theta = d64["n_theta"]
    phi_near = np.abs(d64["phi_cells"] - np.round(d64["phi_cells"])) < EDGE_MARGIN
    nearest = np.round(d64["theta_cells"])
    theta_near = (np.abs(d64["theta_cells"] - nearest) < EDGE_MARGIN) & (nearest >= 1) & (nearest <= n_theta - 1)
    return phi_near | theta_near


def test_float32_restatement_against_float64():
    """over the seeded random bodies (the hand-made ones sit on cell edges by construction)"""
    worst = [0.0, 0.0]
    for n_theta in N_THETAS:
        for medium_name in MEDIA:
            scene, _, d32, _, d64 = seeded_case(n_theta, medium_name)
            a, b = d32["drag"], d64["drag"]
            random = scene["random"]
            assert (a["applies"] == b["applies"])[random].all() and b["applies"][random].all()
            left_out = near_an_edge(b) & random
            share = left_out.sum() / random.sum()
            compared = random & ~left_out
            same_cell = (a["phi_idx"] == b["phi_idx"]) & (a["theta_idx"] == b["theta_idx"])
            assert same_cell[compared].all(), f"n_theta {n_theta}, {medium_name}: float32 and float64 look up different cells outside the margin at {np.flatnonzero(compared & ~same_cell)}"
            errs = []
            for name, unit in (("force", "force_scale"), ("torque", "torque_scale")):
                assert (b[unit][compared] > 0).all()
                errs.append(float((np.abs(a[name].astype(f64) - b[name])[compared].max(axis=1) / b[unit][compared]).max()))
            print(f"n_theta {n_theta}, {medium_name}: left out {100 * share:.2f} %, force {errs[0]:.3e}, torque {errs[1]:.3e}")
            assert share <= 0.01, share
            worst = [max(w, e) for w, e in zip(worst, errs)]
    print(f"drag: force {worst[0]:.3e} (recorded {MEASURED[0]:.1e}), torque {worst[1]:.3e} (recorded {MEASURED[1]:.1e})")
    assert worst[0] <= ALLOW * MEASURED[0] and worst[1] <= ALLOW * MEASURED[1]


# ---- 3. the place of the phase -----------------------------------------------------------------------------------------------------------------------
def composition_scene(seed):
    """body 1 carries a constant acceleration, a damped spring to a kinematic body, two drag generators, membership in a field of three and a gravity
    alignment torque"""
    rng = np.random.default_rng(seed)
    dyn, kin = fr.random_dynamic(rng, 3, spread=2.0), fr.random_kinematic(rng, 1, spread=2.0)
    dyn["position"] = fr.spread_positions(rng, 3, 2.0, 1.0)
    gens = np.array([forces.alignment_gravity(1, (0, 0, 1), 0.4, 0.3, 0.2), forces.spring_dynamic_kinematic(1, (0.1, 0.2, 0.0), 0, (0.0, 0.1, 0.0), forces.standard_spring(30.0, 1.5, 0.5)),
                     forces.constant_acceleration(1, (0.0, -9.81, 0.0))], dtype=capi.FORCE_GENERATOR_DTYPE)
    maps = [dr.random_map(rng, 8), dr.random_map(rng, 3)]
    drag_gens = [forces.detailed_drag(1, 1, 0.8, 1.5), forces.detailed_drag(1, 0, 1.2, 0.7)]
    return {"generators": gens, "dynamic": dyn, "kinematic": kin, "field": np.array([2, 1, 0], dtype=np.uint32), "g": 3.0, "drag": drag_gens, "maps": maps,
            "medium": forces.UniformMedium.still_air()}


def test_composition_has_the_drag_phase_between_the_springs_and_gravity():
    s = composition_scene(11)
    got, got_loads = forces.apply_host(s["generators"], s["dynamic"], s["kinematic"], s["field"], s["g"], drag=s["drag"], maps=s["maps"], medium=s["medium"])
    want, want_loads = dr.apply(s["generators"], s["dynamic"], s["kinematic"], s["field"], s["g"], s["drag"], s["maps"], s["medium"])
    wrong, _ = dr.apply(s["generators"], s["dynamic"], s["kinematic"], s["field"], s["g"], s["drag"], s["maps"], s["medium"], drag_after_gravity=True)
    assert want[1].tobytes() != wrong[1].tobytes(), "this seed does not tell drag-before-gravity from drag-after-gravity"
    assert_same_bytes(got, want, "composition")
    assert got_loads.tobytes() == want_loads.tobytes()
    # ... and inside the phase the list order
    swapped, _ = forces.apply_host(s["generators"], s["dynamic"], s["kinematic"], s["field"], s["g"], drag=s["drag"][::-1], maps=s["maps"], medium=s["medium"])
    assert_same_bytes(swapped, dr.apply(s["generators"], s["dynamic"], s["kinematic"], s["field"], s["g"], s["drag"][::-1], s["maps"], s["medium"])[0], "swapped")
    without, _ = forces.apply_host(s["generators"], s["dynamic"], s["kinematic"], s["field"], s["g"])
    assert without[1].tobytes() != got[1].tobytes() and without[[0, 2]].tobytes() == got[[0, 2]].tobytes()


# ---- 4. no drag set, and the vacuum --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", range(6), ids=fr.KIND_NAMES)
def test_without_a_drag_set_it_is_apply_host(kind):
    scenes = fr.seeded_gravity_alignment_scenes(2000, 1) if kind == fr.ALIGNMENT_GRAVITY else [fr.seeded_scene(kind, 2000, 1)]
    rng = np.random.default_rng(17)
    maps = [dr.random_map(rng, 8)]
    for s in scenes:
        plain = fr.run_host(s)
        for medium in (forces.UniformMedium.vacuum(), forces.UniformMedium.still_water()):
            got = forces.apply_host(s["generators"], s["dynamic"], s["kinematic"], s["field"], s["g"], drag=[], maps=maps, medium=medium)
            assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes()
        # the vacuum: every body drags through a medium without density — fs is zero, and adding a zero changes no byte
        everybody = [forces.detailed_drag(b, 0, 1.1, 1.5) for b in range(len(s["dynamic"]))]
        got = forces.apply_host(s["generators"], s["dynamic"], s["kinematic"], s["field"], s["g"], drag=everybody, maps=maps, medium=forces.UniformMedium.vacuum())
        assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes()


# ---- 5. validation and layout ----------------------------------------------------------------------------------------------------------------------------
BAD = {
    "body out of range": (forces.detailed_drag(3, 0, 1.0), "dynamic body 3"),
    "slot past the table": (forces.detailed_drag(0, 3, 1.0), "map slot 3"),
    "slot without a map": (forces.detailed_drag(0, 1, 1.0), "holds no drag load map"),
}


@pytest.mark.parametrize("name", list(BAD))
def test_validation_errors_name_the_generator_and_a_refused_call_writes_nothing(name):
    bad, says = BAD[name]
    rng = np.random.default_rng(41)
    dyn = fr.random_dynamic(rng, 3)
    maps = [dr.random_map(rng, 3), None, dr.random_map(rng, 1)]
    good = forces.detailed_drag(1, 2, 0.5)
    with pytest.raises(capi.IvxError) as e:
        forces.apply_host([], dyn, drag=[good, bad], maps=maps, medium=forces.UniformMedium.still_air())
    assert e.value.code == capi.IVX_ERR_INVALID and "generator 1" in str(e.value) and "detailed drag" in str(e.value) and says in str(e.value), str(e.value)
    d = np.array(dyn, copy=True)
    dg = forces._drag_records([good, bad])
    held = [m for m in maps]
    views = np.zeros(3, dtype=capi.DRAG_MAP_VIEW_DTYPE)
    for i, m in enumerate(held):
        if m is not None:
            views[i] = (m.ctypes.data, m.shape[0], 0)
    med = forces.UniformMedium.still_air().record().reshape(1)
    rc = capi.lib().ivx_fg_apply_host_drag(None, 0, None, 0, 1.0, capi.ptr(d), d.size, None, 0, None, capi.ptr(dg), dg.size, capi.ptr(views), views.size, capi.ptr(med))
    assert rc == capi.IVX_ERR_INVALID and d.tobytes() == dyn.tobytes()
    ok = capi.lib().ivx_fg_apply_host_drag(None, 0, None, 0, 1.0, capi.ptr(d), d.size, None, 0, None, capi.ptr(dg), 1, capi.ptr(views), views.size, capi.ptr(med))
    assert ok == capi.IVX_OK and d.tobytes() != dyn.tobytes()


def test_the_host_stage_still_refuses_a_seventh_kind_and_null_arguments():
    rng = np.random.default_rng(42)
    dyn = fr.random_dynamic(rng, 2)
    with pytest.raises(capi.IvxError) as e:
        forces.apply_host([forces._generator(6, 0, 0, [])], dyn, drag=[], maps=[], medium=None)
    assert e.value.code == capi.IVX_ERR_INVALID and "kind 6" in str(e.value)
    dg = forces._drag_records([forces.detailed_drag(0, 0, 1.0)])
    d = np.array(dyn, copy=True)
    assert capi.lib().ivx_fg_apply_host_drag(None, 0, None, 0, 1.0, capi.ptr(d), d.size, None, 0, None, capi.ptr(dg), 1, None, 1, None) == capi.IVX_ERR_INVALID
    assert d.tobytes() == dyn.tobytes()


def test_record_layouts_match_the_c_compiler(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "impact_voxel_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu\\n", sizeof(ivx_uniform_medium), offsetof(ivx_uniform_medium, mass_density), offsetof(ivx_uniform_medium, velocity));\n'
                   '    printf("%zu %zu %zu %zu %zu\\n", sizeof(ivx_drag_generator), offsetof(ivx_drag_generator, body), offsetof(ivx_drag_generator, map), '
                   'offsetof(ivx_drag_generator, drag_coefficient), offsetof(ivx_drag_generator, scaling));\n'
                   '    printf("%zu %zu %zu %zu\\n", sizeof(ivx_drag_map_view), offsetof(ivx_drag_map_view, loads), offsetof(ivx_drag_map_view, n_theta), '
                   'offsetof(ivx_drag_map_view, reserved));\n'
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    lines = [[int(x) for x in line.split()] for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    m, g, v = capi.UNIFORM_MEDIUM_DTYPE, capi.DRAG_GENERATOR_DTYPE, capi.DRAG_MAP_VIEW_DTYPE
    assert lines[0] == [m.itemsize, m.fields["mass_density"][1], m.fields["velocity"][1]] == [16, 0, 4]
    assert lines[1] == [g.itemsize] + [g.fields[f][1] for f in ("body", "map", "drag_coefficient", "scaling")] == [16, 0, 4, 8, 12]
    assert lines[2] == [v.itemsize] + [v.fields[f][1] for f in ("loads", "n_theta", "reserved")] == [16, 0, 8, 12]
    sizes = capi.extra_struct_sizes()
    assert sizes["ivx_uniform_medium"] == (m, 16) and sizes["ivx_drag_generator"] == (g, 16) and sizes["ivx_drag_map_view"] == (v, 16)
    for name in ("ivx_world_set_medium", "ivx_world_medium", "ivx_world_set_drag_map", "ivx_world_set_drag_map_from_grid", "ivx_world_drag_map_download",
                 "ivx_world_set_detailed_drag", "ivx_fg_apply_host_drag"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(capi.lib(), name)


CPP_PROGRAM = r"""
#include <cstdio>
#include "impact_voxel.hpp"
using namespace impact_voxel;
template <typename R>
static void dump(const R& r) {
    const unsigned char* b = reinterpret_cast<const unsigned char*>(&r);
    for (size_t i = 0; i < sizeof(r); ++i) std::printf("%02x", b[i]);
    std::printf("\n");
}
int main() {
    const float wind[3] = {1.0f, 2.0f, -3.0f};
    dump(UniformMedium::vacuum().record());
    dump(UniformMedium::still_air().record());
    dump(UniformMedium::moving_air(wind).record());
    dump(UniformMedium::still_water().record());
    dump(UniformMedium::moving_water(wind).record());
    dump(UniformMedium{0.4f, {0.5f, 0.25f, 0.125f}}.record());
    dump(DetailedDragForce{2u, 0.8f, 1.5f}.record(7));
    dump(DetailedDragForce{0u, 1.25f}.record(3));
    return 0;
}
"""


def test_cpp_setup_structs_make_the_records_of_the_python_constructors(tmp_path):
    src = tmp_path / "records.cpp"
    src.write_text(CPP_PROGRAM)
    exe = tmp_path / "records"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)  # (header-only: nothing of the library is used)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    wind = (1.0, 2.0, -3.0)
    U = forces.UniformMedium
    want = [U.vacuum().record(), U.still_air().record(), U.moving_air(wind).record(), U.still_water().record(), U.moving_water(wind).record(),
            U(0.4, (0.5, 0.25, 0.125)).record(), forces.detailed_drag(7, 2, 0.8, 1.5), forces.detailed_drag(3, 0, 1.25)]
    assert len(lines) == len(want)
    for i, w in enumerate(want):
        assert lines[i] == w.tobytes().hex(), (i, lines[i], w.tobytes().hex())


def test_against_the_single_body_host_call():
    """`ivx_drag_force_and_torque` divides where the stage multiplies by the reciprocal and takes atan2f / acosf: the two agree to tolerance; how many
    of the seeded random cases differ by at least one bit is printed (DESIGN.md records it)"""
    differ = total = 0
    worst = 0.0
    for n_theta in N_THETAS:
        scene, _, d32, _, _ = seeded_case(n_theta, "moving water")
        d = d32["drag"]
        rho, vm = dr.medium_of(scene["medium"])
        for j in np.flatnonzero(scene["random"])[:500]:
            gen = scene["drag"][j]
            body = np.array(scene["dynamic"][gen["body"]:gen["body"] + 1], copy=True)
            body["total_force"] = body["total_torque"] = 0
            drag.DetailedDragForce(drag.DragLoadMap(scene["maps"][gen["map"]]), float(gen["drag_coefficient"]), float(gen["scaling"])).apply(body, (vm, float(rho)))
            same_cell = True
            for name, scale_name in (("force", "force_scale"), ("torque", "torque_scale")):
                err = np.abs(body["total_" + name][0].astype(f64) - d[name][j].astype(f64)).max() / max(float(d[scale_name][j]), 1e-300)
                same_cell = same_cell and err < 1e-3  # (a case at a cell edge may look up the neighbouring cell)
                if same_cell:
                    worst = max(worst, err)
            total += 1
            differ += body["total_force"][0].tobytes() != d["force"][j].tobytes() or body["total_torque"][0].tobytes() != d["torque"][j].tobytes()
    print(f"ivx_drag_force_and_torque against the stage's arithmetic: {differ} of {total} seeded cases differ by at least one bit, largest relative difference {worst:.3e}")
    assert worst <= 1e-5 and total == 2000
