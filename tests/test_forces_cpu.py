"""Host-side checks of the force generators and dynamic gravity (impact_amd/csrc/forces.hip): `ivx_fg_apply_host` — the code the kernels run —
against the numpy restatement (tests/forces_ref.py) byte for byte, the float32 restatement against its float64 version, the validation errors,
the record's layout, and the C++ setup structs of include/impact_voxel.hpp against the Python constructors. No kernels are launched here."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import forces_ref as fr
from impact_amd import capi, forces

f32, f64 = np.float32, np.float64
N_SEEDED, SEED = 2000, 1
GRAVITY_FIELDS = (2, 3, 17, 64)
# The largest error of the float32 restatement against the float64 one over the seeded scenes, relative to the case's scale, as measured and
# recorded in DESIGN.md (Force generators); the tests allow four times these. (force, torque); None: the kind has no such output. The scales:
#   constant acceleration  |acceleration| * mass
#   local force            |force|;  |force| * |point|
#   springs                S = |stiffness| * (length + |rest_length|) + |damping| * (|v1| + |v2|) (the speeds of the two attachment points);  S * the arm of
#                          the attachment point about the centre of mass
#   alignment torques      max|I| * (nf^2 * pi + (2 nf + spin frequency + precession frequency) * |w|) + |w| * |L|
#   gravity                the sum of the pair-force (pair-torque) magnitudes on the body, in float64 — not the net load, which cancels
MEASURED = {
    fr.CONSTANT_ACCELERATION: (5.8e-8, None),
    fr.LOCAL_FORCE: (2.1e-7, 1.1e-6),
    fr.SPRING_DD: (2.4e-7, 1.4e-6),
    fr.SPRING_DK: (2.3e-7, 1.6e-6),
    fr.ALIGNMENT_FIXED: (None, 9.2e-7),
    fr.ALIGNMENT_GRAVITY: (None, 2.6e-6),
    "gravity": (5.6e-7, 2.9e-6),
}
ALLOW = 4.0


def freeze(scene):
    for v in scene.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return scene


@functools.lru_cache(maxsize=None)
def seeded_case(kind):
    """the scenes of a kind with the float32 and float64 restatements of each: computed once, shared, never written"""
    scenes = fr.seeded_gravity_alignment_scenes(N_SEEDED, SEED) if kind == fr.ALIGNMENT_GRAVITY else [fr.seeded_scene(kind, N_SEEDED, SEED)]
    out = []
    for scene in scenes:
        d32, d64 = {}, {}
        r32, r64 = fr.run(scene, f32, d32), fr.run(scene, f64, d64)
        out.append((freeze(scene), r32, d32, r64, d64))
    assert sum(len(s[0]["generators"]) for s in out) == N_SEEDED
    return out


@functools.lru_cache(maxsize=None)
def gravity_case(n):
    scene = freeze(fr.gravity_scene(n, SEED))
    d32, d64 = {}, {}
    return scene, fr.run(scene, f32, d32), d32, fr.run(scene, f64, d64), d64


def assert_same_bytes(got, want, what):
    got_dyn, got_loads = got
    want_dyn, want_loads = want
    bad = [i for i in range(len(want_dyn)) if got_dyn[i].tobytes() != want_dyn[i].tobytes()]
    assert not bad, (f"{what}: {len(bad)} of {len(want_dyn)} bodies differ, first at {bad[0]}: force {got_dyn['total_force'][bad[0]]} != {want_dyn['total_force'][bad[0]]}, "
                     f"torque {got_dyn['total_torque'][bad[0]]} != {want_dyn['total_torque'][bad[0]]}")
    assert got_loads.tobytes() == want_loads.tobytes(), f"{what}: gravity loads differ at {np.flatnonzero((got_loads.view(np.uint32) != want_loads.view(np.uint32)).any(axis=1))}"


# ---- byte equality with the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", range(6), ids=fr.KIND_NAMES)
def test_apply_host_equals_the_restatement_on_seeded_generators(kind):
    for i, (scene, r32, _, _, _) in enumerate(seeded_case(kind)):
        got = fr.run_host(scene)
        assert_same_bytes(got, r32, f"{fr.KIND_NAMES[kind]} scene {i}")
        assert got[0]["total_force"].tobytes() != scene["dynamic"]["total_force"].tobytes()  # (the host-set totals are gone)


@pytest.mark.parametrize("n", GRAVITY_FIELDS)
def test_apply_host_equals_the_restatement_on_gravity_fields(n):
    scene, r32, _, _, _ = gravity_case(n)
    got = fr.run_host(scene)
    assert_same_bytes(got, r32, f"field of {n}")
    assert np.abs(got[1]).min() > 0 and got[0]["total_force"].tobytes() == got[1][:, 0:3].tobytes()  # (field order is body order here)


def test_seeded_sets_contain_the_branches():
    for kind in (fr.SPRING_DD, fr.SPRING_DK):
        d = seeded_case(kind)[0][2][kind]
        for branch in ("coincident", "undamped", "slack", "plain"):
            assert d[branch].sum() >= 100, (fr.KIND_NAMES[kind], branch, int(d[branch].sum()))
    d = seeded_case(fr.ALIGNMENT_FIXED)[0][2]["alignment"]
    assert (d["fallback"] & (d["cosine"] > 0)).sum() >= 100 and (d["fallback"] & (d["cosine"] < 0)).sum() >= 100, "the fallback axis, parallel and antiparallel"
    assert (~d["fallback"]).sum() >= 100
    counts = {k: sum(int(s[2]["alignment"][k].sum()) for s in seeded_case(fr.ALIGNMENT_GRAVITY)) for k in ("not_in_field", "weak_load", "applies")}
    assert min(counts.values()) >= 100, counts


HAND_MADE = fr.hand_made()


@pytest.mark.parametrize("name,scene", HAND_MADE, ids=[c[0] for c in HAND_MADE])
def test_apply_host_equals_the_restatement_on_hand_made_cases(name, scene):
    diag = {}
    want = fr.run(scene, f32, diag)
    got = fr.run_host(scene)
    assert_same_bytes(got, want, name)
    dyn, loads = got
    zero6 = np.zeros(6, dtype=f32).tobytes()
    if "coincident points" in name:
        kind = fr.SPRING_DK if " dk " in name else fr.SPRING_DD
        assert diag[kind]["coincident"].all() and (dyn["total_force"] == 0).all() and (dyn["total_torque"] == 0).all()
    if "undamped" in name or "damping at epsilon" in name:
        assert diag[fr.SPRING_DK if " dk " in name else fr.SPRING_DD]["undamped"].all()
    if "just above epsilon" in name:
        assert diag[fr.SPRING_DD]["plain"].all()
    if "slack band" in name:
        assert diag[fr.SPRING_DK if " dk " in name else fr.SPRING_DD]["slack"].all() and (dyn["total_force"] == 0).all()
    if "taut band" in name or name == "spring dk damped":
        assert np.abs(dyn["total_force"]).max() > 0
    if "fallback" in name:
        assert diag["alignment"]["fallback"].all() and np.isfinite(dyn["total_torque"]).all() and np.abs(dyn["total_torque"][0]).max() > 0
        if "antiparallel" in name or "-z" in name:
            assert diag["alignment"]["cosine"][0] < 0
    if name == "alignment plain":
        assert not diag["alignment"]["fallback"].any()
    if name in ("gravity alignment outside the field", "gravity alignment without a field"):
        assert diag["alignment"]["not_in_field"].all()
    if name in ("gravity alignment under a negligible load", "gravity alignment in a field of one"):
        assert diag["alignment"]["weak_load"].all()
    if name == "gravity alignment in the field":
        assert diag["alignment"]["applies"].all()
        without, _ = forces.apply_host([], scene["dynamic"], scene["kinematic"], scene["field"], scene["g"])
        assert dyn["total_torque"][1].tobytes() != without["total_torque"][1].tobytes() and dyn["total_force"].tobytes() == without["total_force"].tobytes()
    if name == "gravity alignment in a field of one" or name == "gravity field of one":
        assert loads.tobytes() == zero6
    if name == "coincident gravity bodies":
        assert np.isfinite(loads).all() and np.isfinite(dyn["total_force"]).all()
        two, _ = forces.apply_host([], scene["dynamic"][:2], (), [0, 1], scene["g"])
        assert (two["total_force"] == 0).all() and (two["total_torque"] == 0).all(), "r = 0 gives zero, not NaN"
    if name == "gravity field of two":
        assert loads[0, 0:3].tobytes() == (-loads[1, 0:3] + f32(0)).tobytes() and np.abs(loads).min() > 0
        assert dyn["total_force"][2].tobytes() == loads[0, 0:3].tobytes() and (dyn["total_force"][1] == 0).all()


def test_the_reset_reaches_every_body_and_the_order_in_a_phase_is_the_list_order():
    rng = np.random.default_rng(31)
    dyn = fr.random_dynamic(rng, 6)
    got, _ = forces.apply_host([forces.constant_acceleration(4, [1, 2, 3])], dyn)
    zero3 = np.zeros(3, dtype=f32).tobytes()
    for b in (0, 1, 2, 3, 5):
        assert got["total_force"][b].tobytes() == zero3 and got["total_torque"][b].tobytes() == zero3  # (+0.0, whatever the host had set)
    differ = 0
    for seed in range(40):
        p = fr.seeded_parameters(fr.LOCAL_FORCE, 3, np.random.default_rng(100 + seed))
        gens = fr.generators(fr.LOCAL_FORCE, 2, 0, p)
        results = []
        for order in ([0, 1, 2], [2, 1, 0]):
            got = forces.apply_host(gens[order], dyn)
            assert_same_bytes(got, fr.apply(gens[order], dyn), f"seed {seed}")
            results.append(got[0])
        differ += results[0].tobytes() != results[1].tobytes()
    assert differ > 0, "no seeded triple distinguishes the two orders"


# ---- the float32 restatement against float64 ------------------------------------------------------------------------------------------------------
def relative_errors(r32, d64, bodies, force_scale, torque_scale):
    """largest |float32 - float64| component of the totals of `bodies`, relative to the scales"""
    dyn32 = r32[0]
    out = []
    for name, total, unit in (("total_force", d64["force"], force_scale), ("total_torque", d64["torque"], torque_scale)):
        if unit is None or len(bodies) == 0:
            out.append(None)
            continue
        err = np.abs(dyn32[name][bodies].astype(f64) - total[bodies]).max(axis=1)
        assert (unit > 0).all()
        out.append(float((err / unit).max()))
    return out


def norm(v):
    return np.sqrt((np.asarray(v, dtype=f64) ** 2).sum(axis=-1))


def kind_errors(kind):
    worst = [None, None]
    for scene, r32, d32, r64, d64 in seeded_case(kind):
        gens = scene["generators"]
        p, body = gens["p"].astype(f64), gens["body"].astype(np.int64)
        if kind == fr.CONSTANT_ACCELERATION:
            errs = relative_errors(r32, d64, body, norm(p[:, 0:3]) * scene["dynamic"]["mass"][body], None)
        elif kind == fr.LOCAL_FORCE:
            errs = relative_errors(r32, d64, body, norm(p[:, 0:3]), norm(p[:, 0:3]) * norm(p[:, 3:6]))
        elif kind in (fr.SPRING_DD, fr.SPRING_DK):
            d = d64[kind]
            live = ~d["coincident"] & ~d["slack"]
            same_branch = (d32[kind]["coincident"] == d["coincident"]) & (d32[kind]["slack"] == d["slack"]) & (d32[kind]["undamped"] == d["undamped"])
            assert same_branch.all()
            errs = relative_errors(r32, d64, body[live], d["force_scale"][live], (d["force_scale"] * d["arm_1"])[live])
            if kind == fr.SPRING_DD:
                second = relative_errors(r32, d64, gens["body_b"].astype(np.int64)[live], d["force_scale"][live], (d["force_scale"] * d["arm_2"])[live])
                errs = [max(a, b) for a, b in zip(errs, second)]
        else:
            d = d64["alignment"]
            # left out of THIS comparison only: the fallback axis. The seeded directions along and against the axis are exact in float32 alone (the
            # float64 cross product of the same inputs is 1e-8 long and takes the other branch), and at such a direction the rotation axis, and with
            # it the split of the angular velocity, is arbitrary
            live = d["applies"] & d32["alignment"]["applies"] & ~d["fallback"] & ~d32["alignment"]["fallback"]
            assert (d["applies"] == d32["alignment"]["applies"]).all()
            errs = relative_errors(r32, d64, body[live], None, d["torque_scale"][live])
        worst = [e if w is None else (w if e is None else max(w, e)) for w, e in zip(worst, errs)]
    return worst


@pytest.mark.parametrize("kind", range(6), ids=fr.KIND_NAMES)
def test_float32_restatement_against_float64(kind):
    err_force, err_torque = kind_errors(kind)
    bound_force, bound_torque = MEASURED[kind]
    print(f"{fr.KIND_NAMES[kind]}: force {err_force} (recorded {bound_force}), torque {err_torque} (recorded {bound_torque})")
    assert (err_force is None) == (bound_force is None) and (err_torque is None) == (bound_torque is None)
    assert err_force is None or err_force <= ALLOW * bound_force
    assert err_torque is None or err_torque <= ALLOW * bound_torque


def test_float32_gravity_against_float64():
    """relative to the sum of the pair-force magnitudes on the body (the net force cancels), positions no closer than 1 so that the reference's own
    EPS terms stay small"""
    worst_force = worst_torque = 0.0
    for n in GRAVITY_FIELDS:
        scene, r32, _, _, d64 = gravity_case(n)
        field = scene["field"].astype(np.int64)
        g = d64["gravity"]
        err_force, err_torque = relative_errors(r32, d64, field, g["pair_force_sum"], g["pair_torque_sum"])
        print(f"field of {n}: force {err_force:.3e}, torque {err_torque:.3e}")
        worst_force, worst_torque = max(worst_force, err_force), max(worst_torque, err_torque)
    print(f"gravity: force {worst_force:.3e} (recorded {MEASURED['gravity'][0]:.1e}), torque {worst_torque:.3e} (recorded {MEASURED['gravity'][1]:.1e})")
    assert worst_force <= ALLOW * MEASURED["gravity"][0] and worst_torque <= ALLOW * MEASURED["gravity"][1]


# ---- validation and layout ---------------------------------------------------------------------------------------------------------------------
Z3, X3 = [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]
SPRING = forces.standard_spring(1.0, 0.1, 1.0)
BAD_GENERATORS = {
    "unknown kind": (forces._generator(6, 0, 0, []), "kind 6"),
    "body out of range": (forces.constant_acceleration(3, X3), "body 3"),
    "spring second dynamic body out of range": (forces.spring_dynamic_dynamic(0, Z3, 3, Z3, SPRING), "dynamic-dynamic spring"),
    "spring between a body and itself": (forces.spring_dynamic_dynamic(2, Z3, 2, X3, SPRING), "both ends"),
    "spring kinematic body out of range": (forces.spring_dynamic_kinematic(0, Z3, 2, Z3, SPRING), "kinematic body 2"),
    "settling time zero": (forces.alignment_fixed(0, X3, X3, 0.0, 0.1, 0.1), "settling time"),
    "settling time negative": (forces.alignment_gravity(0, X3, -1.0, 0.1, 0.1), "gravity alignment torque"),
    "settling time nan": (forces.alignment_fixed(0, X3, X3, math.nan, 0.1, 0.1), "settling time"),
}


@pytest.mark.parametrize("name", list(BAD_GENERATORS))
def test_validation_errors_name_the_generator(name):
    bad, says = BAD_GENERATORS[name]
    rng = np.random.default_rng(41)
    dyn, kin = fr.random_dynamic(rng, 3), fr.random_kinematic(rng, 2)
    good = forces.constant_acceleration(0, X3)
    with pytest.raises(capi.IvxError) as e:
        forces.apply_host([good, bad], dyn, kin)
    assert e.value.code == capi.IVX_ERR_INVALID and "generator 1" in str(e.value) and says in str(e.value), str(e.value)


def test_gravity_field_validation_and_a_refused_call_leaves_the_bodies():
    rng = np.random.default_rng(42)
    dyn = fr.random_dynamic(rng, 4)
    for field, says in (([0, 1, 4], "member 2"), ([0, 2, 1, 2], "member 3")):
        with pytest.raises(capi.IvxError) as e:
            forces.apply_host([], dyn, (), field)
        assert e.value.code == capi.IVX_ERR_INVALID and says in str(e.value), str(e.value)
    # a refused call writes nothing: the caller's bodies keep their totals (what "the set in force stays" is on the host side), and the set that
    # was good before still applies
    good = [forces.constant_acceleration(1, X3)]
    before = dyn.copy()
    d = np.array(dyn, copy=True)
    g = forces._records(good + [forces.constant_acceleration(4, X3)])
    rc = capi.lib().ivx_fg_apply_host(capi.ptr(g), g.size, None, 0, 1.0, capi.ptr(d), d.size, None, 0, None)
    assert rc == capi.IVX_ERR_INVALID and d.tobytes() == before.tobytes()
    assert_same_bytes(forces.apply_host(good, dyn), fr.apply(good, dyn), "the good set")
    with pytest.raises(capi.IvxError) as e:
        capi.check(capi.lib().ivx_fg_apply_host(None, 1, None, 0, 1.0, None, 0, None, 0, None))
    assert e.value.code == capi.IVX_ERR_INVALID


def test_damping_frequencies_are_the_float32_quotients():
    """spin_damping / settling_time in float32, as the reference's constructors compute them: a settling time whose reciprocal is inexact"""
    rng = np.random.default_rng(43)
    dyn = fr.random_dynamic(rng, 1)
    gen = [forces.alignment_fixed(0, X3, [0.0, 1.0, 0.0], 0.3, 1.1, 1.1)]
    assert_same_bytes(forces.apply_host(gen, dyn), fr.apply(gen, dyn), "alignment")
    assert f32(1.1) / f32(0.3) != f32(1.1) * (f32(1) / f32(0.3))


def test_record_layout_matches_the_c_compiler(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "impact_voxel_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %zu\\n", sizeof(ivx_force_generator), offsetof(ivx_force_generator, kind), offsetof(ivx_force_generator, body), '
                   'offsetof(ivx_force_generator, body_b), offsetof(ivx_force_generator, p));\n'
                   '    printf("%u %u %u %u %u %u\\n", IVX_FG_CONSTANT_ACCELERATION, IVX_FG_LOCAL_FORCE, IVX_FG_SPRING_DYNAMIC_DYNAMIC, IVX_FG_SPRING_DYNAMIC_KINEMATIC, '
                   'IVX_FG_ALIGNMENT_FIXED, IVX_FG_ALIGNMENT_GRAVITY);\n'
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.run(["gcc", "-I", inc, str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    dt = capi.FORCE_GENERATOR_DTYPE
    assert [int(x) for x in lines[0].split()] == [dt.itemsize, dt.fields["kind"][1], dt.fields["body"][1], dt.fields["body_b"][1], dt.fields["p"][1]] == [64, 0, 4, 8, 12]
    assert [int(x) for x in lines[1].split()] == [capi.FG_CONSTANT_ACCELERATION, capi.FG_LOCAL_FORCE, capi.FG_SPRING_DYNAMIC_DYNAMIC, capi.FG_SPRING_DYNAMIC_KINEMATIC,
                                                  capi.FG_ALIGNMENT_FIXED, capi.FG_ALIGNMENT_GRAVITY]
    assert capi.extra_struct_sizes()["ivx_force_generator"] == (dt, 64)
    for name in ("ivx_world_set_force_generators", "ivx_world_set_dynamic_gravity", "ivx_world_apply_forces", "ivx_world_gravity_loads", "ivx_fg_apply_host"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(capi.lib(), name)


CPP_PROGRAM = r"""
#include <cstdio>
#include "impact_voxel.hpp"
using namespace impact_voxel;
static void dump(const ivx_force_generator& g) {
    const unsigned char* b = reinterpret_cast<const unsigned char*>(&g);
    for (size_t i = 0; i < sizeof(g); ++i) std::printf("%02x", b[i]);
    std::printf("\n");
}
int main() {
    dump(ConstantAcceleration{{0.5f, -9.81f, 0.25f}}.record(3));
    dump(ConstantAcceleration::earth().record(1));
    dump(LocalForce{{1.0f, 2.0f, 3.0f}, {0.1f, 0.2f, 0.3f}}.record(4));
    dump(DynamicDynamicSpringForceProperties{{0.1f, 0.2f, 0.3f}, {-0.1f, -0.2f, -0.3f}, Spring::standard(5.0f, 0.5f, 1.5f)}.record(2, 7));
    dump(DynamicKinematicSpringForceProperties{{0.1f, 0.2f, 0.3f}, {-0.1f, -0.2f, -0.3f}, Spring::elastic_band(5.0f, 0.5f, 2.5f)}.record(2, 1));
    dump(DynamicDynamicSpringForceProperties{{0.0f, 0.0f, 0.0f}, {1.0f, 0.0f, 0.0f}, Spring{3.0f, 0.25f, 1.0f, 0.5f}}.record(0, 1));
    dump(FixedDirectionAlignmentTorque{{0.0f, 0.0f, 1.0f}, {0.0f, 1.0f, 0.0f}, 0.5f, 0.3f, 0.2f}.record(6));
    dump(GravityAlignmentTorque{{1.0f, 0.0f, 0.0f}, 0.7f, 0.1f, 0.4f}.record(5));
    std::printf("%g\n", (double)DynamicGravityConfig{}.gravitational_constant);
    return 0;
}
"""


def test_cpp_setup_structs_make_the_records_of_the_python_constructors(tmp_path):
    src = tmp_path / "records.cpp"
    src.write_text(CPP_PROGRAM)
    exe = tmp_path / "records"
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", inc, str(src), "-o", str(exe)], check=True)  # (header-only: nothing of the library is used)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    want = [forces.constant_acceleration(3, [0.5, -9.81, 0.25]), forces.constant_acceleration(1, [0.0, -9.81, 0.0]), forces.local_force(4, [1, 2, 3], [0.1, 0.2, 0.3]),
            forces.spring_dynamic_dynamic(2, [0.1, 0.2, 0.3], 7, [-0.1, -0.2, -0.3], forces.standard_spring(5.0, 0.5, 1.5)),
            forces.spring_dynamic_kinematic(2, [0.1, 0.2, 0.3], 1, [-0.1, -0.2, -0.3], forces.elastic_band(5.0, 0.5, 2.5)),
            forces.spring_dynamic_dynamic(0, [0, 0, 0], 1, [1, 0, 0], forces.spring(3.0, 0.25, 1.0, 0.5)),
            forces.alignment_fixed(6, [0, 0, 1], [0, 1, 0], 0.5, 0.3, 0.2), forces.alignment_gravity(5, [1, 0, 0], 0.7, 0.1, 0.4)]
    assert len(lines) == len(want) + 1
    for i, w in enumerate(want):
        assert lines[i] == w.tobytes().hex(), (i, lines[i], w.tobytes().hex())
    assert float(lines[-1]) == 1.0
