"""Frame instances without a GPU: the library's host form (`ivx_fi_views_host`, the functions the kernels run) against the float32 restatement of
instances_ref.py byte for byte and against the transliterated reference loops, every refusal of the records, and_view chains, NaN and signed-zero
bounds, empty kept sets, hand cases whose answers follow from the reference's text, the float32 composition against float64, the record
layouts through gcc and the C++ forwards of include/impact_voxel.hpp."""
import os
import subprocess

import numpy as np
import pytest

import instances_ref as ir
from impact_amd import bvol, capi, instances

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_QUERIES = 9
NAMES = ("pairs", "offsets", "objects", "transforms", "kept", "results")

# the largest componentwise differences of the float32 composition against the float64 one over the 400 seeded cases below, as measured
# (translation relative to |a.s| |b.t| + |a.t|, rotation and scaling relative to 1), and the gate: four times each
MEASURED_COMPOSITION_ERROR = {"translation": 1.51e-7, "rotation": 9.51e-8, "scaling": 5.66e-8}
ALLOW = 4.0


def assert_outputs_equal(got, want, what=""):
    """got: instances.FrameInstanceOutputs; want: the tuple of instances_ref.views_f32"""
    for name, w, g in zip(NAMES, want, (got.pairs, got.offsets, got.objects, got.transforms, got.kept, got.results)):
        if g is None:
            continue
        w = np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0] if g.ndim else [0]
            raise AssertionError(f"{what}: {name} differs in {len(bad)} rows, first {bad[0]}: {g[bad[0]]} != {w[bad[0]]}")


@pytest.mark.parametrize("n_views", [0, 1, 11, 64])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 300])
def test_host_form_equals_the_float32_restatement(n, n_views):
    """the seeded scene and seeded views (every flag combination, excluded entities, REACH / BOX in all four combinations), two calls: the second
    takes and_view from the first. Every output byte of both equals the restatement's."""
    world, inst = ir.scene(n)
    masks, _ = ir.scene_masks(n, N_QUERIES)
    first = ir.seeded_views(n, min(n_views, 5), N_QUERIES, 0, seed=1)
    a = instances.views_host(world, inst, masks, first)
    assert_outputs_equal(a, ir.views_f32(world, inst, masks, first), f"n {n} first call")
    second = ir.seeded_views(n, n_views, N_QUERIES, len(first), seed=2)
    b = instances.views_host(world, inst, masks, second, a.kept)
    assert_outputs_equal(b, ir.views_f32(world, inst, masks, second, a.kept), f"n {n} x {n_views} views")
    if n >= 63 and n_views >= 11:  # the case can show something: kept and skipped pairs, and_view at work, all four flag combinations with members
        assert 0 < int(b.offsets[-1]) < n * n_views
        assert (second["and_view"] != capi.FI_NONE).any() and len(set(second["flags"].tolist())) == 4
        assert all((b.results["count"][second["flags"] == f] > 0).any() for f in range(4))


@pytest.mark.parametrize("n,n_views", [(1, 1), (65, 11), (300, 7)])
def test_batch_form_equals_the_reference_loops(n, n_views):
    """the transliteration of light.rs's loops (one hit at a time, ascending index, scalar float32) gives the lists, transforms and reductions of
    the batch restatement, which the library equals above"""
    world, inst = ir.scene(n)
    masks, _ = ir.scene_masks(n, N_QUERIES)
    first = ir.seeded_views(n, 3, N_QUERIES, 0, seed=1)
    prev = ir.views_f32(world, inst, masks, first)[4]
    views = ir.seeded_views(n, n_views, N_QUERIES, 3, seed=2)
    pairs, offsets, objects, transforms, kept, results = ir.views_f32(world, inst, masks, views, prev)
    for v, (objs, sims, r) in enumerate(ir.reference_frame(world, inst, masks, views, prev)):
        lo, hi = int(offsets[v]), int(offsets[v + 1])
        assert objects[lo:hi].tolist() == objs, v
        assert transforms[lo:hi].tobytes() == b"".join(s.tobytes() for s in sims), v
        assert results[v].tobytes() == r.tobytes(), (v, results[v], r)
        assert pairs["instance_idx"][v, objs].tolist() == [int(views["instance_base"][v]) + k for k in range(len(objs))]


def raw_views_host(world, inst, masks, n_queries, views, prev=None, n_prev=0, n=None, n_views=None):
    w, i, v = np.ascontiguousarray(world), np.ascontiguousarray(inst), np.ascontiguousarray(views)
    m = np.ascontiguousarray(masks, dtype=np.uint64)
    n = len(w) if n is None else n
    n_views = len(v) if n_views is None else n_views
    return capi.lib().ivx_fi_views_host(capi.ptr(w), n, capi.ptr(i), capi.ptr(m), n_queries, capi.ptr(v), n_views, None if prev is None else capi.ptr(prev), n_prev, None, None,
                                        None, None, 0, None, None)


def test_every_refusal_of_the_records():
    world, inst = ir.scene(65)
    masks, _ = ir.scene_masks(65, N_QUERIES)
    views = ir.seeded_views(65, 3, N_QUERIES, 0, seed=1)
    assert raw_views_host(world, inst, masks, N_QUERIES, views) == capi.IVX_OK
    lib = capi.lib()
    # instances: a scaling that is not positive (NaN included), unknown flag bits, too many
    for field, value in (("scaling", 0.0), ("scaling", -1.0), ("scaling", np.nan), ("flags", 32), ("flags", 0x80000000)):
        bad = inst.copy()
        if field == "scaling":
            bad["model_to_world"]["scaling"][40] = value
        else:
            bad["flags"][40] = value
        assert raw_views_host(world, bad, masks, N_QUERIES, views) == capi.IVX_ERR_INVALID, (field, value)
        assert lib.ivx_fi_set_instances(None, capi.ptr(bad), len(bad)) == capi.IVX_ERR_INVALID  # (no context: refused before anything else)
    assert raw_views_host(world, inst, masks, N_QUERIES, views, n=capi.BV_MAX_OBJECTS + 1) == capi.IVX_ERR_CAPACITY
    # views: more than 64, a scaling that is not positive, a query or an and_view out of range, unknown flags
    many = np.repeat(views[:1], 65)
    assert raw_views_host(world, inst, masks, N_QUERIES, many) == capi.IVX_ERR_INVALID
    assert raw_views_host(world, inst, masks, N_QUERIES, many[:64]) == capi.IVX_OK
    prev = instances.views_host(world, inst, masks, views).kept
    for field, value in (("scaling", 0.0), ("scaling", -2.0), ("scaling", np.nan), ("query", N_QUERIES), ("and_view", 3), ("and_view", capi.FI_NONE - 1), ("flags", 4),
                         ("reject_flags", 32)):
        bad = views.copy()
        if field == "scaling":
            bad["world_to_view"]["scaling"][1] = value
        else:
            bad[field][1] = value
        assert raw_views_host(world, inst, masks, N_QUERIES, bad, prev, 3) == capi.IVX_ERR_INVALID, (field, value)
    ok = views.copy()
    ok["and_view"][1], ok["query"][1] = 2, N_QUERIES - 1
    assert raw_views_host(world, inst, masks, N_QUERIES, ok, prev, 3) == capi.IVX_OK
    assert raw_views_host(world, inst, masks, N_QUERIES, ok) == capi.IVX_ERR_INVALID  # (no previous call: and_view 2 names nothing)
    # the lists do not fit: nothing is written
    objects = np.full(4, 77, dtype=np.uint32)
    offsets = np.full(4, 77, dtype=np.uint32)
    rc = lib.ivx_fi_views_host(capi.ptr(world), 65, capi.ptr(inst), capi.ptr(masks), N_QUERIES, capi.ptr(views), 3, None, 0, None, capi.ptr(offsets), capi.ptr(objects), None, 4,
                               None, None)
    assert rc == capi.IVX_ERR_CAPACITY and (objects == 77).all() and (offsets == 77).all()
    # the device entry points without a context
    assert lib.ivx_fi_views(None, capi.ptr(views), 3, None) == capi.IVX_ERR_INVALID
    assert lib.ivx_fi_download(None, None, 0, None, 0, None, None, 0, None, 0, None) == capi.IVX_ERR_INVALID
    assert not lib.ivx_fi_device_ptr(None, capi.FI_PTR_PAIRS)


def one_view(query=0, **kw):
    return np.array([instances.view(bvol.similarities(1)[0], query, **kw)])


def all_hit(n, rows=1):
    return np.full((rows, (n + 63) // 64), np.uint64(0xFFFFFFFFFFFFFFFF))


def test_and_view_chains_over_two_calls():
    """call 2 keeps only what its and_view of call 1 kept; call 3 sees call 2's sets, not call 1's"""
    world, inst = ir.scene(130)
    inst = inst.copy()
    inst["flags"] = 0
    masks = all_hit(130)
    keep1 = np.zeros(130, dtype=bool)
    keep1[[0, 5, 63, 64, 65, 129]] = True
    m1, _ = ir.br.masks_of(np.stack([keep1, ~keep1]))
    a = instances.views_host(world, inst, m1, np.concatenate([one_view(0), one_view(1)]))
    assert a.objects[a.offsets[0]:a.offsets[1]].tolist() == [0, 5, 63, 64, 65, 129] and int(a.results["count"][1]) == 124
    b = instances.views_host(world, inst, masks, np.concatenate([one_view(0, and_view=0), one_view(0, and_view=1), one_view(0)]), a.kept)
    assert b.kept[0].tobytes() == a.kept[0].tobytes() and b.kept[1].tobytes() == a.kept[1].tobytes() and int(b.results["count"][2]) == 130
    c = instances.views_host(world, inst, masks, one_view(0, and_view=2), b.kept)  # (view 2 of call 2 kept everything: call 1's sets are gone)
    assert int(c.results["count"][0]) == 130
    assert (c.pairs["flags"] == 0).all() and c.pairs["instance_idx"][0].tolist() == list(range(130))


def test_nan_bounds_signed_zeros_and_empty_sets():
    inst = instances.instances(bvol.similarities(4))
    # an object with a NaN bound is never kept, whatever the mask says
    world = bvol.boxes([(0, 0, 0), (np.nan, 0, 0), (2, 2, 2), (3, 3, 3)], [(1, 1, 1), (1, 1, 1), (3, 3, np.nan), (4, 4, 4)])
    out = instances.views_host(world, inst, all_hit(4), one_view(flags=capi.FI_VIEW_BOX | capi.FI_VIEW_REACH, squared_reach=1e9))
    assert out.objects.tolist() == [0, 3] and out.pairs["flags"][0].tolist() == [0, 1, 1, 0]
    assert out.results["world_box"]["lower"][0].tolist() == [0, 0, 0] and out.results["world_box"]["upper"][0].tolist() == [4, 4, 4]
    # +-0 bounds: the merge takes -0.0 as the smaller and +0.0 as the larger, in either order of the objects
    for order in ([0, 1], [1, 0]):
        lower, upper = np.array([(0.0, -0.0, 1.0), (-0.0, 0.0, 1.0)], dtype=np.float32)[order], np.array([(-0.0, 0.0, 2.0), (0.0, -0.0, 2.0)], dtype=np.float32)[order]
        out = instances.views_host(bvol.boxes(lower, upper), inst[:2], all_hit(2), one_view())
        r = out.results[0]
        assert int(r["count"]) == 2
        assert np.signbit(r["world_box"]["lower"][:2]).all() and not np.signbit(r["world_box"]["upper"][:2]).any(), r
    # a view that keeps nothing (its mask row is empty; every instance rejected; everything beyond reach): the empty values, every pair a defined skip
    world = bvol.boxes([(0, 0, 0)] * 4, [(1, 1, 1)] * 4)
    hidden = inst.copy()
    hidden["flags"] = capi.FI_HIDDEN
    cases = [(inst, np.zeros((1, 1), dtype=np.uint64), one_view(flags=3, squared_reach=100.0)), (hidden, all_hit(4), one_view(reject_flags=capi.FI_HIDDEN, flags=3, squared_reach=100.0)),
             (inst, all_hit(4), one_view(flags=3, point=(10.0, 0.0, 0.0), squared_reach=80.0))]
    for records, masks, view in cases:
        pairs = np.frombuffer(b"\xff" * (4 * capi.CULL_PAIR_DTYPE.itemsize), dtype=capi.CULL_PAIR_DTYPE).copy()
        results = np.frombuffer(b"\xff" * capi.FI_VIEW_RESULT_DTYPE.itemsize, dtype=capi.FI_VIEW_RESULT_DTYPE).copy()
        kept, offsets = np.full(1, 0xFFFF, dtype=np.uint64), np.full(2, 9, dtype=np.uint32)
        rc = capi.lib().ivx_fi_views_host(capi.ptr(world), 4, capi.ptr(records), capi.ptr(masks), 1, capi.ptr(view), 1, None, 0, capi.ptr(pairs), capi.ptr(offsets), None, None, 0,
                                          capi.ptr(kept), capi.ptr(results))
        assert rc == capi.IVX_OK
        assert pairs.tobytes() == ir.identity_skip_pairs(4).tobytes() and results[0].tobytes() == ir.empty_result().tobytes()
        assert int(kept[0]) == 0 and offsets.tolist() == [0, 0]
    # a reduction that was not asked for is stored with the empty values, next to one that was
    out = instances.views_host(world, inst, all_hit(4), one_view())
    r, e = out.results[0], ir.empty_result()
    assert int(r["count"]) == 4 and r["view_box"].tobytes() == e["view_box"].tobytes()
    assert r["min_squared_distance"] == np.inf and r["max_squared_distance"] == -np.inf and r["world_box"]["upper"].tolist() == [1, 1, 1]


def test_hand_cases_of_the_distances():
    inst = instances.instances(bvol.similarities(1))
    reach = dict(flags=capi.FI_VIEW_REACH)

    def result(lower, upper, point, squared_reach):
        return instances.views_host(bvol.boxes([lower], [upper]), inst, all_hit(1), one_view(point=point, squared_reach=squared_reach, **reach)).results[0]

    # a light on a face of the box: the closest interior point is the light's position, d_close = 0; the farthest corner is the opposite one
    r = result((0, 0, 0), (2, 4, 6), (2.0, 1.0, 1.0), 0.0)
    assert int(r["count"]) == 1 and float(r["min_squared_distance"]) == 0.0 and float(r["max_squared_distance"]) == 4.0 + 9.0 + 25.0
    # the point exactly at the box centre takes the UPPER corners (`point > centre` is false). lower = 1 + 2^-23, upper = 2: lower + upper rounds
    # to 3, the centre is 1.5, and |1.5 - upper| = 0.5 exactly while |1.5 - lower| is one ulp less: 3 x 0.25 only from the upper corner
    lo = np.nextafter(np.float32(1.0), np.float32(2.0))
    r = result((lo, lo, lo), (2, 2, 2), (1.5, 1.5, 1.5), 1.0)
    assert float(r["max_squared_distance"]) == 0.75 and float(r["min_squared_distance"]) == 0.0
    below = np.nextafter(np.float32(1.5), np.float32(2.0))  # one ulp past the centre: the lower corners
    r = result((lo, lo, lo), (2, 2, 2), (below, below, below), 1.0)
    d = np.float32(below) - lo
    assert float(r["max_squared_distance"]) == float((d * d + d * d) + d * d) < 0.7500003
    # a reach exactly equal to d_close is kept (the test is a strict >); one ulp less is not
    d_close = np.float32(9.0) + np.float32(16.0)  # the box corner (3, 4, z) from a point at the origin level with the box in z
    assert int(result((3, 4, -1), (5, 6, 1), (0.0, 0.0, 0.0), d_close)["count"]) == 1
    assert int(result((3, 4, -1), (5, 6, 1), (0.0, 0.0, 0.0), np.nextafter(d_close, np.float32(0.0)))["count"]) == 0
    r = result((3, 4, -1), (5, 6, 1), (0.0, 0.0, 0.0), d_close)
    assert float(r["min_squared_distance"]) == 25.0 and float(r["max_squared_distance"]) == 25.0 + 36.0 + 1.0


def test_float32_composition_against_float64():
    """400 seeded cases: world_to_view with rotations uniform on the sphere, translations within 10 of the origin, scalings in [0.25, 4] (every other
    one an isometry), model_to_world of the seeded scene (translations within 20). Measured: the largest componentwise difference of the
    translation is 1.51e-7 of |a.s| |b.t| + |a.t|, of the rotation 9.51e-8, of the scaling 5.66e-8 (relative). The gate is four times each: it
    catches a wrong formula, not rounding. The library's composition (through `ivx_fi_views_host`) is the one under test; it equals the float32
    restatement byte for byte."""
    _, inst = ir.scene(300)
    rng = np.random.default_rng(5)
    worst = {"translation": 0.0, "rotation": 0.0, "scaling": 0.0}
    views = np.zeros(400, dtype=capi.FI_VIEW_DTYPE)
    for i in range(400):
        views[i] = instances.view(ir.random_similarity(rng, 1.0 if i % 2 else None), 0)
    world = bvol.boxes(np.zeros((300, 3)), np.ones((300, 3)))
    got = np.concatenate([instances.views_host(world, inst, all_hit(300), views[k:k + 50]).pairs for k in range(0, 400, 50)])
    for i in range(400):
        a, o = views["world_to_view"][i], i % 300
        b = inst["model_to_world"][o]
        assert got[i, o].tobytes()[:32] == ir.compose_f32(a, inst["model_to_world"][o:o + 1])[0].tobytes()
        t, q, s = ir.compose_f64(a, b)
        scale = abs(float(a["scaling"])) * np.linalg.norm(b["translation"].astype(np.float64)) + np.linalg.norm(a["translation"].astype(np.float64))
        worst["translation"] = max(worst["translation"], np.abs(got["translation"][i, o].astype(np.float64) - t).max() / scale)
        worst["rotation"] = max(worst["rotation"], np.abs(got["rotation"][i, o].astype(np.float64) - q).max())
        worst["scaling"] = max(worst["scaling"], abs(float(got["scaling"][i, o]) - s) / s)
    print("largest composition differences", worst)
    for name, measured in MEASURED_COMPOSITION_ERROR.items():
        assert worst[name] <= ALLOW * measured, (name, worst[name], measured)


def test_record_layouts_match_the_c_compiler(tmp_path):
    records = {"ivx_fi_instance": (capi.FI_INSTANCE_DTYPE, 48), "ivx_fi_view": (capi.FI_VIEW_DTYPE, 72), "ivx_fi_view_result": (capi.FI_VIEW_RESULT_DTYPE, 60)}
    members = {"ivx_fi_instance": ["model_to_world", "flags", "entity", "reserved"],
               "ivx_fi_view": ["world_to_view", "query", "reject_flags", "exclude_entity", "and_view", "instance_base", "flags", "point", "squared_reach"],
               "ivx_fi_view_result": ["count", "world_box", "view_box", "min_squared_distance", "max_squared_distance"]}
    constants = {"IVX_FI_ABSENT": capi.FI_ABSENT, "IVX_FI_HIDDEN": capi.FI_HIDDEN, "IVX_FI_CASTS_NO_SHADOWS": capi.FI_CASTS_NO_SHADOWS,
                 "IVX_FI_SHADOWS_OFF_BY_DISTANCE": capi.FI_SHADOWS_OFF_BY_DISTANCE, "IVX_FI_NO_SHADOW_FEATURES": capi.FI_NO_SHADOW_FEATURES, "IVX_FI_ALL_FLAGS": capi.FI_ALL_FLAGS,
                 "IVX_FI_NONE": capi.FI_NONE, "IVX_FI_VIEW_REACH": capi.FI_VIEW_REACH, "IVX_FI_VIEW_BOX": capi.FI_VIEW_BOX, "IVX_FI_MAX_VIEWS": capi.FI_MAX_VIEWS,
                 "IVX_FI_PTR_INSTANCES": capi.FI_PTR_INSTANCES, "IVX_FI_PTR_PAIRS": capi.FI_PTR_PAIRS, "IVX_FI_PTR_OFFSETS": capi.FI_PTR_OFFSETS, "IVX_FI_PTR_OBJECTS": capi.FI_PTR_OBJECTS,
                 "IVX_FI_PTR_TRANSFORMS": capi.FI_PTR_TRANSFORMS, "IVX_FI_PTR_KEPT_MASKS": capi.FI_PTR_KEPT_MASKS, "IVX_FI_PTR_RESULTS": capi.FI_PTR_RESULTS}
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "impact_voxel_hip.h"\nint main(void) {\n' +
                   "".join(f'    printf("{n} %zu\\n", sizeof({n}));\n' for n in records) +
                   "".join(f'    printf("{n}.{m} %zu\\n", offsetof({n}, {m}));\n' for n, ms in members.items() for m in ms) +
                   "".join(f'    printf("{c} %llu\\n", (unsigned long long)({c}));\n' for c in constants) + "    return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for n, (dt, documented) in records.items():
        assert int(got[n]) == dt.itemsize == documented, f"{n}: the header's struct is {got[n]} bytes, its numpy mirror {dt.itemsize}, documented {documented}"
        assert documented % 4 == 0 and capi.extra_struct_sizes()[n] == (dt, documented)
        for m in members[n]:
            assert int(got[f"{n}.{m}"]) == dt.fields[m][1], (n, m, got[f"{n}.{m}"])
    assert capi.FI_INSTANCE_DTYPE.itemsize % 16 == 0
    for c, value in constants.items():
        assert int(got[c]) == value, c
    for name in ("ivx_fi_set_instances", "ivx_fi_views", "ivx_fi_download", "ivx_fi_device_ptr", "ivx_fi_views_host", "ivx_cull_many_resident"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(capi.lib(), name)


CPP_PROGRAM = r"""
#include <cstdio>
#include "impact_voxel.hpp"
using namespace impact_voxel;
int main() {
    // two unit boxes, one hit by the only query; the view halves and shifts: the kept pair carries scaling 0.5 x 2 and translation 0.5 x 4 + 1
    std::vector<ivx_aabb> world = {{{0, 0, 0}, {1, 1, 1}}, {{2, 2, 2}, {3, 3, 3}}};
    std::vector<ivx_fi_instance> inst(2);
    for (auto& i : inst) i.model_to_world = {{0, 0, 0, 1}, {4, 0, 0}, 2.0f}, i.flags = 0, i.entity = 7;
    ivx_fi_view v{};
    v.world_to_view = {{0, 0, 0, 1}, {1, 0, 0}, 0.5f};
    v.query = 0, v.exclude_entity = IVX_FI_NONE, v.and_view = IVX_FI_NONE, v.instance_base = 40, v.flags = IVX_FI_VIEW_BOX;
    FrameInstances::Outputs out;
    const std::vector<ivx_fi_view_result> r = FrameInstances::views_host(world, inst, {2ull}, 1, {v}, {}, 0, &out);
    std::printf("%u %g %g %u %u %u %zu %g %g %llu\n", r[0].count, (double)r[0].view_box.lower[0], (double)r[0].view_box.upper[0], out.pairs[0].flags, out.pairs[1].flags,
                out.pairs[1].instance_idx, out.objects.size(), (double)out.transforms[0].scaling, (double)out.transforms[0].translation[0],
                (unsigned long long)out.kept_masks[0]);
    // what needs a context compiles and links
    if (r.empty()) {
        Context* c = nullptr;
        FrameInstances fi(*c);
        fi.set_instances(inst), fi.enqueue({v}), (void)fi.views({v}), (void)fi.download(1, 2), (void)fi.device_ptr(IVX_FI_PTR_PAIRS), (void)fi.enqueue_cull({}, {}, {}, IVX_CULL_ZEROED);
    }
    return 0;
}
"""


def test_cpp_forwards_compile_link_and_run(tmp_path):
    src = tmp_path / "forwards.cpp"
    src.write_text(CPP_PROGRAM)
    exe = tmp_path / "forwards"
    lib_dir = os.path.dirname(capi.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", lib_dir, "-limpact_voxel_hip",
                    f"-Wl,-rpath,{lib_dir}"], check=True)
    line = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    # (the hit box is [2, 3]^3: centre 2.5 and half extent 0.5 through scaling 0.5 and translation 1 give [2, 2.5] along x)
    assert line == ["1", "2", "2.5", "1", "0", "40", "1", "1", "3", "2"], line
