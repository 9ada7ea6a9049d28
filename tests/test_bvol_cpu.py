"""Bounding volumes without a GPU: the record layouts through gcc, the library's host derivation (`ivx_bv_world_aabb`) against the float64
restatement in bvol_ref.py and on fixed cases, the corners `ivx_bv_frustum_query` picks, the refusals and the empty calls that need no context,
and the restatement's own decisions on hand-made cases (the GPU tests' expectations rest on them)."""
import ctypes as C
import os
import subprocess

import numpy as np

import bvol_ref as br
import cull_ref as cr
from impact_amd import bvol, capi, cull

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the largest corner error measured over the 400 seeded cases below (seed 21), as a fraction of S, and the tolerance: four times it
MEASURED_DERIVATION_ERROR = 2.69e-7
DERIVATION_TOLERANCE = 4 * MEASURED_DERIVATION_ERROR


def test_record_sizes_match_the_c_compiler(tmp_path):
    records = {"ivx_aabb": (capi.AABB_DTYPE, 24), "ivx_similarity": (capi.SIMILARITY_DTYPE, 32), "ivx_bv_query": (capi.BV_QUERY_DTYPE, 128)}
    offsets = {"u.box.upper": "upper", "u.sphere.radius": "radius", "u.frustum.planes": "planes", "u.frustum.corners": "corners", "u.oriented_box.axes": "axes",
               "u.oriented_box.center": "box_center", "u.oriented_box.half_extents": "half_extents", "u.words": "words"}
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "impact_voxel_hip.h"\nint main(void) {\n' +
                   "".join(f'    printf("{n} %zu\\n", sizeof({n}));\n' for n in records) +
                   "".join(f'    printf("{m} %zu\\n", offsetof(ivx_bv_query, {m}));\n' for m in offsets) +
                   '    printf("scaling %zu\\n", offsetof(ivx_similarity, scaling));\n    printf("pair_scaling %zu\\n", offsetof(ivx_cull_pair, scaling));\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for n, (dt, documented) in records.items():
        assert int(got[n]) == dt.itemsize == documented, f"{n}: the header's struct is {got[n]} bytes, its numpy mirror {dt.itemsize}, documented {documented}"
    for member, field in offsets.items():
        assert int(got[member]) == capi.BV_QUERY_DTYPE.fields[field][1], (member, got[member])
    # ivx_similarity is the leading part of ivx_cull_pair
    assert int(got["scaling"]) == int(got["pair_scaling"]) == capi.SIMILARITY_DTYPE.fields["scaling"][1] == capi.CULL_PAIR_DTYPE.fields["scaling"][1]
    for name in ("rotation", "translation"):
        assert capi.SIMILARITY_DTYPE.fields[name][1] == capi.CULL_PAIR_DTYPE.fields[name][1]
    for name, dt in capi.extra_struct_sizes().items():
        assert dt[0].itemsize == dt[1], name


def test_host_derivation_against_the_float64_restatement():
    """400 seeded cases (rotations uniform on the sphere, scalings 0.05 - 20, translations up to 10^3, boxes up to 10^2 across). The error of every
    corner is a fraction of S = max(1, |translation|, scaling x largest |corner|). Measured: the largest is 2.69e-7 (seeds 22 - 25 of the same recipe:
    2.6e-7 .. 3.2e-7); the tolerance is four times the measured figure, 1.08e-6 — a sum of three products per component, well inside the project's
    1e-5 for rigid-body state."""
    boxes, sims = br.seeded_derivation_cases(400, 21)
    worst = 0.0
    for model, sim in zip(boxes, sims):
        worst = max(worst, br.derivation_error(bvol.world_aabb(model, sim), model, sim))
    print(f"largest derivation error {worst:.3g} S (tolerance {DERIVATION_TOLERANCE:.3g})")
    assert worst <= DERIVATION_TOLERANCE
    assert DERIVATION_TOLERANCE <= 1e-5


def test_host_derivation_fixed_cases():
    identity = bvol.similarities(1)[0]
    # the identity returns the box's own bytes (lower + upper and upper - lower exact in f32, as the header says)
    for lower, upper in (((0.125, -2.5, 3.0), (1.5, 4.25, 7.75)), ((-8.0, -8.0, -8.0), (8.0, 8.0, 8.0)), ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))):
        box = bvol.boxes([lower], [upper])[0]
        assert bvol.world_aabb(box, identity).tobytes() == box.tobytes()
    # a quarter turn about z (w = z = the float32 nearest sqrt(1/2): unit only to rounding) swaps the x and y extents exactly, for any box
    turn = identity.copy()
    turn["rotation"] = (0.0, 0.0, np.float32(np.sqrt(0.5)), np.float32(np.sqrt(0.5)))
    rng = np.random.default_rng(7)
    for _ in range(20):
        centre, half = rng.uniform(-30, 30, 3), rng.uniform(0.01, 20, 3)
        box = bvol.boxes([centre - half], [centre + half])[0]
        same, turned = bvol.world_aabb(box, identity), bvol.world_aabb(box, turn)
        assert turned["lower"][0] == -same["upper"][1] and turned["upper"][0] == -same["lower"][1]  # x' = -y
        assert turned["lower"][1] == same["lower"][0] and turned["upper"][1] == same["upper"][0]    # y' = x
        assert turned["lower"][2] == same["lower"][2] and turned["upper"][2] == same["upper"][2]
        assert turned["upper"][0] - turned["lower"][0] == same["upper"][1] - same["lower"][1]
        assert turned["upper"][1] - turned["lower"][1] == same["upper"][0] - same["lower"][0]
    # scaling and translation on a box with exact arithmetic
    sim = identity.copy()
    sim["scaling"], sim["translation"] = 2.0, (10.0, -20.0, 0.5)
    got = bvol.world_aabb(bvol.boxes([(-1.0, 0.0, 1.0)], [(1.0, 4.0, 2.0)])[0], sim)
    assert got["lower"].tolist() == [8.0, -20.0, 2.5] and got["upper"].tolist() == [12.0, -12.0, 4.5]
    # a scaling that is not positive is refused
    lib, out = capi.lib(), np.zeros(1, dtype=capi.AABB_DTYPE)
    box = bvol.boxes([(0, 0, 0)], [(1, 1, 1)])
    for scaling in (0.0, -0.0, -2.0, float("nan")):
        s = bvol.similarities(1)
        s["scaling"] = scaling
        assert lib.ivx_bv_world_aabb(capi.ptr(box), capi.ptr(s), capi.ptr(out)) == capi.IVX_ERR_INVALID, scaling
    assert lib.ivx_bv_world_aabb(None, capi.ptr(bvol.similarities(1)), capi.ptr(out)) == capi.IVX_ERR_INVALID
    assert lib.ivx_bv_world_aabb(capi.ptr(box), None, capi.ptr(out)) == capi.IVX_ERR_INVALID
    assert lib.ivx_bv_world_aabb(capi.ptr(box), capi.ptr(bvol.similarities(1)), None) == capi.IVX_ERR_INVALID


def test_frustum_query_corners():
    """`corners` follows the convention of ivx_culling_frustum.most_inside_corners (bit 2 / 1 / 0 = upper x / y / z) and names the box corner with
    the largest signed distance — for the planes of the reference's own case (frustum.rs:796-815: aspect 1, 90 degrees, near 1, far 10), for
    seeded normals, and for components of -0.0, which choose the lower corner"""
    for i in range(8):
        assert tuple(cr.CORNERS_OFFSETS[i]) == ((i >> 2) & 1, (i >> 1) & 1, i & 1)
    rec = cull.culling_frustum_from_view(cr.perspective_view(90.0, 90.0, 1.0, 10.0), cull.pairs(1, 1)[0, 0], 1.0)
    q = bvol.frustum_query(rec["planes"])
    assert int(q["kind"]) == capi.BV_QUERY_FRUSTUM and q["planes"].tobytes() == rec["planes"].tobytes()
    assert q["corners"].tolist() == rec["most_inside_corners"].tolist()
    rng = np.random.default_rng(3)
    planes = np.zeros((6, 4), dtype=np.float32)
    for _ in range(10):
        n = rng.normal(size=(6, 3))
        planes[:, :3], planes[:, 3] = n / np.linalg.norm(n, axis=1, keepdims=True), rng.uniform(-5, 5, 6)
        q = bvol.frustum_query(planes)
        for p in range(6):
            dist = cr.CORNERS_OFFSETS.astype(np.float64) @ planes[p, :3].astype(np.float64)
            assert np.all(dist <= dist[int(q["corners"][p])]) and int(q["corners"][p]) == br.corner_of(planes[p, :3]) == cr.corner_of(planes[p, :3])
    planes = np.array([[1, 0, 0, 0], [-1, -0.0, 0, 0], [0, 1, 0, 0], [-0.0, -1, -0.0, 0], [0, 0, 1, 0], [-0.0, 0, -1, 0]], dtype=np.float32)
    q = bvol.frustum_query(planes)
    assert q["corners"].tolist() == [7, 1, 7, 0, 7, 2]
    assert not q["words"][30:].any()  # (the words behind `corners` are zero)
    lib = capi.lib()
    assert lib.ivx_bv_frustum_query(None, capi.ptr(np.zeros(1, dtype=capi.BV_QUERY_DTYPE))) == capi.IVX_ERR_INVALID
    assert lib.ivx_bv_frustum_query(capi.ptr(planes), None) == capi.IVX_ERR_INVALID


def test_refusals_and_empty_calls_without_a_context():
    lib = capi.lib()
    box, sim, kinds = bvol.boxes([(0, 0, 0)], [(1, 1, 1)]), bvol.similarities(1), np.zeros(1, dtype=np.uint32)
    found = C.c_size_t(7)
    out = np.zeros((4, 2), dtype=np.uint32)
    # every device call refuses a null context, whatever else it is given
    assert lib.ivx_bv_set(None, capi.ptr(box), capi.ptr(sim), capi.ptr(kinds), 1) == capi.IVX_ERR_INVALID
    assert lib.ivx_bv_set(None, None, None, None, 0) == capi.IVX_ERR_INVALID
    assert lib.ivx_bv_download(None, capi.ptr(box), 1, capi.ptr(box)) == capi.IVX_ERR_INVALID
    assert lib.ivx_bv_pairs(None, 0, capi.ptr(out), 4, C.byref(found)) == capi.IVX_ERR_INVALID and found.value == 0
    assert lib.ivx_bv_queries(None, None, 0, None, None) == capi.IVX_ERR_INVALID
    assert not lib.ivx_bv_device_ptr(None, capi.BV_PTR_WORLD_BOXES)
    assert lib.ivx_grid_model_aabb(None, capi.ptr(box)) == capi.IVX_ERR_INVALID
    # no objects: ivx_bv_set_grids names no context and succeeds
    assert lib.ivx_bv_set_grids(None, 0, None, None) == capi.IVX_OK
    assert bvol.set_grids([]).n == 0
    # ... but objects without a list, a null object, a bad kind or scaling are refused before any context is looked at
    assert lib.ivx_bv_set_grids(None, 3, None, None) == capi.IVX_ERR_INVALID
    handles = np.zeros(1, dtype=np.uint64)  # (a null object)
    assert lib.ivx_bv_set_grids(capi.ptr(handles), 1, None, None) == capi.IVX_ERR_INVALID
    bad_kind = np.array([3], dtype=np.uint32)
    assert lib.ivx_bv_set_grids(capi.ptr(handles), 1, None, capi.ptr(bad_kind)) == capi.IVX_ERR_INVALID
    assert b"kind 3" in lib.ivx_last_error()
    for scaling in (0.0, -1.0, float("nan")):
        s = bvol.similarities(1)
        s["scaling"] = scaling
        assert lib.ivx_bv_set_grids(capi.ptr(handles), 1, capi.ptr(s), None) == capi.IVX_ERR_INVALID
        assert b"scaling" in lib.ivx_last_error()


def test_restatement_decisions_on_hand_made_cases():
    f = np.float32
    one = lambda lo, hi: bvol.boxes([lo], [hi])
    hit = lambda a, b: bool(br.boxes_intersect(a["lower"], a["upper"], b["lower"], b["upper"])[0])
    unit = one((0, 0, 0), (1, 1, 1))
    assert hit(unit, one((1, 0, 0), (2, 1, 1))) and hit(unit, one((1, 1, 1), (2, 2, 2)))  # touching faces and corners intersect
    assert not hit(unit, one((1.0000001, 0, 0), (2, 1, 1)))
    # the sign bit of the difference, not a `<`: (-0.0) - (+0.0) = -0.0 is outside, (+0.0) - (+0.0) is not
    assert not hit(one((-1, 0, 0), (-0.0, 1, 1)), one((0.0, 0, 0), (1, 1, 1)))
    assert hit(one((-1, 0, 0), (0.0, 1, 1)), one((0.0, 0, 0), (1, 1, 1)))
    assert not hit(one((float("nan"), 0, 0), (1, 1, 1)), unit)  # a NaN bound intersects nothing
    p, touching = br.pairs(bvol.boxes([(0, 0, 0), (1, 0, 0), (3, 0, 0), (0.5, 0.5, 0.5)], [(1, 1, 1), (2, 1, 1), (4, 1, 1), (3.5, 0.75, 0.75)]))
    assert p.tolist() == [[0, 1], [0, 3], [1, 3], [2, 3]] and touching.tolist() == [True, False, False, False]
    kinds = np.array([0, 1, 1, 2], dtype=np.uint32)
    assert br.pairs(bvol.boxes([(0, 0, 0)] * 4, [(1, 1, 1)] * 4), kinds, capi.BV_DYNAMIC_PAIRS)[0].tolist() == [[0, 1], [0, 2]]
    # the queries: a face exactly on the boundary is a hit, the next float32 beyond it a miss
    world = one((2, 2, 2), (3, 3, 3))
    beyond = np.nextafter(f(3), f(4))
    assert br.query_hits(world, bvol.box_query((3, 0, 0), (4, 4, 4)))[0] and not br.query_hits(world, bvol.box_query((beyond, 0, 0), (4, 4, 4)))[0]
    assert br.query_hits(world, bvol.sphere_query((3.5, 2.5, 2.5), 0.5))[0] and not br.query_hits(world, bvol.sphere_query((3.5, 2.5, 2.5), np.nextafter(f(0.5), f(0))))[0]
    assert br.query_hits(world, bvol.sphere_query((3.5, 3.5, 2.5), 0.75))[0] and not br.query_hits(world, bvol.sphere_query((3.5, 3.5, 2.5), 0.7))[0]
    far = [[0, 1, 0, -100], [0, -1, 0, -100], [0, 0, 1, -100], [0, 0, -1, -100], [-1, 0, 0, -100]]
    assert br.query_hits(world, bvol.frustum_query([[1, 0, 0, 3]] + far))[0] and not br.query_hits(world, bvol.frustum_query([[1, 0, 0, beyond]] + far))[0]
    assert br.query_hits(world, bvol.oriented_box_query((3.5, 2.5, 2.5), (0, 0, 0, 1), (0.5, 1, 1)))[0]
    assert not br.query_hits(world, bvol.oriented_box_query((np.nextafter(f(3.5), f(4)), 2.5, 2.5), (0, 0, 0, 1), (0.5, 1, 1)))[0]
    masks, counts = br.queries(bvol.boxes([(0, 0, 0)] * 70, [(1, 1, 1)] * 70), bvol.query_array([bvol.box_query((0, 0, 0), (1, 1, 1)), bvol.box_query((5, 5, 5), (6, 6, 6))]))
    assert masks.tolist() == [[2 ** 64 - 1, 63], [0, 0]] and counts.tolist() == [70, 0]
    assert [m.tolist() for m in bvol.mask_indices(masks, 70)] == [list(range(70)), []]


def test_seeded_scene_shows_what_the_pair_tests_need():
    """the figures of the recipe with seed 11: intersecting pairs and pairs with an exactly-zero face difference at every size the GPU tests use from
    63 up — at least n pairs, at most a quarter of all pairs, at least a tenth of them touching"""
    expected = {63: (128, 38), 64: (115, 35), 65: (124, 31), 200: (460, 134), 1025: (3245, 1003)}
    for n in (63, 64, 65, 200, 511, 512, 513, 1023, 1024, 1025):
        p, touching = br.scene_pairs(n, capi.BV_ALL_PAIRS)
        assert n <= len(p) <= n * (n - 1) // 8 and touching.sum() * 10 >= len(p), n
        if n in expected:
            assert (len(p), int(touching.sum())) == expected[n], n
        assert np.all(p[:, 0] < p[:, 1]) and np.all(np.lexsort((p[:, 1], p[:, 0])) == np.arange(len(p)))
        filtered = br.scene_pairs(n, capi.BV_DYNAMIC_PAIRS)[0]
        assert 0 < len(filtered) < len(p)
