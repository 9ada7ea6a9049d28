"""Host-side checks of the primitive collidable calls (impact_amd/csrc/narrow.hip): `ivx_cw_contact` and `ivx_cw_transform` run the very functions
the kernels run, so the arithmetic is checked here without a GPU — byte-equal to the float32 restatement of narrow_ref.py, that restatement against
the oracle's two sphere forms, against the known answers of the reference's own tests, and against its float64 version. No kernels are launched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bvol_ref as br
import narrow_ref as nr
import oracle_lib as ol
from impact_amd import capi, collision

S, P, CAP = nr.SPHERE, nr.PLANE, nr.CAPSULE
COMBINATIONS = [(a, b) for a in (S, P, CAP) for b in (S, P, CAP)]  # every shape combination in both argument orders
N_SEEDED = 2000

# The largest error of the float32 restatement against its float64 version, measured on the seeded cases below (2 000 decided pairs per ordered
# combination, seed 5) and keyed by the members after the swap: max over the hits of (|position - position64|_inf, |depth - depth64|) / scale and of
# |normal - normal64|_inf, scale = max(1, largest |coordinate| of the two members). Near-parallel capsule segments are ill-conditioned in the
# closest-point parameters, and a sphere centre close to a capsule's segment in the normal: that is where the two large figures come from. The tests allow FOUR TIMES these (the GPU and the host run one operation
# order, so nothing else has to be covered).
MEASURED = {(S, S): 1.3e-7, (S, P): 2.5e-7, (CAP, S): 2.9e-4, (CAP, P): 2.4e-7, (CAP, CAP): 1.4e-3}


def bound_of(first, second):
    return np.array([4.0 * MEASURED[(int(a), int(b))] for a, b in zip(first["shape"], second["shape"])])


def scale_of(first, second):
    return np.maximum(1.0, np.maximum(np.abs(first["a"]).max(axis=1), np.abs(second["a"]).max(axis=1))).astype(np.float64)


def library_contacts(a_world, b_world):
    """`ivx_cw_contact` over arrays of pairs -> (verdicts, records: all-zero where the verdict is not CONTACT)"""
    lib = capi.lib()
    a_world, b_world = np.ascontiguousarray(a_world), np.ascontiguousarray(b_world)
    out, verdicts, hit = np.zeros(len(a_world), dtype=capi.CONTACT_DTYPE), np.zeros(len(a_world), dtype=np.int64), C.c_int(0)
    pa, pb, po, hit_ref = a_world.ctypes.data, b_world.ctypes.data, out.ctypes.data, C.byref(hit)
    for i in range(len(a_world)):
        capi.check(lib.ivx_cw_contact(pa + 64 * i, pb + 64 * i, po + 64 * i, hit_ref))
        verdicts[i] = hit.value
    return verdicts, out


@pytest.fixture(scope="module")
def decided_pairs():
    """per ordered combination: N_SEEDED seeded pairs none of which is within the allowed error of the hit / miss decision (asserted here, on the
    reference side) -> {(shape_a, shape_b): (A, B, first, second, margin64)}"""
    out = {}
    for sa, sb in COMBINATIONS:
        a, b = nr.seeded_pairs(sa, sb, N_SEEDED + 300)
        first, second, _ = nr.ordered(a, b)
        if (sa, sb) == (P, P):
            keep = np.arange(N_SEEDED)
            margin = np.zeros(len(a))
        else:
            margin = nr.decision_margin(first, second)
            keep = np.nonzero(np.abs(margin) > bound_of(first, second) * scale_of(first, second))[0][:N_SEEDED]
            assert len(keep) == N_SEEDED, (sa, sb, len(keep))
            hits = (margin[keep] >= 0).mean()
            assert 0.25 <= hits <= 0.85, (sa, sb, hits)  # (both verdicts well represented)
        out[(sa, sb)] = (a[keep], b[keep], first[keep], second[keep], margin[keep])
    return out


def test_contact_is_byte_equal_to_the_restatement_on_seeded_pairs():
    """2 300 seeded pairs per ordered shape combination (the decided ones and the ones close to the decision alike): verdict and record"""
    for sa, sb in COMBINATIONS:
        a, b = nr.seeded_pairs(sa, sb, N_SEEDED + 300)
        want_verdict, want = nr.pair_contacts(a, b)
        got_verdict, got = library_contacts(a, b)
        assert got_verdict.tolist() == want_verdict.tolist(), (sa, sb)
        assert got.tobytes() == want.tobytes(), (sa, sb, int(np.nonzero(got != want)[0][0]))
        assert ((want_verdict == nr.CONTACT).any() and (want_verdict == nr.NO_CONTACT).any()) or (sa, sb) == (P, P)


def test_contact_is_byte_equal_to_the_restatement_on_every_branch():
    cases = nr.hand_made_cases()
    for name, (a, b) in cases.items():
        for x, y in ((a, b), (b, a)):
            want_verdict, want = nr.pair_contacts(x, y)
            got_verdict, got = collision.contact(x, y)
            assert got_verdict == want_verdict[0], name
            assert got is None or got.tobytes() == want[0].tobytes(), (name, got, want[0])

    def verdict(name):
        return int(nr.pair_contacts(*cases[name])[0][0])

    def geometry(name):
        c = nr.pair_contacts(*cases[name])[1][0]
        return c["position"].tolist(), c["normal"].tolist(), float(c["depth"])

    def parameters(name):
        a, b = cases[name]
        return [float(v[0]) for v in nr.closest_parameters(a["a"][None], a["b"][None], b["a"][None], b["b"][None], details=True)]

    # the cases take the branches they are named after
    assert geometry("coincident sphere centres") == ([1.0, 2.0, 3.25], [0.0, 0.0, 1.0], 0.75)
    assert geometry("spheres touching exactly")[2] == 0.0 and verdict("spheres touching exactly") == nr.CONTACT and verdict("spheres apart") == nr.NO_CONTACT
    assert geometry("sphere centre on a capsule's segment") == ([1.0, 0.0, -0.5], [0.0, 0.0, -1.0], 0.75)  # ortho((2, 0, 0)) = (0, 0, 1), negated
    assert geometry("sphere centre on a capsule's segment along y")[1] == [0.0, 0.0, 1.0]  # ortho((0, 2, 0)) = (0, 0, -1), negated
    assert geometry("sphere on a zero-length capsule")[1] == [0.0, 0.0, -1.0]  # ortho(0) falls back to unit z, negated
    # the segments cross a quarter along A; ortho((2, 0, 0)) = (-0, 0, 1): A's vector (0, 2, -2) runs against it and A clears B after 0.25 x 2 more,
    # (0, 2, 2) runs along it and A clears B after 0.75 x 2 more; (2, 0, 0) of the third case is normal to it and adds nothing
    assert parameters("crossing capsules, A against the normal")[:2] == [0.25, 0.5] == parameters("crossing capsules, A along the normal")[:2]
    assert geometry("crossing capsules, A against the normal") == ([0.0, 0.0, 0.25], [0.0, 0.0, 1.0], 0.5 + 0.5)
    assert geometry("crossing capsules, A along the normal") == ([0.0, 0.0, 0.25], [0.0, 0.0, 1.0], 0.5 + 1.5)
    assert geometry("crossing capsules, A normal to the normal")[2] == 0.5
    assert parameters("parallel capsules")[2] == 0.0 and parameters("antiparallel capsules")[2] == 0.0
    assert parameters("capsules, B parameter below 0")[3] < 0 and parameters("capsules, B parameter below 0")[1] == 0.0
    minus_zero = parameters("capsules, B parameter minus zero")[3]
    assert minus_zero == 0.0 and np.signbit(minus_zero) and parameters("capsules, B parameter minus zero")[:2] == [0.0, 0.0]
    assert parameters("capsules, B parameter above 1")[3] > 1 and parameters("capsules, B parameter above 1")[1] == 1.0
    for name in ("capsules touching exactly", "sphere on a plane, touching exactly", "capsule on a plane, touching exactly"):
        assert verdict(name) == nr.CONTACT and geometry(name)[2] == 0.0, name
    for name in ("sphere just clear of a plane", "capsule just clear of a plane", "capsules apart", "plane against plane"):
        assert verdict(name) == nr.NO_CONTACT, name
    assert verdict("voxel object against a sphere") == nr.DEFERRED and verdict("plane against a voxel object") == nr.DEFERRED
    # the swap: the plane's contact names the sphere / the capsule first
    a, b = cases["plane under a sphere (swapped)"]
    c = nr.pair_contacts(a, b)[1][0]
    assert int(c["id"]) == int(nr.splitmix(b["id"] ^ nr.splitmix(a["id"]))) and int(c["body_a"]) == int(b["body"])


def test_sphere_forms_of_the_restatement_equal_the_oracle(decided_pairs):
    """narrow_ref's sphere-sphere and sphere-plane against oracle_lib on the same seeds: verdict, position, normal and depth byte for byte"""
    for (sa, sb), call in (((S, S), lambda f, s: ol.sphere_sphere_contact(f["a"], float(f["s"]), s["a"], float(s["s"]))),
                           ((S, P), lambda f, s: ol.sphere_plane_contact(f["a"], float(f["s"]), s["a"], float(s["s"])))):
        a, b = nr.seeded_pairs(sa, sb, N_SEEDED + 300)
        verdict, want = nr.pair_contacts(a, b)
        for i in range(len(a)):
            got = call(a[i], b[i])
            assert (got is not None) == (verdict[i] == nr.CONTACT), (sa, sb, i)
            if got is not None:
                pos, nrm, depth = got
                assert pos.tobytes() == want["position"][i].tobytes() and nrm.tobytes() == want["normal"][i].tobytes(), (sa, sb, i)
                assert np.float32(depth).tobytes() == want["depth"][i].tobytes(), (sa, sb, i)


def test_closest_point_parameters_reproduce_the_reference_tests():
    """the known answers of impact_geometry/src/line.rs's own tests (closest_points_*), re-typed: (A start, A vector, B start, B vector) -> the two
    closest points, to its 1e-6"""
    known = [
        ((1, 0, 0), (0, 0, 0), (4, 5, 6), (0, 0, 0), (1, 0, 0), (4, 5, 6)),          # both segments are points
        ((1, 0, 0), (0, 0, 0), (0, -1, 0), (0, 2, 0), (1, 0, 0), (0, 0, 0)),         # segment A is a point
        ((0, 0, 0), (2, 0, 0), (1, 1, 0), (0, 0, 0), (1, 0, 0), (1, 1, 0)),          # segment B is a point
        ((-1, 0, 0), (2, 0, 0), (0, -1, 0), (0, 2, 0), (0, 0, 0), (0, 0, 0)),        # intersecting perpendicular segments
        ((0, 0, 0), (1, 0, 0), (0.5, 0, 1), (0, 1, 0), (0.5, 0, 0), (0.5, 0, 1)),    # skew segments
        ((0, 0, 0), (1, 0, 0), (0, 2, 0), (0, -1, 0), (0, 0, 0), (0, 1, 0)),         # t clamped to the segment's end, s recomputed
    ]
    for dtype in (np.float32, np.float64):
        rows = np.array(known, dtype=dtype)
        a1, v1, a2, v2 = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
        s, t = nr.closest_parameters(a1, v1, a2, v2)
        assert s.dtype == dtype
        assert np.abs((a1 + nr.scale(v1, s)) - rows[:, 4]).max() <= 1e-6 and np.abs((a2 + nr.scale(v2, t)) - rows[:, 5]).max() <= 1e-6
    # parallel segments: the returned points are the perpendicular distance apart
    a1, v1, a2, v2 = (np.array([v], dtype=np.float32) for v in ((0, 0, 0), (1, 0, 0), (0, 0, 1), (1, 0, 0)))
    s, t = nr.closest_parameters(a1, v1, a2, v2)
    assert abs(np.linalg.norm((a1 + nr.scale(v1, s)) - (a2 + nr.scale(v2, t))) - 1.0) <= 1e-6
    # the point forms (closest_point_on_line_segments_to_point): degenerate segment, interior projection, both clamps, a point on the segment
    for start, vector, point, want in (((1, 2, 3), (0, 0, 0), (5, 6, 7), (1, 2, 3)), ((0, 0, 0), (4, 0, 0), (3, 2, 0), (3, 0, 0)), ((2, 0, 0), (2, 0, 0), (0, 0, 0), (2, 0, 0)),
                                       ((0, 0, 0), (2, 0, 0), (5, 0, 0), (2, 0, 0)), ((0, 0, 0), (0, 6, 0), (0, 3, 0), (0, 3, 0))):
        a, v, c = (np.array([x], dtype=np.float32) for x in (start, vector, point))
        hit, pos, nrm, depth = nr.capsule_sphere(a, v, np.float32([100.0]), c, np.float32([0.0]))  # (position = the sphere's centre; depth = 100 - distance)
        assert abs((100.0 - float(depth[0])) - np.linalg.norm(np.array(point, dtype=np.float64) - want)) <= 1e-4


def test_float32_results_against_the_float64_version(decided_pairs):
    """on the decided seeded pairs: the same verdict as the float64 version; the normal has unit length, depth and position lie within the allowed
    error of the float64 values, and the position lies on B's surface (B = the second member after the swap). The allowed error is four times
    MEASURED (this test prints what it measures)."""
    measured = {}
    for (sa, sb), (a, b, first, second, margin) in decided_pairs.items():
        if (sa, sb) == (P, P):
            continue
        key = (int(first["shape"][0]), int(second["shape"][0]))
        hit32, pos32, nrm32, depth32 = nr.pair_geometry(first, second, np.float32)
        hit64, pos64, nrm64, depth64 = nr.pair_geometry(first, second, np.float64)
        assert hit32.tolist() == hit64.tolist() == (margin >= 0).tolist(), (sa, sb)
        h = np.nonzero(hit32)[0]
        scale, bound = scale_of(first, second)[h], bound_of(first, second)[h]
        err = np.maximum(np.maximum(np.abs(pos32[h] - pos64[h]).max(axis=1), np.abs(depth32[h] - depth64[h])) / scale, np.abs(nrm32[h] - nrm64[h]).max(axis=1))
        measured[key] = max(measured.get(key, 0.0), float(err.max()))
        assert (err <= bound).all(), (sa, sb, float(err.max()))
        assert (np.abs(np.linalg.norm(nrm32[h].astype(np.float64), axis=1) - 1.0) <= bound).all(), (sa, sb)
        # the position on B's surface, B's geometry in float64
        p, b_a, b_v, b_s = pos32[h].astype(np.float64), second["a"][h].astype(np.float64), second["b"][h].astype(np.float64), second["s"][h].astype(np.float64)
        if key[1] == P:
            off = nr.dot(b_a, p) - b_s
        elif key[1] == S:
            off = np.linalg.norm(p - b_a, axis=1) - b_s
        else:
            t = nr.clamp01(nr.dot(b_v, p - b_a) / nr.dot(b_v, b_v))
            off = np.linalg.norm(p - (b_a + nr.scale(b_v, t)), axis=1) - b_s
        assert (np.abs(off) <= bound * scale).all(), (sa, sb, float(np.abs(off / scale).max()))
    print("measured float32 errors:", {k: f"{v:.2e}" for k, v in measured.items()})
    for key, value in measured.items():
        assert MEASURED[key] / 4.0 <= value <= MEASURED[key] * 1.05, (key, value)  # (MEASURED is what this machine measures, not a looser figure)


def test_capsule_distance_equals_a_brute_force_minimum(decided_pairs):
    """the float64 closest-point distance of 200 seeded capsule pairs against the minimum over a 200 x 200 grid of the two parameters: never above
    it, and below it by no more than the grid's resolution, (|A's vector| + |B's vector|) / (2 x 199)"""
    a, b = decided_pairs[(CAP, CAP)][:2]
    a, b = a[:200], b[:200]
    a1, v1, a2, v2 = (x.astype(np.float64) for x in (a["a"], a["b"], b["a"], b["b"]))
    s, t = nr.closest_parameters(a1, v1, a2, v2)
    dist = np.linalg.norm((a1 + nr.scale(v1, s)) - (a2 + nr.scale(v2, t)), axis=1)
    grid = np.linspace(0.0, 1.0, 200)
    p1 = a1[:, None, :] + grid[None, :, None] * v1[:, None, :]
    p2 = a2[:, None, :] + grid[None, :, None] * v2[:, None, :]
    brute = np.linalg.norm(p1[:, :, None, :] - p2[:, None, :, :], axis=-1).reshape(len(a), -1).min(axis=1)
    resolution = (np.linalg.norm(v1, axis=1) + np.linalg.norm(v2, axis=1)) / (2.0 * 199.0)
    assert (dist <= brute + 1e-12).all() and (brute - dist <= resolution).all(), float((brute - dist - resolution).max())


def test_transform_is_byte_equal_to_the_restatement_and_its_boxes_contain_the_shape():
    rng = np.random.default_rng(9)
    n = 400
    local = np.zeros(4 * n, dtype=capi.COLLIDABLE_DTYPE)
    local["shape"] = np.repeat(np.array([S, P, CAP, nr.VOXEL], dtype=np.uint32), n)
    local["kind"], local["body"], local["id"] = rng.integers(0, 3, 4 * n), rng.integers(0, 1 << 31, 4 * n), rng.integers(1, 2 ** 63, 4 * n, dtype=np.uint64)
    local["a"], local["b"], local["s"] = rng.uniform(-2, 2, (4 * n, 3)), rng.uniform(-2, 2, (4 * n, 3)), rng.uniform(0.1, 1.5, 4 * n)
    local["response"] = rng.uniform(0, 1, (4 * n, 3))
    planes = local["shape"] == P
    local["a"][planes] /= np.linalg.norm(local["a"][planes], axis=1, keepdims=True)
    boxes_lo = np.minimum(local["a"], local["b"])
    vo = local["shape"] == nr.VOXEL
    local["a"][vo], local["b"][vo] = boxes_lo[vo], boxes_lo[vo] + rng.uniform(0.1, 3.0, (int(vo.sum()), 3))
    positions = rng.uniform(-30, 30, (4 * n, 3)).astype(np.float32)
    orientations = np.array([br.random_unit_quaternion(rng) for _ in range(4 * n)], dtype=np.float32)
    want_world, want_boxes = nr.transform(local, positions, orientations)
    for i in range(4 * n):
        world, box = collision.transform(local[i], positions[i], orientations[i])
        assert world.tobytes() == want_world[i].tobytes(), (i, world, want_world[i])
        assert box.tobytes() == want_boxes[i].tobytes(), (i, box, want_boxes[i])
    # containment, against the float64 shape: the allowance is a few float32 roundings of the coordinates involved (|position| <= 30, |local| <= 4)
    q, p = orientations.astype(np.float64), positions.astype(np.float64)
    rot = np.array([br.rotation_matrix_f64(x) for x in q])
    a64 = np.einsum("nij,nj->ni", rot, local["a"].astype(np.float64)) + p
    v64 = np.einsum("nij,nj->ni", rot, local["b"].astype(np.float64))
    r = local["s"].astype(np.float64)[:, None]
    lo, hi, slack = want_boxes["lower"].astype(np.float64), want_boxes["upper"].astype(np.float64), 64 * 2.0 ** -24 * 40.0
    sp, cp = local["shape"] == S, local["shape"] == CAP
    assert (lo[sp] <= a64[sp] - r[sp] + slack).all() and (hi[sp] >= a64[sp] + r[sp] - slack).all()
    for end in (a64, a64 + v64):
        assert (lo[cp] <= end[cp] - r[cp] + slack).all() and (hi[cp] >= end[cp] + r[cp] - slack).all()
    assert (want_boxes["lower"][planes] == -nr.FLT_MAX).all() and (want_boxes["upper"][planes] == nr.FLT_MAX).all()
    for corner in range(8):
        pick = np.array([(corner >> 2) & 1, (corner >> 1) & 1, corner & 1], dtype=bool)
        c64 = np.einsum("nij,nj->ni", rot, np.where(pick, local["b"], local["a"]).astype(np.float64)) + p
        assert (lo[vo] <= c64[vo]).all() and (hi[vo] >= c64[vo]).all()  # (no allowance: a voxel object's box is widened past its derivation's rounding)
    # a plane keeps its geometry: the transformed point n x displacement lies on the transformed plane
    tp = np.einsum("nij,nj->ni", rot, (local["a"] * local["s"][:, None]).astype(np.float64)) + p
    assert np.abs(nr.dot(want_world["a"].astype(np.float64), tp) - want_world["s"])[planes].max() <= slack


def test_plane_boxes_pair_with_every_finite_box_and_each_other():
    """the unbounded box a plane gets, against tests/bvol_ref.py: it intersects every finite box and its like; a box with a NaN bound still intersects
    nothing"""
    world, _ = br.scene(200)
    boxes = np.concatenate([world, np.zeros(3, dtype=capi.AABB_DTYPE)])
    boxes["lower"][200:202], boxes["upper"][200:202] = -nr.FLT_MAX, nr.FLT_MAX
    boxes["lower"][202], boxes["upper"][202] = (-nr.FLT_MAX, np.nan, -nr.FLT_MAX), nr.FLT_MAX
    with np.errstate(over="ignore"):
        pairs = br.pairs(boxes)[0]
    for plane in (200, 201):
        partners = set(pairs[pairs[:, 1] == plane][:, 0].tolist()) | set(pairs[pairs[:, 0] == plane][:, 1].tolist())
        assert partners == set(range(202)) - {plane}
    assert not ((pairs == 202).any())


def test_the_collidable_record_is_64_bytes_by_the_c_compiler(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "impact_voxel_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %zu\\n", sizeof(ivx_collidable), offsetof(ivx_collidable, id), offsetof(ivx_collidable, a), offsetof(ivx_collidable, s),\n'
                   '           offsetof(ivx_collidable, response));\n    return 0;\n}\n')
    exe = tmp_path / "size"
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.run(["gcc", "-I", inc, str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    fields = capi.COLLIDABLE_DTYPE.fields
    assert got == [64, fields["id"][1], fields["a"][1], fields["s"][1], fields["response"][1]] == [64, 16, 24, 48, 52]
    assert capi.COLLIDABLE_DTYPE.itemsize == 64 and capi.extra_struct_sizes()["ivx_collidable"][1] == 64
    for name in ("ivx_cw_transform", "ivx_cw_contact", "ivx_cw_set_collidables", "ivx_cw_synchronize", "ivx_cw_download", "ivx_cw_collide", "ivx_cw_device_ptr"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(capi.lib(), name)


def test_host_exports_refuse_bad_shapes():
    bad = np.zeros(1, dtype=capi.COLLIDABLE_DTYPE)
    bad["shape"] = 4
    good = np.zeros(1, dtype=capi.COLLIDABLE_DTYPE)
    with pytest.raises(capi.IvxError):
        collision.contact(bad, good)
    with pytest.raises(capi.IvxError):
        collision.transform(bad, (0, 0, 0), (0, 0, 0, 1))


@pytest.mark.parametrize("n", [10, 100, 500, 2000])
def test_the_scene_of_the_device_tests_mixes_hits_and_misses(n):
    """narrow_ref.scene(n): planes last, a fifth of the bodies kinematic, and between a quarter and three quarters of the broad phase's pairs yield a
    contact under both modes, so most waves of the narrow phase hold hits and misses; some pairs are deferred"""
    local, dyn, kin = nr.scene(n)
    assert (local["shape"][-3:] == P).all() and not (local["shape"][:-3] == P).any()
    kinematic = (local["body"][:-3] & capi.KINEMATIC_BIT) != 0
    assert n < 100 or 0.1 <= kinematic.mean() <= 0.3
    for mode in (capi.BV_ALL_PAIRS, capi.BV_DYNAMIC_PAIRS):
        world, boxes, pairs, contacts, deferred = nr.scene_reference(n, mode)
        assert len(pairs) >= n and 0.25 <= len(contacts) / len(pairs) <= 0.75, (n, mode, len(pairs), len(contacts))
        assert n < 100 or len(deferred) > 0
        assert len(contacts) + len(deferred) < len(pairs)
