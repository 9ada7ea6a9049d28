"""The sets and queries both files of the hierarchy's region queries use (test_bvh_queries_cpu.py, test_gpu_bvh_queries.py): the seeded scene with
bvol_ref.mixed_queries, the hand-made sets of bvh_ref.py, and the sets made to catch a node decision that skips a leaf the flat form hits.
Every expectation is bvol_ref's float32 restatement of the flat decisions; nothing here comes from the tree."""
import functools

import numpy as np

import bvh_ref as hr
import bvol_ref as br
from impact_amd import bvol, capi

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max
SIZES = [0, 1, 2, 3, 63, 64, 65, 129, 1000, 4097]
QUERY_COUNTS = [1, 7, 1024]


def reference(world, queries):
    with np.errstate(over="ignore", invalid="ignore"):
        return br.queries(world, queries)


def random_rotation(rng):
    return br.rotation_matrix_f64(br.random_unit_quaternion(rng))


def box_planes(center, axes, half):
    """the six planes of the box with the rows of `axes` as its axes (inside where n . p - d >= 0)"""
    planes = []
    for a in range(3):
        along = float(axes[a] @ np.asarray(center, dtype=np.float64))
        planes.append(np.append(axes[a], along - half[a]))
        planes.append(np.append(-axes[a], -(along + half[a])))
    return np.array(planes, dtype=np.float32)


def queries_around(lo, hi, n_queries, seed, sizes=(0.05, 0.45)):
    """`n_queries` records, kind = index % 4, with centres uniform in the box (lo, hi) and sizes a fraction of its diagonal drawn from `sizes`;
    frusta and oriented boxes under rotations uniform on the sphere"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    diagonal = float(np.linalg.norm(hi - lo)) or 1.0
    out = []
    for i in range(n_queries):
        centre = rng.uniform(lo, hi)
        size = rng.uniform(*sizes) * diagonal
        kind = i % 4
        if kind == capi.BV_QUERY_BOX:
            half = size * rng.uniform(0.3, 1.0, 3)
            out.append(bvol.box_query(centre - half, centre + half))
        elif kind == capi.BV_QUERY_SPHERE:
            out.append(bvol.sphere_query(centre, size))
        else:
            axes, half = random_rotation(rng), size * rng.uniform(0.3, 1.0, 3)
            if kind == capi.BV_QUERY_FRUSTUM:
                out.append(bvol.frustum_query(box_planes(centre, axes, half)))
            else:
                q = np.zeros((), dtype=capi.BV_QUERY_DTYPE)
                q["kind"], q["axes"], q["box_center"], q["half_extents"] = capi.BV_QUERY_ORIENTED_BOX, axes, centre, half
                out.append(q)
    return bvol.query_array(out)


def extent_of(world):
    """the box around the members that have no NaN bound and are not unbounded ((0, 0, 0) - (1, 1, 1) when there is none)"""
    sound = world[~(hr.has_nan(world) | hr.unbounded(world))]
    if not len(sound):
        return np.zeros(3), np.ones(3)
    return np.minimum(sound["lower"], sound["upper"]).min(axis=0).astype(np.float64), np.maximum(sound["lower"], sound["upper"]).max(axis=0).astype(np.float64)


def queries_over(world, n_queries, seed):
    return queries_around(*extent_of(world), n_queries, seed)


# ---- the adversarial sets ----------------------------------------------------------------------------------------------------------------------
def touching_case():
    """the seeded scene (bounds on multiples of 1/8) under box queries with corners on the same lattice: faces touch the query exactly"""
    world = np.array(br.scene(257)[0])
    rng = np.random.default_rng(8)
    ext = br.scene_extent(257)
    out = []
    for _ in range(48):
        centre, half = np.round(rng.uniform(0, ext, 3) * 8) / 8, np.round(rng.uniform(0.25, 2.5, 3) * 8) / 8
        out.append(bvol.box_query(centre - half, centre + half))
    return world, bvol.query_array(out)


def signed_zero_case():
    """(-0.0) - (+0.0) = -0.0: a box whose upper x is -0.0 misses a query whose lower x is +0.0, one whose upper x is +0.0 touches it; and the same
    with the roles exchanged (the query's upper -0.0 against lowers of +0.0 and -0.0)"""
    world = bvol.boxes([(-1, 0, 0), (-1, 2, 0), (0.0, 4, 0), (-0.0, 6, 0), (5, 5, 5)], [(-0.0, 1, 1), (0.0, 3, 1), (1, 5, 1), (1, 7, 1), (6, 6, 6)])
    queries = bvol.query_array([bvol.box_query((0.0, -1, -1), (3, 8, 2)), bvol.box_query((-3, -1, -1), (-0.0, 8, 2)), bvol.box_query((-0.0, -1, -1), (3, 8, 2))])
    return world, queries


def nan_bound_case():
    """the seeded scene with a NaN in one bound of every ninth object, under spheres (which the flat form lets hit them) and the other kinds"""
    world = np.array(br.scene(257)[0])
    rng = np.random.default_rng(9)
    for o in range(0, 257, 9):
        world[("lower", "upper")[int(rng.integers(2))]][o][int(rng.integers(3))] = np.nan
    world["lower"][100], world["upper"][100] = np.nan, np.nan
    return world, queries_over(world, 64, 19)


def inverted_case():
    """the seeded scene with lower > upper on one or more axes of every seventh object (a set stored as given may hold them)"""
    world = np.array(br.scene(257)[0])
    rng = np.random.default_rng(10)
    for o in range(0, 257, 7):
        for k in rng.choice(3, size=int(rng.integers(1, 4)), replace=False):
            world["lower"][o][k], world["upper"][o][k] = world["upper"][o][k] + f32(rng.uniform(0, 3)), world["lower"][o][k] - f32(rng.uniform(0, 3))
    world["lower"][5], world["upper"][5] = np.inf, -np.inf  # (the neutral box, as given)
    return world, queries_over(world, 64, 20)


def scrambled_corners(queries, seed):
    """the frustum records with `corners` drawn at random: caller data that disagrees with the normals' signs"""
    rng = np.random.default_rng(seed)
    q = queries.copy()
    for i in np.nonzero(q["kind"] == capi.BV_QUERY_FRUSTUM)[0]:
        q["corners"][i] = rng.integers(0, 8, 6)
    return q


def frusta_over(world, n_queries, seed):
    """frusta only: boxes under rotations uniform on the sphere, and every fourth axis-aligned (normals with zero components, signed both ways)"""
    rng = np.random.default_rng(seed)
    lo, hi = extent_of(world)
    diagonal = float(np.linalg.norm(hi - lo))
    out = []
    for i in range(n_queries):
        axes = random_rotation(rng) if i % 4 else np.diag(rng.choice([-1.0, 1.0], 3))
        out.append(bvol.frustum_query(box_planes(rng.uniform(lo, hi), axes, rng.uniform(0.05, 0.4) * diagonal * rng.uniform(0.3, 1.0, 3))))
    return bvol.query_array(out)


def unbounded_case():
    """planes' +-FLT_MAX boxes, half spaces and slabs mixed into the seeded scene — in the middle, so that they sit under nodes with bounded
    leaves only if their code is the last: both the unkeyed boxes at the end of the order and bounded ones with huge extents — under frusta"""
    world = np.array(br.scene(257)[0])
    for o in (3, 120, 121, 256):
        world["lower"][o], world["upper"][o] = -FLT_MAX, FLT_MAX
    world["lower"][40][0], world["upper"][40][0] = -FLT_MAX, 2.0        # a half space (unkeyed)
    world["lower"][41][1], world["upper"][41][1] = f32(-9e29), f32(9e29)  # a slab that still takes a key
    world["upper"][42] = f32(9e29)
    return world, frusta_over(world, 64, 21)


def nan_queries(world, seed):
    """queries of each kind with one member a NaN, every member in turn"""
    base = queries_over(world, 4, seed)
    out = []
    members = {capi.BV_QUERY_BOX: [("lower", k) for k in range(3)] + [("upper", k) for k in range(3)],
               capi.BV_QUERY_SPHERE: [("center", k) for k in range(3)] + [("radius", None)],
               capi.BV_QUERY_FRUSTUM: [("planes", (p, k)) for p in (0, 3) for k in range(4)],
               capi.BV_QUERY_ORIENTED_BOX: [("axes", (0, 1)), ("axes", (2, 2)), ("box_center", 0), ("box_center", 2), ("half_extents", 1)]}
    for q in base:
        for name, at in members[int(q["kind"])]:
            r = q.copy()
            if at is None:
                r[name] = np.nan
            else:
                r[name][at] = np.nan
            out.append(r)
    return bvol.query_array(out)


OBB_ORIGIN = 1.0e6
OBB_ULP = 0.0625  # the spacing of float32 in [2^19, 2^20), which holds 1e6 and the whole set


@functools.lru_cache(maxsize=None)
def _far_oriented_case(seed):
    rng = np.random.default_rng(seed)
    queries = []
    for _ in range(6):
        q = np.zeros((), dtype=capi.BV_QUERY_DTYPE)
        q["kind"], q["axes"], q["half_extents"] = capi.BV_QUERY_ORIENTED_BOX, random_rotation(rng), rng.uniform(1.0, 4.0, 3)
        q["box_center"] = OBB_ORIGIN + rng.uniform(-2.0, 2.0, 3)
        queries.append(q)
    queries = bvol.query_array(queries)
    lowers, uppers = [], []
    xs = (f32(OBB_ORIGIN - 12.0) + f32(OBB_ULP) * np.arange(384, dtype=np.float32)).astype(np.float32)
    assert (np.nextafter(xs[:-1], f32(np.inf)) == xs[1:]).all()  # (a step of OBB_ULP is one nextafter)
    for line in range(48):
        # a line of boxes one nextafter apart in x: the same y, z and extents (0 or 1 ulp an axis: extents near 1e-2 are below the spacing here)
        yz = (f32(OBB_ORIGIN) + f32(OBB_ULP) * rng.integers(-48, 48, 2).astype(np.float32)).astype(np.float32)
        ext = f32(OBB_ULP) * rng.integers(0, 2, 3).astype(np.float32)
        lo = np.stack([xs, np.full_like(xs, yz[0]), np.full_like(xs, yz[1])], axis=1)
        line_boxes = bvol.boxes(lo, lo + ext)
        hits = br.query_hits(line_boxes, queries[line % len(queries)])
        for flip in np.nonzero(hits[1:] != hits[:-1])[0]:  # boxes flip and flip + 1 lie on the two sides of the decision
            for k in range(max(flip - 2, 0), min(flip + 4, len(xs))):
                lowers.append(line_boxes["lower"][k]), uppers.append(line_boxes["upper"][k])
    world = bvol.boxes(np.array(lowers), np.array(uppers))
    for a in (world, queries):
        a.setflags(write=False)
    return world, queries


def far_oriented_case(seed=12):
    """oriented boxes around (1e6, 1e6, 1e6) over boxes placed on both sides of the decision e - |l| = 0 within three float32 steps: along 48 lines
    in x every box is tried one nextafter from the last, and where bvol_ref.query_hits flips the three boxes on either side join the set"""
    return _far_oriented_case(seed)


def adversarial_cases():
    """name -> (world boxes, queries)"""
    cases = {"touching faces": touching_case(), "signed zero": signed_zero_case(), "nan bounds": nan_bound_case(), "lower above upper": inverted_case(),
             "unbounded under frusta": unbounded_case(), "far oriented boxes": far_oriented_case()}
    world, queries = unbounded_case()
    cases["unbounded, scrambled corners"] = (world, scrambled_corners(queries, 31))
    world = np.array(br.scene(257)[0])
    cases["scrambled corners"] = (world, scrambled_corners(queries_over(world, 64, 22), 32))
    cases["scrambled corners, frusta"] = (world, scrambled_corners(frusta_over(world, 64, 23), 33))
    cases["nan queries"] = (world, nan_queries(world, 24))
    world, _ = nan_bound_case()
    cases["nan queries over nan bounds"] = (world, nan_queries(world, 25))
    return cases


def hand_made_sets():
    """name -> world boxes: the hand-made sets of bvh_ref.py"""
    sets = {"identical 130": hr.identical_boxes(130), "line": hr.line_boxes(), "plane": hr.plane_boxes()}
    for at in (0, 77, 149, None):
        sets[f"full row {at}"] = hr.full_row_boxes(at)
    for name, (world, _) in hr.hand_made_cases().items():
        sets[name] = world
    return sets
