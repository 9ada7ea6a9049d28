"""numpy restatement of chunk culling (impact_amd/csrc/cull.hip), in two parts:

  derive_f64   the culling frustum of a view and an object-to-view similarity in float64 (mesh.rs:638-696, render_commands.rs:591-598,
               plane.rs:186-192, oriented_box.rs:167-173, 221-240)
  classify / expected   the decision in FLOAT32 in the library's operation order — ((nx px + ny py) + nz pz) - d < -0.05f, the obscuredness
               lookup — and both output modes: slot layout, zero tail, counts (voxel_chunk_culling.template.wgsl)

plus the helpers the tests build views from (perspective planes, orthographic boxes, composed similarities).
"""
import numpy as np

from impact_amd import capi

F32 = np.float32
THRESHOLD = F32(-0.05)
# the shader's CORNERS_OFFSETS (AxisAlignedBox::corner): bit 2 / 1 / 0 of the index = upper x / y / z
CORNERS_OFFSETS = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 1, 1], [1, 0, 0], [1, 0, 1], [1, 1, 0], [1, 1, 1]], dtype=np.float32)


# ---- float64 derivation ------------------------------------------------------------------------------------------------------------------
def q_conj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]], dtype=np.float64)


def q_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz], dtype=np.float64)


def q_rot(q, v):
    u, w = np.asarray(q[:3], dtype=np.float64), float(q[3])
    v = np.asarray(v, dtype=np.float64)
    t = 2.0 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


def corner_of(normal):
    """maximum_corner_idx_along_direction: bit set where the component's sign bit is NOT set"""
    s = np.signbit(np.asarray(normal))
    return (0 if s[0] else 4) | (0 if s[1] else 2) | (0 if s[2] else 1)


def derive_f64(view, pair, chunk_extent):
    """-> (planes [6, 4], apex [3], T's translation) in float64 from the float32 inputs"""
    q = np.asarray(pair["rotation"], dtype=np.float64)
    t = np.asarray(pair["translation"], dtype=np.float64)
    s = float(pair["scaling"]) * float(chunk_extent)
    tq, ts = q_conj(q), 1.0 / s
    tt = -q_rot(tq, ts * t)

    def tp(p):
        return q_rot(tq, ts * np.asarray(p, dtype=np.float64)) + tt

    planes = np.zeros((6, 4))
    if int(view["kind"]) == 0:
        for i in range(6):
            n, d = np.asarray(view["planes"][i][:3], dtype=np.float64), float(view["planes"][i][3])
            n2 = q_rot(tq, n)
            planes[i, :3], planes[i, 3] = n2, float(np.dot(n2, tp(n * d)))
        apex = tt.copy()
    else:
        c = tp(view["box_center"])
        o = q_mul(tq, np.asarray(view["box_orientation"], dtype=np.float64))
        h = ts * np.asarray(view["box_half_extents"], dtype=np.float64)
        local = q_rot(q_conj(o), c)
        for a in range(3):
            axis = q_rot(o, np.eye(3)[a])
            planes[2 * a, :3], planes[2 * a, 3] = axis, local[a] - h[a]
            planes[2 * a + 1, :3], planes[2 * a + 1, 3] = -axis, -(local[a] + h[a])
        apex = c + float(view["apex_distance"]) * q_rot(o, np.eye(3)[2])
    return planes, apex, tt


# ---- float32 decision --------------------------------------------------------------------------------------------------------------------
def classify(table, rec):
    """-> (outside, obscured) per entry of the submesh table under one frustum record, float32 in the library's operation order"""
    ci = table["chunk_indices"].astype(np.float32)
    outside = np.zeros(len(table), dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(6):
            corner = int(rec["most_inside_corners"][q])
            off = CORNERS_OFFSETS[corner & 7]
            px, py, pz = ci[:, 0] + off[0], ci[:, 1] + off[1], ci[:, 2] + off[2]
            n = rec["planes"][q].astype(np.float32)
            dist = ((n[0] * px + n[1] * py) + n[2] * pz) - n[3]
            assert dist.dtype == np.float32
            outside |= dist < THRESHOLD
        apex = rec["apex"].astype(np.float32)
        view_dir = (ci + F32(0.5)) - apex[None, :]
        idx = (view_dir < F32(0.0)).astype(np.int64)
    obscured = table["is_obscured_from_direction"][np.arange(len(table)), idx[:, 0], idx[:, 1], idx[:, 2]] > 0
    return outside, obscured


def expected(tables, frusta, view_flags, pair_flags=None, objects=None, mode=0):
    """the argument region and the count record of every view: frusta [n_views, n_objects] CULLING_FRUSTUM_DTYPE records (as downloaded from the
    device), view_flags [n_views], pair_flags [n_views, n_objects] or None, objects CULL_OBJECT_DTYPE or None -> list of (args, (draws, indices))"""
    n_views, n_obj = len(view_flags), len(tables)
    frusta = np.asarray(frusta).reshape(n_views, n_obj) if n_obj else np.zeros((n_views, 0), dtype=capi.CULLING_FRUSTUM_DTYPE)
    total = sum(len(t) for t in tables)
    out = []
    for v in range(n_views):
        indexed = bool(int(view_flags[v]) & capi.CULL_VIEW_INDEXED)
        args = np.zeros(total, dtype=capi.DRAW_INDEXED_ARGS_DTYPE if indexed else capi.DRAW_ARGS_DTYPE)
        drawn_all = np.zeros(total, dtype=bool)
        base = 0
        for o, t in enumerate(tables):
            n = len(t)
            if n == 0:
                continue
            outside, obscured = classify(t, frusta[v, o])
            skip = pair_flags is not None and bool(int(np.asarray(pair_flags).reshape(n_views, n_obj)[v, o]) & capi.CULL_PAIR_SKIP)
            drawn = ~(outside | obscured) & (not skip)
            a = args[base:base + n]
            a["index_count"] = np.where(drawn, t["index_count"], 0)
            a["instance_count"] = drawn.astype(np.uint32)
            a["first_index"] = t["index_offset"] + (np.uint32(objects[o]["first_index_base"]) if objects is not None else np.uint32(0))
            if indexed:
                a["base_vertex"] = objects[o]["base_vertex"] if objects is not None else 0
            a["first_instance"] = frusta[v, o]["instance_idx"]
            drawn_all[base:base + n] = drawn
            base += n
        draws = int(drawn_all.sum())
        indices = int(args["index_count"].astype(np.uint64).sum() % (1 << 32))
        if mode == 1:
            compact = np.zeros_like(args)
            compact[:draws] = args[drawn_all]
            args = compact
        out.append((args, (draws, indices)))
    return out


def census(tables, frusta, n_views):
    """per view the fractions of slots (frustum-culled and not obscured, obscured and inside, drawn)"""
    n_obj = len(tables)
    frusta = np.asarray(frusta).reshape(n_views, n_obj)
    total = max(1, sum(len(t) for t in tables))
    out = np.zeros((n_views, 3))
    for v in range(n_views):
        for o, t in enumerate(tables):
            if len(t):
                outside, obscured = classify(t, frusta[v, o])
                out[v] += [(outside & ~obscured).sum(), (obscured & ~outside).sum(), (~outside & ~obscured).sum()]
    return out / total


# ---- views and similarities for the tests -------------------------------------------------------------------------------------------------
def random_unit_quaternion(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def perspective_view(fov_x_deg=90.0, fov_y_deg=90.0, near=0.1, far=100.0, indexed=False):
    """a kind-0 view looking along -z from the origin: left, right, bottom, top, near, far; inward unit normals, signed distance n . p - d"""
    v = np.zeros((), dtype=capi.CULL_VIEW_DTYPE)
    a, b = np.radians(fov_x_deg) / 2.0, np.radians(fov_y_deg) / 2.0
    v["planes"] = np.array([[np.cos(a), 0, -np.sin(a), 0], [-np.cos(a), 0, -np.sin(a), 0], [0, np.cos(b), -np.sin(b), 0], [0, -np.cos(b), -np.sin(b), 0],
                            [0, 0, -1, near], [0, 0, 1, -far]], dtype=np.float32)
    v["box_orientation"] = (0, 0, 0, 1)
    v["flags"] = capi.CULL_VIEW_INDEXED if indexed else 0
    return v


def orthographic_view(half_width, half_height, near, far, apex_distance=10000.0, orientation=(0.0, 0.0, 0.0, 1.0), indexed=True):
    """a kind-1 view: a box in front of the origin along -z (before `orientation` turns it about the origin)"""
    v = np.zeros((), dtype=capi.CULL_VIEW_DTYPE)
    v["kind"] = 1
    v["box_center"] = q_rot(np.asarray(orientation, dtype=np.float64), (0.0, 0.0, -0.5 * (near + far)))
    v["box_orientation"] = orientation
    v["box_half_extents"] = (half_width, half_height, 0.5 * (far - near))
    v["apex_distance"] = apex_distance
    v["flags"] = capi.CULL_VIEW_INDEXED if indexed else 0
    return v


def pair_record(view_rotation, view_position, object_rotation, object_translation, object_scaling, instance_idx=0, flags=0):
    """object-to-view similarity of a camera at `view_position` with orientation `view_rotation` (view -> world) and an object placed by
    (rotation, translation, scaling) in the world"""
    p = np.zeros((), dtype=capi.CULL_PAIR_DTYPE)
    vq = q_conj(np.asarray(view_rotation, dtype=np.float64))
    q = q_mul(vq, np.asarray(object_rotation, dtype=np.float64))
    p["rotation"] = q / np.linalg.norm(q)
    p["translation"] = q_rot(vq, np.asarray(object_translation, dtype=np.float64) - np.asarray(view_position, dtype=np.float64))
    p["scaling"] = object_scaling
    p["instance_idx"], p["flags"] = instance_idx, flags
    return p


def look_rotation(direction):
    """a unit quaternion (view -> world) that turns -z onto `direction`"""
    d = np.asarray(direction, dtype=np.float64)
    d = d / np.linalg.norm(d)
    z = np.array([0.0, 0.0, -1.0])
    c = float(np.dot(z, d))
    if c < -1.0 + 1e-12:
        return np.array([0.0, 1.0, 0.0, 0.0])
    ax = np.cross(z, d)
    q = np.array([ax[0], ax[1], ax[2], 1.0 + c])
    return q / np.linalg.norm(q)


def random_table(rng, n, max_index=40, p_obscured=0.5):
    """a seeded submesh table: chunk indices 0..max_index, each obscuredness entry set with probability p_obscured, disjoint index ranges"""
    t = np.zeros(n, dtype=capi.SUBMESH_DTYPE)
    t["chunk_indices"] = rng.integers(0, max_index + 1, size=(n, 3))
    t["index_count"] = 3 * rng.integers(1, 200, size=n)
    t["index_offset"] = np.concatenate(([0], np.cumsum(t["index_count"][:-1]))) if n else 0
    t["is_obscured_from_direction"] = (rng.random(size=(n, 2, 2, 2)) < p_obscured) * rng.integers(1, 3, size=(n, 2, 2, 2))
    t["vertex_count"] = rng.integers(4, 300, size=n)
    t["vertex_offset"] = np.concatenate(([0], np.cumsum(t["vertex_count"][:-1]))) if n else 0
    return t


def host_frusta(views, pairs, extents):
    """[n_views, n_objects] records by the library's host function"""
    from impact_amd import cull

    pairs = np.asarray(pairs).reshape(len(views), len(extents))
    out = np.zeros((len(views), len(extents)), dtype=capi.CULLING_FRUSTUM_DTYPE)
    for v in range(len(views)):
        for o in range(len(extents)):
            out[v, o] = cull.culling_frustum_from_view(views[v], pairs[v, o], extents[o])
    return out


_scenes = {}


def tiling_scene(sub_counts, n_views, seed, margin=0.12):
    """Seeded objects and views for the tiling tests: every object's 41^3 block of chunks lies, turned about its centre, over the same world
    cube; every view (kinds and `indexed` bits mixed) is drawn again until, by the restatement over the library's host records, at least
    `margin` of the slots are frustum-culled and not obscured, `margin` obscured and inside, `margin` drawn.
    -> (tables, extents, views, pairs [n_views, n_objects])"""
    key = (tuple(sub_counts), n_views, seed)
    if key in _scenes:
        return _scenes[key]
    rng = np.random.default_rng(seed)
    tables = [random_table(rng, n) for n in sub_counts]
    n_obj = len(tables)
    centre = np.full(3, 20.5)
    extents = rng.uniform(0.5, 2.0, size=n_obj).astype(np.float32)
    placed = []
    for o in range(n_obj):
        q, s = random_unit_quaternion(rng), rng.uniform(0.9, 1.1) / float(extents[o])
        t = centre + rng.uniform(-2.0, 2.0, size=3) - q_rot(q, s * float(extents[o]) * centre)
        placed.append((q, t, s))
    views = np.zeros(n_views, dtype=capi.CULL_VIEW_DTYPE)
    pairs = np.zeros((n_views, n_obj), dtype=capi.CULL_PAIR_DTYPE)
    # (kind, indexed) cycles through (0, 0) (1, 1) (0, 1) (1, 0): any two views in a row from an even start mix both kinds and both bits; the
    # start depends on the object set, so the one-view cases differ from one another
    cycle = ((False, False), (True, True), (False, True), (True, False))
    start = sum(sub_counts) % 4 if n_views == 1 else 2 * (sum(sub_counts) % 2)
    for v in range(n_views):
        orthographic, indexed = cycle[(v + start) % 4]
        for _ in range(400):
            direction = rng.normal(size=3)
            direction /= np.linalg.norm(direction)
            vq = q_mul(look_rotation(direction), np.array([0.0, 0.0, np.sin(0.5 * (a := rng.uniform(0, 2 * np.pi))), np.cos(0.5 * a)]))
            if orthographic:
                view = orthographic_view(rng.uniform(8, 30), rng.uniform(8, 30), 0.0, rng.uniform(15, 50), indexed=indexed)
                position = centre - direction * rng.uniform(0.0, 25.0) + rng.uniform(-8, 8, size=3)
            else:
                view = perspective_view(rng.uniform(70, 110), rng.uniform(70, 110), 0.1, rng.uniform(30, 80), indexed=indexed)
                position = centre - direction * rng.uniform(0.0, 18.0) + rng.uniform(-5, 5, size=3)
            row = np.zeros(n_obj, dtype=capi.CULL_PAIR_DTYPE)
            for o, (q, t, s) in enumerate(placed):
                row[o] = pair_record(vq, position, q, t, s, instance_idx=1000 * v + o)
            recs = host_frusta(view.reshape(1), row.reshape(1, n_obj), extents)
            if n_obj == 0 or sum(len(t) for t in tables) == 0 or census(tables, recs, 1).min() >= margin:
                views[v], pairs[v] = view, row
                break
        else:
            raise AssertionError(f"no view {v} with the wanted census for seed {seed}")
    _scenes[key] = (tables, extents, views, pairs)
    return _scenes[key]
