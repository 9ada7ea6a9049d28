"""Numpy checker of the frame-instance stage (impact_amd/csrc/instances.hip), written from the reference lines the header names
(impact_scene/src/light.rs:383-450, 747-787, model.rs:171-297, impact_geometry/src/axis_aligned_box.rs:208-239, 350-363,
impact_math/src/transform/similarity.rs:278-284) and from the text of include/impact_voxel_hip.h, in four parts:

  * the FLOAT32 form: every intermediate is an np.float32 array, in exactly the operation order the header states (`views_f32`, vectorised);
  * a float64 form of the composition and of the boxes (`compose_f64`, `distances_f64`);
  * `reference_frame`: a transliteration of the reference's loops — per view over that view's hits in ascending index, filter, take min / max,
    append — one object at a time with scalar float32 arithmetic; the batch form is held against it;
  * the seeded scene (instances over `bvol_ref.scene`) and seeded views."""
import functools

import numpy as np

import bvol_ref as br
from impact_amd import capi

f32 = np.float32
INF = f32(np.inf)


# ---- the total order of the bit patterns (-0.0 below +0.0; a positive NaN above +inf) -------------------------------------------------------------
def order_key(a):
    """the bit pattern as a signed 32-bit integer b; a negative one becomes int32(b ^ 0x7FFFFFFF), which is negative again and ascends with the
    float (computed in int64)"""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    u = (b & 0xFFFFFFFF) ^ 0x7FFFFFFF
    flipped = np.where(u >= 1 << 31, u - (1 << 32), u)
    return np.where(b < 0, flipped, b)


def order_reduce(values, want_min, empty):
    """the order_min / order_max of a 1-d float32 array (bit pattern kept), `empty` for none"""
    values = np.ascontiguousarray(values, dtype=np.float32)
    if values.size == 0:
        return f32(empty)
    k = order_key(values)
    return values[int(np.argmin(k) if want_min else np.argmax(k))]


# ---- float32 arithmetic of the header -----------------------------------------------------------------------------------------------------------
def distances_f32(lo, hi, p):
    """(d_close, d_far) of [n, 3] boxes from point p"""
    lo, hi, p = lo.astype(f32), hi.astype(f32), np.asarray(p, dtype=f32)
    c = np.where(lo > p, lo, p)
    c = np.where(hi < c, hi, c).astype(f32)
    e = p - c
    m = f32(0.5) * (lo + hi)
    far = np.where(p > m, lo, hi).astype(f32)
    g = p - far
    return (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2], (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]


def transformed_boxes_f32(lo, hi, sim):
    """ivx_bv_world_aabb's arithmetic over [n, 3] boxes under one similarity -> (lower, upper)"""
    lo, hi = lo.astype(f32), hi.astype(f32)
    c, h = f32(0.5) * (lo + hi), f32(0.5) * (hi - lo)
    x, y, z, w = (f32(v) for v in sim["rotation"])
    s = f32(sim["scaling"])
    xx, yy, zz, ww = x * x, y * y, z * z, w * w
    n2 = ((xx + yy) + zz) + ww
    xy, xz, yz, wx, wy, wz = x * y, x * z, y * z, w * x, w * y, w * z
    two = f32(2.0)
    N = [[((ww + xx) - yy) - zz, two * (xy - wz), two * (xz + wy)], [two * (xy + wz), ((ww - xx) + yy) - zz, two * (yz - wx)], [two * (xz - wy), two * (yz + wx), ((ww - xx) - yy) + zz]]
    out_lo, out_hi = np.zeros_like(lo), np.zeros_like(hi)
    for i in range(3):
        m0, m1, m2 = (s * (f32(N[i][j]) / n2) for j in range(3))
        ct = ((m0 * c[:, 0] + m1 * c[:, 1]) + m2 * c[:, 2]) + f32(sim["translation"][i])
        ht = (np.abs(m0) * h[:, 0] + np.abs(m1) * h[:, 1]) + np.abs(m2) * h[:, 2]
        out_lo[:, i], out_hi[:, i] = ct - ht, ct + ht
    assert out_lo.dtype == np.float32
    return out_lo, out_hi


def rotate_f32(q, v):
    """glam's mul_vec3a as the header writes it: q [4] (xyzw), v [n, 3]"""
    q, v = np.asarray(q, dtype=f32), np.asarray(v, dtype=f32)
    b, w = q[:3], q[3]
    b2 = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]
    dv = (v[:, 0] * b[0] + v[:, 1] * b[1]) + v[:, 2] * b[2]
    cross = np.stack([b[1] * v[:, 2] - v[:, 1] * b[2], b[2] * v[:, 0] - v[:, 2] * b[0], b[0] * v[:, 1] - v[:, 0] * b[1]], axis=1)
    k0, k2 = w * w - b2, w * f32(2.0)
    return (v * k0 + b[None, :] * (dv * f32(2.0))[:, None]) + cross * k2


def compose_f32(a, b):
    """world_to_view (one record) x model_to_world ([n] records) -> [n] SIMILARITY_DTYPE"""
    out = np.zeros(len(b), dtype=capi.SIMILARITY_DTYPE)
    a_s, at, aq = f32(a["scaling"]), a["translation"].astype(f32), a["rotation"].astype(f32)
    bt, bq = b["translation"].astype(f32), b["rotation"].astype(f32)
    out["translation"] = rotate_f32(aq, a_s * bt) + at[None, :]
    ax, ay, az, aw = aq
    bx, by, bz, bw = bq[:, 0], bq[:, 1], bq[:, 2], bq[:, 3]
    out["rotation"][:, 0] = ((aw * bx + ax * bw) + ay * bz) - az * by
    out["rotation"][:, 1] = ((aw * by - ax * bz) + ay * bw) + az * bx
    out["rotation"][:, 2] = ((aw * bz + ax * by) - ay * bx) + az * bw
    out["rotation"][:, 3] = ((aw * bw - ax * bx) - ay * by) - az * bz
    out["scaling"] = a_s * b["scaling"].astype(f32)
    return out


# ---- float64 -----------------------------------------------------------------------------------------------------------------------------------
def compose_f64(a, b):
    """one pair in float64 -> (translation [3], rotation [4], scaling), the rotation by the rotation matrix of the (unit) quaternion"""
    aq, bq = a["rotation"].astype(np.float64), b["rotation"].astype(np.float64)
    r = br.rotation_matrix_f64(aq)
    t = r @ (np.float64(a["scaling"]) * b["translation"].astype(np.float64)) + a["translation"].astype(np.float64)
    ax, ay, az, aw = aq
    bx, by, bz, bw = bq
    q = np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])
    return t, q, np.float64(a["scaling"]) * np.float64(b["scaling"])


def distances_f64(lo, hi, p):
    lo, hi, p = lo.astype(np.float64), hi.astype(np.float64), np.asarray(p, dtype=np.float64)
    c = np.minimum(np.maximum(p, lo), hi)
    far = np.where(p > 0.5 * (lo + hi), lo, hi)
    return ((p - c) ** 2).sum(axis=-1), ((p - far) ** 2).sum(axis=-1)


# ---- the batch form, float32 ------------------------------------------------------------------------------------------------------------------
def bits_of(masks, n):
    """[rows, W] uint64 -> [rows, n] bool"""
    masks = np.ascontiguousarray(masks, dtype="<u8")
    if masks.size == 0:
        return np.zeros((masks.shape[0], 0), dtype=bool)
    return np.unpackbits(masks.view(np.uint8).reshape(masks.shape[0], -1), axis=1, bitorder="little")[:, :n].astype(bool)


def identity_skip_pairs(shape):
    p = np.zeros(shape, dtype=capi.CULL_PAIR_DTYPE)
    p["rotation"][..., 3], p["scaling"], p["flags"] = 1.0, 1.0, capi.CULL_PAIR_SKIP
    return p


def empty_result():
    r = np.zeros((), dtype=capi.FI_VIEW_RESULT_DTYPE)
    for box in ("world_box", "view_box"):
        r[box]["lower"], r[box]["upper"] = np.inf, -np.inf
    r["min_squared_distance"], r["max_squared_distance"] = np.inf, -np.inf
    return r


def kept_f32(world, inst, hits, view, prev_bits):
    """the kept-set rule for one view -> ([n] bool, d_close, d_far)"""
    lo, hi = world["lower"].astype(f32), world["upper"].astype(f32)
    keep = hits.copy()
    keep &= (inst["flags"] & view["reject_flags"]) == 0
    keep &= inst["entity"] != view["exclude_entity"]
    if int(view["and_view"]) != capi.FI_NONE:
        keep &= prev_bits[int(view["and_view"])]
    keep &= ~(np.isnan(lo).any(axis=1) | np.isnan(hi).any(axis=1))
    d_close = d_far = None
    if int(view["flags"]) & capi.FI_VIEW_REACH:
        with np.errstate(invalid="ignore", over="ignore"):
            d_close, d_far = distances_f32(lo, hi, view["point"])
        keep &= ~(d_close > f32(view["squared_reach"]))
    return keep, d_close, d_far


def views_f32(world, inst, masks, views, prev_kept=None):
    """-> (pairs [nv, n], offsets [nv + 1], objects, transforms, kept [nv, W] uint64, results [nv]) exactly as the header states them"""
    n, nv = len(world), len(views)
    hits_all = bits_of(masks, n)
    prev_bits = None if prev_kept is None else bits_of(prev_kept, n)
    pairs, results = identity_skip_pairs((nv, n)), np.zeros(nv, dtype=capi.FI_VIEW_RESULT_DTYPE)
    offsets, objects, transforms, kept_bits = np.zeros(nv + 1, dtype=np.uint32), [], [], np.zeros((nv, n), dtype=bool)
    lo, hi = world["lower"].astype(f32), world["upper"].astype(f32)
    for v, view in enumerate(views):
        keep, d_close, d_far = kept_f32(world, inst, hits_all[int(view["query"])], view, prev_bits)
        idx = np.nonzero(keep)[0]
        kept_bits[v] = keep
        r = empty_result()
        r["count"] = idx.size
        for k in range(3):
            r["world_box"]["lower"][k] = order_reduce(lo[idx, k], True, np.inf)
            r["world_box"]["upper"][k] = order_reduce(hi[idx, k], False, -np.inf)
        if int(view["flags"]) & capi.FI_VIEW_BOX:
            with np.errstate(invalid="ignore", over="ignore"):
                vlo, vhi = transformed_boxes_f32(lo[idx], hi[idx], view["world_to_view"])
            for k in range(3):
                r["view_box"]["lower"][k] = order_reduce(vlo[:, k], True, np.inf)
                r["view_box"]["upper"][k] = order_reduce(vhi[:, k], False, -np.inf)
        if int(view["flags"]) & capi.FI_VIEW_REACH:
            r["min_squared_distance"] = order_reduce(d_close[idx], True, np.inf)
            r["max_squared_distance"] = order_reduce(d_far[idx], False, -np.inf)
        results[v] = r
        sims = compose_f32(view["world_to_view"], inst["model_to_world"][idx])
        for name in ("rotation", "translation", "scaling"):
            pairs[name][v, idx] = sims[name]
        pairs["instance_idx"][v, idx] = (int(view["instance_base"]) + np.arange(idx.size)).astype(np.uint32)
        pairs["flags"][v, idx] = 0
        objects.append(idx.astype(np.uint32))
        transforms.append(sims)
        offsets[v + 1] = offsets[v] + idx.size
    kept, _ = br.masks_of(kept_bits)
    objects = np.concatenate(objects) if objects else np.zeros(0, dtype=np.uint32)
    transforms = np.concatenate(transforms) if transforms else np.zeros(0, dtype=capi.SIMILARITY_DTYPE)
    return pairs, offsets, objects.astype(np.uint32), transforms, kept, results


# ---- the reference's loops, one hit at a time ----------------------------------------------------------------------------------------------------
def _less(a, b):
    return int(order_key(np.array([a], dtype=f32))[0]) < int(order_key(np.array([b], dtype=f32))[0])


def reference_frame(world, inst, masks, views, prev_kept=None):
    """light.rs step by step: for each view, for each hit of its query in ascending index: skip the light's own entity, skip a missing node or
    rejected flags, skip what the previous view did not keep (shadowing_models.get), skip beyond reach; min / max; append the transform ->
    per view (list of object indices, list of composed records, result record)"""
    n = len(world)
    hits_all = bits_of(masks, n)
    prev_bits = None if prev_kept is None else bits_of(prev_kept, n)
    out = []
    for view in views:
        reach, box = bool(int(view["flags"]) & capi.FI_VIEW_REACH), bool(int(view["flags"]) & capi.FI_VIEW_BOX)
        r, objs, sims = empty_result(), [], []
        for o in np.nonzero(hits_all[int(view["query"])])[0]:
            if int(inst["entity"][o]) == int(view["exclude_entity"]):
                continue  # ignore self-shadowing
            if int(inst["flags"][o]) & int(view["reject_flags"]):
                continue  # get_node -> None, or flags().intersects(..)
            if int(view["and_view"]) != capi.FI_NONE and not prev_bits[int(view["and_view"])][o]:
                continue  # only include models deemed as shadowing
            lo, hi = world["lower"][o].astype(f32), world["upper"][o].astype(f32)
            if np.isnan(lo).any() or np.isnan(hi).any():
                continue
            if reach:
                p = view["point"].astype(f32)
                closest = np.array([min(max(p[k], lo[k]), hi[k]) for k in range(3)], dtype=f32)  # point.max_with(lower).min_with(upper)
                e = p - closest
                d_close = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
                if d_close > f32(view["squared_reach"]):
                    continue  # the light doesn't reach the model
                centre = f32(0.5) * (lo + hi)
                far = np.array([lo[k] if p[k] > centre[k] else hi[k] for k in range(3)], dtype=f32)
                g = p - far
                d_far = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
                if _less(d_close, r["min_squared_distance"]):
                    r["min_squared_distance"] = d_close
                if _less(r["max_squared_distance"], d_far):
                    r["max_squared_distance"] = d_far
            boxes = [("world_box", lo, hi)]
            if box:
                vlo, vhi = transformed_boxes_f32(lo[None, :], hi[None, :], view["world_to_view"])
                boxes.append(("view_box", vlo[0], vhi[0]))
            for name, blo, bhi in boxes:
                for k in range(3):
                    if _less(blo[k], r[name]["lower"][k]):
                        r[name]["lower"][k] = blo[k]
                    if _less(r[name]["upper"][k], bhi[k]):
                        r[name]["upper"][k] = bhi[k]
            objs.append(int(o))
            sims.append(compose_f32(view["world_to_view"], inst["model_to_world"][o:o + 1])[0])
        r["count"] = len(objs)
        out.append((objs, sims, r))
    return out


# ---- the seeded scene ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene(n, seed):
    world, _ = br.scene(n, 11)
    rng = np.random.default_rng(seed)
    inst = np.zeros(n, dtype=capi.FI_INSTANCE_DTYPE)
    for o in range(n):
        inst["model_to_world"]["rotation"][o] = br.random_unit_quaternion(rng)
    inst["model_to_world"]["translation"] = rng.uniform(-20.0, 20.0, (n, 3))
    inst["model_to_world"]["scaling"] = rng.uniform(0.25, 4.0, n)
    # every flag combination: half of the objects have none (so that views keep something), the others walk through all 32
    flags = np.where(rng.random(n) < 0.5, 0, rng.permutation(np.arange(n)) % 32).astype(np.uint32)
    if n >= 64:
        flags[rng.choice(n, 32, replace=False)] = np.arange(32, dtype=np.uint32)
    inst["flags"] = flags
    inst["entity"] = rng.permutation(n).astype(np.uint32) + 100
    inst.setflags(write=False)
    return world, inst


def scene(n, seed=31):
    """`bvol_ref.scene(n)`'s world boxes with n instances: random unit quaternions, translations within 20 of the origin, scalings in [0.25, 4],
    flags covering every combination (for n >= 64), entities a permutation of 100 .. 100 + n -> (world boxes, instances); cached and read-only"""
    return _scene(int(n), int(seed))


def scene_masks(n, n_queries, seed=3):
    """the masks of `bvol_ref.mixed_queries` over the scene, by the float32 restatement of bvol_ref -> ([n_queries, W] uint64, the records)"""
    world, _ = scene(n)
    q = br.mixed_queries(max(n, 1), n_queries, seed)
    masks, _ = br.queries(world, q)
    return masks, q


def random_similarity(rng, scaling=None):
    s = np.zeros((), dtype=capi.SIMILARITY_DTYPE)
    s["rotation"], s["translation"] = br.random_unit_quaternion(rng), rng.uniform(-10.0, 10.0, 3)
    s["scaling"] = rng.uniform(0.25, 4.0) if scaling is None else scaling
    return s


def seeded_views(n, n_views, n_queries, n_previous=0, seed=7, reach=True, box=True):
    """`n_views` views over the scene of n: random world_to_view similarities, query v % n_queries, a reject mask from a short list, every third an
    excluded entity of the scene, every other an and_view when there is a previous call, distinct instance bases, REACH / BOX bits cycling
    through the four combinations (as far as `reach` / `box` allow), the point in the scene and a reach that takes in part of it"""
    rng = np.random.default_rng(seed + 1000 * n + n_views)
    _, inst = scene(n) if n else (None, np.zeros(0, dtype=capi.FI_INSTANCE_DTYPE))
    ext = br.scene_extent(max(n, 1))
    out = np.zeros(n_views, dtype=capi.FI_VIEW_DTYPE)
    rejects = [0, capi.FI_ABSENT | capi.FI_HIDDEN, 31, capi.FI_CASTS_NO_SHADOWS, capi.FI_ABSENT | capi.FI_NO_SHADOW_FEATURES | capi.FI_SHADOWS_OFF_BY_DISTANCE]
    for v in range(n_views):
        out["world_to_view"][v] = random_similarity(rng, 1.0 if v % 2 else None)
        out["query"][v] = v % n_queries
        out["reject_flags"][v] = rejects[v % len(rejects)]
        out["exclude_entity"][v] = int(inst["entity"][rng.integers(n)]) if n and v % 3 == 0 else capi.FI_NONE
        out["and_view"][v] = int(rng.integers(n_previous)) if n_previous and v % 2 == 1 else capi.FI_NONE
        out["instance_base"][v] = 1000 * v + 7
        out["flags"][v] = ((v & 1) * capi.FI_VIEW_REACH if reach else 0) | (((v >> 1) & 1) * capi.FI_VIEW_BOX if box else 0)
        out["point"][v] = rng.uniform(0.0, ext, 3)
        out["squared_reach"][v] = (rng.uniform(0.3, 0.8) * ext) ** 2
    return out


def outputs_bytes(pairs, offsets, objects, transforms, kept, results):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (pairs, offsets, objects, transforms, kept, results))
