"""Numpy restatement of the hierarchy over a bounding-volume set (impact_amd/csrc/bvh.hip), written from the words of include/impact_voxel_hip.h
alone: the frame and the key in float32 (every intermediate an np.float32), the Karras node in Python integers, the union in the total order of
the bit patterns, and the descent rule of the pair walk. The box decision itself is bvol_ref's."""
import functools

import numpy as np

import bvol_ref as br
from impact_amd import bvol, capi

f32 = np.float32
LEAF = capi.BV_LEAF
LAST_CODE = 0x3FFFFFFF


# ---- the bit order ---------------------------------------------------------------------------------------------------------------------------
def order_key(x):
    """the bit pattern of one float32 as a signed integer that orders like the float, -0.0 below +0.0: a pattern with the sign bit set has its
    other 31 bits flipped"""
    b = int(np.float32(x).view(np.uint32))
    return ((b ^ 0x7FFFFFFF) - (1 << 32)) if b >> 31 else b


def order_min(a, b):
    return b if order_key(b) < order_key(a) else a


def order_max(a, b):
    return b if order_key(b) > order_key(a) else a


def union(lo_a, hi_a, lo_b, hi_b):
    """(lower, upper) of the union of two boxes, per component in the bit order"""
    return (np.array([order_min(x, y) for x, y in zip(lo_a, lo_b)], dtype=np.float32),
            np.array([order_max(x, y) for x, y in zip(hi_a, hi_b)], dtype=np.float32))


# ---- frame and key -----------------------------------------------------------------------------------------------------------------------------
def has_nan(world):
    return np.isnan(world["lower"]).any(axis=-1) | np.isnan(world["upper"]).any(axis=-1)


def unbounded(world):
    with np.errstate(invalid="ignore"):
        return (np.abs(world["lower"]) >= f32(1e30)).any(axis=-1) | (np.abs(world["upper"]) >= f32(1e30)).any(axis=-1)


def frame(world):
    """the union of the boxes with no NaN bound that are not unbounded; the all-zero box when there is none"""
    out = np.zeros((), dtype=capi.AABB_DTYPE)
    sound = world[~(has_nan(world) | unbounded(world))]
    if len(sound):
        for k in range(3):
            lo, hi = sound["lower"][:, k], sound["upper"][:, k]
            out["lower"][k] = functools.reduce(order_min, lo.tolist(), lo[0])
            out["upper"][k] = functools.reduce(order_max, hi.tolist(), hi[0])
    return out


def spread3(q):
    return sum(((q >> k) & 1) << (3 * k) for k in range(10))


def code(frame_box, box):
    one = np.array([box], dtype=capi.AABB_DTYPE)
    if has_nan(one)[0] or unbounded(one)[0]:
        return LAST_CODE
    q = []
    with np.errstate(all="ignore"):
        for k in range(3):
            c = f32(0.5) * (f32(box["lower"][k]) + f32(box["upper"][k]))
            t = (c - f32(frame_box["lower"][k])) / (f32(frame_box["upper"][k]) - f32(frame_box["lower"][k]))
            assert isinstance(t, np.float32)
            q.append(0 if not t > 0 else (int(t * f32(1024.0)) if t < 1 else 1023))
    return (spread3(q[0]) << 2) | (spread3(q[1]) << 1) | spread3(q[2])


def key(frame_box, box, index):
    return (code(frame_box, box) << 32) | int(index)


# ---- Karras's node -------------------------------------------------------------------------------------------------------------------------------
def delta(keys, i, j):
    if j < 0 or j >= len(keys):
        return -1
    x = keys[i] ^ keys[j]
    assert x != 0, "the keys are unique"
    return 64 - x.bit_length()


def karras(keys, i):
    """node i over the sorted keys -> (left, right, first, last)"""
    d = 1 if delta(keys, i, i + 1) - delta(keys, i, i - 1) > 0 else -1
    dmin = delta(keys, i, i - d)
    lmax = 2
    while delta(keys, i, i + lmax * d) > dmin:
        lmax *= 2
    length, t = 0, lmax // 2
    while t >= 1:
        if delta(keys, i, i + (length + t) * d) > dmin:
            length += t
        t //= 2
    j = i + length * d
    dnode = delta(keys, i, j)
    s, t = 0, (length + 1) // 2
    while True:
        if delta(keys, i, i + (s + t) * d) > dnode:
            s += t
        if t <= 1:
            break
        t = (t + 1) // 2
    split = i + s * d + min(d, 0)
    lo, hi = min(i, j), max(i, j)
    left = (LEAF | split) if lo == split else split
    right = (LEAF | (split + 1)) if hi == split + 1 else split + 1
    return left, right, lo, hi


# ---- the tree ------------------------------------------------------------------------------------------------------------------------------------
def leaf_boxes(world, leaf_objects):
    """the leaves' boxes in Morton order: the object's world box, the neutral box for an object with a NaN bound"""
    boxes = world[leaf_objects].copy()
    nan = has_nan(boxes)
    boxes["lower"][nan], boxes["upper"][nan] = np.inf, -np.inf
    return boxes


def child_box(nodes, leaves, ref):
    b = leaves[ref & ~LEAF] if ref & LEAF else nodes[ref]
    return b["lower"], b["upper"]


def build(world):
    """-> (nodes [max(n - 1, 0)], leaf objects [n], frame, sorted keys)"""
    n = len(world)
    fr = frame(world)
    keys = sorted(key(fr, world[o], o) for o in range(n))
    leaf_objects = np.array([k & 0xFFFFFFFF for k in keys], dtype=np.uint32)
    nodes = np.zeros(max(n - 1, 0), dtype=capi.BV_NODE_DTYPE)
    if n < 2:
        return nodes, leaf_objects, fr, keys
    leaves = leaf_boxes(world, leaf_objects)
    for i in range(n - 1):
        nodes["left"][i], nodes["right"][i], _, _ = karras(keys, i)
    depth, _ = bvol.node_info(nodes, n)
    for i in np.argsort(-depth.astype(np.int64), kind="stable"):  # (deepest first: a node's children are done before it)
        lo, hi = union(*child_box(nodes, leaves, int(nodes["left"][i])), *child_box(nodes, leaves, int(nodes["right"][i])))
        nodes["lower"][i], nodes["upper"][i] = lo, hi
    return nodes, leaf_objects, fr, keys


def range_ends(nodes, n):
    """per internal node the last leaf position below it"""
    depth, _ = bvol.node_info(nodes, n)
    last = np.zeros(len(nodes), dtype=np.int64)
    for i in np.argsort(-depth.astype(np.int64), kind="stable"):
        last[i] = max((c & ~LEAF) if c & LEAF else last[c] for c in (int(nodes["left"][i]), int(nodes["right"][i])))
    return last


def outside(lo_a, hi_a, lo_b, hi_b):
    with np.errstate(over="ignore", invalid="ignore"):  # (FLT_MAX - -FLT_MAX is +inf: not negative; inf - inf is a NaN: negative)
        return bool(br.negative(np.concatenate([hi_b - lo_a, hi_a - lo_b])).any())


def walk(world, kinds, mode, nodes, leaf_objects):
    """the pair walk over a given tree: from every leaf position p, descend from the root into a child only when its box is not outside the leaf's
    and its leaf range ends beyond p; at a leaf q > p the mode's kind filter -> [m, 2] uint32 (a < b as object indices), sorted"""
    n = len(world)
    kinds = np.zeros(n, dtype=np.uint32) if kinds is None else np.asarray(kinds)
    if n < 2:
        return np.zeros((0, 2), dtype=np.uint32)
    leaves = leaf_boxes(world, leaf_objects)
    last = range_ends(nodes, n)
    found = []
    for p in range(n):
        lo, hi, op = leaves["lower"][p], leaves["upper"][p], int(leaf_objects[p])
        stack = [0]
        while stack:
            i = stack.pop()
            for ref in (int(nodes["right"][i]), int(nodes["left"][i])):
                is_leaf, at = bool(ref & LEAF), ref & ~LEAF
                if (at if is_leaf else last[at]) <= p or outside(lo, hi, *child_box(nodes, leaves, ref)):
                    continue
                if not is_leaf:
                    stack.append(at)
                elif br.kinds_pass(kinds[op], kinds[int(leaf_objects[at])], mode):
                    oq = int(leaf_objects[at])
                    found.append((min(op, oq), max(op, oq)))
    return np.array(sorted(found), dtype=np.uint32).reshape(-1, 2)


# ---- the cases both test files use -------------------------------------------------------------------------------------------------------------
def identical_boxes(n=130):
    return bvol.boxes([(1, 2, 3)] * n, [(2, 3, 4)] * n)


def line_boxes(n=200, seed=5):
    """centres on one line (two zero-extent axes of the centres' frame are impossible: the boxes have extent; the codes still vary in x only)"""
    rng = np.random.default_rng(seed)
    c = np.stack([np.round(rng.uniform(0, 40, n) * 8) / 8, np.full(n, 1.0), np.full(n, -2.0)], axis=1)
    return bvol.boxes(c - 0.5, c + 0.5)


def plane_boxes(n=200, seed=6):
    rng = np.random.default_rng(seed)
    c = np.stack([np.round(rng.uniform(0, 12, n) * 8) / 8, np.round(rng.uniform(0, 12, n) * 8) / 8, np.full(n, 3.0)], axis=1)
    return bvol.boxes(c - 0.5, c + 0.5)


def full_row_boxes(at, n=150, seed=2):
    """test_pairs_hand_made_cases's full row: one box around n - 1 disjoint ones, at position `at`"""
    rng = np.random.default_rng(seed)
    small = np.stack([np.arange(n) * 2.0, rng.uniform(0, 5, n), rng.uniform(0, 5, n)], axis=1)
    world = bvol.boxes(small, small + 1.0)
    if at is not None:
        world["lower"][at], world["upper"][at] = (-1, -1, -1), (2 * n + 1, 7, 7)
    return world


def hand_made_cases():
    """name -> (world boxes, kinds or None): the cases of test_pairs_hand_made_cases, a NaN box in the middle, unbounded boxes at the end and in
    the middle"""
    flt_max = np.finfo(np.float32).max
    cases = {}
    for upper in (-0.0, 0.0):
        cases[f"signed zero {upper!r}"] = (bvol.boxes([(-1, 0, 0), (0.0, 0, 0)], [(upper, 1, 1), (1, 1, 1)]), None)
    cases["touching faces"] = (bvol.boxes([(0, 0, 0), (1, 0, 0), (3, 0, 0), (0.5, 0.5, 0.5)], [(1, 1, 1), (2, 1, 1), (4, 1, 1), (3.5, 0.75, 0.75)]), None)
    cases["identical 70"] = (identical_boxes(70), None)
    for at in (0, 77, 149):
        cases[f"full row {at}"] = (full_row_boxes(at), None)
    cases["disjoint"] = (full_row_boxes(None), None)
    world, kinds = (a.copy() for a in br.scene(65))
    world["upper"][31][2] = np.nan
    cases["nan in the middle"] = (world, kinds)
    for name, where in (("unbounded at the end", (63, 64)), ("unbounded in the middle", (20, 41))):
        world, kinds = (a.copy() for a in br.scene(65))
        for o in where:
            world["lower"][o], world["upper"][o] = -flt_max, flt_max
        cases[name] = (world, kinds)
    return cases
