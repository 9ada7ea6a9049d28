"""numpy restatement of the reference's block evaluation of an atomic SDF program (SDFGenerator::compute_signed_distances_for_block,
atomic.rs:633-875) with multifractal noise nodes (atomic.rs:1420-1571), chunk by chunk, in the f32 operation order of the library's
sampler. The noise is the library's own (noise_ref.py). Used to check noisy objects voxel byte for voxel byte."""
from __future__ import annotations

import numpy as np

import noise_ref as nr
from impact_amd.voxel import SDFGenerator, SDFVoxelGenerator

f32 = np.float32
S, H = f32(15), f32(7.5)
II, JJ = np.meshgrid(np.arange(16, dtype=f32), np.arange(16, dtype=f32), indexing="ij")


def xform_point(m, p):
    r = m[0:3] * p[0]
    r = m[4:7] * p[1] + r
    r = m[8:11] * p[2] + r
    return m[12:15] + r


def aabb_of_transformed(lo, hi, m):
    c = xform_point(m, (lo + hi) * f32(0.5))
    h = (hi - lo) * f32(0.5)
    he = (np.abs(m[0:3]) * h[0] + np.abs(m[4:7]) * h[1]) + np.abs(m[8:11]) * h[2]
    return c - he, c + he


def lies_outside(dlo, dhi, blo, bhi):
    return bool(np.any(np.signbit(bhi - dlo)) or np.any(np.signbit(dhi - blo)))


def contains_box(ilo, ihi, blo, bhi):
    return not (np.any(np.signbit(blo - ilo)) or np.any(np.signbit(ihi - bhi)))


def positions(m, o_root):
    """node-space voxel positions [i, j, k, 3]: ((origin + i dx) + j dy), then += dz voxel by voxel"""
    origin = xform_point(m, o_root)
    dx, dy, dz = m[0:3], m[4:7], m[8:11]
    pos = np.empty((16, 16, 16, 3), f32)
    p = (origin + II[..., None] * dx) + JJ[..., None] * dy
    for k in range(16):
        pos[:, :, k] = p
        p = p + dz
    return pos


def leaf_values(nd, pos):
    kind = int(nd["kind"])
    x, y, z = pos[..., 0], pos[..., 1], pos[..., 2]
    a, b, c = nd["a"], nd["b"], nd["c"]
    if kind == 1:
        y = y - np.clip(y, -a, a)
    if kind in (0, 1):
        return np.sqrt((x * x + y * y) + z * z) - (a if kind == 0 else b)
    qx, qy, qz = np.abs(x) - a, np.abs(y) - b, np.abs(z) - c
    px, py, pz = np.maximum(qx, f32(0)), np.maximum(qy, f32(0)), np.maximum(qz, f32(0))
    return np.sqrt((px * px + py * py) + pz * pz) + np.minimum(np.maximum(np.maximum(qx, qy), qz), f32(0))


def combine(kind, a, b, s, q):
    def su(d1, d2):
        h = np.maximum(s - np.abs(d1 - d2), f32(0))
        return np.minimum(d1, d2) - (h * h) * q

    if kind == 7:
        return np.minimum(a, b) if s == 0 else su(a, b)
    if kind == 8:
        return np.maximum(a, -b) if s == 0 else -su(-a, b)
    return np.maximum(a, b) if s == 0 else -su(-a, -b)


# the 14 distinct voxels of the 26 block test positions (atomic.rs:1700-1797)
TEST_VOXELS = [(i, j, k) for i in (0, 15) for j in (0, 15) for k in (0, 15)] + [(0, 8, 8), (15, 8, 8), (8, 0, 8), (8, 15, 8), (8, 8, 0), (8, 8, 15)]


def noise_test_points(o, dx, dy, dz):
    """(voxel, point) of the 26 test positions, reference order and f32 operation order"""
    return [
        ((0, 0, 0), o), ((15, 0, 0), o + dx * S), ((0, 15, 0), o + dy * S), ((0, 0, 15), o + dz * S),
        ((15, 15, 0), o + (dx + dy) * S), ((15, 0, 15), o + (dx + dz) * S), ((0, 15, 15), o + (dy + dz) * S),
        ((15, 15, 15), o + ((dx + dy) + dz) * S),
        ((0, 0, 0), o + dx * H), ((0, 15, 0), (o + dx * H) + dy * S), ((0, 0, 15), (o + dx * H) + dz * S),
        ((0, 15, 15), (o + dx * H) + (dy + dz) * S),
        ((0, 0, 0), o + dy * H), ((15, 0, 0), (o + dy * H) + dx * S), ((0, 0, 15), (o + dy * H) + dz * S),
        ((15, 0, 15), (o + dy * H) + (dx + dz) * S),
        ((0, 0, 0), o + dz * H), ((15, 0, 0), (o + dz * H) + dx * S), ((0, 15, 0), (o + dz * H) + dy * S),
        ((15, 15, 0), (o + dz * H) + (dx + dy) * S),
        ((0, 8, 8), (o + dy * H) + dz * H), ((15, 8, 8), ((o + dx * S) + dy * H) + dz * H),
        ((8, 0, 8), (o + dx * H) + dz * H), ((8, 15, 8), ((o + dy * S) + dx * H) + dz * H),
        ((8, 8, 0), (o + dx * H) + dy * H), ((8, 8, 15), ((o + dz * S) + dx * H) + dy * H),
    ]


# how often the noise nodes took each branch of their block test: "inside" (applied, the block meets the domain), "outside_applied" (a
# test position failed), "outside_skipped" (every test position passed)
NOISE_BRANCHES = {"inside": 0, "outside_applied": 0, "outside_skipped": 0}


def apply_noise(nd, d, o_root, blo, bhi):
    """atomic.rs:755-787: the noise is added unless the block lies outside and every test position passes"""
    m = nd["transform"]
    ns, freq0, lac = nd["a"], nd["b"], nd["c"]
    gain = nd["reserved"][0:1].view(f32)[0]
    octaves, seed = int(nd["reserved"][1]), int(nd["reserved"][2])
    on = xform_point(m, o_root)
    dx, dy, dz = m[0:3], m[4:7], m[8:11]
    inv = np.sqrt((dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2])
    sc = f32(1) / inv
    freq = freq0 * inv
    o, dxn, dyn, dzn = on * sc, dx * sc, dy * sc, dz * sc

    def fbm(p):  # dimensions reversed
        return nr.fbm3(p[..., 2], p[..., 1], p[..., 0], octaves, freq, lac, gain, seed)

    bnlo, bnhi = aabb_of_transformed(blo, bhi, m)
    if lies_outside(nd["domain_lo"], nd["domain_hi"], bnlo, bnhi):
        tests = noise_test_points(o, dxn, dyn, dzn)
        pts = np.stack([p for _, p in tests]).astype(f32)
        vals = np.array([d[v] for v, _ in tests], f32)
        if np.all(vals + fbm(pts) * ns >= nd["margin"]):
            NOISE_BRANCHES["outside_skipped"] += 1
            return d, False
        NOISE_BRANCHES["outside_applied"] += 1
    else:
        NOISE_BRANCHES["inside"] += 1
    rotated = not (abs(dx[0] * inv - f32(1)) <= f32(1e-6)) or not (abs(dy[1] * inv - f32(1)) <= f32(1e-6))
    if not rotated:
        kk = np.arange(16, dtype=f32)
        n = nr.fbm3(o[2] + kk[None, None, :], (o[1] + JJ)[..., None], (o[0] + II)[..., None], octaves, freq, lac, gain, seed)
    else:
        pos = np.empty((16, 16, 16, 3), f32)
        p = (o + II[..., None] * dxn) + JJ[..., None] * dyn
        for k in range(16):
            pos[:, :, k] = p
            p = p + dzn
        n = fbm(pos)
    return d + n * ns, True


def chunk_values(nodes, o_root):
    blo, bhi = o_root, o_root + f32(16)
    stack = []
    for nd in nodes:
        kind = int(nd["kind"])
        m = nd["transform"]
        if kind <= 2:
            bnlo, bnhi = aabb_of_transformed(blo, bhi, m)
            margin = nd["margin"]
            if lies_outside(nd["domain_lo"], nd["domain_hi"], bnlo, bnhi):
                stack.append(np.full((16, 16, 16), margin, f32))
                continue
            if kind == 0:
                e = nd["a"] * f32(0.57735026) + (-margin)
                ih = np.array([e, e, e], f32)
            elif kind == 1:
                e = nd["b"] * f32(0.57735026) + (-margin)
                ih = np.array([e, e + nd["a"], e], f32)
            else:
                ih = np.array([nd["a"] + (-margin), nd["b"] + (-margin), nd["c"] + (-margin)], f32)
            if contains_box(-ih, ih, bnlo, bnhi):
                stack.append(np.full((16, 16, 16), -margin, f32))
            else:
                stack.append(leaf_values(nd, positions(m, o_root)).astype(f32))
        elif kind == 5:
            stack[-1] = stack[-1] * nd["a"]
        elif kind == 6:
            stack[-1], _ = apply_noise(nd, stack[-1], o_root, blo, bhi)
        elif kind >= 7:
            d2 = stack.pop()
            d1 = stack[-1]
            s, q = nd["a"], nd["b"]
            bnlo, bnhi = aabb_of_transformed(blo, bhi, m)
            apply = not lies_outside(nd["domain_lo"], nd["domain_hi"], bnlo, bnhi)
            if not apply:
                idx = tuple(np.array(TEST_VOXELS).T)
                apply = not np.all(combine(kind, d1[idx], d2[idx], s, q) >= nd["margin"])
            if apply:
                stack[-1] = combine(kind, d1, d2, s, q).astype(f32)
    assert len(stack) == 1
    return stack[0]


def restated_planes(graph, voxel_type=0):
    """dense chunk-tiled sdf and type planes of the graph's voxel object (SameVoxelTypeGenerator), as the reference computes them"""
    nodes = SDFGenerator(graph).nodes
    gen = SDFVoxelGenerator(1.0, graph, voxel_type)
    shape, center, cc = gen.grid_shape(), np.asarray(gen.shifted_grid_center, f32), gen.chunk_counts()
    n_chunks = cc[0] * cc[1] * cc[2]
    sdf = np.full((n_chunks, 16, 16, 16), 127, np.int8)
    typ = np.full((n_chunks, 16, 16, 16), 255, np.uint8)
    gi0, gj0, gk0 = np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij")
    for ci in range(cc[0]):
        for cj in range(cc[1]):
            for ck in range(cc[2]):
                o = (np.array([ci * 16, cj * 16, ck * 16], f32) - center).astype(f32)
                v = chunk_values(nodes, o)
                with np.errstate(invalid="ignore"):
                    q = np.clip(np.trunc(v * f32(50)), -128, 127).astype(np.int8)
                inside = (ci * 16 + gi0 < shape[0]) & (cj * 16 + gj0 < shape[1]) & (ck * 16 + gk0 < shape[2])
                q = np.where(inside, q, np.int8(127))
                c = (ci * cc[1] + cj) * cc[2] + ck
                sdf[c] = q
                if np.any(q < 0):
                    typ[c] = voxel_type
    return cc, sdf.reshape(-1), typ.reshape(-1)
