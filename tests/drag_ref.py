"""numpy float64 restatement of the detailed-drag formulas (the load of a direction, the smoothing of the samples into an equirectangular
map, the force on a body), written from the formulas as include/impact_voxel_hip.h states them. Inputs that the library takes in f32
(directions, vertex positions, the interpolation distance) are taken as those f32 values; everything else is f64."""
import numpy as np

F32_EPS = float(np.finfo(np.float32).eps)
TWO_PI = 2.0 * np.pi


def directions_f32(n):
    """the direction formula in numpy f32, operation by operation: z = 1 - 2 i / (n - 1), r = sqrt(1 - z z), azimuth i pi (3 - sqrt 5)"""
    f = np.float32
    i = np.arange(n, dtype=np.float32)
    idx_norm = f(1.0) / (f(n - 1) if n > 1 else f(1.0))
    golden = f(np.pi) * (f(3.0) - np.sqrt(f(5.0)))
    z = f(1.0) - f(2.0) * i * idx_norm
    r = np.sqrt(np.maximum(f(0.0), f(1.0) - z * z))
    az = i * golden
    v = np.stack([r * np.cos(az), r * np.sin(az), z], axis=1).astype(np.float32)
    norm = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    return (v / norm[:, None]).astype(np.float32)


def triangle_properties(positions, indices):
    """(normal [T,3], area [T], centre [T,3]) of the triangles with |e1 x e2| > f32::EPSILON"""
    P = np.asarray(positions, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    tri = np.asarray(indices).astype(np.int64).reshape(-1, 3)
    v1, v2, v3 = P[tri[:, 0]], P[tri[:, 1]], P[tri[:, 2]]
    c = np.cross(v2 - v1, v3 - v1)
    ln = np.linalg.norm(c, axis=1)
    keep = ln > F32_EPS
    c, ln = c[keep], ln[keep]
    return c / ln[:, None], 0.5 * ln, ((v1 + v2 + v3) / 3.0)[keep]


def drag_loads(positions, indices, com, dirs):
    """force [D,3], torque [D,3] and the scales S_F = sum cos+ area, S_T = sum cos+ area |centre - com| per direction"""
    normal, area, centre = triangle_properties(positions, indices)
    d = np.asarray(dirs, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    arm = centre - np.asarray(com, dtype=np.float32).astype(np.float64)
    arm_x_n = np.cross(arm, normal)
    force, torque = np.zeros((d.shape[0], 3)), np.zeros((d.shape[0], 3))
    s_f, s_t = np.zeros(d.shape[0]), np.zeros(d.shape[0])
    arm_len = np.linalg.norm(arm, axis=1)
    for lo in range(0, d.shape[0], 64):  # (blocks of directions bound the [D, T] intermediate)
        w = np.maximum(d[lo:lo + 64] @ normal.T, 0.0) * area[None, :]
        force[lo:lo + 64] = -(w @ normal)
        torque[lo:lo + 64] = -(w @ arm_x_n)
        s_f[lo:lo + 64] = w.sum(axis=1)
        s_t[lo:lo + 64] = w @ arm_len
    return force, torque, s_f, s_t


def rem_euclid(a, m):
    r = np.fmod(a, m)
    return np.where(r < 0.0, r + m, r)


def folded_theta(theta):
    t = rem_euclid(theta, TWO_PI)
    return np.where(t > np.pi, TWO_PI - t, t)


def phi_index(phi, n_theta):
    return np.minimum(2 * n_theta - 1, np.floor(rem_euclid(phi, TWO_PI) * (n_theta / np.pi)).astype(np.int64))


def theta_index(theta, n_theta):
    return np.minimum(n_theta - 1, np.floor(folded_theta(theta) * (n_theta / np.pi)).astype(np.int64))


def _near_integer(x, delta):
    return np.abs(x - np.round(x)) < delta


def map_from_samples(dirs, loads6, n_theta, distance, mask_delta=None):
    """The smoothing stage: returns map [n_theta, 2 n_theta, 6]; with `mask_delta` (in units of a cell) also the boolean mask of the cells whose
    index assignment is decided within that margin: a sample whose 2 ext / cell lies within it of an integer marks its region under both
    counts; a row (column) whose folded angle over the cell size lies within it of an integer marks that index and both its neighbours
    across all columns (rows) of the region — phi wraps, theta is clipped."""
    d = np.asarray(dirs, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    loads6 = np.asarray(loads6, dtype=np.float64).reshape(-1, 6)
    distance = float(np.float32(distance))
    n_phi = 2 * n_theta
    cell = np.pi / n_theta
    half = 0.5 * cell
    acc = np.zeros((n_theta, n_phi, 6))
    wsum = np.zeros((n_theta, n_phi))
    mask = np.zeros((n_theta, n_phi), dtype=bool)
    for s in range(d.shape[0]):
        phi_s = np.arctan2(d[s, 1], d[s, 0])
        theta_s = np.arccos(np.clip(d[s, 2], -1.0, 1.0))
        scaled = distance / (1.0 - 0.75 * abs(d[s, 2]))
        ext = max(half, scaled)
        q = 2.0 * ext / cell
        counts = [int(np.ceil(q))]
        if mask_delta is not None and _near_integer(q, mask_delta):
            counts = [int(np.round(q)), int(np.round(q)) + 1]
        for n_across in counts:
            k = np.arange(n_across, dtype=np.float64)
            th = theta_s - ext + half + k * cell
            ph = phi_s - ext + half + k * cell
            ti, pi = theta_index(th, n_theta), phi_index(ph, n_theta)
            if mask_delta is not None:
                if len(counts) == 2:
                    mask[np.ix_(ti, pi)] = True
                rows = ti[_near_integer(folded_theta(th) / cell, mask_delta)]
                cols = pi[_near_integer(rem_euclid(ph, TWO_PI) / cell, mask_delta)]
                for o in (-1, 0, 1):
                    mask[np.ix_(np.clip(rows + o, 0, n_theta - 1), pi)] = True
                    mask[np.ix_(ti, (cols + o) % n_phi)] = True
            if n_across != int(np.ceil(q)):
                continue  # (only the count the formula gives is accumulated)
            arg = np.sin(theta_s) * np.sin(th)[:, None] + np.cos(theta_s) * np.cos(th)[:, None] * np.cos(ph - phi_s)[None, :]
            x = np.arccos(np.clip(arg, -1.0, 1.0)) / scaled
            w = np.maximum(0.0, 1.0 - x * x) ** 2
            np.add.at(wsum, (ti[:, None], pi[None, :]), w)
            np.add.at(acc, (ti[:, None], pi[None, :]), w[:, :, None] * loads6[s][None, None, :])
    out = np.where(wsum[:, :, None] > 0.0, acc / np.where(wsum > 0.0, wsum, 1.0)[:, :, None], acc)
    return (out, mask) if mask_delta is not None else out


def rotate(q_xyzw, v):
    q = np.asarray(q_xyzw, dtype=np.float64)
    u, w = q[:3], q[3]
    v = np.asarray(v, dtype=np.float64)
    return v + 2.0 * w * np.cross(u, v) + 2.0 * np.cross(u, np.cross(u, v))


def body_space_direction(body, medium_velocity):
    """(unit body-space direction of the body's velocity relative to the medium, squared relative speed), f64 from the record's f32 fields"""
    v_rel = np.asarray(body["momentum"], dtype=np.float64) / float(body["mass"]) - np.asarray(medium_velocity, dtype=np.float64)
    s2 = float(v_rel @ v_rel)
    q = np.asarray(body["orientation"], dtype=np.float64)
    return rotate(np.array([-q[0], -q[1], -q[2], q[3]]), v_rel) / np.sqrt(s2), s2


def force_and_torque(map_loads, body, medium_velocity, density, drag_coefficient, scaling):
    """world-space (force, torque) the drag adds to the body; `map_loads` [n_theta, 2 n_theta] records with force / torque"""
    n_theta = map_loads.shape[0]
    d, s2 = body_space_direction(body, medium_velocity)
    phi, theta = np.arctan2(d[1], d[0]), np.arccos(np.clip(d[2], -1.0, 1.0))
    load = map_loads[int(theta_index(theta, n_theta)), int(phi_index(phi, n_theta))]
    fs = scaling * scaling * density * drag_coefficient * s2
    q = np.asarray(body["orientation"], dtype=np.float64)
    return fs * rotate(q, load["force"]), scaling * fs * rotate(q, load["torque"])


def uv_sphere(n_rings):
    """unit sphere with `n_rings` latitude rings of 2 n_rings + 2 vertices between two pole vertices, outward-facing triangles:
    2 (2 n_rings + 2) n_rings triangles (40 rings: 6 560)"""
    n_c = 2 * n_rings + 2
    theta = (np.arange(n_rings) + 1.0) * np.pi / (n_rings + 1)
    phi = np.arange(n_c) * TWO_PI / n_c
    ring = np.stack([np.outer(np.sin(theta), np.cos(phi)), np.outer(np.cos(theta), np.ones(n_c)), np.outer(np.sin(theta), np.sin(phi))], axis=2)
    pos = np.concatenate([[[0.0, 1.0, 0.0], [0.0, -1.0, 0.0]], ring.reshape(-1, 3)]).astype(np.float32)
    at = lambda r, j: 2 + r * n_c + (j % n_c)
    tris = []
    for j in range(n_c):
        tris.append((0, at(0, j), at(0, j + 1)))
        tris.append((1, at(n_rings - 1, j + 1), at(n_rings - 1, j)))
        for r in range(n_rings - 1):
            tris.append((at(r, j), at(r + 1, j), at(r + 1, j + 1)))
            tris.append((at(r, j), at(r + 1, j + 1), at(r, j + 1)))
    idx = np.asarray(tris, dtype=np.uint32)
    # outward: flip whatever faces inward
    P = pos.astype(np.float64)
    n = np.cross(P[idx[:, 1]] - P[idx[:, 0]], P[idx[:, 2]] - P[idx[:, 0]])
    inward = np.einsum("ij,ij->i", n, P[idx].mean(axis=1)) < 0.0
    idx[inward] = idx[inward][:, [0, 2, 1]]
    return pos, idx.reshape(-1)
