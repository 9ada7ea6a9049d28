"""Detailed drag on the device (impact_amd/csrc/drag.hip): the drag loads of triangle lists and of the resident mesh, the smoothing of
samples into the equirectangular map, and the one-call map — against the numpy float64 restatement in drag_ref.py.

Load tolerance, per direction and per component: 1e-5 S_F for the force and 1e-5 S_T for the torque, S_F = sum cos+ area and
S_T = sum cos+ area |centre - com| from the restatement (the project's 1e-5 against an f64 oracle, taken norm-wise); where the expected
load is exactly zero the result must be exactly zero."""

import numpy as np
import pytest

import drag_ref as dr
from impact_amd import capi, drag, scenes
from impact_amd.voxel import SDFVoxelGenerator, VoxelObject, VoxelObjectMesh

pytestmark = pytest.mark.gpu


def assert_loads_match(got, positions, indices, com, dirs, what):
    f, t, s_f, s_t = dr.drag_loads(positions, indices, com, dirs)
    gf, gt = got["force"].astype(np.float64), got["torque"].astype(np.float64)
    assert not np.isnan(gf).any() and not np.isnan(gt).any(), what
    ef = np.abs(gf - f) / np.maximum(s_f, 1e-300)[:, None]
    et = np.abs(gt - t) / np.maximum(s_t, 1e-300)[:, None]
    print(f"{what}: force error {ef[s_f > 0].max() if (s_f > 0).any() else 0.0:.3g} S_F, torque error {et[s_t > 0].max() if (s_t > 0).any() else 0.0:.3g} S_T")
    assert np.all(np.abs(gf - f) <= 1e-5 * s_f[:, None]), what
    assert np.all(np.abs(gt - t) <= 1e-5 * s_t[:, None]), what
    zero_f, zero_t = np.all(f == 0.0, axis=1) & (s_f == 0.0), np.all(t == 0.0, axis=1) & (s_t == 0.0)
    assert np.all(gf[zero_f] == 0.0) and np.all(gt[zero_t] == 0.0), what
    return f, t, s_f, s_t


def seeded_directions(n, seed):
    rng = np.random.default_rng(seed)
    phi, theta = rng.uniform(0.0, 2.0 * np.pi, n), rng.uniform(0.0, np.pi, n)
    d = np.stack([np.cos(phi) * np.sin(theta), np.sin(phi) * np.sin(theta), np.cos(theta)], axis=1)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def test_sphere_drag_load(ctx):
    """the reference's own test of the load (drag_load.rs:272-303): a unit UV sphere with 40 rings, |F| = 2 pi / 3 against the direction,
    no torque — with the reference's tolerances; the restatement itself is 3e-3, 1.7e-4 and 1.4e-4 off on this mesh"""
    pos, idx = dr.uv_sphere(40)
    assert idx.size == 3 * 6560
    dirs = seeded_directions(10, 7)
    com = np.zeros(3, dtype=np.float32)
    got = drag.drag_loads_for_triangles(ctx, pos, idx, com, dirs)
    assert_loads_match(got, pos, idx, com, dirs, "sphere")
    f = got["force"].astype(np.float64)
    norm = np.linalg.norm(f, axis=1)
    print(f"sphere: | |F| - 2 pi / 3 | {np.abs(norm - 2.0 * np.pi / 3.0).max():.3g}, direction {np.abs(f / norm[:, None] + dirs).max():.3g}, torque {np.abs(got['torque']).max():.3g}")
    assert np.all(np.abs(norm - 2.0 * np.pi / 3.0) <= 1e-2)
    assert np.all(np.abs(f / norm[:, None] + dirs) <= 1e-3)
    assert np.all(np.abs(got["torque"]) <= 1e-3)


def random_triangles(n_tris, n_degenerate, seed):
    """`n_tris` triangles over shared random vertices, `n_degenerate` of them with a repeated vertex"""
    rng = np.random.default_rng(seed)
    n_vertices = max(3, n_tris // 2 + 3)
    pos = (rng.normal(size=(n_vertices, 3)) * 3.0 + np.array([4.0, -2.0, 1.0])).astype(np.float32)
    idx = np.zeros((n_tris, 3), dtype=np.uint32)
    for t in range(0, n_tris, 4096):
        k = min(4096, n_tris - t)
        a = rng.integers(0, n_vertices, size=k)
        b = (a + rng.integers(1, n_vertices // 2 + 1, size=k)) % n_vertices
        c = (b + rng.integers(1, n_vertices // 2, size=k)) % n_vertices
        c = np.where((c == a) | (c == b), (np.maximum(a, b) + 1) % n_vertices, c)
        c = np.where((c == a) | (c == b), (np.maximum(a, b) + 2) % n_vertices, c)
        idx[t:t + k] = np.stack([a, b, c], axis=1)
    assert np.all((idx[:, 0] != idx[:, 1]) & (idx[:, 1] != idx[:, 2]) & (idx[:, 0] != idx[:, 2]))
    deg = rng.choice(n_tris, size=n_degenerate, replace=False)
    idx[deg, 2] = idx[deg, 0]
    return pos, idx.reshape(-1)


ONE_TRIANGLE = (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=np.float32), np.array([0, 1, 2], dtype=np.uint32))  # normal +z
_meshes = {}


def tiling_mesh(name):
    if name not in _meshes:
        _meshes[name] = {"one_facing": ONE_TRIANGLE, "one_away": ONE_TRIANGLE, "65": random_triangles(65, 0, 3), "20001": random_triangles(20001, 500, 4)}[name]
    return _meshes[name]


@pytest.mark.parametrize("n_dirs", [1, 65, 200])
@pytest.mark.parametrize("mesh", ["one_facing", "one_away", "65", "20001"])
def test_loads_where_tiling_can_go_wrong(ctx, mesh, n_dirs):
    """triangle counts 1 (facing the flow and facing away), 65 and 20 001 (500 degenerate) x direction counts 1, 65, 200, off-centre com"""
    pos, idx = tiling_mesh(mesh)
    com = np.array([0.75, -1.25, 2.5], dtype=np.float32)
    if mesh == "one_facing":  # every direction has a positive z
        dirs = seeded_directions(n_dirs, 5)
        dirs[:, 2] = np.abs(dirs[:, 2]) + np.float32(0.05)
    elif mesh == "one_away":
        dirs = seeded_directions(n_dirs, 5)
        dirs[:, 2] = -np.abs(dirs[:, 2]) - np.float32(0.05)
    else:
        dirs = dr.directions_f32(n_dirs)
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    got = drag.drag_loads_for_triangles(ctx, pos, idx, com, dirs)
    f, t, s_f, _ = assert_loads_match(got, pos, idx, com, dirs, f"{mesh} x {n_dirs}")
    if mesh == "one_facing":
        assert np.all(s_f > 0.0) and np.all(got["force"][:, 2] < 0.0)
    if mesh == "one_away":
        assert np.all(s_f == 0.0) and not got["force"].any() and not got["torque"].any()


@pytest.mark.parametrize("mesh", ["65", "20001"])
def test_loads_with_four_directions_to_a_lane(ctx, mesh):
    """from 512 directions on a lane of the load kernel holds four directions: 600 of them (no multiple of the 256 a wave then takes)"""
    pos, idx = tiling_mesh(mesh)
    com = np.array([0.75, -1.25, 2.5], dtype=np.float32)
    dirs = dr.directions_f32(600)
    got = drag.drag_loads_for_triangles(ctx, pos, idx, com, dirs)
    assert_loads_match(got, pos, idx, com, dirs, f"{mesh} x 600")
    # the same directions in the one-to-a-lane form, 200 at a time: the same sums up to the rounding of another tiling
    for lo in range(0, 600, 200):
        part = drag.drag_loads_for_triangles(ctx, pos, idx, com, dirs[lo:lo + 200])
        _, _, s_f, s_t = dr.drag_loads(pos, idx, com, dirs[lo:lo + 200])
        assert np.all(np.abs(part["force"].astype(np.float64) - got["force"][lo:lo + 200]) <= 2e-5 * s_f[:, None])
        assert np.all(np.abs(part["torque"].astype(np.float64) - got["torque"][lo:lo + 200]) <= 2e-5 * s_t[:, None])


@pytest.fixture(scope="module")
def sphere_object(ctx):
    g = VoxelObject.generate(ctx, SDFVoxelGenerator(1.0, scenes.sphere_scene(30.0)))
    yield g
    g.close()


def live_indices(idx, sub):
    return np.concatenate([idx[int(s["index_offset"]):int(s["index_offset"]) + int(s["index_count"])] for s in sub]) if len(sub) else idx[:0]


def test_resident_mesh_and_freed_ranges(ctx, sphere_object):
    g = sphere_object
    mesh = VoxelObjectMesh.create(g)
    centre = np.array([0.5 * (a + b) for a, b in g.occupied_voxel_ranges], dtype=np.float32)
    com = centre + np.array([1.5, -2.0, 0.5], dtype=np.float32)
    dirs = dr.directions_f32(65)
    pos, _, idx, _, sub = mesh.download()
    assert int(sub["index_count"].sum()) == idx.size
    assert_loads_match(drag.drag_loads_for_voxel_object(g, com, dirs), pos, idx, com, dirs, "resident sphere")
    # a bite, then the incremental sync: the buffers now hold freed ranges with stale triangles
    r = g.absorb_sphere(centre + np.array([0.0, 0.0, 30.0], dtype=np.float32), 14.0, 12.0)
    mesh.sync_with_voxel_object(r["invalidated"])
    pos, _, idx, _, sub = mesh.download()
    assert int(sub["index_count"].sum()) < idx.size
    got = drag.drag_loads_for_voxel_object(g, com, dirs)
    assert_loads_match(got, pos, live_indices(idx, sub), com, dirs, "bitten sphere, live submeshes")
    f_all, t_all, s_f, s_t = dr.drag_loads(pos, idx, com, dirs)
    off = (np.abs(got["force"] - f_all) > 1e-5 * s_f[:, None]).any() or (np.abs(got["torque"] - t_all) > 1e-5 * s_t[:, None]).any()
    assert off, "the loads match the whole index buffer, freed ranges included"


def test_one_call_map_equals_the_two_stages(ctx, sphere_object):
    """`ivx_drag_load_map` = `ivx_drag_loads` + `ivx_drag_load_map_from_samples`, byte for byte, and two calls give the same bytes"""
    g = sphere_object
    mesh = VoxelObjectMesh.create(g)
    com = np.array([30.0, 29.0, 33.0], dtype=np.float32)
    cfg = drag.DragLoadMapConfig(200, 8, 2.0)
    one = drag.DragLoadMap.compute_from_voxel_object_mesh(mesh, com, 200, 8, 2.0)
    again = drag.DragLoadMap.compute_from_voxel_object_mesh(mesh, com, 200, 8, 2.0)
    d200 = drag.uniformly_distributed_radial_directions(200)
    loads = drag.drag_loads_for_voxel_object(g, com, d200)
    two = drag.DragLoadMap.from_samples(ctx, d200, loads, 8, cfg.angular_interpolation_distance())
    assert one.loads.tobytes() == again.loads.tobytes()
    assert one.loads.tobytes() == two.loads.tobytes()
    assert np.abs(one.loads["force"]).max() > 0.0
    pi, ti = one.indices(0.3, 1.1)
    assert one.value(0.3, 1.1).tobytes() == one.loads[ti, pi].tobytes()
    # the triangle-list form of the map over the downloaded mesh: the same map up to the rounding of another tiling
    pos, _, idx, _, _ = mesh.download()
    listed = drag.DragLoadMap.compute_from_mesh(ctx, pos, idx, com, 200, 8, 2.0)
    _, _, s_f, s_t = dr.drag_loads(pos, idx, com, d200)
    assert np.abs(listed.loads["force"].astype(np.float64) - one.loads["force"]).max() <= 2e-5 * s_f.max()
    assert np.abs(listed.loads["torque"].astype(np.float64) - one.loads["torque"]).max() <= 2e-5 * s_t.max()


def synthetic_samples(n):
    dirs = drag.uniformly_distributed_radial_directions(n)
    loads = np.zeros(n, dtype=capi.DRAG_LOAD_DTYPE)
    loads["force"], loads["torque"] = dirs, -dirs
    return dirs, loads


def map_against_restatement(ctx, n, n_theta, smoothness, mask_delta):
    dirs, loads = synthetic_samples(n)
    distance = drag.DragLoadMapConfig(n, n_theta, smoothness).angular_interpolation_distance()
    got = drag.DragLoadMap.from_samples(ctx, dirs, loads, n_theta, distance).loads
    got6 = np.concatenate([got["force"], got["torque"]], axis=2).astype(np.float64)
    want, mask = dr.map_from_samples(dirs, np.concatenate([loads["force"], loads["torque"]], axis=1), n_theta, distance, mask_delta)
    scale = float(np.abs(np.concatenate([loads["force"], loads["torque"]], axis=1)).max())
    err = np.abs(got6 - want).max(axis=2) / scale
    assert not np.isnan(got6).any()
    return err, mask


@pytest.mark.parametrize("n,n_theta,smoothness", [(200, 8, 2.0), (777, 16, 1.5), (50, 64, 1.0)])
def test_map_stage(ctx, n, n_theta, smoothness):
    """every cell within 1e-5 max|load| of the restatement (a numpy-f32 twin of the formulas is 3.5e-7 and 4.8e-7 off on the first two); no
    cell of these maps is decided within rounding, so none is left out. The third has few samples with wide regions: six of them are more
    than 64 cells across (up to 82), which the map kernel walks in its general form."""
    err, mask = map_against_restatement(ctx, n, n_theta, smoothness, 3e-4)
    print(f"map ({n}, {n_theta}, {smoothness}): max error {err.max():.3g} of the load scale, masked {mask.mean():.3%}")
    assert not mask.any()
    assert np.all(err <= 1e-5)


def test_map_stage_default_configuration(ctx):
    """(5000, 64, 2.0): the same tolerance; cells whose index assignment is decided within 3e-4 of a cell may be left out — fewer than 10 %"""
    err, mask = map_against_restatement(ctx, 5000, 64, 2.0, 3e-4)
    print(f"map (5000, 64, 2.0): max error outside the mask {err[~mask].max():.3g}, inside {err[mask].max():.3g}, masked {mask.mean():.3%}")
    assert mask.mean() <= 0.10
    assert np.all(err[~mask] <= 1e-5)


def test_no_triangles_is_not_an_error(ctx):
    dirs = dr.directions_f32(65)
    com = np.zeros(3, dtype=np.float32)
    got = drag.drag_loads_for_triangles(ctx, np.zeros((0, 3), np.float32), np.zeros(0, np.uint32), com, dirs)
    assert got.shape == (65,) and not got["force"].any() and not got["torque"].any()
    # an object eaten whole: no live submesh is left, the buffers still hold its old triangles
    g = VoxelObject.generate(ctx, SDFVoxelGenerator(1.0, scenes.sphere_scene(10.0)))
    mesh = VoxelObjectMesh.create(g)
    centre = np.array([0.5 * (a + b) for a, b in g.occupied_voxel_ranges], dtype=np.float32)
    r = g.absorb_sphere(centre, 22.0, 20.0)
    mesh.sync_with_voxel_object(r["invalidated"])
    assert mesh.n_chunks() == 0
    got = drag.drag_loads_for_voxel_object(g, centre, dirs)
    assert not got["force"].any() and not got["torque"].any()
    m = drag.DragLoadMap.compute_from_voxel_object_mesh(mesh, centre, 200, 8, 2.0)
    assert m.loads.shape == (8, 16) and not m.loads["force"].any() and not m.loads["torque"].any()
    # ... and a mesh made from nothing at all
    mesh.recreate()
    assert mesh.n_indices() == 0
    got = drag.drag_loads_for_voxel_object(g, centre, dirs)
    assert not got["force"].any() and not got["torque"].any()
    m = drag.DragLoadMap.compute_from_voxel_object_mesh(mesh, centre, 200, 8, 2.0)
    assert not m.loads["force"].any() and not m.loads["torque"].any()
    g.close()


def test_state_and_argument_errors(ctx, sphere_object):
    L = capi.lib()
    p = capi.ptr
    dirs = dr.directions_f32(4)
    com = np.zeros(3, dtype=np.float32)
    out = np.zeros(4, dtype=capi.DRAG_LOAD_DTYPE)
    m = np.zeros((8, 16), dtype=capi.DRAG_LOAD_DTYPE)
    cfg = drag.DragLoadMapConfig(200, 8, 2.0)

    def expect(rc, code):
        assert rc == code
        assert len(L.ivx_last_error()) > 0

    # never meshed
    fresh = VoxelObject.generate(ctx, SDFVoxelGenerator(1.0, scenes.box_scene()))
    expect(L.ivx_drag_loads(fresh.h, p(com), p(dirs), 4, p(out)), capi.IVX_ERR_STATE)
    expect(L.ivx_drag_load_map(fresh.h, p(com), p(cfg.as_record()), p(m)), capi.IVX_ERR_STATE)
    with pytest.raises(capi.IvxError):
        drag.drag_loads_for_voxel_object(fresh, com, dirs)
    fresh.close()
    g = sphere_object
    VoxelObjectMesh.create(g)
    pos, idx = ONE_TRIANGLE
    expect(L.ivx_drag_loads(g.h, p(com), p(dirs), 0, p(out)), capi.IVX_ERR_INVALID)
    expect(L.ivx_drag_loads_triangles(ctx.h, p(pos), 3, p(idx), 3, p(com), p(dirs), 0, p(out)), capi.IVX_ERR_INVALID)
    expect(L.ivx_drag_loads_triangles(ctx.h, p(pos), 3, p(idx), 2, p(com), p(dirs), 4, p(out)), capi.IVX_ERR_INVALID)
    bad = np.array([0, 1, 3], dtype=np.uint32)
    expect(L.ivx_drag_loads_triangles(ctx.h, p(pos), 3, p(bad), 3, p(com), p(dirs), 4, p(out)), capi.IVX_ERR_INVALID)
    for n, n_theta, smoothness in ((0, 8, 2.0), (200, 0, 2.0), (200, 8, 0.0), (200, 8, -1.0)):
        expect(L.ivx_drag_load_map(g.h, p(com), p(drag.DragLoadMapConfig(n, n_theta, smoothness).as_record()), p(m)), capi.IVX_ERR_INVALID)
    expect(L.ivx_drag_load_map_from_samples(ctx.h, p(dirs), p(out), 0, 8, 0.5, p(m)), capi.IVX_ERR_INVALID)
    expect(L.ivx_drag_load_map_from_samples(ctx.h, p(dirs), p(out), 4, 0, 0.5, p(m)), capi.IVX_ERR_INVALID)
    expect(L.ivx_drag_load_map_from_samples(ctx.h, p(dirs), p(out), 4, 8, 0.0, p(m)), capi.IVX_ERR_INVALID)
    expect(L.ivx_drag_load_map_from_samples(ctx.h, p(dirs), p(out), 4, 8, -0.5, p(m)), capi.IVX_ERR_INVALID)
    # the calls above changed nothing: the object still answers
    assert np.abs(drag.drag_loads_for_voxel_object(g, com, dirs)["force"]).max() > 0.0
