"""The step's derive sweep one chunk per wave (k_derive_wave): sampled grids with a one-region chunk whose flood does not settle within
IVX_DERIVE_FLOOD_CAP rounds (it takes the multi-region list and the exact numbering instead of the direct path), chunks with several
regions (some touching only along an edge or at a corner), material on every face of the grid, and non-integer densities. Each case is
compared with the oracle, and bit for bit with the workgroup form of the sweep (k_derive_signs_many, which a `_many` step of the same grid
runs). Which chunks need more rounds than the cap is settled by a model of the kernel's flood over the oracle's voxels (`flood_rounds`)."""
import numpy as np
import pytest

import parity_util as pu
from impact_amd import capi, many, scenes
from impact_amd.sdf_graph import SDFGraph, SDFNode
from impact_amd.voxel import SDFVoxelGenerator, VoxelObject

pytestmark = pytest.mark.gpu

NO_SAMPLE = capi.STAGE_ALL & ~capi.STAGE_SAMPLE


def _box(g, extents, at):
    return g.add_node(SDFNode.new_translation(g.add_node(SDFNode.new_box(extents)), at))


def _union_all(g, ids):
    acc = ids[0]
    for i in ids[1:]:
        acc = g.add_node(SDFNode.new_union(acc, i, 0.0))
    return acc


FLOOD_CAP = 32  # IVX_DERIVE_FLOOD_CAP's default (derive.hip)


def serpentine_scene():
    """A bar one voxel thick that winds back and forth along x in one chunk (seven bars, one-voxel gaps): one region, whose flood takes
    about twice the cap's rounds, and no line of the chunk is one run of rows (the slab test does not settle it)."""
    g = SDFGraph()
    parts = []
    n, pitch, length = 7, 2.0, 12.0
    for b in range(n):
        y = pitch * (b - 0.5 * (n - 1))
        parts.append(_box(g, (length + 1.0, 1.0, 1.0), (0.0, y, 0.0)))
        if b + 1 < n:
            parts.append(_box(g, (1.0, pitch + 1.0, 1.0), (0.5 * length if b % 2 == 0 else -0.5 * length, y + 0.5 * pitch, 0.0)))
    _union_all(g, parts)
    return g


def flood_rounds(m):
    """The rounds k_derive_wave's flood (ivx_flood_connected) takes over one chunk's 16 x 16 row masks `m[i, j]` (bit k = voxel k non-empty)
    to reach every voxel, or None when it settles short of that. The same seed (the first non-empty lane from lane 40 on, lane l holding
    rows i = 4 (l >> 4) + q, j = l & 15; its first non-empty row, lowest voxel), one step along i and j per round, runs along k filled."""
    m = m.astype(np.int64)
    rev = np.array([int(f"{v:016b}"[::-1], 2) for v in range(1 << 16)], np.int64)

    def fill_up(mm, x):
        return mm & (((mm + x) ^ mm) | x) & 0xFFFF

    def fill(x):
        x = x & m
        return fill_up(m, x) | rev[fill_up(rev[m], rev[x])]

    seed = min((l for l in range(64) if any(m[4 * (l >> 4) + q, l & 15] for q in range(4))), key=lambda l: (l - 40) % 64)
    f = np.zeros_like(m)
    for q in range(4):
        v = int(m[4 * (seed >> 4) + q, seed & 15])
        if v:
            f[4 * (seed >> 4) + q, seed & 15] = v & -v
            break
    for r in range(1, 4096):
        g = f.copy()
        g[:, 1:] |= f[:, :-1]
        g[:, :-1] |= f[:, 1:]
        g[1:, :] |= f[:-1, :]
        g[:-1, :] |= f[1:, :]
        n = fill(g)
        if (n == m).all():
            return r
        if (n == f).all():
            return None
        f = n
    return None


def oracle_row_masks(o):
    """chunk records and the 16 x 16 row masks of every chunk, from the oracle's flags"""
    _, _, flg, _, info = o.export_dense()
    ne = (flg.reshape(len(info), 16, 16, 16) & 1) == 0
    return info, (ne.astype(np.int64) << np.arange(16)).sum(axis=3)


def many_regions_scene():
    """Small spheres spaced inside a chunk (many regions each), and two cubes that meet only along an edge (two regions that touch
    diagonally), and two that meet only at a corner."""
    g = SDFGraph()
    parts = [g.add_node(SDFNode.new_translation(g.add_node(SDFNode.new_sphere(1.2)), (4.0 * x, 4.0 * y, 4.0 * z)))
             for x in range(4) for y in range(3) for z in range(2)]
    parts.append(_box(g, (4.0, 4.0, 4.0), (20.0, 0.0, 0.0)))
    parts.append(_box(g, (4.0, 4.0, 4.0), (24.0, 4.0, 0.0)))
    parts.append(_box(g, (4.0, 4.0, 4.0), (20.0, 12.0, 0.0)))
    parts.append(_box(g, (4.0, 4.0, 4.0), (24.0, 16.0, 4.0)))
    _union_all(g, parts)
    return g


def hollow_sphere_scene():
    """A thick hollow sphere with a box cut out: Void chunks inside and outside, surfaces facing both ways."""
    g = SDFGraph()
    shell = g.add_node(SDFNode.new_subtraction(g.add_node(SDFNode.new_sphere(44.0)), g.add_node(SDFNode.new_sphere(14.0)), 0.0))
    g.add_node(SDFNode.new_subtraction(shell, _box(g, (20.0, 20.0, 100.0), (30.0, 0.0, 0.0)), 0.0))
    return g


def face_box_scene():
    """A box that fills its grid but for the border: material on all six faces of the grid, in a grid that is not a cube."""
    return scenes.box_scene((29.0, 61.0, 45.0))


SCENES = {
    "serpentine": serpentine_scene,
    "many_regions": many_regions_scene,
    "hollow_sphere": hollow_sphere_scene,
    "grid_faces": face_box_scene,
    "asteroid": lambda: scenes.asteroid_scene(0.5),
}


def sampled(ctx, graph, dens):
    gen = SDFVoxelGenerator(1.0, graph, 0)
    obj = VoxelObject(ctx, gen.chunk_counts(), 1.0)
    obj.set_sdf_program(gen)
    obj.set_densities(dens)
    return obj


def densities(kind):
    if kind == "ones":
        return np.ones(256, dtype=np.float32)
    return np.random.default_rng(5).uniform(0.3, 7.9, 256).astype(np.float32)


@pytest.mark.parametrize("dens_kind", ["ones", "fractional"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_wave_sweep_against_oracle_and_workgroup_form(ctx, name, dens_kind):
    graph = SCENES[name]()
    dens = densities(dens_kind)
    o = pu.oracle_from_graph(graph)
    o.update_occupied_voxel_ranges()
    o.compute_all_derived_state()
    # the wave form: the object's own step, twice (the second starts from the first one's list)
    a = sampled(ctx, graph, dens)
    for _ in range(2):
        ra = a.step(capi.STAGE_ALL)
        p = pu.step_parity(o, a, ra, densities=dens)
        assert p["equal"], (name, p)
    # the workgroup form: a `_many` step of the same grid beside another one
    b = sampled(ctx, graph, dens)
    b.step(capi.STAGE_ALL)
    other = sampled(ctx, scenes.box_scene(), dens)
    other.step(capi.STAGE_ALL)
    rb = many.voxel_step_many([b, other], NO_SAMPLE)[0]
    ra = a.step(NO_SAMPLE)
    for x, y in zip(a.download(), b.download()):
        assert np.array_equal(np.asarray(x), np.asarray(y)), name
    assert int(ra["region_count"]) == int(rb["region_count"])
    assert np.array_equal(np.asarray(ra["moments"]["m64"]), np.asarray(rb["moments"]["m64"])), name
    assert (int(ra["mesh"]["n_vertices"]), int(ra["mesh"]["n_indices"])) == (int(rb["mesh"]["n_vertices"]), int(rb["mesh"]["n_indices"]))
    if name == "many_regions":
        assert int(ra["region_count"]) > 20
    for obj in (a, b, other):
        obj.close()


def test_serpentine_takes_the_multi_region_list(ctx):
    """The serpentine's chunk is one region whose flood needs more rounds than the cap (and is not settled by the slab test: some line i
    holds several runs of rows j), so the sweep lists it for the exact numbering; what the step leaves is the oracle's and the direct
    path's: one region, label 0 on every non-empty voxel, the boundary count."""
    graph = serpentine_scene()
    o = pu.oracle_from_graph(graph)
    o.update_occupied_voxel_ranges()
    o.compute_all_derived_state()
    info, masks = oracle_row_masks(o)
    assert len(info) == 1 and int(info["kind"][0]) == 2 and int(info["region_count"][0]) == 1
    lines = (masks[0] != 0)
    assert any(int(((row[1:] & ~row[:-1]).sum()) + int(row[0])) > 1 for row in lines)  # (several runs of rows j in some line i)
    rounds = flood_rounds(masks[0])
    assert rounds is not None and rounds > FLOOD_CAP, rounds
    a = sampled(ctx, graph, densities("ones"))
    r = a.step(capi.STAGE_ALL)
    p = pu.step_parity(o, a, r)
    assert p["equal"], p
    _, _, _, lab, ginfo = a.download()
    assert int(ginfo["region_count"][0]) == 1 and int(ginfo["boundary_region_count"][0]) == int(info["boundary_region_count"][0])
    assert set(np.unique(lab).tolist()) <= {0, 255}
    a.close()


def test_flood_model_on_the_scenes():
    """(no GPU needed for the model itself) every one-region chunk of the other scenes settles within the cap from the middle seed, so
    the multi-region list gets only chunks with several regions there"""
    for name in ("many_regions", "hollow_sphere", "grid_faces", "asteroid"):
        o = pu.oracle_from_graph(SCENES[name]())
        o.update_occupied_voxel_ranges()
        o.compute_all_derived_state()
        info, masks = oracle_row_masks(o)
        for c in np.nonzero((info["kind"] == 2) & (info["gen_kind"] == 2) & (info["region_count"] == 1))[0]:
            if masks[c].any() and not (masks[c] == 0xFFFF).all():
                r = flood_rounds(masks[c])
                assert r is not None and r <= FLOOD_CAP, (name, int(c), r)
