"""Random SDF programs through the whole generate → derive → remesh → inertia → regions path (fixed seeds): trees of spheres, boxes and
capsules under translations, rotations and scalings, joined by hard and smooth unions, subtractions and intersections. The sampler's
interval pre-pass, its constant-chunk shortcuts and the LDS classes of the evaluator decide per chunk what gets evaluated; every
decision must leave the voxel bytes bit-identical to the oracle's plain per-voxel evaluation."""
import numpy as np
import pytest

import parity_util as pu
import sampler_census as sc
from impact_amd import capi
from impact_amd.sdf_graph import SDFGraph, SDFNode
from impact_amd.voxel import SDFVoxelGenerator, VoxelObject
from test_gpu_parity import full_pipeline

pytestmark = pytest.mark.gpu


def random_tree(g, rng, depth):
    if depth == 0 or rng.random() < 0.25:
        kind = rng.integers(0, 3)
        if kind == 0:
            node = g.add_node(SDFNode.new_sphere(float(rng.uniform(4.0, 22.0))))
        elif kind == 1:
            node = g.add_node(SDFNode.new_box([float(x) for x in rng.uniform(4.0, 36.0, 3)]))
        else:
            node = g.add_node(SDFNode.new_capsule(float(rng.uniform(2.0, 30.0)), float(rng.uniform(3.0, 12.0))))
    else:
        a = random_tree(g, rng, depth - 1)
        b = random_tree(g, rng, depth - 1)
        smooth = 0.0 if rng.random() < 0.5 else float(rng.uniform(0.5, 6.0))
        op = rng.choice(3, p=[0.6, 0.25, 0.15])
        node = g.add_node((SDFNode.new_union, SDFNode.new_subtraction, SDFNode.new_intersection)[op](a, b, smooth))
    if rng.random() < 0.5:
        node = g.add_node(SDFNode.new_translation(node, [float(x) for x in rng.uniform(-18.0, 18.0, 3)]))
    if rng.random() < 0.35:
        axis = rng.normal(size=3)
        node = g.add_node(SDFNode.new_rotation_from_axis_angle(node, [float(x) for x in axis / np.linalg.norm(axis)], float(rng.uniform(0, 6.28))))
    if rng.random() < 0.25:
        node = g.add_node(SDFNode.new_scaling(node, float(rng.uniform(0.6, 1.5))))
    return node


# 210, 247, 279, 341, 398, 479: the round-1 sweep's wrong-output seeds (a Scaling above a combination that the evaluator leaves
# un-applied with a constant first operand: the constant was not scaled; fixed in k_sdf_eval's OP_SCALE). 167, 362, 404: programs
# whose root domain is degenerate (an intersection of disjoint shapes) — oracle and host compile both report grid shape [0; 3]
# (generation.rs:217-225).
FORMER_FAILURES = [167, 210, 247, 279, 341, 362, 398, 404, 479]


@pytest.mark.parametrize("seed", pu.fuzz_seeds([31, 32, 33, 34, 35, 36] + FORMER_FAILURES))
def test_random_sdf_program(ctx, seed):
    rng = np.random.default_rng(seed)
    g = SDFGraph()
    random_tree(g, rng, int(rng.integers(1, 5)))
    extent = [1.0, 0.5, 0.25, 2.0][seed % 4]
    o = pu.oracle_from_graph(g, extent)
    gen = SDFVoxelGenerator(extent, g, 0)
    assert tuple(gen.chunk_counts()) == tuple(o.chunk_counts)
    if min(o.chunk_counts) == 0:  # degenerate root domain: both sides say "grid shape [0; 3]"; there is nothing to sample
        assert gen.grid_shape() == (0, 0, 0) and tuple(gen.shifted_grid_center) == (-0.5, -0.5, -0.5)
        with pytest.raises(ValueError):
            pu.gpu_from_graph(ctx, g, extent)
        return
    del o
    _, obj = full_pipeline(ctx, g, extent)
    obj.close()


# Seeds whose programs are KNOWN to reach the pre-pass's rules (a census of seeds 1000..1299 at voxel extent 1.0, tests/sampler_census.py;
# 1122, 1191, 1193, 1221 and 1245 of that range have a degenerate root domain), all on grids of at most 336 chunks. What a seed witnesses:
#   P  chunks on the `poisoned` fallback (a saturation-class drop, then a combination behind the 14-position test: the full program)
#   S  OP_SKIP ops (a first operand dropped as a mirror image or by its saturation class)
#   O  OP_COMBINE_OUTSIDE ops (a combination behind the 14-position test)
#   1  a non-empty two-level list          2  a non-empty general list (programs of stack size >= 3)
#   M  one-level and two-level lists both non-empty: the second step takes both in one launch (`merge01`)
# 1039 and 1160 have stack size 2: their poisoned chunks run the full program in the two-level class, the others' in the general class.
WITNESSED = {1024: "PSO12M", 1039: "PO1", 1041: "PSO12M", 1042: "PSO12M", 1072: "PSO12M", 1092: "PSO12M", 1093: "PSO12M", 1141: "PSO12M", 1160: "PS1M",
             1169: "PSO12M", 1195: "PSO12M", 1254: "PSO12M", 1259: "PSO12M", 1260: "PSO12M", 1261: "PSO12M", 1263: "PSO12M", 1268: "PSO12M", 1272: "PSO12M"}
assert all(sum(1 for w in WITNESSED.values() if k in w) >= 8 for k in "PSO12M")


def witnessed_program(seed):
    """(graph, generator at voxel extent 1.0) of a seed of the table"""
    rng = np.random.default_rng(seed)
    g = SDFGraph()
    random_tree(g, rng, int(rng.integers(1, 5)))
    return g, SDFVoxelGenerator(1.0, g, 0)


def resident_object(ctx, gen, ahead=False):
    obj = VoxelObject(ctx, gen.chunk_counts(), 1.0)
    obj.set_sdf_program(gen)
    obj.set_densities(np.ones(256, dtype=np.float32))
    obj.set_sample_ahead(ahead)
    return obj


def witnesses_of(cen):
    found = ""
    found += "P" if cen.poisoned_chunks else ""
    found += "S" if cen.op_total(sc.OP_SKIP) else ""
    found += "O" if cen.op_total(sc.OP_COMBINE_OUTSIDE) else ""
    found += "1" if cen.lists[1] else ""
    found += "2" if cen.lists[2] else ""
    found += "M" if cen.lists[0] and cen.lists[1] else ""
    return found


@pytest.mark.parametrize("seed", pu.fuzz_seeds(list(WITNESSED)))
def test_witnessed_seed_stepped_twice(ctx, seed):
    """a resident program stepped twice through every stage, each step against the oracle: the second runs with the remembered list
    lengths, the class gating and, where two classes have work, the merged launch"""
    g, gen = witnessed_program(seed)
    if min(gen.chunk_counts()) == 0 or int(np.prod(gen.chunk_counts())) > 2000:
        assert pu.fuzzing()  # (no committed seed is a degenerate or an oversized one)
        return
    o = pu.oracle_from_graph(g)
    o.update_occupied_voxel_ranges()
    o.compute_all_derived_state()
    obj = resident_object(ctx, gen)
    for i in range(2):
        r = obj.step(capi.STAGE_ALL)
        p = pu.step_parity(o, obj, r)
        assert p["equal"], (i, p)
    obj.close()


def test_witnessed_seeds_still_witness(ctx):
    """the census again on every seed of the table: a change to the pruning must not quietly turn them into trivial programs"""
    if pu.fuzzing():
        pytest.skip("holds for the committed seeds")
    for seed, want in WITNESSED.items():
        _, gen = witnessed_program(seed)
        assert 0 < int(np.prod(gen.chunk_counts())) <= 2000
        assert len(gen.sdf_generator.nodes) <= sc.OP_CAP  # (an OP_OVERFLOW chunk of such a program is a poisoned one)
        obj = resident_object(ctx, gen)
        obj.step(capi.STAGE_ALL)
        cen = sc.census(obj, len(gen.sdf_generator.nodes))
        assert sum(cen.lists) == obj.stage_counters()["evaluated_chunks"]
        obj.close()
        found = witnesses_of(cen)
        assert all(k in found for k in want), (seed, want, found)


def _far_first_operand_scene(s_outer, s_inner, op, smooth_top):
    """A combination whose domain is far from the chunks around its SECOND operand, under nested scalings.

    Sub/Intersection(capsule A at the origin, box B 50 voxels away): the node's domain is A's (atomic.rs:395-420), so in the
    chunks around B the reference takes the "domain lies outside the block" path: A fills +margin, B is evaluated, the 14 block
    test positions all give `>= margin`, the node is not applied and +margin stays (atomic.rs:788-806). The scalings above
    (child margin = margin / scaling, atomic.rs:546-558) must then bring that constant back to the root's 2.54 -> +127 (Void).
    A third body far along x only widens the grid so that such chunks exist."""
    g = SDFGraph()
    a = g.add_node(SDFNode.new_capsule(10.0, 5.0))
    b = g.add_node(SDFNode.new_translation(g.add_node(SDFNode.new_box([20.0, 24.0, 18.0])), [50.0, 2.0, -3.0]))
    comb = g.add_node((SDFNode.new_subtraction, SDFNode.new_intersection, SDFNode.new_union)[op](a, b, 0.0))
    inner = g.add_node(SDFNode.new_scaling(g.add_node(SDFNode.new_translation(comb, [1.5, -2.0, 0.5])), s_inner))
    other = g.add_node(SDFNode.new_scaling(g.add_node(SDFNode.new_translation(g.add_node(SDFNode.new_capsule(6.0, 4.0)), [0.0, 30.0, 0.0])), 0.8))
    both = g.add_node(SDFNode.new_union(inner, other, smooth_top))
    outer = g.add_node(SDFNode.new_scaling(both, s_outer))
    far = g.add_node(SDFNode.new_translation(g.add_node(SDFNode.new_sphere(9.0)), [150.0, 0.0, 0.0]))
    g.add_node(SDFNode.new_union(outer, far, 0.0))
    return g


@pytest.mark.parametrize("s_outer,s_inner,op,smooth_top", [(1.4, 1.3, 0, 0.0), (1.4836, 1.3553, 0, 0.0), (0.7, 1.487, 0, 2.0),
                                                             (1.25, 0.8, 1, 0.0), (1.4, 1.3, 2, 0.0)])
def test_nested_scalings_over_a_far_combination(ctx, s_outer, s_inner, op, smooth_top):
    g = _far_first_operand_scene(s_outer, s_inner, op, smooth_top)
    o, obj = full_pipeline(ctx, g, 1.0)
    # the scene must contain what it is for: Void chunks between the bodies
    info = obj.download(flags=False, labels=False)[4]
    assert (info["kind"] == 0).sum() > 0
    obj.close()


def _slab_scene(rng):
    """walls, floors and pillars: boxes under translations and scalings only (no rotation), joined by hard and smooth unions and cut by a
    box-shaped subtraction — most voxel columns lie inside some box's footprint in x and y, where the evaluator takes the length of
    (0, 0, pz) as pz (box_column_inside, csrc/sdf_sample.hip) instead of the rounded square root the reference computes"""
    g = SDFGraph()
    acc = None
    for _ in range(int(rng.integers(3, 7))):
        ext = [float(x) for x in rng.uniform(3.0, 60.0, 3)]
        ext[int(rng.integers(0, 3))] = float(rng.uniform(0.7, 6.0))  # a slab along one axis
        n = g.add_node(SDFNode.new_box(ext))
        if rng.random() < 0.5:
            n = g.add_node(SDFNode.new_scaling(n, float(rng.uniform(0.37, 1.9))))
        n = g.add_node(SDFNode.new_translation(n, [float(x) for x in rng.uniform(-25.0, 25.0, 3)]))
        acc = n if acc is None else g.add_node(SDFNode.new_union(acc, n, 0.0 if rng.random() < 0.6 else float(rng.uniform(0.5, 3.0))))
    hole = g.add_node(SDFNode.new_translation(g.add_node(SDFNode.new_box([float(x) for x in rng.uniform(2.0, 9.0, 3)])), [float(x) for x in rng.uniform(-10.0, 10.0, 3)]))
    acc = g.add_node(SDFNode.new_subtraction(acc, hole, 0.0 if rng.random() < 0.5 else 1.5))
    if rng.random() < 0.5:
        g.add_node(SDFNode.new_scaling(acc, float(rng.uniform(0.8, 1.3))))
    return g


@pytest.mark.parametrize("seed", pu.fuzz_seeds([61, 62, 63, 64, 65, 66, 67, 68]))
def test_box_built_scenes(ctx, seed):
    rng = np.random.default_rng(seed)
    g = _slab_scene(rng)
    extent = [1.0, 0.5, 0.37, 1.0 / 3.0][seed % 4]
    _, obj = full_pipeline(ctx, g, extent)
    obj.close()
