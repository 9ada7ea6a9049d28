"""The sampler's paths that only a LONG program reaches, each witnessed through the census (tests/sampler_census.py) and then held to the
oracle over two consecutive steps of a resident program (the second runs with the remembered list lengths and class gating):

  * compact per-chunk programs around the evaluator's register rounds: op i sits in lane i & 63 of one of two rounds, so 63, 64 and 65 ops
    straddle the first round's end, 127 and 128 (OP_CAP, the exact fit) the second's, and one op more overflows to the full program;
  * node programs around SUPER_MAX_WORDS * 32 = 2048 nodes: up to there the pre-pass builds the super-block far bits and skip table itself
    (`fused_super`), beyond it k_sdf_super does, hosts the step's presets, and the pre-pass reads both tables from global memory.

The scenes that fill one chunk's program are lattices of small spheres inside a single chunk under hard unions: every leaf's surface lies
in the chunk, nothing is an identity, a mirror or a saturation drop, and a left-deep chain of K leaves leaves the chunk 2K - 1 ops."""
import numpy as np
import pytest

import parity_util as pu
import sampler_census as sc
from impact_amd import capi
from impact_amd.sdf_graph import SDFGraph, SDFNode
from impact_amd.voxel import SDFVoxelGenerator, VoxelObject

pytestmark = pytest.mark.gpu
ONES = np.ones(256, dtype=np.float32)


def oracle_of(graph):
    o = pu.oracle_from_graph(graph)
    o.update_occupied_voxel_ranges()
    o.compute_all_derived_state()
    return o


def resident(ctx, gen, ahead=False):
    obj = VoxelObject(ctx, gen.chunk_counts(), 1.0)
    obj.set_sdf_program(gen)
    obj.set_densities(ONES)
    obj.set_sample_ahead(ahead)
    return obj


def assert_step(o, obj, stages=capi.STAGE_ALL, what=""):
    r = obj.step(stages)
    p = pu.step_parity(o, obj, r)
    assert p["equal"], (what, p)
    return r


# ---- many live leaves in one chunk --------------------------------------------------------------------------------------------------
LATTICE = (5, 4, 4)  # positions of the cluster, x fastest
PITCH, RADIUS = 2.6, 1.0


def cluster_centres(k):
    assert k <= LATTICE[0] * LATTICE[1] * LATTICE[2]
    return [(PITCH * (i % LATTICE[0]), PITCH * ((i // LATTICE[0]) % LATTICE[1]), PITCH * (i // (LATTICE[0] * LATTICE[1]))) for i in range(k)]


def small_sphere(g, c):
    return g.add_node(SDFNode.new_translation(g.add_node(SDFNode.new_sphere(RADIUS)), [float(x) for x in c]))


def chain_cluster(k, root_scaling=None):
    """K small spheres under hard unions in a left-deep chain (stack size 2), optionally under a root Scaling"""
    g = SDFGraph()
    acc = None
    for c in cluster_centres(k):
        s = small_sphere(g, c)
        acc = s if acc is None else g.add_node(SDFNode.new_union(acc, s, 0.0))
    if root_scaling is not None:
        g.add_node(SDFNode.new_scaling(acc, root_scaling))
    return g


def balanced_cluster(k, seed):
    """K small spheres under a balanced union tree; about a third of the unions smooth"""
    rng = np.random.default_rng(seed)
    g = SDFGraph()

    def build(cs):
        if len(cs) == 1:
            return small_sphere(g, cs[0])
        half = 1 << ((len(cs) - 1).bit_length() - 1)  # (a full tree first: 80 leaves = 64 + 16 need the seven levels that 64 need)
        a, b = build(cs[:half]), build(cs[half:])
        return g.add_node(SDFNode.new_union(a, b, float(rng.uniform(2.0, 4.0)) if rng.random() < 1.0 / 3.0 else 0.0))

    build(cluster_centres(k))
    return g


def cluster_all_in_one_chunk(gen, k, scaling=1.0):
    """every sphere's centre, in voxel coordinates of the generator's grid, lies inside the voxels of ONE chunk"""
    v = np.array(cluster_centres(k), dtype=np.float64) * scaling + np.asarray(gen.shifted_grid_center, dtype=np.float64)
    ch = np.floor(v / 16.0)
    return bool(np.all(ch == ch[0]) and np.all(v - 16.0 * ch <= 15.0))


def stepped_twice_with_census(ctx, graph, check):
    """first step, `check(census, generator)`, then the bytes of two consecutive steps against the oracle"""
    gen = SDFVoxelGenerator(1.0, graph, 0)
    o = oracle_of(graph)
    obj = resident(ctx, gen)
    r = obj.step(capi.STAGE_ALL)
    cen = sc.census(obj, len(gen.sdf_generator.nodes))
    print("census:", len(gen.sdf_generator.nodes), "nodes, stack", gen.sdf_generator.required_forward_stack_size, "chunks", gen.chunk_counts(), "lists", cen.counters,
          "max prog_len", cen.max_prog_len(), "full", cen.overflow_chunks)
    check(cen, gen)
    p = pu.step_parity(o, obj, r)
    assert p["equal"], (0, p)
    assert_step(o, obj, what=1)
    assert obj.stage_counters()["evaluated_chunks"] == sum(cen.lists)
    obj.close()


# (K spheres, root Scaling or None) -> the longest compact program: 2K - 1 ops, one more under the Scaling
@pytest.mark.parametrize("k,root_scaling,want", [(32, None, 63), (32, 1.1, 64), (33, None, 65), (64, None, 127), (64, 1.1, 128)])
def test_left_deep_chain_fills_the_register_rounds(ctx, k, root_scaling, want):
    """the chunk that holds the whole cluster gets a compact program of exactly `want` ops; every combination is applied to a bare leaf from
    registers, so the program needs one LDS level and runs in the one-level class, on the long end of its list"""
    graph = chain_cluster(k, root_scaling)

    def check(cen, gen):
        assert gen.sdf_generator.required_forward_stack_size == 2
        assert cluster_all_in_one_chunk(gen, k, root_scaling or 1.0)
        assert cen.overflow_chunks == 0
        assert cen.max_prog_len() == want
        top = [c for c in cen.chunks if c.prog_len == want]
        assert len(top) == 1 and top[0].on_list == "0 long", top
        assert top[0].hist[sc.OP_LEAF] == k and top[0].hist[sc.OP_COMBINE] == k - 1 and top[0].hist[sc.OP_SCALE] == (0 if root_scaling is None else 1)

    stepped_twice_with_census(ctx, graph, check)


def test_left_deep_chain_overflows_by_length(ctx):
    """65 leaves: 129 ops do not fit OP_CAP; the chunk runs the FULL program (195 nodes, stack 2) in the two-level class"""
    k = 65
    graph = chain_cluster(k)

    def check(cen, gen):
        assert len(gen.sdf_generator.nodes) == 3 * k - 1 and gen.sdf_generator.required_forward_stack_size == 2
        assert cluster_all_in_one_chunk(gen, k)
        assert cen.overflow_is_poisoned is None  # (more than OP_CAP nodes: the length can do it)
        full = [c for c in cen.chunks if c.prog_len is None]
        assert len(full) == 1 and full[0].on_list == "1", full
        assert cen.max_prog_len() < sc.OP_CAP  # (the other chunks see a part of the cluster)

    stepped_twice_with_census(ctx, graph, check)


def test_balanced_tree_long_program_in_the_general_class(ctx):
    """64 leaves under a balanced tree: 127 ops again, but six operands wait on levels of their own — the general class k_sdf_eval<0>"""
    k = 64
    graph = balanced_cluster(k, 5)

    def check(cen, gen):
        assert gen.sdf_generator.required_forward_stack_size == 7
        assert cluster_all_in_one_chunk(gen, k)
        assert cen.overflow_chunks == 0
        assert cen.max_prog_len() == 2 * k - 1
        top = [c for c in cen.chunks if c.prog_len == 2 * k - 1]
        assert len(top) == 1 and top[0].on_list == "2", top
        assert top[0].hist[sc.OP_LEAF] == k and top[0].hist[sc.OP_COMBINE] + top[0].hist[sc.OP_COMBINE_OUTSIDE] == k - 1

    stepped_twice_with_census(ctx, graph, check)


def test_balanced_tree_overflow_runs_all_seven_levels(ctx):
    """80 leaves under a balanced tree: 159 ops, the full program on every level of its stack"""
    k = 80
    graph = balanced_cluster(k, 6)

    def check(cen, gen):
        assert gen.sdf_generator.required_forward_stack_size == 7
        assert cluster_all_in_one_chunk(gen, k)
        full = [c for c in cen.chunks if c.prog_len is None]
        assert len(full) >= 1 and all(c.on_list == "2" for c in full), full

    stepped_twice_with_census(ctx, graph, check)


# ---- programs around and beyond 2048 nodes ------------------------------------------------------------------------------------------------
def padded_lattice(dims, pitch, n_nodes, seed):
    """Bodies on a lattice, each a leaf under a chain of nested translations, rotations and scalings (the skip table's nested subtrees), joined
    by a left-deep chain of hard and smooth unions: exactly `n_nodes` nodes, graph and compiled program alike."""
    rng = np.random.default_rng(seed)
    b = dims[0] * dims[1] * dims[2]
    wraps_total = n_nodes - (2 * b - 1)  # beyond a leaf per body and the unions
    assert wraps_total >= b
    g = SDFGraph()
    acc = None
    for i in range(b):
        wraps = wraps_total // b + (1 if i < wraps_total % b else 0)
        kind = i % 3
        if kind == 0:
            n = g.add_node(SDFNode.new_sphere(float(rng.uniform(5.0, 7.0))))
        elif kind == 1:
            n = g.add_node(SDFNode.new_box([float(x) for x in rng.uniform(8.0, 13.0, 3)]))
        else:
            n = g.add_node(SDFNode.new_capsule(float(rng.uniform(4.0, 8.0)), float(rng.uniform(3.0, 5.0))))
        scale = 1.0
        for w in range(wraps - 1):
            what = 2 if w % 9 == 8 else (1 if w in (3, 20) else 0)  # (few rotations: every one widens the domain box of what lies beneath it)
            if what == 0:
                n = g.add_node(SDFNode.new_translation(n, [float(x) for x in rng.uniform(-0.4, 0.4, 3)]))
            elif what == 1:
                axis = rng.normal(size=3)
                n = g.add_node(SDFNode.new_rotation_from_axis_angle(n, [float(x) for x in axis / np.linalg.norm(axis)], float(rng.uniform(-0.3, 0.3))))
            else:  # (the scalings of a chain stay near 1 in product)
                s = float(rng.uniform(0.9, 1.1)) if scale < 1.0 else float(rng.uniform(0.85, 1.0))
                scale *= s
                n = g.add_node(SDFNode.new_scaling(n, s))
        at = [pitch * (i % dims[0]), pitch * ((i // dims[0]) % dims[1]), pitch * (i // (dims[0] * dims[1]))]
        n = g.add_node(SDFNode.new_translation(n, [float(x + d) for x, d in zip(at, rng.uniform(-3.0, 3.0, 3))]))
        acc = n if acc is None else g.add_node(SDFNode.new_union(acc, n, float(rng.uniform(1.0, 4.0)) if rng.random() < 0.3 else 0.0))
    return g


# what: (lattice, pitch, nodes, seed). 2048 nodes: 64 words, every word of the pre-pass's own far bits in use; 2070: 65 words, the first program
# k_sdf_super takes; 4200: 132 words, three rounds of k_sdf_super's 64-lane loops over the far words and nodes
HUGE = {"2048": ((4, 3, 3), 26.0, 2048, 21), "2070": ((4, 3, 3), 26.0, 2070, 22), "4200": ((3, 4, 3), 26.0, 4200, 23)}
SUPER_MAX_NODES = 2048
_huge = {}


def huge(what):
    """(graph, generator, oracle) of a huge program, made once"""
    if what not in _huge:
        dims, pitch, n_nodes, seed = HUGE[what]
        graph = padded_lattice(dims, pitch, n_nodes, seed)
        gen = SDFVoxelGenerator(1.0, graph, 0)
        assert len(gen.sdf_generator.nodes) == n_nodes  # (the boundary cannot drift)
        cc = gen.chunk_counts()
        assert all(c % 4 != 0 for c in cc) and sum(1 for c in cc if c > 4) >= 2, cc  # ragged super-blocks, two or more of them along two axes
        _huge[what] = (graph, gen, oracle_of(graph))
    return _huge[what]


def small_twin(gen_huge):
    """a program of a few nodes on the same chunk counts as `gen_huge`: a box with a smooth crater, sized to the huge program's grid"""
    shape = gen_huge.grid_shape()
    for shrink in np.arange(2.0, 12.0, 0.5):
        g = SDFGraph()
        half = [0.5 * s - shrink for s in shape]
        box = g.add_node(SDFNode.new_box([2.0 * h for h in half]))
        crater = g.add_node(SDFNode.new_translation(g.add_node(SDFNode.new_sphere(0.6 * min(half))), [half[0], 0.3 * half[1], -0.2 * half[2]]))
        g.add_node(SDFNode.new_subtraction(box, crater, 2.0))
        gen = SDFVoxelGenerator(1.0, g, 0)
        if tuple(gen.chunk_counts()) == tuple(gen_huge.chunk_counts()):
            return g, gen
    raise AssertionError("no small program on the huge program's chunk counts")


@pytest.mark.parametrize("what", list(HUGE))
def test_program_around_the_super_table_limit(ctx, what):
    graph, gen, o = huge(what)
    n_nodes = HUGE[what][2]
    assert (n_nodes <= SUPER_MAX_NODES) == (what == "2048") and (n_nodes + 31) // 32 == {"2048": 64, "2070": 65, "4200": 132}[what]
    obj = resident(ctx, gen)
    r = obj.step(capi.STAGE_ALL)
    cen = sc.census(obj, n_nodes)
    print("census:", n_nodes, "nodes, chunks", gen.chunk_counts(), "lists", cen.counters, "max prog_len", cen.max_prog_len(), "full", cen.overflow_chunks,
          "consts", cen.op_total(sc.OP_CONST))
    assert sum(cen.lists) > 50  # (surface chunks all over the lattice; the pre-pass settled the rest from the far tables)
    p = pu.step_parity(o, obj, r)
    assert p["equal"], (0, p)
    assert_step(o, obj, what=1)
    obj.close()


def test_small_huge_small_with_the_pre_pass_ahead(ctx):
    """One resident grid with sample-ahead on: a small program (its next pre-pass goes under way), a huge one — `ahead_fits` is false beyond
    2048 nodes: no pre-pass runs ahead of its steps —, and the small one again, whose pre-pass must come back. Every step against the oracle."""
    graph, gen, o = huge("2070")
    g_small, gen_small = small_twin(gen)
    o_small = oracle_of(g_small)
    obj = resident(ctx, gen_small, ahead=True)
    for i in range(2):
        assert_step(o_small, obj, what=("small", i))
    obj.set_sdf_program(gen)
    for i in range(2):
        assert_step(o, obj, what=("huge", i))
    obj.set_sdf_program(gen_small)
    for i in range(3):
        assert_step(o_small, obj, what=("small again", i))
    obj.close()


def test_huge_program_with_stage_timing(ctx):
    """k_sdf_super is the stamped first launch of the sample slot: the bytes are the untimed step's (the oracle's), and slot 0 reports"""
    graph, gen, o = huge("2070")
    obj = resident(ctx, gen)
    obj.set_stage_timing(0xFFFFFFFF)
    for i in range(2):
        r = assert_step(o, obj, what=("timed", i))
        assert r["stage_ms"][0] > 0.0, list(r["stage_ms"])
        ticks, khz = obj.stage_ticks()
        assert khz > 0 and 0 < ticks[0, 0] < ticks[0, 1]
    obj.set_stage_timing(0)
    r = assert_step(o, obj, what="untimed")
    assert not np.any(r["stage_ms"])
    obj.close()


def test_huge_program_sample_alone_then_the_rest(ctx):
    """a step of the sample stage alone (k_sdf_super hosts only the sampler's own presets), then the other stages; then whole steps"""
    graph, gen, o = huge("4200")
    obj = resident(ctx, gen)
    for i in range(2):
        obj.step(capi.STAGE_SAMPLE)
        assert_step(o, obj, capi.STAGE_ALL & ~capi.STAGE_SAMPLE, what=("split", i))
    assert_step(o, obj, what="whole")
    obj.close()
