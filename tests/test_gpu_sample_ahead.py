"""Sample-ahead (`ivx_grid_set_sample_ahead`): the next sample stage's interval pre-pass rides on the context's second stream behind this
stage's evaluator, into a second set of the sampler's buffers, and the records it settles wait in a shadow array until the next evaluator
launch commits them. Whatever order the steps come in, what a step leaves on the device must be what the oracle computes.

A step of an unchanged program rewrites bytes that are resident already: a consumed pre-pass that handed the evaluator an empty list, or
shadow records that were never committed, would go unseen. So the tests overwrite the planes with junk between sampled steps
(`clobber`): `ivx_grid_upload_dense` also re-classifies every chunk — all of them come out NonUniform — so the next step has to restore
the bytes of the evaluated chunks AND the records of the chunks its pre-pass settled (Void / Uniform, parked in the shadow array)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import parity_util as pu
from impact_amd import capi, scenes
from impact_amd.sdf_graph import SDFGraph, SDFNode
from impact_amd.voxel import SDFVoxelGenerator, VoxelObject

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def clobber(obj):
    """0x55 into every byte of the sdf and type planes; every chunk record becomes NonUniform (k_classify)"""
    n = obj.n_voxels
    junk_sdf, junk_typ = np.full(n, 0x55, np.int8), np.full(n, 0x55, np.uint8)
    capi.check(capi.lib().ivx_grid_upload_dense(obj.h, junk_sdf.ctypes.data, junk_typ.ctypes.data, n))
    info = obj.download(sdf=False, types=False, flags=False, labels=False)[4]
    assert np.all(info["kind"] == 2) and np.all(info["gen_kind"] == 2)  # (nothing of the step before is left in the records either)


def resident_object(ctx, graph, ahead):
    gen = SDFVoxelGenerator(1.0, graph, 0)
    obj = VoxelObject(ctx, gen.chunk_counts(), 1.0)
    obj.set_sdf_program(gen)
    obj.set_densities(np.ones(256, dtype=np.float32))
    obj.set_sample_ahead(ahead)
    return gen, obj


def oracle_of(graph):
    o = pu.oracle_from_graph(graph)
    o.update_occupied_voxel_ranges()
    o.compute_all_derived_state()
    return o


def craters(n=3):
    g = SDFGraph()
    acc = g.add_node(SDFNode.new_sphere(30.0))
    for i in range(n):
        s = g.add_node(SDFNode.new_sphere(9.0))
        t = g.add_node(SDFNode.new_translation(s, (26.0 - 20.0 * i, 8.0 * i, -6.0 * i)))
        acc = g.add_node(SDFNode.new_subtraction(acc, t, 2.0))
    return g


def test_steps_with_the_pre_pass_a_step_ahead_are_the_same_steps(ctx):
    """Config 2's asteroid: five steps in a row (the first runs its own pre-pass, the others find theirs done), each against the oracle;
    a twin without sample-ahead gives the same step results."""
    graph = scenes.asteroid_scene(1.0)
    o = oracle_of(graph)
    _, a = resident_object(ctx, graph, True)
    _, b = resident_object(ctx, graph, False)
    for i in range(5):
        ra, rb = a.step(capi.STAGE_ALL), b.step(capi.STAGE_ALL)
        p = pu.step_parity(o, a, ra)
        assert p["equal"], (i, p)
        assert ra["mesh"] == rb["mesh"] and ra["region_count"] == rb["region_count"]
        np.testing.assert_array_equal(np.asarray(ra["occupied"]), np.asarray(rb["occupied"]))
        np.testing.assert_array_equal(np.asarray(ra["moments"]["m64"]), np.asarray(rb["moments"]["m64"]))
        if i < 4:  # (the counters below are the last step's)
            clobber(a)
    assert a.stage_counters()["evaluated_chunks"] == b.stage_counters()["evaluated_chunks"]
    a.close()
    b.close()


def test_other_steps_in_between_and_a_new_program(ctx):
    """Between two sampled steps: a step without the sample stage, a remesh alone, then ANOTHER program (the pre-pass under way was made for
    the old one and must be dropped), then the first program again."""
    g1, g2 = craters(3), craters(1)
    gen1 = SDFVoxelGenerator(1.0, g1, 0)
    gen2 = SDFVoxelGenerator(1.0, g2, 0)
    cc = tuple(max(a_, b_) for a_, b_ in zip(gen1.chunk_counts(), gen2.chunk_counts()))
    assert gen1.chunk_counts() == cc and gen2.chunk_counts() == cc  # (a subtraction's domain is its first operand's: both are the sphere's)
    o1, o2 = oracle_of(g1), oracle_of(g2)
    obj = VoxelObject(ctx, cc, 1.0)
    obj.set_densities(np.ones(256, dtype=np.float32))
    obj.set_sample_ahead(True)
    obj.set_sdf_program(gen1)
    r = obj.step(capi.STAGE_ALL)
    assert pu.step_parity(o1, obj, r)["equal"]
    obj.step(capi.STAGE_DERIVE | capi.STAGE_REGIONS)
    obj.step(capi.STAGE_REMESH)
    clobber(obj)
    r = obj.step(capi.STAGE_ALL)
    assert pu.step_parity(o1, obj, r)["equal"]
    obj.set_sdf_program(gen2)
    for _ in range(2):
        clobber(obj)
        r = obj.step(capi.STAGE_ALL)
        assert pu.step_parity(o2, obj, r)["equal"]
    obj.set_sdf_program(gen1)
    for _ in range(2):
        clobber(obj)
        r = obj.step(capi.STAGE_ALL)
        assert pu.step_parity(o1, obj, r)["equal"]
    obj.set_sample_ahead(False)  # (drops the pre-pass under way)
    clobber(obj)
    r = obj.step(capi.STAGE_ALL)
    assert pu.step_parity(o1, obj, r)["equal"]
    obj.close()


def test_an_object_goes_while_its_pre_pass_is_under_way(ctx):
    """close() right behind a step: the grid waits for its pre-pass on the second stream before its buffers go; many times over, and a
    sampled object made afterwards is sound."""
    graph = craters(2)
    for _ in range(20):
        _, obj = resident_object(ctx, graph, True)
        obj.step(capi.STAGE_ALL)
        obj.close()
    o = oracle_of(graph)
    _, obj = resident_object(ctx, graph, True)
    for _ in range(3):
        r = obj.step(capi.STAGE_ALL)
        assert pu.step_parity(o, obj, r)["equal"]
    obj.close()


def test_sample_alone_then_the_rest(ctx):
    """A step of the sample stage alone (no derive sweep rolls the list counters over), then the other stages, with the pre-pass ahead."""
    graph = craters(3)
    o = oracle_of(graph)
    _, obj = resident_object(ctx, graph, True)
    for _ in range(3):
        obj.step(capi.STAGE_SAMPLE)
        r = obj.step(capi.STAGE_ALL & ~capi.STAGE_SAMPLE)
        assert pu.step_parity(o, obj, r)["equal"]
    for _ in range(2):
        r = obj.step(capi.STAGE_ALL)
        assert pu.step_parity(o, obj, r)["equal"]
    obj.close()


@pytest.mark.parametrize("seed", pu.fuzz_seeds([31, 32, 33, 34, 35, 36, 210, 341]))
def test_random_programs_with_the_pre_pass_a_step_ahead(ctx, seed):
    """tests/test_gpu_random_sdf.py's programs as resident programs stepped three times with the pre-pass ahead: the second and third step start
    at their evaluator, whose first launch commits the records the pre-pass parked — the chunk records and voxel bytes of every step against
    the oracle's"""
    from test_gpu_random_sdf import random_tree

    rng = np.random.default_rng(seed)
    g = SDFGraph()
    random_tree(g, rng, int(rng.integers(1, 5)))
    gen = SDFVoxelGenerator(1.0, g, 0)
    if min(gen.chunk_counts()) == 0:
        pytest.skip("degenerate root domain")
    o = oracle_of(g)
    obj = VoxelObject(ctx, gen.chunk_counts(), 1.0)
    obj.set_sdf_program(gen)
    obj.set_densities(np.ones(256, dtype=np.float32))
    obj.set_sample_ahead(True)
    for i in range(3):
        r = obj.step(capi.STAGE_ALL)
        p = pu.step_parity(o, obj, r)
        assert p["equal"], (i, p)
        clobber(obj)
    obj.close()


def test_two_programs_alternated_every_step(ctx):
    """two programs of equal chunk counts, the resident one swapped before every step for ten steps: every pre-pass under way was made for
    the other program and must be dropped, and nothing of the step before may stand in for this step's work (planes clobbered)"""
    g1, g2 = craters(3), craters(1)
    gens = (SDFVoxelGenerator(1.0, g1, 0), SDFVoxelGenerator(1.0, g2, 0))
    assert gens[0].chunk_counts() == gens[1].chunk_counts()
    os_ = (oracle_of(g1), oracle_of(g2))
    obj = VoxelObject(ctx, gens[0].chunk_counts(), 1.0)
    obj.set_densities(np.ones(256, dtype=np.float32))
    obj.set_sample_ahead(True)
    for i in range(10):
        obj.set_sdf_program(gens[i % 2])
        r = obj.step(capi.STAGE_ALL)
        p = pu.step_parity(os_[i % 2], obj, r)
        assert p["equal"], (i, p)
        clobber(obj)
    obj.close()


def test_steps_enqueued_without_a_collect_in_between(ctx):
    """three whole steps enqueued back to back, one collect: from the second on the caller has not collected what it enqueued before, so the
    pre-pass ahead takes its place in the stream's order behind the step's last big launch; then a collected step"""
    graph = scenes.asteroid_scene(1.0)
    o = oracle_of(graph)
    _, obj = resident_object(ctx, graph, True)
    r = obj.step(capi.STAGE_ALL)
    assert pu.step_parity(o, obj, r)["equal"]
    clobber(obj)
    for _ in range(3):
        obj.step_enqueue(capi.STAGE_ALL)
    r = obj.step_collect().copy()
    p = pu.step_parity(o, obj, r)
    assert p["equal"], p
    clobber(obj)
    r = obj.step(capi.STAGE_ALL)
    p = pu.step_parity(o, obj, r)
    assert p["equal"], p
    obj.close()


# ---- a 2 x 2 x 2-chunk grid whose setting and program change between steps, against a twin that never samples ahead --------------------
SUPER_MAX_NODES = 2048  # (32 * SUPER_MAX_WORDS: beyond it k_sdf_super builds the far tables and no pre-pass runs ahead)


def small_body():
    """a ball with a smooth crater: 28^3 voxels"""
    g = SDFGraph()
    ball = g.add_node(SDFNode.new_sphere(13.0))
    dent = g.add_node(SDFNode.new_translation(g.add_node(SDFNode.new_sphere(6.0)), (9.0, 4.0, -3.0)))
    g.add_node(SDFNode.new_subtraction(ball, dent, 2.0))
    return g


def sphere_chain(n_nodes):
    """small spheres on a 9^3 lattice under a left-deep chain of hard unions, 3 K - 1 nodes, padded by translations to exactly `n_nodes`: 28^3 voxels"""
    k = (n_nodes + 1) // 3
    pad = n_nodes - (3 * k - 1)
    assert k <= 729 and 0 <= pad < 3
    g = SDFGraph()
    acc = None
    for i in range(k):
        s = g.add_node(SDFNode.new_sphere(1.0))
        for _ in range(pad if i == 0 else 0):
            s = g.add_node(SDFNode.new_translation(s, (0.0, 0.0, 0.0)))
        s = g.add_node(SDFNode.new_translation(s, (3.0 * (i % 9) - 12.0, 3.0 * ((i // 9) % 9) - 12.0, 3.0 * (i // 81) - 12.0)))
        acc = s if acc is None else g.add_node(SDFNode.new_union(acc, s, 0.0))
    return g


def everything(obj):
    sdf, typ, flg, lab, info = obj.download()
    return {"sdf": sdf, "type": typ, "flags": flg, "labels": lab, "info": info.view(np.uint8)}


def assert_same_bytes(a, b, what):
    ea, eb = everything(a), everything(b)
    for k in ea:
        np.testing.assert_array_equal(ea[k], eb[k], err_msg=f"{what}: {k}")


def active_set_words(obj):
    """the active set of the sampler's buffers (developer pointer 7): [n] program lengths, [16] list counters, [3 n] lists"""
    import ctypes as C

    lib = capi.lib()
    lib.ivx_grid_device_ptr.restype = C.c_void_p
    hip = C.CDLL("libamdhip64.so")
    words = np.zeros(4 * obj.n_chunks + 16, dtype=np.uint32)
    hip.hipDeviceSynchronize()
    assert hip.hipMemcpy(words.ctypes.data_as(C.c_void_p), C.c_void_p(lib.ivx_grid_device_ptr(obj.h, 7)), words.nbytes, 2) == 0
    return words


def test_program_swapped_from_short_to_long_and_back(ctx):
    """sample-ahead on: two steps of a short program (the second consumes), then one of 2049 nodes (the pre-pass under way is dropped, the stage
    runs its own behind k_sdf_super, nothing runs ahead of the next), then the short one again (its pre-pass comes back): every step's
    bytes and records are those of a twin with sample-ahead off, which are the oracle's"""
    g_short, g_long = small_body(), sphere_chain(SUPER_MAX_NODES + 1)
    gens = {"short": SDFVoxelGenerator(1.0, g_short, 0), "long": SDFVoxelGenerator(1.0, g_long, 0)}
    assert len(gens["long"].sdf_generator.nodes) == SUPER_MAX_NODES + 1
    assert tuple(gens["short"].chunk_counts()) == tuple(gens["long"].chunk_counts()) == (2, 2, 2)
    oracles = {"short": oracle_of(g_short), "long": oracle_of(g_long)}
    objs = []
    for ahead in (True, False):
        obj = VoxelObject(ctx, (2, 2, 2), 1.0)
        obj.set_densities(np.ones(256, dtype=np.float32))
        obj.set_sample_ahead(ahead)
        objs.append(obj)
    a, b = objs
    for which in ("short", "long", "short"):
        for obj in objs:
            obj.set_sdf_program(gens[which])
        for i in range(2):
            ra, rb = a.step(capi.STAGE_ALL), b.step(capi.STAGE_ALL)
            p = pu.step_parity(oracles[which], a, ra)
            assert p["equal"], (which, i, p)
            assert ra["mesh"] == rb["mesh"] and ra["region_count"] == rb["region_count"]
            assert_same_bytes(a, b, (which, i))
            clobber(a)
            clobber(b)
    a.close()
    b.close()


def test_sample_ahead_turned_off_and_on_between_steps(ctx):
    """the setting changes between collected steps and between steps enqueued back to back: the bytes are the twin's that never samples ahead,
    and a step behind set_sample_ahead(0) leaves the active set's counters and lists as its own pre-pass made them"""
    graph = small_body()
    o = oracle_of(graph)
    _, a = resident_object(ctx, graph, True)
    _, b = resident_object(ctx, graph, False)
    assert a.chunk_counts == (2, 2, 2)
    n = a.n_chunks

    def both(what, settings, collect_each):
        """one step per entry of `settings` (sample-ahead of `a` before the step; None: left as it is)"""
        for on in settings:
            if on is not None:
                a.set_sample_ahead(on)
            for obj in (a, b):
                obj.step(capi.STAGE_ALL) if collect_each else obj.step_enqueue(capi.STAGE_ALL)
        ra = a.step_collect().copy() if not collect_each else None
        if not collect_each:
            b.step_collect()
            p = pu.step_parity(o, a, ra)
            assert p["equal"], (what, p)
        assert_same_bytes(a, b, what)

    both("on, collected", [None, None], True)  # (the second consumes; a pre-pass is under way behind it)
    both("off", [False], True)
    wa, wb = active_set_words(a), active_set_words(b)
    np.testing.assert_array_equal(wa[n:n + 16], wb[n:n + 16])  # live counters zero (rolled over by the derive sweep), their rolled copy this step's
    assert not wa[n:n + 8].any() and wa[n + 8:n + 11].sum() > 0
    np.testing.assert_array_equal(wa[:n], wb[:n])
    for c in range(3):  # (the order within a list is the order the pre-pass's blocks came by)
        cnt = int(wa[n + 8 + c])
        seg = slice(n + 16 + c * n, n + 16 + c * n + cnt)
        if c == 0:  # long entries from the front, short ones from the back
            cnt_long = int(wa[n + 8 + 3])
            np.testing.assert_array_equal(np.sort(wa[n + 16:n + 16 + cnt_long]), np.sort(wb[n + 16:n + 16 + cnt_long]))
            np.testing.assert_array_equal(np.sort(wa[n + 16 + n - (cnt - cnt_long):n + 16 + n]), np.sort(wb[n + 16 + n - (cnt - cnt_long):n + 16 + n]))
        else:
            np.testing.assert_array_equal(np.sort(wa[seg]), np.sort(wb[seg]))
    clobber(a), clobber(b)
    both("on again, collected", [True, None], True)
    clobber(a), clobber(b)
    both("back to back", [None, None, None], False)
    clobber(a), clobber(b)
    both("off and on back to back", [None, False, True, None], False)
    clobber(a), clobber(b)
    both("off back to back, then collected", [False, None], False)
    both("on after that", [True, None], True)
    a.close()
    b.close()


def _poisoned_seeds():
    from test_gpu_random_sdf import WITNESSED

    return [s for s, w in WITNESSED.items() if "P" in w][:6]


@pytest.mark.parametrize("seed", _poisoned_seeds())
def test_poisoned_chunks_with_the_pre_pass_a_step_ahead(ctx, seed):
    """witnessed seeds with chunks on the `poisoned` fallback: from the second step on their OP_OVERFLOW lengths come out of the second set of
    the sampler's buffers"""
    import sampler_census as sc
    from test_gpu_random_sdf import witnessed_program

    g, gen = witnessed_program(seed)
    o = oracle_of(g)
    obj = VoxelObject(ctx, gen.chunk_counts(), 1.0)
    obj.set_sdf_program(gen)
    obj.set_densities(np.ones(256, dtype=np.float32))
    obj.set_sample_ahead(True)
    poisoned = []
    for i in range(3):
        r = obj.step(capi.STAGE_ALL)
        poisoned.append(sc.census(obj, len(gen.sdf_generator.nodes)).poisoned_chunks)
        p = pu.step_parity(o, obj, r)
        assert p["equal"], (i, p)
        clobber(obj)
    assert poisoned[0] > 0 and poisoned == [poisoned[0]] * 3, poisoned  # (both sets of buffers carried them)
    obj.close()


# ---- the ahead pre-pass's block loop: fewer blocks than super-blocks (IVX_AHEAD_BLOCKS is read once, on first use: a child process) ----
def ahead_blocks_graph():
    """6 x 7 x 5 chunks: 2 x 2 x 2 super-blocks, the upper ones ragged"""
    g = SDFGraph()
    acc = g.add_node(SDFNode.new_box([64.0, 78.0, 62.0]))
    for i in range(4):
        s = g.add_node(SDFNode.new_sphere(14.0 + 2.0 * i))
        t = g.add_node(SDFNode.new_translation(s, (30.0 - 18.0 * i, -36.0 + 24.0 * i, 28.0 - 16.0 * i)))
        acc = g.add_node(SDFNode.new_subtraction(acc, t, 2.0) if i % 2 == 0 else SDFNode.new_union(acc, t, 3.0))
    return g


def ahead_blocks_steps(ctx):
    """three steps with sample-ahead on and the planes clobbered in between: what the last one left (planes, records, step record)"""
    graph = ahead_blocks_graph()
    gen, obj = resident_object(ctx, graph, True)
    for i in range(3):
        if i:
            clobber(obj)
        r = obj.step(capi.STAGE_ALL)
    sdf, typ, flg, lab, info = obj.download()
    out = {"sdf": sdf, "type": typ, "flags": flg, "labels": lab, "info": info.view(np.uint8),
           "counts": np.array([int(r["mesh"]["n_vertices"]), int(r["mesh"]["n_indices"]), int(r["region_count"]), obj.stage_counters()["evaluated_chunks"]], dtype=np.int64),
           "moments": np.asarray(r["moments"]["m64"], dtype=np.float64).view(np.uint64)}
    obj.close()
    return graph, gen, out


def test_ahead_pre_pass_walks_the_super_blocks_in_turn(ctx):
    """IVX_AHEAD_BLOCKS=1: one block walks all eight super-blocks through the loop's barrier; =3: three blocks, two or three rounds each.
    The bytes are those of the same steps in this process (a block per super-block), which are the oracle's."""
    graph, gen, want = ahead_blocks_steps(ctx)
    cc = gen.chunk_counts()
    assert all(c % 4 != 0 and c > 4 for c in cc), cc
    o = oracle_of(graph)
    o_sdf, o_typ, o_flg, o_lab, o_info = o.export_dense()
    np.testing.assert_array_equal(want["sdf"], o_sdf)
    np.testing.assert_array_equal(want["flags"], o_flg)
    np.testing.assert_array_equal(want["info"].view(capi.CHUNK_INFO_DTYPE)["kind"], o_info["kind"])
    for blocks in ("1", "3"):
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "steps.npz")
            p = subprocess.run([sys.executable, os.path.join(HERE, "sample_ahead_worker.py"), out], env=dict(os.environ, IVX_AHEAD_BLOCKS=blocks),
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
            assert p.returncode == 0, p.stdout[-3000:]
            got = dict(np.load(out))
        assert sorted(got) == sorted(want)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"IVX_AHEAD_BLOCKS={blocks}: {k}")
