"""Region queries through the hierarchy without a GPU: `ivx_bv_queries_hierarchy_host` — the decision functions the kernels run — over the tree of
`ivx_bv_hierarchy_host`, against bvol_ref's float32 restatement of the flat decisions, masks and counts byte for byte; and the node decisions on
their own (`ivx_bv_query_skips_boxes`): no node above a leaf the flat reference hits may be skipped. No tolerance anywhere in this file.

The hit lists (`ivx_bv_query_lists`) have no host form: test_gpu_bvh_queries.py covers them."""
import os
import subprocess

import numpy as np
import pytest

import bvh_query_cases as qc
import bvh_ref as hr
import bvol_ref as br
from impact_amd import bvol, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assert_masks_equal(got, want, what):
    (got_masks, got_counts), (want_masks, want_counts) = got, want
    assert got_masks.dtype == np.uint64 and got_masks.shape == want_masks.shape and got_counts.dtype == np.uint32, what
    if got_masks.tobytes() != want_masks.tobytes():
        q, w = (int(x[0]) for x in np.nonzero(got_masks != want_masks))
        missing, extra = int(want_masks[q, w] & ~got_masks[q, w]), int(got_masks[q, w] & ~want_masks[q, w])
        raise AssertionError(f"{what}: query {q}, word {w}: objects missed {missing:#x}, objects added {extra:#x}")
    assert got_counts.tobytes() == want_counts.tobytes(), what


def through_the_host_tree(world, queries):
    nodes, leaves, _ = bvol.hierarchy_host(world)
    return bvol.queries_hierarchy_host(world, nodes, leaves, queries)


def test_symbols_and_constants(tmp_path):
    src = tmp_path / "ptr.c"
    src.write_text('#include <stdio.h>\n#include "impact_voxel_hip.h"\nint main(void) {\n    printf("%d %d\\n", IVX_BV_PTR_HIT_OFFSETS, IVX_BV_PTR_HIT_OBJECTS);\n    return 0;\n}\n')
    exe = tmp_path / "ptr"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()] == [capi.BV_PTR_HIT_OFFSETS, capi.BV_PTR_HIT_OBJECTS] == [5, 6]
    for name in ("ivx_bv_queries_hierarchy", "ivx_bv_queries_hierarchy_host", "ivx_bv_query_lists", "ivx_bv_query_skips_boxes"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(capi.lib(), name)


@pytest.mark.parametrize("n_queries", qc.QUERY_COUNTS)
@pytest.mark.parametrize("n", qc.SIZES)
def test_seeded_scene_with_mixed_queries(n, n_queries):
    world = br.scene(n)[0]
    queries = br.mixed_queries(n, n_queries)
    want = qc.reference(world, queries)
    if n >= 63:  # the case can show something: every kind hits a part of the scene
        for kind in range(min(4, n_queries)):
            assert 0 < int(want[1][kind]) < n, (kind, want[1][kind])
    assert_masks_equal(through_the_host_tree(world, queries), want, f"n {n}, {n_queries} queries")


@pytest.mark.parametrize("name", list(qc.hand_made_sets()))
def test_hand_made_sets(name):
    world = qc.hand_made_sets()[name]
    queries = qc.queries_over(world, 32, 40)
    want = qc.reference(world, queries)
    assert int(want[1].sum()) > 0, name
    assert_masks_equal(through_the_host_tree(world, queries), want, name)


@pytest.mark.parametrize("name", list(qc.adversarial_cases()))
def test_adversarial_sets(name):
    world, queries = qc.adversarial_cases()[name]
    want = qc.reference(world, queries)
    hits = np.stack([np.isin(np.arange(len(world)), idx) for idx in bvol.mask_indices(want[0], len(world))])
    # each case shows what it is there for
    if name == "touching faces":
        d = np.concatenate([br.face_differences(q["lower"].astype(np.float32), q["upper"].astype(np.float32), world["lower"], world["upper"])[h] for q, h in zip(queries, hits)])
        assert (d == 0).any(axis=-1).sum() >= 20, "too few hits with a face exactly on the query's"
    if name == "signed zero":
        assert hits.tolist() == [[False, True, True, True, False], [True, True, False, True, False], [True, True, True, True, False]]
    if name.startswith("nan bounds"):
        nan = hr.has_nan(world)
        spheres = queries["kind"] == capi.BV_QUERY_SPHERE
        assert nan.sum() >= 29 and hits[spheres][:, nan].any() and not hits[~spheres][:, nan].any()
    if name == "lower above upper":
        inverted = (world["lower"] > world["upper"]).any(axis=-1)
        assert inverted.sum() >= 37 and hits[:, inverted].any()
    if name.startswith("unbounded"):
        assert hr.unbounded(world).sum() >= 5 and hits[:, ~hr.unbounded(world)].any()
    if "scrambled" in name:
        frusta = queries["kind"] == capi.BV_QUERY_FRUSTUM
        agree = [[int(c) == br.corner_of(p[:3]) for c, p in zip(q["corners"], q["planes"])] for q in queries[frusta]]
        assert not np.all(agree) and hits[frusta].any()
    if name == "far oriented boxes":
        assert len(world) >= 257 and (hits.sum(axis=1) >= 12).all() and ((~hits).sum(axis=1) >= 12).all()  # (boxes on both sides of every query's decision)
    if name == "nan queries":
        assert all(int(k) in queries["kind"] for k in range(4)) and want[1][queries["kind"] == capi.BV_QUERY_SPHERE].max() == len(world)  # (a NaN radius hits all)
    assert_masks_equal(through_the_host_tree(world, queries), want, name)


def sweep_sets():
    """seed -> (257 world boxes, 64 queries): seeded random sets at several scales, and the adversarial sets cut or filled to 257"""
    adversarial = list(qc.adversarial_cases().items())
    for seed in range(200):
        rng = np.random.default_rng(1000 + seed)
        if seed % 4 == 3:
            name, (world, queries) = adversarial[(seed // 4) % len(adversarial)]
            filler = np.array(br.scene(257, seed=50 + seed)[0])
            if name == "far oriented boxes":
                world, queries = qc.far_oriented_case(seed)
                filler["lower"] += np.float32(qc.OBB_ORIGIN)
                filler["upper"] += np.float32(qc.OBB_ORIGIN)
            world = np.concatenate([world, filler])[rng.permutation(len(world) + 257)[:257]] if len(world) != 257 else world
            yield f"{seed} {name}", world, (queries if len(queries) >= 64 else bvol.query_array(list(queries) + list(qc.queries_over(world, 64 - len(queries), seed))))[:64]
            continue
        scale = 10.0 ** rng.uniform(-3, 4)
        origin = rng.normal(size=3) * scale * 10.0 ** rng.uniform(-1, 3)
        centres = origin + rng.uniform(0, scale, (257, 3)) * np.array([1.0, rng.choice([1.0, 0.02]), rng.choice([1.0, 1e-3])])
        half = scale * 10.0 ** rng.uniform(-3, -0.5, (257, 3))
        world = bvol.boxes(centres - half, centres + half)
        yield f"{seed} scale {scale:.3g}", world, qc.queries_over(world, 64, seed)


def test_no_node_above_a_hit_leaf_is_skipped():
    """200 sets of 257 boxes under 64 queries each: wherever the flat reference hits a proper leaf, the node decision enters every node above it.
    (Irregular leaves are decided outside the walk; the other tests hold the whole call to the reference.)"""
    skipped = looked_at = 0
    by_kind = np.zeros(4, dtype=np.int64)
    for name, world, queries in sweep_sets():
        assert len(world) == 257 and len(queries) == 64, name
        nodes, leaves, _ = bvol.hierarchy_host(world)
        hits = np.stack([np.isin(np.arange(257), idx) for idx in bvol.mask_indices(qc.reference(world, queries)[0], 257)])
        proper = (world["lower"] <= world["upper"]).all(axis=-1)
        by_position = (hits & proper)[:, leaves]
        below = np.concatenate([np.zeros((64, 1), dtype=np.int64), np.cumsum(by_position, axis=1)], axis=1)
        last = hr.range_ends(nodes, 257)
        _, count = bvol.node_info(nodes, 257)
        first = last - count.astype(np.int64) + 1
        hit_below = (below[:, last + 1] - below[:, first]) > 0  # [64, 256]: the query hits a proper leaf under the node
        skips = bvol.query_skips_boxes(queries, nodes)
        bad = np.argwhere(skips & hit_below)
        assert not len(bad), f"{name}: query {bad[0][0]} (kind {int(queries['kind'][bad[0][0]])}) skips node {bad[0][1]} above a leaf it hits; {len(bad)} such"
        skipped, looked_at = skipped + int(skips.sum()), looked_at + skips.size
        np.add.at(by_kind, queries["kind"].astype(np.int64), skips.sum(axis=1))
    # ... and the decisions do skip: a sweep over decisions that enter everything would show nothing
    assert skipped * 4 >= looked_at and (by_kind > looked_at // 64).all(), (skipped, looked_at, by_kind)


def test_refusals_and_empty_inputs():
    lib = capi.lib()
    world = np.array(br.scene(65)[0])
    nodes, leaves, _ = bvol.hierarchy_host(world)
    queries = br.mixed_queries(65, 8)
    masks, counts = np.zeros((8, 2), dtype=np.uint64), np.zeros(8, dtype=np.uint32)
    call = lambda q=queries, nq=8, m=masks, w=world, n=65, t=nodes, l=leaves: lib.ivx_bv_queries_hierarchy_host(
        capi.ptr(w) if w is not None else None, n, capi.ptr(t) if t is not None else None, capi.ptr(l) if l is not None else None, capi.ptr(q) if q is not None else None, nq,
        capi.ptr(m) if m is not None else None, capi.ptr(counts))
    assert call() == capi.IVX_OK
    assert call(nq=capi.BV_MAX_QUERIES + 1) == capi.IVX_ERR_CAPACITY and call(n=capi.BV_MAX_OBJECTS + 1) == capi.IVX_ERR_CAPACITY
    assert call(q=None) == capi.IVX_ERR_INVALID and call(m=None) == capi.IVX_ERR_INVALID and call(w=None) == capi.IVX_ERR_INVALID
    assert call(t=None) == capi.IVX_ERR_INVALID and call(l=None) == capi.IVX_ERR_INVALID
    bad = queries.copy()
    bad["kind"][3] = 4
    assert call(q=bad) == capi.IVX_ERR_INVALID
    # no queries: nothing is written; no objects: the counts are zero
    masks[:], counts[:] = 7, 7
    assert call(nq=0) == capi.IVX_OK and (masks == 7).all() and (counts == 7).all()
    assert call(n=0, w=None, t=None, l=None, m=None) == capi.IVX_OK and (counts == 0).all()
    # a tree that is none: a link out of range, a cycle
    broken = nodes.copy()
    broken["left"][0] = 64
    assert call(t=broken) == capi.IVX_ERR_STATE and b"inconsistent" in lib.ivx_last_error()
    cycle = nodes.copy()
    cycle["left"][:], cycle["right"][:] = 0, 0
    cycle["lower"][:], cycle["upper"][:] = -1e9, 1e9
    assert call(t=cycle) == capi.IVX_ERR_STATE
    broken_leaves = leaves.copy()
    broken_leaves[:] = 65
    assert call(l=broken_leaves) == capi.IVX_ERR_STATE
    # the node decision's own refusals
    skips = np.zeros(1, dtype=np.uint8)
    box = bvol.boxes([(0, 0, 0)], [(1, 1, 1)])
    assert lib.ivx_bv_query_skips_boxes(capi.ptr(bad[3:4]), 1, capi.ptr(box), 1, capi.ptr(skips)) == capi.IVX_ERR_INVALID
    assert lib.ivx_bv_query_skips_boxes(None, 1, capi.ptr(box), 1, capi.ptr(skips)) == capi.IVX_ERR_INVALID
