"""The hierarchy over a bounding-volume set without a GPU: the node record through gcc, the library's host key and host tree
(`ivx_bv_morton_key`, `ivx_bv_hierarchy_host` — the functions the kernels run) against the restatement in bvh_ref.py, byte for byte, and the
restated pair walk over the host-built tree against bvol_ref's exact upper triangle: the proof that no node box rejects a pair its members
accept. No tolerance anywhere in this file."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bvh_ref as hr
import bvol_ref as br
from impact_amd import bvol, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = np.finfo(np.float32).max


def test_node_record_matches_the_c_compiler(tmp_path):
    src = tmp_path / "node.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "impact_voxel_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %u %d %d %u %u\\n", sizeof(ivx_bv_node), offsetof(ivx_bv_node, upper), offsetof(ivx_bv_node, left),\n'
                   '           offsetof(ivx_bv_node, right), IVX_BV_LEAF, IVX_BV_PTR_NODES, IVX_BV_PTR_LEAF_OBJECTS, IVX_CW_BROAD_FLAT, IVX_CW_BROAD_HIERARCHY);\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "node"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    dt = capi.BV_NODE_DTYPE
    assert got == [32, dt.fields["upper"][1], dt.fields["left"][1], dt.fields["right"][1], capi.BV_LEAF, capi.BV_PTR_NODES, capi.BV_PTR_LEAF_OBJECTS,
                   capi.CW_BROAD_FLAT, capi.CW_BROAD_HIERARCHY]
    assert dt.itemsize == 32 and capi.extra_struct_sizes()["ivx_bv_node"] == (dt, 32)
    for name in ("ivx_bv_morton_key", "ivx_bv_hierarchy_host", "ivx_bv_build_hierarchy", "ivx_bv_hierarchy_download", "ivx_bv_pairs_hierarchy", "ivx_cw_set_broad_phase"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(capi.lib(), name)


def test_morton_key_against_the_restatement():
    """the 400 seeded cases' world boxes in their own frame, then the special boxes in the frame (0, 0, 0) - (8, 8, 8)"""
    world = br.host_world_boxes(*br.seeded_derivation_cases(400, 21))
    fr = hr.frame(world)
    codes = set()
    for o in range(len(world)):
        want = hr.key(fr, world[o], o)
        assert bvol.morton_key(fr, world[o], o) == want, o
        codes.add(want >> 32)
    assert len(codes) > 300 and hr.LAST_CODE not in codes  # (the cases spread over the frame)
    fr = bvol.boxes([(0, 0, 0)], [(8, 8, 8)])[0]
    one = lambda lo, hi: bvol.boxes([lo], [hi])[0]
    special = {"centre on the lower face": one((-1, 3, 3), (1, 5, 5)), "centre on the upper face": one((7, 3, 3), (9, 5, 5)),
               "negative zero bounds": one((-0.0, -0.0, -0.0), (0.0, 4.0, 8.0)), "nan bound": one((1, np.nan, 1), (2, 2, 2)),
               "plane": one((-FLT_MAX,) * 3, (FLT_MAX,) * 3), "bound of exactly 1e30": one((1, 1, 1), (2, 2, np.float32(1e30))),
               "just below 1e30": one((1, 1, 1), (2, 2, np.nextafter(np.float32(1e30), np.float32(0))))}
    for name, box in special.items():
        assert bvol.morton_key(fr, box, 7) == hr.key(fr, box, 7), name
    q_of = lambda box: bvol.morton_key(fr, box, 0) >> 32
    assert q_of(special["centre on the lower face"]) == (hr.spread3(512) << 1) | hr.spread3(512)  # x: q = 0
    assert q_of(special["centre on the upper face"]) == (hr.spread3(1023) << 2) | (hr.spread3(512) << 1) | hr.spread3(512)  # x: t = 1, q = 1023
    for name in ("nan bound", "plane", "bound of exactly 1e30"):
        assert q_of(special[name]) == hr.LAST_CODE, name
    assert q_of(special["just below 1e30"]) != hr.LAST_CODE
    # a zero-extent axis of the frame: t is 0 / 0, a NaN, and q is 0
    flat = bvol.boxes([(0, 2, 0)], [(8, 2, 8)])[0]
    box = one((1, 2, 1), (3, 2, 3))
    assert bvol.morton_key(flat, box, 3) == hr.key(flat, box, 3) == (((hr.spread3(256) << 2) | hr.spread3(256)) << 32) | 3
    # the index is the key's low word
    assert bvol.morton_key(fr, box, 0xFFFFF) & 0xFFFFFFFF == 0xFFFFF


def tree_cases():
    for n in (0, 1, 2, 3, 63, 64, 65, 257, 1025, 4161):
        yield f"scene {n}", br.scene(n)[0]
    yield "identical 130", hr.identical_boxes(130)
    yield "line 200", hr.line_boxes(200)
    yield "plane 200", hr.plane_boxes(200)


@pytest.mark.parametrize("name,world", list(tree_cases()), ids=[n for n, _ in tree_cases()])
def test_host_hierarchy(name, world):
    n = len(world)
    nodes, leaf_objects, fr = bvol.hierarchy_host(world)
    assert nodes.shape == (max(n - 1, 0),) and leaf_objects.shape == (n,)
    want_frame = hr.frame(world)
    assert fr.tobytes() == want_frame.tobytes()
    # leaves: a permutation in ascending restated-key order
    keys = [hr.key(want_frame, world[int(o)], int(o)) for o in leaf_objects]
    assert sorted(leaf_objects.tolist()) == list(range(n)) and keys == sorted(keys) and len(set(keys)) == n
    if n < 2:
        return
    # every internal node but the root is referenced exactly once, every leaf position exactly once
    refs = np.concatenate([nodes["left"], nodes["right"]]).astype(np.int64)
    leaf_refs, node_refs = refs[(refs & capi.BV_LEAF) != 0] & ~capi.BV_LEAF, refs[(refs & capi.BV_LEAF) == 0]
    assert sorted(leaf_refs.tolist()) == list(range(n)) and sorted(node_refs.tolist()) == list(range(1, n - 1))
    # every node box is the restated union of its children's
    leaves = hr.leaf_boxes(world, leaf_objects)
    for i in range(n - 1):
        lo, hi = hr.union(*hr.child_box(nodes, leaves, int(nodes["left"][i])), *hr.child_box(nodes, leaves, int(nodes["right"][i])))
        assert nodes["lower"][i].tobytes() == lo.tobytes() and nodes["upper"][i].tobytes() == hi.tobytes(), i
    depth, count = bvol.node_info(nodes, n)
    assert int(depth.max()) + 1 <= 50 and int(count[0]) == n and depth[0] == 0
    assert np.all(count >= 2)
    # ... and the whole tree is the restatement's own
    want_nodes, want_leaves, _, _ = hr.build(world)
    assert leaf_objects.tobytes() == want_leaves.tobytes() and nodes.tobytes() == want_nodes.tobytes()


def walk_cases():
    for n, totals in ((257, (682, 495)), (1025, (3245, 2441))):
        world, kinds = br.scene(n)
        for mode in (0, 1):
            yield f"scene {n} mode {mode}", world, kinds, mode, totals[mode]
    yield "identical 130", hr.identical_boxes(130), None, 0, 8385
    for name, (world, kinds) in hr.hand_made_cases().items():
        for mode in ((0, 1) if kinds is not None else (0,)):
            yield f"{name} mode {mode}", world, kinds, mode, None


@pytest.mark.parametrize("name,world,kinds,mode,total", list(walk_cases()), ids=[c[0] for c in walk_cases()])
def test_restated_walk_over_the_host_tree_gives_the_exact_pairs(name, world, kinds, mode, total):
    nodes, leaf_objects, _ = bvol.hierarchy_host(world)
    want = br.pairs(world, kinds, mode)[0]
    if total is not None:
        assert len(want) == total
    got = hr.walk(world, kinds, mode, nodes, leaf_objects)
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), name


def test_hand_made_cases_show_what_they_are_for():
    cases = hr.hand_made_cases()
    count = lambda name: len(br.pairs(*cases[name])[0])
    assert count("signed zero -0.0") == 0 and count("signed zero 0.0") == 1 and count("full row 77") == 149 and count("disjoint") == 0
    world, kinds = cases["nan in the middle"]
    assert not (br.pairs(world, kinds)[0] == 31).any() and (br.scene_pairs(65, 0)[0] == 31).any()
    for name in ("unbounded at the end", "unbounded in the middle"):
        world, kinds = cases[name]
        assert hr.unbounded(world).sum() == 2 and count(name) >= 2 * 63
        # the unbounded boxes sit behind every keyed box in Morton order and stay out of the frame
        _, leaf_objects, fr = bvol.hierarchy_host(world)
        assert sorted(leaf_objects[-2:].tolist()) == np.nonzero(hr.unbounded(world))[0].tolist()
        assert np.abs(fr["lower"]).max() < 100 and np.abs(fr["upper"]).max() < 100


def test_refusals():
    lib = capi.lib()
    box, key = bvol.boxes([(0, 0, 0)], [(1, 1, 1)]), C.c_uint64(0)
    assert lib.ivx_bv_morton_key(None, capi.ptr(box), 0, C.byref(key)) == capi.IVX_ERR_INVALID
    assert lib.ivx_bv_morton_key(capi.ptr(box), None, 0, C.byref(key)) == capi.IVX_ERR_INVALID
    assert lib.ivx_bv_morton_key(capi.ptr(box), capi.ptr(box), 0, None) == capi.IVX_ERR_INVALID
    world = br.scene(3)[0]
    nodes, leaves, fr = np.zeros(2, dtype=capi.BV_NODE_DTYPE), np.zeros(3, dtype=np.uint32), np.zeros(1, dtype=capi.AABB_DTYPE)
    assert lib.ivx_bv_hierarchy_host(None, 3, capi.ptr(nodes), capi.ptr(leaves), capi.ptr(fr)) == capi.IVX_ERR_INVALID
    assert lib.ivx_bv_hierarchy_host(capi.ptr(world), 3, None, capi.ptr(leaves), capi.ptr(fr)) == capi.IVX_ERR_INVALID
    assert lib.ivx_bv_hierarchy_host(capi.ptr(world), 3, capi.ptr(nodes), None, capi.ptr(fr)) == capi.IVX_ERR_INVALID
    assert lib.ivx_bv_hierarchy_host(capi.ptr(world), 3, capi.ptr(nodes), capi.ptr(leaves), None) == capi.IVX_OK  # (the frame is optional)
    assert lib.ivx_bv_hierarchy_host(capi.ptr(world), capi.BV_MAX_OBJECTS + 1, capi.ptr(nodes), capi.ptr(leaves), capi.ptr(fr)) == capi.IVX_ERR_CAPACITY
    assert lib.ivx_bv_hierarchy_host(None, 0, None, None, capi.ptr(fr)) == capi.IVX_OK and not fr.tobytes().strip(b"\0")
    # the mirror measures the arrays it is given: one short is refused before the call, and the arrays stay as they were
    for short_nodes, short_leaves in ((1, 3), (2, 2)):
        nodes, leaves = np.full(short_nodes, 7, dtype=np.uint8).repeat(32).view(capi.BV_NODE_DTYPE), np.full(short_leaves, 9, dtype=np.uint32)
        with pytest.raises(capi.IvxError) as e:
            bvol.hierarchy_host(world, nodes, leaves)
        assert e.value.code == capi.IVX_ERR_CAPACITY and np.all(leaves == 9) and np.all(nodes.view(np.uint8) == 7)
    # the device calls refuse a null context, whatever else they are given
    found = C.c_size_t(5)
    out = np.zeros((4, 2), dtype=np.uint32)
    assert lib.ivx_bv_build_hierarchy(None) == capi.IVX_ERR_INVALID
    assert lib.ivx_bv_hierarchy_download(None, None, 0, None, 0, C.byref(found)) == capi.IVX_ERR_INVALID and found.value == 0
    found = C.c_size_t(5)
    assert lib.ivx_bv_pairs_hierarchy(None, 0, capi.ptr(out), 4, C.byref(found)) == capi.IVX_ERR_INVALID and found.value == 0
    assert lib.ivx_bv_pairs_hierarchy(None, 0, capi.ptr(out), 4, None) == capi.IVX_ERR_INVALID
    assert lib.ivx_cw_set_broad_phase(None, capi.CW_BROAD_HIERARCHY) == capi.IVX_ERR_INVALID
    assert not lib.ivx_bv_device_ptr(None, capi.BV_PTR_NODES)
    with pytest.raises(ValueError):
        bvol.node_info(np.zeros(3, dtype=capi.BV_NODE_DTYPE), 4)  # (every child is node 0: not a tree)
