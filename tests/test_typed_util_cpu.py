"""tests/typed_util.py pinned without a GPU: the overlay of restated noise types on the oracle generator's own planes against
voxel_type_ref.restated_planes_with_noise_types (which restates the SDF evaluation too) — the type planes are equal, and the objects
OracleObject.from_dense makes of the two sets of planes are equal after export_dense. (The sdf planes themselves may differ inside chunks the
oracle classes Void — the sphere's: 6 voxels, 123 against the Void chunk's 127 — which from_dense removes.)"""
import numpy as np
import pytest

import oracle_lib as ol
import typed_util as tu
import voxel_type_ref as vr
from impact_amd import scenes
from impact_amd.sdf_graph import SDFGraph, SDFNode


def rotated_capsule():
    g = SDFGraph()
    c = g.add_node(SDFNode.new_capsule(30.0, 9.0))
    g.set_root_node(g.add_node(SDFNode.new_rotation_from_axis_angle(c, [0.3, 0.8, 0.5], 0.9)))
    return g


CASES = {
    "sphere60": (tu.sphere60, tu.SPHERE60_NOISE),
    "rotated_capsule": (rotated_capsule, (5, 0.04, 0.8, 0xFFFFFFFF)),
    "asteroid_0.3": (lambda: scenes.asteroid_scene(0.3), (4, 0.02, 1.0, 0)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_overlay_equals_the_restated_planes(case):
    make, noise = CASES[case]
    graph = make()
    cc, sdf, typ = tu.typed_planes(graph, 1.0, noise)
    r_cc, r_sdf, r_typ = vr.restated_planes_with_noise_types(graph, *noise)
    assert tuple(cc) == tuple(r_cc)
    np.testing.assert_array_equal(typ, r_typ)
    assert len(np.unique(typ[sdf < 0])) >= 2
    a = ol.OracleObject.from_dense(cc, sdf, typ).export_dense()
    b = ol.OracleObject.from_dense(r_cc, r_sdf, r_typ).export_dense()
    for x, y, what in zip(a[:4], b[:4], ("sdf", "types", "flags", "labels")):
        np.testing.assert_array_equal(x, y, err_msg=what)
    np.testing.assert_array_equal(a[4], b[4])


def test_sphere_conditions_of_the_slab_cases():
    """what the typed slab cases of tests/test_gpu_slabs.py rely on, on the sphere of radius 60: 8^3 chunks, Uniform chunks of a non-zero
    type on the face layers of the cuts of 2, 3 and 4 slabs, several types on every cut plane, mixed-material submeshes beside every cut"""
    o = tu.typed_oracle(tu.sphere60(), 1.0, tu.SPHERE60_NOISE)
    assert o.chunk_counts == (8, 8, 8)
    info = o.export_dense()[4]
    uni = info["kind"] == 1
    assert int(uni.sum()) == 22 and set(np.unique(info["uniform_type"][uni]).tolist()) == {0, 1, 2, 3}
    for world in (2, 3, 4):
        cuts, uniform = tu.assert_slab_case_shows_types(o, world, need_uniform=True)
        assert all(len(t) >= 3 for cut in cuts for t in tu.cut_face_types(o, cut))
