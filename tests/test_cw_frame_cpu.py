"""Host-side checks of the collision frame's join (impact_amd/csrc/cw_rows.hpp): `ivx_cw_to_object_space` and `ivx_cw_voxel_row` run the very functions
k_cw_rows runs, so the arithmetic and the dispatch table are checked here without a GPU — byte-equal to tests/frame_ref.py, which states both once for
every test of the project. No kernels are launched."""
import os
import subprocess

import numpy as np

import frame_ref as fr
import narrow_ref as nr
import test_frame_cpu as tf
from impact_amd import capi, collision

S, P, CAP, V = nr.SPHERE, nr.PLANE, nr.CAPSULE, nr.VOXEL
ROW = capi.CW_VOXEL_ROW_DTYPE


def body_of(world_record, bodies):
    dyn, kin = bodies
    ref = int(world_record["body"])
    return kin[ref & 0x7FFFFFFF] if ref & capi.KINEMATIC_BIT else dyn[ref]


def library_rows(world, deferred, bodies, voxel_bodies):
    """`ivx_cw_voxel_row` over the deferred pairs, the collidable indices filled in as k_cw_rows fills them"""
    rows = np.zeros(len(deferred), dtype=ROW)
    for n, (a, b) in enumerate(np.asarray(deferred).reshape(-1, 2).tolist()):
        args = []
        for i in (a, b):
            if int(world["shape"][i]) == V:
                body = body_of(world[i], bodies)
                args.append(((body["position"], body["orientation"]), collision.voxel_object_record(None, voxel_bodies[i].origin_offset, voxel_bodies[i].center_of_mass)))
            else:
                args.append((None, None))
        r = collision.voxel_row(world[a], world[b], args[0][0], args[1][0], args[0][1], args[1][1]).copy()
        assert {int(r["voxel"]), int(r["other"])} == {0, 1}
        r["voxel"], r["other"] = ((a, b)[int(r["voxel"])], (a, b)[int(r["other"])])
        rows[n] = r
    return rows


def assert_rows_are_the_dispatch(rows, world, deferred, bodies, voxel_bodies):
    """every row converts by field copies to exactly the records, generators and source order of frame_ref.dispatch"""
    want_rows, want_mutual = fr.dispatch(world, deferred, bodies, voxel_bodies)
    cq, c_source, mq, m_source = collision.row_queries(rows)
    assert c_source.tolist() == want_rows.source and m_source.tolist() == want_mutual.source
    assert cq.tobytes() == want_rows.queries.tobytes(), int(np.nonzero(cq != want_rows.queries)[0][0])
    assert mq.tobytes() == want_mutual.queries.tobytes()
    assert [fr.GENERATORS[int(g)] for g in rows["generator"]] == fr.generator_of(want_rows, want_mutual, len(rows))
    assert rows["voxel"][c_source].tolist() == want_rows.objects
    assert list(zip(rows["voxel"][m_source].tolist(), rows["other"][m_source].tolist())) == want_mutual.objects
    assert not rows["reserved"].any()
    return want_rows, want_mutual


def test_to_object_space_is_byte_equal_to_the_restatement():
    p, q, off = tf.seeded_poses()
    want_q, want_t = fr.to_object_space_f32(p, q, off)
    differing = 0
    for i in range(len(p)):
        got_q, got_t = collision.to_object_space(p[i], q[i], off[i])
        assert got_q.tobytes() == want_q[i].tobytes() and got_t.tobytes() == want_t[i].tobytes(), (i, got_q, got_t, want_q[i], want_t[i])
        q_r, t_r = fr.to_object_space_f64_rounded(q[i], p[i], off[i].astype(np.float64))
        differing += q_r.tobytes() != got_q.tobytes() or t_r.tobytes() != got_t.tobytes()
    # the witness: the float64 composition rounded once gives other bits on most poses, so a library that composed it that way would fail above
    print(f"poses on which ivx_cw_to_object_space differs from the float64 composition rounded once: {differing} of {len(p)}")
    assert differing > len(p) // 2, differing


def test_voxel_row_is_the_dispatch_over_the_static_scene():
    local, dyn, kin, voxel_bodies = fr.static_scene()
    for mode in (capi.BV_ALL_PAIRS, capi.BV_DYNAMIC_PAIRS):
        f = fr.oracle_frame(local, voxel_bodies, (dyn, kin), mode)
        world, deferred = f["world"], f["deferred"]
        assert len(deferred) >= 10
        # on the reference side: every ordered shape pair the whole-frame test of the static scene asks for occurs
        shape_pairs = {(int(world["shape"][a]), int(world["shape"][b])) for a, b in deferred.tolist()}
        assert {(S, V), (V, S), (CAP, V), (V, CAP), (V, V), (V, P)} <= shape_pairs, (mode, shape_pairs)
        rows = library_rows(world, deferred, (dyn, kin), voxel_bodies)
        want_rows, want_mutual = assert_rows_are_the_dispatch(rows, world, deferred, (dyn, kin), voxel_bodies)
        assert want_rows.queries.tobytes() == f["rows"].queries.tobytes() and want_mutual.queries.tobytes() == f["mutual"].queries.tobytes()
        assert set(fr.generator_of(want_rows, want_mutual, len(deferred))) == set(fr.GENERATORS)


def test_voxel_row_with_a_kinematic_voxel_member():
    """a voxel object that follows a KINEMATIC body, against a sphere, a plane and another voxel object on a dynamic body, in both argument orders: the
    pose is the kinematic body's, and the body references keep the kinematic bit"""
    vb = fr.voxel_body(fr.scenes.sphere_scene(12.0), 0.5)
    other = fr.VoxelBody(vb.o, vb.graph, vb.extent, vb.densities, vb.mesh, vb.probe_state, vb.center_of_mass + np.float32(0.25), vb.origin_offset - np.float32(0.5))
    dyn = np.array([nr.unit_body((3.0, -1.0, 2.0), fr.axis_angle((0.3, -1.0, 0.5), 0.9)), nr.unit_body((-2.0, 0.5, 1.0), fr.axis_angle((1.0, 0.2, 0.0), 0.4))],
                   dtype=capi.RIGID_BODY_DTYPE)
    kin = fr.static_kinematic(2)
    kin["position"][1], kin["orientation"][1] = (1.5, 2.5, -0.75), fr.axis_angle((0.1, 0.3, 1.0), -0.5)
    local = np.array([fr.voxel_collidable(vb.o, vb.origin_offset, 1, 300, response=(0.3, 0.6, 0.4), kinematic=True),
                      collision.sphere((0.5, 0.0, 0.25), 0.75, 0, 301, response=(0.1, 0.2, 0.9)),
                      fr.voxel_collidable(other.o, other.origin_offset, 1, 302, response=(0.5, 0.4, 0.8)),
                      collision.plane((0, 1, 0), 0.25, 0, 303, response=(0.7, 0.5, 0.3), kinematic=True)], dtype=capi.COLLIDABLE_DTYPE)
    voxel_bodies = {0: vb, 2: other}
    world, _ = nr.transform(local, *nr.body_frames(local, dyn, kin))
    deferred = np.array([(0, 1), (1, 0), (0, 2), (2, 0), (0, 3), (3, 0)], dtype=np.uint32)
    rows = library_rows(world, deferred, (dyn, kin), voxel_bodies)
    want_rows, want_mutual = assert_rows_are_the_dispatch(rows, world, deferred, (dyn, kin), voxel_bodies)
    # the kinematic body's pose, not dynamic body 1's, and its reference with the bit
    want_q, want_t = fr.to_object_space_f32(kin[1]["position"], kin[1]["orientation"], vb.origin_offset)
    wrong_q, wrong_t = fr.to_object_space_f32(dyn[1]["position"], dyn[1]["orientation"], vb.origin_offset)
    assert want_t.tobytes() != wrong_t.tobytes()
    kinematic_ref = 1 | capi.KINEMATIC_BIT
    for r in rows[[0, 1, 4, 5]]:
        assert r["rotation_a"].tobytes() == want_q.tobytes() and r["translation_a"].tobytes() == want_t.tobytes()
    assert [int(r["body_b"]) for r in rows[[0, 1]]] == [kinematic_ref] * 2 and [int(r["body_a"]) for r in rows[[4, 5]]] == [kinematic_ref] * 2
    assert int(rows[2]["body_a"]) == kinematic_ref and int(rows[3]["body_b"]) == kinematic_ref
    assert rows[2]["translation_a"].tobytes() == want_t.tobytes() and rows[3]["translation_b"].tobytes() == want_t.tobytes()
    assert rows[2]["center_of_mass_b"].tobytes() == other.center_of_mass.tobytes() and rows[3]["center_of_mass_a"].tobytes() == other.center_of_mass.tobytes()
    assert len(want_rows.queries) == 4 and len(want_mutual.queries) == 2


def test_voxel_row_refuses_what_is_no_deferred_pair():
    sphere, plane = collision.sphere((0, 0, 0), 1.0, 0, 1), collision.plane((0, 1, 0), 0.0, 0, 2)
    voxel = collision.voxel_object((0, 0, 0), (1, 1, 1), 0, 3)
    record = collision.voxel_object_record(None, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
    pose = ((0, 0, 0), (0, 0, 0, 1))
    for call in (lambda: collision.voxel_row(sphere, plane), lambda: collision.voxel_row(voxel, sphere), lambda: collision.voxel_row(voxel, sphere, pose_a=pose),
                 lambda: collision.voxel_row(sphere, voxel, pose_a=pose, voxel_a=record)):
        try:
            call()
        except capi.IvxError as e:
            assert e.code == capi.IVX_ERR_INVALID
        else:
            raise AssertionError("accepted")
    assert int(collision.voxel_row(voxel, sphere, pose_a=pose, voxel_a=record)["generator"]) == 0


def test_the_frame_records_by_the_c_compiler(tmp_path):
    fields = ["generator", "voxel", "other", "reserved", "collidable_id_a", "collidable_id_b", "body_a", "body_b", "response", "shape1", "shape3", "shape3b", "rotation_a",
              "translation_a", "center_of_mass_a", "rotation_b", "translation_b", "center_of_mass_b"]
    object_fields = ["grid", "origin_offset", "center_of_mass"]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "impact_voxel_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu\\n", sizeof(struct ivx_cw_voxel_row), sizeof(ivx_cw_voxel_object));\n' +
                   "".join(f'    printf("%zu\\n", offsetof(struct ivx_cw_voxel_row, {f}));\n' for f in fields) +
                   "".join(f'    printf("%zu\\n", offsetof(ivx_cw_voxel_object, {f}));\n' for f in object_fields) + "    return 0;\n}\n")
    exe = tmp_path / "size"
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.run(["gcc", "-I", inc, str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:2] == [160, 32] == [ROW.itemsize, capi.CW_VOXEL_OBJECT_DTYPE.itemsize] and ROW.itemsize % 8 == 0
    assert got[2:2 + len(fields)] == [ROW.fields[f][1] for f in fields] == [0, 4, 8, 12, 16, 24, 32, 36, 40, 52, 56, 68, 80, 96, 108, 120, 136, 148]
    assert got[2 + len(fields):] == [capi.CW_VOXEL_OBJECT_DTYPE.fields[f][1] for f in object_fields] == [0, 8, 20]
    sizes = capi.extra_struct_sizes()
    assert sizes["ivx_cw_voxel_row"] == (ROW, 160) and sizes["ivx_cw_voxel_object"] == (capi.CW_VOXEL_OBJECT_DTYPE, 32)
    for name in ("ivx_cw_to_object_space", "ivx_cw_voxel_row", "ivx_cw_set_voxel_objects", "ivx_cw_collide_frame", "ivx_cw_rows_download"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(capi.lib(), name)
    # every field of the two query records has its source in the row: the conversion is field copies and nothing else
    assert set(capi.COLLIDABLE_QUERY_DTYPE.names) - {"mode", "rotation_xyzw", "translation", "reserved"} <= set(ROW.names)
    assert set(capi.MUTUAL_QUERY_DTYPE.names) - {"a", "b", "reserved"} <= set(ROW.names)
