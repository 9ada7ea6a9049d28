"""The NATIVE slab protocol (impact_amd/csrc/slab_comm.cpp: ivx_slabs_step_enqueue / _collect — three partial enqueues, the record kernel,
the doorbell, error flags decided on the gathered records) as separate PROCESSES, one per rank, on the one GPU a test box has: RCCL refuses
two ranks on one device, the shared-device transport (ivx_comm_init_ipc: face planes copied straight into the neighbour's receive buffer
through hipIpc handles, sequence numbers and the record gather through POSIX shared memory) does not. Every rank is a fresh Python process;
what the ranks end with is compared with the oracle on the WHOLE grid, as tests/test_gpu_slabs.py does for slabs that share a process."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import oracle_lib as ol
import typed_util as tu
from impact_amd import scenes

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("scene,world,regions", [("asteroid", 2, 1), ("fracture", 3, 8), ("typed_sphere", 3, 1)])
def test_native_protocol_as_separate_processes(scene, world, regions):
    if scene == "typed_sphere":  # (the worker builds the same scene under this name: four noise types, densities 1 + t)
        graph, dens = tu.sphere60(), tu.DENSITIES
        o = tu.typed_oracle(graph, 1.0, tu.SPHERE60_NOISE)
        tu.assert_slab_case_shows_types(o, world, need_uniform=True)
    else:
        graph = {"asteroid": scenes.asteroid_scene, "fracture": scenes.fracture_scene}[scene]()
        dens = np.linspace(0.5, 2.0, 256).astype(np.float32)
        o = ol.OracleObject.from_sdf(graph, 1.0, 0)
        o.update_occupied_voxel_ranges()
        o.compute_all_derived_state()
    with tempfile.TemporaryDirectory() as tmp:
        name = f"/ivx_ipc_{os.getpid()}_{scene}"
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "ipc_slab_worker.py"), str(r), str(world), name, scene, "2", os.path.join(tmp, f"r{r}.npz")],
                                  env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
        outs = []
        for p in procs:
            try:
                outs.append(p.communicate(timeout=300)[0])
            except subprocess.TimeoutExpired:
                for q in procs:
                    q.kill()
                raise
        assert all(p.returncode == 0 for p in procs), "\n".join(o[-3000:] for o in outs)
        ranks = [np.load(os.path.join(tmp, f"r{r}.npz")) for r in range(world)]
        # ---- against the oracle on the whole grid
        cc = o.chunk_counts
        assert tuple(ranks[0]["chunk_counts"]) == tuple(cc)
        o_sdf, o_typ, o_flg, o_lab, o_info = o.export_dense()
        per_chunk = cc[1] * cc[2]
        for d in ranks:
            x0, x1 = (int(v) for v in d["x_range"])
            sl = slice(x0 * per_chunk * 4096, x1 * per_chunk * 4096)
            np.testing.assert_array_equal(d["sdf"], o_sdf[sl])
            np.testing.assert_array_equal(d["typ"], o_typ[sl])
            np.testing.assert_array_equal(d["flg"], o_flg[sl])
            oi = o_info[x0 * per_chunk:x1 * per_chunk]
            for f in ("kind", "gen_kind", "flags", "face_dist", "uniform_type", "region_count", "boundary_region_count"):
                np.testing.assert_array_equal(d["info"][f], oi[f], err_msg=f)
        om = o.mesh()
        idx = np.concatenate([d["idx"] + np.uint32(int(d["vertex_offset"])) for d in ranks])
        np.testing.assert_array_equal(idx, om.indices)
        np.testing.assert_array_equal(np.concatenate([d["pos"] for d in ranks]).view(np.uint32), om.positions.view(np.uint32))
        np.testing.assert_array_equal(np.concatenate([d["nrm"] for d in ranks]).view(np.uint32), om.normals.view(np.uint32))
        np.testing.assert_array_equal(np.concatenate([d["im"] for d in ranks]), om.index_materials)
        assert int(ranks[0]["total_triangles"]) == om.indices.size // 3
        _, o64 = o.inertia(dens)
        for d in ranks:
            np.testing.assert_allclose(d["moments"], o64, rtol=1e-5)
            np.testing.assert_array_equal(d["moments"], ranks[0]["moments"])  # identical on every rank
            np.testing.assert_array_equal(d["occupied"], ranks[0]["occupied"])
        info = o.info()
        occ = ranks[0]["occupied"]
        assert [(int(occ[2 * k]), int(occ[2 * k + 1])) for k in range(3)] == info["occupied_chunk_ranges"]
        assert [(int(occ[6 + 2 * k]), int(occ[7 + 2 * k])) for k in range(3)] == info["occupied_voxel_ranges"]
        n_o, olab = o.region_labels()
        assert n_o == regions and all(int(d["region_count"]) == n_o for d in ranks)
        glab = []
        for d in ranks:
            loc = d["loc"]
            out = np.full(loc.shape, 0xFFFFFFFF, dtype=np.uint32)
            m = loc != 0xFFFFFFFF
            out[m] = d["region_of_local"][loc[m]]
            glab.append(out)
        glab = ol.tiled_to_dense(np.concatenate(glab), cc)
        np.testing.assert_array_equal(ol.canonicalize_labels(glab, 0xFFFFFFFF), ol.canonicalize_labels(olab, 0xFFFFFFFF))


def test_config5_1024_as_8_ranks():
    """BASELINE config 5 (the 1024^3 grid, 8 x-slabs of 8 chunk planes) through the native protocol as EIGHT ranks across process boundaries:
    four fresh processes of two ranks each (one thread and one context per rank; the GPU box allows six processes on its card), every rank's
    voxel planes and the protocol's global results against the oracle's digests of that grid (tests/golden/config5_golden.json)."""
    import json

    gold = json.load(open(os.path.join(HERE, "golden", "config5_golden.json")))
    m64 = np.array([float.fromhex(x) for x in gold["moments64"]])
    world, per_proc = 8, 2
    with tempfile.TemporaryDirectory() as tmp:
        name = f"/ivx_ipc_{os.getpid()}_config5"
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "ipc_slab_worker8.py"), str(f), str(per_proc), str(world), name, "4.2", "2",
                                   os.path.join(tmp, f"p{f}.json")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                 for f in range(0, world, per_proc)]
        outs = []
        for p in procs:
            try:
                outs.append(p.communicate(timeout=900)[0])
            except subprocess.TimeoutExpired:
                for q in procs:
                    q.kill()
                raise
        assert all(p.returncode == 0 for p in procs), "\n".join(o[-3000:] for o in outs)
        ranks = [r for f in range(0, world, per_proc) for r in json.load(open(os.path.join(tmp, f"p{f}.json")))]
    assert [r["rank"] for r in ranks] == list(range(world))
    want_occ = [x for r in gold["occupied_chunk_ranges"] for x in r] + [x for r in gold["occupied_voxel_ranges"] for x in r]
    voff = ioff = 0
    for r in ranks:
        assert r["comm"] == {"transport": "shared-device", "nranks": world, "rank": r["rank"]}
        assert r["x_range"] == [8 * r["rank"], 8 * r["rank"] + 8]
        assert r["voxel_sha"] == gold["slab_voxel_sha"][r["rank"]], f"slab {r['rank']}"
        assert r["region_count"] == gold["regions"] and r["total_triangles"] == gold["triangles"]
        assert r["occupied"] == want_occ
        assert r["moments"] == ranks[0]["moments"]  # the same bits on every rank
        assert (r["vertex_offset"], r["index_offset"]) == (voff, ioff)  # this slab's place in the concatenated mesh
        voff, ioff = voff + r["vertices"], ioff + r["indices"]
    assert voff == gold["vertices"] and ioff == 3 * gold["triangles"]
    g64 = np.array([float.fromhex(x) for x in ranks[0]["moments"]])
    assert float(np.max(np.abs(g64 - m64) / np.maximum(np.abs(m64), 1e-300))) <= 1e-5
