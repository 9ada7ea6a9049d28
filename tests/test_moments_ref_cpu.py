"""The exact restatement of the ten moments (tests/moments_ref.py) against values worked by hand, against the closed forms of a solid
chunk written out as rationals, against itself (linearity), and against the oracle's f64 moments with the general rule — the oracle is the
same integer form as the kernels summed in another order, so it is held to the rule the kernels are held to. No GPU."""
from fractions import Fraction as F

import numpy as np
import pytest

import moments_ref as mr
import oracle_lib as ol
import parity_util as pu
from impact_amd import scenes


def one_voxel_grid(cc, ijk, vtype=7):
    n = cc[0] * cc[1] * cc[2] * 4096
    flags = np.ones((cc[0] * 16, cc[1] * 16, cc[2] * 16), dtype=np.uint8)  # bit 0: empty
    types = np.full(flags.shape, 9, dtype=np.uint8)
    flags[ijk] = 0x7E  # (other flag bits are not looked at)
    types[ijk] = vtype
    assert flags.size == n
    return ol.dense_to_tiled(flags), ol.dense_to_tiled(types)


def test_one_voxel_at_the_origin_by_hand():
    """the unit cube [0,1)^3 of density 1: mass 1, int x = 1/2, int (y^2 + z^2) = 2/3, int xy = 1/4"""
    flags, types = one_voxel_grid((1, 1, 1), (0, 0, 0))
    m, n, exact = mr.moments_exact(flags, types, (1, 1, 1), np.ones(256, np.float32), 1.0)
    assert n == 1 and exact
    assert m == [1, F(1, 2), F(1, 2), F(1, 2), F(2, 3), F(2, 3), F(2, 3), F(1, 4), F(1, 4), F(1, 4)]


def test_one_voxel_at_17_3_40_by_hand():
    """the cube [17,18) x [3,4) x [40,41) in voxel units: int x = 17.5, 3.5, 40.5; int x^2 = (18^3 - 17^3)/3 = 919/3, (64 - 27)/3 = 37/3,
    (41^3 - 40^3)/3 = 4921/3. Density 3 (type 7), extent 1/2: e^3 = 1/8, e^4 = 1/16, e^5 = 1/32."""
    cc = (2, 1, 3)
    flags, types = one_voxel_grid(cc, (17, 3, 40))
    dens = np.full(256, 100.0, np.float32)
    dens[7] = 3.0
    m, n, exact = mr.moments_exact(flags, types, cc, dens, 0.5)
    assert n == 1 and exact
    d, e3, e4, e5 = 3, F(1, 8), F(1, 16), F(1, 32)
    hand = [d * e3, d * e4 * F(35, 2), d * e4 * F(7, 2), d * e4 * F(81, 2),
            d * e5 * F(37 + 4921, 3), d * e5 * F(919 + 4921, 3), d * e5 * F(919 + 37, 3),
            d * e5 * F(35 * 7, 4), d * e5 * F(7 * 81, 4), d * e5 * F(81 * 35, 4)]
    assert m == hand
    # a slab that starts one chunk in: the same voxel at local i = 1 with a chunk offset of 1
    flags1, types1 = one_voxel_grid((1, 1, 3), (1, 3, 40))
    m1, _, _ = mr.moments_exact(flags1, types1, (1, 1, 3), dens, 0.5, x_off=1)
    assert m1 == hand
    # extent 0.3 is the f32 nearest to 0.3, not 3/10; no exact case
    m3, _, exact3 = mr.moments_exact(flags, types, cc, dens, 0.3)
    e = F(float(np.float32(0.3)))
    assert e != F(3, 10) and not exact3 and m3[0] == 3 * e**3 and m3[4] == 3 * e**5 * F(37 + 4921, 3)
    # a fractional density: no exact case either
    dens[7] = 0.3
    mf, _, exactf = mr.moments_exact(flags, types, cc, dens, 0.5)
    assert not exactf and mf[0] == F(float(np.float32(0.3))) / 8


def test_solid_chunk_against_the_uniform_closed_forms():
    """a solid 16^3 chunk at chunk origin (2, 1, 3): sum_{X0}^{X0+15} (2X + 1) = 32 X0 + 256, sum (3X^2 + 3X + 1) = (X0 + 16)^3 - X0^3"""
    cc = (3, 2, 4)
    flags = np.ones((48, 32, 64), dtype=np.uint8)
    flags[32:48, 16:32, 48:64] = 0
    types = np.full(flags.shape, 4, dtype=np.uint8)
    dens = (1 + np.arange(256) % 7).astype(np.float32)
    d = int(dens[4])
    for extent in (1.0, 0.25, 0.3):
        m, n, exact = mr.moments_exact(ol.dense_to_tiled(flags), ol.dense_to_tiled(types), cc, dens, extent)
        e = F(float(np.float32(extent)))
        X0, Y0, Z0 = 32, 16, 48
        a1 = [32 * v + 256 for v in (X0, Y0, Z0)]
        a2 = [(v + 16) ** 3 - v**3 for v in (X0, Y0, Z0)]
        closed = [4096 * d * e**3] + [256 * d * a * e**4 / 2 for a in a1]
        closed += [256 * d * (a2[1] + a2[2]) * e**5 / 3, 256 * d * (a2[0] + a2[2]) * e**5 / 3, 256 * d * (a2[0] + a2[1]) * e**5 / 3]
        closed += [16 * d * a1[0] * a1[1] * e**5 / 4, 16 * d * a1[1] * a1[2] * e**5 / 4, 16 * d * a1[2] * a1[0] * e**5 / 4]
        assert n == 4096 and m == closed and exact == (extent != 0.3)
    # the same chunk as a one-chunk-wide slab at x offset 2
    sl = flags[32:48]
    ms, _, _ = mr.moments_exact(ol.dense_to_tiled(sl), ol.dense_to_tiled(types[32:48]), (1, 2, 4), dens, 0.3, x_off=2)
    assert ms == m


def test_disjoint_masks_sum_to_the_union():
    cc, sd, ty = mr.random_upload_grid(0, 0.5)
    flags = (sd >= 0).astype(np.uint8)
    rng = np.random.default_rng(1)
    a = rng.random(flags.size) < 0.3
    b = ~a & (rng.random(flags.size) < 0.5)
    dens = mr.FRAC_DENSITIES
    ma, na, _ = mr.moments_exact(flags, ty, cc, dens, 0.3, mask=a)
    mb, nb, _ = mr.moments_exact(flags, ty, cc, dens, 0.3, mask=b)
    mu, nu, _ = mr.moments_exact(flags, ty, cc, dens, 0.3, mask=a | b)
    assert na > 1000 and nb > 1000 and nu == na + nb
    assert [x + y for x, y in zip(ma, mb)] == mu
    # a dense (nx, ny, nz) mask is the tiled one
    md, nd, _ = mr.moments_exact(flags, ty, cc, dens, 0.3, mask=ol.tiled_to_dense(a, cc))
    assert md == ma and nd == na
    # nothing selected: ten zeros, and the rule wants +0.0
    mz, nz, _ = mr.moments_exact(flags, ty, cc, dens, 0.3, mask=np.zeros(flags.size, bool))
    assert nz == 0 and mz == [0] * 10
    mr.assert_moments(np.zeros(10), mz, 0, False)
    with pytest.raises(AssertionError):
        mr.assert_moments(-np.zeros(10), mz, 0, False)


def test_margin_form_gives_the_same_integers():
    cc, sd, ty = mr.random_upload_grid(3, 0.56)
    flags = (sd >= 0).astype(np.uint8)
    mask = np.random.default_rng(2).random(flags.size) < 0.7
    for m, x_off in ((None, 0), (mask, 5)):
        assert mr.integer_sums_by_margins(flags, ty, cc, m, x_off) == mr.integer_sums(flags, ty, cc, m, x_off)
    one = np.full_like(ty, 9)
    assert mr.integer_sums_by_margins(flags, one, cc) == mr.integer_sums(flags, one, cc)


def test_the_rule_sees_one_voxel():
    """what the gate is for: one dropped voxel of ~50 k, and one ulp in the exact case"""
    cc, sd, ty = mr.random_upload_grid(0, 0.5)
    flags = (sd >= 0).astype(np.uint8)
    for dens, extent in ((mr.INT_DENSITIES, 1.0), (mr.FRAC_DENSITIES, 0.3)):
        m, n, exact = mr.moments_exact(flags, ty, cc, dens, extent)
        assert n > 40000 and exact == (extent == 1.0)
        good = np.array([float(v) for v in m])
        mr.assert_moments(good, m, n, exact)
        drop = np.zeros(flags.size, bool)
        drop[np.flatnonzero(flags == 0)[-1]] = True
        m1, _, _ = mr.moments_exact(flags, ty, cc, dens, extent, mask=~drop)
        with pytest.raises(AssertionError):
            mr.assert_moments(np.array([float(v) for v in m1]), m, n, exact)
        if exact:
            for q in (0, 1, 7):
                off = good.copy()
                off[q] = np.nextafter(off[q], np.inf)
                with pytest.raises(AssertionError):
                    mr.assert_moments(off, m, n, exact)
            off = good.copy()
            off[4] = np.nextafter(off[4], np.inf)
            mr.assert_moments(off, m, n, exact)  # (one ulp of a second moment is within 2^-52)
            off[4] *= 1.0 + 2.0**-50
            with pytest.raises(AssertionError):
                mr.assert_moments(off, m, n, exact)


def _oracle_of(graph, extent):
    o = pu.oracle_from_graph(graph, extent)
    o.update_occupied_voxel_ranges()
    o.compute_all_derived_state()
    return o


def _check_oracle(o, extent, what):
    for kind, dens in mr.DENSITY_SETS.items():
        m, n, exact = mr.exact_of_oracle(o, dens, extent)
        _, o64 = o.inertia(dens)
        print("%s %s extent %g: n_terms %d exact_case %s oracle rel err %.3e" % (what, kind, extent, n, exact, mr.rel_err(o64, m)))
        mr.assert_moments(o64, m, n, exact, "%s %s %g" % (what, kind, extent))


@pytest.mark.parametrize("extent", [0.25, 1.0, 0.3])
@pytest.mark.parametrize("seed,level", [(0, 0.5), (3, 0.56), (4, 0.6)])
def test_oracle_inertia_on_random_uploads(seed, level, extent):
    cc, sd, ty = mr.random_upload_grid(seed, level)
    o = ol.OracleObject.from_dense(cc, sd, ty, extent)
    o.update_occupied_voxel_ranges()
    o.compute_all_derived_state()
    _check_oracle(o, extent, "upload seed %d" % seed)


@pytest.mark.parametrize("extent", [1.0, 0.3])
def test_oracle_inertia_on_a_sphere_with_uniform_chunks(extent):
    o = _oracle_of(scenes.sphere_scene(30.0), extent)
    info = o.export_dense()[4]
    assert np.count_nonzero(info["kind"] == 1) == 3
    _check_oracle(o, extent, "sphere")


@pytest.mark.parametrize("extent", [1.0, 0.3])
def test_oracle_inertia_on_the_asteroid(extent):
    o = _oracle_of(scenes.asteroid_scene(0.5), extent)
    info = o.export_dense()[4]
    assert (np.count_nonzero(info["kind"] == 1), np.count_nonzero(info["kind"] == 2)) == (32, 245)
    _check_oracle(o, extent, "asteroid")


@pytest.mark.parametrize("kind", ["int", "frac"])
def test_oracle_removed_moments_of_a_sphere_bite(kind):
    """removed64 of one bite against the restatement over (non-empty before) & (empty after), with the types from before"""
    dens = mr.DENSITY_SETS[kind]
    cc, sd, ty = mr.random_upload_grid(0, 0.5)
    o = ol.OracleObject.from_dense(cc, sd, ty, 1.0)
    o.update_occupied_voxel_ranges()
    o.compute_all_derived_state()
    _, typ0, flg0, _, _ = o.export_dense()
    r = o.absorb_sphere(np.array([16.5, 15.0, 17.0], np.float32), 11.0, 9.0, dens)  # across a chunk corner
    _, _, flg1, _, _ = o.export_dense()
    emptied = ((flg0 & 1) == 0) & ((flg1 & 1) != 0)
    assert int(emptied.sum()) == int(r["emptied_by_type"].sum()) > 500
    m, n, exact = mr.moments_exact(flg0, typ0, cc, dens, 1.0, mask=emptied)
    assert exact == (kind == "int")
    print("bite %s: n_terms %d oracle rel err %.3e" % (kind, n, mr.rel_err(r["removed64"], m)))
    mr.assert_moments(r["removed64"], m, n, exact, "removed64")
