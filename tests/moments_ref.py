"""The ten mass moments restated exactly, and the rule a device result is held to.

TEST INFRASTRUCTURE ONLY. Independent of the kernels and of the oracle: no floating-point sum anywhere. The moments of a
set of voxels about the grid origin are integrals of 1, x, y, z, y^2 + z^2, x^2 + z^2, x^2 + y^2, xy, yz, zx over the cubes
[I e, (I + 1) e) x [J e, (J + 1) e) x [K e, (K + 1) e), times the density of the voxel's type. With

    int x dx   = e^2 (2I + 1) / 2          int x^2 dx = e^3 (3I^2 + 3I + 1) / 3

they are, per type t, ten INTEGER sums over the selected non-empty voxels of the weights

    1 | 2I+1, 2J+1, 2K+1 | cy+cz, cx+cz, cx+cy (c = 3X^2 + 3X + 1) | (2I+1)(2J+1), (2J+1)(2K+1), (2K+1)(2I+1)

times dens[t], times e^3 | e^4/2 | e^5/3 | e^5/4. The order of the ten and of the products (xy, yz, zx) is that of
impact_amd/csrc/inertia.hip. The integer sums are taken in int64 (asserted not to overflow), converted to Python ints and
carried on as fractions.Fraction of the f32 densities and the f32 extent, which are rationals.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

U = Fraction(1, 2**53)  # unit roundoff of f64
_FACTOR_KIND = (0, 1, 1, 1, 2, 2, 2, 3, 3, 3)  # e^3 | e^4/2 | e^5/3 | e^5/4
SECOND = (4, 5, 6)


def _is_pow2(x: float) -> bool:
    m, _ = np.frexp(x)
    return x > 0 and m == 0.5


def factors(extent):
    e = Fraction(float(np.float32(extent)))
    f = (e**3, e**4 / 2, e**5 / 3, e**5 / 4)
    return [f[k] for k in _FACTOR_KIND]


def integer_sums(flags, types, chunk_counts, mask=None, x_off=0):
    """-> ({type: [ten Python ints]}, n_terms). `flags`, `types`: chunk-tiled u8 (n_chunks * 4096; bit 0 of a flag = empty).
    `mask`: boolean, chunk-tiled or dense (nx, ny, nz); `x_off`: global chunk offset of the grid in x."""
    cx, cy, cz = (int(c) for c in chunk_counts)
    n = cx * cy * cz * 4096
    flags = np.asarray(flags).reshape(-1)
    types = np.asarray(types).reshape(-1)
    assert flags.size == n and types.size == n
    sel = (flags & 1) == 0
    if mask is not None:
        mask = np.asarray(mask)
        if mask.ndim == 3:
            assert mask.shape == (cx * 16, cy * 16, cz * 16)
            mask = mask.reshape(cx, 16, cy, 16, cz, 16).transpose(0, 2, 4, 1, 3, 5).reshape(-1)
        assert mask.size == n and mask.dtype == np.bool_
        sel = sel & mask.reshape(-1)
    idx = np.flatnonzero(sel).astype(np.int64)
    chunk, loc = idx >> 12, idx & 4095
    I = ((chunk // (cy * cz)) + int(x_off)) * 16 + (loc >> 8)
    J = ((chunk // cz) % cy) * 16 + ((loc >> 4) & 15)
    K = (chunk % cz) * 16 + (loc & 15)
    t = types[idx]
    # int64 cannot overflow: every sum is at most (largest weight) * (number of voxels)
    top = max((cx + int(x_off)) * 16, cy * 16, cz * 16)
    largest = max(2 * (3 * top * top + 3 * top + 1), (2 * top + 1) ** 2)
    assert largest * max(1, idx.size) < 2**63, "the int64 sums could overflow"
    qx, qy, qz = 2 * I + 1, 2 * J + 1, 2 * K + 1
    c_x, c_y, c_z = 3 * I * I + 3 * I + 1, 3 * J * J + 3 * J + 1, 3 * K * K + 3 * K + 1
    w = (None, qx, qy, qz, c_y + c_z, c_x + c_z, c_x + c_y, qx * qy, qy * qz, qz * qx)
    sums = {}
    for tt in np.unique(t):
        s = t == tt
        sums[int(tt)] = [int(np.count_nonzero(s))] + [int(w[q][s].sum(dtype=np.int64)) for q in range(1, 10)]
    return sums, int(idx.size)


def integer_sums_by_margins(flags, types, chunk_counts, mask=None, x_off=0):
    """integer_sums for grids too large to list voxel by voxel (1024^3): every weight is a product of factors of one or two of I, J, K, so the
    ten sums follow from the counts of selected voxels per I, per J, per K and per (I, J), (J, K), (K, I) — three reductions of the boolean
    grid per type, no index arrays. The same integers (test_moments_ref_cpu.py compares the two)."""
    cx, cy, cz = (int(c) for c in chunk_counts)
    n = cx * cy * cz * 4096
    flags = np.asarray(flags).reshape(-1)
    types = np.asarray(types).reshape(-1)
    assert flags.size == n and types.size == n
    sel = (flags & 1) == 0
    if mask is not None:
        mask = np.asarray(mask)
        assert mask.size == n and mask.dtype == np.bool_ and mask.ndim == 1
        sel &= mask
    present = np.flatnonzero(np.bincount(types[sel], minlength=256))
    n_terms = int(np.count_nonzero(sel))
    top = max((cx + int(x_off)) * 16, cy * 16, cz * 16)
    largest = max(2 * (3 * top * top + 3 * top + 1), (2 * top + 1) ** 2)
    assert largest * max(1, n_terms) < 2**63, "the int64 sums could overflow"
    I = np.arange(cx * 16, dtype=np.int64) + 16 * int(x_off)
    J, K = np.arange(cy * 16, dtype=np.int64), np.arange(cz * 16, dtype=np.int64)
    q = [2 * v + 1 for v in (I, J, K)]
    c = [3 * v * v + 3 * v + 1 for v in (I, J, K)]
    sums = {}
    for tt in present:
        st = (sel if len(present) == 1 else sel & (types == tt)).reshape(cx, cy, cz, 16, 16, 16)  # [ci, cj, ck, i, j, k]
        nIJ = st.sum(axis=(2, 5), dtype=np.int64).transpose(0, 2, 1, 3).reshape(cx * 16, cy * 16)
        nJK = st.sum(axis=(0, 3), dtype=np.int64).transpose(0, 2, 1, 3).reshape(cy * 16, cz * 16)
        nIK = st.sum(axis=(1, 4), dtype=np.int64).transpose(0, 2, 1, 3).reshape(cx * 16, cz * 16)
        nI, nJ, nK = nIJ.sum(1), nIJ.sum(0), nJK.sum(0)
        s1 = [int((q[a] * m).sum()) for a, m in enumerate((nI, nJ, nK))]
        s2 = [int((c[a] * m).sum()) for a, m in enumerate((nI, nJ, nK))]
        sums[int(tt)] = [int(nI.sum()), s1[0], s1[1], s1[2], s2[1] + s2[2], s2[0] + s2[2], s2[0] + s2[1],
                         int((q[0][:, None] * q[1][None, :] * nIJ).sum()), int((q[1][:, None] * q[2][None, :] * nJK).sum()),
                         int((q[0][:, None] * q[2][None, :] * nIK).sum())]
    return sums, n_terms


def moments_exact(flags, types, chunk_counts, densities, extent, mask=None, x_off=0):
    """-> (ten Fractions, n_terms, exact_case). exact_case: every density is an integer, every one of the ten integer sums times
    its densities stays below 2^53 and the extent is a power of two — then every intermediate of ANY summation in f64 is an integer
    below 2^53 and only the final scaling can round."""
    return moments_of_sums(integer_sums(flags, types, chunk_counts, mask, x_off), densities, extent)


def moments_of_sums(sums_and_count, densities, extent):
    """moments_exact from what integer_sums returned (the integer sums of one set of voxels serve every density table and extent)"""
    sums, n_terms = sums_and_count
    dens = np.asarray(densities, dtype=np.float32)
    assert dens.shape == (256,)
    tot = [Fraction(0)] * 10
    for tt, s in sums.items():
        d = Fraction(float(dens[tt]))
        assert d >= 0
        tot = [tot[q] + s[q] * d for q in range(10)]
    f = factors(extent)
    exact_case = bool(np.all(dens == np.floor(dens))) and all(v < 2**53 for v in tot) and _is_pow2(float(np.float32(extent)))
    return [tot[q] * f[q] for q in range(10)], n_terms, exact_case


def bound(exact, n_terms, exact_case, q, parts=1):
    """The largest |got - exact| assert_moments lets pass for moment q."""
    if exact_case:
        return exact * (2 + (parts - 1)) * U if q in SECOND else Fraction(0)
    return (n_terms + 64 * parts + (parts - 1)) * U * exact


def assert_moments(got, exact, n_terms, exact_case, what="", parts=1):
    """`got`: ten f64 from a device (or the oracle); `exact`, `n_terms`, `exact_case`: what moments_exact returned for the same voxels.
    Two rules, both derived, neither tuned:

    Exact case. The integer sums times integer densities are integers below 2^53 in every partial sum of every order, so nothing
    rounds before the final scaling. For the mass, the first moments and the products the factor (e^3, e^4/2, e^5/4) is a power of
    two: the result must equal the exact value bit for bit. The three second moments carry one rounding of 1/3 (relative 2^-54)
    and one of the product (2^-53): within 2^-52 relative.

    General case. |got - exact| <= (n_terms + 64) * 2^-53 * exact. All terms are non-negative. A term (density times weights) passes
    through at most three roundings before it is added, a sum of n non-negative terms in any order then has a relative error of at most
    about n u (every partial sum is at most the total, and each of the n - 1 additions rounds once), and the 64 covers the handful of
    roundings in the scaling factors of an extent that is no power of two (e^5 by four products, 1/3, the final product).

    An exact value of zero requires +0.0.

    `parts` > 1: `got` is an f64 sum of that many results, each scaled on its own (the slab protocol's host sum). Each part is within
    its own bound of its exact share, and each of the parts - 1 additions rounds once, by at most 2^-53 of a partial sum that is at most
    the total: the exact case allows (2 + parts - 1) 2^-53 on the second moments (the others stay exact: sums of integers times one power
    of two), the general case (n_terms + 64 parts + parts - 1) 2^-53."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == (10,), what
    assert np.all(np.isfinite(got)), (what, got)
    bad = []
    for q in range(10):
        g = float(got[q])
        if exact[q] == 0:
            if not (g == 0.0 and not np.signbit(g)):
                bad.append((q, g, "+0.0"))
            continue
        err = abs(Fraction(g) - exact[q])
        lim = bound(exact[q], n_terms, exact_case, q, parts)
        if err > lim:
            bad.append((q, g, float(exact[q]), "rel err %.3e > %.3e" % (float(err / exact[q]), float(lim / exact[q]))))
    assert not bad, "%s: moments off (n_terms=%d, exact_case=%s): %s" % (what, n_terms, exact_case, bad)


def rel_err(got, exact):
    """largest relative error of the ten (for printing)"""
    return max((float(abs(Fraction(float(g)) - e) / e) if e != 0 else abs(float(g))) for g, e in zip(got, exact))


INT_DENSITIES = (1 + np.arange(256) % 7).astype(np.float32)
FRAC_DENSITIES = np.random.default_rng(5).uniform(0.3, 7.9, 256).astype(np.float32)
DENSITY_SETS = {"int": INT_DENSITIES, "frac": FRAC_DENSITIES}


# ---- grids the moment tests share -------------------------------------------------------------------------------------------------
def random_upload_grid(seed, level, cc=(3, 2, 3)):
    """the grid of test_gpu_parity.test_random_dense_upload -> (cc, sdf tiled i8, type tiled u8): ragged voxels of five types, a
    solid chunk, a void chunk"""
    import oracle_lib as ol

    rng = np.random.default_rng(seed)
    blobs = rng.random((cc[0] * 16, cc[1] * 16, cc[2] * 16))
    for ax in range(3):
        blobs = 0.5 * blobs + 0.25 * (np.roll(blobs, 1, ax) + np.roll(blobs, -1, ax))
    sd = np.where(blobs > level, -128, np.where(blobs > level - 0.03, rng.integers(-60, -1, blobs.shape), rng.integers(0, 127, blobs.shape))).astype(np.int8)
    sd[16:32, :, 0:16] = -128
    sd[32:48, 16:32, 32:48] = 127
    ty = rng.integers(0, 5, blobs.shape).astype(np.uint8)
    ty[16:32, :, 0:16] = 3
    return cc, ol.dense_to_tiled(sd), ol.dense_to_tiled(ty)


def exact_of_oracle(o, densities, extent, mask=None, x_off=0):
    """moments_exact over the oracle object's voxels"""
    _, typ, flg, _, _ = o.export_dense()
    if mask is None:  # (whole objects, some of 256^3 and more: the margin form, the same integers in a tenth of the time)
        return moments_of_sums(integer_sums_by_margins(flg, typ, o.chunk_counts, None, x_off), densities, extent)
    return moments_exact(flg, typ, o.chunk_counts, densities, extent, mask, x_off)


def exact_of_device(g, densities, mask=None, x_off=None):
    """moments_exact over the bytes downloaded from a device grid (its own extent and slab offset)"""
    _, typ, flg, _, _ = g.download(sdf=False, labels=False, info=False)
    return moments_exact(flg, typ, g.chunk_counts, densities, g.voxel_extent, mask, g.x_chunk_offset if x_off is None else x_off)


def emptied_exact(flags_before, types_before, o_after, densities, extent):
    """moments_exact of what an edit removed from an oracle object: the voxels that were non-empty in the planes exported before the edit
    and are empty in `o_after`, with the types from before"""
    flags_after = o_after.export_dense()[2]
    emptied = ((flags_before & 1) == 0) & ((flags_after & 1) != 0)
    d = np.ones(256, dtype=np.float32) if densities is None else densities
    return moments_exact(flags_before, types_before, o_after.chunk_counts, d, extent, mask=emptied)
