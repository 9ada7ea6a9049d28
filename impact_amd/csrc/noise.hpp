// Gradient noise of the multifractal SDF modifier (SDF node kind 6) and of the gradient-noise voxel type generator.
//
// The reference draws both from the `simdnoise` crate, which is not a dependency of this library. The noise defined here is
// the same CONSTRUCTION (Gustavson's simplex noise, fractal Brownian motion over octaves) but not simdnoise's VALUES: a
// voxel object generated from a noisy SDF graph differs from the reference's in which voxels the perturbation moves, not in
// how the graph, its domains and margins, the per-block early-outs or the quantisation treat it.
//
// One definition for the host build, the device build and the numpy restatement of the tests (tests/noise_ref.py): every
// expression is written in one evaluation order (the comments spell it out where C++ would allow a choice), and the library
// is built with -ffp-contract=off, so the three agree bit for bit. Coordinates must satisfy |v| < 2^31 after the frequency
// is applied (the lattice index is floorf(v) as a 32-bit integer).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define IVX_NOISE_FN __host__ __device__ __forceinline__
#else
#define IVX_NOISE_FN inline
#endif

namespace ivx_noise {

// Lattice hash: h = seed ^ (i * 501125321) ^ (j * 1136930381) ^ (k * 1720413743) [^ (l * 1338594911)], u32 wrap-around, then
// h *= 0x27d4eb2d, h ^= h >> 15.
IVX_NOISE_FN uint32_t hash3(uint32_t seed, int32_t i, int32_t j, int32_t k) {
    uint32_t h = seed ^ ((uint32_t)i * 501125321u) ^ ((uint32_t)j * 1136930381u) ^ ((uint32_t)k * 1720413743u);
    h *= 0x27d4eb2du;
    return h ^ (h >> 15);
}
IVX_NOISE_FN uint32_t hash4(uint32_t seed, int32_t i, int32_t j, int32_t k, int32_t l) {
    uint32_t h = seed ^ ((uint32_t)i * 501125321u) ^ ((uint32_t)j * 1136930381u) ^ ((uint32_t)k * 1720413743u) ^ ((uint32_t)l * 1338594911u);
    h *= 0x27d4eb2du;
    return h ^ (h >> 15);
}

// g . d for the gradient h & 15 of Perlin's table: the 12 cube-edge vectors (+-1, +-1, 0), (+-1, 0, +-1), (0, +-1, +-1),
// padded to 16 by repeating (1, 1, 0), (-1, 1, 0), (0, -1, 1), (0, -1, -1). Selected by integer tests, no table: the two
// non-zero components u, v are picked as u = h < 8 ? x : y, v = h < 4 ? y : (h == 12 || h == 14 ? x : z), and the result is
// (+-u) + (+-v) (bit 0 negates u, bit 1 negates v). A sum of two terms has one rounding whatever the order.
IVX_NOISE_FN float grad3(uint32_t h, float x, float y, float z) {
    h &= 15u;
    const float u = h < 8u ? x : y;
    const float v = h < 4u ? y : ((h == 12u || h == 14u) ? x : z);
    return ((h & 1u) ? -u : u) + ((h & 2u) ? -v : v);
}
// g . d for the gradient h & 31 of the 32 standard 4D gradients (one component 0, three +-1): the zero axis is h >> 3 (x, y, z,
// w), the other three components a, b, c are taken in axis order and negated by bits 2, 1, 0. Sum ((+-a) + (+-b)) + (+-c).
IVX_NOISE_FN float grad4(uint32_t h, float x, float y, float z, float w) {
    h &= 31u;
    const uint32_t zero = h >> 3;
    const float a = zero == 0u ? y : x;
    const float b = zero <= 1u ? z : y;
    const float c = zero <= 2u ? w : z;
    return (((h & 4u) ? -a : a) + ((h & 2u) ? -b : b)) + ((h & 1u) ? -c : c);
}

// f32 constants, each rounded once: F3 = 1/3, G3 = 1/6 and its multiples 2 G3, 3 G3 (as f32 products of the rounded G3);
// F4 = (sqrt(5) - 1) / 4, G4 = (5 - sqrt(5)) / 20 and 2 G4, 3 G4, 4 G4 (f32 products of the rounded G4).
constexpr float F3 = 0.333333343f, G3 = 0.166666672f, G3_2 = 0.333333343f, G3_3 = 0.5f;
constexpr float F4 = 0.309017003f, G4 = 0.138196602f, G4_2 = 0.276393205f, G4_3 = 0.414589822f, G4_4 = 0.55278641f;

// One corner's term: t = 0.6 - ((x^2 + y^2) + z^2) [+ w^2 last in 4D]; t > 0 ? (t^2)^2 * (g . d) : 0.
IVX_NOISE_FN float corner3(uint32_t h, float x, float y, float z) {
    const float t = 0.6f - ((x * x + y * y) + z * z);
    if (!(t > 0.0f)) return 0.0f;
    const float t2 = t * t;
    return (t2 * t2) * grad3(h, x, y, z);
}
IVX_NOISE_FN float corner4(uint32_t h, float x, float y, float z, float w) {
    const float t = 0.6f - (((x * x + y * y) + z * z) + w * w);
    if (!(t > 0.0f)) return 0.0f;
    const float t2 = t * t;
    return (t2 * t2) * grad4(h, x, y, z, w);
}

// Gustavson's 3D simplex noise. Skew s = ((x + y) + z) * F3, cell i = floorf(x + s) (j, k alike), unskew t = ((i + j) + k) * G3,
// offsets x0 = x - (i - t); corner order from comparing x0, y0, z0 (x0 >= y0, y0 >= z0, x0 >= z0, as in Gustavson's paper);
// corner offsets x1 = (x0 - i1) + G3, x2 = (x0 - i2) + 2 G3, x3 = (x0 - 1) + 3 G3; result 32 * (((n0 + n1) + n2) + n3).
IVX_NOISE_FN float simplex3(float x, float y, float z, uint32_t seed) {
    const float s = ((x + y) + z) * F3;
    const float fi = floorf(x + s), fj = floorf(y + s), fk = floorf(z + s);
    const float t = ((fi + fj) + fk) * G3;
    const float x0 = x - (fi - t), y0 = y - (fj - t), z0 = z - (fk - t);
    int i1, j1, k1, i2, j2, k2;
    if (x0 >= y0) {
        if (y0 >= z0) { i1 = 1; j1 = 0; k1 = 0; i2 = 1; j2 = 1; k2 = 0; }
        else if (x0 >= z0) { i1 = 1; j1 = 0; k1 = 0; i2 = 1; j2 = 0; k2 = 1; }
        else { i1 = 0; j1 = 0; k1 = 1; i2 = 1; j2 = 0; k2 = 1; }
    } else {
        if (y0 < z0) { i1 = 0; j1 = 0; k1 = 1; i2 = 0; j2 = 1; k2 = 1; }
        else if (x0 < z0) { i1 = 0; j1 = 1; k1 = 0; i2 = 0; j2 = 1; k2 = 1; }
        else { i1 = 0; j1 = 1; k1 = 0; i2 = 1; j2 = 1; k2 = 0; }
    }
    const int32_t i = (int32_t)fi, j = (int32_t)fj, k = (int32_t)fk;
    const float x1 = (x0 - (float)i1) + G3, y1 = (y0 - (float)j1) + G3, z1 = (z0 - (float)k1) + G3;
    const float x2 = (x0 - (float)i2) + G3_2, y2 = (y0 - (float)j2) + G3_2, z2 = (z0 - (float)k2) + G3_2;
    const float x3 = (x0 - 1.0f) + G3_3, y3 = (y0 - 1.0f) + G3_3, z3 = (z0 - 1.0f) + G3_3;
    const float n0 = corner3(hash3(seed, i, j, k), x0, y0, z0);
    const float n1 = corner3(hash3(seed, i + i1, j + j1, k + k1), x1, y1, z1);
    const float n2 = corner3(hash3(seed, i + i2, j + j2, k + k2), x2, y2, z2);
    const float n3 = corner3(hash3(seed, i + 1, j + 1, k + 1), x3, y3, z3);
    return 32.0f * (((n0 + n1) + n2) + n3);
}

// Gustavson's 4D simplex noise. Skew s = (((x + y) + z) + w) * F4, unskew t = (((i + j) + k) + l) * G4; the corner order from
// the ranks of x0, y0, z0, w0 (six comparisons x>y, x>z, x>w, y>z, y>w, z>w, the greater gets the rank point); corner c (1..3)
// steps the axes of rank >= 4 - c; offsets (x0 - step) + c G4, the last corner (x0 - 1) + 4 G4; result 27 * ((((n0 + n1) + n2) +
// n3) + n4).
IVX_NOISE_FN float simplex4(float x, float y, float z, float w, uint32_t seed) {
    const float s = (((x + y) + z) + w) * F4;
    const float fi = floorf(x + s), fj = floorf(y + s), fk = floorf(z + s), fl = floorf(w + s);
    const float t = (((fi + fj) + fk) + fl) * G4;
    const float x0 = x - (fi - t), y0 = y - (fj - t), z0 = z - (fk - t), w0 = w - (fl - t);
    int rx = 0, ry = 0, rz = 0, rw = 0;
    if (x0 > y0) rx++; else ry++;
    if (x0 > z0) rx++; else rz++;
    if (x0 > w0) rx++; else rw++;
    if (y0 > z0) ry++; else rz++;
    if (y0 > w0) ry++; else rw++;
    if (z0 > w0) rz++; else rw++;
    const int32_t i = (int32_t)fi, j = (int32_t)fj, k = (int32_t)fk, l = (int32_t)fl;
    float sum = corner4(hash4(seed, i, j, k, l), x0, y0, z0, w0);
    const float gc[3] = {G4, G4_2, G4_3};
    for (int c = 1; c <= 3; ++c) {
        const int si = rx >= 4 - c, sj = ry >= 4 - c, sk = rz >= 4 - c, sl = rw >= 4 - c;
        const float g = gc[c - 1];
        sum = sum + corner4(hash4(seed, i + si, j + sj, k + sk, l + sl), (x0 - (float)si) + g, (y0 - (float)sj) + g, (z0 - (float)sk) + g,
                            (w0 - (float)sl) + g);
    }
    sum = sum + corner4(hash4(seed, i + 1, j + 1, k + 1, l + 1), (x0 - 1.0f) + G4_4, (y0 - 1.0f) + G4_4, (z0 - 1.0f) + G4_4, (w0 - 1.0f) + G4_4);
    return 27.0f * sum;
}

// Gradient-noise voxel types (GradientNoiseVoxelTypeGenerator, voxel_type.rs:125-168): one 4D noise value per candidate type, the
// fourth dimension being the type index, and the voxel takes the first type whose value is greatest.
// A voxel's coordinate along one axis: (o + (float)i) * noise_frequency, o the chunk origin's component in root space.
IVX_NOISE_FN float type_coord(float o, uint32_t i, float noise_frequency) { return (o + (float)i) * noise_frequency; }
// y, z, w: type_coord of the voxel's k, j, i (dimensions reversed, as the reference hands them to its noise builder); x = (float)t *
// voxel_type_frequency. best = v_0; for t = 1 .. n - 1: v_t > best replaces it (strict: the first maximum stays, a NaN never wins).
IVX_NOISE_FN uint32_t type_argmax4(float y, float z, float w, uint32_t n, float voxel_type_frequency, uint32_t seed) {
    float best = simplex4((float)0u * voxel_type_frequency, y, z, w, seed);
    uint32_t type = 0u;
    for (uint32_t t = 1u; t < n; ++t) {
        const float v = simplex4((float)t * voxel_type_frequency, y, z, w, seed);
        if (v > best) {
            best = v;
            type = t;
        }
    }
    return type;
}

// Fractal Brownian motion: x *= freq (y, z alike), amp = 1, sum = 0; per octave sum = sum + simplex3(x, y, z, seed) * amp, then
// x *= lacunarity (y, z alike), amp *= gain. The seed is the same for every octave.
IVX_NOISE_FN float fbm3(float x, float y, float z, uint32_t octaves, float freq, float lacunarity, float gain, uint32_t seed) {
    x = x * freq;
    y = y * freq;
    z = z * freq;
    float amp = 1.0f, sum = 0.0f;
    for (uint32_t o = 0; o < octaves; ++o) {
        sum = sum + simplex3(x, y, z, seed) * amp;
        x = x * lacunarity;
        y = y * lacunarity;
        z = z * lacunarity;
        amp = amp * gain;
    }
    return sum;
}

// Proven bounds |simplex3| <= B3, |simplex4| <= B4, for every input.
// A corner at distance r contributes |(0.6 - r^2)^4 (g . d)| <= (0.6 - r^2)^4 |g| r =: |g| h(r) when r^2 < 0.6, else 0
// (Cauchy-Schwarz; |g| = sqrt 2 for the 3D gradients, sqrt 3 for the 4D ones). On [0, sqrt 0.6] h rises to its maximum at
// r* = sqrt(0.6 / 9) (h' = (0.6 - r^2)^3 (0.6 - 9 r^2)), h(r*) = 0.0208908, and falls after it.
// The corners of a cell are the vertices of one simplex of the unskewed lattice. Its edges join the vertices v_a, v_b whose
// skewed coordinates differ in a set S of m axes: in unskewed space e_S - m G 1, of squared length m - 2 m^2 G + n m^2 G^2 in n
// dimensions — 3D (G = 1/6): 0.75, 1, 0.75 (m = 1, 2, 3); 4D (G = (5 - sqrt 5) / 20): 0.8, 1.2, 1.2, 0.8. By the triangle
// inequality r_a + r_b >= |v_a - v_b| >= the shortest edge L, so at most ONE corner lies closer than L / 2 to the point; it
// contributes at most |g| h(r*), every other one at most |g| h(L / 2) (L / 2 > r*, where h falls):
//   3D: 32 sqrt 2 (h(r*) + 3 h(sqrt 0.75 / 2)) = 45.2548 (0.0208908 + 3 * 0.0125372) = 2.6475
//   4D: 27 sqrt 3 (h(r*) + 4 h(sqrt 0.8 / 2))  = 46.7654 (0.0208908 + 4 * 0.0114487) = 3.1186
// rounded up with room for the f32 rounding of the evaluation (relative 1e-6 per operation, a few dozen operations).
constexpr float B3 = 2.65f, B4 = 3.125f;

// |fbm3| <= B3 * sum_{o < octaves} |gain|^o (f32, rounded up by the caller's slack)
IVX_NOISE_FN float fbm3_bound(uint32_t octaves, float gain) {
    float amp = 1.0f, sum = 0.0f;
    const float g = gain < 0.0f ? -gain : gain;
    for (uint32_t o = 0; o < octaves; ++o) {
        sum = sum + amp;
        amp = amp * g;
    }
    return B3 * sum;
}

}  // namespace ivx_noise
