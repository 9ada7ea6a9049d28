// The one range rule of the host units (impact_amd/csrc/voxel_ranges.hpp: clamped_ranges, then chunk_box) checked on the host, without the HIP
// runtime, against a transcription of the loop ivx_absorb_*_enqueue spelt out itself before the edit host code became a unit of its own:
//   voxel_ranges_check scenarios        cases written out by hand (tests/test_voxel_ranges_cpu.py runs this, and `random 200000`)
//   voxel_ranges_check random N [seed]  N random absorber boxes (spheres and capsules) and occupied ranges through both: the same hit, and on
//                                       a hit the same voxel ranges and chunk box
// Build: g++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/voxel_ranges_check.cpp -o voxel_ranges_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>

#include "../impact_amd/csrc/voxel_ranges.hpp"

// ---- what the header replaced in the edit path, with its local names: false is its "nothing touched" exit ------------------------------------
static bool old_absorb_ranges(const uint32_t occ[12], int capsule, const float center[3], const float seg[3], float influence_radius, int32_t vlo[3],
                              int32_t vhi[3], uint32_t lo[3], uint32_t cc[3]) {
    for (int d = 0; d < 3; ++d) {
        float a = center[d] - influence_radius, b = center[d] + influence_radius;  // Sphere::compute_aabb
        if (capsule) {  // Capsule::compute_aabb: the boxes of the two end spheres (capsule.rs:132-137)
            const float end = center[d] + seg[d];
            const float a1 = end - influence_radius, b1 = end + influence_radius;
            a = a1 < a ? a1 : a;
            b = b1 > b ? b1 : b;
        }
        const float fl = std::floor(a), ce = std::ceil(b);
        // `as usize` saturates at 0; the occupied ranges bound the other side
        const long s_ = fl > 0.0f ? (fl < 2.0e9f ? (long)fl : 2000000000L) : 0, e_ = ce > 0.0f ? (ce < 2.0e9f ? (long)ce : 2000000000L) : 0;
        vlo[d] = (int32_t)std::max<long>((long)occ[6 + 2 * d], s_);
        vhi[d] = (int32_t)std::min<long>((long)occ[7 + 2 * d], e_);
        if (vlo[d] >= vhi[d]) return false;
        lo[d] = (uint32_t)vlo[d] / 16u;
        cc[d] = ((uint32_t)vhi[d] + 15u) / 16u - lo[d];
    }
    return true;
}

// ---- the same absorber through the header: its box as the edit's enqueue makes it, then the two functions ------------------------------------
static bool new_absorb_ranges(const uint32_t occ[12], int capsule, const float center[3], const float seg[3], float influence_radius, int32_t vlo[3],
                              int32_t vhi[3], uint32_t lo[3], uint32_t cc[3]) {
    float lo_f[3], hi_f[3];
    for (int d = 0; d < 3; ++d) {
        float a = center[d] - influence_radius, b = center[d] + influence_radius;
        if (capsule) {
            const float end = center[d] + seg[d];
            const float a1 = end - influence_radius, b1 = end + influence_radius;
            a = a1 < a ? a1 : a;
            b = b1 > b ? b1 : b;
        }
        lo_f[d] = a, hi_f[d] = b;
    }
    long rlo[3], rhi[3];
    clamped_ranges(occ, lo_f, hi_f, true, rlo, rhi);
    return chunk_box(rlo, rhi, vlo, vhi, lo, cc);
}

static int failures = 0;
static void fail(const char* what, const uint32_t occ[12], int capsule, const float c[3], const float s[3], float r) {
    ++failures;
    printf("FAIL %s: occ [%u,%u) [%u,%u) [%u,%u) %s centre %a %a %a seg %a %a %a radius %a\n", what, occ[6], occ[7], occ[8], occ[9], occ[10], occ[11],
           capsule ? "capsule" : "sphere", c[0], c[1], c[2], s[0], s[1], s[2], r);
}
// both forms on one absorber: the same hit; on a hit the same vlo, vhi, lo, cc. Returns the hit.
static bool compare(const uint32_t occ[12], int capsule, const float c[3], const float s[3], float r) {
    int32_t vlo0[3], vhi0[3], vlo1[3], vhi1[3];
    uint32_t lo0[3], cc0[3], lo1[3], cc1[3];
    const bool hit0 = old_absorb_ranges(occ, capsule, c, s, r, vlo0, vhi0, lo0, cc0), hit1 = new_absorb_ranges(occ, capsule, c, s, r, vlo1, vhi1, lo1, cc1);
    if (hit0 != hit1) fail("hit", occ, capsule, c, s, r);
    else if (hit0 && (memcmp(vlo0, vlo1, 12) || memcmp(vhi0, vhi1, 12) || memcmp(lo0, lo1, 12) || memcmp(cc0, cc1, 12))) fail("ranges", occ, capsule, c, s, r);
    return hit1;
}
static void set_occ(uint32_t occ[12], uint32_t x0, uint32_t x1, uint32_t y0, uint32_t y1, uint32_t z0, uint32_t z1) {
    const uint32_t v[6] = {x0, x1, y0, y1, z0, z1};
    for (int i = 0; i < 6; ++i) occ[6 + i] = v[i], occ[i] = (i & 1) ? (v[i] + 15u) / 16u : v[i] / 16u;  // (the chunk ranges in front: neither form reads them)
}

// a box given by its bounds (a sphere cannot state them independently: the functions of the header directly), against expected values
struct Expect {
    bool hit;
    int32_t vlo[3], vhi[3];
    uint32_t lo[3], cc[3];
};
static void expect_box(const char* name, const uint32_t occ[12], const float lo_f[3], const float hi_f[3], bool saturate, const Expect& want) {
    long rlo[3], rhi[3];
    int32_t vlo[3], vhi[3];
    uint32_t lo[3], cc[3];
    clamped_ranges(occ, lo_f, hi_f, saturate, rlo, rhi);
    const bool hit = chunk_box(rlo, rhi, vlo, vhi, lo, cc);
    bool ok = hit == want.hit;
    if (ok && hit) ok = !memcmp(vlo, want.vlo, 12) && !memcmp(vhi, want.vhi, 12) && !memcmp(lo, want.lo, 12) && !memcmp(cc, want.cc, 12);
    if (!ok) {
        ++failures;
        printf("FAIL scenario %s (%s): hit %d, voxels [%d,%d) [%d,%d) [%d,%d), chunks %u+%u %u+%u %u+%u\n", name, saturate ? "saturating" : "plain", (int)hit, vlo[0],
               vhi[0], vlo[1], vhi[1], vlo[2], vhi[2], lo[0], cc[0], lo[1], cc[1], lo[2], cc[2]);
    }
}

static int scenarios() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    uint32_t occ[12];
    set_occ(occ, 3, 45, 16, 32, 0, 64);  // x inside chunks 0..2, y exactly chunk 1, z chunks 0..3
    const float none[3] = {0.0f, 0.0f, 0.0f};
    for (int sat = 0; sat < 2; ++sat) {
        const bool s = sat != 0;
        {  // inside the occupied ranges: floor and ceil of the bounds
            const float lo[3] = {10.5f, 17.25f, 20.0f}, hi[3] = {20.5f, 30.75f, 21.0f};
            expect_box("inside", occ, lo, hi, s, {true, {10, 17, 20}, {21, 31, 21}, {0, 1, 1}, {2, 1, 1}});
        }
        {  // straddling: clamped onto the occupied ranges on both sides
            const float lo[3] = {-5.0f, 2.0f, 60.5f}, hi[3] = {100.0f, 40.0f, 90.0f};
            expect_box("straddling", occ, lo, hi, s, {true, {3, 16, 60}, {45, 32, 64}, {0, 1, 3}, {3, 1, 1}});
        }
        {  // a bound exactly on a voxel: floor and ceil leave it; exactly on a chunk boundary: the chunk behind it is not touched
            const float lo[3] = {16.0f, 16.0f, 32.0f}, hi[3] = {32.0f, 17.0f, 48.0f};
            expect_box("on boundaries", occ, lo, hi, s, {true, {16, 16, 32}, {32, 17, 48}, {1, 1, 2}, {1, 1, 1}});
        }
        {  // one voxel past a chunk boundary on either side: both chunks
            const float lo[3] = {15.0f, 16.0f, 31.5f}, hi[3] = {17.0f, 32.0f, 32.5f};
            expect_box("across a chunk boundary", occ, lo, hi, s, {true, {15, 16, 31}, {17, 32, 33}, {0, 1, 1}, {2, 1, 2}});
        }
        {  // negative bounds and -0.0 convert to 0
            const float lo[3] = {-3.5f, -0.0f, -0.0f}, hi[3] = {4.0f, 17.0f, 0.5f};
            expect_box("negative and -0.0", occ, lo, hi, s, {true, {3, 16, 0}, {4, 17, 1}, {0, 1, 0}, {1, 1, 1}});
        }
        {  // a high bound of -0.0 or below: 0, nothing touched
            const float lo[3] = {-3.5f, 16.0f, -4.0f}, hi[3] = {4.0f, 17.0f, -0.0f};
            expect_box("high bound -0.0", occ, lo, hi, s, {false, {}, {}, {}, {}});
        }
        {  // NaN converts to 0: a NaN low bound reaches down to the occupied range, a NaN high bound touches nothing
            const float lo[3] = {nan, 16.0f, nan}, hi[3] = {4.0f, 17.0f, 3.0f};
            expect_box("NaN low bounds", occ, lo, hi, s, {true, {3, 16, 0}, {4, 17, 3}, {0, 1, 0}, {1, 1, 1}});
            const float hi2[3] = {4.0f, nan, 3.0f};
            expect_box("NaN high bound", occ, lo, hi2, s, {false, {}, {}, {}, {}});
        }
        {  // outside, and an empty range on the first, the middle or the last axis alone
            const float lo[3] = {50.0f, 40.0f, 70.0f}, hi[3] = {60.0f, 50.0f, 80.0f};
            expect_box("outside", occ, lo, hi, s, {false, {}, {}, {}, {}});
            for (int axis = 0; axis < 3; ++axis) {
                float l[3] = {10.0f, 17.0f, 20.0f}, h[3] = {20.0f, 30.0f, 21.0f};
                l[axis] = 64.0f, h[axis] = 66.0f;  // behind the occupied range of every axis
                expect_box("empty on one axis", occ, l, h, s, {false, {}, {}, {}, {}});
                l[axis] = 20.0f, h[axis] = 20.0f;  // a box without thickness on a voxel boundary
                expect_box("flat on one axis", occ, l, h, s, {false, {}, {}, {}, {}});
            }
        }
    }
    {  // +-inf and bounds above 2e9: the saturating form only (beyond 2^62 the plain conversion is undefined)
        const float lo[3] = {-inf, -inf, 2.5e9f}, hi[3] = {inf, 3.0e9f, inf};
        expect_box("infinite box", occ, lo, hi, true, {false, {}, {}, {}, {}});  // (z starts behind everything)
        const float lo2[3] = {-inf, -inf, -inf}, hi2[3] = {inf, 3.0e9f, 1.0e30f};
        expect_box("everything", occ, lo2, hi2, true, {true, {3, 16, 0}, {45, 32, 64}, {0, 1, 0}, {3, 1, 4}});
        uint32_t big[12];
        set_occ(big, 0, 4000000000u, 0, 16, 0, 16);  // occupied ranges past 2e9: the saturated bound is what is left
        const float lo3[3] = {1.9e9f, 0.0f, 0.0f}, hi3[3] = {3.9e9f, 1.0f, 1.0f};
        expect_box("saturated high bound", big, lo3, hi3, true, {true, {1900000000, 0, 0}, {2000000000, 1, 1}, {118750000u, 0, 0}, {6250000u, 1, 1}});
        const float lo4[3] = {2.5e9f, 0.0f, 0.0f};
        expect_box("saturated low bound", big, lo4, hi3, true, {false, {}, {}, {}, {}});
        // the plain form below 2^62: the conversion is exact, the int32 ranges wrap (the collidable forms have always done so)
        const float lo5[3] = {0.0f, 16.0f, 0.0f}, hi5[3] = {1.0e18f, 17.0f, 1.0f};
        expect_box("plain, far above", occ, lo5, hi5, false, {true, {3, 16, 0}, {45, 17, 1}, {0, 1, 0}, {3, 1, 1}});
    }
    // the same kinds of case as absorbers, through the transcription and the header
    const float centres[][3] = {{20.0f, 24.0f, 30.0f}, {-8.0f, 24.0f, 30.0f}, {16.0f, 16.0f, 32.0f}, {200.0f, 24.0f, 30.0f}, {20.0f, 24.0f, -0.0f},
                                {nan, 24.0f, 30.0f},   {20.0f, inf, 30.0f},   {20.0f, 24.0f, -inf},  {3.0e9f, 24.0f, 30.0f}, {20.0f, 24.0f, 2.1e9f}};
    const float segs[][3] = {{0.0f, 0.0f, 0.0f}, {30.0f, -10.0f, 5.0f}, {-inf, 0.0f, 0.0f}, {0.0f, nan, 0.0f}, {0.0f, 0.0f, 4.0e9f}};
    const float radii[] = {0.0f, 0.5f, 4.0f, 16.0f, 1000.0f, 2.5e9f, inf, nan};
    size_t hits = 0, n = 0;
    for (const auto& c : centres)
        for (const auto& sg : segs)
            for (const float r : radii)
                for (int capsule = 0; capsule < 2; ++capsule) hits += compare(occ, capsule, c, capsule ? sg : none, r), ++n;
    if (hits == 0 || hits == n) ++failures, printf("FAIL the absorber cases are one-sided: %zu hits of %zu\n", hits, n);
    if (!failures) printf("voxel ranges scenarios: ok (%zu absorbers, %zu hits)\n", n, hits);
    return failures ? 1 : 0;
}

static int random_runs(size_t n, unsigned seed) {
    std::mt19937_64 rng(seed);
    auto uni = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    const float special[] = {0.0f, -0.0f, 16.0f, 32.0f, 2.0e9f, 2.1e9f, -1.0f, std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(),
                             std::numeric_limits<float>::quiet_NaN()};
    size_t hits = 0;
    for (size_t it = 0; it < n; ++it) {
        uint32_t occ[12], r6[6];
        const uint32_t span = (rng() & 7u) == 0 ? 4000000000u : 200u;  // (now and then occupied ranges past the saturation bound)
        for (int d = 0; d < 3; ++d) {
            uint32_t a = (uint32_t)(rng() % span), b = (uint32_t)(rng() % span);
            if (a > b) std::swap(a, b);
            r6[2 * d] = a, r6[2 * d + 1] = (rng() & 15u) == 0 ? a : b + 1u;  // (now and then an empty occupied range)
        }
        set_occ(occ, r6[0], r6[1], r6[2], r6[3], r6[4], r6[5]);
        float c[3], s[3];
        for (int d = 0; d < 3; ++d) {
            const float mid = 0.5f * ((float)occ[6 + 2 * d] + (float)occ[7 + 2 * d]), w = 8.0f + (float)(occ[7 + 2 * d] - occ[6 + 2 * d]);
            c[d] = (rng() & 31u) == 0 ? special[rng() % 10u] : ((rng() & 3u) == 0 ? std::floor(uni(mid - w, mid + w)) : uni(mid - w, mid + w));
            s[d] = (rng() & 31u) == 0 ? special[rng() % 10u] : uni(-w, w);
        }
        const float r = (rng() & 31u) == 0 ? special[rng() % 10u] : ((rng() & 3u) == 0 ? std::floor(uni(0.0f, 24.0f)) : uni(0.0f, 24.0f));
        hits += compare(occ, (int)(rng() & 1u), c, s, r);
    }
    if (hits < n / 20 || hits > n - n / 20) ++failures, printf("FAIL the random absorbers are one-sided: %zu hits of %zu\n", hits, n);
    if (!failures) printf("voxel ranges random: ok (%zu absorbers, %zu hits)\n", n, hits);
    return failures ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "scenarios")) return scenarios();
    if (argc >= 3 && !strcmp(argv[1], "random")) return random_runs((size_t)strtoull(argv[2], nullptr, 10), argc >= 4 ? (unsigned)strtoul(argv[3], nullptr, 10) : 1u);
    fprintf(stderr, "usage: %s scenarios | random N [seed]\n", argv[0]);
    return 2;
}
