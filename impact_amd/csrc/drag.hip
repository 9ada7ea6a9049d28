// Detailed drag: aggregate drag loads of a triangle mesh for many directions and the equirectangular drag load map smoothed from them.
//
// Reference: impact_physics/src/force/detailed_drag.rs:200-243, 362-471 (force application, map generation),
//   detailed_drag/drag_load.rs:42-67, 174-245 (world-space load, load of a direction, triangle properties),
//   detailed_drag/equirectangular_map.rs:86-160 (cell indices, region walk), impact_geometry/src/lib.rs:59-91 (directions).
// The reference computes a map once per static mesh asset (5 000 directions x every triangle on one core) and caches it on disk; a voxel
// object, whose mesh changes with every bite, has none. Here the mesh is resident, so the map is two passes over it:
//
// LOAD PASS — relu(D x 3 . 3 x T) . T x 6, attention without a softmax. k_drag_records_* reduce every triangle once to nine floats (unit normal n,
//   f = -area n, t = (centre - com) x f; a degenerate triangle is nine zeros), so a (direction, triangle) pair is a dot product, a max and six
//   multiply-adds: c = max(0, d . n), force += c f, torque += c t. k_drag_loads: one wave per (64 directions, one tile of triangles; 256
//   directions, four to a lane, from 512 directions on); the lane keeps its directions and the accumulators in registers; the triangle record has a wave-uniform address (block index and loop counter only),
//   so it arrives by scalar loads and is broadcast to the lanes without touching LDS. A lane sums 128 triangles in f32, then adds that into
//   f64 accumulators; tiles leave f64 partials that k_drag_reduce sums in a fixed order. Nothing depends on timing: no atomics. The tiling is
//   a function of the triangle and direction counts alone. This file is checked by tolerance, not by bits: fmaf is used freely.
//
// MAP PASS — a gather: one lane per map cell walks the samples in order and, for every sample whose band of theta rows holds the cell's row,
//   walks the sample's region rows-before-columns, adding every hit (near the poles a sample meets a cell several times). That is the
//   reference's summation order for each cell, so the result is deterministic. k_drag_samples prepares per sample what all lanes would
//   otherwise recompute (angles, extent, region origin, the band of theta rows); the wave reads 64 of those records at a time, a lane each,
//   and hands a sample's values round by lane reads — as it does with the rows and columns of the sample's region.
#include <cfloat>
#include <cmath>
#include <vector>

#include "device_common.hpp"
#include "drag_internal.hpp"

namespace {

using ivx_drag::MAX_THETA;
using ivx_drag::PI_F;
using ivx_drag::TWO_PI_F;
using ivx_drag::phi_idx_of;  // the cell index arithmetic: drag_internal.hpp, shared with the force stage
using ivx_drag::theta_idx_of;

constexpr uint32_t CHUNK_TRIS = 128;     // triangles a lane sums in f32 before the sum moves into its f64 accumulators
constexpr uint32_t TARGET_WAVES = 8192;  // the triangle axis is split until about this many waves exist (256 CUs x 4 SIMDs x 8)
constexpr uint32_t WIDE_DIRS = 512;      // from this many directions on a lane holds four of them (k_drag_loads<4>)
constexpr uint32_t MAX_DIRS = 1u << 24;
constexpr float MAX_DISTANCE = 0.5f * PI_F;  // (scaled by up to 4 at the poles: a region of at most 4 n_theta + 1 cells across)

__host__ __device__ __forceinline__ float clamp_unit(float v) { return fminf(1.0f, fmaxf(-1.0f, v)); }

// ---- load pass -----------------------------------------------------------------------------------------------------------------------------
// record of triangle t: three float4 — (n.x n.y n.z 0) (f.x f.y f.z t.x) (t.y t.z 0 0): the six factors of the accumulators are three aligned pairs
__device__ __forceinline__ void write_record(float4* __restrict__ recs, size_t slot, const float* __restrict__ P, uint32_t n_vertices, uint32_t i1, uint32_t i2,
                                             uint32_t i3, float cx, float cy, float cz) {
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0;
    if (i1 < n_vertices && i2 < n_vertices && i3 < n_vertices) {
        const float ax = P[3 * (size_t)i1], ay = P[3 * (size_t)i1 + 1], az = P[3 * (size_t)i1 + 2];
        const float bx = P[3 * (size_t)i2], by = P[3 * (size_t)i2 + 1], bz = P[3 * (size_t)i2 + 2];
        const float gx = P[3 * (size_t)i3], gy = P[3 * (size_t)i3 + 1], gz = P[3 * (size_t)i3 + 2];
        const float e1x = bx - ax, e1y = by - ay, e1z = bz - az;
        const float e2x = gx - ax, e2y = gy - ay, e2z = gz - az;
        const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
        const float len = sqrtf(nx * nx + ny * ny + nz * nz);
        if (len > FLT_EPSILON) {  // (false for NaN as well)
            const float ux = nx / len, uy = ny / len, uz = nz / len;
            const float area = 0.5f * len;
            const float third = 1.0f / 3.0f;
            const float mx = third * (ax + bx + gx) - cx, my = third * (ay + by + gy) - cy, mz = third * (az + bz + gz) - cz;
            const float fx = -area * ux, fy = -area * uy, fz = -area * uz;
            r0 = make_float4(ux, uy, uz, 0.f);
            r1 = make_float4(fx, fy, fz, my * fz - mz * fy);
            r2 = make_float4(mz * fx - mx * fz, mx * fy - my * fx, 0.f, 0.f);
        }
    }
    recs[3 * slot] = r0;
    recs[3 * slot + 1] = r1;
    recs[3 * slot + 2] = r2;
}

// a caller's triangle list: one thread per triangle
__global__ __launch_bounds__(256) void k_drag_records_list(const float* __restrict__ P, uint32_t n_vertices, const uint32_t* __restrict__ idx, uint32_t n_tris, float cx,
                                                           float cy, float cz, float4* __restrict__ recs) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_tris) return;
    write_record(recs, t, P, n_vertices, idx[3 * (size_t)t], idx[3 * (size_t)t + 1], idx[3 * (size_t)t + 2], cx, cy, cz);
}

// the resident mesh: one workgroup per entry of the submesh table (grid-stride), records at the triangles' own slots of the index buffer —
// the slots of freed ranges keep the zeros they were preset to, and a zero record adds exactly nothing
__global__ __launch_bounds__(256) void k_drag_records_submeshes(const float* __restrict__ P, uint32_t n_vertices, const uint32_t* __restrict__ idx, uint32_t n_indices,
                                                                const ivx_submesh* __restrict__ sub, uint32_t n_sub, float cx, float cy, float cz,
                                                                float4* __restrict__ recs) {
    for (uint32_t s = blockIdx.x; s < n_sub; s += gridDim.x) {
        const uint32_t off = sub[s].index_offset, cnt = sub[s].index_count;
        if (off % 3u || (size_t)off + cnt > n_indices) continue;  // (never: ranges are runs of whole quads inside the buffer)
        for (uint32_t t = threadIdx.x; t < cnt / 3u; t += 256u) {
            const size_t i = (size_t)off + 3u * (size_t)t;
            write_record(recs, i / 3u, P, n_vertices, idx[i], idx[i + 1], idx[i + 2], cx, cy, cz);
        }
    }
}

// One wave per (64 ND directions, one tile of `tile_chunks` x 128 triangles): blockIdx.y = tile, wave w of block x = direction group 4 x + w,
// whose lane l holds the directions group * 64 ND + 64 q + l, q < ND. With ND = 4 a triangle's record, one scalar fetch, serves four pairs
// per lane (measured, 431 k triangles x 5 000 directions: 0.98 ms with one direction to a lane, 0.69 ms with four).
// partials[(tile * 6 + component) * d_pad + direction]
template <uint32_t ND>
__global__ __launch_bounds__(256) void k_drag_loads(const float4* __restrict__ recs, uint32_t n_tris, uint32_t tile_chunks, const float* __restrict__ dirs, uint32_t n_dirs,
                                                    uint32_t d_pad, double* __restrict__ partials) {
    const uint32_t base = (blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u * ND + (threadIdx.x & 63u);
    if ((base & ~63u) >= n_dirs) return;  // (whole waves)
    float dx[ND], dy[ND], dz[ND];
#pragma unroll
    for (uint32_t q = 0; q < ND; ++q) {
        const uint32_t dir = base + 64u * q;
        dx[q] = dy[q] = dz[q] = 0.f;
        if (dir < n_dirs) dx[q] = dirs[3 * (size_t)dir], dy[q] = dirs[3 * (size_t)dir + 1], dz[q] = dirs[3 * (size_t)dir + 2];
    }
    const uint32_t tile = blockIdx.y;
    const uint32_t t0 = tile * tile_chunks * CHUNK_TRIS;
    const uint32_t t1 = n_tris - t0 < tile_chunks * CHUNK_TRIS ? n_tris : t0 + tile_chunks * CHUNK_TRIS;
    double a[ND][6];
#pragma unroll
    for (uint32_t q = 0; q < ND; ++q)
#pragma unroll
        for (int m = 0; m < 6; ++m) a[q][m] = 0.0;
    for (uint32_t c0 = t0; c0 < t1; c0 += CHUNK_TRIS) {
        const uint32_t c1 = t1 - c0 < CHUNK_TRIS ? t1 : c0 + CHUNK_TRIS;
        float s[ND][6];
#pragma unroll
        for (uint32_t q = 0; q < ND; ++q)
#pragma unroll
            for (int m = 0; m < 6; ++m) s[q][m] = 0.f;
#pragma unroll 2
        for (uint32_t t = c0; t < c1; ++t) {
            const float4 r0 = recs[3 * (size_t)t], r1 = recs[3 * (size_t)t + 1];
            const float r2x = recs[3 * (size_t)t + 2].x, r2y = recs[3 * (size_t)t + 2].y;
#pragma unroll
            for (uint32_t q = 0; q < ND; ++q) {
                const float c = fmaxf(0.0f, fmaf(dx[q], r0.x, fmaf(dy[q], r0.y, dz[q] * r0.z)));  // only triangles that face the flow
                s[q][0] = fmaf(c, r1.x, s[q][0]);
                s[q][1] = fmaf(c, r1.y, s[q][1]);
                s[q][2] = fmaf(c, r1.z, s[q][2]);
                s[q][3] = fmaf(c, r1.w, s[q][3]);
                s[q][4] = fmaf(c, r2x, s[q][4]);
                s[q][5] = fmaf(c, r2y, s[q][5]);
            }
        }
#pragma unroll
        for (uint32_t q = 0; q < ND; ++q)
#pragma unroll
            for (int m = 0; m < 6; ++m) a[q][m] += (double)s[q][m];
    }
#pragma unroll
    for (uint32_t q = 0; q < ND; ++q) {
        const uint32_t dir = base + 64u * q;
        if (dir >= n_dirs) continue;
        double* __restrict__ p = partials + (size_t)tile * 6u * d_pad + dir;
#pragma unroll
        for (int m = 0; m < 6; ++m) p[(size_t)m * d_pad] = a[q][m];
    }
}

// Sum over the tiles in a fixed order, f64, `L` lanes per (component, direction): L = 1 walks the tiles in order (many directions, few tiles:
// consecutive threads read consecutive directions); L = 64 gives every lane the tiles lane, lane + 64, ... in order and then a fixed shuffle
// tree (few directions, thousands of tiles).
template <uint32_t L>
__global__ __launch_bounds__(256) void k_drag_reduce(const double* __restrict__ partials, uint32_t n_tiles, uint32_t d_pad, uint32_t n_dirs, float* __restrict__ out6) {
    const size_t gid = (size_t)blockIdx.x * 256u + threadIdx.x;
    const size_t sum = gid / L;
    const uint32_t sub = (uint32_t)(gid % L);
    if (sum >= 6u * (size_t)n_dirs) return;  // (whole waves when L = 64)
    const uint32_t comp = (uint32_t)(sum / n_dirs), dir = (uint32_t)(sum % n_dirs);
    double s = 0.0;
    for (uint32_t tile = sub; tile < n_tiles; tile += L) s += partials[((size_t)tile * 6u + comp) * d_pad + dir];
    if (L > 1) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    }
    if (sub == 0) out6[6 * (size_t)dir + comp] = (float)s;
}

// ---- map pass ------------------------------------------------------------------------------------------------------------------------------
struct SampleRec {  // 48 bytes
    float phi, start_phi, start_theta, inv_scaled;
    float sin_theta, cos_theta;
    uint32_t n_across, ti_lo, ti_hi;
    uint32_t pad[3];
};
static_assert(sizeof(SampleRec) == 48, "three 16-byte loads");

__global__ __launch_bounds__(256) void k_drag_samples(const float* __restrict__ dirs, uint32_t n, uint32_t n_theta, float distance, SampleRec* __restrict__ recs) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n) return;
    const float cell = PI_F / (float)n_theta, inv_cell = 1.0f / cell, half = 0.5f * cell;
    const float dx = dirs[3 * (size_t)s], dy = dirs[3 * (size_t)s + 1], dz = dirs[3 * (size_t)s + 2];
    const float phi = atan2f(dy, dx), theta = acosf(clamp_unit(dz));
    // wider towards the poles, where the map has more cells per solid angle than the samples have neighbours (by at most a factor of four)
    const float scaled = distance / (1.0f - 0.75f * fabsf(dz));
    const float ext = fmaxf(half, scaled);
    SampleRec r;
    r.phi = phi;
    r.start_phi = phi - ext + half;
    r.start_theta = theta - ext + half;
    r.inv_scaled = 1.0f / scaled;
    sincosf(theta, &r.sin_theta, &r.cos_theta);
    const float across = ceilf(2.0f * ext / cell);
    r.n_across = across > 0.0f && across < 1.0e6f ? (uint32_t)across : 0u;  // (NaN direction: no region)
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    for (uint32_t k = 0; k < r.n_across; ++k) {
        const uint32_t ti = theta_idx_of(r.start_theta + (float)k * cell, inv_cell, n_theta);
        lo = ti < lo ? ti : lo;
        hi = ti > hi ? ti : hi;
    }
    r.ti_lo = lo, r.ti_hi = hi;
    r.pad[0] = r.pad[1] = r.pad[2] = 0u;
    recs[s] = r;
}

__device__ __forceinline__ float lane_value(float v, uint32_t lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (int)lane)); }
__device__ __forceinline__ uint32_t lane_value(uint32_t v, uint32_t lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane); }

// One lane per cell (theta-major), one wave per workgroup: the 2 n_theta^2 / 64 waves spread over the compute units. The wave takes the
// samples 64 at a time — every lane loads one sample's record and load —, keeps those whose band of theta rows meets the rows of the wave's
// cells, and goes through them in order, the sample's values broadcast from the lane that holds them. For a region of up to 64 cells across,
// lane q then prepares row q and column q once (cell indices, sine and cosine, cos(phi - phi_s): what every lane would otherwise compute
// for itself, with the remainders and the argument reduction that go with it) and the walk rows-before-columns reads them from the lanes:
// a lane notes once per sample which columns fall into its cell and, in every row that does, visits just those, in ascending order.
// A wider region is walked by every lane on its own.
__global__ __launch_bounds__(64) void k_drag_map(const SampleRec* __restrict__ recs, const float* __restrict__ loads6, uint32_t n, uint32_t n_theta, float* __restrict__ map6) {
    const uint32_t lane = threadIdx.x, n_phi = 2u * n_theta, cells = n_theta * n_phi, cell_id = blockIdx.x * 64u + lane;
    const bool live = cell_id < cells;
    const uint32_t my_ti = live ? cell_id / n_phi : 0xFFFFFFFEu, my_pi = cell_id % n_phi;
    const uint32_t last_cell = blockIdx.x * 64u + 63u < cells ? blockIdx.x * 64u + 63u : cells - 1u;
    const uint32_t w_lo = blockIdx.x * 64u / n_phi, w_hi = last_cell / n_phi;  // the rows of the wave's cells
    const float cell = PI_F / (float)n_theta, inv_cell = 1.0f / cell;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f, a5 = 0.f, wsum = 0.f;
    for (uint32_t s0 = 0; s0 < n; s0 += 64u) {
        const uint32_t s = s0 + lane;
        SampleRec r;
        r.phi = r.start_phi = r.start_theta = r.inv_scaled = r.sin_theta = r.cos_theta = 0.f;
        r.n_across = 0u, r.ti_lo = 0xFFFFFFFFu, r.ti_hi = 0u;
        float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f, m5 = 0.f;
        if (s < n) {
            r = recs[s];
            m0 = loads6[6 * (size_t)s], m1 = loads6[6 * (size_t)s + 1], m2 = loads6[6 * (size_t)s + 2];
            m3 = loads6[6 * (size_t)s + 3], m4 = loads6[6 * (size_t)s + 4], m5 = loads6[6 * (size_t)s + 5];
        }
        unsigned long long todo = __ballot(r.n_across > 0u && r.ti_lo <= w_hi && r.ti_hi >= w_lo);  // the band of theta rows first
        while (todo) {
            const uint32_t i = (uint32_t)__ffsll((long long)todo) - 1u;
            todo &= todo - 1ull;
            const float phi_s = lane_value(r.phi, i), start_phi = lane_value(r.start_phi, i), start_theta = lane_value(r.start_theta, i);
            const float inv_scaled = lane_value(r.inv_scaled, i), sin_s = lane_value(r.sin_theta, i), cos_s = lane_value(r.cos_theta, i);
            const uint32_t n_across = lane_value(r.n_across, i);
            const float l0 = lane_value(m0, i), l1 = lane_value(m1, i), l2 = lane_value(m2, i), l3 = lane_value(m3, i), l4 = lane_value(m4, i), l5 = lane_value(m5, i);
            if (n_across <= 64u) {
                const float theta_q = start_theta + (float)lane * cell, phi_q = start_phi + (float)lane * cell;
                const uint32_t ti_q = theta_idx_of(theta_q, inv_cell, n_theta), pi_q = phi_idx_of(phi_q, inv_cell, n_phi);
                float st, ct;
                sincosf(theta_q, &st, &ct);
                const float ss_q = sin_s * st, cc_q = cos_s * ct, cd_q = cosf(phi_q - phi_s);
                // the columns that fall into this lane's cell, as bits (they do not depend on the row)
                unsigned long long cols = 0ull;
                for (uint32_t j = 0; j < n_across; ++j)
                    if (lane_value(pi_q, j) == my_pi) cols |= 1ull << j;
                // (control flow stays wave-uniform down to the hit itself: the lane reads below need their source lanes active)
                for (uint32_t k = 0; k < n_across; ++k) {
                    const bool row_hit = lane_value(ti_q, k) == my_ti;
                    if (!__any(row_hit)) continue;
                    const float ss = lane_value(ss_q, k), cc = lane_value(cc_q, k);
                    unsigned long long todo_cols = row_hit ? cols : 0ull;
                    while (__any(todo_cols != 0ull)) {  // ascending columns: as many rounds as the busiest cell has hits in this row
                        const bool hit = todo_cols != 0ull;
                        const int j = hit ? __ffsll((long long)todo_cols) - 1 : 0;
                        todo_cols &= todo_cols - 1ull;
                        const float cd = __shfl(cd_q, j, 64);
                        if (hit) {
                            const float x = acosf(clamp_unit(ss + cc * cd)) * inv_scaled;
                            const float q = fmaxf(0.0f, 1.0f - x * x), w = q * q;  // quartic weight with finite support
                            a0 += l0 * w, a1 += l1 * w, a2 += l2 * w, a3 += l3 * w, a4 += l4 * w, a5 += l5 * w;
                            wsum += w;
                        }
                    }
                }
            } else if (my_ti >= lane_value(r.ti_lo, i) && my_ti <= lane_value(r.ti_hi, i)) {
                for (uint32_t k = 0; k < n_across; ++k) {
                    const float theta = start_theta + (float)k * cell;
                    if (theta_idx_of(theta, inv_cell, n_theta) != my_ti) continue;
                    float st, ct;
                    sincosf(theta, &st, &ct);
                    const float ss = sin_s * st, cc = cos_s * ct;
                    for (uint32_t j = 0; j < n_across; ++j) {
                        const float phi = start_phi + (float)j * cell;
                        if (phi_idx_of(phi, inv_cell, n_phi) != my_pi) continue;
                        const float x = acosf(clamp_unit(ss + cc * cosf(phi - phi_s))) * inv_scaled;
                        const float q = fmaxf(0.0f, 1.0f - x * x), w = q * q;
                        a0 += l0 * w, a1 += l1 * w, a2 += l2 * w, a3 += l3 * w, a4 += l4 * w, a5 += l5 * w;
                        wsum += w;
                    }
                }
            }
        }
    }
    if (!live) return;
    if (wsum > 0.0f) a0 /= wsum, a1 /= wsum, a2 /= wsum, a3 /= wsum, a4 /= wsum, a5 /= wsum;
    float* __restrict__ m = map6 + 6 * (size_t)cell_id;
    m[0] = a0, m[1] = a1, m[2] = a2, m[3] = a3, m[4] = a4, m[5] = a5;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
// the context's scratch allocation (the parts of a call each on a 256-byte boundary: ivx_layout), at least 1 MiB
int ensure_scratch(ivx_ctx* c, size_t bytes) { return ivx_buf_grow(c, &c->drag_scratch, bytes, 1u << 20); }

// how the load pass tiles `n_tris` triangles for `n_dirs` directions (a function of the two counts alone)
struct LoadPlan {
    uint32_t n_tris, n_dirs, dirs_per_lane, tile_chunks, n_tiles, blocks_x, d_pad;
    size_t recs_bytes() const { return (size_t)n_tris * 48u; }
    size_t partials_bytes() const { return (size_t)n_tiles * 6u * d_pad * sizeof(double); }
};
LoadPlan plan_loads(uint32_t n_tris, uint32_t n_dirs) {
    LoadPlan p;
    p.n_tris = n_tris, p.n_dirs = n_dirs;
    p.dirs_per_lane = n_dirs >= WIDE_DIRS ? 4u : 1u;
    const uint32_t groups = (n_dirs + 64u * p.dirs_per_lane - 1u) / (64u * p.dirs_per_lane), chunks = (n_tris + CHUNK_TRIS - 1u) / CHUNK_TRIS;
    const uint32_t want = TARGET_WAVES / groups ? TARGET_WAVES / groups : 1u;
    p.tile_chunks = chunks ? (chunks + want - 1u) / want : 1u;
    p.n_tiles = chunks ? (chunks + p.tile_chunks - 1u) / p.tile_chunks : 0u;
    p.blocks_x = (groups + 3u) / 4u;
    p.d_pad = p.blocks_x * 256u * p.dirs_per_lane;
    return p;
}

// records are in place: partials, fixed-order sum, f32 loads at d_out (6 floats per direction)
int launch_loads(ivx_ctx* c, const LoadPlan& p, const float4* d_recs, const float* d_dirs, double* d_partials, float* d_out6) {
    if (p.dirs_per_lane == 4u)
        IVX_KLAUNCH(k_drag_loads<4>, dim3(p.blocks_x, p.n_tiles), dim3(256), 0, c->stream, d_recs, p.n_tris, p.tile_chunks, d_dirs, p.n_dirs, p.d_pad, d_partials);
    else
        IVX_KLAUNCH(k_drag_loads<1>, dim3(p.blocks_x, p.n_tiles), dim3(256), 0, c->stream, d_recs, p.n_tris, p.tile_chunks, d_dirs, p.n_dirs, p.d_pad, d_partials);
    const size_t sums = 6u * (size_t)p.n_dirs;
    if (p.n_tiles > 256u)
        IVX_KLAUNCH(k_drag_reduce<64>, dim3((uint32_t)((sums * 64u + 255u) / 256u)), dim3(256), 0, c->stream, (const double*)d_partials, p.n_tiles, p.d_pad, p.n_dirs, d_out6);
    else
        IVX_KLAUNCH(k_drag_reduce<1>, dim3((uint32_t)((sums + 255u) / 256u)), dim3(256), 0, c->stream, (const double*)d_partials, p.n_tiles, p.d_pad, p.n_dirs, d_out6);
    IVX_HIP_CHECK(hipGetLastError());
    return IVX_OK;
}

int launch_records_resident(ivx_grid* g, const LoadPlan& p, const float com[3], float4* d_recs) {
    ivx_ctx* c = g->ctx;
    IVX_HIP_CHECK(ivx_memset_async(d_recs, 0, p.recs_bytes(), c->stream));  // (the slots of freed ranges)
    const uint32_t n_sub = g->mesh_counts.n_submeshes;
    if (n_sub)
        IVX_KLAUNCH(k_drag_records_submeshes, dim3(n_sub < 65535u ? n_sub : 65535u), dim3(256), 0, c->stream, (const float*)g->positions, g->mesh_counts.n_vertices,
                    (const uint32_t*)g->indices, g->mesh_counts.n_indices, (const ivx_submesh*)g->submeshes, n_sub, com[0], com[1], com[2], d_recs);
    IVX_HIP_CHECK(hipGetLastError());
    return IVX_OK;
}

int launch_map(ivx_ctx* c, const float* d_dirs, const float* d_loads6, uint32_t n, uint32_t n_theta, float distance, SampleRec* d_samples, float* d_map6) {
    const uint32_t cells = 2u * n_theta * n_theta;
    IVX_KLAUNCH(k_drag_samples, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, d_dirs, n, n_theta, distance, d_samples);
    IVX_KLAUNCH(k_drag_map, dim3((cells + 63u) / 64u), dim3(64), 0, c->stream, (const SampleRec*)d_samples, d_loads6, n, n_theta, d_map6);
    IVX_HIP_CHECK(hipGetLastError());
    return IVX_OK;
}

int download(ivx_ctx* c, void* dst, const void* d_src, size_t bytes) {
    IVX_HIP_CHECK(ivx_memcpy_async(dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
    IVX_HIP_CHECK(ivx_stream_sync(c->stream));
    return IVX_OK;
}

bool finite3(const float v[3]) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

int check_map_shape(const char* who, uint32_t n_theta, float distance) {
    IVX_REQUIRE(n_theta > 0, IVX_ERR_INVALID, "%s: n_theta_coords is zero", who);
    IVX_REQUIRE(n_theta <= MAX_THETA, IVX_ERR_CAPACITY, "%s: n_theta_coords %u exceeds %u", who, n_theta, MAX_THETA);
    IVX_REQUIRE(distance > 0.0f, IVX_ERR_INVALID, "%s: the angular interpolation distance %g is not positive", who, (double)distance);
    IVX_REQUIRE(distance <= MAX_DISTANCE, IVX_ERR_INVALID, "%s: the angular interpolation distance %g exceeds pi / 2 (too few direction samples for this smoothness)", who,
                (double)distance);
    return IVX_OK;
}

void rotate(const float q[4], const float v[3], float out[3]) {  // q = (x, y, z, w), unit
    const float tx = 2.0f * (q[1] * v[2] - q[2] * v[1]), ty = 2.0f * (q[2] * v[0] - q[0] * v[2]), tz = 2.0f * (q[0] * v[1] - q[1] * v[0]);
    out[0] = v[0] + q[3] * tx + (q[1] * tz - q[2] * ty);
    out[1] = v[1] + q[3] * ty + (q[2] * tx - q[0] * tz);
    out[2] = v[2] + q[3] * tz + (q[0] * ty - q[1] * tx);
}

}  // namespace

extern "C" {

void ivx_drag_map_config_default(ivx_drag_map_config* c) {
    if (!c) return;
    c->n_direction_samples = 5000;
    c->n_theta_coords = 64;
    c->smoothness = 2.0f;
    c->reserved = 0;
}

int ivx_drag_directions(size_t n, float* dirs3) {
    IVX_REQUIRE(n > 0 && dirs3, IVX_ERR_INVALID, "ivx_drag_directions: %s", n ? "null argument" : "the number of directions is zero");
    IVX_REQUIRE(n <= MAX_DIRS, IVX_ERR_CAPACITY, "ivx_drag_directions: %zu directions exceed %u", n, MAX_DIRS);
    const float idx_norm = 1.0f / (n > 1 ? (float)(n - 1) : 1.0f);
    const float golden_angle = PI_F * (3.0f - sqrtf(5.0f));
    for (size_t i = 0; i < n; ++i) {
        const float fi = (float)i;
        const float z = 1.0f - 2.0f * fi * idx_norm;  // evenly in z
        const float r = sqrtf(fmaxf(0.0f, 1.0f - z * z));
        const float azimuth = fi * golden_angle;
        const float x = r * cosf(azimuth), y = r * sinf(azimuth);
        const float norm = sqrtf(x * x + y * y + z * z);
        dirs3[3 * i] = x / norm, dirs3[3 * i + 1] = y / norm, dirs3[3 * i + 2] = z / norm;
    }
    return IVX_OK;
}

int ivx_drag_map_indices(uint32_t n_theta, float phi, float theta, uint32_t* phi_idx, uint32_t* theta_idx) {
    IVX_REQUIRE(phi_idx && theta_idx, IVX_ERR_INVALID, "ivx_drag_map_indices: null argument");
    IVX_REQUIRE(n_theta > 0 && n_theta <= MAX_THETA, IVX_ERR_INVALID, "ivx_drag_map_indices: n_theta_coords %u is not in 1..%u", n_theta, MAX_THETA);
    IVX_REQUIRE(std::isfinite(phi) && std::isfinite(theta), IVX_ERR_INVALID, "ivx_drag_map_indices: an angle is not finite");
    const float cell = PI_F / (float)n_theta, inv_cell = 1.0f / cell;
    *phi_idx = phi_idx_of(phi, inv_cell, 2u * n_theta);
    *theta_idx = theta_idx_of(theta, inv_cell, n_theta);
    return IVX_OK;
}

int ivx_drag_force_and_torque(const ivx_drag_load* map, uint32_t n_theta, ivx_rigid_body* body, const float medium_velocity[3], float medium_mass_density,
                              float drag_coefficient, float scaling) {
    IVX_REQUIRE(map && body && medium_velocity, IVX_ERR_INVALID, "ivx_drag_force_and_torque: null argument");
    IVX_REQUIRE(n_theta > 0 && n_theta <= MAX_THETA, IVX_ERR_INVALID, "ivx_drag_force_and_torque: n_theta_coords %u is not in 1..%u", n_theta, MAX_THETA);
    float v_rel[3];
    for (int a = 0; a < 3; ++a) v_rel[a] = body->momentum[a] / body->mass - medium_velocity[a];
    const float s2 = v_rel[0] * v_rel[0] + v_rel[1] * v_rel[1] + v_rel[2] * v_rel[2];
    if (!(s2 > 0.0f)) return IVX_OK;  // at rest in the medium
    const float* q = body->orientation;
    const float q_inv[4] = {-q[0], -q[1], -q[2], q[3]};
    float v_body[3];
    rotate(q_inv, v_rel, v_body);
    const float speed = sqrtf(s2);
    const float d[3] = {v_body[0] / speed, v_body[1] / speed, v_body[2] / speed};
    IVX_REQUIRE(finite3(d), IVX_ERR_INVALID, "ivx_drag_force_and_torque: the body's velocity relative to the medium is not finite");
    const float phi = atan2f(d[1], d[0]), theta = acosf(clamp_unit(d[2]));
    const float cell = PI_F / (float)n_theta, inv_cell = 1.0f / cell;
    const ivx_drag_load& load = map[(size_t)theta_idx_of(theta, inv_cell, n_theta) * (2u * n_theta) + phi_idx_of(phi, inv_cell, 2u * n_theta)];
    // the force scales with the mesh area, the torque with the mesh extent on top of that
    const float force_scaling = scaling * scaling * medium_mass_density * drag_coefficient * s2;
    const float torque_scaling = scaling * force_scaling;
    float f[3], t[3];
    rotate(q, load.force, f);
    rotate(q, load.torque, t);
    for (int a = 0; a < 3; ++a) body->total_force[a] += force_scaling * f[a], body->total_torque[a] += torque_scaling * t[a];
    return IVX_OK;
}

int ivx_drag_loads_triangles(ivx_ctx* c, const float* positions3, size_t n_vertices, const uint32_t* indices, size_t n_indices, const float com[3], const float* dirs3,
                             size_t n_dirs, ivx_drag_load* out) {
    IVX_REQUIRE(c && com && dirs3 && out && (positions3 || n_vertices == 0) && (indices || n_indices == 0), IVX_ERR_INVALID, "ivx_drag_loads_triangles: null argument");
    IVX_REQUIRE(n_dirs > 0, IVX_ERR_INVALID, "ivx_drag_loads_triangles: the number of directions is zero");
    IVX_REQUIRE(n_dirs <= MAX_DIRS, IVX_ERR_CAPACITY, "ivx_drag_loads_triangles: %zu directions exceed %u", n_dirs, MAX_DIRS);
    IVX_REQUIRE(n_indices % 3 == 0, IVX_ERR_INVALID, "ivx_drag_loads_triangles: %zu indices are not a whole number of triangles", n_indices);
    IVX_REQUIRE(n_vertices < 0xFFFFFFFFull && n_indices < 0xFFFFFFFFull, IVX_ERR_CAPACITY, "ivx_drag_loads_triangles: mesh buffers exceed 2^32 elements");
    for (size_t i = 0; i < n_indices; ++i)
        IVX_REQUIRE(indices[i] < n_vertices, IVX_ERR_INVALID, "ivx_drag_loads_triangles: index %zu is %u, the mesh has %zu vertices", i, indices[i], n_vertices);
    ivx_many_other_context other_(c);
    if (n_indices == 0) {  // no triangles: no load
        memset(out, 0, n_dirs * sizeof(ivx_drag_load));
        return IVX_OK;
    }
    const LoadPlan p = plan_loads((uint32_t)(n_indices / 3), (uint32_t)n_dirs);
    ivx_layout l;
    const size_t o_pos = l.take(n_vertices * 12), o_idx = l.take(n_indices * 4), o_dirs = l.take(n_dirs * 12), o_recs = l.take(p.recs_bytes()),
                 o_part = l.take(p.partials_bytes()), o_out = l.take(n_dirs * sizeof(ivx_drag_load));
    if (int rc = ensure_scratch(c, l.bytes)) return rc;
    char* base = static_cast<char*>(c->drag_scratch.p);
    IVX_HIP_CHECK(ivx_memcpy_async(base + o_pos, positions3, n_vertices * 12, hipMemcpyHostToDevice, c->stream));
    IVX_HIP_CHECK(ivx_memcpy_async(base + o_idx, indices, n_indices * 4, hipMemcpyHostToDevice, c->stream));
    IVX_HIP_CHECK(ivx_memcpy_async(base + o_dirs, dirs3, n_dirs * 12, hipMemcpyHostToDevice, c->stream));
    float4* d_recs = reinterpret_cast<float4*>(base + o_recs);
    IVX_KLAUNCH(k_drag_records_list, dim3((p.n_tris + 255u) / 256u), dim3(256), 0, c->stream, (const float*)(base + o_pos), (uint32_t)n_vertices, (const uint32_t*)(base + o_idx),
                p.n_tris, com[0], com[1], com[2], d_recs);
    if (int rc = launch_loads(c, p, d_recs, reinterpret_cast<const float*>(base + o_dirs), reinterpret_cast<double*>(base + o_part), reinterpret_cast<float*>(base + o_out)))
        return rc;
    return download(c, out, base + o_out, n_dirs * sizeof(ivx_drag_load));
}

int ivx_drag_loads(ivx_grid* g, const float com[3], const float* dirs3, size_t n_dirs, ivx_drag_load* out) {
    IVX_REQUIRE(g && com && dirs3 && out, IVX_ERR_INVALID, "ivx_drag_loads: null argument");
    IVX_REQUIRE(n_dirs > 0, IVX_ERR_INVALID, "ivx_drag_loads: the number of directions is zero");
    IVX_REQUIRE(n_dirs <= MAX_DIRS, IVX_ERR_CAPACITY, "ivx_drag_loads: %zu directions exceed %u", n_dirs, MAX_DIRS);
    IVX_REQUIRE(g->mesh_valid, IVX_ERR_STATE, "ivx_drag_loads: the grid has no current mesh (call ivx_remesh or ivx_mesh_sync first)");
    ivx_ctx* c = g->ctx;
    ivx_many_other_context other_(c);
    if (g->mesh_counts.n_indices < 3) {
        memset(out, 0, n_dirs * sizeof(ivx_drag_load));
        return IVX_OK;
    }
    const LoadPlan p = plan_loads(g->mesh_counts.n_indices / 3u, (uint32_t)n_dirs);
    ivx_layout l;
    const size_t o_dirs = l.take(n_dirs * 12), o_recs = l.take(p.recs_bytes()), o_part = l.take(p.partials_bytes()), o_out = l.take(n_dirs * sizeof(ivx_drag_load));
    if (int rc = ensure_scratch(c, l.bytes)) return rc;
    char* base = static_cast<char*>(c->drag_scratch.p);
    IVX_HIP_CHECK(ivx_memcpy_async(base + o_dirs, dirs3, n_dirs * 12, hipMemcpyHostToDevice, c->stream));
    float4* d_recs = reinterpret_cast<float4*>(base + o_recs);
    if (int rc = launch_records_resident(g, p, com, d_recs)) return rc;
    if (int rc = launch_loads(c, p, d_recs, reinterpret_cast<const float*>(base + o_dirs), reinterpret_cast<double*>(base + o_part), reinterpret_cast<float*>(base + o_out)))
        return rc;
    return download(c, out, base + o_out, n_dirs * sizeof(ivx_drag_load));
}

int ivx_drag_load_map_from_samples(ivx_ctx* c, const float* dirs3, const ivx_drag_load* loads, size_t n, uint32_t n_theta, float angular_interpolation_distance,
                                   ivx_drag_load* map) {
    IVX_REQUIRE(c && dirs3 && loads && map, IVX_ERR_INVALID, "ivx_drag_load_map_from_samples: null argument");
    IVX_REQUIRE(n > 0, IVX_ERR_INVALID, "ivx_drag_load_map_from_samples: the number of direction samples is zero");
    IVX_REQUIRE(n <= MAX_DIRS, IVX_ERR_CAPACITY, "ivx_drag_load_map_from_samples: %zu samples exceed %u", n, MAX_DIRS);
    if (int rc = check_map_shape("ivx_drag_load_map_from_samples", n_theta, angular_interpolation_distance)) return rc;
    ivx_many_other_context other_(c);
    const size_t map_bytes = 2u * (size_t)n_theta * n_theta * sizeof(ivx_drag_load);
    ivx_layout l;
    const size_t o_dirs = l.take(n * 12), o_loads = l.take(n * sizeof(ivx_drag_load)), o_samples = l.take(n * sizeof(SampleRec)), o_map = l.take(map_bytes);
    if (int rc = ensure_scratch(c, l.bytes)) return rc;
    char* base = static_cast<char*>(c->drag_scratch.p);
    IVX_HIP_CHECK(ivx_memcpy_async(base + o_dirs, dirs3, n * 12, hipMemcpyHostToDevice, c->stream));
    IVX_HIP_CHECK(ivx_memcpy_async(base + o_loads, loads, n * sizeof(ivx_drag_load), hipMemcpyHostToDevice, c->stream));
    if (int rc = launch_map(c, reinterpret_cast<const float*>(base + o_dirs), reinterpret_cast<const float*>(base + o_loads), (uint32_t)n, n_theta, angular_interpolation_distance,
                            reinterpret_cast<SampleRec*>(base + o_samples), reinterpret_cast<float*>(base + o_map)))
        return rc;
    return download(c, map, base + o_map, map_bytes);
}

int ivx_drag_load_map(ivx_grid* g, const float com[3], const ivx_drag_map_config* cfg, ivx_drag_load* map) {
    IVX_REQUIRE(g && com && cfg && map, IVX_ERR_INVALID, "ivx_drag_load_map: null argument");
    float* d_map = nullptr;
    if (int rc = ivx_drag_map_build("ivx_drag_load_map", g, com, cfg, nullptr, &d_map)) return rc;
    return download(g->ctx, map, d_map, 2u * (size_t)cfg->n_theta_coords * cfg->n_theta_coords * sizeof(ivx_drag_load));
}

}  // extern "C"

// ---- the one entry that builds a map of a resident mesh (drag_internal.hpp): ivx_drag_load_map downloads what it leaves, the world keeps it ----
int ivx_drag_map_check(const char* who, const ivx_grid* g, const float com[3], const ivx_drag_map_config* cfg) {
    IVX_REQUIRE(g && com && cfg, IVX_ERR_INVALID, "%s: null argument", who);
    IVX_REQUIRE(cfg->n_direction_samples > 0, IVX_ERR_INVALID, "%s: n_direction_samples is zero", who);
    IVX_REQUIRE(cfg->n_direction_samples <= MAX_DIRS, IVX_ERR_CAPACITY, "%s: %u direction samples exceed %u", who, cfg->n_direction_samples, MAX_DIRS);
    IVX_REQUIRE(cfg->n_theta_coords > 0, IVX_ERR_INVALID, "%s: n_theta_coords is zero", who);
    IVX_REQUIRE(cfg->smoothness > 0.0f, IVX_ERR_INVALID, "%s: the smoothness %g is not positive", who, (double)cfg->smoothness);
    // (for a smoothness of one the square regions around the samples add up to the sphere's solid angle)
    const float distance = cfg->smoothness * sqrtf(4.0f * PI_F / (float)cfg->n_direction_samples);
    if (int rc = check_map_shape(who, cfg->n_theta_coords, distance)) return rc;
    IVX_REQUIRE(g->mesh_valid, IVX_ERR_STATE, "%s: the grid has no current mesh (call ivx_remesh or ivx_mesh_sync first)", who);
    return IVX_OK;
}

int ivx_drag_map_build(const char* who, ivx_grid* g, const float com[3], const ivx_drag_map_config* cfg, float* d_map, float** d_where) {
    if (int rc = ivx_drag_map_check(who, g, com, cfg)) return rc;
    const uint32_t n = cfg->n_direction_samples, n_theta = cfg->n_theta_coords;
    const float distance = cfg->smoothness * sqrtf(4.0f * PI_F / (float)n);
    ivx_ctx* c = g->ctx;
    ivx_many_other_context other_(c);
    const size_t map_bytes = 2u * (size_t)n_theta * n_theta * sizeof(ivx_drag_load);
    const bool empty = g->mesh_counts.n_indices < 3;  // zero loads average to zero
    std::vector<float> dirs;
    LoadPlan p = {};
    ivx_layout l;
    size_t o_dirs = 0, o_recs = 0, o_part = 0, o_loads = 0, o_samples = 0;
    if (!empty) {
        dirs.resize(3 * (size_t)n);
        if (int rc = ivx_drag_directions(n, dirs.data())) return rc;
        p = plan_loads(g->mesh_counts.n_indices / 3u, n);
        o_dirs = l.take((size_t)n * 12), o_recs = l.take(p.recs_bytes()), o_part = l.take(p.partials_bytes()), o_loads = l.take((size_t)n * sizeof(ivx_drag_load)),
        o_samples = l.take((size_t)n * sizeof(SampleRec));
    }
    const size_t o_map = d_map ? 0 : l.take(map_bytes);
    if (l.bytes)
        if (int rc = ensure_scratch(c, l.bytes)) return rc;
    char* base = static_cast<char*>(c->drag_scratch.p);
    float* d_out = d_map ? d_map : reinterpret_cast<float*>(base + o_map);
    if (d_where) *d_where = d_out;
    if (empty) {
        IVX_HIP_CHECK(ivx_memset_async(d_out, 0, map_bytes, c->stream));
        return IVX_OK;
    }
    IVX_HIP_CHECK(ivx_memcpy_async(base + o_dirs, dirs.data(), (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
    IVX_HIP_CHECK(ivx_stream_sync(c->stream));  // (`dirs` is pageable memory of this call)
    float4* d_recs = reinterpret_cast<float4*>(base + o_recs);
    const float* d_dirs = reinterpret_cast<const float*>(base + o_dirs);
    float* d_loads = reinterpret_cast<float*>(base + o_loads);
    if (int rc = launch_records_resident(g, p, com, d_recs)) return rc;
    if (int rc = launch_loads(c, p, d_recs, d_dirs, reinterpret_cast<double*>(base + o_part), d_loads)) return rc;
    return launch_map(c, d_dirs, d_loads, n, n_theta, distance, reinterpret_cast<SampleRec*>(base + o_samples), d_out);
}
