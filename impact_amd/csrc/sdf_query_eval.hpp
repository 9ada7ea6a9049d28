// SDF queries: the arithmetic the host exports and the kernels of sdf_query.hip both run (f32, one evaluation order per expression; the files
// that include this are compiled without contraction).
//
// Reference: impact_voxel/src/generation/sdf/atomic.rs:877-1010 (compute_signed_distances_for_block_preserving_gradients, compute_signed_distance),
//   :1423-1507 (noise over a block), :1601-1660 (block positions); generation/sdf/meta.rs:2411-2770 (the three placements and
//   sample_signed_distance_with_gradient); impact_geometry/src/axis_aligned_box.rs:420-455; impact_math/src/transform/similarity.rs:206-242.
//
// One evaluation of the program gives ONE sample of a block: corner (ci, cj, ck) of the 2x2x2 block, or the single sample of the 1x1x1 block
// ((0, 0, 0)). The value stack is a column `st[level * stride]`: the host passes an array of its own (stride 1), a kernel its lane's column of
// LDS (stride = lanes of the workgroup). The eight corners of a block are eight evaluations on the host and the eight lanes of an instance on
// the device (Sampler::corners): everything behind them — the sums, the placements — is the same code.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/impact_voxel_hip.h"
#include "noise.hpp"
#include "vec3.hpp"

namespace ivx_sq {

using namespace ivx_vec;

#define SQ_HD __host__ __device__ __forceinline__

constexpr float SQ_MAX_F32 = 0.02f * 127.0f;  // VoxelSignedDistance::MAX_F32 (lib.rs:155-158)
constexpr float SQ_EPS = 1e-8f;

SQ_HD bool sign_bit(float v) {
#ifdef __HIP_DEVICE_COMPILE__
    return (__float_as_uint(v) >> 31) != 0u;
#else
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u >> 31) != 0u;
#endif
}
SQ_HD float u2f(uint32_t u) {
#ifdef __HIP_DEVICE_COMPILE__
    return __uint_as_float(u);
#else
    float f;
    memcpy(&f, &u, 4);
    return f;
#endif
}
// the first operand wins only when strictly smaller / larger (the restatement's minimum / maximum; no NaN reaches these)
SQ_HD float qmin(float a, float b) { return a < b ? a : b; }
SQ_HD float qmax(float a, float b) { return a > b ? a : b; }
// f32::max / f32::min of find_ray_intersection: a NaN operand (0 * inf on a slab face) loses
SQ_HD float rmax(float a, float b) { return b != b ? a : (a != a ? b : (a > b ? a : b)); }
SQ_HD float rmin(float a, float b) { return b != b ? a : (a != a ? b : (a < b ? a : b)); }

// glam Mat4::transform_point3a: ((c0 x + c1 y) + c2 z) + c3
SQ_HD V3 xform_point(const float* m, V3 p) {
    V3 r = mk(m[0], m[1], m[2]) * p.x;
    r = mk(m[4], m[5], m[6]) * p.y + r;
    r = mk(m[8], m[9], m[10]) * p.z + r;
    return mk(m[12], m[13], m[14]) + r;
}

// sphere a = r | capsule a = half segment, b = r | box a, b, c = half extents
SQ_HD float leaf_value(uint32_t kind, float a, float b, float c, V3 p) {
    if (kind <= 1u) {
        float y = p.y, r = a;
        if (kind == 1u) {
            y = y - qmin(qmax(y, -a), a);
            r = b;
        }
        return sqrtf((p.x * p.x + y * y) + p.z * p.z) - r;
    }
    const float qx = fabsf(p.x) - a, qy = fabsf(p.y) - b, qz = fabsf(p.z) - c;
    const float px = qmax(qx, 0.0f), py = qmax(qy, 0.0f), pz = qmax(qz, 0.0f);
    return sqrtf((px * px + py * py) + pz * pz) + qmin(qmax(qmax(qx, qy), qz), 0.0f);
}

// generation/sdf.rs:89-92 and the three combinations (a = smoothness, b = 0.25 / smoothness)
SQ_HD float smooth_union(float d1, float d2, float s, float q) {
    const float h = qmax(s - fabsf(d1 - d2), 0.0f);
    return qmin(d1, d2) - (h * h) * q;
}
SQ_HD float combine(uint32_t kind, float a, float b, float s, float q) {
    if (kind == 7u) return s == 0.0f ? qmin(a, b) : smooth_union(a, b, s, q);
    if (kind == 8u) return s == 0.0f ? qmax(a, -b) : -smooth_union(-a, b, s, q);
    return s == 0.0f ? qmax(a, b) : -smooth_union(-a, -b, s, q);
}

// modify_signed_distances_for_block (atomic.rs:1423-1507) for one sample of the block: the frame and the `rotated` test of the sampler's
// noise_frame / noise_at (sdf_sample.hip), the parameters in the public form (reserved[0] persistence, [1] octaves, [2] seed)
SQ_HD float noise_value(const ivx_sdf_processed_node& nd, V3 origin_root, uint32_t ci, uint32_t cj, uint32_t ck) {
    const float* m = nd.transform;
    const V3 on = xform_point(m, origin_root);
    const V3 dx = mk(m[0], m[1], m[2]), dy = mk(m[4], m[5], m[6]), dz = mk(m[8], m[9], m[10]);
    const float inverse_scale = sqrtf(dot(dx, dx));
    const float sc = 1.0f / inverse_scale;
    const float freq = nd.b * inverse_scale;
    const V3 o = on * sc;
    const float gain = u2f(nd.reserved[0]);
    const uint32_t octaves = nd.reserved[1], seed = nd.reserved[2];
    const bool rotated = !(fabsf(dx.x * inverse_scale - 1.0f) <= 1e-6f) || !(fabsf(dy.y * inverse_scale - 1.0f) <= 1e-6f);
    float nz;
    if (!rotated) {  // block path: offset + index, one rounding each; dimensions reversed
        nz = ivx_noise::fbm3(o.z + (float)ck, o.y + (float)cj, o.x + (float)ci, octaves, freq, nd.c, gain, seed);
    } else {  // per-voxel path: (o + i dx) + j dy, then += dz voxel by voxel
        V3 pos = (o + (dx * sc) * (float)ci) + (dy * sc) * (float)cj;
        if (ck) pos = pos + dz * sc;
        nz = ivx_noise::fbm3(pos.z, pos.y, pos.x, octaves, freq, nd.c, gain, seed);
    }
    return nz * nd.a;
}

struct Program {
    const ivx_sdf_processed_node* nodes;  // (the kernels read them at wave-uniform indices: scalar loads)
    uint32_t n, stack_size;
};

// One sample of the block at `origin_root`. ivx_sdf_query_create has walked the list (every depth within 1 .. stack_size, one value left); the
// walk here tests its depth all the same and leaves a level it may not touch alone — no stack is indexed on trust.
SQ_HD float eval_sample(const Program& pr, float* st, uint32_t stride, V3 origin_root, uint32_t ci, uint32_t cj, uint32_t ck) {
    if (pr.n == 0u) return SQ_MAX_F32;
    uint32_t top = 0u;
    for (uint32_t i = 0; i < pr.n; ++i) {
        const ivx_sdf_processed_node& nd = pr.nodes[i];
        const uint32_t kind = nd.kind;
        if (kind <= 2u) {
            if (top >= pr.stack_size) continue;
            const float* m = nd.transform;
            const V3 origin = xform_point(m, origin_root);
            V3 pos = (origin + mk(m[0], m[1], m[2]) * (float)ci) + mk(m[4], m[5], m[6]) * (float)cj;
            if (ck) pos = pos + mk(m[8], m[9], m[10]);
            st[top * stride] = leaf_value(kind, nd.a, nd.b, nd.c, pos);
            ++top;
        } else if (kind == 5u) {
            if (top >= 1u) st[(top - 1u) * stride] = st[(top - 1u) * stride] * nd.a;
        } else if (kind == 6u) {
            if (top >= 1u) st[(top - 1u) * stride] = st[(top - 1u) * stride] + noise_value(nd, origin_root, ci, cj, ck);
        } else if (kind >= 7u) {
            if (top < 2u) continue;
            --top;
            st[(top - 1u) * stride] = combine(kind, st[(top - 1u) * stride], st[top * stride], nd.a, nd.b);
        }
    }
    return top >= 1u ? st[0] : SQ_MAX_F32;
}

// A sampler: the program and the lane's (or the host call's) stack column. `corners` fills d[0..8) with the samples of the 2x2x2 block at
// `origin`, in i*4 + j*2 + k order.
struct Sampler {
    Program pr;
    float* st;
    uint32_t stride;
    uint32_t corner;  // device: the corner this lane evaluates (lane & 7)

    SQ_HD void corners(V3 origin, float d[8]) const {
#ifdef __HIP_DEVICE_COMPILE__
        const float v = eval_sample(pr, st, stride, origin, (corner >> 2) & 1u, (corner >> 1) & 1u, corner & 1u);
#pragma unroll
        for (int c = 0; c < 8; ++c) d[c] = __shfl(v, c, 8);  // (the eight lanes of an instance run together: all active or none)
#else
        for (uint32_t c = 0; c < 8u; ++c) d[c] = eval_sample(pr, st, stride, origin, (c >> 2) & 1u, (c >> 1) & 1u, c & 1u);
#endif
    }
    // compute_signed_distance (the 1x1x1 block; on the device the lanes of an instance all compute it)
    SQ_HD float value(V3 p) const { return eval_sample(pr, st, stride, p, 0u, 0u, 0u); }
    // sample_signed_distance_with_gradient (meta.rs:2728-2770)
    SQ_HD void gradient(V3 p, float* value_out, V3* grad) const {
        float d[8];
        corners(mk(p.x - 0.5f, p.y - 0.5f, p.z - 0.5f), d);
        *value_out = (((((((d[0] + d[1]) + d[2]) + d[3]) + d[4]) + d[5]) + d[6]) + d[7]) * 0.125f;
        const float gx = (((d[4] + d[6]) + d[5]) + d[7]) - (((d[0] + d[2]) + d[1]) + d[3]);
        const float gy = (((d[2] + d[6]) + d[3]) + d[7]) - (((d[0] + d[4]) + d[1]) + d[5]);
        const float gz = (((d[1] + d[5]) + d[3]) + d[7]) - (((d[0] + d[4]) + d[2]) + d[6]);
        *grad = mk(0.25f * gx, 0.25f * gy, 0.25f * gz);
    }
};

// ---- similarities (similarity.rs:206-242) ----------------------------------------------------------------------------------------------------
SQ_HD V3 sim_point(const ivx_similarity& s, V3 p) { return qrot(s.rotation, p * s.scaling) + ld3(s.translation); }
SQ_HD V3 sim_vector(const ivx_similarity& s, V3 v) { return qrot(s.rotation, v * s.scaling); }
SQ_HD V3 conj_rot(const ivx_similarity& s, V3 v) {
    const float q[4] = {-s.rotation[0], -s.rotation[1], -s.rotation[2], s.rotation[3]};
    return qrot(q, v);
}
SQ_HD V3 sim_inv_point(const ivx_similarity& s, V3 p) { return conj_rot(s, p - ld3(s.translation)) * (1.0f / s.scaling); }
SQ_HD V3 sim_inv_vector(const ivx_similarity& s, V3 v) { return conj_rot(s, v) * (1.0f / s.scaling); }
// UnitVector3::normalized_from_if_above(v, 1e-8) (impact_math/src/vector.rs:1163-1173)
SQ_HD bool unit_if_above(V3 v, V3* out) {
    const float n2 = dot(v, v);
    if (!(n2 > SQ_EPS * SQ_EPS)) return false;
    const float n = sqrtf(n2);
    *out = mk(v.x / n, v.y / n, v.z / n);
    return true;
}

SQ_HD void set_result(ivx_sdf_query_result* r, uint32_t status, uint32_t steps, uint32_t exit, float x, float y, float z, float w) {
    r->status = status, r->steps = steps, r->exit = exit, r->reserved = 0u;
    const bool ok = status == IVX_SQ_OK;
    r->v[0] = ok ? x : 0.0f, r->v[1] = ok ? y : 0.0f, r->v[2] = ok ? z : 0.0f, r->v[3] = ok ? w : 0.0f;
}

// compute_translation_to_closest_point_on_surface (meta.rs:2411-2479)
SQ_HD void closest(const Sampler& s, const ivx_similarity& surface, const ivx_sdf_query_instance& in, uint32_t max_iterations, float max_distance,
                   ivx_sdf_query_result* out) {
    const V3 center_parent = sim_point(in.subject_to_parent, mk(0.0f, 0.0f, 0.0f));
    const V3 start = sim_inv_point(surface, center_parent);
    V3 pos = start;
    uint32_t it = 0u;
    while (it < max_iterations) {
        float d;
        V3 g;
        s.gradient(pos, &d, &g);
        const float gn2 = dot(g, g);
        if (fabsf(gn2) <= SQ_EPS) {  // abs_diff_eq!(gn2, 0.0, epsilon = 1e-8)
            set_result(out, IVX_SQ_ZERO_GRADIENT, it, 0u, 0, 0, 0, 0);
            return;
        }
        pos = pos + g * (-d / gn2);  // (the step is applied before the test)
        if (fabsf(d) <= max_distance) break;
        ++it;
    }
    const V3 t = sim_vector(surface, pos - start);
    set_result(out, IVX_SQ_OK, it, IVX_SQ_EXIT_CONVERGED, t.x, t.y, t.z, 0.0f);
}

// compute_smallest_signed_distance_on_sphere (meta.rs:2705-2726)
SQ_HD bool smallest_on_sphere(const Sampler& s, float radius, V3 pos, float* out) {
    V3 closest_point = pos;
    if (!(fabsf(radius) <= FLT_EPSILON)) {  // abs_diff_ne!(radius, 0.0)
        float d;
        V3 g, dir;
        s.gradient(pos, &d, &g);
        if (!unit_if_above(g, &dir)) return false;
        closest_point = pos - dir * radius;
    }
    *out = s.value(closest_point);
    return true;
}

// AxisAlignedBox::find_ray_intersection (axis_aligned_box.rs:420-455)
SQ_HD bool ray_box(const float domain[6], V3 o, V3 d, float* t_start, float* t_end) {
    float t_min = 0.0f, t_max = INFINITY;
    const float ov[3] = {o.x, o.y, o.z}, dv[3] = {d.x, d.y, d.z};
    for (int dim = 0; dim < 3; ++dim) {
        if (dv[dim] != 0.0f) {
            const float recip = 1.0f / dv[dim];
            const float t1 = (domain[dim] - ov[dim]) * recip, t2 = (domain[3 + dim] - ov[dim]) * recip;
            const float t_entry = t1 < t2 ? t1 : t2, t_exit = t1 < t2 ? t2 : t1;
            t_min = rmax(t_min, t_entry);
            t_max = rmin(t_max, t_exit);
            if (t_max < t_min) return false;
        } else if (ov[dim] < domain[dim] || ov[dim] > domain[3 + dim]) {
            return false;
        }
    }
    if (!(t_max >= 0.0f)) return false;
    *t_start = rmax(t_min, 0.0f), *t_end = t_max;
    return true;
}

// compute_spherecast_translation_to_surface and ..._same_space (meta.rs:2534-2703)
SQ_HD void spherecast(const Sampler& s, const float domain[6], const ivx_similarity& surface, const ivx_sdf_query_instance& in, V3 direction, uint32_t max_steps,
                      float tolerance, float safety_factor, ivx_sdf_query_result* out) {
    const V3 center_parent = sim_point(in.subject_to_parent, ld3(in.sphere_center));
    const float radius_parent = in.subject_to_parent.scaling * in.sphere_radius;
    const V3 dir_parent = sim_vector(in.subject_to_parent, direction);
    const V3 origin = sim_inv_point(surface, center_parent);
    const float radius = (1.0f / surface.scaling) * radius_parent;
    V3 dir;
    if (!unit_if_above(sim_inv_vector(surface, dir_parent), &dir)) {
        set_result(out, IVX_SQ_DEGENERATE_DIRECTION, 0u, 0u, 0, 0, 0, 0);
        return;
    }
    float t0, t1;
    if (!ray_box(domain, origin, dir, &t0, &t1)) {
        set_result(out, IVX_SQ_RAY_MISSES_DOMAIN, 0u, 0u, 0, 0, 0, 0);
        return;
    }
    const float start = t0 - radius, max_along = t1;
    float along = start;
    V3 pos = origin + dir * along;
    float ssd;
    if (!smallest_on_sphere(s, radius, pos, &ssd)) {
        set_result(out, IVX_SQ_NO_GRADIENT_DIRECTION, 0u, 0u, 0, 0, 0, 0);
        return;
    }
    if (ssd < 0.0f) {
        set_result(out, IVX_SQ_PENETRATING, 0u, 0u, 0, 0, 0, 0);
        return;
    }
    float sd = fabsf(ssd);
    uint32_t steps = 0u, exit = IVX_SQ_EXIT_CONVERGED;
    bool crossed = false;
    while (sd > tolerance) {
        ++steps;
        if (steps >= max_steps) {
            if (crossed) {
                exit = IVX_SQ_EXIT_CROSSED;
                break;
            }
            set_result(out, IVX_SQ_MAX_STEPS, steps, 0u, 0, 0, 0, 0);
            return;
        }
        along = along + ssd * safety_factor;
        if (!crossed && sign_bit(ssd)) crossed = true;  // is_sign_negative: -0.0 counts
        if (along > max_along || along < start) {
            set_result(out, IVX_SQ_LEFT_INTERVAL, steps, 0u, 0, 0, 0, 0);
            return;
        }
        pos = origin + dir * along;
        if (!smallest_on_sphere(s, radius, pos, &ssd)) {
            set_result(out, IVX_SQ_NO_GRADIENT_DIRECTION, steps, 0u, 0, 0, 0, 0);
            return;
        }
        sd = fabsf(ssd);
    }
    const V3 t = sim_vector(surface, pos - origin);
    set_result(out, IVX_SQ_OK, steps, exit, t.x, t.y, t.z, 0.0f);
}

// glam Vec3::any_orthonormal_vector (the second vector of Pixar's orthonormal basis)
SQ_HD V3 any_orthonormal(V3 v) {
    const float sign = copysignf(1.0f, v.z);
    const float a = -1.0f / (sign + v.z);
    const float b = (v.x * v.y) * a;
    return mk(b, sign + (v.y * v.y) * a, -v.y);
}
// glam Quat::from_rotation_arc: the cross product and 1 + dot, normalised; the identity and the half turn near dot = +-1
SQ_HD void rotation_arc(V3 from, V3 to, float q[4]) {
    const float one_minus_eps = 1.0f - 2.0f * FLT_EPSILON;
    const float d = dot(from, to);
    if (d > one_minus_eps) {
        q[0] = 0.0f, q[1] = 0.0f, q[2] = 0.0f, q[3] = 1.0f;
    } else if (d < -one_minus_eps) {  // from_axis_angle(any_orthonormal_vector, PI): sin(PI / 2) = 1, cos(PI / 2) as f32 = -4.371139e-8
        const V3 a = any_orthonormal(from);
        q[0] = a.x * 1.0f, q[1] = a.y * 1.0f, q[2] = a.z * 1.0f, q[3] = -4.371139e-8f;
    } else {
        const V3 c = cross(from, to);
        const float w = 1.0f + d;
        const float l = sqrtf(((c.x * c.x + c.y * c.y) + c.z * c.z) + w * w);
        q[0] = c.x / l, q[1] = c.y / l, q[2] = c.z / l, q[3] = w / l;
    }
}

// compute_rotation_to_gradient (meta.rs:2481-2532)
SQ_HD void rotation(const Sampler& s, const ivx_similarity& surface, const ivx_sdf_query_instance& in, ivx_sdf_query_result* out) {
    const V3 center_parent = sim_point(in.subject_to_parent, mk(0.0f, 0.0f, 0.0f));
    const V3 p = sim_inv_point(surface, center_parent);
    float d;
    V3 g;
    s.gradient(p, &d, &g);
    const V3 y_parent = sim_vector(in.subject_to_parent, mk(0.0f, 1.0f, 0.0f));
    const V3 g_parent = sim_vector(surface, g);
    V3 y, gd;
    if (!unit_if_above(y_parent, &y)) {
        set_result(out, IVX_SQ_DEGENERATE_Y_AXIS, 0u, 0u, 0, 0, 0, 0);
        return;
    }
    if (!unit_if_above(g_parent, &gd)) {
        set_result(out, IVX_SQ_NO_GRADIENT_DIRECTION, 0u, 0u, 0, 0, 0, 0);
        return;
    }
    float q[4];
    rotation_arc(y, gd, q);
    set_result(out, IVX_SQ_OK, 0u, IVX_SQ_EXIT_CONVERGED, q[0], q[1], q[2], q[3]);
}

}  // namespace ivx_sq
