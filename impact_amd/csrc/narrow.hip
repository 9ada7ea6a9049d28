// Primitive collidables: the world-space forms of a world's sphere, plane and capsule collidables under their bodies, and the narrow phase over the
// pairs the bounding-volume pass found.
//
// Reference: impact_physics/src/collision.rs:175-261, 317-373 (synchronize_collidables_with_rigid_bodies, the two collision passes),
//   collision/collidable/basic.rs:57-151 (dispatch and CollidableOrder), sphere.rs:105-157, capsule.rs:142-303, plane.rs,
//   impact_geometry/src/line.rs:26-145 (closest points of two segments), plane.rs:197-203, capsule.rs:119-137, impact_physics/src/material.rs:43-51.
//   include/impact_voxel_hip.h states the operation order of every form; the host exports and the kernels run the functions below.
//
// SYNC — k_cw_sync, one lane per collidable: cw_transform under the body's position and orientation as the world's resident arrays hold them,
//   the world-space record, its box and its kind straight into the context's bounding-volume set buffer (bvol.hip runs k_bv_world<false> and
//   k_bv_total behind it): no host copy, no wait.
// TEST — k_cw_test, one lane per pair of the resident pair buffer (lexicographic in (a, b)): cw_contact's verdict, two ballots per wave: the mask
//   of the pairs that yield a contact and the mask of the pairs with a voxel-object member.
// SCAN — k_cw_scan, one workgroup: exclusive prefix of the masks' popcounts, SCAN_ROUND waves a round with a carry; the two totals.
// EMIT — k_cw_emit, the same lanes: a lane whose bit is set computes its contact again and writes it at its wave's offset plus the number of set
//   bits below its own — pair order, no atomic. The deferred pairs likewise.
// ROWS — k_cw_rows (ivx_cw_collide_frame only), one lane per deferred pair, right behind k_cw_emit: the dispatch of the pair (cw_rows.hpp) over the
//   world-space records, the poses of the voxel members' bodies in the world's resident arrays and the attached offsets; row i of the deferred list.
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <vector>

#include "bvol_internal.hpp"
#include "cw_rows.hpp"
#include "device_common.hpp"
#include "physics_internal.hpp"
#include "vec3.hpp"

namespace {

constexpr uint32_t GROUP = 256;       // pairs per workgroup of k_cw_test / k_cw_emit
constexpr uint32_t SCAN_ROUND = 256;  // waves per round of k_cw_scan (its workgroup): 16 384 pairs

#define CW_HD __host__ __device__ __forceinline__

// ---- shared host / device arithmetic (f32, fixed operation order; the file is compiled without contraction) ---------------------------------
using namespace ivx_vec;  // V3, the operators, dot, cross, qrot, min_rs, max_rs, splitmix
CW_HD V3 ld(const float* p) { return ld3(p); }
CW_HD void st(float* p, V3 v) { st3(p, v); }
CW_HD bool sign_bit(float v) {
#ifdef __HIP_DEVICE_COMPILE__
    return (__float_as_uint(v) >> 31) != 0u;
#else
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u >> 31) != 0u;
#endif
}
CW_HD float max0(float x) { return x > 0.0f ? x : 0.0f; }                             // f32::max(0.0, x)
CW_HD float clamp01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }      // f32::clamp(0.0, 1.0)
constexpr float EPS = 1e-8f;
constexpr float CW_BOX_PAD = 1.9073486328125e-6f;  // 2^-19
CW_HD float max_abs(float u, float v) { return fabsf(v) > fabsf(u) ? fabsf(v) : fabsf(u); }

// Collidable::from_descriptor under the body's isometry, and the world box
CW_HD void cw_transform(const ivx_collidable& local, const float p[3], const float q[4], ivx_collidable* world, ivx_aabb* box) {
    ivx_collidable w = local;
    ivx_aabb b;
    const V3 t = ld(p);
    switch (local.shape) {
        case IVX_CW_SPHERE: {
            const V3 c = qrot(q, ld(local.a)) + t;
            st(w.a, c);
            st(b.lower, mk(c.x - local.s, c.y - local.s, c.z - local.s));
            st(b.upper, mk(c.x + local.s, c.y + local.s, c.z + local.s));
            break;
        }
        case IVX_CW_CAPSULE: {
            const V3 a = qrot(q, ld(local.a)) + t, v = qrot(q, ld(local.b));
            st(w.a, a);
            st(w.b, v);
            const V3 e = a + v;
            const float r = local.s;
            st(b.lower, mk(min_rs(a.x - r, e.x - r), min_rs(a.y - r, e.y - r), min_rs(a.z - r, e.z - r)));
            st(b.upper, mk(max_rs(a.x + r, e.x + r), max_rs(a.y + r, e.y + r), max_rs(a.z + r, e.z + r)));
            break;
        }
        case IVX_CW_PLANE: {
            const V3 n = ld(local.a);
            const V3 tn = qrot(q, n);
            const V3 tp = qrot(q, n * local.s) + t;
            st(w.a, tn);
            w.s = dot(tn, tp);
            for (int k = 0; k < 3; ++k) b.lower[k] = -FLT_MAX, b.upper[k] = FLT_MAX;
            break;
        }
        default: {  // IVX_CW_VOXEL_OBJECT
            ivx_aabb m;
            ivx_similarity s;
            for (int k = 0; k < 3; ++k) m.lower[k] = local.a[k], m.upper[k] = local.b[k], s.translation[k] = p[k];
            for (int k = 0; k < 4; ++k) s.rotation[k] = q[k];
            s.scaling = 1.0f;
            ivx_bv_world_aabb_of(m, s, &b);
            // outward by more than the float32 derivation can have lost (header): the box must HOLD the object the generators see
            const float reach = (max_abs(local.a[0], local.b[0]) + max_abs(local.a[1], local.b[1])) + max_abs(local.a[2], local.b[2]);
            for (int k = 0; k < 3; ++k) {
                const float pad = (reach + fabsf(p[k])) * CW_BOX_PAD;
                b.lower[k] = b.lower[k] - pad, b.upper[k] = b.upper[k] + pad;
            }
            for (int k = 0; k < 3; ++k) w.a[k] = b.lower[k], w.b[k] = b.upper[k];
            break;
        }
    }
    *world = w;
    if (box) *box = b;
}

struct Geom {
    V3 pos, nrm;
    float depth;
};

// glam any_orthogonal_vector + normalized_from_if_above(EPSILON), fallback unit_z
CW_HD V3 ortho(V3 v) {
    const V3 o = __builtin_fabsf(v.x) > __builtin_fabsf(v.y) ? mk(-v.z, 0.0f, v.x) : mk(0.0f, v.z, -v.y);
    const float o2 = dot(o, o);
    if (o2 > EPS * EPS) {
        const float l = sqrtf(o2);
        return mk(o.x / l, o.y / l, o.z / l);
    }
    return mk(0.0f, 0.0f, 1.0f);
}

// determine_sphere_sphere_contact_geometry (sphere.rs:105-136)
CW_HD bool sphere_sphere(V3 c1, float r1, V3 c2, float r2, Geom* g) {
    const V3 d = c1 - c2;
    const float d2 = dot(d, d), m = r1 + r2;
    if (d2 > m * m) return false;
    const float dist = sqrtf(d2);
    g->nrm = dist > EPS ? d * (1.0f / dist) : mk(0.0f, 0.0f, 1.0f);
    g->pos = c2 + g->nrm * r2;
    g->depth = max0(m - dist);
    return true;
}
// determine_sphere_plane_contact_geometry (sphere.rs:138-157)
CW_HD bool sphere_plane(V3 c, float r, V3 n, float k, Geom* g) {
    const float sd = dot(n, c) - k;
    const float depth = r - sd;
    if (depth < 0.0f) return false;
    g->pos = c - n * sd;
    g->nrm = n;
    g->depth = depth;
    return true;
}
// determine_capsule_sphere_contact_geometry (capsule.rs:212-270)
CW_HD bool capsule_sphere(V3 a, V3 v, float rc, V3 c, float r, Geom* g) {
    const float l2 = dot(v, v);
    float t = 0.0f;
    if (!(l2 <= EPS)) t = clamp01(dot(v, c - a) / l2);
    const V3 d = c - (a + v * t);
    const float d2 = dot(d, d), m = r + rc;
    if (d2 > m * m) return false;
    const float dist = sqrtf(d2);
    V3 cn;
    if (dist > EPS) {
        cn = d * (1.0f / dist);
        g->depth = max0(m - dist);
    } else {  // the sphere's centre lies on the segment
        cn = ortho(v);
        g->depth = max0(m);
    }
    g->nrm = mk(-cn.x, -cn.y, -cn.z);
    g->pos = c + g->nrm * r;
    return true;
}
// parameters_of_closest_points_on_line_segments (line.rs:75-145)
CW_HD void closest_parameters(V3 a1, V3 v1, V3 a2, V3 v2, float* s_out, float* t_out) {
    const float l1 = dot(v1, v1), l2 = dot(v2, v2);
    float s = 0.0f, t = 0.0f;
    if (!(l1 <= EPS && l2 <= EPS)) {
        const V3 r = a1 - a2;
        const float f = dot(v2, r);
        if (l1 <= EPS) {
            t = clamp01(f / l2);
        } else {
            const float c = dot(v1, r);
            if (l2 <= EPS) {
                s = clamp01(c / (-l1));
            } else {
                const float g = dot(v1, v2);
                const float den = l1 * l2 - g * g;
                s = den != 0.0f ? clamp01((g * f - c * l2) / den) : 0.0f;
                t = (g * s + f) / l2;
                if (sign_bit(t)) {
                    t = 0.0f;
                    s = clamp01(c / (-l1));
                } else if (t > 1.0f) {
                    t = 1.0f;
                    s = clamp01((g - c) / l1);
                }
            }
        }
    }
    *s_out = s, *t_out = t;
}
// determine_capsule_capsule_contact_geometry (capsule.rs:142-210)
CW_HD bool capsule_capsule(V3 a1, V3 v1, float r1, V3 a2, V3 v2, float r2, Geom* g) {
    float s, t;
    closest_parameters(a1, v1, a2, v2, &s, &t);
    const V3 p1 = a1 + v1 * s, p2 = a2 + v2 * t;
    const V3 d = p1 - p2;
    const float d2 = dot(d, d), m = r1 + r2;
    if (d2 > m * m) return false;
    const float dist = sqrtf(d2);
    if (dist > EPS) {
        g->nrm = d * (1.0f / dist);
        g->depth = max0(m - dist);
    } else {  // the segments intersect: any normal to B's segment, and how far A has to move against it to clear B
        g->nrm = ortho(v2);
        const float w = dot(v1, g->nrm);
        const float shift = !sign_bit(w) ? (1.0f - s) * w : (-s) * w;
        g->depth = max0(m + shift);
    }
    g->pos = p2 + g->nrm * r2;
    return true;
}
// determine_capsule_plane_contact_geometry (capsule.rs:272-303)
CW_HD bool capsule_plane(V3 a, V3 v, float r, V3 n, float k, Geom* g) {
    const V3 e = a + v;
    const float d0 = dot(n, a) - k, d1 = dot(n, e) - k;
    const bool first = d0 <= d1;
    const V3 p = first ? a : e;
    const float low = first ? d0 : d1;
    const float depth = r - low;
    if (depth < 0.0f) return false;
    g->pos = p - n * low;
    g->nrm = n;
    g->depth = depth;
    return true;
}

// generate_contact_manifold (basic.rs:57-151) for world-space A, B -> 0 none, 1 `out` filled, 2 deferred (a voxel-object member)
CW_HD int cw_contact(const ivx_collidable& A, const ivx_collidable& B, ivx_contact* out) {
    if (A.shape == IVX_CW_VOXEL_OBJECT || B.shape == IVX_CW_VOXEL_OBJECT) return 2;
    const bool swapped = (A.shape == IVX_CW_SPHERE && B.shape == IVX_CW_CAPSULE) || (A.shape == IVX_CW_PLANE && B.shape != IVX_CW_PLANE);
    const ivx_collidable& F = swapped ? B : A;
    const ivx_collidable& S = swapped ? A : B;
    Geom g;
    bool hit;
    if (F.shape == IVX_CW_CAPSULE) {
        if (S.shape == IVX_CW_CAPSULE) hit = capsule_capsule(ld(F.a), ld(F.b), F.s, ld(S.a), ld(S.b), S.s, &g);
        else if (S.shape == IVX_CW_SPHERE) hit = capsule_sphere(ld(F.a), ld(F.b), F.s, ld(S.a), S.s, &g);
        else hit = capsule_plane(ld(F.a), ld(F.b), F.s, ld(S.a), S.s, &g);
    } else if (F.shape == IVX_CW_SPHERE) {
        if (S.shape == IVX_CW_SPHERE) hit = sphere_sphere(ld(F.a), F.s, ld(S.a), S.s, &g);
        else hit = sphere_plane(ld(F.a), F.s, ld(S.a), S.s, &g);
    } else {
        hit = false;  // plane against plane
    }
    if (!hit) return 0;
    ivx_contact c;
    c.id = splitmix(F.id ^ splitmix(S.id));
    c.body_a = F.body, c.body_b = S.body;
    st(c.position, g.pos);
    st(c.normal, g.nrm);
    c.depth = g.depth;
    c.restitution = max_rs(F.response[0], S.response[0]);
    c.static_friction = sqrtf(F.response[1] * S.response[1]);
    c.dynamic_friction = sqrtf(F.response[2] * S.response[2]);
    c.flags = IVX_CONTACT_MANIFOLD_START, c.reserved = 0u;
    *out = c;
    return 1;
}

// ---- device side -------------------------------------------------------------------------------------------------------------------------
// `slots` = ceil(n / 64) x 64: the kinds behind n are written as zero (the pair walk reads whole blocks)
__global__ __launch_bounds__(256) void k_cw_sync(const ivx_collidable* __restrict__ local, uint32_t n, uint32_t slots, const ivx_rigid_body* __restrict__ dyn,
                                                 const ivx_kinematic_body* __restrict__ kin, ivx_collidable* __restrict__ world, ivx_aabb* __restrict__ boxes,
                                                 uint32_t* __restrict__ kinds) {
    const uint32_t o = blockIdx.x * 256u + threadIdx.x;
    if (o >= slots) return;
    uint32_t kind = 0u;
    if (o < n) {
        const ivx_collidable l = local[o];
        float p[3], q[4];
        const uint32_t body = l.body & ~IVX_KINEMATIC_BODY;
        if (l.body & IVX_KINEMATIC_BODY) {
            for (int k = 0; k < 3; ++k) p[k] = kin[body].position[k];
            for (int k = 0; k < 4; ++k) q[k] = kin[body].orientation[k];
        } else {
            for (int k = 0; k < 3; ++k) p[k] = dyn[body].position[k];
            for (int k = 0; k < 4; ++k) q[k] = dyn[body].orientation[k];
        }
        ivx_collidable w;
        ivx_aabb b;
        cw_transform(l, p, q, &w, &b);
        world[o] = w;
        boxes[o] = b;
        kind = l.kind;
    }
    kinds[o] = kind;
}

__global__ __launch_bounds__(GROUP) void k_cw_test(const uint2* __restrict__ pairs, uint32_t n_pairs, const ivx_collidable* __restrict__ colls,
                                                   unsigned long long* __restrict__ mask_hit, unsigned long long* __restrict__ mask_def) {
    const uint32_t p = blockIdx.x * GROUP + threadIdx.x, lane = threadIdx.x & 63u, wave = p >> 6;
    if (wave * 64u >= n_pairs) return;  // (whole waves)
    int verdict = 0;
    if (p < n_pairs) {
        const uint2 pr = pairs[p];
        ivx_contact c;
        verdict = cw_contact(colls[pr.x], colls[pr.y], &c);
    }
    const unsigned long long mh = __ballot(verdict == 1), md = __ballot(verdict == 2);
    if (lane == 0u) mask_hit[wave] = mh, mask_def[wave] = md;
}

// exclusive prefixes of the masks' popcounts; totals[0] contacts, totals[1] deferred pairs (the pair count is below 2^31)
__global__ __launch_bounds__(SCAN_ROUND) void k_cw_scan(const unsigned long long* __restrict__ mask_hit, const unsigned long long* __restrict__ mask_def, uint32_t n_waves,
                                                        uint32_t* __restrict__ off_hit, uint32_t* __restrict__ off_def, uint32_t* __restrict__ totals) {
    __shared__ uint32_t wave_totals[2][SCAN_ROUND / 64u];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    uint32_t carry_h = 0u, carry_d = 0u;
    for (uint32_t r0 = 0; r0 < n_waves; r0 += SCAN_ROUND) {
        const uint32_t w = r0 + t;
        const uint32_t ch = w < n_waves ? (uint32_t)__popcll(mask_hit[w]) : 0u, cd = w < n_waves ? (uint32_t)__popcll(mask_def[w]) : 0u;
        const uint32_t ih = ivx_wave_incl_scan(ch), id = ivx_wave_incl_scan(cd);
        if (lane == 63u) wave_totals[0][wv] = ih, wave_totals[1][wv] = id;
        __syncthreads();
        uint32_t before_h = 0u, before_d = 0u, round_h = 0u, round_d = 0u;
        for (uint32_t k = 0; k < SCAN_ROUND / 64u; ++k) {
            const uint32_t th = wave_totals[0][k], td = wave_totals[1][k];
            before_h += k < wv ? th : 0u, before_d += k < wv ? td : 0u;
            round_h += th, round_d += td;
        }
        if (w < n_waves) off_hit[w] = carry_h + before_h + (ih - ch), off_def[w] = carry_d + before_d + (id - cd);
        carry_h += round_h, carry_d += round_d;
        __syncthreads();
    }
    if (t == 0u) totals[0] = carry_h, totals[1] = carry_d;
}

__global__ __launch_bounds__(GROUP) void k_cw_emit(const uint2* __restrict__ pairs, uint32_t n_pairs, const ivx_collidable* __restrict__ colls,
                                                   const unsigned long long* __restrict__ mask_hit, const unsigned long long* __restrict__ mask_def,
                                                   const uint32_t* __restrict__ off_hit, const uint32_t* __restrict__ off_def, ivx_contact* __restrict__ contacts,
                                                   uint2* __restrict__ deferred) {
    const uint32_t p = blockIdx.x * GROUP + threadIdx.x, lane = threadIdx.x & 63u, wave = p >> 6;
    if (p >= n_pairs) return;
    const unsigned long long mh = mask_hit[wave], md = mask_def[wave], below = (1ull << lane) - 1ull;
    if (!(((mh | md) >> lane) & 1ull)) return;
    const uint2 pr = pairs[p];
    if ((mh >> lane) & 1ull) {  // (the verdict k_cw_test reached from the same bytes)
        ivx_contact c;
        (void)cw_contact(colls[pr.x], colls[pr.y], &c);
        contacts[off_hit[wave] + (uint32_t)__popcll(mh & below)] = c;
    } else {
        deferred[off_def[wave] + (uint32_t)__popcll(md & below)] = pr;
    }
}

// what ivx_cw_set_voxel_objects attached to a collidable, as the device holds it (indexed by collidable; all zero: nothing attached)
struct CwVoxel {
    float origin_offset[3], center_of_mass[3];
    uint32_t attached, reserved;
};
static_assert(sizeof(CwVoxel) == 32 && sizeof(ivx_cw_row) == 160 && sizeof(ivx_cw_voxel_object) == 32, "collision frame record layouts");
static_assert(offsetof(ivx_rigid_body, orientation) == offsetof(ivx_rigid_body, position) + 12 &&
                  offsetof(ivx_kinematic_body, orientation) == offsetof(ivx_kinematic_body, position) + 12,
              "a body's pose is position[3] then orientation[4]");

// a lane per deferred pair; `totals[1]` is the deferred count k_cw_scan left (max_rows: what the row buffer holds, never below it)
__global__ __launch_bounds__(GROUP) void k_cw_rows(const uint2* __restrict__ deferred, const uint32_t* __restrict__ totals, uint32_t max_rows,
                                                   const ivx_collidable* __restrict__ colls, const ivx_rigid_body* __restrict__ dyn,
                                                   const ivx_kinematic_body* __restrict__ kin, const CwVoxel* __restrict__ vox, ivx_cw_row* __restrict__ rows) {
    const uint32_t i = blockIdx.x * GROUP + threadIdx.x;
    const uint32_t n = totals[1] < max_rows ? totals[1] : max_rows;
    if (i >= n) return;
    const uint2 pr = deferred[i];
    auto member = [&](uint32_t index) {
        ivx_cw_rows::Member m;
        m.c = colls + index, m.index = index;
        m.pose = nullptr, m.origin_offset = nullptr, m.center_of_mass = nullptr;
        if (m.c->shape == IVX_CW_VOXEL_OBJECT) {
            const uint32_t ref = m.c->body, body = ref & ~IVX_KINEMATIC_BODY;
            m.pose = (ref & IVX_KINEMATIC_BODY) ? kin[body].position : dyn[body].position;
            m.origin_offset = vox[index].origin_offset, m.center_of_mass = vox[index].center_of_mass;
        }
        return m;
    };
    ivx_cw_rows::voxel_row(member(pr.x), member(pr.y), rows + i);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
// world-owned state: device buffers that only grow, a pinned block the results of a call come back through (device_common.hpp)
struct CwState {
    ivx_buf local, world, scratch, contacts, deferred;
    ivx_staging staging;  // (the synchronous path: the call waits for the stream before it reads the block)
    bool has_collidables = false, synchronized = false;
    uint32_t n = 0;
    uint32_t need_dyn = 0, need_kin = 0;  // body counts the collidables' indices were checked against need at least
    uint64_t set_serial = 0;              // the context's bounding-volume set the last synchronize installed
    size_t n_contacts = 0, n_deferred = 0;
    uint32_t broad_phase = IVX_CW_BROAD_FLAT;  // where ivx_cw_collide takes its pairs from (ivx_cw_set_broad_phase)
    // the collision frame (ivx_cw_collide_frame): the shapes of the set and what is attached to its voxel collidables, on the host and (CwVoxel per
    // collidable) on the device; the rows of the last call; the pinned blocks its rows (when they outgrew the guess) and its merged list come through
    std::vector<uint8_t> shapes;
    std::vector<ivx_cw_voxel_object> objects;
    uint32_t n_voxel = 0;
    ivx_buf voxel_dev, rows;
    ivx_staging staging_rows, staging_out;
    size_t n_rows = 0, last_deferred = 0;
};

int state_of(ivx_world* w, CwState** out) { return ivx_state_for(&w->cw_state, "collidables", out); }

int synchronized_state(ivx_world* w, const char* who, CwState** out) {
    IVX_REQUIRE(w, IVX_ERR_INVALID, "%s: null world", who);
    CwState* st = static_cast<CwState*>(w->cw_state);
    IVX_REQUIRE(st && st->has_collidables, IVX_ERR_STATE, "%s: the world holds no collidables (call ivx_cw_set_collidables first)", who);
    IVX_REQUIRE(st->synchronized, IVX_ERR_STATE, "%s: the collidables have not been synchronized with the bodies (call ivx_cw_synchronize first)", who);
    *out = st;
    return IVX_OK;
}

}  // namespace

void ivx_cw_release(ivx_world* w) {
    CwState* s = w ? ivx_state_take<CwState>(&w->cw_state) : nullptr;
    if (!s) return;
    for (ivx_buf* b : {&s->local, &s->world, &s->scratch, &s->contacts, &s->deferred, &s->voxel_dev, &s->rows}) ivx_buf_free(b);
    for (ivx_staging* g : {&s->staging, &s->staging_rows, &s->staging_out}) ivx_staging_release(g);
    delete s;
}

namespace {

// What ivx_cw_collide and ivx_cw_collide_frame share: the pair pass (first wait), k_cw_test | k_cw_scan | k_cw_emit over the resident pairs, for the
// frame k_cw_rows behind them, and the second wait, which brings the two counts and as much of the lists as was asked for (what lies behind the
// counts is dropped by the caller).
struct CollidePass {
    CwState* st = nullptr;
    uint32_t totals[2] = {0u, 0u};  // contacts, deferred pairs
    const char* contacts = nullptr;  // in the world's pinned block: copy_contacts records, copy_deferred pairs
    const char* deferred = nullptr;
    const ivx_cw_row* rows = nullptr;  // (frame) totals[1] of them
};
int collide_pass(ivx_world* w, const char* who, uint32_t mode, size_t contacts_cap, size_t deferred_cap, bool frame, CollidePass* out) {
    CwState* st;
    if (int rc = synchronized_state(w, who, &st)) return rc;
    out->st = st;
    ivx_ctx* c = w->ctx;
    IVX_REQUIRE(ivx_bvol_set_serial(c) == st->set_serial, IVX_ERR_STATE,
                "%s: the context's set of bounding volumes has been replaced since ivx_cw_synchronize (synchronize again)", who);
    ivx_many_other_context other_(c);
    st->n_contacts = 0, st->n_deferred = 0, st->n_rows = 0;
    size_t n_pairs = 0;
    if (st->broad_phase == IVX_CW_BROAD_HIERARCHY) {
        if (int rc = ivx_bvh_build_enqueue(c, who)) return rc;  // (nothing waits)
        if (int rc = ivx_bvh_pairs_enqueue(c, who, mode, false, 0, &n_pairs)) return rc;
    } else if (int rc = ivx_bvol_pairs_enqueue(c, who, mode, false, 0, &n_pairs)) {  // (either way the call's first wait: the grand total)
        return rc;
    }
    if (n_pairs == 0) return IVX_OK;
    const uint32_t np = (uint32_t)n_pairs, n_waves = (np + 63u) / 64u;
    ivx_layout l;
    const size_t o_mh = l.take((size_t)n_waves * 8), o_md = l.take((size_t)n_waves * 8), o_oh = l.take((size_t)n_waves * 4), o_od = l.take((size_t)n_waves * 4), o_tot = l.take(8);
    if (int rc = ivx_buf_grow(c, &st->scratch, l.bytes, 1u << 16)) return rc;
    if (int rc = ivx_buf_grow(c, &st->contacts, n_pairs * sizeof(ivx_contact), 1u << 16)) return rc;  // (at most one contact per pair)
    if (int rc = ivx_buf_grow(c, &st->deferred, n_pairs * 8, 1u << 16)) return rc;
    // the frame's rows: a deferred pair has a voxel member, so there are no more than (voxel collidables) x (n - 1) of them. The host needs ALL rows;
    // how many come with the counts is a guess from the last call (twice its deferred pairs, at least 256): a list that outgrew it is fetched below
    size_t max_rows = 0, copy_rows = 0;
    if (frame && st->n_voxel) {
        max_rows = std::min<size_t>(n_pairs, (size_t)st->n_voxel * (st->n - 1u));
        copy_rows = std::min<size_t>(max_rows, std::max<size_t>(256, 2 * st->last_deferred));
        if (int rc = ivx_buf_grow(c, &st->rows, max_rows * sizeof(ivx_cw_row), 1u << 16)) return rc;
    }
    const size_t copy_contacts = contacts_cap < n_pairs ? contacts_cap : n_pairs, copy_deferred = deferred_cap < n_pairs ? deferred_cap : n_pairs;
    ivx_layout h;
    const size_t h_tot = h.take(8), h_contacts = h.take(copy_contacts * sizeof(ivx_contact)), h_deferred = h.take(copy_deferred * 8),
                 h_rows = h.take(copy_rows * sizeof(ivx_cw_row));
    if (int rc = ivx_staging_for(&st->staging, h.bytes)) return rc;
    char* s = static_cast<char*>(st->scratch.p);
    unsigned long long* d_mh = reinterpret_cast<unsigned long long*>(s + o_mh);
    unsigned long long* d_md = reinterpret_cast<unsigned long long*>(s + o_md);
    uint32_t* d_oh = reinterpret_cast<uint32_t*>(s + o_oh);
    uint32_t* d_od = reinterpret_cast<uint32_t*>(s + o_od);
    uint32_t* d_tot = reinterpret_cast<uint32_t*>(s + o_tot);
    const uint2* d_pairs = static_cast<const uint2*>(ivx_bv_device_ptr(c, IVX_BV_PTR_PAIRS));
    const ivx_collidable* d_colls = static_cast<const ivx_collidable*>(st->world.p);
    IVX_REQUIRE(d_pairs && d_colls, IVX_ERR_STATE, "%s: no resident pair buffer", who);
    const dim3 grid((np + GROUP - 1u) / GROUP);
    IVX_KLAUNCH(k_cw_test, grid, dim3(GROUP), 0, c->stream, d_pairs, np, d_colls, d_mh, d_md);
    IVX_KLAUNCH(k_cw_scan, dim3(1), dim3(SCAN_ROUND), 0, c->stream, (const unsigned long long*)d_mh, (const unsigned long long*)d_md, n_waves, d_oh, d_od, d_tot);
    IVX_KLAUNCH(k_cw_emit, grid, dim3(GROUP), 0, c->stream, d_pairs, np, d_colls, (const unsigned long long*)d_mh, (const unsigned long long*)d_md, (const uint32_t*)d_oh,
                (const uint32_t*)d_od, static_cast<ivx_contact*>(st->contacts.p), static_cast<uint2*>(st->deferred.p));
    if (max_rows)
        IVX_KLAUNCH(k_cw_rows, dim3(((uint32_t)max_rows + GROUP - 1u) / GROUP), dim3(GROUP), 0, c->stream, static_cast<const uint2*>(st->deferred.p), (const uint32_t*)d_tot,
                    (uint32_t)max_rows, d_colls, (const ivx_rigid_body*)w->dyn.p, (const ivx_kinematic_body*)w->kin.p, static_cast<const CwVoxel*>(st->voxel_dev.p),
                    static_cast<ivx_cw_row*>(st->rows.p));
    IVX_HIP_CHECK(hipGetLastError());
    // the call's second wait: the two counts, and as much of the lists as the caller's buffers could hold (what lies behind the counts is dropped)
    char* hs = static_cast<char*>(st->staging.p);
    IVX_HIP_CHECK(ivx_memcpy_async(hs + h_tot, d_tot, 8, hipMemcpyDeviceToHost, c->stream));
    if (copy_contacts) IVX_HIP_CHECK(ivx_memcpy_async(hs + h_contacts, st->contacts.p, copy_contacts * sizeof(ivx_contact), hipMemcpyDeviceToHost, c->stream));
    if (copy_deferred) IVX_HIP_CHECK(ivx_memcpy_async(hs + h_deferred, st->deferred.p, copy_deferred * 8, hipMemcpyDeviceToHost, c->stream));
    if (copy_rows) IVX_HIP_CHECK(ivx_memcpy_async(hs + h_rows, st->rows.p, copy_rows * sizeof(ivx_cw_row), hipMemcpyDeviceToHost, c->stream));
    IVX_HIP_CHECK(ivx_stream_sync(c->stream));
    memcpy(out->totals, hs + h_tot, 8);
    st->n_contacts = out->totals[0], st->n_deferred = out->totals[1];
    out->contacts = hs + h_contacts, out->deferred = hs + h_deferred;
    if (frame) {
        const size_t n_rows = out->totals[1];
        IVX_REQUIRE(n_rows <= max_rows, IVX_ERR_STATE, "%s: %zu deferred pairs for %u voxel collidables among %u", who, n_rows, st->n_voxel, st->n);
        out->rows = reinterpret_cast<const ivx_cw_row*>(hs + h_rows);
        if (n_rows > copy_rows) {  // (the list outgrew the guess: all rows, one more wait)
            if (int rc = ivx_staging_for(&st->staging_rows, n_rows * sizeof(ivx_cw_row))) return rc;
            IVX_HIP_CHECK(ivx_memcpy_async(st->staging_rows.p, st->rows.p, n_rows * sizeof(ivx_cw_row), hipMemcpyDeviceToHost, c->stream));
            IVX_HIP_CHECK(ivx_stream_sync(c->stream));
            out->rows = static_cast<const ivx_cw_row*>(st->staging_rows.p);
        }
        st->n_rows = n_rows, st->last_deferred = n_rows;
    }
    return IVX_OK;
}

}  // namespace

int ivx_cw_frame_pairs(ivx_world* w, const char* who, uint32_t mode, size_t contacts_cap, size_t deferred_cap, ivx_cw_frame_pass* out) {
    CollidePass p;
    if (int rc = collide_pass(w, who, mode, contacts_cap, deferred_cap, true, &p)) return rc;
    out->n_primitive = p.totals[0], out->n_deferred = p.totals[1];
    out->rows = p.rows, out->contacts = reinterpret_cast<const ivx_contact*>(p.contacts), out->deferred = reinterpret_cast<const uint32_t*>(p.deferred);
    out->objects = p.st->objects.data(), out->n_collidables = p.st->n;
    return IVX_OK;
}

int ivx_cw_frame_reserve(ivx_world* w, size_t n_primitive, size_t total, ivx_contact** list) {
    CwState* st = static_cast<CwState*>(w->cw_state);
    ivx_ctx* c = w->ctx;
    if (st->contacts.bytes < total * sizeof(ivx_contact)) {  // grow, keeping what k_cw_emit wrote: the copy on the stream, one wait, then the old block goes
        const size_t bytes = std::max<size_t>(total * sizeof(ivx_contact) * 3 / 2, 1u << 16);
        void* fresh = nullptr;
        IVX_HIP_CHECK(hipMalloc(&fresh, bytes));
        hipError_t e = n_primitive ? ivx_memcpy_async(fresh, st->contacts.p, n_primitive * sizeof(ivx_contact), hipMemcpyDeviceToDevice, c->stream) : hipSuccess;
        if (e == hipSuccess) e = ivx_stream_sync(c->stream);
        if (e != hipSuccess) (void)hipFree(fresh);
        IVX_HIP_CHECK(e);
        if (st->contacts.p) (void)hipFree(st->contacts.p);
        st->contacts.p = fresh, st->contacts.bytes = bytes;
    }
    *list = static_cast<ivx_contact*>(st->contacts.p);
    return IVX_OK;
}

int ivx_cw_frame_finish(ivx_world* w, size_t total, ivx_contact* out) {
    CwState* st = static_cast<CwState*>(w->cw_state);
    ivx_ctx* c = w->ctx;
    if (out && total) {
        if (int rc = ivx_staging_for(&st->staging_out, total * sizeof(ivx_contact))) return rc;
        IVX_HIP_CHECK(ivx_memcpy_async(st->staging_out.p, st->contacts.p, total * sizeof(ivx_contact), hipMemcpyDeviceToHost, c->stream));
    }
    IVX_HIP_CHECK(ivx_stream_sync(c->stream));
    if (out && total) memcpy(out, st->staging_out.p, total * sizeof(ivx_contact));
    return IVX_OK;
}

extern "C" {

int ivx_cw_transform(const ivx_collidable* local, const float position[3], const float orientation_xyzw[4], ivx_collidable* world, ivx_aabb* box) {
    IVX_REQUIRE(local && position && orientation_xyzw && world, IVX_ERR_INVALID, "ivx_cw_transform: null argument");
    IVX_REQUIRE(local->shape <= IVX_CW_VOXEL_OBJECT, IVX_ERR_INVALID, "ivx_cw_transform: shape %u (0 sphere, 1 plane, 2 capsule, 3 voxel object)", local->shape);
    ivx_collidable w;
    cw_transform(*local, position, orientation_xyzw, &w, box);
    *world = w;
    return IVX_OK;
}

int ivx_cw_contact(const ivx_collidable* a_world, const ivx_collidable* b_world, ivx_contact* out, int* hit) {
    IVX_REQUIRE(a_world && b_world && out && hit, IVX_ERR_INVALID, "ivx_cw_contact: null argument");
    *hit = 0;
    IVX_REQUIRE(a_world->shape <= IVX_CW_VOXEL_OBJECT && b_world->shape <= IVX_CW_VOXEL_OBJECT, IVX_ERR_INVALID,
                "ivx_cw_contact: shapes %u, %u (0 sphere, 1 plane, 2 capsule, 3 voxel object)", a_world->shape, b_world->shape);
    ivx_contact c;
    const int verdict = cw_contact(*a_world, *b_world, &c);
    if (verdict == 1) *out = c;
    *hit = verdict;
    return IVX_OK;
}

int ivx_cw_set_collidables(ivx_world* w, const ivx_collidable* collidables, size_t n) {
    const char* who = "ivx_cw_set_collidables";
    IVX_REQUIRE(w && (collidables || n == 0), IVX_ERR_INVALID, "%s: null argument", who);
    IVX_REQUIRE(n <= IVX_BV_MAX_OBJECTS, IVX_ERR_CAPACITY, "%s: %zu collidables exceed %u", who, n, IVX_BV_MAX_OBJECTS);
    uint32_t need_dyn = 0, need_kin = 0;
    for (size_t i = 0; i < n; ++i) {
        const ivx_collidable& c = collidables[i];
        IVX_REQUIRE(c.shape <= IVX_CW_VOXEL_OBJECT, IVX_ERR_INVALID, "%s: collidable %zu has shape %u (0 sphere, 1 plane, 2 capsule, 3 voxel object)", who, i, c.shape);
        IVX_REQUIRE(c.kind <= IVX_BV_PHANTOM, IVX_ERR_INVALID, "%s: collidable %zu has kind %u (0 dynamic, 1 static, 2 phantom)", who, i, c.kind);
        const uint32_t body = c.body & ~IVX_KINEMATIC_BODY;
        const bool kinematic = (c.body & IVX_KINEMATIC_BODY) != 0u;
        IVX_REQUIRE(body < (kinematic ? w->n_kin : w->n_dyn), IVX_ERR_INVALID, "%s: collidable %zu follows %s body %u, the world has %u", who, i,
                    kinematic ? "kinematic" : "dynamic", body, kinematic ? w->n_kin : w->n_dyn);
        uint32_t& need = kinematic ? need_kin : need_dyn;
        if (body + 1u > need) need = body + 1u;
    }
    CwState* st;
    if (int rc = state_of(w, &st)) return rc;
    ivx_many_other_context other_(w->ctx);
    st->has_collidables = false, st->synchronized = false, st->n = 0;  // (until this call's set stands)
    st->objects.clear(), st->n_voxel = 0, st->n_rows = 0, st->last_deferred = 0;  // (what was attached to the set before goes with it)
    uint32_t n_voxel = 0;
    for (size_t i = 0; i < n; ++i) n_voxel += collidables[i].shape == IVX_CW_VOXEL_OBJECT;
    if (n) {
        IVX_HIP_CHECK(ivx_stream_sync(w->ctx->stream));  // (a synchronize in flight reads the records this call replaces)
        if (int rc = ivx_buf_grow(w->ctx, &st->local, n * sizeof(ivx_collidable), 1u << 16)) return rc;
        if (int rc = ivx_buf_grow(w->ctx, &st->world, n * sizeof(ivx_collidable), 1u << 16)) return rc;
        IVX_HIP_CHECK(ivx_memcpy_sync(st->local.p, collidables, n * sizeof(ivx_collidable), hipMemcpyHostToDevice));
        if (n_voxel) {  // nothing attached yet
            if (int rc = ivx_buf_grow(w->ctx, &st->voxel_dev, n * sizeof(CwVoxel), 1u << 12)) return rc;
            IVX_HIP_CHECK(ivx_memset_async(st->voxel_dev.p, 0, n * sizeof(CwVoxel), w->ctx->stream));
        }
    }
    st->shapes.resize(n);
    for (size_t i = 0; i < n; ++i) st->shapes[i] = (uint8_t)collidables[i].shape;
    st->objects.assign(n, ivx_cw_voxel_object{});
    st->n_voxel = n_voxel;
    st->n = (uint32_t)n, st->need_dyn = need_dyn, st->need_kin = need_kin;
    st->has_collidables = true;
    return IVX_OK;
}

int ivx_cw_synchronize(ivx_world* w) {
    const char* who = "ivx_cw_synchronize";
    IVX_REQUIRE(w, IVX_ERR_INVALID, "%s: null world", who);
    CwState* st = static_cast<CwState*>(w->cw_state);
    IVX_REQUIRE(st && st->has_collidables, IVX_ERR_STATE, "%s: the world holds no collidables (call ivx_cw_set_collidables first)", who);
    IVX_REQUIRE(w->n_dyn >= st->need_dyn && w->n_kin >= st->need_kin, IVX_ERR_STATE,
                "%s: the collidables follow %u dynamic and %u kinematic bodies, the world now has %u and %u", who, st->need_dyn, st->need_kin, w->n_dyn, w->n_kin);
    ivx_ctx* c = w->ctx;
    ivx_many_other_context other_(c);
    st->synchronized = false;
    const uint32_t n = st->n;
    ivx_aabb* d_boxes;
    uint32_t* d_kinds;
    if (int rc = ivx_bvol_set_begin(c, n, &d_boxes, &d_kinds)) return rc;
    if (n) {
        const uint32_t slots = ((n + 63u) / 64u) * 64u;
        IVX_KLAUNCH(k_cw_sync, dim3((slots + 255u) / 256u), dim3(256), 0, c->stream, static_cast<const ivx_collidable*>(st->local.p), n, slots, (const ivx_rigid_body*)w->dyn.p,
                    (const ivx_kinematic_body*)w->kin.p, static_cast<ivx_collidable*>(st->world.p), d_boxes, d_kinds);
        IVX_HIP_CHECK(hipGetLastError());
    }
    if (int rc = ivx_bvol_set_finish(c, n)) return rc;
    st->set_serial = ivx_bvol_set_serial(c);
    st->synchronized = true;
    return IVX_OK;
}

int ivx_cw_download(ivx_world* w, ivx_collidable* world_space, size_t cap) {
    const char* who = "ivx_cw_download";
    CwState* st;
    if (int rc = synchronized_state(w, who, &st)) return rc;
    IVX_REQUIRE(cap >= st->n, IVX_ERR_CAPACITY, "%s: the world has %u collidables, the buffer holds %zu", who, st->n, cap);
    IVX_REQUIRE(world_space || st->n == 0, IVX_ERR_INVALID, "%s: null buffer", who);
    if (st->n == 0) return IVX_OK;
    ivx_many_other_context other_(w->ctx);
    IVX_HIP_CHECK(ivx_memcpy_async(world_space, st->world.p, (size_t)st->n * sizeof(ivx_collidable), hipMemcpyDeviceToHost, w->ctx->stream));
    IVX_HIP_CHECK(ivx_stream_sync(w->ctx->stream));
    return IVX_OK;
}

int ivx_cw_collide(ivx_world* w, uint32_t mode, ivx_contact* out, size_t cap, size_t* n_out, uint32_t* deferred_pairs, size_t deferred_cap, size_t* n_deferred) {
    const char* who = "ivx_cw_collide";
    IVX_REQUIRE(n_out && n_deferred, IVX_ERR_INVALID, "%s: null argument", who);
    *n_out = 0, *n_deferred = 0;
    IVX_REQUIRE(mode <= IVX_BV_DYNAMIC_PAIRS, IVX_ERR_INVALID, "%s: mode %u (0 = all pairs, 1 = no phantom and at least one dynamic member)", who, mode);
    IVX_REQUIRE(out || cap == 0, IVX_ERR_INVALID, "%s: null contact buffer of capacity %zu", who, cap);
    IVX_REQUIRE(deferred_pairs || deferred_cap == 0, IVX_ERR_INVALID, "%s: null deferred pair buffer of capacity %zu", who, deferred_cap);
    CollidePass p;
    if (int rc = collide_pass(w, who, mode, out ? cap : 0, deferred_pairs ? deferred_cap : 0, false, &p)) return rc;
    const uint32_t* totals = p.totals;
    *n_out = totals[0], *n_deferred = totals[1];
    IVX_REQUIRE(!out || totals[0] <= cap, IVX_ERR_CAPACITY, "%s: %u contacts, the buffer holds %zu", who, totals[0], cap);
    IVX_REQUIRE(!deferred_pairs || totals[1] <= deferred_cap, IVX_ERR_CAPACITY, "%s: %u deferred pairs, the buffer holds %zu", who, totals[1], deferred_cap);
    if (out && totals[0]) memcpy(out, p.contacts, (size_t)totals[0] * sizeof(ivx_contact));
    if (deferred_pairs && totals[1]) memcpy(deferred_pairs, p.deferred, (size_t)totals[1] * 8);
    return IVX_OK;
}

int ivx_cw_to_object_space(const float position[3], const float orientation_xyzw[4], const float origin_offset[3], float rotation_out[4], float translation_out[3]) {
    IVX_REQUIRE(position && orientation_xyzw && origin_offset && rotation_out && translation_out, IVX_ERR_INVALID, "ivx_cw_to_object_space: null argument");
    const float pose[7] = {position[0], position[1], position[2], orientation_xyzw[0], orientation_xyzw[1], orientation_xyzw[2], orientation_xyzw[3]};
    ivx_cw_rows::to_object_space(pose, origin_offset, rotation_out, translation_out);
    return IVX_OK;
}

int ivx_cw_voxel_row(const ivx_collidable* a_world, const ivx_collidable* b_world, const float pose_a[7], const float pose_b[7], const ivx_cw_voxel_object* voxel_a,
                     const ivx_cw_voxel_object* voxel_b, ivx_cw_row* out) {
    const char* who = "ivx_cw_voxel_row";
    IVX_REQUIRE(a_world && b_world && out, IVX_ERR_INVALID, "%s: null argument", who);
    IVX_REQUIRE(a_world->shape <= IVX_CW_VOXEL_OBJECT && b_world->shape <= IVX_CW_VOXEL_OBJECT, IVX_ERR_INVALID,
                "%s: shapes %u, %u (0 sphere, 1 plane, 2 capsule, 3 voxel object)", who, a_world->shape, b_world->shape);
    IVX_REQUIRE(a_world->shape == IVX_CW_VOXEL_OBJECT || b_world->shape == IVX_CW_VOXEL_OBJECT, IVX_ERR_INVALID, "%s: neither member is a voxel object", who);
    ivx_cw_rows::Member m[2];
    for (int k = 0; k < 2; ++k) {
        const ivx_collidable* c = k ? b_world : a_world;
        const float* pose = k ? pose_b : pose_a;
        const ivx_cw_voxel_object* v = k ? voxel_b : voxel_a;
        const bool voxel = c->shape == IVX_CW_VOXEL_OBJECT;
        IVX_REQUIRE(!voxel || (pose && v), IVX_ERR_INVALID, "%s: member %c is a voxel object and needs its body's pose and its record", who, k ? 'b' : 'a');
        m[k].c = c, m[k].index = (uint32_t)k;
        m[k].pose = voxel ? pose : nullptr;
        m[k].origin_offset = voxel ? v->origin_offset : nullptr, m[k].center_of_mass = voxel ? v->center_of_mass : nullptr;
    }
    ivx_cw_rows::voxel_row(m[0], m[1], out);
    return IVX_OK;
}

int ivx_cw_set_voxel_objects(ivx_world* w, const uint32_t* collidable_index, const ivx_cw_voxel_object* objects, size_t n) {
    const char* who = "ivx_cw_set_voxel_objects";
    IVX_REQUIRE(w && ((collidable_index && objects) || n == 0), IVX_ERR_INVALID, "%s: null argument", who);
    CwState* st = static_cast<CwState*>(w->cw_state);
    IVX_REQUIRE(st && st->has_collidables, IVX_ERR_STATE, "%s: the world holds no collidables (call ivx_cw_set_collidables first)", who);
    static thread_local std::vector<ivx_cw_voxel_object> fresh;
    fresh.assign(st->n, ivx_cw_voxel_object{});
    for (size_t k = 0; k < n; ++k) {
        const uint32_t i = collidable_index[k];
        IVX_REQUIRE(i < st->n, IVX_ERR_INVALID, "%s: attachment %zu names collidable %u, the world has %u", who, k, i, st->n);
        IVX_REQUIRE(st->shapes[i] == IVX_CW_VOXEL_OBJECT, IVX_ERR_INVALID, "%s: attachment %zu: collidable %u has shape %u, not a voxel object", who, k, i, (uint32_t)st->shapes[i]);
        IVX_REQUIRE(objects[k].grid, IVX_ERR_INVALID, "%s: attachment %zu: null grid", who, k);
        IVX_REQUIRE(objects[k].grid->ctx == w->ctx, IVX_ERR_INVALID, "%s: attachment %zu: the grid belongs to another context than the world", who, k);
        IVX_REQUIRE(!fresh[i].grid, IVX_ERR_INVALID, "%s: collidable %u is named twice", who, i);
        fresh[i] = objects[k];
    }
    ivx_ctx* c = w->ctx;
    ivx_many_other_context other_(c);
    if (st->n_voxel) {  // (a set without voxel collidables took no attachment above and has no device array)
        IVX_HIP_CHECK(ivx_stream_sync(c->stream));
        if (int rc = ivx_staging_for(&st->staging_rows, (size_t)st->n * sizeof(CwVoxel))) return rc;
        CwVoxel* h = static_cast<CwVoxel*>(st->staging_rows.p);
        memset(h, 0, (size_t)st->n * sizeof(CwVoxel));
        for (uint32_t i = 0; i < st->n; ++i)
            if (fresh[i].grid) {
                for (int d = 0; d < 3; ++d) h[i].origin_offset[d] = fresh[i].origin_offset[d], h[i].center_of_mass[d] = fresh[i].center_of_mass[d];
                h[i].attached = 1u;
            }
        IVX_HIP_CHECK(ivx_memcpy_sync(st->voxel_dev.p, h, (size_t)st->n * sizeof(CwVoxel), hipMemcpyHostToDevice));
    }
    st->objects = fresh;
    return IVX_OK;
}

int ivx_cw_rows_download(ivx_world* w, ivx_cw_row* rows, size_t cap, size_t* n_rows) {
    const char* who = "ivx_cw_rows_download";
    IVX_REQUIRE(n_rows, IVX_ERR_INVALID, "%s: null argument", who);
    *n_rows = 0;
    CwState* st;
    if (int rc = synchronized_state(w, who, &st)) return rc;
    *n_rows = st->n_rows;
    IVX_REQUIRE(cap >= st->n_rows, IVX_ERR_CAPACITY, "%s: the last frame has %zu rows, the buffer holds %zu", who, st->n_rows, cap);
    IVX_REQUIRE(rows || st->n_rows == 0, IVX_ERR_INVALID, "%s: null buffer", who);
    if (st->n_rows == 0) return IVX_OK;
    ivx_many_other_context other_(w->ctx);
    IVX_HIP_CHECK(ivx_memcpy_async(rows, st->rows.p, st->n_rows * sizeof(ivx_cw_row), hipMemcpyDeviceToHost, w->ctx->stream));
    IVX_HIP_CHECK(ivx_stream_sync(w->ctx->stream));
    return IVX_OK;
}

int ivx_cw_set_broad_phase(ivx_world* w, uint32_t which) {
    const char* who = "ivx_cw_set_broad_phase";
    IVX_REQUIRE(w, IVX_ERR_INVALID, "%s: null world", who);
    IVX_REQUIRE(which <= IVX_CW_BROAD_HIERARCHY, IVX_ERR_INVALID, "%s: broad phase %u (0 = flat, 1 = hierarchy)", who, which);
    CwState* st;
    if (int rc = state_of(w, &st)) return rc;
    st->broad_phase = which;
    return IVX_OK;
}

void* ivx_cw_device_ptr(ivx_world* w, int which) {
    if (!w || !w->cw_state) return nullptr;
    CwState* st = static_cast<CwState*>(w->cw_state);
    switch (which) {
        case IVX_CW_PTR_WORLD_COLLIDABLES: return st->synchronized && st->n ? st->world.p : nullptr;
        case IVX_CW_PTR_CONTACTS: return st->contacts.p;
        case IVX_CW_PTR_DEFERRED_PAIRS: return st->deferred.p;
        case IVX_CW_PTR_FRAME_CONTACTS: return st->contacts.p;
        case IVX_CW_PTR_VOXEL_ROWS: return st->rows.p;
        default: return nullptr;
    }
}

}  // extern "C"
