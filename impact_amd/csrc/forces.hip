// Force generators and dynamic gravity on the device: the reference's ForceGeneratorManager::apply_forces_and_torques
// (impact_physics/src/force.rs:130-159) as the last stage of the step, behind the motion drivers.
//
// Reference behaviour reproduced (engine/crates/impact_physics/src/force):
//   ConstantAcceleration::apply                        constant_acceleration.rs:96-102
//   LocalForceGenerator::apply                         local_force.rs:37-62
//   DynamicDynamicSpringForceGenerator::apply          spring_force.rs:140-189, Spring::scalar_force :317-331
//   DynamicKinematicSpringForceGenerator::apply        spring_force.rs:191-243
//   DynamicGravityManager::compute_and_apply           dynamic_gravity.rs:103-231
//   AlignmentTorqueGenerator::apply                    alignment_torque.rs:107-241
//   DetailedDragForce::apply                           detailed_drag.rs:200-243, drag_load.rs:42-67 (the maps: drag.hip)
//   reset of all bodies, then the phases in order      force.rs:130-159
//
// ONE text for host and device, as in motion.hip: the evaluation functions (fg_spring, fg_alignment, fg_pair), the composition of one body
// (fg_apply_body) and the walk of one field member over its partners (fg_pair_take) are shared with ivx_fg_apply_host. f32 throughout, no
// contraction, IEEE sqrt / div, the operation order of the reference (stated once per kind in include/impact_voxel_hip.h); acos goes through
// double precision rounded once (physics_internal.hpp, acos_rn), and so does the drag phase's atan2.
//
// DETAILED DRAG is a set of its own (a registry of its own in the reference): generators sorted stably by body, in CSR form over the dynamic
// bodies beside the entries of the other kinds. Its maps are resident in the world (FgMedia: a slot table of device allocations, the medium),
// a table of {map address, n_theta} per slot travels with the plan. The table's base and the medium are wave-uniform (kernel arguments); the
// generator, its table row and the map cell are per lane: one 24-byte gather per generator.
//
// EVERY BODY'S SUMS ARE MADE BY ONE LANE IN A FIXED ORDER; there is no float atomic. The host sorts once per set call: per dynamic body the
// list of its entries (generator | role << 31), stably by (phase, list index), in CSR form over ALL dynamic bodies (the reset touches all of
// them). A dynamic-dynamic spring yields two entries; both lanes evaluate the same force_on_2 from the same operands by the same instructions
// and each takes its own end. A lane reads what it needs of the other body field by field and never its totals, which that body's lane is
// writing; it stores its own totals only.
//
// Kernels:
//   k_fg_gravity_records  a lane per field member, 256-thread workgroups: the 64-byte GravitationalBody record (mass, world-space inertia,
//                         position) of synchronize_bodies. A pre-pass, so the two 3x3 products are made once per member and step and not once
//                         per member and workgroup while staging.
//   k_fg_gravity          the tiled N-body kernel. A lane per field member, ONE WAVE per workgroup (64 threads: a 4 096-body field is 64
//                         workgroups on 64 CUs, where 256 threads would use 16), partners staged through LDS in tiles of 64 records (4 KiB).
//                         Inside a tile every lane reads the same record: an LDS broadcast. The lane walks ALL partners in ascending rank,
//                         evaluates each pair with the lower rank as body_i, and takes +force_i, torque_i as the lower rank, -force_i,
//                         torque_j as the higher: per body the very order of the reference's double loop, at twice its arithmetic.
//   k_fg_apply            a lane per dynamic body, 256-thread workgroups, no LDS: reset, the body's entries in phase order, the resident
//                         gravity load at gravity's place.
//   k_fg_apply_drag       the same with the body's drag generators ahead of the gravity load: launched instead of k_fg_apply while a drag set
//                         is installed (the launch count stays).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ivx_internal.hpp"
#include "device_common.hpp"
#include "drag_internal.hpp"
#include "physics_internal.hpp"
#include "vec3.hpp"

namespace {

using namespace ivx_vec;  // V3, Q4, mk, ld3, st3, the operators, dot, cross, qrot
using ivx_phys::acos_rn;
using ivx_phys::atan2_rn;

#define FG_HD __host__ __device__ __forceinline__

#define FG_EPSILON 1.1920929e-07f  // f32::EPSILON
#define FG_GRAVITY_EPS 1e-6f       // dynamic_gravity.rs:194
#define FG_TILE 64u                // records per LDS tile = threads per workgroup of k_fg_gravity
#define FG_NOT_IN_FIELD 0xFFFFFFFFu
#define FG_ROLE_SECOND 0x80000000u  // entry bit: this body is body_b of a dynamic-dynamic spring

// the 3x3 arithmetic of physics.hip (glam Mat3A: column-major, M v = (c0 * x + c1 * y) + c2 * z), here for host and device
struct M3 {
    V3 c0, c1, c2;
};
FG_HD Q4 ldq(const float* p) { return Q4{p[0], p[1], p[2], p[3]}; }
FG_HD M3 ldm(const float* p) { return M3{ld3(p), ld3(p + 3), ld3(p + 6)}; }
FG_HD V3 mul(const M3& m, V3 v) { return (m.c0 * v.x + m.c1 * v.y) + m.c2 * v.z; }
FG_HD M3 transpose(const M3& m) { return {{m.c0.x, m.c1.x, m.c2.x}, {m.c0.y, m.c1.y, m.c2.y}, {m.c0.z, m.c1.z, m.c2.z}}; }
FG_HD M3 mul(const M3& a, const M3& b) { return {mul(a, b.c0), mul(a, b.c1), mul(a, b.c2)}; }
FG_HD M3 m3_from_quat(Q4 q) {  // glam Mat3A::from_quat
    const float x2 = q.x + q.x, y2 = q.y + q.y, z2 = q.z + q.z;
    const float xx = q.x * x2, xy = q.x * y2, xz = q.x * z2;
    const float yy = q.y * y2, yz = q.y * z2, zz = q.z * z2;
    const float wx = q.w * x2, wy = q.w * y2, wz = q.w * z2;
    return {{1.0f - (yy + zz), xy + wz, xz - wy}, {xy - wz, 1.0f - (xx + zz), yz + wx}, {xz + wy, yz - wx, 1.0f - (xx + yy)}};
}
FG_HD M3 rotated(const M3& m, Q4 q) {  // R M R^T (inertia.rs:401-404, 429-432)
    const M3 r = m3_from_quat(q);
    return mul(mul(r, m), transpose(r));
}
FG_HD V3 div_elem(V3 a, float s) { return {a.x / s, a.y / s, a.z / s}; }  // glam Vec3A / f32
FG_HD V3 div_recip(V3 a, float s) {                                       // impact_math Vector3 / f32: a * s.recip()
    const float r = 1.0f / s;
    return {a.x * r, a.y * r, a.z * r};
}
// AngularVelocity::from_vector(..).as_vector() (quantities.rs:160-172): unit axis times speed, zero at or below f32::EPSILON
FG_HD V3 angvel_roundtrip(V3 w) {
    const float n2 = dot(w, w);
    if (n2 > FG_EPSILON * FG_EPSILON) {
        const float n = sqrtf(n2);
        return div_elem(w, n) * n;
    }
    return mk(0.0f, 1.0f, 0.0f) * 0.0f;
}
// DynamicRigidBody::compute_angular_velocity().as_vector(); reads inv_inertia, orientation, angular_momentum
FG_HD V3 dyn_angular_velocity(const ivx_rigid_body& b) {
    return angvel_roundtrip(mul(rotated(ldm(b.inv_inertia), ldq(b.orientation)), ld3(b.angular_momentum)));
}

// ---- springs -----------------------------------------------------------------------------------------------------------------------------
// one end of a spring: what the generator reads of the body it is attached to (never the totals)
struct FgEnd {
    V3 position, attachment;  // centre of mass; attachment point in world space
    V3 velocity, angular;     // filled in only when the spring is damped
};
FG_HD void fg_end_dynamic(const ivx_rigid_body& b, V3 local, bool damped, FgEnd* e) {
    e->position = ld3(b.position);
    e->attachment = e->position + qrot(ldq(b.orientation), local);
    e->velocity = e->angular = mk(0.0f, 0.0f, 0.0f);
    if (damped) {
        e->velocity = div_recip(ld3(b.momentum), b.mass);
        e->angular = dyn_angular_velocity(b);
    }
}
FG_HD void fg_end_kinematic(const ivx_kinematic_body& k, V3 local, bool damped, FgEnd* e) {
    e->position = ld3(k.position);
    e->attachment = e->position + qrot(ldq(k.orientation), local);
    e->velocity = e->angular = mk(0.0f, 0.0f, 0.0f);
    if (damped) {
        e->velocity = ld3(k.velocity);
        e->angular = ld3(k.angular_axis) * k.angular_speed;
    }
}
// force_on_2 of the spring between two ends; false: no force (the ends coincide)
FG_HD bool fg_spring(const FgEnd& e1, const FgEnd& e2, const float* p, bool damped, V3* force_on_2) {
    const float stiffness = p[6], damping = p[7], rest_length = p[8], slack_length = p[9];
    const V3 d = e2.attachment - e1.attachment;
    const float n2 = dot(d, d);
    if (!(n2 > FG_EPSILON * FG_EPSILON)) return false;
    const float length = sqrtf(n2);
    const V3 dir = div_elem(d, length);
    float rate = 0.0f;
    if (damped) {
        const V3 v1 = e1.velocity + cross(e1.angular, e1.attachment - e1.position);
        const V3 v2 = e2.velocity + cross(e2.angular, e2.attachment - e2.position);
        rate = dot(v2, dir) - dot(v1, dir);
    }
    const float scalar = length <= slack_length ? 0.0f : (-stiffness) * (length - rest_length) + (-damping) * rate;
    *force_on_2 = dir * scalar;
    return true;
}
FG_HD bool fg_spring_damped(const float* p) { return !(fabsf(p[7]) <= FG_EPSILON); }  // abs_diff_eq!(damping, 0.0) is false

// DynamicRigidBody::apply_force (rigid_body.rs:598-603)
FG_HD void fg_add_force(V3& F, V3& T, V3 position, V3 force, V3 at) {
    F = F + force;
    T = T + cross(at - position, force);
}

// ---- alignment torque --------------------------------------------------------------------------------------------------------------------
// glam Vec3A::any_orthonormal_vector (Direction::orthogonal_to)
FG_HD V3 fg_any_orthonormal(V3 v) {
    const float sign = copysignf(1.0f, v.z);
    const float a = -1.0f / (sign + v.z);
    const float b = (v.x * v.y) * a;
    return mk(b, sign + (v.y * v.y) * a, -v.y);
}
FG_HD float fg_clamp_unit(float x) { return x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x); }
// the torque towards `direction` (world, unit)
FG_HD V3 fg_alignment(const ivx_rigid_body& b, const float* p, V3 direction) {
    const float settling_time = p[6];
    const float spin_frequency = p[7] / settling_time, precession_frequency = p[8] / settling_time;
    const Q4 q = ldq(b.orientation);
    const V3 axis = qrot(q, ld3(p));
    const V3 c = cross(direction, axis);
    const float c2 = dot(c, c);
    const V3 rotation_axis = c2 > 1e-8f * 1e-8f ? div_elem(c, sqrtf(c2)) : fg_any_orthonormal(axis);
    const M3 inertia = rotated(ldm(b.inertia), q);
    const V3 momentum = ld3(b.angular_momentum);
    const V3 w = dyn_angular_velocity(b);
    const float speed_rotation = dot(w, rotation_axis);
    const V3 w_rotation = rotation_axis * speed_rotation;
    const float speed_axis = dot(w, axis);
    const V3 w_axis = axis * speed_axis;
    const V3 w_precession = (w - w_rotation) - w_axis;
    const float angle = acos_rn(fg_clamp_unit(dot(direction, axis)));
    // compute_critically_dampened_angular_acceleration (:229-241)
    const float time_constant = 0.25f * settling_time;
    const float natural_frequency = 1.0f / time_constant;
    const float critical_damping = 2.0f * natural_frequency;
    const float acceleration_rotation = (-(natural_frequency * natural_frequency)) * angle - critical_damping * speed_rotation;
    const V3 acceleration = (rotation_axis * acceleration_rotation - w_axis * spin_frequency) - w_precession * precession_frequency;
    return mul(inertia, acceleration) + cross(w, momentum);
}

// ---- dynamic gravity ---------------------------------------------------------------------------------------------------------------------
// GravitationalBody (dynamic_gravity.rs:48-55), 64 bytes
struct FgGravBody {
    float mass;
    float inertia[9];  // world space, column-major
    float position[3];
    float pad[3];
};
static_assert(sizeof(FgGravBody) == 64, "FgGravBody layout");
// GravitationalLoad, padded to two float4
struct FgLoad {
    float force[3], pad0, torque[3], pad1;
};
static_assert(sizeof(FgLoad) == 32, "FgLoad layout");

FG_HD FgGravBody fg_grav_record(const ivx_rigid_body& b) {
    FgGravBody r;
    r.mass = b.mass;
    const M3 m = rotated(ldm(b.inertia), ldq(b.orientation));
    st3(r.inertia, m.c0), st3(r.inertia + 3, m.c1), st3(r.inertia + 6, m.c2);
    st3(r.position, ld3(b.position));
    r.pad[0] = r.pad[1] = r.pad[2] = 0.0f;
    return r;
}
// compute_gravitational_force_and_torques (dynamic_gravity.rs:188-231)
FG_HD void fg_pair(float g, const FgGravBody& bi, const FgGravBody& bj, V3* force_i, V3* torque_i, V3* torque_j) {
    const float m_i = bi.mass, m_j = bj.mass;
    const M3 imat_i = ldm(bi.inertia), imat_j = ldm(bj.inertia);
    const V3 r_vec = ld3(bj.position) - ld3(bi.position);
    const float r_squared = dot(r_vec, r_vec);
    const float r = sqrtf(r_squared);
    const float r_cubed = r_squared * r;
    const float r_to_fifth = r_cubed * r_squared;
    const V3 force_mono = r_vec * (((g * m_i) * m_j) / (r_cubed + FG_GRAVITY_EPS));
    const float quad_scale = (1.5f * g) / (r_to_fifth + FG_GRAVITY_EPS);
    const V3 m_j_imat_i_r = mul(imat_i, r_vec) * m_j;
    const V3 m_i_imat_j_r = mul(imat_j, r_vec) * m_i;
    const V3 sum = m_j_imat_i_r + m_i_imat_j_r;
    const float trace_i = (imat_i.c0.x + imat_i.c1.y) + imat_i.c2.z, trace_j = (imat_j.c0.x + imat_j.c1.y) + imat_j.c2.z;
    const float radial = (m_j * trace_i + m_i * trace_j) - (5.0f * dot(r_vec, sum)) / (r_squared + FG_GRAVITY_EPS);
    const V3 force_quad = (r_vec * radial + sum * 2.0f) * quad_scale;
    *force_i = force_mono + force_quad;
    const float torque_scale = 2.0f * quad_scale;
    *torque_i = cross(r_vec, m_j_imat_i_r) * torque_scale;
    *torque_j = cross(r_vec, m_i_imat_j_r) * torque_scale;
}
// what member `own` (rank k) takes of its pair with `other` (rank j != k): the operands are selected first, so the same instructions run whichever
// end the lane is, and the two ends of a pair see the same force_i
FG_HD FgGravBody fg_select(bool first, const FgGravBody& a, const FgGravBody& b) {
    FgGravBody r;
    r.mass = first ? a.mass : b.mass;
    for (int e = 0; e < 9; ++e) r.inertia[e] = first ? a.inertia[e] : b.inertia[e];
    for (int e = 0; e < 3; ++e) r.position[e] = first ? a.position[e] : b.position[e];
    r.pad[0] = r.pad[1] = r.pad[2] = 0.0f;
    return r;
}
FG_HD void fg_pair_take(float g, const FgGravBody& own, const FgGravBody& other, bool own_is_lower, V3& F, V3& T) {
    const FgGravBody bi = fg_select(own_is_lower, own, other), bj = fg_select(own_is_lower, other, own);  // (by value: registers, no address taken)
    V3 force_i, torque_i, torque_j;
    fg_pair(g, bi, bj, &force_i, &torque_i, &torque_j);
    if (own_is_lower) {
        F = F + force_i;
        T = T + torque_i;
    } else {
        F = F - force_i;
        T = T + torque_j;
    }
}

// ---- detailed drag ---------------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(ivx_uniform_medium) == 16 && sizeof(ivx_drag_generator) == 16 && sizeof(ivx_drag_map_view) == 16 && sizeof(ivx_drag_load) == 24, "drag layouts");
FG_HD bool fg_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }  // (false for NaN)
// DetailedDragForce::apply + DragLoad::compute_world_space_drag_force_and_torque; `maps`: the slot table (device addresses on the device)
FG_HD void fg_drag(const ivx_rigid_body& b, const ivx_drag_generator& gen, const ivx_drag_map_view* maps, const ivx_uniform_medium& medium, V3& F, V3& T) {
    const V3 v_rel = div_recip(ld3(b.momentum), b.mass) - ld3(medium.velocity);
    const float s2 = dot(v_rel, v_rel);
    if (!(s2 > 0.0f)) return;  // at rest in the medium (or NaN)
    const Q4 q = ldq(b.orientation);
    const V3 d = div_recip(qrot(Q4{-q.x, -q.y, -q.z, q.w}, v_rel), sqrtf(s2));
    if (!(fg_finite(d.x) && fg_finite(d.y) && fg_finite(d.z))) return;
    const float phi = atan2_rn(d.y, d.x), theta = acos_rn(fg_clamp_unit(d.z));
    const ivx_drag_map_view map = maps[gen.map];
    const float cell = ivx_drag::PI_F / (float)map.n_theta, inv_cell = 1.0f / cell;
    const ivx_drag_load& load = map.loads[(size_t)ivx_drag::theta_idx_of(theta, inv_cell, map.n_theta) * (2u * map.n_theta) + ivx_drag::phi_idx_of(phi, inv_cell, 2u * map.n_theta)];
    const float fs = (((gen.scaling * gen.scaling) * medium.mass_density) * gen.drag_coefficient) * s2;
    const float ts = gen.scaling * fs;
    F = F + qrot(q, ld3(load.force)) * fs;
    T = T + qrot(q, ld3(load.torque)) * ts;
}
// what the drag phase reads: the generators sorted by body, per body its range of them (null: no drag set), the slot table, the medium
struct FgDrag {
    const ivx_drag_generator* gens;
    const uint32_t* offsets;
    const ivx_drag_map_view* maps;
    ivx_uniform_medium medium;
};

// ---- the composition for ONE body ----------------------------------------------------------------------------------------------------------
// the body's drag generators in list order, then its gravity load (apply_loads): what stands between the springs and the alignment torques
FG_HD void fg_drag_and_gravity(uint32_t body, const ivx_rigid_body& b, const FgDrag& drag, uint32_t rank, const FgLoad* loads, V3& F, V3& T) {
    if (drag.offsets)  // (wave-uniform: a kernel argument)
        for (uint32_t e = drag.offsets[body], end = drag.offsets[body + 1u]; e < end; ++e) fg_drag(b, drag.gens[e], drag.maps, drag.medium, F, T);
    if (rank != FG_NOT_IN_FIELD) {
        F = F + ld3(loads[rank].force);
        T = T + ld3(loads[rank].torque);
    }
}

// reset, then the body's entries [begin, end) in phase order, the drag generators and the gravity load between the springs and the alignment
// torques. `dyn` is the whole array: the other end of a dynamic-dynamic spring is read from it field by field.
FG_HD void fg_apply_body(uint32_t body, const ivx_rigid_body* dyn, const ivx_kinematic_body* kin, const ivx_force_generator* gens, const uint32_t* entries,
                         uint32_t begin, uint32_t end, uint32_t rank, const FgLoad* loads, const FgDrag& drag, V3* force_out, V3* torque_out) {
    const ivx_rigid_body& b = dyn[body];
    const V3 position = ld3(b.position);
    V3 F = mk(0.0f, 0.0f, 0.0f), T = mk(0.0f, 0.0f, 0.0f);
    // (the entries are sorted by phase: those ahead of drag and gravity, that middle ONCE — one inlined copy of it —, then the alignment torques)
    uint32_t e = begin;
    for (; e < end; ++e) {
        const uint32_t entry = entries[e];
        const ivx_force_generator& gen = gens[entry & ~FG_ROLE_SECOND];
        const float* p = gen.p;
        if (gen.kind >= IVX_FG_ALIGNMENT_FIXED) break;
        switch (gen.kind) {
        case IVX_FG_CONSTANT_ACCELERATION: F = F + ld3(p) * b.mass; break;
        case IVX_FG_LOCAL_FORCE: {
            const Q4 q = ldq(b.orientation);
            fg_add_force(F, T, position, qrot(q, ld3(p)), position + qrot(q, ld3(p + 3)));
        } break;
        case IVX_FG_SPRING_DYNAMIC_DYNAMIC: {
            const bool second = (entry & FG_ROLE_SECOND) != 0u, damped = fg_spring_damped(p);
            const ivx_rigid_body& b1 = second ? dyn[gen.body] : b;
            const ivx_rigid_body& b2 = second ? b : dyn[gen.body_b];
            FgEnd e1, e2;
            fg_end_dynamic(b1, ld3(p), damped, &e1);
            fg_end_dynamic(b2, ld3(p + 3), damped, &e2);
            V3 force_on_2;
            if (fg_spring(e1, e2, p, damped, &force_on_2)) {
                if (second) fg_add_force(F, T, position, force_on_2, e2.attachment);
                else fg_add_force(F, T, position, -force_on_2, e1.attachment);
            }
        } break;
        default: {  // IVX_FG_SPRING_DYNAMIC_KINEMATIC (the kinds are validated on the host)
            const bool damped = fg_spring_damped(p);
            FgEnd e1, e2;
            fg_end_dynamic(b, ld3(p), damped, &e1);
            fg_end_kinematic(kin[gen.body_b], ld3(p + 3), damped, &e2);
            V3 force_on_2;
            if (fg_spring(e1, e2, p, damped, &force_on_2)) fg_add_force(F, T, position, -force_on_2, e1.attachment);
        } break;
        }
    }
    fg_drag_and_gravity(body, b, drag, rank, loads, F, T);
    for (; e < end; ++e) {
        const ivx_force_generator& gen = gens[entries[e]];
        const float* p = gen.p;
        V3 direction = ld3(p + 3);  // IVX_FG_ALIGNMENT_FIXED
        if (gen.kind != IVX_FG_ALIGNMENT_FIXED) {  // IVX_FG_ALIGNMENT_GRAVITY
            if (rank == FG_NOT_IN_FIELD) continue;
            const V3 load = ld3(loads[rank].force);
            const float n2 = (load.x * load.x + load.y * load.y) + load.z * load.z;
            if (!(n2 > 1e-9f * 1e-9f)) continue;
            direction = div_recip(load, sqrtf(n2));
        }
        T = T + fg_alignment(b, p, direction);
    }
    *force_out = F, *torque_out = T;
}

__global__ __launch_bounds__(256) void k_fg_gravity_records(const ivx_rigid_body* __restrict__ dyn, const uint32_t* __restrict__ field, uint32_t n_field,
                                                            FgGravBody* __restrict__ records) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_field) return;
    records[i] = fg_grav_record(dyn[field[i]]);  // (field[i] < the world's dynamic bodies: checked on the host before every launch)
}

__global__ __launch_bounds__(FG_TILE) void k_fg_gravity(const FgGravBody* __restrict__ records, uint32_t n_field, float g, FgLoad* __restrict__ loads) {
    __shared__ FgGravBody tile[FG_TILE];
    const uint32_t k = blockIdx.x * FG_TILE + threadIdx.x;
    const bool live = k < n_field;
    FgGravBody own = {};
    if (live) own = records[k];
    V3 F = mk(0.0f, 0.0f, 0.0f), T = mk(0.0f, 0.0f, 0.0f);
    for (uint32_t base = 0; base < n_field; base += FG_TILE) {
        const uint32_t count = n_field - base < FG_TILE ? n_field - base : FG_TILE;
        __syncthreads();  // (the tile before has been read by every lane)
        if (threadIdx.x < count) tile[threadIdx.x] = records[base + threadIdx.x];
        __syncthreads();
        if (live)
            for (uint32_t t = 0; t < count; ++t) {
                const uint32_t j = base + t;
                if (j != k) fg_pair_take(g, own, tile[t], k < j, F, T);
            }
    }
    if (live) {
        FgLoad l;
        st3(l.force, F), st3(l.torque, T);
        l.pad0 = l.pad1 = 0.0f;
        loads[k] = l;
    }
}

// (no __restrict__ on dyn: a lane reads other bodies' configurations and momenta from the array it writes its totals into)
// Two forms of one body: without a drag set the kernel has the argument list and the code it had before the drag phase existed (the null CSR is
// a constant there, and the phase is compiled out); with one it also takes the drag generators, their CSR, the slot table and the medium.
__global__ __launch_bounds__(256) void k_fg_apply(ivx_rigid_body* dyn, uint32_t n_dyn, const ivx_kinematic_body* __restrict__ kin,
                                                  const ivx_force_generator* __restrict__ gens, const uint32_t* __restrict__ offsets,
                                                  const uint32_t* __restrict__ entries, const uint32_t* __restrict__ ranks, const FgLoad* __restrict__ loads) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_dyn) return;
    V3 F, T;
    fg_apply_body(i, dyn, kin, gens, entries, offsets[i], offsets[i + 1u], ranks[i], loads, FgDrag{nullptr, nullptr, nullptr, ivx_uniform_medium{0.0f, {0.0f, 0.0f, 0.0f}}}, &F, &T);
    st3(dyn[i].total_force, F);
    st3(dyn[i].total_torque, T);
}
__global__ __launch_bounds__(256) void k_fg_apply_drag(ivx_rigid_body* dyn, uint32_t n_dyn, const ivx_kinematic_body* __restrict__ kin,
                                                       const ivx_force_generator* __restrict__ gens, const uint32_t* __restrict__ offsets,
                                                       const uint32_t* __restrict__ entries, const uint32_t* __restrict__ ranks, const FgLoad* __restrict__ loads,
                                                       const ivx_drag_generator* __restrict__ drag_gens, const uint32_t* __restrict__ drag_offsets,
                                                       const ivx_drag_map_view* __restrict__ drag_maps, ivx_uniform_medium medium) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_dyn) return;
    V3 F, T;
    fg_apply_body(i, dyn, kin, gens, entries, offsets[i], offsets[i + 1u], ranks[i], loads, FgDrag{drag_gens, drag_offsets, drag_maps, medium}, &F, &T);
    st3(dyn[i].total_force, F);
    st3(dyn[i].total_torque, T);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
const char* const FG_KIND_NAMES[6] = {"constant acceleration", "local force", "dynamic-dynamic spring", "dynamic-kinematic spring",
                                      "fixed-direction alignment torque", "gravity alignment torque"};

int fg_validate(const char* who, const ivx_force_generator* gens, size_t n, size_t n_dyn, size_t n_kin) {
    for (size_t i = 0; i < n; ++i) {
        const ivx_force_generator& g = gens[i];
        IVX_REQUIRE(g.kind <= IVX_FG_ALIGNMENT_GRAVITY, IVX_ERR_INVALID,
                    "%s: generator %zu has kind %u (0 constant acceleration, 1 local force, 2 dynamic-dynamic spring, 3 dynamic-kinematic spring, 4 fixed-direction "
                    "alignment, 5 gravity alignment)",
                    who, i, g.kind);
        const char* name = FG_KIND_NAMES[g.kind];
        IVX_REQUIRE(g.body < n_dyn, IVX_ERR_INVALID, "%s: generator %zu (%s) acts on dynamic body %u, there are %zu", who, i, name, g.body, n_dyn);
        if (g.kind == IVX_FG_SPRING_DYNAMIC_DYNAMIC) {
            IVX_REQUIRE(g.body_b < n_dyn, IVX_ERR_INVALID, "%s: generator %zu (%s) has dynamic body %u at its second end, there are %zu", who, i, name, g.body_b, n_dyn);
            IVX_REQUIRE(g.body_b != g.body, IVX_ERR_INVALID, "%s: generator %zu (%s) has body %u at both ends", who, i, name, g.body);
        } else if (g.kind == IVX_FG_SPRING_DYNAMIC_KINEMATIC) {
            IVX_REQUIRE(g.body_b < n_kin, IVX_ERR_INVALID, "%s: generator %zu (%s) has kinematic body %u at its second end, there are %zu", who, i, name, g.body_b, n_kin);
        } else if (g.kind >= IVX_FG_ALIGNMENT_FIXED) {
            IVX_REQUIRE(g.p[6] > 0.0f, IVX_ERR_INVALID, "%s: generator %zu (%s): the settling time %g does not exceed zero", who, i, name, (double)g.p[6]);
        }
    }
    return IVX_OK;
}
int fg_validate_field(const char* who, const uint32_t* field, size_t n, size_t n_dyn) {
    std::vector<uint8_t> seen(n_dyn, 0);
    for (size_t i = 0; i < n; ++i) {
        IVX_REQUIRE(field[i] < n_dyn, IVX_ERR_INVALID, "%s: field member %zu is dynamic body %u, there are %zu", who, i, field[i], n_dyn);
        IVX_REQUIRE(!seen[field[i]], IVX_ERR_INVALID, "%s: field member %zu: dynamic body %u is already included in the field", who, i, field[i]);
        seen[field[i]] = 1;
    }
    return IVX_OK;
}

// detailed-drag generators against `n_dyn` bodies and a slot table of `n_maps` rows, of which has_map(row) says whether it holds a map
template <typename HasMap>
int fg_validate_drag(const char* who, const ivx_drag_generator* gens, size_t n, size_t n_dyn, size_t n_maps, HasMap has_map) {
    for (size_t i = 0; i < n; ++i) {
        const ivx_drag_generator& g = gens[i];
        IVX_REQUIRE(g.body < n_dyn, IVX_ERR_INVALID, "%s: generator %zu (detailed drag) acts on dynamic body %u, there are %zu", who, i, g.body, n_dyn);
        IVX_REQUIRE(g.map < n_maps, IVX_ERR_INVALID, "%s: generator %zu (detailed drag) names map slot %u, the table has %zu", who, i, g.map, n_maps);
        IVX_REQUIRE(has_map(g.map), IVX_ERR_INVALID, "%s: generator %zu (detailed drag) names map slot %u, which holds no drag load map", who, i, g.map);
    }
    return IVX_OK;
}

// the plan of the sets over n_dyn dynamic bodies: per body its entries in CSR form, stably by (phase, list index) — the phase of a kind is
// the kind, the two alignment kinds sharing one (they share one registry in the reference) — and its rank in the field
// The drag set is a second CSR: its generators sorted stably by body (list order inside a body), and per body its range of them.
struct FgPlan {
    std::vector<uint32_t> offsets, entries, ranks, drag_offsets;
    std::vector<ivx_drag_generator> drag_sorted;
};
void fg_build_drag_plan(const ivx_drag_generator* drag, size_t n_drag, size_t n_dyn, FgPlan* plan) {
    plan->drag_sorted.assign(drag, drag + n_drag);
    plan->drag_offsets.clear();
    if (n_drag == 0) return;
    std::stable_sort(plan->drag_sorted.begin(), plan->drag_sorted.end(), [](const ivx_drag_generator& x, const ivx_drag_generator& y) { return x.body < y.body; });
    plan->drag_offsets.assign(n_dyn + 1, 0);
    for (const ivx_drag_generator& g : plan->drag_sorted) plan->drag_offsets[g.body + 1]++;
    for (size_t b = 0; b < n_dyn; ++b) plan->drag_offsets[b + 1] += plan->drag_offsets[b];
}
void fg_build_plan(const ivx_force_generator* gens, size_t n, const uint32_t* field, size_t n_field, size_t n_dyn, FgPlan* plan) {
    struct Entry {
        uint32_t body, phase, entry;
    };
    std::vector<Entry> all;
    all.reserve(n + n / 2);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t phase = gens[i].kind < IVX_FG_ALIGNMENT_FIXED ? gens[i].kind : (uint32_t)IVX_FG_ALIGNMENT_FIXED;
        all.push_back(Entry{gens[i].body, phase, (uint32_t)i});
        if (gens[i].kind == IVX_FG_SPRING_DYNAMIC_DYNAMIC) all.push_back(Entry{gens[i].body_b, phase, (uint32_t)i | FG_ROLE_SECOND});
    }
    std::stable_sort(all.begin(), all.end(), [](const Entry& x, const Entry& y) { return x.body != y.body ? x.body < y.body : x.phase < y.phase; });
    plan->offsets.assign(n_dyn + 1, 0);
    plan->entries.resize(all.size());
    for (size_t e = 0; e < all.size(); ++e) {
        plan->entries[e] = all[e].entry;
        plan->offsets[all[e].body + 1]++;
    }
    for (size_t b = 0; b < n_dyn; ++b) plan->offsets[b + 1] += plan->offsets[b];
    plan->ranks.assign(n_dyn, FG_NOT_IN_FIELD);
    for (size_t r = 0; r < n_field; ++r) plan->ranks[field[r]] = (uint32_t)r;
}

// the world's medium and its drag load maps: a table of slots, each a device allocation of its own (a map is replaced in place, stream-ordered,
// while it fits). They belong to the world and outlive the sets.
#define FG_MAX_MAP_SLOTS 65536u
struct FgMedia {
    ivx_uniform_medium medium = {0.0f, {0.0f, 0.0f, 0.0f}};  // UniformMedium::vacuum()
    struct Slot {
        ivx_buf buf;
        uint32_t n_theta = 0;  // 0: no map
    };
    std::vector<Slot> slots;
};

// world-owned state: the sets as the caller gave them, and one device allocation (generators | offsets | entries | ranks | field | loads | drag
// generators | drag offsets | slot table, uploaded; then the gravity records, device-only) that only grows, with the pinned block its upload goes through. The plan is made for a
// number of dynamic bodies; a world whose bodies have been replaced by another number since gets a new one at its next apply.
struct FgState {
    std::vector<ivx_force_generator> gens;
    std::vector<uint32_t> field;
    std::vector<ivx_drag_generator> drag;
    float g = 1.0f;
    ivx_buf dev;
    ivx_staging staging;
    size_t at_offsets = 0, at_entries = 0, at_ranks = 0, at_field = 0, at_loads = 0, at_records = 0, at_drag = 0, at_drag_offsets = 0, at_maps = 0;
    uint32_t plan_dyn = 0;                // the plan on the device covers this many dynamic bodies
    bool installed = false;               // ... and stands
    uint32_t need_dyn = 0, need_kin = 0;  // the sets were checked against a world of at least this many bodies
};

int fg_install(ivx_world* w, FgState* st) {
    st->installed = false;  // (until this call's plan stands)
    FgPlan plan;
    const size_t n = st->gens.size(), n_field = st->field.size(), n_dyn = w->n_dyn;
    fg_build_plan(st->gens.data(), n, st->field.data(), n_field, n_dyn, &plan);
    fg_build_drag_plan(st->drag.data(), st->drag.size(), n_dyn, &plan);
    const FgMedia* media = static_cast<const FgMedia*>(w->fg_media);
    const size_t n_drag = st->drag.size(), n_slots = n_drag && media ? media->slots.size() : 0;
    ivx_layout l;
    const size_t at_gens = l.take(n * sizeof(ivx_force_generator)), at_offsets = l.take((n_dyn + 1) * 4), at_entries = l.take(plan.entries.size() * 4),
                 at_ranks = l.take(n_dyn * 4), at_field = l.take(n_field * 4), at_loads = l.take(n_field * sizeof(FgLoad)), at_drag = l.take(n_drag * sizeof(ivx_drag_generator)), at_drag_offsets = l.take(plan.drag_offsets.size() * 4),
                 at_maps = l.take(n_slots * sizeof(ivx_drag_map_view));
    const size_t upload = l.bytes;
    const size_t at_records = l.take(n_field * sizeof(FgGravBody));
    if (int rc = ivx_buf_grow(w->ctx, &st->dev, l.bytes, 1u << 12)) return rc;
    if (int rc = ivx_staging_for(&st->staging, upload)) return rc;
    char* h = static_cast<char*>(st->staging.p);
    memset(h, 0, upload);  // (the loads start as the reference's: zero)
    if (n) memcpy(h + at_gens, st->gens.data(), n * sizeof(ivx_force_generator));
    memcpy(h + at_offsets, plan.offsets.data(), (n_dyn + 1) * 4);
    if (!plan.entries.empty()) memcpy(h + at_entries, plan.entries.data(), plan.entries.size() * 4);
    if (n_dyn) memcpy(h + at_ranks, plan.ranks.data(), n_dyn * 4);
    if (n_field) memcpy(h + at_field, st->field.data(), n_field * 4);
    if (n_drag) {
        memcpy(h + at_drag, plan.drag_sorted.data(), n_drag * sizeof(ivx_drag_generator));
        memcpy(h + at_drag_offsets, plan.drag_offsets.data(), plan.drag_offsets.size() * 4);
        ivx_drag_map_view* rows = reinterpret_cast<ivx_drag_map_view*>(h + at_maps);  // (device addresses; a slot without a map stays null and is named by no generator)
        for (size_t s = 0; s < n_slots; ++s)
            if (media->slots[s].n_theta) rows[s] = ivx_drag_map_view{static_cast<const ivx_drag_load*>(media->slots[s].buf.p), media->slots[s].n_theta, 0u};
    }
    // (stream-ordered behind an apply that still reads the plan this one replaces)
    if (int rc = ivx_staging_upload(&st->staging, st->dev.p, upload, w->ctx->stream)) return rc;
    st->at_offsets = at_offsets, st->at_entries = at_entries, st->at_ranks = at_ranks, st->at_field = at_field, st->at_loads = at_loads, st->at_records = at_records;
    st->at_drag = at_drag, st->at_drag_offsets = at_drag_offsets, st->at_maps = at_maps;
    st->plan_dyn = (uint32_t)n_dyn;
    st->installed = true;
    return IVX_OK;
}

void fg_needs(FgState* st) {
    uint32_t need_dyn = 0, need_kin = 0;
    for (const ivx_force_generator& g : st->gens) {
        need_dyn = std::max(need_dyn, g.body + 1u);
        if (g.kind == IVX_FG_SPRING_DYNAMIC_DYNAMIC) need_dyn = std::max(need_dyn, g.body_b + 1u);
        if (g.kind == IVX_FG_SPRING_DYNAMIC_KINEMATIC) need_kin = std::max(need_kin, g.body_b + 1u);
    }
    for (uint32_t b : st->field) need_dyn = std::max(need_dyn, b + 1u);
    for (const ivx_drag_generator& g : st->drag) need_dyn = std::max(need_dyn, g.body + 1u);
    st->need_dyn = need_dyn, st->need_kin = need_kin;
}

void fg_state_release(ivx_world* w) {
    FgState* st = ivx_state_take<FgState>(&w->fg_state);
    if (!st) return;
    ivx_buf_free(&st->dev);
    ivx_staging_release(&st->staging);
    delete st;
}

// after one of the three sets has changed: all gone — the state leaves (the medium and the maps stay); else a new plan
int fg_sets_changed(ivx_world* w, FgState* st) {
    fg_needs(st);
    if (st->gens.empty() && st->field.empty() && st->drag.empty()) {  // (a launch in flight still reads the buffers: wait for it)
        IVX_HIP_CHECK(ivx_stream_sync(w->ctx->stream));
        fg_state_release(w);
        return IVX_OK;
    }
    if (w->n_dyn < st->need_dyn || w->n_kin < st->need_kin) {  // (the other set has outlived its bodies: no plan until both fit — ivx_forces_ready says so)
        st->installed = false;
        return IVX_OK;
    }
    return fg_install(w, st);
}

int fg_state_for(ivx_world* w, const char* who, FgState** out) { return ivx_state_for(&w->fg_state, who, out); }
int fg_media_for(ivx_world* w, const char* who, FgMedia** out) { return ivx_state_for(&w->fg_media, who, out); }
// the slot's rows of the resident table are stale (another address or n_theta): the next apply uploads the plan again
void fg_maps_changed(ivx_world* w) {
    FgState* st = static_cast<FgState*>(w->fg_state);
    if (st && !st->drag.empty()) st->installed = false;
}
bool fg_slot_in_use(const ivx_world* w, uint32_t slot) {
    const FgState* st = static_cast<const FgState*>(w->fg_state);
    if (st)
        for (const ivx_drag_generator& g : st->drag)
            if (g.map == slot) return true;
    return false;
}
// slot `slot` exists and holds room for a map of n_theta rows (its contents are the caller's to write, on the stream)
int fg_slot_for(ivx_world* w, const char* who, uint32_t slot, uint32_t n_theta, FgMedia::Slot** out) {
    IVX_REQUIRE(slot < FG_MAX_MAP_SLOTS, IVX_ERR_CAPACITY, "%s: map slot %u, the table holds at most %u", who, slot, FG_MAX_MAP_SLOTS);
    FgMedia* m;
    if (int rc = fg_media_for(w, who, &m)) return rc;
    if (m->slots.size() <= slot) m->slots.resize((size_t)slot + 1);
    FgMedia::Slot* s = &m->slots[slot];
    // (a buffer that has to grow waits for the stream first: an apply in flight may still read the old one)
    if (int rc = ivx_buf_grow(w->ctx, &s->buf, 2u * (size_t)n_theta * n_theta * sizeof(ivx_drag_load), 1u << 12)) return rc;
    s->n_theta = n_theta;
    fg_maps_changed(w);
    *out = s;
    return IVX_OK;
}

// the whole stage over host arrays; gravity_loads6: 6 floats per field member or null
void fg_apply_host(const ivx_force_generator* gens, size_t n, const uint32_t* field, size_t n_field, float g, ivx_rigid_body* dyn, size_t n_dyn,
                   const ivx_kinematic_body* kin, float* gravity_loads6, const ivx_drag_generator* drag_gens = nullptr, size_t n_drag = 0,
                   const ivx_drag_map_view* maps = nullptr, const ivx_uniform_medium* medium = nullptr) {
    FgPlan plan;
    fg_build_plan(gens, n, field, n_field, n_dyn, &plan);
    fg_build_drag_plan(drag_gens, n_drag, n_dyn, &plan);
    const FgDrag drag = {plan.drag_sorted.data(), n_drag ? plan.drag_offsets.data() : nullptr, maps, medium ? *medium : ivx_uniform_medium{0.0f, {0.0f, 0.0f, 0.0f}}};
    std::vector<FgGravBody> records(n_field);
    std::vector<FgLoad> loads(n_field);
    for (size_t k = 0; k < n_field; ++k) records[k] = fg_grav_record(dyn[field[k]]);
    for (size_t k = 0; k < n_field; ++k) {
        V3 F = mk(0.0f, 0.0f, 0.0f), T = mk(0.0f, 0.0f, 0.0f);
        for (size_t j = 0; j < n_field; ++j)
            if (j != k) fg_pair_take(g, records[k], records[j], k < j, F, T);
        st3(loads[k].force, F), st3(loads[k].torque, T);
        loads[k].pad0 = loads[k].pad1 = 0.0f;
        if (gravity_loads6) st3(gravity_loads6 + 6 * k, F), st3(gravity_loads6 + 6 * k + 3, T);
    }
    for (size_t b = 0; b < n_dyn; ++b) {
        V3 F, T;
        fg_apply_body((uint32_t)b, dyn, kin, gens, plan.entries.data(), plan.offsets[b], plan.offsets[b + 1], plan.ranks[b], loads.data(), drag, &F, &T);
        st3(dyn[b].total_force, F);
        st3(dyn[b].total_torque, T);
    }
}

}  // namespace

void ivx_fg_release(ivx_world* w) {
    if (!w) return;
    fg_state_release(w);
    if (FgMedia* m = ivx_state_take<FgMedia>(&w->fg_media)) {
        for (FgMedia::Slot& s : m->slots) ivx_buf_free(&s.buf);
        delete m;
    }
}

int ivx_forces_ready(ivx_world* w, const char* who) {
    FgState* st = static_cast<FgState*>(w->fg_state);
    if (!st) return IVX_OK;
    IVX_REQUIRE(w->n_dyn >= st->need_dyn && w->n_kin >= st->need_kin, IVX_ERR_STATE,
                "%s: the force generators, the gravity field and the detailed-drag set refer to %u dynamic and %u kinematic bodies, the world now has %u and %u (call "
                "ivx_world_set_force_generators / ivx_world_set_dynamic_gravity / ivx_world_set_detailed_drag again)",
                who, st->need_dyn, st->need_kin, w->n_dyn, w->n_kin);
    return IVX_OK;
}

int ivx_launch_forces_apply(ivx_world* w, const char* who) {
    FgState* st = static_cast<FgState*>(w->fg_state);
    if (!st) return IVX_OK;
    if (int rc = ivx_forces_ready(w, who)) return rc;
    if (!st->installed || st->plan_dyn != w->n_dyn)  // (the bodies have been replaced by another number since the plan was made)
        if (int rc = fg_install(w, st)) return rc;
    if (w->n_dyn == 0) return IVX_OK;
    char* base = static_cast<char*>(st->dev.p);
    const uint32_t n_field = (uint32_t)st->field.size();
    FgLoad* loads = reinterpret_cast<FgLoad*>(base + st->at_loads);
    if (n_field) {
        FgGravBody* records = reinterpret_cast<FgGravBody*>(base + st->at_records);
        IVX_KLAUNCH(k_fg_gravity_records, dim3((n_field + 255u) / 256u), dim3(256), 0, w->ctx->stream, w->dyn.p, reinterpret_cast<const uint32_t*>(base + st->at_field), n_field,
                    records);
        IVX_KLAUNCH(k_fg_gravity, dim3((n_field + FG_TILE - 1u) / FG_TILE), dim3(FG_TILE), 0, w->ctx->stream, records, n_field, st->g, loads);
    }
    const ivx_force_generator* d_gens = reinterpret_cast<const ivx_force_generator*>(base);
    const uint32_t *d_offsets = reinterpret_cast<const uint32_t*>(base + st->at_offsets), *d_entries = reinterpret_cast<const uint32_t*>(base + st->at_entries),
                   *d_ranks = reinterpret_cast<const uint32_t*>(base + st->at_ranks);
    if (st->drag.empty())
        IVX_KLAUNCH(k_fg_apply, dim3((w->n_dyn + 255u) / 256u), dim3(256), 0, w->ctx->stream, w->dyn.p, w->n_dyn, w->kin.p, d_gens, d_offsets, d_entries, d_ranks, loads);
    else
        IVX_KLAUNCH(k_fg_apply_drag, dim3((w->n_dyn + 255u) / 256u), dim3(256), 0, w->ctx->stream, w->dyn.p, w->n_dyn, w->kin.p, d_gens, d_offsets, d_entries, d_ranks, loads,
                    reinterpret_cast<const ivx_drag_generator*>(base + st->at_drag), reinterpret_cast<const uint32_t*>(base + st->at_drag_offsets),
                    reinterpret_cast<const ivx_drag_map_view*>(base + st->at_maps), static_cast<const FgMedia*>(w->fg_media)->medium);
    IVX_HIP_CHECK(hipGetLastError());
    return IVX_OK;
}

extern "C" {

int ivx_world_set_force_generators(ivx_world* w, const ivx_force_generator* gens, size_t n) {
    const char* who = "ivx_world_set_force_generators";
    IVX_REQUIRE(w && (gens || n == 0), IVX_ERR_INVALID, "%s: null argument", who);
    IVX_REQUIRE(n < (1u << 24), IVX_ERR_CAPACITY, "%s: more than 2^24 generators", who);
    if (n == 0 && !w->fg_state) return IVX_OK;
    if (int rc = fg_validate(who, gens, n, w->n_dyn, w->n_kin)) return rc;
    FgState* st;
    if (int rc = fg_state_for(w, who, &st)) return rc;
    st->gens.assign(gens, gens + n);
    return fg_sets_changed(w, st);
}

int ivx_world_set_dynamic_gravity(ivx_world* w, const uint32_t* bodies, size_t n, float gravitational_constant) {
    const char* who = "ivx_world_set_dynamic_gravity";
    IVX_REQUIRE(w && (bodies || n == 0), IVX_ERR_INVALID, "%s: null argument", who);
    if (n == 0 && !w->fg_state) return IVX_OK;
    if (int rc = fg_validate_field(who, bodies, n, w->n_dyn)) return rc;
    FgState* st;
    if (int rc = fg_state_for(w, who, &st)) return rc;
    st->field.assign(bodies, bodies + n);
    st->g = gravitational_constant;
    return fg_sets_changed(w, st);
}

int ivx_world_apply_forces(ivx_world* w) {
    IVX_REQUIRE(w, IVX_ERR_INVALID, "ivx_world_apply_forces: null world");
    return ivx_launch_forces_apply(w, "ivx_world_apply_forces");
}

int ivx_world_gravity_loads(ivx_world* w, float* out, size_t cap) {
    const char* who = "ivx_world_gravity_loads";
    IVX_REQUIRE(w, IVX_ERR_INVALID, "%s: null world", who);
    FgState* st = static_cast<FgState*>(w->fg_state);
    const size_t n_field = st ? st->field.size() : 0;
    if (n_field == 0) return IVX_OK;
    IVX_REQUIRE(out, IVX_ERR_INVALID, "%s: null argument", who);
    IVX_REQUIRE(cap >= n_field, IVX_ERR_CAPACITY, "%s: room for %zu loads, the field has %zu bodies", who, cap, n_field);
    IVX_REQUIRE(st->installed, IVX_ERR_STATE, "%s: the sets are not resident (an earlier call failed)", who);
    std::vector<FgLoad> loads(n_field);
    IVX_HIP_CHECK(ivx_stream_sync(w->ctx->stream));
    IVX_HIP_CHECK(ivx_memcpy_sync(loads.data(), static_cast<char*>(st->dev.p) + st->at_loads, n_field * sizeof(FgLoad), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < n_field; ++k) {
        memcpy(out + 6 * k, loads[k].force, 12);
        memcpy(out + 6 * k + 3, loads[k].torque, 12);
    }
    return IVX_OK;
}

int ivx_fg_apply_host(const ivx_force_generator* gens, size_t n, const uint32_t* gravity_bodies, size_t n_gravity, float gravitational_constant, ivx_rigid_body* dynamic,
                      size_t n_dynamic, const ivx_kinematic_body* kinematic, size_t n_kinematic, float* gravity_loads6) {
    const char* who = "ivx_fg_apply_host";
    IVX_REQUIRE((gens || n == 0) && (gravity_bodies || n_gravity == 0) && (dynamic || n_dynamic == 0) && (kinematic || n_kinematic == 0), IVX_ERR_INVALID, "%s: null argument",
                who);
    if (int rc = fg_validate(who, gens, n, n_dynamic, n_kinematic)) return rc;
    if (int rc = fg_validate_field(who, gravity_bodies, n_gravity, n_dynamic)) return rc;
    fg_apply_host(gens, n, gravity_bodies, n_gravity, gravitational_constant, dynamic, n_dynamic, kinematic, gravity_loads6);
    return IVX_OK;
}

int ivx_world_set_medium(ivx_world* w, const ivx_uniform_medium* medium) {
    const char* who = "ivx_world_set_medium";
    IVX_REQUIRE(w && medium, IVX_ERR_INVALID, "%s: null argument", who);
    FgMedia* m;
    if (int rc = fg_media_for(w, who, &m)) return rc;
    m->medium = *medium;  // (a kernel argument of the next apply)
    return IVX_OK;
}

int ivx_world_medium(ivx_world* w, ivx_uniform_medium* out) {
    IVX_REQUIRE(w && out, IVX_ERR_INVALID, "ivx_world_medium: null argument");
    *out = w->fg_media ? static_cast<const FgMedia*>(w->fg_media)->medium : ivx_uniform_medium{0.0f, {0.0f, 0.0f, 0.0f}};
    return IVX_OK;
}

int ivx_world_set_drag_map(ivx_world* w, uint32_t slot, const ivx_drag_load* map, uint32_t n_theta) {
    const char* who = "ivx_world_set_drag_map";
    IVX_REQUIRE(w && (map || n_theta == 0), IVX_ERR_INVALID, "%s: null argument", who);
    IVX_REQUIRE(slot < FG_MAX_MAP_SLOTS, IVX_ERR_CAPACITY, "%s: map slot %u, the table holds at most %u", who, slot, FG_MAX_MAP_SLOTS);
    IVX_REQUIRE(n_theta <= ivx_drag::MAX_THETA, IVX_ERR_CAPACITY, "%s: n_theta_coords %u exceeds %u", who, n_theta, ivx_drag::MAX_THETA);
    if (n_theta == 0) {  // free the slot
        FgMedia* m = static_cast<FgMedia*>(w->fg_media);
        if (!m || slot >= m->slots.size() || m->slots[slot].n_theta == 0) return IVX_OK;
        IVX_REQUIRE(!fg_slot_in_use(w, slot), IVX_ERR_STATE, "%s: map slot %u is named by the installed detailed-drag set (replace or remove the set first)", who, slot);
        IVX_HIP_CHECK(ivx_stream_sync(w->ctx->stream));  // (nothing in flight reads it any more; a later set that names it is refused)
        ivx_buf_free(&m->slots[slot].buf);
        m->slots[slot].n_theta = 0;
        return IVX_OK;
    }
    FgMedia::Slot* s;
    if (int rc = fg_slot_for(w, who, slot, n_theta, &s)) return rc;
    // on the stream, behind an apply that still reads the map this one replaces; `map` is the caller's pageable memory: wait until it has left
    IVX_HIP_CHECK(ivx_memcpy_async(s->buf.p, map, 2u * (size_t)n_theta * n_theta * sizeof(ivx_drag_load), hipMemcpyHostToDevice, w->ctx->stream));
    IVX_HIP_CHECK(ivx_stream_sync(w->ctx->stream));
    return IVX_OK;
}

int ivx_world_set_drag_map_from_grid(ivx_world* w, uint32_t slot, ivx_grid* g, const float com[3], const ivx_drag_map_config* cfg) {
    const char* who = "ivx_world_set_drag_map_from_grid";
    IVX_REQUIRE(w && g && com && cfg, IVX_ERR_INVALID, "%s: null argument", who);
    IVX_REQUIRE(g->ctx == w->ctx, IVX_ERR_INVALID, "%s: the grid belongs to another context than the world", who);
    IVX_REQUIRE(slot < FG_MAX_MAP_SLOTS, IVX_ERR_CAPACITY, "%s: map slot %u, the table holds at most %u", who, slot, FG_MAX_MAP_SLOTS);
    if (int rc = ivx_drag_map_check(who, g, com, cfg)) return rc;  // (before the slot changes)
    FgMedia::Slot* s;
    if (int rc = fg_slot_for(w, who, slot, cfg->n_theta_coords, &s)) return rc;
    return ivx_drag_map_build(who, g, com, cfg, static_cast<float*>(s->buf.p), nullptr);  // (enqueued: the map never crosses to the host)
}

int ivx_world_drag_map_download(ivx_world* w, uint32_t slot, ivx_drag_load* map, size_t cap_cells, uint32_t* n_theta) {
    const char* who = "ivx_world_drag_map_download";
    IVX_REQUIRE(w && n_theta, IVX_ERR_INVALID, "%s: null argument", who);
    *n_theta = 0;
    const FgMedia* m = static_cast<const FgMedia*>(w->fg_media);
    if (!m || slot >= m->slots.size() || m->slots[slot].n_theta == 0) return IVX_OK;
    const FgMedia::Slot& s = m->slots[slot];
    const size_t cells = 2u * (size_t)s.n_theta * s.n_theta;
    *n_theta = s.n_theta;
    if (!map && cap_cells == 0) return IVX_OK;  // (the size alone)
    IVX_REQUIRE(map, IVX_ERR_INVALID, "%s: null argument", who);
    IVX_REQUIRE(cap_cells >= cells, IVX_ERR_CAPACITY, "%s: room for %zu cells, the map of slot %u has %zu", who, cap_cells, slot, cells);
    IVX_HIP_CHECK(ivx_memcpy_async(map, s.buf.p, cells * sizeof(ivx_drag_load), hipMemcpyDeviceToHost, w->ctx->stream));
    IVX_HIP_CHECK(ivx_stream_sync(w->ctx->stream));
    return IVX_OK;
}

int ivx_world_set_detailed_drag(ivx_world* w, const ivx_drag_generator* gens, size_t n) {
    const char* who = "ivx_world_set_detailed_drag";
    IVX_REQUIRE(w && (gens || n == 0), IVX_ERR_INVALID, "%s: null argument", who);
    IVX_REQUIRE(n < (1u << 24), IVX_ERR_CAPACITY, "%s: more than 2^24 generators", who);
    if (n == 0 && !w->fg_state) return IVX_OK;
    const FgMedia* m = static_cast<const FgMedia*>(w->fg_media);
    if (int rc = fg_validate_drag(who, gens, n, w->n_dyn, m ? m->slots.size() : 0, [m](uint32_t slot) { return m->slots[slot].n_theta != 0; })) return rc;
    FgState* st;
    if (int rc = fg_state_for(w, who, &st)) return rc;
    st->drag.assign(gens, gens + n);
    return fg_sets_changed(w, st);
}

int ivx_fg_apply_host_drag(const ivx_force_generator* gens, size_t n, const uint32_t* gravity_bodies, size_t n_gravity, float gravitational_constant, ivx_rigid_body* dynamic,
                           size_t n_dynamic, const ivx_kinematic_body* kinematic, size_t n_kinematic, float* gravity_loads6, const ivx_drag_generator* drag, size_t n_drag,
                           const ivx_drag_map_view* maps, size_t n_maps, const ivx_uniform_medium* medium) {
    const char* who = "ivx_fg_apply_host_drag";
    IVX_REQUIRE((gens || n == 0) && (gravity_bodies || n_gravity == 0) && (dynamic || n_dynamic == 0) && (kinematic || n_kinematic == 0) && (drag || n_drag == 0) &&
                    (maps || n_maps == 0) && (medium || n_drag == 0),
                IVX_ERR_INVALID, "%s: null argument", who);
    if (int rc = fg_validate(who, gens, n, n_dynamic, n_kinematic)) return rc;
    if (int rc = fg_validate_field(who, gravity_bodies, n_gravity, n_dynamic)) return rc;
    for (size_t s = 0; s < n_maps; ++s)
        IVX_REQUIRE(maps[s].n_theta <= ivx_drag::MAX_THETA, IVX_ERR_CAPACITY, "%s: map slot %zu: n_theta_coords %u exceeds %u", who, s, maps[s].n_theta, ivx_drag::MAX_THETA);
    if (int rc = fg_validate_drag(who, drag, n_drag, n_dynamic, n_maps, [maps](uint32_t slot) { return maps[slot].loads && maps[slot].n_theta != 0; })) return rc;
    fg_apply_host(gens, n, gravity_bodies, n_gravity, gravitational_constant, dynamic, n_dynamic, kinematic, gravity_loads6, drag, n_drag, maps, medium);
    return IVX_OK;
}

}  // extern "C"
