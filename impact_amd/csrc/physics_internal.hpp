// Device-side layouts and the host-side world object of the rigid-body / contact-solver part
// (a15-a19). See physics.hip for the kernels, contact_schedule.hpp for the host bookkeeping of the contact set, solve_plan.hpp for what a
// solve launches and physics_api.hip for the entry points that tie them together.
#pragma once
#include <cstdint>
#include <vector>

#include "contact_schedule.hpp"
#include "device_common.hpp"
#include "solve_plan.hpp"
#include "vec3.hpp"

// Arithmetic the step's advance of configurations (physics.hip, post_solve_body) and the constant-rotation motion driver (motion.hip) share,
// host and device: one text, so the two cannot drift apart.
namespace ivx_phys {
using ivx_vec::Q4;
using ivx_vec::V3;
#define IVX_PHYS_HD __host__ __device__ __forceinline__
// f32::sin / f32::cos of the reference are libm's sinf / cosf, which are the correctly rounded values in all but rare cases; the device
// library's single-precision versions are one ulp off now and then (found by a random contact graph whose 1-ulp orientation grew past the
// 1e-5 bar in two frames). The double-precision functions rounded once agree with libm on every value the tests have met; it is two calls
// per body and step.
IVX_PHYS_HD float sin_rn(float x) { return (float)sin((double)x); }
IVX_PHYS_HD float cos_rn(float x) { return (float)cos((double)x); }
IVX_PHYS_HD float tan_rn(float x) { return (float)tan((double)x); }
// f32::acos of the alignment torque (forces.hip), for the same reason: the argument is clamped to [-1, 1] by the caller
IVX_PHYS_HD float acos_rn(float x) { return (float)acos((double)x); }
// f32::atan2 of the drag phase (forces.hip: the azimuth of a body's motion through the medium), for the same reason
IVX_PHYS_HD float atan2_rn(float y, float x) { return (float)atan2((double)y, (double)x); }
IVX_PHYS_HD Q4 qnormalize(Q4 q) {
    const float l = sqrtf(((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w);
    return {q.x / l, q.y / l, q.z / l, q.w / l};
}
// advance_orientation (rigid_body.rs:1020-1034): the rotation by angular speed x duration about the unit axis, applied on the left, re-normalised
IVX_PHYS_HD Q4 advance_orientation(Q4 q, V3 axis, float speed, float duration) {
    const float angle = speed * duration;
    const float s = sin_rn(0.5f * angle), co = cos_rn(0.5f * angle);
    const V3 im = ivx_vec::operator*(axis, s);
    return qnormalize(ivx_vec::qmul(Q4{im.x, im.y, im.z, co}, q));
}
#undef IVX_PHYS_HD
}  // namespace ivx_phys

// ConstrainedBody (impact_physics/src/constraint.rs:137-150), 96 bytes. Dynamic bodies first (same index as
// in the rigid-body array), kinematic bodies after them.
struct PhysBody {
    float inv_mass;
    float inv_inertia[9];  // world space, column-major
    float pos[3];
    float q[4];
    float v[3];
    float w[3];
    float pad;
};
static_assert(sizeof(PhysBody) == 96, "PhysBody layout");

// PreparedContact (constraint/contact.rs:63-86) + the constrained-body indices of its pair, 96 bytes
struct PhysContact {
    float local_a[3], local_b[3], normal[3], tangent[3], bitangent[3];
    float m_n, m_t, m_b, friction, target;
    float world_b[3];  // the contact point on body B in world space as the velocity phase sees it: qrot(q_b, local_b) + pos_b, fixed for the step
    uint32_t pad;
};
static_assert(sizeof(PhysContact) == 96, "PhysContact layout");

#define PHYS_LEVEL_TILE 4096

// What the world holds on the device. Every array that only grows is an ivx_dev_array; physics_api.hip keeps ONE table of them (world_arrays:
// which group an array belongs to, the host vector it is uploaded from) that the growth, the uploads and ivx_world_destroy walk.
struct ivx_world {
    ivx_ctx* ctx;
    ivx_solver_config cfg;
    uint32_t n_dyn, n_kin;
    // the body group: one capacity in bodies (floor 64) for the five of them (ivx_world_set_bodies)
    size_t body_cap;
    ivx_dev_array<ivx_rigid_body> dyn;
    ivx_dev_array<ivx_kinematic_body> kin;
    ivx_dev_array<PhysBody> cb;
    ivx_dev_array<uint8_t> touched;
    ivx_dev_array<float> dynst;  // the solve on several workgroups (k_solve_mg, k_solve_cs): the phase's mutable body state as shared records, 64 bytes a
                                 // body (the velocity phase uses 32) and, body_cap * 64 bytes in, as many for the positional phase (48)
    // the contact group: the contacts of the current step in ConstraintCache order (= solve order), the slot each had before, and the prepared
    // contacts and accumulated impulses (float4 per contact) of this and the previous prepare (contact_arrays_grow_keep)
    uint32_t n_contacts, n_prev;
    ivx_dev_array<ivx_contact> contacts;
    ivx_dev_array<int32_t> prev_slot;
    ivx_dev_array<PhysContact> pc[2];
    ivx_dev_array<float> acc[2];
    int cur;
    // the host-side state of the contact set: ConstraintCache, chains, levels, both schedule forms and their per-phase figures
    ivx_contact_schedule sched;
    // form 1 of the schedule (sched.build_form(1)): items, their body pairs (uint2) and tags (uint4), level extents, tiles
    ivx_dev_array<uint32_t> items, item_bodies, item_tags, level_start, tile_base, tile_first;
    // packed per-item records of the multi-workgroup solve (physics.hip, k_pack_items), sized in bytes by pack_items_mg
    float* packed[2];
    size_t packed_cap[2];
    // form 2 (sched.build_form(2)): the chain-stationary slots, rounds and, with kinematic bodies in the positional phase, cs_slot_of
    ivx_dev_array<uint32_t> cs_item, cs_bodies, cs_vers, cs_round_start, cs_round_level, cs_slot_of;
    ivx_dev_array<uint64_t> cs_round_mask;
    uint32_t solver_kind_used;  // 0: one workgroup, 1: tile dataflow on several (k_solve_mg), 2: chain-stationary (k_solve_cs)
    // kinematic orientations in the positional phase (physics.hip, ReplayView): sched.kin_offsets_host / kin_list_host, per-item counts and
    // tables of the two passes (kin_qstart: float4 per (item, side), the orientation a kinematic body has when the chain starts in pass 2)
    ivx_dev_array<uint32_t> kin_offsets, kin_list, kin_applied;
    ivx_dev_array<float> kin_qstart, kin_snap;
    // SphericalJoint constraints (constraint/spherical_joint.rs): the reference's joint computes no impulse and no correction (:62-88);
    // all it does is register its two bodies as constrained bodies, which get their velocities written back after the solve
    uint32_t* joint_refs;  // device: body references (IVX_KINEMATIC_BODY flag) of all joints' anchors, allocated to size
    uint32_t n_joint_refs;
    std::vector<uint32_t> joint_refs_host;  // the same references on the host (the step's body count, sched.constrained_bodies)
    // the grid barrier of the solve on several workgroups: the monotonic arrival counters + an error word (a bounded poll gave up)
    uint32_t* barrier_words;
    uint32_t* mg_err_host;  // host-mapped word the multi-workgroup solve sets when its grid barrier gave up (checked at every wait on the stream)
    uint32_t* mg_err_dev;   // its device-side address
    int mg_disabled;        // a barrier timed out in this world before: the solve stays on the single-workgroup kernel
    uint32_t barrier_count;   // arrivals counted so far on the velocity phase's grid-barrier counter (barrier_words[0])
    uint32_t barrier_count1;  // ... on the positional phase's (barrier_words[1]): the two phases run side by side, each on its own counter
    hipStream_t side_stream;  // the positional phase's stream (ivx_launch_phys_solve); created on first use
    hipEvent_t ev_fork, ev_join;
    uint32_t solver_groups_forced, solver_groups_used;
    int schedule_valid, prepared_fresh;
    hipEvent_t ev[5];
    int ev_ready;
    // the resident contacts in slot order on the host: the pinned block their upload is made from (asynchronous; the block's event follows it)
    ivx_staging stage_contacts;
    // the general path's other uploads (warm-start sources, a new schedule): one pinned block, asynchronous copies behind its event — the
    // path used to make seventeen blocking copies and two waits per frame whose contact set had changed
    ivx_staging stage_sched;
    float time;      // the simulation clock (ivx_world_set_time / ivx_world_time): every step adds its dt; host-side only
    void* md_state;  // motion drivers (motion.hip): the sorted driver set, the compact list of driven bodies and their offsets; made by ivx_world_set_motion_drivers, freed by ivx_md_release
    void* fg_state;  // force generators, dynamic gravity and detailed drag (forces.hip): the three sets, their plan over the dynamic bodies, the resident gravity loads; null while none of the sets is installed; freed by ivx_fg_release
    void* fg_media;  // the uniform medium and the resident drag load maps (forces.hip): they belong to the world and outlive the sets; made on first use, freed by ivx_fg_release
    void* cw_state;  // primitive collidables (narrow.hip): local and world-space records, wave masks and offsets, contact and deferred buffers; made on first use, freed by ivx_cw_release
};

void ivx_cw_release(ivx_world* w);  // narrow.hip (ivx_world_destroy)
void ivx_md_release(ivx_world* w);  // motion.hip (ivx_world_destroy)
int ivx_motion_ready(ivx_world* w, const char* who);  // motion.hip: IVX_ERR_STATE when the driver set refers to more kinematic bodies than the world holds (checked before a step launches anything)
int ivx_launch_motion_apply(ivx_world* w, float time, const char* who);  // motion.hip: nothing without a driver set
void ivx_fg_release(ivx_world* w);  // forces.hip (ivx_world_destroy): the sets, the medium and the maps
int ivx_forces_ready(ivx_world* w, const char* who);  // forces.hip: IVX_ERR_STATE when the sets refer to more bodies than the world holds (checked before a step launches anything)
int ivx_launch_forces_apply(ivx_world* w, const char* who);  // forces.hip: nothing while none of the sets is installed
int ivx_launch_phys_prepare_bodies(ivx_world* w);
int ivx_launch_phys_prepare_contacts(ivx_world* w, const int32_t* d_prev_slot);
int ivx_launch_phys_mark_joint_bodies(ivx_world* w);
int ivx_launch_phys_pre_solve(ivx_world* w, float dt);
int ivx_launch_phys_solve(ivx_world* w);
int ivx_launch_phys_free_step(ivx_world* w, float dt);
int ivx_world_ensure_form(ivx_world* w, uint32_t form);  // physics_api.hip
int ivx_launch_phys_post_solve(ivx_world* w, float dt, int write_back, int advance);
