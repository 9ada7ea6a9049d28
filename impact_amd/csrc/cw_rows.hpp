// The join between the collision world and the voxel contact generators, host and device in ONE text: a voxel body's transform_to_object_space and
// the dispatch of one deferred pair (include/impact_voxel_hip.h states both forms). k_cw_rows (narrow.hip) and the two host exports run these
// functions and nothing else; the files that use them are compiled without contraction. Below them, what narrow.hip (the pair pass, the rows, the
// world's buffers) and voxel_collision_api.hip (the generators over the rows) hand each other inside ivx_cw_collide_frame.
#pragma once
#include "ivx_internal.hpp"
#include "vec3.hpp"

typedef struct ivx_cw_voxel_row ivx_cw_row;  // (the C ABI gives the name to the host export of voxel_row below)

namespace ivx_cw_rows {
using namespace ivx_vec;

#define IVX_CWR_HD __host__ __device__ __forceinline__

// VoxelObjectCollidable::new (impact_voxel/src/collidable.rs:310-327; isometry.rs:112-134): pose = position[3], orientation_xyzw[4]
IVX_CWR_HD void to_object_space(const float* pose, const float* origin_offset, float rotation[4], float translation[3]) {
    const float* q = pose + 3;
    const V3 t_w = qrot(q, -ld3(origin_offset)) + ld3(pose);
    rotation[0] = -q[0], rotation[1] = -q[1], rotation[2] = -q[2], rotation[3] = q[3];
    st3(translation, -qrot(rotation, t_w));
}

// ContactResponseParameters::combined (impact_physics/src/material.rs:43-51), the arguments in the dispatch's order
IVX_CWR_HD void combined(const float* r1, const float* r2, float out[3]) {
    out[0] = max_rs(r1[0], r2[0]);
    out[1] = sqrtf(r1[1] * r2[1]);
    out[2] = sqrtf(r1[2] * r2[2]);
}

// what a voxel member brings besides its world-space record: the pose of its body and the attached offsets (null for the other shapes)
struct Member {
    const ivx_collidable* c;
    const float* pose;            // position[3], orientation_xyzw[4]
    const float* origin_offset;   // [3]
    const float* center_of_mass;  // [3]
    uint32_t index;
};

// generate_contact_manifold (collidable.rs:138-215) for one deferred pair (a, b): at least one member is a voxel object
IVX_CWR_HD void voxel_row(const Member& a, const Member& b, ivx_cw_row* out) {
    ivx_cw_row r = {};
    const bool va = a.c->shape == IVX_CW_VOXEL_OBJECT, vb = b.c->shape == IVX_CW_VOXEL_OBJECT;
    if (va && vb) {  // Original: A is a
        r.generator = IVX_CW_ROW_MUTUAL;
        r.voxel = a.index, r.other = b.index;
        r.collidable_id_a = a.c->id, r.collidable_id_b = b.c->id;
        r.body_a = a.c->body, r.body_b = b.c->body;
        combined(a.c->response, b.c->response, r.response);
        to_object_space(a.pose, a.origin_offset, r.rotation_a, r.translation_a);
        to_object_space(b.pose, b.origin_offset, r.rotation_b, r.translation_b);
        for (int k = 0; k < 3; ++k) r.center_of_mass_a[k] = a.center_of_mass[k], r.center_of_mass_b[k] = b.center_of_mass[k];
    } else {
        const Member& v = va ? a : b;  // the voxel object and the other member
        const Member& c = va ? b : a;
        r.voxel = v.index, r.other = c.index;
        to_object_space(v.pose, v.origin_offset, r.rotation_a, r.translation_a);
        r.shape1 = c.c->s;
        for (int k = 0; k < 3; ++k) r.shape3[k] = c.c->a[k];
        r.collidable_id_a = c.c->id, r.collidable_id_b = v.c->id;
        if (c.c->shape == IVX_CW_PLANE) {  // the voxel object is A; the id hash takes the plane first
            r.generator = 1u;
            r.body_a = v.c->body, r.body_b = c.c->body;
            combined(v.c->response, c.c->response, r.response);
        } else {  // the sphere or capsule is A and its id comes first
            const bool capsule = c.c->shape == IVX_CW_CAPSULE;
            r.generator = capsule ? 2u : 0u;
            for (int k = 0; k < 3; ++k) r.shape3b[k] = capsule ? c.c->b[k] : 0.0f;
            r.body_a = c.c->body, r.body_b = v.c->body;
            combined(c.c->response, v.c->response, r.response);
        }
    }
    *out = r;
}

#undef IVX_CWR_HD
}  // namespace ivx_cw_rows

// ---- inside ivx_cw_collide_frame ------------------------------------------------------------------------------------------------------------------
#pragma GCC visibility push(hidden)
struct ivx_world;
// What narrow.hip holds after the call's second wait. `rows` lies in the world's pinned block and stays until the next call on this world.
struct ivx_cw_frame_pass {
    size_t n_primitive = 0, n_deferred = 0;
    const ivx_cw_row* rows = nullptr;        // n_deferred of them
    const ivx_contact* contacts = nullptr;         // the primitive contacts and the deferred pairs: as many as the caller's capacities let through
    const uint32_t* deferred = nullptr;
    const ivx_cw_voxel_object* objects = nullptr;  // by collidable index (n_collidables); grid null: nothing attached
    size_t n_collidables = 0;
};
// the pair pass, the primitive narrow phase and the rows of ivx_cw_collide_frame: two waits (narrow.hip). contacts_cap, deferred_cap: how many
// primitive contacts and deferred pairs to bring with the counts
int ivx_cw_frame_pairs(ivx_world* w, const char* who, uint32_t mode, size_t contacts_cap, size_t deferred_cap, ivx_cw_frame_pass* out);
// the world's contact buffer holds `total` contacts afterwards and still starts with the n_primitive that k_cw_emit wrote -> its address
int ivx_cw_frame_reserve(ivx_world* w, size_t n_primitive, size_t total, ivx_contact** list);
// behind the emit passes: the merged list comes to `out` (null: it stays on the device); the call's last wait
int ivx_cw_frame_finish(ivx_world* w, size_t total, ivx_contact* out);
#pragma GCC visibility pop
