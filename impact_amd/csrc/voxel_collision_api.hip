// Voxel collision host code of libimpact_voxel_hip.so: contacts of a voxel object with a sphere, plane or capsule collidable, the collision probes
// that follow an object's mesh, mutual contacts of two voxel objects; single calls and the `_many` forms; the host side of
// ivx_cw_collide_frame, which runs both `_many` generator families over the rows narrow.hip made of a frame's deferred pairs; and the overlap
// geometry of two objects (host_intersection_ranges), which their mutual absorption (edit_api.hip) asks for as well.
// Host-side orchestration only: the kernels are those of contacts.hip and collide.hip behind their ivx_launch_* functions.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <limits>
#include <new>
#include <vector>

#include "cw_rows.hpp"
#include "ivx_host.hpp"
#include "physics_internal.hpp"
#include "vec3.hpp"
#include "voxel_ranges.hpp"

namespace {
using namespace ivx_vec;  // V3, Q4, ld3, st3, qrot, qmul, splitmix

// the host geometry keeps its points as float[3] / float[4] (they come from and go to the C ABI's arrays): around ivx_vec's forms
void qrot3(const float q[4], const float v[3], float out[3]) { st3(out, qrot(q, ld3(v))); }
void qmul4(const float a[4], const float b[4], float o[4]) {
    const Q4 r = qmul(Q4{a[0], a[1], a[2], a[3]}, Q4{b[0], b[1], b[2], b[3]});
    o[0] = r.x, o[1] = r.y, o[2] = r.z, o[3] = r.w;
}

// the chunk box and voxel ranges a collidable touches of an object (mode 0 sphere: centre shape3, radius shape1; 1 plane: unit normal shape3,
// displacement shape1; 2 capsule: segment start shape3, segment vector shape3b, radius shape1); false: nothing touched
bool contacts_box(const ivx_grid* g, int mode, const float rotation_xyzw[4], const float translation[3], const float shape3[3], const float shape3b[3],
                  float shape1, const uint32_t occ[12], int32_t vlo[3], int32_t vhi[3], uint32_t lo[3], uint32_t cc[3]) {
    const int plane = mode == 1;
    const float inv = 1.0f / g->extent;
    float lo_f[3], hi_f[3];
    if (mode == 2) {
        // capsule.iso_transformed(transform_to_object_space).scaled(inverse_voxel_extent).compute_aabb() (impact_geometry/src/capsule.rs:100-137;
        // intersection.rs:73-82)
        float ra[3], rv[3];
        qrot3(rotation_xyzw, shape3, ra);
        qrot3(rotation_xyzw, shape3b, rv);
        const float rn = inv * shape1;
        for (int d = 0; d < 3; ++d) {
            const float an = (ra[d] + translation[d]) * inv, vn = rv[d] * inv;
            const float en = an + vn;
            const float la = an - rn, le = en - rn, ha = an + rn, he = en + rn;
            lo_f[d] = le < la ? le : la;
            hi_f[d] = he > ha ? he : ha;
        }
    } else if (!plane) {
        // sphere.iso_transformed(transform_to_object_space).scaled(inverse_voxel_extent) and its box (intersection.rs:51-60)
        float rc3[3];
        qrot3(rotation_xyzw, shape3, rc3);
        const float rn = inv * shape1;
        for (int d = 0; d < 3; ++d) {
            const float cn = (rc3[d] + translation[d]) * inv;
            lo_f[d] = cn - rn;
            hi_f[d] = cn + rn;
        }
    } else {
        // plane.iso_transformed(..).scaled(..) (impact_geometry/src/plane.rs:170-203), then the occupied box projected onto its negative
        // halfspace (voxel_ranges_within_plane, intersection.rs:751-761; axis_aligned_box.rs:460-488)
        const float point[3] = {shape3[0] * shape1, shape3[1] * shape1, shape3[2] * shape1};
        float tp[3], tn[3];
        qrot3(rotation_xyzw, point, tp);
        for (int d = 0; d < 3; ++d) tp[d] += translation[d];
        qrot3(rotation_xyzw, shape3, tn);
        const float disp = ((tn[0] * tp[0] + tn[1] * tp[1]) + tn[2] * tp[2]) * inv;
        float blo[3], bhi[3];
        for (int d = 0; d < 3; ++d) {
            blo[d] = lo_f[d] = (float)occ[6 + 2 * d];
            bhi[d] = hi_f[d] = (float)occ[7 + 2 * d];
        }
        const int perm[3][3] = {{0, 1, 2}, {1, 2, 0}, {2, 0, 1}};
        auto mn2 = [](float x, float y) { return (y < x) ? y : x; };
        auto mx2 = [](float x, float y) { return (y > x) ? y : x; };
        for (int r = 0; r < 3; ++r) {
            const int i = perm[r][0], j = perm[r][1], k = perm[r][2];
            if (std::fabs(tn[k]) > 1e-8f) {
                const float a0 = tn[i] * blo[i] + tn[j] * blo[j], b0 = tn[i] * blo[i] + tn[j] * bhi[j], c0 = tn[i] * bhi[i] + tn[j] * blo[j],
                            d0 = tn[i] * bhi[i] + tn[j] * bhi[j];
                const float extremal = (disp - mn2(mn2(mn2(a0, b0), c0), d0)) / tn[k];
                if (!std::signbit(tn[k])) {
                    lo_f[k] = mn2(lo_f[k], extremal);
                    hi_f[k] = mn2(hi_f[k], extremal);
                } else {
                    lo_f[k] = mx2(lo_f[k], extremal);
                    hi_f[k] = mx2(hi_f[k], extremal);
                }
            }
        }
    }
    long rlo[3], rhi[3];
    clamped_ranges(occ, lo_f, hi_f, false, rlo, rhi);
    return chunk_box(rlo, rhi, vlo, vhi, lo, cc);
}

struct HBox {
    float lo[3], hi[3];
};
// AxisAlignedBox::find_contained_subsegment (impact_geometry/src/axis_aligned_box.rs:385-415)
bool host_subsegment(const HBox& b, const float s[3], const float v[3], float* t0, float* t1) {
    float a = 0.0f, z = 1.0f;
    for (int d = 0; d < 3; ++d) {
        if (std::fabs(v[d]) > 1e-8f) {
            const float r = 1.0f / v[d];
            const float u1 = (b.lo[d] - s[d]) * r, u2 = (b.hi[d] - s[d]) * r;
            const float en = u1 < u2 ? u1 : u2, ex = u1 < u2 ? u2 : u1;
            a = en > a ? en : a;
            z = ex < z ? ex : z;
        } else if (s[d] < b.lo[d] || s[d] > b.hi[d]) {
            return false;
        }
    }
    *t0 = a;
    *t1 = z;
    return a <= z;
}
// compute_box_intersection_bounds (impact_geometry/src/oriented_box.rs:315-431): box A axis-aligned, box B = (centre, orientation, half
// extents) in A's frame; bounds of the overlap in A's frame and in B's own frame (relative to its centre)
bool host_box_bounds(const HBox& a, const float bc[3], const float bq[4], const float bh[3], HBox* in_a, HBox* in_b) {
    static const int E[12][2] = {{0, 1}, {2, 3}, {4, 5}, {6, 7}, {0, 2}, {1, 3}, {4, 6}, {5, 7}, {0, 4}, {1, 5}, {2, 6}, {3, 7}};
    const float inf = std::numeric_limits<float>::infinity();
    for (int d = 0; d < 3; ++d) in_a->lo[d] = in_b->lo[d] = inf, in_a->hi[d] = in_b->hi[d] = -inf;
    bool any = false;
    auto grow = [&](const float pa[3], const float pb[3]) {
        for (int d = 0; d < 3; ++d) {
            in_a->lo[d] = pa[d] < in_a->lo[d] ? pa[d] : in_a->lo[d];
            in_a->hi[d] = pa[d] > in_a->hi[d] ? pa[d] : in_a->hi[d];
            in_b->lo[d] = pb[d] < in_b->lo[d] ? pb[d] : in_b->lo[d];
            in_b->hi[d] = pb[d] > in_b->hi[d] ? pb[d] : in_b->hi[d];
        }
        any = true;
    };
    const float bqi[4] = {-bq[0], -bq[1], -bq[2], bq[3]};
    auto to_b = [&](const float p[3], float o[3]) {  // OrientedBox::transform_point_to_box_frame
        const float r[3] = {p[0] - bc[0], p[1] - bc[1], p[2] - bc[2]};
        qrot3(bqi, r, o);
    };
    auto from_b = [&](const float p[3], float o[3]) {
        qrot3(bq, p, o);
        for (int d = 0; d < 3; ++d) o[d] = bc[d] + o[d];
    };
    // corners of B: centre -/+ half width -/+ half height -/+ half depth along the columns of Mat3A::from_quat
    float ax[3][3];
    {
        const float x = bq[0], y = bq[1], z = bq[2], w = bq[3];
        const float x2 = x + x, y2 = y + y, z2 = z + z, xx = x * x2, xy = x * y2, xz = x * z2, yy = y * y2, yz = y * z2, zz = z * z2, wx = w * x2, wy = w * y2,
                    wz = w * z2;
        ax[0][0] = 1.0f - (yy + zz), ax[0][1] = xy + wz, ax[0][2] = xz - wy;
        ax[1][0] = xy - wz, ax[1][1] = 1.0f - (xx + zz), ax[1][2] = yz + wx;
        ax[2][0] = xz + wy, ax[2][1] = yz - wx, ax[2][2] = 1.0f - (xx + yy);
    }
    float corner[8][3];
    for (int c = 0; c < 8; ++c)
        for (int d = 0; d < 3; ++d) {
            const float hw = bh[0] * ax[0][d], hh = bh[1] * ax[1][d], hd = bh[2] * ax[2][d];
            float v = (c & 4) ? bc[d] + hw : bc[d] - hw;
            v = (c & 2) ? v + hh : v - hh;
            corner[c][d] = (c & 1) ? v + hd : v - hd;
        }
    for (const auto& e : E) {
        const float* s = corner[e[0]];
        const float v[3] = {corner[e[1]][0] - s[0], corner[e[1]][1] - s[1], corner[e[1]][2] - s[2]};
        float t0, t1;
        if (!host_subsegment(a, s, v, &t0, &t1)) continue;
        const float p0[3] = {s[0] + v[0] * t0, s[1] + v[1] * t0, s[2] + v[2] * t0}, p1[3] = {s[0] + v[0] * t1, s[1] + v[1] * t1, s[2] + v[2] * t1};
        float q0[3], q1[3];
        to_b(p0, q0);
        to_b(p1, q1);
        grow(p0, q0);
        grow(p1, q1);
    }
    float acorner[8][3];
    for (int c = 0; c < 8; ++c) {
        const float p[3] = {(c & 4) ? a.hi[0] : a.lo[0], (c & 2) ? a.hi[1] : a.lo[1], (c & 1) ? a.hi[2] : a.lo[2]};
        to_b(p, acorner[c]);
    }
    HBox self;
    for (int d = 0; d < 3; ++d) self.lo[d] = -bh[d], self.hi[d] = bh[d];
    for (const auto& e : E) {
        const float* s = acorner[e[0]];
        const float v[3] = {acorner[e[1]][0] - s[0], acorner[e[1]][1] - s[1], acorner[e[1]][2] - s[2]};
        float t0, t1;
        if (!host_subsegment(self, s, v, &t0, &t1)) continue;
        const float q0[3] = {s[0] + v[0] * t0, s[1] + v[1] * t0, s[2] + v[2] * t0}, q1[3] = {s[0] + v[0] * t1, s[1] + v[1] * t1, s[2] + v[2] * t1};
        float p0[3], p1[3];
        from_b(q0, p0);
        from_b(q1, p1);
        grow(p0, q0);
        grow(p1, q1);
    }
    return any;
}

}  // namespace

// determine_voxel_ranges_encompassing_intersection (object/intersection.rs:706-746) from the two objects' occupied ranges and world -> object
// transforms; also transform_from_b_to_a = world_to_a * world_to_b.inverted() (impact_math/src/transform/isometry.rs:128-134, 200-205).
// The ranges are not checked for emptiness (the reference does not either). false: the occupied boxes do not meet.
bool host_intersection_ranges(const ivx_grid* a, const uint32_t occ_a[12], const float rotation_a[4], const float translation_a[3], const ivx_grid* b,
                                     const uint32_t occ_b[12], const float rotation_b[4], const float translation_b[3], long ra_lo[3], long ra_hi[3],
                                     long rb_lo[3], long rb_hi[3], float q_ba[4], float t_ba[3]) {
    const float qbi[4] = {-rotation_b[0], -rotation_b[1], -rotation_b[2], rotation_b[3]};
    float tbi[3];
    qrot3(qbi, translation_b, tbi);
    for (int d = 0; d < 3; ++d) tbi[d] = -tbi[d];
    qmul4(rotation_a, qbi, q_ba);
    qrot3(rotation_a, tbi, t_ba);
    for (int d = 0; d < 3; ++d) t_ba[d] += translation_a[d];
    HBox box_a, box_b;
    for (int d = 0; d < 3; ++d) {
        box_a.lo[d] = a->extent * (float)occ_a[6 + 2 * d];
        box_a.hi[d] = a->extent * (float)occ_a[7 + 2 * d];
        box_b.lo[d] = b->extent * (float)occ_b[6 + 2 * d];
        box_b.hi[d] = b->extent * (float)occ_b[7 + 2 * d];
    }
    float b_center[3], b_half[3], bc_in_a[3], bq_in_a[4];
    for (int d = 0; d < 3; ++d) {
        b_center[d] = 0.5f * (box_b.lo[d] + box_b.hi[d]);
        b_half[d] = 0.5f * (box_b.hi[d] - box_b.lo[d]);
    }
    qrot3(q_ba, b_center, bc_in_a);
    for (int d = 0; d < 3; ++d) bc_in_a[d] += t_ba[d];
    const float ident[4] = {0.0f, 0.0f, 0.0f, 1.0f};
    qmul4(q_ba, ident, bq_in_a);
    HBox in_a, in_b;
    if (!host_box_bounds(box_a, bc_in_a, bq_in_a, b_half, &in_a, &in_b)) return false;
    const float inv_a = 1.0f / a->extent, inv_b = 1.0f / b->extent;
    float na_lo[3], na_hi[3], nb_lo[3], nb_hi[3];
    for (int d = 0; d < 3; ++d) {
        na_lo[d] = inv_a * in_a.lo[d];
        na_hi[d] = inv_a * in_a.hi[d];
        nb_lo[d] = inv_b * (in_b.lo[d] + b_center[d]);
        nb_hi[d] = inv_b * (in_b.hi[d] + b_center[d]);
    }
    clamped_ranges(occ_a, na_lo, na_hi, true, ra_lo, ra_hi);
    clamped_ranges(occ_b, nb_lo, nb_hi, true, rb_lo, rb_hi);
    return true;
}

namespace {
// the end of the single calls: the total, then that many contacts, each a copy and a wait
int contacts_download(ivx_grid* g, const char* who, const uint32_t* d_total, const ivx_contact* d_out, ivx_contact* out, size_t cap, size_t* n_out) {
    uint32_t total = 0;
    int rc;
    if ((rc = d2h(g, &total, d_total, sizeof(total)))) return rc;
    *n_out = total;
    IVX_REQUIRE(total <= cap, IVX_ERR_CAPACITY, "%s: %u contacts exceed the capacity %zu", who, total, cap);
    return total ? d2h(g, out, d_out, (size_t)total * sizeof(ivx_contact)) : IVX_OK;
}

// the context's pinned, device-visible scratch (ivx_ctx::pinned_scratch): at least `bytes`
int ctx_pinned_scratch(ivx_ctx* c, size_t bytes) { return ivx_mapped_grow(&c->pinned_scratch, bytes, std::max<size_t>(2 * bytes, 1 << 20), c->stream); }

// The batched contact calls (the two `_many` generators, and ivx_cw_collide_frame over both families at once) in pieces. Once the count phase is
// on the stream and has written every query's total into the pinned block: wait, the totals into out_offsets (n + 1) and aside into `counts`
// (the pinned block may move afterwards) -> *run, the contacts of all queries |
// `emit(i, list, count)` for every query that found any, under the recorder (many_phase; `chain`: the object that stands for query i), its
// contacts going to list[0 .. count) = `list` + out_offsets[i]: the destination is the caller's (the pinned block, or the world's contact buffer).
int contacts_many_wait_totals(ivx_ctx* c, size_t n, uint32_t* out_offsets, std::vector<uint32_t>& counts, size_t* run_out) {
    IVX_HIP_CHECK(ivx_stream_sync(c->stream));
    const uint32_t* totals = static_cast<const uint32_t*>(c->pinned_scratch.p);
    size_t run = 0;
    for (size_t i = 0; i < n; ++i) {
        out_offsets[i] = (uint32_t)run;
        run += totals[i];
    }
    out_offsets[n] = (uint32_t)run;
    counts.assign(totals, totals + n);
    *run_out = run;
    return IVX_OK;
}
int contacts_many_emit(ivx_grid* const* chain, size_t n, const std::vector<uint32_t>& counts, const uint32_t* out_offsets, ivx_contact* list,
                       const std::function<int(size_t, ivx_contact*, uint32_t)>& emit) {
    return many_phase(chain, n, [&](size_t i) -> int { return counts[i] ? emit(i, list + out_offsets[i], counts[i]) : IVX_OK; });
}
// The second half of the two `_many` calls: the totals; the capacity check; the pinned block grown for all contacts; the emit passes into it;
// wait; copy out.
int contacts_many_finish(ivx_ctx* c, ivx_grid* const* chain, size_t n, const char* who, ivx_contact* out, size_t cap, uint32_t* out_offsets,
                         const std::function<int(size_t, ivx_contact*, uint32_t)>& emit) {
    static thread_local std::vector<uint32_t> counts;
    size_t run = 0;
    int rc;
    if ((rc = contacts_many_wait_totals(c, n, out_offsets, counts, &run))) return rc;
    IVX_REQUIRE(run <= cap, IVX_ERR_CAPACITY, "%s: %zu contacts exceed the capacity %zu", who, run, cap);
    if (run == 0) return IVX_OK;
    if ((rc = ctx_pinned_scratch(c, run * sizeof(ivx_contact)))) return rc;
    if ((rc = contacts_many_emit(chain, n, counts, out_offsets, static_cast<ivx_contact*>(c->pinned_scratch.dev), emit))) return rc;
    IVX_HIP_CHECK(ivx_stream_sync(c->stream));
    memcpy(out, c->pinned_scratch.p, run * sizeof(ivx_contact));
    return IVX_OK;
}
// the start of both: the pinned block holds a zeroed total per query; *totals_dev: the device's address of them
int contacts_many_totals(ivx_ctx* c, size_t n, uint32_t** totals_dev) {
    const int rc = ctx_pinned_scratch(c, ((n * 4 + 63) & ~(size_t)63) + 4096);
    if (rc) return rc;
    memset(c->pinned_scratch.p, 0, n * 4);
    *totals_dev = static_cast<uint32_t*>(c->pinned_scratch.dev);
    return IVX_OK;
}
}  // namespace

static int voxel_object_contacts(ivx_grid* g, const char* who, int mode, const float rotation_xyzw[4], const float translation[3], const float shape3[3],
                                 const float shape3b[3], float shape1, uint64_t id_a, uint64_t id_b, uint32_t body_a, uint32_t body_b, const float response[3], ivx_contact* out,
                                 size_t cap, size_t* n_out) {
    IVX_REQUIRE(g && rotation_xyzw && translation && shape3 && (shape3b || mode != 2) && response && n_out && (out || cap == 0), IVX_ERR_INVALID,
                "%s: null argument", who);
    int rc;
    if ((rc = require_whole_object(g, who, false))) return rc;
    *n_out = 0;
    uint32_t occ[12];
    if ((rc = ivx_reference_occupied(g, who, occ))) return rc;
    int32_t vlo[3], vhi[3];
    uint32_t lo[3], cc[3];
    if (!contacts_box(g, mode, rotation_xyzw, translation, shape3, shape3b, shape1, occ, vlo, vhi, lo, cc)) return IVX_OK;
    const size_t n_box = (size_t)cc[0] * cc[1] * cc[2];
    const size_t off_offsets = n_box * 4, off_total = 2 * n_box * 4, off_out = (off_total + 16 + 63) & ~(size_t)63;
    if ((rc = ensure_dev_scratch(g, off_out + cap * sizeof(ivx_contact)))) return rc;
    char* base = static_cast<char*>(g->dev_scratch);
    uint32_t* d_counts = reinterpret_cast<uint32_t*>(base);
    uint32_t* d_offsets = reinterpret_cast<uint32_t*>(base + off_offsets);
    uint32_t* d_total = reinterpret_cast<uint32_t*>(base + off_total);
    ivx_contact* d_out = reinterpret_cast<ivx_contact*>(base + off_out);
    for (int pass = 0; pass < 2; ++pass)
        if ((rc = ivx_launch_sphere_contacts(g, lo, cc, vlo, vhi, rotation_xyzw, translation, shape3, shape3b, shape1, id_a, id_b, body_a, body_b, response,
                                             d_counts, d_offsets, d_total, d_out, (uint32_t)std::min<size_t>(cap, 0xFFFFFFFFu), pass, mode)))
            return rc;
    return contacts_download(g, who, d_total, d_out, out, cap, n_out);
}

namespace {
// ivx_voxel_object_contacts_many in pieces (ivx_cw_collide_frame runs the same ones over its rows). check: what a query must satisfy | plan: what
// may wait or allocate, ahead of the recording — occupied ranges, the chunk box, a range of the object's scratch for counts and offsets | launch:
// the count pass (pass 0: the scan writes the total to d_total) or the emit pass (pass 1: the contacts go to d_out[0 .. cap_i)), recorded.
struct CollidablePlan {
    struct Box {
        int32_t vlo[3], vhi[3];
        uint32_t lo[3], cc[3];
        bool hit;
        size_t off;  // where this query's counts and offsets start in its object's scratch
    };
    std::vector<Box> box;
    // (an object may appear more than once — near a sphere AND the ground plane, the reference's collision pass visits every collidable near an
    // object —: each query gets a range of its own in the object's scratch, the recorded chains of one object must not share counts)
    std::vector<std::pair<ivx_grid*, size_t>> scratch_need;
    void begin(size_t n) {
        box.assign(n, Box{});
        scratch_need.clear();
    }
};
int collidable_check(ivx_ctx* c, ivx_grid* g, const ivx_collidable_query& q, const char* who, size_t i) {
    IVX_REQUIRE(g && g->ctx == c, IVX_ERR_INVALID, "%s: object %zu is null or belongs to another context", who, i);
    IVX_REQUIRE(q.mode >= 0 && q.mode <= 2, IVX_ERR_INVALID, "%s: query %zu: mode %d", who, i, q.mode);
    return require_whole_object(g, who, false, "object", i);
}
int collidable_plan_row(CollidablePlan& plan, size_t i, ivx_grid* g, const ivx_collidable_query& q, const char* who) {
    uint32_t occ[12];
    if (int rc = ivx_reference_occupied(g, who, occ)) return rc;
    CollidablePlan::Box& b = plan.box[i];
    b.hit = contacts_box(g, q.mode, q.rotation_xyzw, q.translation, q.shape3, q.shape3b, q.shape1, occ, b.vlo, b.vhi, b.lo, b.cc);
    if (!b.hit) return IVX_OK;
    const size_t need = (2 * (size_t)b.cc[0] * b.cc[1] * b.cc[2] * 4 + 64 + 255) & ~(size_t)255;
    auto it = std::find_if(plan.scratch_need.begin(), plan.scratch_need.end(), [&](const std::pair<ivx_grid*, size_t>& e) { return e.first == g; });
    if (it == plan.scratch_need.end()) {
        plan.scratch_need.emplace_back(g, (size_t)0);
        it = plan.scratch_need.end() - 1;
    }
    b.off = it->second;
    it->second += need;
    return IVX_OK;
}
int collidable_plan_scratch(const CollidablePlan& plan) {
    for (const auto& e : plan.scratch_need)
        if (int rc = ensure_dev_scratch(e.first, e.second)) return rc;
    return IVX_OK;
}
int collidable_launch(const CollidablePlan& plan, size_t i, ivx_grid* g, const ivx_collidable_query& q, int pass, uint32_t* d_total, ivx_contact* d_out, uint32_t cap_i) {
    const CollidablePlan::Box& b = plan.box[i];
    const size_t n_box = (size_t)b.cc[0] * b.cc[1] * b.cc[2];
    char* base = static_cast<char*>(g->dev_scratch) + b.off;
    return ivx_launch_sphere_contacts(g, b.lo, b.cc, b.vlo, b.vhi, q.rotation_xyzw, q.translation, q.shape3, q.shape3b, q.shape1, q.collidable_id_a, q.collidable_id_b,
                                      q.body_a, q.body_b, q.response, reinterpret_cast<uint32_t*>(base), reinterpret_cast<uint32_t*>(base + n_box * 4), d_total, d_out,
                                      cap_i, pass, q.mode);
}
}  // namespace

// One collidable per object, N objects, in the launches of one (many.hpp): the reference's collision pass walks every voxel object of the
// scene against the collidables near it (impact_voxel/src/collidable.rs:1051-1286: the per-pair dispatch) — here the pairs (object i,
// collidable i) of one call. Two recorded phases, two waits for ALL objects where the single-object call has two per object: (1) count + scan
// per object, the totals written by the scan straight into host-mapped memory; (2) the emit passes, each object's contacts at its offset of one
// host-mapped buffer, copied to `out` by the host. out_offsets[i] .. out_offsets[i + 1]: object i's contacts, in the order the single-object
// call returns them (a manifold each).
int ivx_voxel_object_contacts_many(ivx_grid* const* grids, size_t n, const ivx_collidable_query* queries, ivx_contact* out, size_t cap, uint32_t* out_offsets) {
    const char* who = "ivx_voxel_object_contacts_many";
    IVX_REQUIRE(out_offsets, IVX_ERR_INVALID, "%s: null argument", who);
    out_offsets[0] = 0;
    if (n == 0) return IVX_OK;
    IVX_REQUIRE(grids && queries && (out || cap == 0), IVX_ERR_INVALID, "%s: null argument", who);
    ivx_ctx* c = grids[0] ? grids[0]->ctx : nullptr;
    int rc;
    for (size_t i = 0; i < n; ++i)
        if ((rc = collidable_check(c, grids[i], queries[i], who, i))) return rc;
    IVX_REQUIRE(!ivx_many_recording(), IVX_ERR_STATE, "%s: not inside an ivx_many_begin bracket (the call waits for its own phases)", who);
    static thread_local CollidablePlan plan;
    plan.begin(n);
    for (size_t i = 0; i < n; ++i)
        if ((rc = collidable_plan_row(plan, i, grids[i], queries[i], who))) return rc;
    if ((rc = collidable_plan_scratch(plan))) return rc;
    uint32_t* totals_dev;
    if ((rc = contacts_many_totals(c, n, &totals_dev))) return rc;
    if ((rc = many_phase(grids, n, [&](size_t i) -> int { return plan.box[i].hit ? collidable_launch(plan, i, grids[i], queries[i], 0, totals_dev + i, nullptr, 0u) : IVX_OK; })))
        return rc;
    return contacts_many_finish(c, grids, n, who, out, cap, out_offsets,
                                [&](size_t i, ivx_contact* list, uint32_t count) { return collidable_launch(plan, i, grids[i], queries[i], 1, nullptr, list, count); });
}

int ivx_sphere_voxel_object_contacts(ivx_grid* g, const float rotation_xyzw[4], const float translation[3], const float sphere_center[3], float sphere_radius,
                                     uint64_t collidable_id_a, uint64_t collidable_id_b, uint32_t body_a, uint32_t body_b, const float response[3],
                                     ivx_contact* out, size_t cap, size_t* n_out) {
    return voxel_object_contacts(g, "ivx_sphere_voxel_object_contacts", 0, rotation_xyzw, translation, sphere_center, nullptr, sphere_radius, collidable_id_a,
                                 collidable_id_b, body_a, body_b, response, out, cap, n_out);
}

int ivx_plane_voxel_object_contacts(ivx_grid* g, const float rotation_xyzw[4], const float translation[3], const float plane_unit_normal[3],
                                    float plane_displacement, uint64_t collidable_id_a, uint64_t collidable_id_b, uint32_t body_a, uint32_t body_b,
                                    const float response[3], ivx_contact* out, size_t cap, size_t* n_out) {
    return voxel_object_contacts(g, "ivx_plane_voxel_object_contacts", 1, rotation_xyzw, translation, plane_unit_normal, nullptr, plane_displacement,
                                 collidable_id_a, collidable_id_b, body_a, body_b, response, out, cap, n_out);
}

int ivx_capsule_voxel_object_contacts(ivx_grid* g, const float rotation_xyzw[4], const float translation[3], const float segment_start[3],
                                      const float segment_vector[3], float capsule_radius, uint64_t collidable_id_a, uint64_t collidable_id_b,
                                      uint32_t body_a, uint32_t body_b, const float response[3], ivx_contact* out, size_t cap, size_t* n_out) {
    return voxel_object_contacts(g, "ivx_capsule_voxel_object_contacts", 2, rotation_xyzw, translation, segment_start, segment_vector, capsule_radius,
                                 collidable_id_a, collidable_id_b, body_a, body_b, response, out, cap, n_out);
}

// ---- collision probes + mutual contacts (second part) ---------------------------------------------------------
void ivx_probe_manager_free(ivx_probe_manager* m) { delete m; }  // (ivx_grid_destroy)
// determine_log2_block_size_for_object (collidable.rs:451-471)
static uint32_t probe_log2_block_size(const uint32_t occ[12]) {
    uint32_t min_extent = 0xFFFFFFFFu;
    for (int d = 0; d < 3; ++d) min_extent = std::min(min_extent, occ[7 + 2 * d] > occ[6 + 2 * d] ? occ[7 + 2 * d] - occ[6 + 2 * d] : 0u);
    return min_extent >= 16 ? 3 : (min_extent >= 8 ? 2 : (min_extent >= 4 ? 1 : 0));
}
int ivx_collision_probes_recompute(ivx_grid* g, size_t* n_points) {
    IVX_REQUIRE(g && n_points, IVX_ERR_INVALID, "ivx_collision_probes_recompute: null argument");
    IVX_REQUIRE(g->mesh_valid, IVX_ERR_STATE, "ivx_collision_probes_recompute: call ivx_remesh first");
    IVX_REQUIRE(g->x_off == 0 && g->gx == g->cc[0] && !g->has_ghost[0] && !g->has_ghost[1], IVX_ERR_STATE,
                "ivx_collision_probes_recompute: not available on a slab of a decomposed grid");
    IVX_REQUIRE(g->cc[0] <= 1024 && g->cc[1] <= 1024 && g->cc[2] <= 1024, IVX_ERR_INVALID, "ivx_collision_probes_recompute: more than 1024 chunks along an axis");
    *n_points = 0;
    int rc;
    uint32_t occ[12];
    if ((rc = ivx_reference_occupied(g, "ivx_collision_probes_recompute", occ))) return rc;
    const uint32_t log2_bs = probe_log2_block_size(occ);
    const uint32_t n_blocks = 1u << (3u * (4u - log2_bs));
    const uint32_t n_sub = g->mesh_counts.n_submeshes;
    g->n_probe_points = 0;
    g->n_probe_sub = n_sub;
    g->probes_serial = g->mesh_serial;
    if (!g->probe_manager) g->probe_manager = new (std::nothrow) ivx_probe_manager();
    IVX_REQUIRE(g->probe_manager, IVX_ERR_HIP, "ivx_collision_probes_recompute: out of host memory");
    ivx_probe_manager* pm = g->probe_manager;
    pm->range_of.clear();
    pm->points.free_ranges.clear();
    pm->total = 0;
    if (n_sub == 0) return IVX_OK;
    if (n_sub > g->probe_entry_cap) {
        if (g->probe_entries) (void)hipFree(g->probe_entries);
        g->probe_entries = nullptr;
        g->probe_entry_cap = 0;
        if ((rc = dev_alloc(&g->probe_entries, (size_t)n_sub * 5))) return rc;
        g->probe_entry_cap = n_sub;
    }
    // scratch: [corner lists: one u32 per index][selected vertices: n_sub * n_blocks][counts n_sub][offsets n_sub + 1][error word]
    const size_t ni = g->mesh_counts.n_indices;
    const size_t off_sel = ni * 4, off_counts = off_sel + (size_t)n_sub * n_blocks * 4, off_offsets = off_counts + (size_t)n_sub * 4,
                 off_err = off_offsets + ((size_t)n_sub + 1) * 4, total = off_err + 4;
    if ((rc = ensure_dev_scratch(g, total))) return rc;
    char* base = static_cast<char*>(g->dev_scratch);
    uint32_t* d_counts = reinterpret_cast<uint32_t*>(base + off_counts);
    uint32_t* d_offsets = reinterpret_cast<uint32_t*>(base + off_offsets);
    uint32_t* d_err = reinterpret_cast<uint32_t*>(base + off_err);
    IVX_HIP_CHECK(ivx_memset_async(d_err, 0, 4, g->ctx->stream));
    if ((rc = ivx_launch_probe_select(g, n_sub, log2_bs, reinterpret_cast<uint32_t*>(base), reinterpret_cast<uint32_t*>(base + off_sel), d_counts, d_offsets,
                                      d_err, nullptr)))
        return rc;
    uint32_t tail[2];  // offsets[n_sub] = total, error word
    if ((rc = d2h(g, tail, d_offsets + n_sub, sizeof(tail)))) return rc;
    IVX_REQUIRE(tail[1] == 0, IVX_ERR_CAPACITY, "ivx_collision_probes_recompute: a chunk submesh holds more vertices than a Surface Nets chunk can");
    const uint32_t n_pts = tail[0];
    if (n_pts > g->probe_point_cap) {
        const size_t cap = std::max<size_t>(n_pts, g->probe_point_cap * 2);
        if (g->probe_points) (void)hipFree(g->probe_points);
        if (g->probe_chunk) (void)hipFree(g->probe_chunk);
        g->probe_points = nullptr;
        g->probe_chunk = nullptr;
        g->probe_point_cap = 0;
        if ((rc = dev_alloc(&g->probe_points, cap * 3))) return rc;
        if ((rc = dev_alloc(&g->probe_chunk, cap))) return rc;
        g->probe_point_cap = cap;
    }
    if ((rc = ivx_launch_probe_gather(g, n_sub, log2_bs, reinterpret_cast<uint32_t*>(base + off_sel), d_counts, d_offsets, g->probe_entries, nullptr))) return rc;
    pm->total = n_pts;
    pm->built = false;  // (the entries stay on the device until a sync or a download asks for them)
    IVX_HIP_CHECK(ivx_stream_sync(g->ctx->stream));
    g->n_probe_points = n_pts;
    *n_points = n_pts;
    return IVX_OK;
}

// the host mirror of chunk_point_ranges after a recompute (clear(): no free ranges), from the entries the gather pass left on the device
static int probe_manager_build(ivx_grid* g) {
    ivx_probe_manager* pm = g->probe_manager;
    if (!pm || pm->built) return IVX_OK;
    std::vector<uint32_t> e((size_t)g->n_probe_sub * 5);
    int rc;
    if (!e.empty() && (rc = d2h(g, e.data(), g->probe_entries, e.size() * 4))) return rc;
    pm->range_of.clear();
    pm->range_of.reserve(g->n_probe_sub);
    pm->points.free_ranges.clear();
    for (uint32_t sidx = 0; sidx < g->n_probe_sub; ++sidx)
        if (e[5 * (size_t)sidx + 4] > e[5 * (size_t)sidx + 3]) {
            const uint32_t c3[3] = {e[5 * (size_t)sidx], e[5 * (size_t)sidx + 1], e[5 * (size_t)sidx + 2]};
            pm->range_of[linear_chunk(g, c3)] = {e[5 * (size_t)sidx + 3], e[5 * (size_t)sidx + 4]};
        }
    pm->built = true;
    return IVX_OK;
}

int ivx_collision_probes_download(ivx_grid* g, float* points, size_t cap_points, uint32_t* chunk_entries, size_t cap_entries, size_t* n_points,
                                  size_t* n_entries) {
    IVX_REQUIRE(g && n_points && n_entries, IVX_ERR_INVALID, "ivx_collision_probes_download: null argument");
    IVX_REQUIRE(g->mesh_valid && g->probes_serial == g->mesh_serial, IVX_ERR_STATE, "ivx_collision_probes_download: call ivx_collision_probes_recompute first");
    *n_points = g->n_probe_points;
    *n_entries = 0;
    int rc;
    size_t ne = 0;  // the live entries in the order of their ranges (= submesh order right after a recompute)
    if ((rc = probe_manager_build(g))) return rc;
    if (g->probe_manager) {
        std::vector<std::pair<uint32_t, uint32_t>> order;
        for (const auto& kv : g->probe_manager->range_of) order.push_back({kv.second.first, kv.first});
        std::sort(order.begin(), order.end());
        for (const auto& o : order) {
            if (chunk_entries && ne < cap_entries) {
                const uint32_t c = o.second;
                const auto& r = g->probe_manager->range_of.at(c);
                uint32_t* e = chunk_entries + 5 * ne;
                e[0] = c / (g->cc[1] * g->cc[2]), e[1] = (c / g->cc[2]) % g->cc[1], e[2] = c % g->cc[2], e[3] = r.first, e[4] = r.second;
            }
            ne += 1;
        }
    }
    *n_entries = ne;
    IVX_REQUIRE(!points || g->n_probe_points <= cap_points, IVX_ERR_CAPACITY, "ivx_collision_probes_download: %u points exceed the capacity %zu",
                g->n_probe_points, cap_points);
    IVX_REQUIRE(!chunk_entries || ne <= cap_entries, IVX_ERR_CAPACITY, "ivx_collision_probes_download: %zu entries exceed the capacity %zu", ne, cap_entries);
    if (points && g->n_probe_points && (rc = d2h(g, points, g->probe_points, (size_t)g->n_probe_points * 12))) return rc;
    return IVX_OK;
}

// VoxelObjectCollisionProbes::sync_with_voxel_object_and_mesh (collidable.rs:394-433, 524-612) in the stages the single-object call and the
// many-objects call share: prepare (host: which chunks, which submesh slots, scratch) | select (device: the points of the listed submeshes
// picked again, their counts) | allocate (host: update_for_chunk chunk by chunk, the RangeAllocator) | gather (device: freed ranges marked,
// the picked points copied to their ranges).
namespace {
struct ProbeSyncJob {
    ivx_grid* g = nullptr;
    uint32_t log2_bs = 0, n_blocks = 0, n_rec = 0;
    std::vector<uint32_t> list, slots, dst;
    std::vector<int32_t> rec_index;
    std::vector<std::pair<uint32_t, uint32_t>> freed;
    size_t off_sel = 0, off_counts = 0, off_dst = 0, off_slots = 0, off_err = 0;
    char* base = nullptr;
};
}  // namespace
static int probe_sync_prepare(ivx_grid* g, const uint8_t* invalidated_chunks, const char* who, ProbeSyncJob& j) {
    IVX_REQUIRE(g && invalidated_chunks, IVX_ERR_INVALID, "%s: null argument", who);
    ivx_submesh_manager* m = g->submesh_manager;
    ivx_probe_manager* pm = g->probe_manager;
    IVX_REQUIRE(g->mesh_valid && m && m->serial == g->mesh_serial, IVX_ERR_STATE, "%s: call ivx_mesh_sync first", who);
    IVX_REQUIRE(pm && (g->probes_serial + 1 == g->mesh_serial || g->probes_serial == g->mesh_serial), IVX_ERR_STATE,
                "%s: the probes must be those of the mesh before the last ivx_mesh_sync (ivx_collision_probes_recompute, or a sync per mesh sync)", who);
    int rc;
    if ((rc = probe_manager_build(g))) return rc;
    uint32_t occ[12];
    if ((rc = ivx_reference_occupied(g, who, occ))) return rc;
    j.g = g;
    j.log2_bs = probe_log2_block_size(occ);
    j.n_blocks = 1u << (3u * (4u - j.log2_bs));
    // the invalidated chunks in chunk-linear order (the reference walks a hash set: unpinned); those that have a submesh get their points picked
    j.list.clear(), j.slots.clear(), j.freed.clear();
    for (uint32_t c = 0; c < g->n_chunks; ++c)
        if (invalidated_chunks[c]) j.list.push_back(c);
    j.rec_index.assign(j.list.size(), -1);
    for (size_t e = 0; e < j.list.size(); ++e) {
        auto it = m->slot_of.find(j.list[e]);
        if (it != m->slot_of.end()) {
            j.rec_index[e] = (int32_t)j.slots.size();
            j.slots.push_back(it->second);
        }
    }
    j.n_rec = (uint32_t)j.slots.size();
    j.dst.assign(j.n_rec, 0u);
    // scratch: [corner lists: one u32 per index][selected vertices: n_rec * n_blocks][counts][dst offsets][slots][error word]
    const size_t ni = m->total_indices, n_rec = j.n_rec;
    j.off_sel = ni * 4, j.off_counts = j.off_sel + n_rec * j.n_blocks * 4, j.off_dst = j.off_counts + n_rec * 4, j.off_slots = j.off_dst + n_rec * 4;
    j.off_err = j.off_slots + n_rec * 4;
    j.base = nullptr;
    if (n_rec) {
        if ((rc = ensure_dev_scratch(g, j.off_err + 4))) return rc;
        j.base = static_cast<char*>(g->dev_scratch);
    }
    return IVX_OK;
}
// d_err: the error word the select pass sets (zeroed by the caller); d_counts_host: optional host-mapped copy of the counts
static int probe_sync_select(ProbeSyncJob& j, uint32_t* d_err, uint32_t* d_counts_host) {
    if (!j.n_rec) return IVX_OK;
    ivx_grid* g = j.g;
    int rc;
    if (!ivx_many_upload(g->ctx, g, j.base + j.off_slots, j.slots.data(), (size_t)j.n_rec * 4) && (rc = h2d(g, j.base + j.off_slots, j.slots.data(), (size_t)j.n_rec * 4)))
        return rc;
    return ivx_launch_probe_select(g, j.n_rec, j.log2_bs, reinterpret_cast<uint32_t*>(j.base), reinterpret_cast<uint32_t*>(j.base + j.off_sel),
                                   reinterpret_cast<uint32_t*>(j.base + j.off_counts), nullptr, d_err, reinterpret_cast<const uint32_t*>(j.base + j.off_slots),
                                   d_counts_host);
}
// update_for_chunk, chunk by chunk (collidable.rs:524-612); *grow: the point buffers must hold pm->total points before the gather
static int probe_sync_allocate(ProbeSyncJob& j, const uint32_t* counts, const char* who, bool* grow) {
    ivx_grid* g = j.g;
    ivx_probe_manager* pm = g->probe_manager;
    for (size_t e = 0; e < j.list.size(); ++e) {
        const uint32_t c = j.list[e];
        const uint32_t n = j.rec_index[e] >= 0 ? counts[(size_t)j.rec_index[e]] : 0u;
        auto old = pm->range_of.find(c);
        if (n == 0) {  // no mesh, or no points
            if (old != pm->range_of.end()) {
                pm->points.free_range(old->second.first, old->second.second);
                j.freed.push_back(old->second);
                pm->range_of.erase(old);
            }
            continue;
        }
        if (old != pm->range_of.end()) {
            pm->points.free_range(old->second.first, old->second.second);
            j.freed.push_back(old->second);
        }
        size_t start;
        if (!pm->points.allocate(n, &start)) start = pm->total, pm->total += n;
        IVX_REQUIRE(pm->total < 0xFFFFFFF0ull, IVX_ERR_CAPACITY, "%s: more than 2^32 probe points", who);
        pm->range_of[c] = {(uint32_t)start, (uint32_t)(start + n)};
        j.dst[(size_t)j.rec_index[e]] = (uint32_t)start;
    }
    pm->points.merge_consecutive();
    *grow = pm->total > g->probe_point_cap;
    return IVX_OK;
}
// grow the point buffers of the listed jobs, keeping what is there: the copies of all, one wait, then the old buffers go
static int probe_sync_grow(ProbeSyncJob* const* jobs, size_t n) {
    if (n == 0) return IVX_OK;
    std::vector<GrowKeep> pending;
    std::vector<size_t> caps(n);
    int rc;
    for (size_t i = 0; i < n; ++i) {
        ivx_grid* g = jobs[i]->g;
        const size_t total = g->probe_manager->total;
        caps[i] = std::max<size_t>(total + total / 2 + 4096, 2 * g->probe_point_cap);
        if ((rc = grow_keep_enqueue(g, &g->probe_points, g->probe_point_cap * 3, caps[i] * 3, pending, 0u))) return rc;
        if ((rc = grow_keep_enqueue(g, &g->probe_chunk, g->probe_point_cap, caps[i], pending, 0u))) return rc;
    }
    IVX_HIP_CHECK(ivx_stream_sync(jobs[0]->g->ctx->stream));
    for (GrowKeep& k : pending) {
        if (*k.slot) (void)hipFree(*k.slot);
        *k.slot = k.fresh;
    }
    for (size_t i = 0; i < n; ++i) jobs[i]->g->probe_point_cap = caps[i];
    return IVX_OK;
}
static int probe_sync_gather(ProbeSyncJob& j) {
    ivx_grid* g = j.g;
    int rc;
    for (const auto& r : j.freed) {  // holes read as "no probe" until a later chunk takes them (the gather below overwrites what was taken now)
        const size_t bytes = (size_t)(r.second - r.first) * 4;
        if (!ivx_many_fill(g->ctx, g, g->probe_chunk + r.first, 0xFFFFFFFFu, bytes)) IVX_HIP_CHECK(ivx_memset_async(g->probe_chunk + r.first, 0xFF, bytes, g->ctx->stream));
    }
    if (j.n_rec) {
        if (!ivx_many_upload(g->ctx, g, j.base + j.off_dst, j.dst.data(), (size_t)j.n_rec * 4) && (rc = h2d(g, j.base + j.off_dst, j.dst.data(), (size_t)j.n_rec * 4)))
            return rc;
        if ((rc = ivx_launch_probe_gather(g, j.n_rec, j.log2_bs, reinterpret_cast<uint32_t*>(j.base + j.off_sel), reinterpret_cast<uint32_t*>(j.base + j.off_counts),
                                          reinterpret_cast<uint32_t*>(j.base + j.off_dst), nullptr, reinterpret_cast<const uint32_t*>(j.base + j.off_slots))))
            return rc;
    }
    return IVX_OK;
}
int ivx_collision_probes_sync(ivx_grid* g, const uint8_t* invalidated_chunks, size_t* n_points) {
    const char* who = "ivx_collision_probes_sync";
    IVX_REQUIRE(g && invalidated_chunks && n_points, IVX_ERR_INVALID, "%s: null argument", who);
    IVX_REQUIRE(!ivx_many_recording(), IVX_ERR_STATE, "%s: not inside an ivx_many_begin bracket (the call waits for the device twice)", who);
    ProbeSyncJob j;
    int rc;
    if ((rc = probe_sync_prepare(g, invalidated_chunks, who, j))) return rc;
    std::vector<uint32_t> counts(j.n_rec);
    if (j.n_rec) {
        uint32_t* d_err = reinterpret_cast<uint32_t*>(j.base + j.off_err);
        IVX_HIP_CHECK(ivx_memset_async(d_err, 0, 4, g->ctx->stream));
        if ((rc = probe_sync_select(j, d_err, nullptr))) return rc;
        if ((rc = d2h(g, counts.data(), j.base + j.off_counts, (size_t)j.n_rec * 4))) return rc;
        uint32_t err = 0;
        if ((rc = d2h(g, &err, d_err, 4))) return rc;
        IVX_REQUIRE(err == 0, IVX_ERR_CAPACITY, "%s: a chunk submesh holds more vertices than a Surface Nets chunk can", who);
    }
    bool grow = false;
    if ((rc = probe_sync_allocate(j, counts.data(), who, &grow))) return rc;
    ProbeSyncJob* one = &j;
    if (grow && (rc = probe_sync_grow(&one, 1))) return rc;
    if ((rc = probe_sync_gather(j))) return rc;
    IVX_HIP_CHECK(ivx_stream_sync(g->ctx->stream));
    g->n_probe_points = (uint32_t)g->probe_manager->total;
    g->probes_serial = g->mesh_serial;
    *n_points = g->probe_manager->total;
    return IVX_OK;
}

// The same for N objects of one context in the launches of one (many.hpp) — every voxel object's probes follow its mesh each frame
// (impact_voxel/src/lib.rs:729-733 with collidable.rs:394-433) —: the select passes of all objects merged, their counts and error words written
// into host-mapped memory, ONE wait; the allocators of all objects on the host; the fills and gathers of all objects merged, ONE wait.
int ivx_collision_probes_sync_many(ivx_grid* const* grids, size_t n, const uint8_t* const* invalidated_chunks, size_t* n_points) {
    const char* who = "ivx_collision_probes_sync_many";
    if (n == 0) return IVX_OK;
    IVX_REQUIRE(grids && invalidated_chunks && n_points, IVX_ERR_INVALID, "%s: null argument", who);
    int rc = many_check(grids, n, who);
    if (rc) return rc;
    IVX_REQUIRE(!ivx_many_recording(), IVX_ERR_STATE, "%s: not inside an ivx_many_begin bracket (the call waits for its own phases)", who);
    ivx_ctx* c = grids[0]->ctx;
    static thread_local std::vector<ProbeSyncJob> jobs;
    if (jobs.size() < n) jobs.resize(n);
    size_t words = 0;
    static thread_local std::vector<size_t> off;
    off.assign(n, 0);
    for (size_t i = 0; i < n; ++i) {
        if ((rc = probe_sync_prepare(grids[i], invalidated_chunks[i], who, jobs[i]))) return rc;
        off[i] = n + words;  // [error word per object][counts of every object]
        words += jobs[i].n_rec;
    }
    if ((rc = ctx_pinned_scratch(c, (n + words) * 4 + 64))) return rc;
    uint32_t* host = static_cast<uint32_t*>(c->pinned_scratch.p);
    uint32_t* host_dev = static_cast<uint32_t*>(c->pinned_scratch.dev);
    memset(host, 0, (n + words) * 4);
    if (words) {
        if ((rc = many_phase(grids, n, [&](size_t i) -> int { return probe_sync_select(jobs[i], host_dev + i, host_dev + off[i]); }))) return many_fail(grids, n, rc);
        IVX_HIP_CHECK(ivx_stream_sync(c->stream));
    }
    for (size_t i = 0; i < n; ++i)
        IVX_REQUIRE(host[i] == 0, IVX_ERR_CAPACITY, "%s: object %zu: a chunk submesh holds more vertices than a Surface Nets chunk can", who, i);
    static thread_local std::vector<ProbeSyncJob*> growing;
    growing.clear();
    for (size_t i = 0; i < n; ++i) {
        bool grow = false;
        if ((rc = probe_sync_allocate(jobs[i], host + off[i], who, &grow))) return rc;
        if (grow) growing.push_back(&jobs[i]);
    }
    if ((rc = probe_sync_grow(growing.data(), growing.size()))) return rc;
    if ((rc = many_phase(grids, n, [&](size_t i) -> int { return probe_sync_gather(jobs[i]); }))) return many_fail(grids, n, rc);
    IVX_HIP_CHECK(ivx_stream_sync(c->stream));
    for (size_t i = 0; i < n; ++i) {
        ivx_grid* g = grids[i];
        g->n_probe_points = (uint32_t)g->probe_manager->total;
        g->probes_serial = g->mesh_serial;
        n_points[i] = g->probe_manager->total;
    }
    return IVX_OK;
}

// what the two passes of a pair's mutual contacts need (for_each_mutual_voxel_object_contact, collidable.rs:859-1049): the intersection ranges of
// the two objects' occupied boxes in each other's frames, the probers' chunk ranges, the id prefix. *hit false: the boxes do not meet.
static int mutual_prepare(const char* who, ivx_grid* a, const float rotation_a[4], const float translation_a[3], const float center_of_mass_a[3], ivx_grid* b,
                          const float rotation_b[4], const float translation_b[3], const float center_of_mass_b[3], uint64_t collidable_id_a,
                          uint64_t collidable_id_b, uint32_t body_a, uint32_t body_b, const float response[3], ivx_mutual_pass pass[2], bool* hit) {
    int rc;
    *hit = true;
    uint32_t occ_a[12], occ_b[12];
    if ((rc = ivx_reference_occupied(a, who, occ_a))) return rc;
    if ((rc = ivx_reference_occupied(b, who, occ_b))) return rc;
    long ra_lo[3], ra_hi[3], rb_lo[3], rb_hi[3];
    float q_ba[4], t_ba[3];
    if (!host_intersection_ranges(a, occ_a, rotation_a, translation_a, b, occ_b, rotation_b, translation_b, ra_lo, ra_hi, rb_lo, rb_hi, q_ba, t_ba)) {
        *hit = false;
        return IVX_OK;
    }
    // ContactID::from_two_u64_and_n_indices: the part that does not depend on the probe
    pass[0].id_ab = pass[1].id_ab = splitmix(collidable_id_a ^ splitmix(collidable_id_b));
    for (int w = 0; w < 2; ++w) {
        ivx_mutual_pass& p = pass[w];
        ivx_grid* prober = w ? b : a;
        ivx_grid* sampled = w ? a : b;
        const long* rlo = w ? rb_lo : ra_lo;
        const long* rhi = w ? rb_hi : ra_hi;
        const float* com_s = w ? center_of_mass_a : center_of_mass_b;
        const float inv_s = 1.0f / sampled->extent;
        for (int d = 0; d < 3; ++d) {
            p.center_s[d] = com_s[d] * inv_s;
            p.q_s[d] = (w ? rotation_a : rotation_b)[d];
            p.q_p[d] = (w ? rotation_b : rotation_a)[d];
            p.t_s[d] = (w ? translation_a : translation_b)[d];
            p.t_p[d] = (w ? translation_b : translation_a)[d];
            // aabb_from_voxel_ranges(prober's extent, ranges).expanded_about_center(object_a.voxel_extent()) — A's extent in both passes
            p.box_lo[d] = prober->extent * (float)rlo[d] - a->extent;
            p.box_hi[d] = prober->extent * (float)rhi[d] + a->extent;
            // chunk_range_encompassing_voxel_range (object.rs:3236-3240)
            p.clo[d] = (uint32_t)(rlo[d] / 16);
            p.chi[d] = (uint32_t)((rhi[d] + 15) / 16);
            p.response[d] = response[d];
        }
        p.q_s[3] = (w ? rotation_a : rotation_b)[3];
        p.q_p[3] = (w ? rotation_b : rotation_a)[3];
        p.negate = w;
        p.body_a = body_a;
        p.body_b = body_b;
    }
    return IVX_OK;
}

int ivx_mutual_voxel_object_contacts(ivx_grid* a, const float rotation_a[4], const float translation_a[3], const float center_of_mass_a[3], ivx_grid* b,
                                     const float rotation_b[4], const float translation_b[3], const float center_of_mass_b[3], uint64_t collidable_id_a,
                                     uint64_t collidable_id_b, uint32_t body_a, uint32_t body_b, const float response[3], ivx_contact* out, size_t cap,
                                     size_t* n_out) {
    const char* who = "ivx_mutual_voxel_object_contacts";
    IVX_REQUIRE(a && b && rotation_a && translation_a && center_of_mass_a && rotation_b && translation_b && center_of_mass_b && response && n_out &&
                    (out || cap == 0),
                IVX_ERR_INVALID, "%s: null argument", who);
    IVX_REQUIRE(a != b && a->ctx == b->ctx, IVX_ERR_INVALID, "%s: two different objects of one context are needed", who);
    int rc;
    for (ivx_grid* g : {a, b})
        if ((rc = require_whole_object(g, who, true))) return rc;
    *n_out = 0;
    ivx_mutual_pass pass[2];
    bool hit = false;
    if ((rc = mutual_prepare(who, a, rotation_a, translation_a, center_of_mass_a, b, rotation_b, translation_b, center_of_mass_b, collidable_id_a, collidable_id_b, body_a,
                             body_b, response, pass, &hit)))
        return rc;
    if (!hit) return IVX_OK;
    const uint32_t wg_a = (a->n_probe_points + 255u) / 256u, wg_b = (b->n_probe_points + 255u) / 256u, n_wg = wg_a + wg_b;
    if (n_wg == 0) return IVX_OK;
    // scratch (object A's): [counts n_wg][offsets n_wg + 1][contacts]
    const size_t off_offsets = (size_t)n_wg * 4, off_out = (off_offsets + ((size_t)n_wg + 1) * 4 + 63) & ~(size_t)63;
    if ((rc = ensure_dev_scratch(a, off_out + cap * sizeof(ivx_contact)))) return rc;
    char* base = static_cast<char*>(a->dev_scratch);
    uint32_t* d_counts = reinterpret_cast<uint32_t*>(base);
    uint32_t* d_offsets = reinterpret_cast<uint32_t*>(base + off_offsets);
    ivx_contact* d_out = reinterpret_cast<ivx_contact*>(base + off_out);
    const uint32_t cap32 = (uint32_t)std::min<size_t>(cap, 0xFFFFFFFFu);
    if ((rc = ivx_launch_mutual_pass(a, b, &pass[0], d_counts, nullptr, nullptr, cap32, 0))) return rc;
    if ((rc = ivx_launch_mutual_pass(b, a, &pass[1], d_counts + wg_a, nullptr, nullptr, cap32, 0))) return rc;
    if ((rc = ivx_launch_scan_counts(a->ctx, n_wg, d_counts, d_offsets))) return rc;
    if ((rc = ivx_launch_mutual_pass(a, b, &pass[0], nullptr, d_offsets, d_out, cap32, 1))) return rc;
    if ((rc = ivx_launch_mutual_pass(b, a, &pass[1], nullptr, d_offsets + wg_a, d_out, cap32, 1))) return rc;
    return contacts_download(a, who, d_offsets + n_wg, d_out, out, cap, n_out);
}

namespace {
// ivx_mutual_voxel_object_contacts_many in pieces (ivx_cw_collide_frame runs the same ones over its rows). check | plan: mutual_prepare and the
// pair's range of counts and offsets in the context's device scratch, which plan_scratch then grows | count: A's probes in B's field, B's in A's,
// the scan with its total to d_total | emit: both passes into list[0 .. count), recorded.
struct MutualPlan {
    struct Pair {
        ivx_mutual_pass pass[2];
        uint32_t wg_a, wg_b;
        size_t off;  // of the pair's counts / offsets in the context's scratch (u32 words)
        bool hit;
    };
    std::vector<Pair> pr;
    size_t words = 0;
    uint32_t* base = nullptr;
    void begin(size_t n) {
        pr.assign(n, Pair{});
        words = 0, base = nullptr;
    }
};
int mutual_check(ivx_ctx* c, const ivx_mutual_query& q, const char* who, size_t i) {
    IVX_REQUIRE(q.a && q.b && q.a != q.b && q.a->ctx == c && q.b->ctx == c, IVX_ERR_INVALID, "%s: pair %zu: two different objects of the call's context are needed", who, i);
    for (ivx_grid* g : {q.a, q.b})
        if (int rc = require_whole_object(g, who, true, "pair", i)) return rc;
    return IVX_OK;
}
int mutual_plan_row(MutualPlan& plan, size_t i, const ivx_mutual_query& q, const char* who) {
    MutualPlan::Pair& p = plan.pr[i];
    if (int rc = mutual_prepare(who, q.a, q.rotation_a, q.translation_a, q.center_of_mass_a, q.b, q.rotation_b, q.translation_b, q.center_of_mass_b, q.collidable_id_a,
                                q.collidable_id_b, q.body_a, q.body_b, q.response, p.pass, &p.hit))
        return rc;
    p.wg_a = (q.a->n_probe_points + 255u) / 256u, p.wg_b = (q.b->n_probe_points + 255u) / 256u;
    if (p.wg_a + p.wg_b == 0) p.hit = false;
    p.off = plan.words;
    if (p.hit) plan.words += 2 * (size_t)(p.wg_a + p.wg_b) + 16;
    return IVX_OK;
}
// counts and offsets of all pairs: one block of the context's device scratch
int mutual_plan_scratch(MutualPlan& plan, ivx_ctx* c) {
    if (int rc = ivx_buf_grow(c, &c->dev_scratch, plan.words * 4 + 64, 1 << 20)) return rc;
    plan.base = static_cast<uint32_t*>(c->dev_scratch.p);
    return IVX_OK;
}
int mutual_count(const MutualPlan& plan, size_t i, const ivx_mutual_query& q, ivx_ctx* c, uint32_t* d_total) {
    const MutualPlan::Pair& p = plan.pr[i];
    if (!p.hit) return IVX_OK;
    const uint32_t n_wg = p.wg_a + p.wg_b;
    uint32_t* d_counts = plan.base + p.off;
    uint32_t* d_offsets = d_counts + n_wg;
    int r;
    if ((r = ivx_launch_mutual_pass(q.a, q.b, &p.pass[0], d_counts, nullptr, nullptr, 0u, 0))) return r;
    if ((r = ivx_launch_mutual_pass(q.b, q.a, &p.pass[1], d_counts + p.wg_a, nullptr, nullptr, 0u, 0))) return r;
    return ivx_launch_scan_counts(c, n_wg, d_counts, d_offsets, d_total, q.a);
}
int mutual_emit(const MutualPlan& plan, size_t i, const ivx_mutual_query& q, ivx_contact* list, uint32_t count) {
    const MutualPlan::Pair& p = plan.pr[i];
    const uint32_t* d_offsets = plan.base + p.off + (p.wg_a + p.wg_b);
    const int r = ivx_launch_mutual_pass(q.a, q.b, &p.pass[0], nullptr, d_offsets, list, count, 1);
    return r ? r : ivx_launch_mutual_pass(q.b, q.a, &p.pass[1], nullptr, d_offsets + p.wg_a, list, count, 1);
}
}  // namespace

// The same for a LIST of pairs in the launches of one (many.hpp) — the reference's narrow phase visits every pair of voxel objects the broad
// phase hands it (collidable.rs:859-1049 per pair) —: per pair count (A's probes in B's field) | count (B's in A's) | scan, recorded for all
// pairs and issued merged, the totals written by the scans into host-mapped memory; one wait; then the emit passes of all pairs into one
// host-mapped list; one wait. out_offsets[i] .. out_offsets[i + 1]: pair i's manifold, the list the single-pair call returns.
int ivx_mutual_voxel_object_contacts_many(const ivx_mutual_query* queries, size_t n, ivx_contact* out, size_t cap, uint32_t* out_offsets) {
    const char* who = "ivx_mutual_voxel_object_contacts_many";
    IVX_REQUIRE(out_offsets, IVX_ERR_INVALID, "%s: null argument", who);
    out_offsets[0] = 0;
    if (n == 0) return IVX_OK;
    IVX_REQUIRE(queries && (out || cap == 0), IVX_ERR_INVALID, "%s: null argument", who);
    ivx_ctx* c = queries[0].a ? queries[0].a->ctx : nullptr;
    int rc;
    for (size_t i = 0; i < n; ++i)
        if ((rc = mutual_check(c, queries[i], who, i))) return rc;
    IVX_REQUIRE(!ivx_many_recording(), IVX_ERR_STATE, "%s: not inside an ivx_many_begin bracket (the call waits for its own phases)", who);
    static thread_local MutualPlan plan;
    plan.begin(n);
    for (size_t i = 0; i < n; ++i)
        if ((rc = mutual_plan_row(plan, i, queries[i], who))) return rc;
    // totals and contacts: the context's pinned block
    if ((rc = mutual_plan_scratch(plan, c))) return rc;
    uint32_t* totals_dev;
    if ((rc = contacts_many_totals(c, n, &totals_dev))) return rc;
    std::vector<ivx_grid*> chain(n);  // (the recorder's chains go by pair: the first object of each stands for it)
    for (size_t i = 0; i < n; ++i) chain[i] = queries[i].a;
    if ((rc = many_phase(chain.data(), n, [&](size_t i) -> int { return mutual_count(plan, i, queries[i], c, totals_dev + i); }))) return rc;
    return contacts_many_finish(c, chain.data(), n, who, out, cap, out_offsets,
                                [&](size_t i, ivx_contact* list, uint32_t count) -> int { return mutual_emit(plan, i, queries[i], list, count); });
}

// The whole collision pass of a frame (include/impact_voxel_hip.h): narrow.hip's pair pass, primitive narrow phase and rows (two waits), then the
// two generator families over the rows — planned with the pieces above, their count passes and scans recorded in ONE phase so that collidable
// rows and mutual rows merge launch by launch (third wait: the totals), their emit passes writing behind the primitive contacts in the world's
// contact buffer (fourth wait: the list).
int ivx_cw_collide_frame(ivx_world* w, uint32_t mode, ivx_contact* out, size_t cap, size_t* n_out, size_t* n_primitive, uint32_t* deferred_pairs,
                         uint32_t* manifold_offsets, size_t deferred_cap, size_t* n_deferred) {
    const char* who = "ivx_cw_collide_frame";
    IVX_REQUIRE(n_out && n_primitive && n_deferred, IVX_ERR_INVALID, "%s: null argument", who);
    *n_out = 0, *n_primitive = 0, *n_deferred = 0;
    IVX_REQUIRE(w, IVX_ERR_INVALID, "%s: null world", who);
    IVX_REQUIRE(mode <= IVX_BV_DYNAMIC_PAIRS, IVX_ERR_INVALID, "%s: mode %u (0 = all pairs, 1 = no phantom and at least one dynamic member)", who, mode);
    IVX_REQUIRE(out || cap == 0, IVX_ERR_INVALID, "%s: null contact buffer of capacity %zu", who, cap);
    IVX_REQUIRE((deferred_pairs && manifold_offsets) || deferred_cap == 0, IVX_ERR_INVALID, "%s: null deferred pair or offset buffer of capacity %zu", who, deferred_cap);
    IVX_REQUIRE(!ivx_many_recording(), IVX_ERR_STATE, "%s: not inside an ivx_many_begin bracket (the call waits for its own phases)", who);
    const bool lists = deferred_pairs && manifold_offsets;
    ivx_cw_frame_pass fp;
    int rc;
    if ((rc = ivx_cw_frame_pairs(w, who, mode, out ? cap : 0, lists ? deferred_cap : 0, &fp))) return rc;
    const size_t np = fp.n_primitive, nd = fp.n_deferred;
    *n_out = np, *n_primitive = np, *n_deferred = nd;
    ivx_ctx* c = w->ctx;
    // the rows as the generators' queries, by field copies; the object that stands for row i in the recorder
    static thread_local std::vector<ivx_collidable_query> cq;
    static thread_local std::vector<ivx_mutual_query> mq;
    static thread_local std::vector<ivx_grid*> chain;
    static thread_local std::vector<uint32_t> offsets, counts;
    static thread_local CollidablePlan cplan;
    static thread_local MutualPlan mplan;
    cq.assign(nd, ivx_collidable_query{}), mq.assign(nd, ivx_mutual_query{}), chain.assign(nd, nullptr), offsets.assign(nd + 1, 0u);
    for (size_t i = 0; i < nd; ++i) {
        const ivx_cw_row& r = fp.rows[i];
        IVX_REQUIRE(r.voxel < fp.n_collidables && r.other < fp.n_collidables && r.generator <= IVX_CW_ROW_MUTUAL, IVX_ERR_STATE, "%s: row %zu is not a dispatch", who, i);
        ivx_grid* g = fp.objects[r.voxel].grid;
        IVX_REQUIRE(g, IVX_ERR_STATE, "%s: deferred pair %zu names voxel collidable %u, which has no object attached (ivx_cw_set_voxel_objects)", who, i, r.voxel);
        chain[i] = g;
        if (r.generator == IVX_CW_ROW_MUTUAL) {
            ivx_grid* b = fp.objects[r.other].grid;
            IVX_REQUIRE(b, IVX_ERR_STATE, "%s: deferred pair %zu names voxel collidable %u, which has no object attached (ivx_cw_set_voxel_objects)", who, i, r.other);
            ivx_mutual_query& q = mq[i];
            q.a = g, q.b = b;
            memcpy(q.rotation_a, r.rotation_a, 16), memcpy(q.translation_a, r.translation_a, 12), memcpy(q.center_of_mass_a, r.center_of_mass_a, 12);
            memcpy(q.rotation_b, r.rotation_b, 16), memcpy(q.translation_b, r.translation_b, 12), memcpy(q.center_of_mass_b, r.center_of_mass_b, 12);
            q.collidable_id_a = r.collidable_id_a, q.collidable_id_b = r.collidable_id_b, q.body_a = r.body_a, q.body_b = r.body_b;
            memcpy(q.response, r.response, 12);
            if ((rc = mutual_check(c, q, who, i))) return rc;
        } else {
            ivx_collidable_query& q = cq[i];
            q.mode = (int32_t)r.generator;
            memcpy(q.rotation_xyzw, r.rotation_a, 16), memcpy(q.translation, r.translation_a, 12);
            memcpy(q.shape3, r.shape3, 12), memcpy(q.shape3b, r.shape3b, 12);
            q.shape1 = r.shape1, q.body_a = r.body_a, q.body_b = r.body_b, q.collidable_id_a = r.collidable_id_a, q.collidable_id_b = r.collidable_id_b;
            memcpy(q.response, r.response, 12);
            if ((rc = collidable_check(c, g, q, who, i))) return rc;
        }
    }
    size_t run = 0;
    const auto mutual = [&](size_t i) { return fp.rows[i].generator == IVX_CW_ROW_MUTUAL; };
    if (nd) {
        cplan.begin(nd), mplan.begin(nd);
        for (size_t i = 0; i < nd; ++i)
            if ((rc = mutual(i) ? mutual_plan_row(mplan, i, mq[i], who) : collidable_plan_row(cplan, i, chain[i], cq[i], who))) return rc;
        if ((rc = collidable_plan_scratch(cplan))) return rc;
        if ((rc = mutual_plan_scratch(mplan, c))) return rc;
        uint32_t* totals_dev;
        if ((rc = contacts_many_totals(c, nd, &totals_dev))) return rc;
        if ((rc = many_phase(chain.data(), nd, [&](size_t i) -> int {
                 if (mutual(i)) return mutual_count(mplan, i, mq[i], c, totals_dev + i);
                 return cplan.box[i].hit ? collidable_launch(cplan, i, chain[i], cq[i], 0, totals_dev + i, nullptr, 0u) : IVX_OK;
             })))
            return rc;
        if ((rc = contacts_many_wait_totals(c, nd, offsets.data(), counts, &run))) return rc;
    }
    const size_t total = np + run;
    *n_out = total;
    IVX_REQUIRE(!out || total <= cap, IVX_ERR_CAPACITY, "%s: %zu contacts (%zu primitive), the buffer holds %zu", who, total, np, cap);
    IVX_REQUIRE(!lists || nd <= deferred_cap, IVX_ERR_CAPACITY, "%s: %zu deferred pairs, the buffers hold %zu", who, nd, deferred_cap);
    if (run) {
        ivx_contact* list;
        if ((rc = ivx_cw_frame_reserve(w, np, total, &list))) return rc;
        if ((rc = contacts_many_emit(chain.data(), nd, counts, offsets.data(), list + np, [&](size_t i, ivx_contact* at, uint32_t count) -> int {
                 return mutual(i) ? mutual_emit(mplan, i, mq[i], at, count) : collidable_launch(cplan, i, chain[i], cq[i], 1, nullptr, at, count);
             })))
            return rc;
        if ((rc = ivx_cw_frame_finish(w, total, out))) return rc;
    } else if (out && np) {
        memcpy(out, fp.contacts, np * sizeof(ivx_contact));  // (no manifold: the primitive contacts came with the counts, as in ivx_cw_collide)
    }
    if (lists) {
        if (nd) memcpy(deferred_pairs, fp.deferred, nd * 8);
        memcpy(manifold_offsets, offsets.data(), (nd + 1) * 4);
    }
    return IVX_OK;
}
