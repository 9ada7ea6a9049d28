// Motion drivers of kinematic bodies on the device: the reference's MotionDriverManager::apply_motion (impact_physics/src/driven_motion.rs:50-82)
// behind the step's advance of configurations.
//
// Reference behaviour reproduced (engine/crates/impact_physics/src/driven_motion):
//   CircularTrajectory::compute_position_and_velocity              circular.rs:134-194
//   ConstantAccelerationTrajectory::compute_position_and_velocity  constant_acceleration.rs:143-157
//   HarmonicOscillatorTrajectory::compute_position_and_velocity    harmonic_oscillation.rs:139-159
//   OrbitalTrajectory::compute_position_and_velocity               orbit.rs:149-365
//   ConstantRotation::compute_orientation                          constant_rotation.rs:111-120
//   reset + additive apply per driver, rotations last              driven_motion.rs:50-82
//
// ONE evaluation function with a switch over the kind (md_eval), host and device: the kinds diverge inside a wave, and five kernels would only
// make five launches of mostly idle waves. The composition (md_apply_body) is shared with ivx_md_apply_host in the same way. f32 throughout, no
// contraction, IEEE sqrt / div, the operation order of the reference (stated once per kind in include/impact_voxel_hip.h); sin, cos and tan go
// through double precision rounded once (physics_internal.hpp, sin_rn).
//
// k_motion_apply: a lane per DRIVEN body, 256-thread workgroups, no atomics, no LDS. The host sorts the set once per
// ivx_world_set_motion_drivers, stably by (body, kind, list index), and builds the compact list of driven bodies with their offsets into the
// sorted array; a lane reads its body, walks its drivers in that order and stores the body once.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ivx_internal.hpp"
#include "device_common.hpp"
#include "physics_internal.hpp"
#include "vec3.hpp"

namespace {

using namespace ivx_vec;  // V3, Q4, mk, ld3, st3, the operators, qrot
using ivx_phys::advance_orientation;
using ivx_phys::cos_rn;
using ivx_phys::sin_rn;
using ivx_phys::tan_rn;

#define MD_HD __host__ __device__ __forceinline__

#define MD_TWO_PI 6.2831855f  // impact_math::consts::f32::TWO_PI
#define MD_PI 3.1415927f

struct MdOut {
    V3 a, b;  // trajectory kinds: position, velocity; constant rotation: axis in a
    Q4 q;     // constant rotation: orientation
    float speed;
};

MD_HD Q4 ldq4(const float* p) { return Q4{p[0], p[1], p[2], p[3]}; }

// OrbitalTrajectory::compute_eccentric_anomaly (orbit.rs:243-269): Newton from the mean anomaly, |step| <= 1e-4 or 100 iterations
MD_HD float md_eccentric_anomaly(float e, float mean_anomaly) {
    float ecc = mean_anomaly;
    float error = INFINITY;
    int it = 0;
    while (error > 1e-4f && it < 100) {
        const float f = (ecc - e * sin_rn(ecc)) - mean_anomaly;
        const float df = 1.0f - e * cos_rn(ecc);
        const float next = ecc - f / df;
        error = fabsf(next - ecc);
        ecc = next;
        ++it;
    }
    return ecc;
}

// one driver at `time` (the operation order: include/impact_voxel_hip.h, "Arithmetic")
MD_HD MdOut md_eval(uint32_t kind, const float* p, float time) {
    MdOut o;
    o.a = mk(0.0f, 0.0f, 0.0f), o.b = mk(0.0f, 0.0f, 0.0f), o.q = Q4{0.0f, 0.0f, 0.0f, 0.0f}, o.speed = 0.0f;
    switch (kind) {
    case IVX_MD_CIRCULAR: {
        const Q4 q = ldq4(p + 1);
        const float radius = p[8], period = p[9];
        const float w = MD_TWO_PI / period;
        const float angle = fmodf(w * (time - p[0]), MD_TWO_PI);
        const float s = sin_rn(angle), c = cos_rn(angle);
        o.a = ld3(p + 5) + qrot(q, mk(radius * c, radius * s, 0.0f));
        const float v = radius * w;
        o.b = qrot(q, mk(-v * s, v * c, 0.0f));
    } break;
    case IVX_MD_CONSTANT_ACCELERATION: {
        const float dt = time - p[0];
        const V3 v0 = ld3(p + 4), acc = ld3(p + 7);
        o.a = (ld3(p + 1) + v0 * dt) + acc * (0.5f * (dt * dt));
        o.b = v0 + acc * dt;
    } break;
    case IVX_MD_HARMONIC: {
        const float dt = time - p[0];
        const V3 dir = ld3(p + 4);
        const float amplitude = p[7];
        const float w = MD_TWO_PI / p[8];
        o.a = ld3(p + 1) + dir * (amplitude * sin_rn(w * dt));
        o.b = dir * ((amplitude * w) * cos_rn(w * dt));
    } break;
    case IVX_MD_ORBITAL: {
        const Q4 q = ldq4(p + 1);
        const float a = p[8], e = p[9], period = p[10];
        const float n = MD_TWO_PI / period;
        const float mean_anomaly = fmodf(n * (time - p[0]), MD_TWO_PI);
        const float ecc = md_eccentric_anomaly(e, mean_anomaly);
        const float f2 = (1.0f + e) / (1.0f - e);
        const float f = sqrtf(f2);
        const float th = tan_rn(0.5f * ecc);
        const float th2 = th * th;
        const float tv2 = f2 * th2;
        const float k = 1.0f / (1.0f + tv2);
        const float cos_v = (1.0f - tv2) * k;
        const float dv_de = (f * (1.0f + th2)) * k;
        const float r = (a * (1.0f - e * e)) / (1.0f + e * cos_v);
        const float root = sqrtf(1.0f - cos_v * cos_v);
        const float sin_v = ecc <= MD_PI ? root : -root;  // (the sign comes from the eccentric anomaly alone: a negative one takes the positive root)
        o.a = ld3(p + 5) + qrot(q, mk(r * cos_v, r * sin_v, 0.0f));
        const float dv = (n * dv_de) / (1.0f - e * cos_rn(ecc));
        const float den = 1.0f + e * cos_v;
        const float vr = ((((dv * e) * a) * (1.0f - e * e)) * sin_v) / (den * den);
        const float vt = r * dv;
        o.b = qrot(q, mk(vr * cos_v - vt * sin_v, vr * sin_v + vt * cos_v, 0.0f));
    } break;
    default: {  // IVX_MD_CONSTANT_ROTATION (the kinds are validated on the host)
        o.a = ld3(p + 5);
        o.speed = p[8];
        o.q = advance_orientation(ldq4(p + 1), o.a, o.speed, time - p[0]);
    } break;
    }
    return o;
}

// apply_motion for ONE body: its drivers [begin, end) of the sorted array — trajectory kinds first (kind order, then list order), rotations last
MD_HD void md_apply_body(ivx_kinematic_body& k, const ivx_motion_driver* drv, uint32_t begin, uint32_t end, float time) {
    bool reset = false;
    for (uint32_t j = begin; j < end; ++j) {
        const uint32_t kind = drv[j].kind;
        const MdOut o = md_eval(kind, drv[j].p, time);
        if (kind < IVX_MD_CONSTANT_ROTATION) {
            if (!reset) {
                st3(k.position, mk(0.0f, 0.0f, 0.0f));
                st3(k.velocity, mk(0.0f, 0.0f, 0.0f));
                reset = true;
            }
            st3(k.position, ld3(k.position) + o.a);
            st3(k.velocity, ld3(k.velocity) + o.b);
        } else {
            k.orientation[0] = o.q.x, k.orientation[1] = o.q.y, k.orientation[2] = o.q.z, k.orientation[3] = o.q.w;
            st3(k.angular_axis, o.a);
            k.angular_speed = o.speed;
        }
    }
}

__global__ __launch_bounds__(256) void k_motion_apply(const ivx_motion_driver* __restrict__ drv, const uint32_t* __restrict__ bodies,
                                                      const uint32_t* __restrict__ offsets, uint32_t n_driven, float time,
                                                      ivx_kinematic_body* __restrict__ kin) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_driven) return;
    const uint32_t b = bodies[i];  // (< the world's kinematic bodies: checked on the host before every launch)
    ivx_kinematic_body k = kin[b];
    md_apply_body(k, drv, offsets[i], offsets[i + 1u], time);
    kin[b] = k;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
const char* const MD_KIND_NAMES[5] = {"circular trajectory", "constant-acceleration trajectory", "harmonic-oscillator trajectory", "orbital trajectory",
                                      "constant rotation"};

// what the reference asserts when it applies a driver (abs_diff_ne!(period, 0.0) with the default epsilon: |period| > f32::EPSILON)
int md_validate_one(const char* who, const ivx_motion_driver& d, size_t i) {
    IVX_REQUIRE(d.kind <= IVX_MD_CONSTANT_ROTATION, IVX_ERR_INVALID, "%s: driver %zu has kind %u (0 circular, 1 constant acceleration, 2 harmonic, 3 orbital, 4 constant rotation)",
                who, i, d.kind);
    const float eps = 1.1920929e-07f;
    const char* name = MD_KIND_NAMES[d.kind];
    if (d.kind == IVX_MD_CIRCULAR) {
        IVX_REQUIRE(d.p[8] > 0.0f, IVX_ERR_INVALID, "%s: driver %zu (%s): the radius %g does not exceed zero", who, i, name, (double)d.p[8]);
        IVX_REQUIRE(fabsf(d.p[9]) > eps, IVX_ERR_INVALID, "%s: driver %zu (%s): the period %g is zero", who, i, name, (double)d.p[9]);
    } else if (d.kind == IVX_MD_HARMONIC) {
        IVX_REQUIRE(fabsf(d.p[8]) > eps, IVX_ERR_INVALID, "%s: driver %zu (%s): the period %g is zero", who, i, name, (double)d.p[8]);
    } else if (d.kind == IVX_MD_ORBITAL) {
        IVX_REQUIRE(d.p[8] > 0.0f, IVX_ERR_INVALID, "%s: driver %zu (%s): the semi-major axis %g does not exceed zero", who, i, name, (double)d.p[8]);
        IVX_REQUIRE(d.p[9] >= 0.0f && d.p[9] < 1.0f, IVX_ERR_INVALID, "%s: driver %zu (%s): the eccentricity %g is not in [0, 1)", who, i, name, (double)d.p[9]);
        IVX_REQUIRE(fabsf(d.p[10]) > eps, IVX_ERR_INVALID, "%s: driver %zu (%s): the period %g is zero", who, i, name, (double)d.p[10]);
    }
    return IVX_OK;
}

// the plan of a set: the drivers sorted stably by (body, kind, list index), the driven bodies in ascending order, per driven body its extent
struct MdPlan {
    std::vector<ivx_motion_driver> sorted;
    std::vector<uint32_t> bodies, offsets;
};
int md_build_plan(const char* who, const ivx_motion_driver* drivers, size_t n, size_t n_kin, MdPlan* plan) {
    for (size_t i = 0; i < n; ++i) {
        if (int rc = md_validate_one(who, drivers[i], i)) return rc;
        IVX_REQUIRE(drivers[i].body < n_kin, IVX_ERR_INVALID, "%s: driver %zu (%s) drives kinematic body %u, there are %zu", who, i, MD_KIND_NAMES[drivers[i].kind],
                    drivers[i].body, n_kin);
    }
    std::vector<uint32_t> order(n);
    for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        return drivers[x].body != drivers[y].body ? drivers[x].body < drivers[y].body : drivers[x].kind < drivers[y].kind;
    });
    plan->sorted.resize(n);
    plan->bodies.clear();
    plan->offsets.clear();
    for (size_t i = 0; i < n; ++i) {
        plan->sorted[i] = drivers[order[i]];
        if (i == 0 || plan->sorted[i].body != plan->sorted[i - 1].body) {
            plan->bodies.push_back(plan->sorted[i].body);
            plan->offsets.push_back((uint32_t)i);
        }
    }
    plan->offsets.push_back((uint32_t)n);
    return IVX_OK;
}

// world-owned state: one device allocation (sorted drivers | driven bodies | offsets) that only grows, the pinned block its upload goes through
struct MdState {
    ivx_buf dev;
    ivx_staging staging;
    size_t at_bodies = 0, at_offsets = 0;
    uint32_t n_driven = 0;
    uint32_t need_kin = 0;  // the body indices were checked against a world of at least this many kinematic bodies
};

}  // namespace

void ivx_md_release(ivx_world* w) {
    MdState* st = w ? ivx_state_take<MdState>(&w->md_state) : nullptr;
    if (!st) return;
    ivx_buf_free(&st->dev);
    ivx_staging_release(&st->staging);
    delete st;
}

int ivx_motion_ready(ivx_world* w, const char* who) {
    MdState* st = static_cast<MdState*>(w->md_state);
    if (!st || st->n_driven == 0) return IVX_OK;
    IVX_REQUIRE(w->n_kin >= st->need_kin, IVX_ERR_STATE, "%s: the motion drivers refer to %u kinematic bodies, the world now has %u (call ivx_world_set_motion_drivers again)", who,
                st->need_kin, w->n_kin);
    return IVX_OK;
}

int ivx_launch_motion_apply(ivx_world* w, float time, const char* who) {
    MdState* st = static_cast<MdState*>(w->md_state);
    if (!st || st->n_driven == 0) return IVX_OK;
    if (int rc = ivx_motion_ready(w, who)) return rc;
    const char* base = static_cast<const char*>(st->dev.p);
    IVX_KLAUNCH(k_motion_apply, dim3((st->n_driven + 255u) / 256u), dim3(256), 0, w->ctx->stream, reinterpret_cast<const ivx_motion_driver*>(base),
                reinterpret_cast<const uint32_t*>(base + st->at_bodies), reinterpret_cast<const uint32_t*>(base + st->at_offsets), st->n_driven, time, w->kin.p);
    IVX_HIP_CHECK(hipGetLastError());
    return IVX_OK;
}

extern "C" {

int ivx_world_set_motion_drivers(ivx_world* w, const ivx_motion_driver* drivers, size_t n) {
    const char* who = "ivx_world_set_motion_drivers";
    IVX_REQUIRE(w && (drivers || n == 0), IVX_ERR_INVALID, "%s: null argument", who);
    IVX_REQUIRE(n < (1u << 24), IVX_ERR_CAPACITY, "%s: more than 2^24 drivers", who);
    if (n == 0) {  // the set leaves (a launch in flight still reads the buffers: wait for it)
        if (w->md_state) IVX_HIP_CHECK(ivx_stream_sync(w->ctx->stream));
        ivx_md_release(w);
        return IVX_OK;
    }
    MdPlan plan;
    if (int rc = md_build_plan(who, drivers, n, w->n_kin, &plan)) return rc;
    MdState* st;
    if (int rc = ivx_state_for(&w->md_state, who, &st)) return rc;
    st->n_driven = 0;  // (until this call's set stands)
    const size_t n_driven = plan.bodies.size();
    ivx_layout l;
    const size_t at_drivers = l.take(n * sizeof(ivx_motion_driver)), at_bodies = l.take(n_driven * 4), at_offsets = l.take((n_driven + 1) * 4);
    if (int rc = ivx_buf_grow(w->ctx, &st->dev, l.bytes, 1u << 12)) return rc;
    if (int rc = ivx_staging_for(&st->staging, l.bytes)) return rc;
    char* h = static_cast<char*>(st->staging.p);
    memset(h, 0, l.bytes);
    memcpy(h + at_drivers, plan.sorted.data(), n * sizeof(ivx_motion_driver));
    memcpy(h + at_bodies, plan.bodies.data(), n_driven * 4);
    memcpy(h + at_offsets, plan.offsets.data(), (n_driven + 1) * 4);
    // (stream-ordered behind an apply that still reads the set this one replaces)
    if (int rc = ivx_staging_upload(&st->staging, st->dev.p, l.bytes, w->ctx->stream)) return rc;
    st->at_bodies = at_bodies, st->at_offsets = at_offsets;
    st->need_kin = plan.bodies.back() + 1u;
    st->n_driven = (uint32_t)n_driven;
    return IVX_OK;
}

int ivx_world_set_time(ivx_world* w, float time) {
    IVX_REQUIRE(w, IVX_ERR_INVALID, "ivx_world_set_time: null world");
    w->time = time;
    return IVX_OK;
}

int ivx_world_time(ivx_world* w, float* out) {
    IVX_REQUIRE(w && out, IVX_ERR_INVALID, "ivx_world_time: null argument");
    *out = w->time;
    return IVX_OK;
}

int ivx_world_apply_motion(ivx_world* w, float time) {
    IVX_REQUIRE(w, IVX_ERR_INVALID, "ivx_world_apply_motion: null world");
    return ivx_launch_motion_apply(w, time, "ivx_world_apply_motion");
}

int ivx_md_eval(const ivx_motion_driver* driver, float time, float out[10]) {
    IVX_REQUIRE(driver && out, IVX_ERR_INVALID, "ivx_md_eval: null argument");
    if (int rc = md_validate_one("ivx_md_eval", *driver, 0)) return rc;
    const MdOut o = md_eval(driver->kind, driver->p, time);
    for (int i = 0; i < 10; ++i) out[i] = 0.0f;
    if (driver->kind < IVX_MD_CONSTANT_ROTATION) {
        st3(out, o.a);
        st3(out + 3, o.b);
    } else {
        out[0] = o.q.x, out[1] = o.q.y, out[2] = o.q.z, out[3] = o.q.w;
        st3(out + 4, o.a);
        out[7] = o.speed;
    }
    return IVX_OK;
}

int ivx_md_apply_host(const ivx_motion_driver* drivers, size_t n, ivx_kinematic_body* bodies, size_t n_kin, float time) {
    const char* who = "ivx_md_apply_host";
    IVX_REQUIRE((drivers || n == 0) && (bodies || n_kin == 0), IVX_ERR_INVALID, "%s: null argument", who);
    MdPlan plan;
    if (int rc = md_build_plan(who, drivers, n, n_kin, &plan)) return rc;
    for (size_t i = 0; i < plan.bodies.size(); ++i) md_apply_body(bodies[plan.bodies[i]], plan.sorted.data(), plan.offsets[i], plan.offsets[i + 1], time);
    return IVX_OK;
}

}  // extern "C"
