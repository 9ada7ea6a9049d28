// The f32 vector and quaternion arithmetic of the contact, collision and physics kernels, host and device, in ONE stated operation order: the
// bit-exact gates against the reference depend on these expressions as written (the files that use them are compiled without contraction).
// Each file pulls the namespace into its anonymous namespace. (sn_roles.hpp and sdf_sample.hip have vector helpers of their own under other names.)
#pragma once
#include <hip/hip_runtime.h>

namespace ivx_vec {

#define IVX_VEC_HD __host__ __device__ __forceinline__

struct V3 {
    float x, y, z;
};
struct Q4 {
    float x, y, z, w;
};
IVX_VEC_HD V3 mk(float x, float y, float z) { return {x, y, z}; }
IVX_VEC_HD V3 ld3(const float* p) { return {p[0], p[1], p[2]}; }
IVX_VEC_HD void st3(float* p, V3 v) { p[0] = v.x, p[1] = v.y, p[2] = v.z; }
IVX_VEC_HD V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
IVX_VEC_HD V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
IVX_VEC_HD V3 operator-(V3 a) { return {-a.x, -a.y, -a.z}; }
IVX_VEC_HD V3 operator*(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
IVX_VEC_HD float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
IVX_VEC_HD V3 cross(V3 a, V3 b) { return {a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }
// glam Quat::mul_vec3a
IVX_VEC_HD V3 qrot(Q4 q, V3 v) {
    const V3 b = mk(q.x, q.y, q.z);
    const float b2 = dot(b, b);
    return (v * (q.w * q.w - b2) + b * (dot(v, b) * 2.0f)) + cross(b, v) * (q.w * 2.0f);
}
IVX_VEC_HD V3 qrot(const float q[4], V3 v) {
    const V3 b = mk(q[0], q[1], q[2]);
    const float b2 = dot(b, b);
    return (v * (q[3] * q[3] - b2) + b * (dot(v, b) * 2.0f)) + cross(b, v) * (q[3] * 2.0f);
}
// glam Quat::mul_quat (xyzw)
IVX_VEC_HD Q4 qmul(Q4 a, Q4 b) {
    return {a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x,
            a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
// (the second operand wins only when strictly smaller / larger: the order of the operands matters for -0.0 and NaN)
IVX_VEC_HD float min_rs(float a, float b) { return b < a ? b : a; }
IVX_VEC_HD float max_rs(float a, float b) { return b > a ? b : a; }
// impact_math/src/random/splitmix.rs:4-10
IVX_VEC_HD unsigned long long splitmix(unsigned long long state) {
    state += 0x9E3779B97F4A7C15ull;
    unsigned long long z = state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

#undef IVX_VEC_HD

}  // namespace ivx_vec
