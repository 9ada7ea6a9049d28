// What bvol.hip shares with narrow.hip: the world box derivation both files run on the host and on the device, and the two halves of the
// bounding-volume calls that narrow.hip drives with inputs that are on the device already.
#pragma once
#include "ivx_internal.hpp"

__host__ __device__ __forceinline__ float ivx_bv_abs(float v) { return __builtin_fabsf(v); }  // (clears the sign bit)

// ivx_bv_world_aabb (include/impact_voxel_hip.h states the operation order)
__host__ __device__ inline void ivx_bv_world_aabb_of(const ivx_aabb& m, const ivx_similarity& s, ivx_aabb* out) {
    const float c[3] = {0.5f * (m.lower[0] + m.upper[0]), 0.5f * (m.lower[1] + m.upper[1]), 0.5f * (m.lower[2] + m.upper[2])};
    const float h[3] = {0.5f * (m.upper[0] - m.lower[0]), 0.5f * (m.upper[1] - m.lower[1]), 0.5f * (m.upper[2] - m.lower[2])};
    const float x = s.rotation[0], y = s.rotation[1], z = s.rotation[2], w = s.rotation[3];
    const float xx = x * x, yy = y * y, zz = z * z, ww = w * w;
    const float n2 = ((xx + yy) + zz) + ww;
    const float xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    const float N[3][3] = {{((ww + xx) - yy) - zz, 2.0f * (xy - wz), 2.0f * (xz + wy)},
                           {2.0f * (xy + wz), ((ww - xx) + yy) - zz, 2.0f * (yz - wx)},
                           {2.0f * (xz - wy), 2.0f * (yz + wx), ((ww - xx) - yy) + zz}};
    for (int i = 0; i < 3; ++i) {
        const float m0 = s.scaling * (N[i][0] / n2), m1 = s.scaling * (N[i][1] / n2), m2 = s.scaling * (N[i][2] / n2);
        const float ct = ((m0 * c[0] + m1 * c[1]) + m2 * c[2]) + s.translation[i];
        const float ht = (ivx_bv_abs(m0) * h[0] + ivx_bv_abs(m1) * h[1]) + ivx_bv_abs(m2) * h[2];
        out->lower[i] = ct - ht;
        out->upper[i] = ct + ht;
    }
}

// A set of n world boxes whose inputs a kernel of the caller writes on the context's stream, no host copy involved:
//   begin:  lays the context's set buffer out for n objects (the context holds no set until `finish`) and hands out where the boxes (n, world
//           space) and the kinds (whole blocks of 64: ceil(n / 64) x 64 words, the ones behind n zero) are to be written; n == 0: both null
//   finish: the launches of ivx_bv_set behind that kernel (boxes stored as given, block boxes, total); the set stands
int ivx_bvol_set_begin(ivx_ctx* c, size_t n, ivx_aabb** d_boxes, uint32_t** d_kinds);
int ivx_bvol_set_finish(ivx_ctx* c, size_t n);
// which of the sets the context has held stands now (from 1; 0: none): whoever installed a set can tell whether it is still the one
uint64_t ivx_bvol_set_serial(const ivx_ctx* c);
// The pair pass of ivx_bv_pairs over the context's set, up to and including the emit launch into the context's pair buffer (ivx_bv_device_ptr):
// waits once, for the grand total (*n_pairs, set before any refusal). check_cap: refuse (IVX_ERR_CAPACITY, nothing emitted) when it exceeds cap.
int ivx_bvol_pairs_enqueue(ivx_ctx* c, const char* who, uint32_t mode, bool check_cap, size_t cap, size_t* n_pairs);
