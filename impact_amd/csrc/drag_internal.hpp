// What drag.hip (the maps) and forces.hip (the drag phase of the force stage, the world's resident maps) share: the cell index arithmetic of the
// equirectangular map — one text, host and device, so that the cell a sample is smoothed into and the cell a body looks up cannot drift apart —
// and the one internal entry that builds a map of a grid's resident mesh at a device address.
#pragma once
#include <cmath>
#include <cstdint>

#include "ivx_internal.hpp"

namespace ivx_drag {

constexpr float PI_F = 3.14159265358979323846f;
constexpr float TWO_PI_F = 6.28318530717958647692f;
constexpr uint32_t MAX_THETA = 2048;

// EquirectangularMap::compute_phi_idx / compute_theta_idx (equirectangular_map.rs:86-98), f32 as the reference; phi clamped as well (header)
__host__ __device__ __forceinline__ float rem_euclid_two_pi(float a) {
    float r = fmodf(a, TWO_PI_F);
    if (r < 0.0f) r += TWO_PI_F;
    return r;
}
__host__ __device__ __forceinline__ uint32_t clamped_idx(float angle, float inv_cell, uint32_t n) {
    const float f = floorf(angle * inv_cell);
    const uint32_t i = f > 0.0f ? (uint32_t)f : 0u;
    return i < n - 1u ? i : n - 1u;
}
__host__ __device__ __forceinline__ uint32_t phi_idx_of(float phi, float inv_cell, uint32_t n_phi) { return clamped_idx(rem_euclid_two_pi(phi), inv_cell, n_phi); }
__host__ __device__ __forceinline__ uint32_t theta_idx_of(float theta, float inv_cell, uint32_t n_theta) {
    float t = rem_euclid_two_pi(theta);
    if (t > PI_F) t = TWO_PI_F - t;
    return clamped_idx(t, inv_cell, n_theta);
}

}  // namespace ivx_drag

// drag.hip. DragLoadMap::compute_from_mesh over the grid's resident mesh, all of it enqueued on the grid's context's stream: validation (messages
// under `who`: IVX_ERR_INVALID / IVX_ERR_CAPACITY for the configuration, IVX_ERR_STATE without a current mesh), the three passes, the map — n_theta x
// 2 n_theta ivx_drag_load, theta-major — at `d_map`, a device address of the caller's. d_map null: the map goes into the context's drag scratch and
// *d_where says where (valid until the next drag call on the context). A mesh of fewer than 3 indices gives a zero map. Nothing is waited for
// beyond the upload of the directions. ivx_drag_map_check is the validation alone (a caller that sizes the destination by the configuration asks
// first); ivx_drag_map_build makes it again.
int ivx_drag_map_check(const char* who, const ivx_grid* g, const float com[3], const ivx_drag_map_config* cfg);
int ivx_drag_map_build(const char* who, ivx_grid* g, const float com[3], const ivx_drag_map_config* cfg, float* d_map, float** d_where);
