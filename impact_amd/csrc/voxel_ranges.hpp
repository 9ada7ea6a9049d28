// The voxels and chunks of an object that a box touches: the one host statement of the reference's voxel_ranges_touching_aab, for the edit
// unit (edit_api.hip) and the collision unit (voxel_collision_api.hip). Plain C++, no HIP runtime: tools/voxel_ranges_check.cpp compiles it
// on its own.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

// voxel_ranges_touching_aab (intersection.rs:766-782): the voxels a box in voxel units touches, clamped onto the occupied ranges; not checked for
// emptiness (the reference does not either). `as usize` stops at 0 below (NaN included); `saturate`: ... and at 2e9 above, which the edits and the
// mutual forms need for the bounds of an absorber's or an overlap's box. The collidable forms have never saturated and still do not: the two
// conversions agree for every bound below 2^31 voxels, past it the unsaturated one wraps in the int32 ranges of chunk_box where the reference
// finds nothing touched.
static inline void clamped_ranges(const uint32_t occ[12], const float lo_f[3], const float hi_f[3], bool saturate, long lo[3], long hi[3]) {
    auto index = [saturate](float f) -> long { return f > 0.0f ? (!saturate || f < 2.0e9f ? (long)f : 2000000000L) : 0; };
    for (int d = 0; d < 3; ++d) {
        lo[d] = std::max<long>((long)occ[6 + 2 * d], index(std::floor(lo_f[d])));
        hi[d] = std::min<long>((long)occ[7 + 2 * d], index(std::ceil(hi_f[d])));
    }
}
// the voxel ranges as the kernels take them and the box of chunks that holds them (meaningless when a range is empty: false)
static inline bool chunk_box(const long rlo[3], const long rhi[3], int32_t vlo[3], int32_t vhi[3], uint32_t lo[3], uint32_t cc[3]) {
    bool any = true;
    for (int d = 0; d < 3; ++d) {
        vlo[d] = (int32_t)rlo[d];
        vhi[d] = (int32_t)rhi[d];
        any = any && vlo[d] < vhi[d];
        lo[d] = (uint32_t)vlo[d] / 16u;
        cc[d] = ((uint32_t)vhi[d] + 15u) / 16u - lo[d];
    }
    return any;
}
