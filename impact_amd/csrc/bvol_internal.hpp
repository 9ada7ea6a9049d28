// What bvol.hip, bvh.hip and narrow.hip share: the world box derivation run on the host and on the device, the hierarchy's rules as functions
// its host call and its kernels both run, and the halves of the bounding-volume calls that narrow.hip drives with inputs that are on the
// device already.
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

// ---- the hierarchy (bvh.hip): what its host function and its kernels both run, so that both leave the same bytes ----------------------------
// (include/impact_voxel_hip.h states the rules: frame, key, leaves, nodes)
__host__ __device__ __forceinline__ uint32_t ivx_bv_bits(float v) { return __builtin_bit_cast(uint32_t, v); }
// the bit pattern of a float as a signed integer that orders like the float, with -0.0 below +0.0 (bvol.hip's order of the block boxes)
__host__ __device__ __forceinline__ int32_t ivx_bv_order_key(float v) {
    const int32_t b = (int32_t)ivx_bv_bits(v);
    return b < 0 ? (int32_t)((uint32_t)b ^ 0x7FFFFFFFu) : b;
}
__host__ __device__ __forceinline__ float ivx_bv_order_min(float a, float b) { return ivx_bv_order_key(b) < ivx_bv_order_key(a) ? b : a; }
__host__ __device__ __forceinline__ float ivx_bv_order_max(float a, float b) { return ivx_bv_order_key(b) > ivx_bv_order_key(a) ? b : a; }
__host__ __device__ __forceinline__ void ivx_bv_union(ivx_aabb* into, const ivx_aabb& b) {
    for (int k = 0; k < 3; ++k) into->lower[k] = ivx_bv_order_min(into->lower[k], b.lower[k]), into->upper[k] = ivx_bv_order_max(into->upper[k], b.upper[k]);
}
__host__ __device__ __forceinline__ ivx_aabb ivx_bv_neutral_box() {
    ivx_aabb b;
    for (int k = 0; k < 3; ++k) b.lower[k] = __builtin_inff(), b.upper[k] = -__builtin_inff();
    return b;
}
__host__ __device__ __forceinline__ bool ivx_bv_has_nan(const ivx_aabb& b) {
    bool nan = false;
    for (int k = 0; k < 3; ++k) nan = nan || b.lower[k] != b.lower[k] || b.upper[k] != b.upper[k];
    return nan;
}
// box_lies_outside, the header's box decision: a difference with its sign bit set, or a NaN one (bvol.hip's pair walk decides the same way)
__host__ __device__ __forceinline__ bool ivx_bv_lies_outside(const ivx_aabb& self, const ivx_aabb& other) {
    uint32_t bits = 0u;
    bool nan = false;
    for (int k = 0; k < 3; ++k) {
        const float d0 = other.upper[k] - self.lower[k], d1 = self.upper[k] - other.lower[k];
        bits |= ivx_bv_bits(d0) | ivx_bv_bits(d1);
        nan = nan || d0 != d0 || d1 != d1;
    }
    return (bits >> 31) != 0u || nan;
}
// a NaN bound, or a bound of magnitude 1e30f or more: the box stays out of the frame and takes the last code
__host__ __device__ __forceinline__ bool ivx_bv_unkeyed(const ivx_aabb& b) {
    bool out = ivx_bv_has_nan(b);
    for (int k = 0; k < 3; ++k) out = out || ivx_bv_abs(b.lower[k]) >= 1e30f || ivx_bv_abs(b.upper[k]) >= 1e30f;
    return out;
}
// the frame of no box at all (the union's neutral element came through): the all-zero box
__host__ __device__ __forceinline__ void ivx_bv_frame_finish(ivx_aabb* f) {
    if (ivx_bv_order_key(f->lower[0]) > ivx_bv_order_key(f->upper[0]))
        for (int k = 0; k < 3; ++k) f->lower[k] = 0.0f, f->upper[k] = 0.0f;
}
__host__ __device__ __forceinline__ uint32_t ivx_bv_spread3(uint32_t q) {  // bit k of a 10-bit value to bit 3 k
    uint32_t r = 0u;
    for (int k = 0; k < 10; ++k) r |= ((q >> k) & 1u) << (3 * k);
    return r;
}
__host__ __device__ __forceinline__ uint64_t ivx_bv_key_of(const ivx_aabb& frame, const ivx_aabb& box, uint32_t index) {
    uint32_t code = 0x3FFFFFFFu;
    if (!ivx_bv_unkeyed(box)) {
        uint32_t q[3];
        for (int k = 0; k < 3; ++k) {
            const float c = 0.5f * (box.lower[k] + box.upper[k]);
            const float t = (c - frame.lower[k]) / (frame.upper[k] - frame.lower[k]);
            q[k] = !(t > 0.0f) ? 0u : (t < 1.0f ? (uint32_t)(t * 1024.0f) : 1023u);
        }
        code = (ivx_bv_spread3(q[0]) << 2) | (ivx_bv_spread3(q[1]) << 1) | ivx_bv_spread3(q[2]);
    }
    return ((uint64_t)code << 32) | index;
}
// Karras's delta: the length of the common prefix of keys i and j, -1 when j lies past either end (the keys are unique)
__host__ __device__ __forceinline__ int ivx_bv_delta(const uint64_t* keys, int n, int i, int j) {
    if (j < 0 || j >= n) return -1;
    return __builtin_clzll(keys[i] ^ keys[j]);
}
// Karras's node i of n sorted keys (0 <= i <= n - 2): its leaf range [first, last] and its two children as IVX_BV_LEAF | position or a node index.
// Every loop is bounded by the 21 doublings n <= 2^20 allows.
__host__ __device__ inline void ivx_bv_karras(const uint64_t* keys, int n, int i, uint32_t* left, uint32_t* right, uint32_t* first, uint32_t* last) {
    const int d = ivx_bv_delta(keys, n, i, i + 1) - ivx_bv_delta(keys, n, i, i - 1) < 0 ? -1 : 1;
    const int dmin = ivx_bv_delta(keys, n, i, i - d);
    int lmax = 2;
    for (int k = 0; k < 24 && ivx_bv_delta(keys, n, i, i + lmax * d) > dmin; ++k) lmax *= 2;
    int l = 0;
    for (int t = lmax / 2; t >= 1; t /= 2)
        if (ivx_bv_delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = ivx_bv_delta(keys, n, i, j);
    int s = 0;
    for (int t = (l + 1) / 2, k = 0; k < 24; t = (t + 1) / 2, ++k) {
        if (ivx_bv_delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
        if (t <= 1) break;
    }
    const int split = i + s * d + (d < 0 ? -1 : 0);
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    *left = lo == split ? (IVX_BV_LEAF | (uint32_t)split) : (uint32_t)split;
    *right = hi == split + 1 ? (IVX_BV_LEAF | (uint32_t)(split + 1)) : (uint32_t)(split + 1);
    *first = (uint32_t)lo, *last = (uint32_t)hi;
}

// ---- region queries: the leaf decision (bvol.hip's flat kernel, bvh.hip's walk and both host forms run it) and the hierarchy's node decisions ------
// "has its sign bit set, or is a NaN" for any of six differences
__host__ __device__ __forceinline__ bool ivx_bv_any_negative(float d0, float d1, float d2, float d3, float d4, float d5) {
    const uint32_t bits = ((ivx_bv_bits(d0) | ivx_bv_bits(d1)) | (ivx_bv_bits(d2) | ivx_bv_bits(d3))) | (ivx_bv_bits(d4) | ivx_bv_bits(d5));
    const bool nan = __builtin_isunordered(d0, d1) || __builtin_isunordered(d2, d3) || __builtin_isunordered(d4, d5);
    return (bits >> 31) != 0u || nan;
}
// c and h of a world box, as ivx_bv_world_aabb takes them of a model box
__host__ __device__ __forceinline__ void ivx_bv_center_half(const ivx_aabb& b, float c[3], float h[3]) {
    for (int k = 0; k < 3; ++k) c[k] = 0.5f * (b.lower[k] + b.upper[k]), h[k] = 0.5f * (b.upper[k] - b.lower[k]);
}
// the four decisions of include/impact_voxel_hip.h over one world box b (c, h: ivx_bv_center_half of b)
__host__ __device__ __forceinline__ bool ivx_bv_query_hits(const ivx_bv_query* __restrict__ q, const ivx_aabb& b, const float c[3], const float h[3]) {
    switch (q->kind) {  // (uniform)
        case IVX_BV_QUERY_BOX:  // box_lies_outside, self = the query
            return !ivx_bv_any_negative(b.upper[0] - q->u.box.lower[0], b.upper[1] - q->u.box.lower[1], b.upper[2] - q->u.box.lower[2], q->u.box.upper[0] - b.lower[0],
                                        q->u.box.upper[1] - b.lower[1], q->u.box.upper[2] - b.lower[2]);
        case IVX_BV_QUERY_SPHERE: {
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float ck = q->u.sphere.center[k];
                if (b.upper[k] < ck) {
                    const float d = ck - b.upper[k];
                    s += d * d;
                } else if (b.lower[k] > ck) {
                    const float d = b.lower[k] - ck;
                    s += d * d;
                }
            }
            return !(s > q->u.sphere.radius * q->u.sphere.radius);
        }
        case IVX_BV_QUERY_FRUSTUM: {
            bool hit = true;
#pragma unroll
            for (int p = 0; p < 6; ++p) {
                const uint32_t corner = q->u.frustum.corners[p];
                const float px = (corner & 4u) ? b.upper[0] : b.lower[0], py = (corner & 2u) ? b.upper[1] : b.lower[1], pz = (corner & 1u) ? b.upper[2] : b.lower[2];
                const float dist = ((q->u.frustum.planes[p][0] * px + q->u.frustum.planes[p][1] * py) + q->u.frustum.planes[p][2] * pz) - q->u.frustum.planes[p][3];
                hit = hit && dist >= 0.0f;
            }
            return hit;
        }
        default: {  // IVX_BV_QUERY_ORIENTED_BOX
            const float dx = c[0] - q->u.oriented_box.center[0], dy = c[1] - q->u.oriented_box.center[1], dz = c[2] - q->u.oriented_box.center[2];
            float diff[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float a0 = q->u.oriented_box.axes[a][0], a1 = q->u.oriented_box.axes[a][1], a2 = q->u.oriented_box.axes[a][2];
                const float e = ((ivx_bv_abs(a0) * h[0] + ivx_bv_abs(a1) * h[1]) + ivx_bv_abs(a2) * h[2]) + q->u.oriented_box.half_extents[a];
                const float l = (a0 * dx + a1 * dy) + a2 * dz;
                diff[a] = e - ivx_bv_abs(l);
            }
            return !ivx_bv_any_negative(diff[0], diff[1], diff[2], 0.0f, 0.0f, 0.0f);
        }
    }
}
// An IRREGULAR box: a NaN bound, or lower > upper on an axis (a set stored as given may hold one; the neutral leaf box of a NaN-bounded object is
// one). The node decisions below are sound for PROPER boxes only — lower <= upper on every axis — so the walk leaves irregular objects alone
// and every query decides them with the leaf decision, outside the walk.
__host__ __device__ __forceinline__ bool ivx_bv_irregular(const ivx_aabb& b) {
    bool r = false;
    for (int k = 0; k < 3; ++k) r = r || !(b.lower[k] <= b.upper[k]);
    return r;
}
// The node decision: true only when NO proper box inside `nb` (lower >= nb.lower, upper <= nb.upper per component, which the union in the bit
// order gives every leaf under a node) can be hit by ivx_bv_query_hits in f32. DESIGN.md section 4 gives the argument per kind; in short:
//   box      box_lies_outside on the node box: each difference is monotone in the bound it takes, the sign-bit and NaN cases included.
//   sphere   the leaf expression on the node box: per axis the node adds a term only where every leaf inside adds a larger one, and subtraction,
//            squaring of a non-negative and the running sum are monotone in f32. A NaN compares false: entered.
//   frustum  NOT the leaf expression (corners[] is caller data, and an unbounded member makes inf - inf): per plane and axis the larger of
//            n lower and n upper, summed in the leaf's order, minus d; skipped only when that is < 0. A NaN anywhere: entered.
//   oriented e - |l| is not monotone under f32 rounding, so the node is evaluated in f64 and skipped only when |l| - e exceeds a margin that bounds
//            the f32 error of the leaf expression for any proper box inside (IVX_BV_OBB_MARGIN_ULPS x 2^-24 x the magnitudes that enter it, plus a
//            floor for underflow); magnitudes near the f32 range, or a NaN: entered.
#define IVX_BV_OBB_MARGIN_ULPS 16.0
__host__ __device__ inline bool ivx_bv_query_skips_node(const ivx_bv_query* __restrict__ q, const ivx_aabb& nb) {
    switch (q->kind) {  // (uniform)
        case IVX_BV_QUERY_BOX: {
            ivx_aabb self;
            for (int k = 0; k < 3; ++k) self.lower[k] = q->u.box.lower[k], self.upper[k] = q->u.box.upper[k];
            return ivx_bv_lies_outside(self, nb);
        }
        case IVX_BV_QUERY_SPHERE: {
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float ck = q->u.sphere.center[k];
                if (nb.upper[k] < ck) {
                    const float d = ck - nb.upper[k];
                    s += d * d;
                } else if (nb.lower[k] > ck) {
                    const float d = nb.lower[k] - ck;
                    s += d * d;
                }
            }
            return s > q->u.sphere.radius * q->u.sphere.radius;
        }
        case IVX_BV_QUERY_FRUSTUM: {
            bool skip = false;
#pragma unroll
            for (int p = 0; p < 6; ++p) {
                float m[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float lo = q->u.frustum.planes[p][k] * nb.lower[k], hi = q->u.frustum.planes[p][k] * nb.upper[k];
                    m[k] = lo > hi ? lo : hi;  // (hi when either is a NaN ...
                    if (lo != lo) m[k] = lo;   //  ... so a NaN lo is put back: a NaN on either side stays one)
                }
                const float dist = ((m[0] + m[1]) + m[2]) - q->u.frustum.planes[p][3];
                skip = skip || dist < 0.0f;
            }
            return skip;
        }
        default: {  // IVX_BV_QUERY_ORIENTED_BOX
            const double u24 = 5.9604644775390625e-08;  // 2^-24, the unit roundoff of f32
            double D[3], M[3], H[3], dc[3], reach = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double lo = (double)nb.lower[k], hi = (double)nb.upper[k], ck = (double)q->u.oriented_box.center[k];
                H[k] = 0.5 * (hi - lo), dc[k] = 0.5 * (lo + hi) - ck;
                M[k] = __builtin_fmax(__builtin_fabs(lo), __builtin_fabs(hi));
                D[k] = __builtin_fabs(dc[k]) + H[k];
                reach = __builtin_fmax(reach, M[k] + __builtin_fabs(ck));  // (fmax drops a NaN; `scale` below keeps it, through D)
            }
            bool skip = false;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double a0 = (double)q->u.oriented_box.axes[a][0], a1 = (double)q->u.oriented_box.axes[a][1], a2 = (double)q->u.oriented_box.axes[a][2];
                const double b0 = __builtin_fabs(a0), b1 = __builtin_fabs(a1), b2 = __builtin_fabs(a2), half = (double)q->u.oriented_box.half_extents[a];
                const double e = ((b0 * H[0] + b1 * H[1]) + b2 * H[2]) + half;
                const double l = (a0 * dc[0] + a1 * dc[1]) + a2 * dc[2];
                // what the f32 leaf expression's intermediates are bounded by, and its error in units of 2^-24 of
                const double scale = ((b0 * (D[0] + M[0]) + b1 * (D[1] + M[1])) + b2 * (D[2] + M[2])) + __builtin_fabs(half);
                // the floor: 2^-126 a product or a halving may lose when f32 results are flushed (2^-150 when they are not), the halving's times |A|
                const double margin = IVX_BV_OBB_MARGIN_ULPS * (u24 * scale + ((b0 + b1) + b2 + 1.0) * 1.1754943508222875e-38);
                const bool in_range = scale < 0x1p+120 && reach < 0x1p+120;  // (no f32 intermediate overflows; false for a NaN)
                skip = skip || (in_range && __builtin_fabs(l) - e > margin);
            }
            return skip;
        }
    }
}

// What bvh.hip takes from the context's set (bvol.hip owns it): the resident world boxes and kinds, the set's serial, the pair buffer both pair
// passes leave their result in, and the slot that holds the hierarchy's own state (freed through ivx_bvh_release when the set's state goes).
struct ivx_bvol_view {
    const ivx_aabb* world = nullptr;
    const uint32_t* kinds = nullptr;
    uint32_t n = 0;
    uint64_t serial = 0;
    ivx_buf* pairs = nullptr;
    void** hierarchy = nullptr;
    const unsigned long long* masks = nullptr;  // the resident masks of the last queries call on this set (either form), n_queried rows; ...
    uint32_t n_queried = 0;                     // ... 0: no queries call has left any since the set
};
int ivx_bvol_view_of(ivx_ctx* c, const char* who, ivx_bvol_view* out);  // IVX_ERR_STATE without a set
void ivx_bvh_release(void** hierarchy);  // (the slot: empty afterwards)
void* ivx_bvh_device_ptr(void* hierarchy, uint64_t set_serial, int which);  // IVX_BV_PTR_NODES / _LEAF_OBJECTS
// ivx_bv_build_hierarchy and the pair pass of ivx_bv_pairs_hierarchy, with ivx_bvol_pairs_enqueue's contract (narrow.hip drives both)
int ivx_bvh_build_enqueue(ivx_ctx* c, const char* who);
int ivx_bvh_pairs_enqueue(ivx_ctx* c, const char* who, uint32_t mode, bool check_cap, size_t cap, size_t* n_pairs);

// ivx_bv_queries in two halves, with whoever fills the masks in between (bvol.hip's flat kernel; bvh.hip's walk):
//   begin:  the flat call's refusals (who names the caller), then the records uploaded, the mask buffer grown. run->n_queries == 0 or run->n == 0:
//           nothing is on the device and `finish` only fills the counts with zeros.
//   finish: k_bv_query_counts, the download of masks and counts, the call's one wait; remembers the call for ivx_bv_query_lists.
struct ivx_bvol_query_run {
    const ivx_bv_query* d_queries = nullptr;
    unsigned long long* d_masks = nullptr;
    uint32_t* d_counts = nullptr;
    uint32_t n = 0, n_words = 0, n_queries = 0;
    size_t mask_bytes = 0;
};
int ivx_bvol_query_kinds_check(const char* who, const ivx_bv_query* queries, size_t n);  // every kind is one of the four (IVX_ERR_INVALID names the first that is not)
int ivx_bvol_queries_check(const char* who, ivx_ctx* c, const ivx_bv_query* queries, size_t n_queries);
int ivx_bvol_queries_begin(ivx_ctx* c, const char* who, const ivx_bv_query* queries, size_t n_queries, uint64_t* masks, ivx_bvol_query_run* run);
int ivx_bvol_queries_finish(ivx_ctx* c, const ivx_bvol_query_run& run, uint64_t* masks, uint32_t* counts);

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
// What ivx_bv_pairs and ivx_bv_pairs_hierarchy refuse before they look at the set (*n_out is zero afterwards), and what both pair passes refuse once
// the grand total is known: 2^31 pairs or more, then (*n_pairs set) a total beyond the caller's buffer.
int ivx_bvol_pairs_check(const char* who, ivx_ctx* c, uint32_t mode, const uint32_t* pairs, size_t cap, size_t* n_out);
int ivx_bvol_pairs_total(const char* who, unsigned long long grand, bool check_cap, size_t cap, size_t* n_pairs);
