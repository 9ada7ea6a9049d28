// Frame instances: for every view of a pass, which objects of the context's bounding-volume set it keeps, their model-to-view transforms, the
// ivx_cull_pair of every (view, object), and the reductions over the kept set that the light geometry needs.
//
// Reference: BufferModelInstancesAndBoundLights (engine/src/tasks.rs:779) = impact_scene/src/model.rs:171-297 (buffer_model_instances_for_rendering)
//   and impact_scene/src/light.rs:85-284, 383-450, 465-641, 747-787, 827-848 (the omnidirectional and unidirectional shadow passes),
//   impact_geometry/src/axis_aligned_box.rs:208-239 (closest_interior_point_to, farthest_corner_from), :350-363 (aabb_of_transformed),
//   impact_math/src/transform/similarity.rs:278-284 (Similarity3 x Similarity3). The reference loops per view over the hits of a query on the
//   host; include/impact_voxel_hip.h states the kept-set rule, the reductions and every operation order.
//
// DECIDE — k_fi_decide, a workgroup per reduction tile of TILE = 256 consecutive objects and group of VIEW_GROUP = 8 consecutive views, a wave per
//   64 of the objects, an object per lane (its world box, flags and entity in registers). The wave walks the group's views: the view record, the
//   mask word and the previous call's kept word have wave-uniform addresses (scalar loads); fi_keeps is the very function the host form runs; __ballot is the kept word of (view, 64 objects), its popcount goes
//   to the prefix array. A wave that keeps something reduces its 14 values (world box, view box, the two distances) by xor shuffles in the bit
//   order, leaves them in LDS, and after the walk the workgroup merges its four waves per (view, value): partials[view][tile].
// VIEW — k_fi_view, a workgroup per view: the exclusive prefix of the view's kept-word popcounts in place (ivx_scan_rounds; the total is the
//   count), and the final pass over the view's partials: strided, xor shuffles, LDS across the waves. The result record.
// OFFSETS — k_fi_offsets, one workgroup: the exclusive prefix of the counts, offsets[n_views + 1].
// EMIT — k_fi_emit, a lane per (view, object) pair in view-major order, EMIT_BLOCK = 256 pairs a workgroup: a kept lane composes its similarity
//   (fi_compose, the host's function), takes its rank from the word's prefix and the set bits below it, and writes its list entry; every lane
//   lays its 40-byte pair down in LDS and the workgroup stores the 10 240 bytes as consecutive 8-byte words, whoever made them.
// No atomic anywhere: two calls leave the same bytes. Every minimum and maximum is taken in the total order of the bit patterns
// (ivx_bv_order_min / _max, bvol_internal.hpp), so no result depends on the partition above.
#include <cmath>
#include <vector>

#include "bvol_internal.hpp"
#include "device_common.hpp"
#include "instances_internal.hpp"
#include "vec3.hpp"

namespace {
using namespace ivx_vec;

constexpr uint32_t MAX_VIEWS = IVX_FI_MAX_VIEWS;
constexpr uint32_t TILE = 256;         // objects per workgroup of k_fi_decide: the reduction tile
constexpr uint32_t VIEW_GROUP = 8;     // views per workgroup of k_fi_decide (blockIdx.y): 64 views over a few hundred tiles still fill the chip
constexpr uint32_t EMIT_BLOCK = 256;   // pairs per workgroup of k_fi_emit
constexpr uint32_t SCAN_ROUND = 1024;  // kept words per round of k_fi_view's prefix (its workgroup)
constexpr uint32_t N_VALUES = 14;      // world lower 0-2, world upper 3-5, view lower 6-8, view upper 9-11, min d_close 12, max d_far 13
static_assert(sizeof(ivx_fi_instance) == 48 && sizeof(ivx_fi_view) == 72 && sizeof(ivx_fi_view_result) == 60 && sizeof(ivx_cull_pair) == 40, "record sizes of the header");
static_assert(sizeof(ivx_fi_view_result) == 4 * (1 + N_VALUES), "the result record is the count and the 14 values");

// ---- shared host / device arithmetic (f32, the header's operation order; the file is compiled without contraction) ---------------------------
__host__ __device__ __forceinline__ bool value_is_min(uint32_t f) { return f < 3u || (f >= 6u && f < 9u) || f == 12u; }
__host__ __device__ __forceinline__ float value_neutral(uint32_t f) { return value_is_min(f) ? __builtin_inff() : -__builtin_inff(); }
__host__ __device__ __forceinline__ float value_merge(uint32_t f, float a, float b) { return value_is_min(f) ? ivx_bv_order_min(a, b) : ivx_bv_order_max(a, b); }

// d_close and d_far of the header
__host__ __device__ __forceinline__ void fi_distances(const ivx_aabb& b, const float p[3], float* d_close, float* d_far) {
    float e[3], g[3];
    for (int k = 0; k < 3; ++k) {
        float c = b.lower[k] > p[k] ? b.lower[k] : p[k];
        c = b.upper[k] < c ? b.upper[k] : c;
        e[k] = p[k] - c;
        const float m = 0.5f * (b.lower[k] + b.upper[k]);
        const float f = p[k] > m ? b.lower[k] : b.upper[k];
        g[k] = p[k] - f;
    }
    *d_close = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
    *d_far = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
}
// the kept-set rule. `hit`: the object's bit of the view's mask row; `and_ok`: no and_view, or the object's bit of that kept row. Leaves the
// object's 14 values (neutral where the view does not ask for them) when it is kept.
__host__ __device__ inline bool fi_keeps(const ivx_aabb& b, uint32_t flags, uint32_t entity, bool hit, bool and_ok, const ivx_fi_view& v, float vals[N_VALUES]) {
    if (!hit || !and_ok || (flags & v.reject_flags) != 0u || entity == v.exclude_entity || ivx_bv_has_nan(b)) return false;
    float d_close = __builtin_inff(), d_far = -__builtin_inff();
    if (v.flags & IVX_FI_VIEW_REACH) {
        fi_distances(b, v.point, &d_close, &d_far);
        if (d_close > v.squared_reach) return false;
    }
    ivx_aabb vb = ivx_bv_neutral_box();
    if (v.flags & IVX_FI_VIEW_BOX) ivx_bv_world_aabb_of(b, v.world_to_view, &vb);
    for (int k = 0; k < 3; ++k) vals[k] = b.lower[k], vals[3 + k] = b.upper[k], vals[6 + k] = vb.lower[k], vals[9 + k] = vb.upper[k];
    vals[12] = d_close, vals[13] = d_far;
    return true;
}
// world_to_view * model_to_world (Similarity3 x Similarity3)
__host__ __device__ __forceinline__ ivx_similarity fi_compose(const ivx_similarity& a, const ivx_similarity& b) {
    ivx_similarity out;
    const V3 u = mk(a.scaling * b.translation[0], a.scaling * b.translation[1], a.scaling * b.translation[2]);
    st3(out.translation, qrot(a.rotation, u) + ld3(a.translation));
    const Q4 q = qmul(Q4{a.rotation[0], a.rotation[1], a.rotation[2], a.rotation[3]}, Q4{b.rotation[0], b.rotation[1], b.rotation[2], b.rotation[3]});
    out.rotation[0] = q.x, out.rotation[1] = q.y, out.rotation[2] = q.z, out.rotation[3] = q.w;
    out.scaling = a.scaling * b.scaling;
    return out;
}
__host__ __device__ __forceinline__ ivx_cull_pair fi_pair(const ivx_similarity& s, uint32_t instance_idx, uint32_t flags) {
    ivx_cull_pair p;
    for (int k = 0; k < 4; ++k) p.rotation[k] = s.rotation[k];
    for (int k = 0; k < 3; ++k) p.translation[k] = s.translation[k];
    p.scaling = s.scaling, p.instance_idx = instance_idx, p.flags = flags;
    return p;
}
__host__ __device__ __forceinline__ ivx_cull_pair fi_skip_pair() {
    ivx_similarity id;
    id.rotation[0] = id.rotation[1] = id.rotation[2] = 0.0f, id.rotation[3] = 1.0f;
    id.translation[0] = id.translation[1] = id.translation[2] = 0.0f, id.scaling = 1.0f;
    return fi_pair(id, 0u, IVX_CULL_PAIR_SKIP);
}
__host__ __device__ __forceinline__ void fi_store_result(ivx_fi_view_result* r, uint32_t count, const float vals[N_VALUES]) {
    r->count = count;
    for (int k = 0; k < 3; ++k) r->world_box.lower[k] = vals[k], r->world_box.upper[k] = vals[3 + k], r->view_box.lower[k] = vals[6 + k], r->view_box.upper[k] = vals[9 + k];
    r->min_squared_distance = vals[12], r->max_squared_distance = vals[13];
}

// ---- device side -------------------------------------------------------------------------------------------------------------------------
// lane l with lane l ^ d, d = 1, 2, .. 32: every lane ends with the wave's value
__device__ __forceinline__ void wave_merge(float vals[N_VALUES]) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
#pragma unroll
        for (uint32_t f = 0; f < N_VALUES; ++f) vals[f] = value_merge(f, vals[f], __shfl_xor(vals[f], d, 64));
}

// kept: [n_views][W]; prefix: [n_views][W], the popcounts; partials: [n_views][n_tiles][N_VALUES]. prev_kept: [.][W] of the call before (null: none)
__global__ __launch_bounds__(TILE) void k_fi_decide(const ivx_aabb* __restrict__ world, const ivx_fi_instance* __restrict__ inst, uint32_t n, uint32_t n_words,
                                                    const unsigned long long* __restrict__ masks, const unsigned long long* __restrict__ prev_kept,
                                                    const ivx_fi_view* __restrict__ views, uint32_t n_views, unsigned long long* __restrict__ kept,
                                                    uint32_t* __restrict__ prefix, float* __restrict__ partials, uint32_t n_tiles) {
    __shared__ float s_part[VIEW_GROUP][TILE / 64u][N_VALUES];
    const uint32_t v_first = blockIdx.y * VIEW_GROUP, v_end = min(n_views, v_first + VIEW_GROUP);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t word = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (TILE / 64u) + wave));
    const bool in_range = word < n_words;  // (a tile's last waves may lie past the set: they keep nothing and still meet the barrier)
    const uint32_t o = word * 64u + lane;
    const bool live = in_range && o < n;
    ivx_aabb b = ivx_bv_neutral_box();
    uint32_t flags = 0u, entity = 0u;
    if (live) b = world[o], flags = inst[o].flags, entity = inst[o].entity;
    for (uint32_t v = v_first; v < v_end; ++v) {
        const ivx_fi_view& vw = views[v];  // (uniform address)
        unsigned long long hits = 0ull, also = ~0ull;
        if (in_range) {
            hits = masks[(size_t)vw.query * n_words + word];
            if (vw.and_view != IVX_FI_NONE) also = prev_kept[(size_t)vw.and_view * n_words + word];
        }
        float vals[N_VALUES];
#pragma unroll
        for (uint32_t f = 0; f < N_VALUES; ++f) vals[f] = value_neutral(f);
        const bool keep = live && fi_keeps(b, flags, entity, ((hits >> lane) & 1ull) != 0ull, ((also >> lane) & 1ull) != 0ull, vw, vals);
        const unsigned long long kmask = __ballot(keep);
        if (in_range && lane == 0u) kept[(size_t)v * n_words + word] = kmask, prefix[(size_t)v * n_words + word] = (uint32_t)__popcll(kmask);
        if (kmask != 0ull) wave_merge(vals);  // (uniform; a wave that keeps nothing holds the neutral values already)
        if (lane == 0u)
#pragma unroll
            for (uint32_t f = 0; f < N_VALUES; ++f) s_part[v - v_first][wave][f] = vals[f];
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < (v_end - v_first) * N_VALUES; i += TILE) {
        const uint32_t g = i / N_VALUES, f = i - g * N_VALUES;
        float r = s_part[g][0][f];
        for (uint32_t w = 1; w < TILE / 64u; ++w) r = value_merge(f, r, s_part[g][w][f]);
        partials[((size_t)(v_first + g) * n_tiles + blockIdx.x) * N_VALUES + f] = r;
    }
}

__global__ __launch_bounds__(SCAN_ROUND) void k_fi_view(uint32_t* __restrict__ prefix, uint32_t n_words, const float* __restrict__ partials, uint32_t n_tiles,
                                                        ivx_fi_view_result* __restrict__ results) {
    __shared__ uint32_t wave_totals[SCAN_ROUND / 64u];
    __shared__ float s_red[SCAN_ROUND / 64u][N_VALUES];
    const uint32_t v = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t* row = prefix + (size_t)v * n_words;
    const uint32_t count = ivx_scan_rounds<SCAN_ROUND, uint32_t>(row, row, n_words, wave_totals);  // (at most 2^20 objects a view)
    float vals[N_VALUES];
#pragma unroll
    for (uint32_t f = 0; f < N_VALUES; ++f) vals[f] = value_neutral(f);
    for (uint32_t t = threadIdx.x; t < n_tiles; t += SCAN_ROUND) {
        const float* __restrict__ p = partials + ((size_t)v * n_tiles + t) * N_VALUES;
#pragma unroll
        for (uint32_t f = 0; f < N_VALUES; ++f) vals[f] = value_merge(f, vals[f], p[f]);
    }
    wave_merge(vals);
    if (lane == 0u)
#pragma unroll
        for (uint32_t f = 0; f < N_VALUES; ++f) s_red[wave][f] = vals[f];
    __syncthreads();
    if (threadIdx.x < N_VALUES) {
        const uint32_t f = threadIdx.x;
        float r = s_red[0][f];
        for (uint32_t w = 1; w < SCAN_ROUND / 64u; ++w) r = value_merge(f, r, s_red[w][f]);
        reinterpret_cast<float*>(results + v)[1u + f] = r;  // (the record is the count and the 14 values, in this order)
    }
    if (threadIdx.x == 0u) results[v].count = count;
}

// offsets[n_views + 1] (at most 64 views of at most 2^20 objects: no 32-bit sum overflows)
__global__ __launch_bounds__(64) void k_fi_offsets(const ivx_fi_view_result* __restrict__ results, uint32_t n_views, uint32_t* __restrict__ offsets) {
    const uint32_t lane = threadIdx.x;
    const uint32_t c = lane < n_views ? results[lane].count : 0u;
    const uint32_t incl = ivx_wave_incl_scan(c);
    if (lane < n_views) offsets[lane] = incl - c;
    if (lane == 63u) offsets[n_views] = incl;
}

__global__ __launch_bounds__(EMIT_BLOCK) void k_fi_emit(const ivx_fi_instance* __restrict__ inst, uint32_t n, uint32_t n_words, const ivx_fi_view* __restrict__ views,
                                                        uint32_t n_pairs, const unsigned long long* __restrict__ kept, const uint32_t* __restrict__ prefix,
                                                        const uint32_t* __restrict__ offsets, uint2* __restrict__ pairs, uint32_t* __restrict__ objects,
                                                        ivx_similarity* __restrict__ transforms) {
    constexpr uint32_t PAIR_WORDS = sizeof(ivx_cull_pair) / 8u;  // 5
    __shared__ uint2 s_pairs[EMIT_BLOCK * PAIR_WORDS];
    const uint32_t first = blockIdx.x * EMIT_BLOCK, i = first + threadIdx.x;
    if (i < n_pairs) {
        const uint32_t v = i / n, o = i - v * n;
        const size_t w = (size_t)v * n_words + (o >> 6);
        const unsigned long long word = kept[w];
        ivx_cull_pair p = fi_skip_pair();
        if ((word >> (o & 63u)) & 1ull) {
            const uint32_t rank = prefix[w] + (uint32_t)__popcll(word & ((1ull << (o & 63u)) - 1ull));
            const ivx_similarity s = fi_compose(views[v].world_to_view, inst[o].model_to_world);
            p = fi_pair(s, views[v].instance_base + rank, 0u);
            const uint32_t at = offsets[v] + rank;
            if (at < n_pairs) objects[at] = o, transforms[at] = s;  // (always: the ranks came from these very words)
        }
        const uint32_t* src = reinterpret_cast<const uint32_t*>(&p);
#pragma unroll
        for (uint32_t k = 0; k < PAIR_WORDS; ++k) s_pairs[threadIdx.x * PAIR_WORDS + k] = make_uint2(src[2u * k], src[2u * k + 1u]);
    }
    __syncthreads();
    const uint32_t live_words = min(EMIT_BLOCK, n_pairs - first) * PAIR_WORDS;
    uint2* __restrict__ out = pairs + (size_t)first * PAIR_WORDS;
#pragma unroll
    for (uint32_t k = 0; k < PAIR_WORDS; ++k) {
        const uint32_t j = k * EMIT_BLOCK + threadIdx.x;
        if (j < live_words) out[j] = s_pairs[j];
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
// context-owned state: device buffers that only grow, a pinned staging block for the one upload of a call (device_common.hpp), the instances the
// context holds and the layout of the last call
struct FiState {
    ivx_buf inst;     // ivx_fi_instance[n_inst]
    ivx_buf scratch;  // views | partials | prefix
    ivx_buf pairs;    // ivx_cull_pair[n_views x n]
    ivx_buf lists;    // offsets | objects | transforms
    ivx_buf results;  // ivx_fi_view_result[MAX_VIEWS]
    ivx_buf kept[2];  // kept[cur]: the last call's masks; the other one: the next call's
    ivx_staging staging;
    bool has_inst = false;
    uint32_t n_inst = 0;
    int cur = 0;
    bool has_views = false;  // a call has succeeded and its outputs stand
    uint32_t n_views = 0, n = 0;
    uint64_t serial = 0;  // the set that call ran on (ivx_bvol_set_serial)
    size_t o_objects = 0, o_transforms = 0;
};

int state_of(ivx_ctx* c, FiState** out) { return ivx_state_for(&c->fi_state, "frame instances", out); }

int check_instances(const char* who, const ivx_fi_instance* instances, size_t n) {
    IVX_REQUIRE(n <= IVX_BV_MAX_OBJECTS, IVX_ERR_CAPACITY, "%s: %zu instances exceed %u", who, n, IVX_BV_MAX_OBJECTS);
    IVX_REQUIRE(instances || n == 0, IVX_ERR_INVALID, "%s: null instances", who);
    for (size_t o = 0; o < n; ++o) {
        IVX_REQUIRE(instances[o].model_to_world.scaling > 0.0f, IVX_ERR_INVALID, "%s: the scaling %g of instance %zu is not positive", who,
                    (double)instances[o].model_to_world.scaling, o);
        IVX_REQUIRE((instances[o].flags & ~IVX_FI_ALL_FLAGS) == 0u, IVX_ERR_INVALID, "%s: instance %zu has unknown flag bits (flags %#x)", who, o, instances[o].flags);
    }
    return IVX_OK;
}

int check_views(const char* who, const ivx_fi_view* views, size_t n_views, size_t n_queries, size_t n_previous_views) {
    IVX_REQUIRE(n_views <= MAX_VIEWS, IVX_ERR_INVALID, "%s: %zu views exceed %u per call", who, n_views, MAX_VIEWS);
    IVX_REQUIRE(views || n_views == 0, IVX_ERR_INVALID, "%s: null views", who);
    for (size_t v = 0; v < n_views; ++v) {
        IVX_REQUIRE(views[v].world_to_view.scaling > 0.0f, IVX_ERR_INVALID, "%s: the scaling %g of view %zu is not positive", who, (double)views[v].world_to_view.scaling, v);
        IVX_REQUIRE(views[v].query < n_queries, IVX_ERR_INVALID, "%s: view %zu names query %u, the last queries call had %zu", who, v, views[v].query, n_queries);
        IVX_REQUIRE(views[v].and_view == IVX_FI_NONE || views[v].and_view < n_previous_views, IVX_ERR_INVALID, "%s: view %zu names view %u of the previous call, which had %zu", who,
                    v, views[v].and_view, n_previous_views);
        IVX_REQUIRE((views[v].reject_flags & ~IVX_FI_ALL_FLAGS) == 0u, IVX_ERR_INVALID, "%s: view %zu rejects unknown flag bits (%#x)", who, v, views[v].reject_flags);
        IVX_REQUIRE((views[v].flags & ~(IVX_FI_VIEW_REACH | IVX_FI_VIEW_BOX)) == 0u, IVX_ERR_INVALID, "%s: view %zu has unknown flag bits (flags %#x)", who, v, views[v].flags);
    }
    return IVX_OK;
}

void empty_result(ivx_fi_view_result* r) {
    float vals[N_VALUES];
    for (uint32_t f = 0; f < N_VALUES; ++f) vals[f] = value_neutral(f);
    fi_store_result(r, 0u, vals);
}

}  // namespace

void ivx_fi_release(ivx_ctx* c) {
    FiState* s = c ? ivx_state_take<FiState>(&c->fi_state) : nullptr;
    if (!s) return;
    for (ivx_buf* b : {&s->inst, &s->scratch, &s->pairs, &s->lists, &s->results, &s->kept[0], &s->kept[1]}) ivx_buf_free(b);
    ivx_staging_release(&s->staging);
    delete s;
}

int ivx_fi_resident_pairs(ivx_ctx* c, const char* who, size_t n_views, const ivx_cull_pair** d_pairs, uint32_t* n) {
    const FiState* st = static_cast<const FiState*>(c->fi_state);
    IVX_REQUIRE(st && st->has_views, IVX_ERR_STATE, "%s: the context holds no frame-instance pairs (call ivx_fi_views first)", who);
    IVX_REQUIRE(st->n_views == n_views, IVX_ERR_STATE, "%s: the context's last ivx_fi_views call had %u views, not %zu", who, st->n_views, n_views);
    *n = st->n;
    *d_pairs = st->n && st->n_views ? static_cast<const ivx_cull_pair*>(st->pairs.p) : nullptr;
    return IVX_OK;
}

extern "C" {

int ivx_fi_set_instances(ivx_ctx* c, const ivx_fi_instance* instances, size_t n) {
    const char* who = "ivx_fi_set_instances";
    IVX_REQUIRE(c, IVX_ERR_INVALID, "%s: null context", who);
    if (int rc = check_instances(who, instances, n)) return rc;
    FiState* st;
    if (int rc = state_of(c, &st)) return rc;
    ivx_many_other_context other_(c);
    st->has_inst = false, st->n_inst = 0;  // (until this call's instances stand)
    if (n != 0) {
        const size_t bytes = n * sizeof(ivx_fi_instance);
        if (int rc = ivx_staging_for(&st->staging, bytes)) return rc;
        if (int rc = ivx_buf_grow(c, &st->inst, bytes, 1u << 16)) return rc;
        memcpy(st->staging.p, instances, bytes);
        (void)ivx_many_break();
        if (int rc = ivx_staging_upload(&st->staging, st->inst.p, bytes, c->stream)) return rc;
    }
    st->has_inst = true, st->n_inst = (uint32_t)n;
    return IVX_OK;
}

int ivx_fi_views(ivx_ctx* c, const ivx_fi_view* views, size_t n_views, ivx_fi_view_result* results) {
    const char* who = "ivx_fi_views";
    IVX_REQUIRE(c, IVX_ERR_INVALID, "%s: null context", who);
    IVX_REQUIRE(n_views <= MAX_VIEWS, IVX_ERR_INVALID, "%s: %zu views exceed %u per call", who, n_views, MAX_VIEWS);
    ivx_bvol_view set;
    if (int rc = ivx_bvol_view_of(c, who, &set)) return rc;
    IVX_REQUIRE(set.n_queried != 0u, IVX_ERR_STATE, "%s: no queries call since the context's set (call ivx_bv_queries or ivx_bv_queries_hierarchy first)", who);
    FiState* st = static_cast<FiState*>(c->fi_state);
    IVX_REQUIRE(st && st->has_inst, IVX_ERR_STATE, "%s: the context holds no instances (call ivx_fi_set_instances first)", who);
    IVX_REQUIRE(st->n_inst == set.n, IVX_ERR_STATE, "%s: the context holds %u instances, its set of bounding volumes has %u objects", who, st->n_inst, set.n);
    const bool has_previous = st->has_views && st->serial == set.serial;  // (a new set drops the kept masks of the call before)
    const uint32_t n_previous = has_previous ? st->n_views : 0u;
    if (int rc = check_views(who, views, n_views, set.n_queried, n_previous)) return rc;
    ivx_many_other_context other_(c);
    const uint32_t n = set.n, n_words = (n + 63u) / 64u, n_tiles = (n + TILE - 1u) / TILE, n_pairs = (uint32_t)(n_views * n);  // (at most 2^6 x 2^20)
    st->has_views = false;  // (until this call's outputs stand)
    if (n_pairs == 0u) {
        for (size_t v = 0; v < n_views && results; ++v) empty_result(results + v);
        st->has_views = true, st->n_views = (uint32_t)n_views, st->n = n, st->serial = set.serial, st->cur ^= 1;
        return IVX_OK;
    }
    ivx_layout l;
    const size_t o_views = l.take(n_views * sizeof(ivx_fi_view)), o_partials = l.take(n_views * n_tiles * N_VALUES * 4), o_prefix = l.take(n_views * (size_t)n_words * 4);
    ivx_layout ll;
    const size_t o_offsets = ll.take((n_views + 1u) * 4), o_objects = ll.take((size_t)n_pairs * 4), o_transforms = ll.take((size_t)n_pairs * sizeof(ivx_similarity));
    ivx_buf* kept_new = &st->kept[st->cur ^ 1];
    if (int rc = ivx_staging_for(&st->staging, n_views * sizeof(ivx_fi_view))) return rc;
    if (int rc = ivx_buf_grow(c, &st->scratch, l.bytes, 1u << 16)) return rc;
    if (int rc = ivx_buf_grow(c, &st->pairs, (size_t)n_pairs * sizeof(ivx_cull_pair), 1u << 16)) return rc;
    if (int rc = ivx_buf_grow(c, &st->lists, ll.bytes, 1u << 16)) return rc;
    if (int rc = ivx_buf_grow(c, &st->results, MAX_VIEWS * sizeof(ivx_fi_view_result), 0)) return rc;
    if (int rc = ivx_buf_grow(c, kept_new, n_views * (size_t)n_words * 8, 1u << 12)) return rc;
    char* s = static_cast<char*>(st->scratch.p);
    char* d_lists = static_cast<char*>(st->lists.p);
    memcpy(st->staging.p, views, n_views * sizeof(ivx_fi_view));
    (void)ivx_many_break();
    if (int rc = ivx_staging_upload(&st->staging, s + o_views, n_views * sizeof(ivx_fi_view), c->stream)) return rc;
    const ivx_fi_view* d_views = reinterpret_cast<const ivx_fi_view*>(s + o_views);
    const ivx_fi_instance* d_inst = static_cast<const ivx_fi_instance*>(st->inst.p);
    float* d_partials = reinterpret_cast<float*>(s + o_partials);
    uint32_t* d_prefix = reinterpret_cast<uint32_t*>(s + o_prefix);
    unsigned long long* d_kept = static_cast<unsigned long long*>(kept_new->p);
    const unsigned long long* d_prev = n_previous ? static_cast<const unsigned long long*>(st->kept[st->cur].p) : nullptr;
    ivx_fi_view_result* d_results = static_cast<ivx_fi_view_result*>(st->results.p);
    uint32_t* d_offsets = reinterpret_cast<uint32_t*>(d_lists + o_offsets);
    IVX_KLAUNCH(k_fi_decide, dim3(n_tiles, (uint32_t)((n_views + VIEW_GROUP - 1u) / VIEW_GROUP)), dim3(TILE), 0, c->stream, set.world, d_inst, n, n_words, set.masks, d_prev, d_views, (uint32_t)n_views, d_kept, d_prefix, d_partials,
                n_tiles);
    IVX_KLAUNCH(k_fi_view, dim3((uint32_t)n_views), dim3(SCAN_ROUND), 0, c->stream, d_prefix, n_words, (const float*)d_partials, n_tiles, d_results);
    IVX_KLAUNCH(k_fi_offsets, dim3(1), dim3(64), 0, c->stream, (const ivx_fi_view_result*)d_results, (uint32_t)n_views, d_offsets);
    IVX_KLAUNCH(k_fi_emit, dim3((n_pairs + EMIT_BLOCK - 1u) / EMIT_BLOCK), dim3(EMIT_BLOCK), 0, c->stream, d_inst, n, n_words, d_views, n_pairs, (const unsigned long long*)d_kept,
                (const uint32_t*)d_prefix, (const uint32_t*)d_offsets, static_cast<uint2*>(st->pairs.p), reinterpret_cast<uint32_t*>(d_lists + o_objects),
                reinterpret_cast<ivx_similarity*>(d_lists + o_transforms));
    IVX_HIP_CHECK(hipGetLastError());
    if (results) {
        IVX_HIP_CHECK(ivx_memcpy_async(results, d_results, n_views * sizeof(ivx_fi_view_result), hipMemcpyDeviceToHost, c->stream));
        IVX_HIP_CHECK(ivx_stream_sync(c->stream));
    }
    st->o_objects = o_objects, st->o_transforms = o_transforms;
    st->has_views = true, st->n_views = (uint32_t)n_views, st->n = n, st->serial = set.serial, st->cur ^= 1;
    return IVX_OK;
}

int ivx_fi_download(ivx_ctx* c, ivx_cull_pair* pairs, size_t pair_cap, uint32_t* offsets, size_t offset_cap, uint32_t* objects, ivx_similarity* transforms, size_t list_cap,
                    uint64_t* kept_masks, size_t kept_cap, size_t* n_listed) {
    const char* who = "ivx_fi_download";
    if (n_listed) *n_listed = 0;
    IVX_REQUIRE(c, IVX_ERR_INVALID, "%s: null context", who);
    const FiState* st = static_cast<const FiState*>(c->fi_state);
    IVX_REQUIRE(st && st->has_views, IVX_ERR_STATE, "%s: no frame instances on this context (call ivx_fi_views first)", who);
    const size_t n_views = st->n_views, n = st->n, n_words = (n + 63u) / 64u, n_pairs = n_views * n;
    IVX_REQUIRE(!pairs || pair_cap >= n_pairs, IVX_ERR_CAPACITY, "%s: the last call left %zu pairs, the buffer holds %zu", who, n_pairs, pair_cap);
    IVX_REQUIRE(!offsets || offset_cap >= n_views + 1u, IVX_ERR_CAPACITY, "%s: %zu offsets, the buffer holds %zu", who, n_views + 1u, offset_cap);
    IVX_REQUIRE(!kept_masks || kept_cap >= n_views * n_words, IVX_ERR_CAPACITY, "%s: %zu kept words, the buffer holds %zu", who, n_views * n_words, kept_cap);
    if (n_pairs == 0) {  // (nothing is on the device)
        for (size_t v = 0; v <= n_views && offsets; ++v) offsets[v] = 0u;
        return IVX_OK;
    }
    ivx_many_other_context other_(c);
    (void)ivx_many_break();
    const char* d_lists = static_cast<const char*>(st->lists.p);
    uint32_t total = 0;
    IVX_HIP_CHECK(ivx_memcpy_async(&total, d_lists + n_views * 4, 4, hipMemcpyDeviceToHost, c->stream));
    IVX_HIP_CHECK(ivx_stream_sync(c->stream));
    if (n_listed) *n_listed = total;
    IVX_REQUIRE((!objects && !transforms) || list_cap >= total, IVX_ERR_CAPACITY, "%s: %u list entries, the buffers hold %zu", who, total, list_cap);
    if (pairs) IVX_HIP_CHECK(ivx_memcpy_async(pairs, st->pairs.p, n_pairs * sizeof(ivx_cull_pair), hipMemcpyDeviceToHost, c->stream));
    if (offsets) IVX_HIP_CHECK(ivx_memcpy_async(offsets, d_lists, (n_views + 1u) * 4, hipMemcpyDeviceToHost, c->stream));
    if (objects && total) IVX_HIP_CHECK(ivx_memcpy_async(objects, d_lists + st->o_objects, (size_t)total * 4, hipMemcpyDeviceToHost, c->stream));
    if (transforms && total) IVX_HIP_CHECK(ivx_memcpy_async(transforms, d_lists + st->o_transforms, (size_t)total * sizeof(ivx_similarity), hipMemcpyDeviceToHost, c->stream));
    if (kept_masks) IVX_HIP_CHECK(ivx_memcpy_async(kept_masks, st->kept[st->cur].p, n_views * n_words * 8, hipMemcpyDeviceToHost, c->stream));
    IVX_HIP_CHECK(ivx_stream_sync(c->stream));
    return IVX_OK;
}

void* ivx_fi_device_ptr(ivx_ctx* c, int which) {
    if (!c || !c->fi_state) return nullptr;
    FiState* st = static_cast<FiState*>(c->fi_state);
    if (which == IVX_FI_PTR_INSTANCES) return st->has_inst && st->n_inst ? st->inst.p : nullptr;
    if (!st->has_views || st->n == 0u || st->n_views == 0u) return nullptr;
    char* d_lists = static_cast<char*>(st->lists.p);
    switch (which) {
        case IVX_FI_PTR_PAIRS: return st->pairs.p;
        case IVX_FI_PTR_OFFSETS: return d_lists;
        case IVX_FI_PTR_OBJECTS: return d_lists + st->o_objects;
        case IVX_FI_PTR_TRANSFORMS: return d_lists + st->o_transforms;
        case IVX_FI_PTR_KEPT_MASKS: return st->kept[st->cur].p;
        case IVX_FI_PTR_RESULTS: return st->results.p;
        default: return nullptr;
    }
}

int ivx_fi_views_host(const ivx_aabb* world_boxes, size_t n, const ivx_fi_instance* instances, const uint64_t* masks, size_t n_queries, const ivx_fi_view* views,
                      size_t n_views, const uint64_t* previous_kept, size_t n_previous_views, ivx_cull_pair* pairs, uint32_t* offsets, uint32_t* objects,
                      ivx_similarity* transforms, size_t list_cap, uint64_t* kept_masks, ivx_fi_view_result* results) {
    const char* who = "ivx_fi_views_host";
    if (int rc = check_instances(who, instances, n)) return rc;
    if (int rc = check_views(who, views, n_views, n_queries, n_previous_views)) return rc;
    IVX_REQUIRE((world_boxes && masks) || n == 0 || n_views == 0, IVX_ERR_INVALID, "%s: null argument", who);
    IVX_REQUIRE(previous_kept || n_previous_views == 0 || n == 0, IVX_ERR_INVALID, "%s: null previous kept masks of %zu views", who, n_previous_views);
    const size_t n_words = (n + 63u) / 64u;
    // the kept sets first: the lists are written only when they fit
    std::vector<uint64_t> kept(n_views * n_words, 0ull);
    std::vector<ivx_fi_view_result> res(n_views);
    size_t total = 0;
    for (size_t v = 0; v < n_views; ++v) {
        const ivx_fi_view& vw = views[v];
        float acc[N_VALUES];
        for (uint32_t f = 0; f < N_VALUES; ++f) acc[f] = value_neutral(f);
        uint32_t count = 0u;
        for (size_t o = 0; o < n; ++o) {
            const bool hit = ((masks[vw.query * n_words + (o >> 6)] >> (o & 63u)) & 1ull) != 0ull;
            const bool and_ok = vw.and_view == IVX_FI_NONE || ((previous_kept[vw.and_view * n_words + (o >> 6)] >> (o & 63u)) & 1ull) != 0ull;
            float vals[N_VALUES];
            if (!fi_keeps(world_boxes[o], instances[o].flags, instances[o].entity, hit, and_ok, vw, vals)) continue;
            kept[v * n_words + (o >> 6)] |= 1ull << (o & 63u);
            for (uint32_t f = 0; f < N_VALUES; ++f) acc[f] = value_merge(f, acc[f], vals[f]);
            ++count;
        }
        fi_store_result(&res[v], count, acc);
        total += count;
    }
    IVX_REQUIRE((!objects && !transforms) || list_cap >= total, IVX_ERR_CAPACITY, "%s: %zu list entries, the buffers hold %zu", who, total, list_cap);
    uint32_t at = 0u;
    for (size_t v = 0; v < n_views; ++v) {
        if (offsets) offsets[v] = at;
        uint32_t rank = 0u;
        for (size_t o = 0; o < n; ++o) {
            ivx_cull_pair p = fi_skip_pair();
            if ((kept[v * n_words + (o >> 6)] >> (o & 63u)) & 1ull) {
                const ivx_similarity s = fi_compose(views[v].world_to_view, instances[o].model_to_world);
                p = fi_pair(s, views[v].instance_base + rank, 0u);
                if (objects) objects[at] = (uint32_t)o;
                if (transforms) transforms[at] = s;
                ++rank, ++at;
            }
            if (pairs) pairs[v * n + o] = p;
        }
        if (results) results[v] = res[v];
    }
    if (offsets) offsets[n_views] = at;
    if (kept_masks && !kept.empty()) memcpy(kept_masks, kept.data(), kept.size() * 8);
    return IVX_OK;
}

}  // extern "C"
