// Chunk culling: indirect draw arguments for every chunk submesh of every object under every view of a frame, in one call.
//
// Reference: impact_voxel/shaders/compute/voxel_chunk_culling.template.wgsl (the decision), impact_voxel/src/render_commands.rs:392-598 (one
//   dispatch, push constants and bind group per object per view; the transform to normalised object space), impact_voxel/src/mesh.rs:128-131,
//   638-696 (CullingFrustum), impact_geometry/src/plane.rs:186-192, oriented_box.rs:167-173, 221-240, axis_aligned_box.rs:494-507;
//   docs/voxel_gpu_buffer_pooling.md (the per-object dispatches are 21 % of its stress scene's frame; its end state is this file's call).
//
// DERIVE — k_cull_frusta, one lane per (view, object): the view's planes (or oriented box) through the inverse of the object-to-view similarity
//   with the chunk extent folded into its scaling, so that chunk (i, j, k) is the unit box at (i, j, k). The same __host__ __device__ function is
//   exported for the host (ivx_culling_frustum_from_view): IEEE division, no contraction, so both sides give the same bytes.
// DECIDE — k_cull_tiles, one wave per tile of 64 consecutive submeshes of one object (the host lists the tiles from the counts it holds). A lane
//   reads its 64-byte record once and keeps chunk indices, index range and the obscuredness table packed to 8 bits; the wave then walks the
//   views. The frustum record of (view, object) has a wave-uniform address (the tile's object index goes through readfirstlane), so it arrives by
//   scalar loads and costs no vector memory instruction and no LDS. Each (view, tile) leaves its __ballot mask and the sum of the index counts drawn;
//   mode 0 also stores the arguments here, lanes writing consecutive 16- or 20-byte slots.
// SCAN — k_cull_scan, one wave per view: exclusive prefix of the tiles' popcounts 64 tiles at a time with a carry, in tile order; the totals are
//   the view's count record. No atomics anywhere: the order of a compacted list is (object, submesh) and two calls leave the same bytes.
// PLACE — k_cull_place (mode 1), one wave per (tile, view): a drawn lane's slot is the tile's prefix plus the set bits of the mask below it; every
//   lane whose own slot lies at or behind the view's count zeroes that slot — the two sets of slots are disjoint and together cover the region.
// GATHER — k_cull_gather (ivx_cull_many_resident), one lane per (view, object): the pair and its flags from the frame-instance pairs the context
//   holds (instances.hip), at the object's index there, to where the upload of the other entry points puts them.
#include <cmath>
#include <vector>

#include "device_common.hpp"
#include "instances_internal.hpp"

namespace {

constexpr uint32_t MAX_VIEWS = 64;
constexpr float CULLING_THRESHOLD = -0.05f;

// ---- shared host / device arithmetic of the derivation (f32, fixed operation order) --------------------------------------------------------
__host__ __device__ __forceinline__ float dot3(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__host__ __device__ __forceinline__ void q_rotate(const float q[4], const float v[3], float out[3]) {  // q = (x, y, z, w), unit
    const float tx = 2.0f * (q[1] * v[2] - q[2] * v[1]), ty = 2.0f * (q[2] * v[0] - q[0] * v[2]), tz = 2.0f * (q[0] * v[1] - q[1] * v[0]);
    out[0] = v[0] + q[3] * tx + (q[1] * tz - q[2] * ty);
    out[1] = v[1] + q[3] * ty + (q[2] * tx - q[0] * tz);
    out[2] = v[2] + q[3] * tz + (q[0] * ty - q[1] * tx);
}
__host__ __device__ __forceinline__ void q_mul(const float a[4], const float b[4], float out[4]) {  // Hamilton product a b
    out[0] = ((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1];
    out[1] = ((a[3] * b[1] - a[0] * b[2]) + a[1] * b[3]) + a[2] * b[0];
    out[2] = ((a[3] * b[2] + a[0] * b[1]) - a[1] * b[0]) + a[2] * b[3];
    out[3] = ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2];
}
__host__ __device__ __forceinline__ uint32_t sign_bit(float v) {
#ifdef __HIP_DEVICE_COMPILE__
    return __float_as_uint(v) >> 31;
#else
    uint32_t u;
    memcpy(&u, &v, 4);
    return u >> 31;
#endif
}
// maximum_corner_idx_along_direction: bit 2 / 1 / 0 set where x / y / z does not have its sign bit set (-0.0 and a negative NaN choose the lower corner)
__host__ __device__ __forceinline__ uint32_t most_inside_corner(const float n[3]) {
    return ((sign_bit(n[0]) ^ 1u) << 2) | ((sign_bit(n[1]) ^ 1u) << 1) | (sign_bit(n[2]) ^ 1u);
}
__host__ __device__ __forceinline__ void set_plane(ivx_culling_frustum* f, int i, const float n[3], float d) {
    f->planes[i][0] = n[0], f->planes[i][1] = n[1], f->planes[i][2] = n[2], f->planes[i][3] = d;
    f->most_inside_corners[i] = most_inside_corner(n);
}

__host__ __device__ inline void derive_frustum(const ivx_cull_view* v, const ivx_cull_pair* p, float chunk_extent, ivx_culling_frustum* f) {
    // T = inverse of (translation, rotation, scaling x chunk extent): Similarity3::applied_to_scaling, ::inverted
    const float inv_s = 1.0f / (p->scaling * chunk_extent);
    const float tq[4] = {-p->rotation[0], -p->rotation[1], -p->rotation[2], p->rotation[3]};
    const float st[3] = {inv_s * p->translation[0], inv_s * p->translation[1], inv_s * p->translation[2]};
    float r[3];
    q_rotate(tq, st, r);
    const float tt[3] = {-r[0], -r[1], -r[2]};
    if (v->kind == 0u) {
        for (int i = 0; i < 6; ++i) {  // Plane::transformed
            const float n[3] = {v->planes[i][0], v->planes[i][1], v->planes[i][2]};
            const float d = v->planes[i][3];
            const float sp[3] = {inv_s * (n[0] * d), inv_s * (n[1] * d), inv_s * (n[2] * d)};
            float pt[3], nt[3];
            q_rotate(tq, sp, pt);
            pt[0] += tt[0], pt[1] += tt[1], pt[2] += tt[2];
            q_rotate(tq, n, nt);
            set_plane(f, i, nt, dot3(nt, pt));
        }
        f->apex[0] = tt[0], f->apex[1] = tt[1], f->apex[2] = tt[2];
    } else {
        // OrientedBox::transformed, ::compute_bounding_planes
        const float sc[3] = {inv_s * v->box_center[0], inv_s * v->box_center[1], inv_s * v->box_center[2]};
        float c[3], o[4];
        q_rotate(tq, sc, c);
        c[0] += tt[0], c[1] += tt[1], c[2] += tt[2];
        q_mul(tq, v->box_orientation, o);
        const float h[3] = {inv_s * v->box_half_extents[0], inv_s * v->box_half_extents[1], inv_s * v->box_half_extents[2]};
        const float oi[4] = {-o[0], -o[1], -o[2], o[3]};
        float local[3];
        q_rotate(oi, c, local);
        for (int a = 0; a < 3; ++a) {
            const float e[3] = {a == 0 ? 1.0f : 0.0f, a == 1 ? 1.0f : 0.0f, a == 2 ? 1.0f : 0.0f};
            float axis[3];
            q_rotate(o, e, axis);
            const float neg[3] = {-axis[0], -axis[1], -axis[2]};
            set_plane(f, 2 * a, axis, local[a] - h[a]);
            set_plane(f, 2 * a + 1, neg, -(local[a] + h[a]));
            if (a == 2)  // apex = centre - apex_distance x view direction, view direction = -depth axis
                for (int k = 0; k < 3; ++k) f->apex[k] = c[k] - v->apex_distance * neg[k];
        }
    }
    f->instance_idx = p->instance_idx;
}

// ---- device records ----------------------------------------------------------------------------------------------------------------------
struct CullObj {  // 32 bytes
    const ivx_submesh* table;
    uint32_t n_sub, base, first_index_base;
    int32_t base_vertex;
    float chunk_extent;
    uint32_t pad;
};
static_assert(sizeof(CullObj) == 32, "scalar loads of whole records");
struct CullViewOut {  // 16 bytes: where the view's region starts in the argument buffer, and its slot layout
    uint64_t offset;
    uint32_t indexed, pad;
};
// per (view, tile): x, y the mask of drawn lanes, z the sum of their index counts, w the drawn slots of the view's earlier tiles (k_cull_scan)

__global__ __launch_bounds__(256) void k_cull_frusta(const ivx_cull_view* __restrict__ views, uint32_t n_views, const ivx_cull_pair* __restrict__ pairs,
                                                     const CullObj* __restrict__ objs, uint32_t n_obj, ivx_culling_frustum* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_views * n_obj) return;
    const ivx_cull_view v = views[i / n_obj];
    const ivx_cull_pair p = pairs[i];
    ivx_culling_frustum f;
    derive_frustum(&v, &p, objs[i % n_obj].chunk_extent, &f);
    out[i] = f;
}

// pairs[v * n_obj + g] = src[v * src_n + index[g]] (index null: g), and the pair's flags beside it
__global__ __launch_bounds__(256) void k_cull_gather(const ivx_cull_pair* __restrict__ src, uint32_t src_n, const uint32_t* __restrict__ index, uint32_t n_views, uint32_t n_obj,
                                                     ivx_cull_pair* __restrict__ pairs, uint32_t* __restrict__ pair_flags) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_views * n_obj) return;
    const uint32_t v = i / n_obj, g = i - v * n_obj;
    const uint32_t o = index ? index[g] : g;
    const ivx_cull_pair p = src[(size_t)v * src_n + (o < src_n ? o : 0u)];  // (the host has refused an index past src_n)
    pairs[i] = p;
    pair_flags[i] = p.flags;
}

__device__ __forceinline__ void store_args(char* __restrict__ region, uint32_t indexed, uint32_t slot, uint32_t index_count, uint32_t instance_count, uint32_t first_index,
                                           int32_t base_vertex, uint32_t first_instance) {
    if (indexed) {
        uint32_t* a = reinterpret_cast<uint32_t*>(region + (size_t)slot * 20u);
        a[0] = index_count, a[1] = instance_count, a[2] = first_index, a[3] = (uint32_t)base_vertex, a[4] = first_instance;
    } else {
        uint32_t* a = reinterpret_cast<uint32_t*>(region + (size_t)slot * 16u);
        a[0] = index_count, a[1] = instance_count, a[2] = first_index, a[3] = first_instance;
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_cull_tiles(const uint2* __restrict__ tiles, uint32_t n_tiles, const CullObj* __restrict__ objs, uint32_t n_obj,
                                                    const ivx_culling_frustum* __restrict__ frusta, const uint32_t* __restrict__ pair_flags,
                                                    const CullViewOut* __restrict__ vout, uint32_t n_views, char* __restrict__ args, uint4* __restrict__ tile_info) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (tile >= n_tiles) return;  // (whole waves)
    const uint2 t = tiles[tile];
    const uint32_t obj = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.x), s0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.y);
    const CullObj o = objs[obj];
    const uint32_t s = s0 + lane;
    const bool live = s < o.n_sub;
    float lx = 0.f, ly = 0.f, lz = 0.f;
    uint32_t index_offset = 0u, index_count = 0u, obscured = 0u;
    if (live) {
        const ivx_submesh r = o.table[s];
        lx = (float)r.chunk_indices[0], ly = (float)r.chunk_indices[1], lz = (float)r.chunk_indices[2];
        index_offset = r.index_offset, index_count = r.index_count;
#pragma unroll
        for (int b = 0; b < 8; ++b) obscured |= (r.is_obscured_from_direction[b >> 2][(b >> 1) & 1][b & 1] > 0u ? 1u : 0u) << b;
    }
    const float cx = lx + 0.5f, cy = ly + 0.5f, cz = lz + 0.5f;
    const uint32_t first_index = index_offset + o.first_index_base;
    for (uint32_t v = 0; v < n_views; ++v) {
        const size_t pair = (size_t)v * n_obj + obj;
        const ivx_culling_frustum* __restrict__ f = frusta + pair;
        bool culled = (pair_flags[pair] & 1u) != 0u;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const uint32_t corner = f->most_inside_corners[q];
            const float px = lx + ((corner & 4u) ? 1.0f : 0.0f), py = ly + ((corner & 2u) ? 1.0f : 0.0f), pz = lz + ((corner & 1u) ? 1.0f : 0.0f);
            const float dist = ((f->planes[q][0] * px + f->planes[q][1] * py) + f->planes[q][2] * pz) - f->planes[q][3];
            culled = culled || dist < CULLING_THRESHOLD;
        }
        const uint32_t ix = cx - f->apex[0] < 0.0f ? 1u : 0u, iy = cy - f->apex[1] < 0.0f ? 1u : 0u, iz = cz - f->apex[2] < 0.0f ? 1u : 0u;
        culled = culled || ((obscured >> (ix * 4u + iy * 2u + iz)) & 1u) != 0u;
        const bool drawn = live && !culled;
        const unsigned long long mask = __ballot(drawn);
        const uint32_t drawn_indices = ivx_wave_sum(drawn ? index_count : 0u);
        if (lane == 0u) tile_info[(size_t)v * n_tiles + tile] = make_uint4((uint32_t)mask, (uint32_t)(mask >> 32), drawn_indices, 0u);
        if (MODE == 0) {
            const CullViewOut w = vout[v];
            if (live) store_args(args + w.offset, w.indexed, o.base + s, drawn ? index_count : 0u, drawn ? 1u : 0u, first_index, o.base_vertex, f->instance_idx);
        }
    }
}

__global__ __launch_bounds__(64) void k_cull_scan(uint4* __restrict__ tile_info, uint32_t n_tiles, ivx_cull_count* __restrict__ counts) {
    const uint32_t lane = threadIdx.x, v = blockIdx.x;
    uint4* __restrict__ info = tile_info + (size_t)v * n_tiles;
    uint32_t draws = 0u, indices = 0u;
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += 64u) {
        const uint32_t t = t0 + lane;
        uint32_t c = 0u, ic = 0u;
        if (t < n_tiles) {
            const uint4 r = info[t];
            c = (uint32_t)__popc(r.x) + (uint32_t)__popc(r.y), ic = r.z;
        }
        const uint32_t incl = ivx_wave_incl_scan(c);
        if (t < n_tiles) info[t].w = draws + incl - c;
        draws += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        indices += ivx_wave_sum(ic);
    }
    if (lane == 0u) counts[v].draws = draws, counts[v].indices = indices;
}

__global__ __launch_bounds__(256) void k_cull_place(const uint2* __restrict__ tiles, uint32_t n_tiles, const CullObj* __restrict__ objs, uint32_t n_obj,
                                                    const ivx_culling_frustum* __restrict__ frusta, const CullViewOut* __restrict__ vout,
                                                    const ivx_cull_count* __restrict__ counts, const uint4* __restrict__ tile_info, char* __restrict__ args) {
    const uint32_t lane = threadIdx.x & 63u, v = blockIdx.y;
    const uint32_t tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (tile >= n_tiles) return;  // (whole waves)
    const uint2 t = tiles[tile];
    const uint32_t obj = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.x), s0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.y);
    const CullObj o = objs[obj];
    const uint4 info = tile_info[(size_t)v * n_tiles + tile];
    const CullViewOut w = vout[v];
    const uint32_t count = counts[v].draws;
    const uint32_t s = s0 + lane;
    if (s >= o.n_sub) return;
    char* __restrict__ region = args + w.offset;
    const unsigned long long mask = ((unsigned long long)info.y << 32) | info.x;
    if ((mask >> lane) & 1ull) {
        const uint32_t rank = info.w + __builtin_amdgcn_mbcnt_hi(info.y, __builtin_amdgcn_mbcnt_lo(info.x, 0u));
        store_args(region, w.indexed, rank, o.table[s].index_count, 1u, o.table[s].index_offset + o.first_index_base, o.base_vertex, frusta[(size_t)v * n_obj + obj].instance_idx);
    }
    if (o.base + s >= count) store_args(region, w.indexed, o.base + s, 0u, 0u, 0u, 0, 0u);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
// context-owned state: device buffers that only grow, a pinned staging block for the one upload of a call (device_common.hpp), and the layout of the last call
struct CullState {
    ivx_buf args, frusta, scratch;
    ivx_buf counts;  // ivx_cull_count[MAX_VIEWS], made by the first enqueue (n_views != 0 only behind one)
    ivx_staging staging;
    uint32_t n_views = 0, n_obj = 0, total = 0;
    ivx_cull_region regions[MAX_VIEWS];
};

int state_of(ivx_ctx* c, CullState** out) { return ivx_state_for(&c->cull_state, "chunk culling", out); }

// what a call culls: the objects' tables (device pointers, or host arrays to upload), and either views + pairs or ready records
struct CullJob {
    const char* who;
    size_t n_obj, n_views;
    const ivx_submesh* const* d_tables;  // resident tables ...
    const ivx_submesh* const* h_tables;  // ... or host arrays
    const uint32_t* counts;
    const float* extents;  // per object (views + pairs form)
    const ivx_cull_object* objects;
    const ivx_cull_view* views;
    const ivx_cull_pair* pairs;
    bool records;                       // the second form: ready records with view_flags (and pair_flags, may be null) instead of views and pairs
    const ivx_culling_frustum* frusta;
    const uint32_t* view_flags;
    const uint32_t* pair_flags;
    uint32_t mode;
    // ivx_cull_many_resident: the frame-instance pairs on the device ([n_views][fi_n]) in place of `pairs`, and which of them each object takes (null: its own index)
    const ivx_cull_pair* fi_pairs;
    uint32_t fi_n;
    const uint32_t* object_indices;
};

int check_views_and_pairs(const char* who, const ivx_cull_view* views, size_t n_views, const ivx_cull_pair* pairs, const float* extents, size_t n_obj) {
    for (size_t v = 0; v < n_views; ++v)
        IVX_REQUIRE(views[v].kind <= 1u, IVX_ERR_INVALID, "%s: view %zu has kind %u (0 = frustum planes, 1 = orthographic box)", who, v, views[v].kind);
    for (size_t o = 0; o < n_obj; ++o) IVX_REQUIRE(extents[o] > 0.0f, IVX_ERR_INVALID, "%s: the chunk extent %g of object %zu is not positive", who, (double)extents[o], o);
    for (size_t i = 0; i < n_views * n_obj && pairs; ++i)  // (pairs null: they are on the device, ivx_cull_many_resident)
        IVX_REQUIRE(pairs[i].scaling > 0.0f, IVX_ERR_INVALID, "%s: the scaling %g of pair %zu (view %zu, object %zu) is not positive", who, (double)pairs[i].scaling, i, i / n_obj,
                    i % n_obj);
    return IVX_OK;
}

int cull_enqueue(ivx_ctx* c, const CullJob& j, ivx_cull_region* out_layout) {
    CullState* st;
    if (int rc = state_of(c, &st)) return rc;
    if (int rc = ivx_buf_grow(c, &st->counts, MAX_VIEWS * sizeof(ivx_cull_count), 0)) return rc;
    st->n_views = 0, st->n_obj = 0, st->total = 0;  // (until this call's layout stands: a call that fails leaves nothing to download)
    const size_t n_obj = j.n_obj, n_views = j.n_views, n_pairs = n_obj * n_views;
    // slots and tiles
    uint64_t total64 = 0;
    size_t n_tiles = 0, table_bytes = 0;
    for (size_t o = 0; o < n_obj; ++o) {
        total64 += j.counts[o];
        n_tiles += (j.counts[o] + 63u) / 64u;
        if (j.h_tables) table_bytes += ((size_t)j.counts[o] * sizeof(ivx_submesh) + 255u) & ~(size_t)255u;
    }
    IVX_REQUIRE(total64 < (1ull << 31) && n_pairs < (1ull << 31), IVX_ERR_CAPACITY, "%s: %llu submeshes in all, %zu (view, object) pairs: too many for one call", j.who,
                (unsigned long long)total64, n_pairs);
    const uint32_t total = (uint32_t)total64;
    ivx_layout regions;
    for (size_t v = 0; v < n_views; ++v) {
        const bool indexed = ((j.records ? j.view_flags[v] : j.views[v].flags) & IVX_CULL_VIEW_INDEXED) != 0u;
        st->regions[v].stride = indexed ? 20u : 16u;
        st->regions[v].n_slots = total;
        st->regions[v].offset = regions.take((size_t)total * st->regions[v].stride);
    }
    const auto done = [&]() {
        for (size_t v = 0; v < n_views && out_layout; ++v) out_layout[v] = st->regions[v];
        st->n_views = (uint32_t)n_views, st->n_obj = (uint32_t)n_obj, st->total = total;
        return IVX_OK;
    };
    if (n_views == 0) return done();
    // one staging block: views | pairs | records | pair flags | objects | view regions | tiles | tables
    ivx_layout l;
    // (resident pairs: pairs and pair flags lie behind the upload, where k_cull_gather writes them, and the objects' indices ride the upload)
    const bool resident = j.fi_pairs != nullptr;
    size_t o_pairs = l.take(0), o_flags = 0;
    const size_t o_views = l.take(j.records ? 0 : n_views * sizeof(ivx_cull_view));
    if (!resident) o_pairs = l.take(j.records ? 0 : n_pairs * sizeof(ivx_cull_pair));
    const size_t o_recs = l.take(j.records ? n_pairs * sizeof(ivx_culling_frustum) : 0);
    if (!resident) o_flags = l.take(n_pairs * 4);
    const size_t o_objs = l.take(n_obj * sizeof(CullObj)), o_vout = l.take(n_views * sizeof(CullViewOut)), o_tiles = l.take(n_tiles * sizeof(uint2)), o_tables = l.take(table_bytes),
                 o_index = l.take(resident && j.object_indices ? n_obj * 4 : 0);
    const size_t upload_bytes = l.bytes;
    const size_t o_info = l.take(n_views * n_tiles * sizeof(uint4));
    if (resident) o_pairs = l.take(n_pairs * sizeof(ivx_cull_pair)), o_flags = l.take(n_pairs * 4);
    if (int rc = ivx_staging_for(&st->staging, upload_bytes)) return rc;
    if (int rc = ivx_buf_grow(c, &st->scratch, l.bytes, 1u << 20)) return rc;
    if (int rc = ivx_buf_grow(c, &st->args, regions.bytes, 1u << 20)) return rc;
    if (int rc = ivx_buf_grow(c, &st->frusta, n_pairs * sizeof(ivx_culling_frustum), 1u << 16)) return rc;
    char* h = static_cast<char*>(st->staging.p);
    char* d = static_cast<char*>(st->scratch.p);
    if (j.records) {
        if (n_pairs) memcpy(h + o_recs, j.frusta, n_pairs * sizeof(ivx_culling_frustum));
    } else {
        memcpy(h + o_views, j.views, n_views * sizeof(ivx_cull_view));
        if (n_pairs && !resident) memcpy(h + o_pairs, j.pairs, n_pairs * sizeof(ivx_cull_pair));
    }
    if (resident) {
        if (j.object_indices) memcpy(h + o_index, j.object_indices, n_obj * 4);
    } else {
        uint32_t* flags = reinterpret_cast<uint32_t*>(h + o_flags);
        for (size_t i = 0; i < n_pairs; ++i) flags[i] = j.records ? (j.pair_flags ? j.pair_flags[i] : 0u) : j.pairs[i].flags;
    }
    CullObj* objs = reinterpret_cast<CullObj*>(h + o_objs);
    uint2* tiles = reinterpret_cast<uint2*>(h + o_tiles);
    size_t tile = 0, table_at = o_tables;
    uint32_t base = 0;
    for (size_t o = 0; o < n_obj; ++o) {
        const uint32_t cnt = j.counts[o];
        if (j.h_tables) {
            if (cnt) memcpy(h + table_at, j.h_tables[o], (size_t)cnt * sizeof(ivx_submesh));
            objs[o].table = reinterpret_cast<const ivx_submesh*>(d + table_at);
            table_at += ((size_t)cnt * sizeof(ivx_submesh) + 255u) & ~(size_t)255u;
        } else {
            objs[o].table = j.d_tables[o];
        }
        objs[o].n_sub = cnt, objs[o].base = base;
        objs[o].first_index_base = j.objects ? j.objects[o].first_index_base : 0u;
        objs[o].base_vertex = j.objects ? j.objects[o].base_vertex : 0;
        objs[o].chunk_extent = j.extents ? j.extents[o] : 1.0f;
        objs[o].pad = 0u;
        for (uint32_t s0 = 0; s0 < cnt; s0 += 64u) tiles[tile++] = make_uint2((uint32_t)o, s0);
        base += cnt;
    }
    CullViewOut* vout = reinterpret_cast<CullViewOut*>(h + o_vout);
    for (size_t v = 0; v < n_views; ++v) vout[v].offset = st->regions[v].offset, vout[v].indexed = st->regions[v].stride == 20u ? 1u : 0u, vout[v].pad = 0u;
    if (int rc = ivx_staging_upload(&st->staging, d, upload_bytes, c->stream)) return rc;  // (ahead of k_cull_gather, which reads the indices it brings)
    ivx_culling_frustum* d_frusta = static_cast<ivx_culling_frustum*>(st->frusta.p);
    const CullObj* d_objs = reinterpret_cast<const CullObj*>(d + o_objs);
    if (n_pairs && resident)
        IVX_KLAUNCH(k_cull_gather, dim3((uint32_t)((n_pairs + 255u) / 256u)), dim3(256), 0, c->stream, j.fi_pairs, j.fi_n,
                    j.object_indices ? reinterpret_cast<const uint32_t*>(d + o_index) : (const uint32_t*)nullptr, (uint32_t)n_views, (uint32_t)n_obj,
                    reinterpret_cast<ivx_cull_pair*>(d + o_pairs), reinterpret_cast<uint32_t*>(d + o_flags));
    if (n_pairs) {
        if (j.records)
            IVX_HIP_CHECK(ivx_memcpy_async(d_frusta, d + o_recs, n_pairs * sizeof(ivx_culling_frustum), hipMemcpyDeviceToDevice, c->stream));
        else
            IVX_KLAUNCH(k_cull_frusta, dim3((uint32_t)((n_pairs + 255u) / 256u)), dim3(256), 0, c->stream, reinterpret_cast<const ivx_cull_view*>(d + o_views), (uint32_t)n_views,
                        reinterpret_cast<const ivx_cull_pair*>(d + o_pairs), d_objs, (uint32_t)n_obj, d_frusta);
    }
    ivx_cull_count* d_counts = static_cast<ivx_cull_count*>(st->counts.p);
    if (n_tiles == 0) {  // no submesh anywhere: empty regions, zero counts
        IVX_HIP_CHECK(ivx_memset_async(d_counts, 0, n_views * sizeof(ivx_cull_count), c->stream));
        return done();
    }
    const uint2* d_tiles = reinterpret_cast<const uint2*>(d + o_tiles);
    const uint32_t* d_flags = reinterpret_cast<const uint32_t*>(d + o_flags);
    const CullViewOut* d_vout = reinterpret_cast<const CullViewOut*>(d + o_vout);
    uint4* d_info = reinterpret_cast<uint4*>(d + o_info);
    char* d_args = static_cast<char*>(st->args.p);
    const uint32_t tile_blocks = (uint32_t)((n_tiles + 3u) / 4u);
    if (j.mode == 0u)
        IVX_KLAUNCH(k_cull_tiles<0>, dim3(tile_blocks), dim3(256), 0, c->stream, d_tiles, (uint32_t)n_tiles, d_objs, (uint32_t)n_obj, (const ivx_culling_frustum*)d_frusta, d_flags,
                    d_vout, (uint32_t)n_views, d_args, d_info);
    else
        IVX_KLAUNCH(k_cull_tiles<1>, dim3(tile_blocks), dim3(256), 0, c->stream, d_tiles, (uint32_t)n_tiles, d_objs, (uint32_t)n_obj, (const ivx_culling_frustum*)d_frusta, d_flags,
                    d_vout, (uint32_t)n_views, d_args, d_info);
    IVX_KLAUNCH(k_cull_scan, dim3((uint32_t)n_views), dim3(64), 0, c->stream, d_info, (uint32_t)n_tiles, d_counts);
    if (j.mode == 1u)
        IVX_KLAUNCH(k_cull_place, dim3(tile_blocks, (uint32_t)n_views), dim3(256), 0, c->stream, d_tiles, (uint32_t)n_tiles, d_objs, (uint32_t)n_obj,
                    (const ivx_culling_frustum*)d_frusta, d_vout, (const ivx_cull_count*)d_counts, (const uint4*)d_info, d_args);
    IVX_HIP_CHECK(hipGetLastError());
    return done();
}

int cull_collect(ivx_ctx* c, const char* who, ivx_cull_count* out_counts, size_t n_views) {
    IVX_REQUIRE(c->cull_state, IVX_ERR_STATE, "%s: nothing has been culled on this context", who);
    CullState* st = static_cast<CullState*>(c->cull_state);
    IVX_REQUIRE(n_views == st->n_views, IVX_ERR_INVALID, "%s: the last call had %u views, not %zu", who, st->n_views, n_views);
    if (n_views) IVX_HIP_CHECK(ivx_memcpy_async(out_counts, st->counts.p, n_views * sizeof(ivx_cull_count), hipMemcpyDeviceToHost, c->stream));
    IVX_HIP_CHECK(ivx_stream_sync(c->stream));
    return IVX_OK;
}

int check_common(const char* who, const void* ctx_or_grids, size_t n_obj, size_t n_views, uint32_t mode) {
    IVX_REQUIRE(ctx_or_grids, IVX_ERR_INVALID, "%s: null argument", who);
    IVX_REQUIRE(n_views <= MAX_VIEWS, IVX_ERR_INVALID, "%s: %zu views exceed %u per call", who, n_views, MAX_VIEWS);
    IVX_REQUIRE(mode <= 1u, IVX_ERR_INVALID, "%s: mode %u (0 = zeroed in place, 1 = compacted)", who, mode);
    IVX_REQUIRE(n_obj < (1u << 24), IVX_ERR_CAPACITY, "%s: %zu objects exceed 2^24", who, n_obj);
    return IVX_OK;
}

// the resident tables of `n` grids of one context (live entries only)
int resident_tables(const char* who, ivx_grid* const* grids, size_t n, std::vector<const ivx_submesh*>& tables, std::vector<uint32_t>& counts, std::vector<float>& extents) {
    tables.resize(n), counts.resize(n), extents.resize(n);
    for (size_t i = 0; i < n; ++i) {
        IVX_REQUIRE(grids[i], IVX_ERR_INVALID, "%s: object %zu is null", who, i);
        IVX_REQUIRE(grids[i]->ctx == grids[0]->ctx, IVX_ERR_INVALID, "%s: object %zu belongs to another context", who, i);
        IVX_REQUIRE(grids[i]->mesh_valid, IVX_ERR_STATE, "%s: object %zu has no current mesh (call ivx_remesh or ivx_mesh_sync first)", who, i);
        tables[i] = grids[i]->submeshes, counts[i] = grids[i]->mesh_counts.n_submeshes, extents[i] = (float)IVX_CHUNK * grids[i]->extent;
    }
    return IVX_OK;
}

// `records`: ready frustum records with view_flags / pair_flags in place of views and pairs. n == 0 (a frame without voxel objects): empty regions and
// zero counts, written here — no object names a context, and none is needed
int many_enqueue(const char* who, ivx_grid* const* grids, size_t n, const ivx_cull_object* objects, bool records, const ivx_cull_view* views, size_t n_views,
                 const ivx_cull_pair* pairs, const ivx_culling_frustum* frusta, const uint32_t* view_flags, const uint32_t* pair_flags, uint32_t mode,
                 ivx_cull_region* out_layout, ivx_cull_count* out_counts, ivx_ctx** ctx_out, bool resident = false, const uint32_t* object_indices = nullptr) {
    *ctx_out = nullptr;
    IVX_REQUIRE(n_views <= MAX_VIEWS, IVX_ERR_INVALID, "%s: %zu views exceed %u per call", who, n_views, MAX_VIEWS);
    IVX_REQUIRE(mode <= 1u, IVX_ERR_INVALID, "%s: mode %u (0 = zeroed in place, 1 = compacted)", who, mode);
    IVX_REQUIRE(n < (1u << 24), IVX_ERR_CAPACITY, "%s: %zu objects exceed 2^24", who, n);
    IVX_REQUIRE(grids || n == 0, IVX_ERR_INVALID, "%s: null object list", who);
    if (records)
        IVX_REQUIRE(n_views == 0 || (view_flags && (frusta || n == 0)), IVX_ERR_INVALID, "%s: null argument", who);
    else
        IVX_REQUIRE(n_views == 0 || (views && (pairs || n == 0 || resident)), IVX_ERR_INVALID, "%s: null argument", who);
    if (!records)
        for (size_t v = 0; v < n_views; ++v)
            IVX_REQUIRE(views[v].kind <= 1u, IVX_ERR_INVALID, "%s: view %zu has kind %u (0 = frustum planes, 1 = orthographic box)", who, v, views[v].kind);
    if (n == 0) {
        for (size_t v = 0; v < n_views; ++v) {
            const bool indexed = ((records ? view_flags[v] : views[v].flags) & IVX_CULL_VIEW_INDEXED) != 0u;
            out_layout[v].offset = 0, out_layout[v].stride = indexed ? 20u : 16u, out_layout[v].n_slots = 0;
            if (out_counts) out_counts[v].draws = 0, out_counts[v].indices = 0;
        }
        return IVX_OK;
    }
    std::vector<const ivx_submesh*> tables;
    std::vector<uint32_t> counts;
    std::vector<float> extents;
    if (int rc = resident_tables(who, grids, n, tables, counts, extents)) return rc;
    if (!records && n_views)
        if (int rc = check_views_and_pairs(who, views, n_views, pairs, extents.data(), n)) return rc;
    ivx_ctx* c = grids[0]->ctx;
    const ivx_cull_pair* fi_pairs = nullptr;
    uint32_t fi_n = 0;
    if (resident) {
        if (int rc = ivx_fi_resident_pairs(c, who, n_views, &fi_pairs, &fi_n)) return rc;
        for (size_t g = 0; g < n; ++g) {
            const size_t o = object_indices ? object_indices[g] : g;
            IVX_REQUIRE(o < fi_n, IVX_ERR_INVALID, "%s: object %zu takes the pairs of instance %zu, the context's frame instances have %u", who, g, o, fi_n);
        }
    }
    *ctx_out = c;
    ivx_many_other_context other_(c);
    const CullJob j = {who, n, n_views, tables.data(), nullptr, counts.data(), extents.data(), objects, views, pairs, records, frusta, view_flags, pair_flags, mode,
                       n_views ? fi_pairs : nullptr, fi_n, object_indices};
    return cull_enqueue(c, j, out_layout);
}

}  // namespace

void ivx_cull_release(ivx_ctx* c) {
    CullState* s = c ? ivx_state_take<CullState>(&c->cull_state) : nullptr;
    if (!s) return;
    for (ivx_buf* b : {&s->args, &s->frusta, &s->scratch, &s->counts}) ivx_buf_free(b);
    ivx_staging_release(&s->staging);
    delete s;
}

extern "C" {

int ivx_culling_frustum_from_view(const ivx_cull_view* view, const ivx_cull_pair* pair, float chunk_extent, ivx_culling_frustum* out) {
    IVX_REQUIRE(view && pair && out, IVX_ERR_INVALID, "ivx_culling_frustum_from_view: null argument");
    if (int rc = check_views_and_pairs("ivx_culling_frustum_from_view", view, 1, pair, &chunk_extent, 1)) return rc;
    derive_frustum(view, pair, chunk_extent, out);
    return IVX_OK;
}

int ivx_cull_frusta(ivx_ctx* c, const ivx_cull_view* views, size_t n_views, const ivx_cull_pair* pairs, const float* chunk_extents, size_t n_objects,
                    ivx_culling_frustum* out) {
    if (int rc = check_common("ivx_cull_frusta", c, n_objects, n_views, 0u)) return rc;
    const size_t n_pairs = n_views * n_objects;
    if (n_pairs == 0) return IVX_OK;
    IVX_REQUIRE(views && pairs && chunk_extents && out, IVX_ERR_INVALID, "ivx_cull_frusta: null argument");
    if (int rc = check_views_and_pairs("ivx_cull_frusta", views, n_views, pairs, chunk_extents, n_objects)) return rc;
    ivx_many_other_context other_(c);
    // the derivation stage of a cull over objects without submeshes
    std::vector<uint32_t> counts(n_objects, 0u);
    std::vector<const ivx_submesh*> tables(n_objects, nullptr);
    const CullJob j = {"ivx_cull_frusta", n_objects, n_views, nullptr, tables.data(), counts.data(), chunk_extents, nullptr, views, pairs, false, nullptr, nullptr, nullptr, 0u};
    if (int rc = cull_enqueue(c, j, nullptr)) return rc;
    CullState* st = static_cast<CullState*>(c->cull_state);
    IVX_HIP_CHECK(ivx_memcpy_async(out, st->frusta.p, n_pairs * sizeof(ivx_culling_frustum), hipMemcpyDeviceToHost, c->stream));
    IVX_HIP_CHECK(ivx_stream_sync(c->stream));
    return IVX_OK;
}

int ivx_cull_submesh_tables(ivx_ctx* c, const ivx_submesh* const* tables, const uint32_t* counts, size_t n_objects, const ivx_cull_object* objects,
                            const float* chunk_extents, const ivx_cull_view* views, size_t n_views, const ivx_cull_pair* pairs, uint32_t mode, ivx_cull_region* out_layout,
                            ivx_cull_count* out_counts) {
    const char* who = "ivx_cull_submesh_tables";
    if (int rc = check_common(who, c, n_objects, n_views, mode)) return rc;
    IVX_REQUIRE((tables && counts && chunk_extents) || n_objects == 0, IVX_ERR_INVALID, "%s: null argument", who);
    IVX_REQUIRE((views && out_layout && out_counts) || n_views == 0, IVX_ERR_INVALID, "%s: null argument", who);
    IVX_REQUIRE(pairs || n_views * n_objects == 0, IVX_ERR_INVALID, "%s: null argument", who);
    for (size_t o = 0; o < n_objects; ++o) IVX_REQUIRE(tables[o] || counts[o] == 0, IVX_ERR_INVALID, "%s: the table of object %zu is null", who, o);
    if (int rc = check_views_and_pairs(who, views, n_views, pairs, chunk_extents, n_views ? n_objects : 0)) return rc;
    ivx_many_other_context other_(c);
    const CullJob j = {who, n_objects, n_views, nullptr, tables, counts, chunk_extents, objects, views, pairs, false, nullptr, nullptr, nullptr, mode};
    if (int rc = cull_enqueue(c, j, out_layout)) return rc;
    return cull_collect(c, who, out_counts, n_views);
}

int ivx_cull_submesh_tables_frusta(ivx_ctx* c, const ivx_submesh* const* tables, const uint32_t* counts, size_t n_objects, const ivx_cull_object* objects,
                                   const ivx_culling_frustum* frusta, const uint32_t* view_flags, const uint32_t* pair_flags, size_t n_views, uint32_t mode,
                                   ivx_cull_region* out_layout, ivx_cull_count* out_counts) {
    const char* who = "ivx_cull_submesh_tables_frusta";
    if (int rc = check_common(who, c, n_objects, n_views, mode)) return rc;
    IVX_REQUIRE((tables && counts) || n_objects == 0, IVX_ERR_INVALID, "%s: null argument", who);
    IVX_REQUIRE((view_flags && out_layout && out_counts) || n_views == 0, IVX_ERR_INVALID, "%s: null argument", who);
    IVX_REQUIRE(frusta || n_views * n_objects == 0, IVX_ERR_INVALID, "%s: null argument", who);
    for (size_t o = 0; o < n_objects; ++o) IVX_REQUIRE(tables[o] || counts[o] == 0, IVX_ERR_INVALID, "%s: the table of object %zu is null", who, o);
    ivx_many_other_context other_(c);
    const CullJob j = {who, n_objects, n_views, nullptr, tables, counts, nullptr, objects, nullptr, nullptr, true, frusta, view_flags, pair_flags, mode};
    if (int rc = cull_enqueue(c, j, out_layout)) return rc;
    return cull_collect(c, who, out_counts, n_views);
}

int ivx_cull_many_enqueue(ivx_grid* const* grids, size_t n, const ivx_cull_object* objects, const ivx_cull_view* views, size_t n_views, const ivx_cull_pair* pairs,
                          uint32_t mode, ivx_cull_region* out_layout) {
    IVX_REQUIRE(out_layout || n_views == 0, IVX_ERR_INVALID, "ivx_cull_many_enqueue: null argument");
    ivx_ctx* c = nullptr;
    return many_enqueue("ivx_cull_many_enqueue", grids, n, objects, false, views, n_views, pairs, nullptr, nullptr, nullptr, mode, out_layout, nullptr, &c);
}

int ivx_cull_many_resident(ivx_grid* const* grids, size_t n, const ivx_cull_object* objects, const uint32_t* object_indices, const ivx_cull_view* views, size_t n_views,
                           uint32_t mode, ivx_cull_region* out_layout) {
    IVX_REQUIRE(out_layout || n_views == 0, IVX_ERR_INVALID, "ivx_cull_many_resident: null argument");
    ivx_ctx* c = nullptr;
    return many_enqueue("ivx_cull_many_resident", grids, n, objects, false, views, n_views, nullptr, nullptr, nullptr, nullptr, mode, out_layout, nullptr, &c, true, object_indices);
}

int ivx_cull_collect(ivx_ctx* c, ivx_cull_count* out_counts, size_t n_views) {
    IVX_REQUIRE(c && (out_counts || n_views == 0), IVX_ERR_INVALID, "ivx_cull_collect: null argument");
    ivx_many_other_context other_(c);
    return cull_collect(c, "ivx_cull_collect", out_counts, n_views);
}

int ivx_cull_many(ivx_grid* const* grids, size_t n, const ivx_cull_object* objects, const ivx_cull_view* views, size_t n_views, const ivx_cull_pair* pairs, uint32_t mode,
                  ivx_cull_region* out_layout, ivx_cull_count* out_counts) {
    IVX_REQUIRE((out_layout && out_counts) || n_views == 0, IVX_ERR_INVALID, "ivx_cull_many: null argument");
    ivx_ctx* c = nullptr;
    if (int rc = many_enqueue("ivx_cull_many", grids, n, objects, false, views, n_views, pairs, nullptr, nullptr, nullptr, mode, out_layout, out_counts, &c)) return rc;
    if (!c) return IVX_OK;  // (no objects)
    ivx_many_other_context other_(c);
    return cull_collect(c, "ivx_cull_many", out_counts, n_views);
}

int ivx_cull_many_frusta(ivx_grid* const* grids, size_t n, const ivx_cull_object* objects, const ivx_culling_frustum* frusta, const uint32_t* view_flags,
                         const uint32_t* pair_flags, size_t n_views, uint32_t mode, ivx_cull_region* out_layout, ivx_cull_count* out_counts) {
    IVX_REQUIRE((out_layout && out_counts) || n_views == 0, IVX_ERR_INVALID, "ivx_cull_many_frusta: null argument");
    ivx_ctx* c = nullptr;
    if (int rc = many_enqueue("ivx_cull_many_frusta", grids, n, objects, true, nullptr, n_views, nullptr, frusta, view_flags, pair_flags, mode, out_layout, out_counts, &c)) return rc;
    if (!c) return IVX_OK;  // (no objects)
    ivx_many_other_context other_(c);
    return cull_collect(c, "ivx_cull_many_frusta", out_counts, n_views);
}

int ivx_cull_download(ivx_ctx* c, uint32_t view, void* args, size_t args_bytes, ivx_cull_count* count, ivx_culling_frustum* frusta, size_t n_frusta) {
    IVX_REQUIRE(c, IVX_ERR_INVALID, "ivx_cull_download: null argument");
    IVX_REQUIRE(c->cull_state, IVX_ERR_STATE, "ivx_cull_download: nothing has been culled on this context");
    CullState* st = static_cast<CullState*>(c->cull_state);
    IVX_REQUIRE(view < st->n_views, IVX_ERR_INVALID, "ivx_cull_download: view %u, the last call had %u", view, st->n_views);
    const ivx_cull_region& r = st->regions[view];
    const size_t region_bytes = (size_t)r.n_slots * r.stride;
    IVX_REQUIRE(!args || args_bytes >= region_bytes, IVX_ERR_CAPACITY, "ivx_cull_download: the region of view %u is %zu bytes, the buffer %zu", view, region_bytes, args_bytes);
    IVX_REQUIRE(!frusta || n_frusta >= st->n_obj, IVX_ERR_CAPACITY, "ivx_cull_download: a view has %u frustum records, the buffer holds %zu", st->n_obj, n_frusta);
    ivx_many_other_context other_(c);
    if (args && region_bytes) IVX_HIP_CHECK(ivx_memcpy_async(args, static_cast<char*>(st->args.p) + r.offset, region_bytes, hipMemcpyDeviceToHost, c->stream));
    if (count) IVX_HIP_CHECK(ivx_memcpy_async(count, static_cast<ivx_cull_count*>(st->counts.p) + view, sizeof(ivx_cull_count), hipMemcpyDeviceToHost, c->stream));
    if (frusta && st->n_obj)
        IVX_HIP_CHECK(ivx_memcpy_async(frusta, static_cast<ivx_culling_frustum*>(st->frusta.p) + (size_t)view * st->n_obj, st->n_obj * sizeof(ivx_culling_frustum),
                                       hipMemcpyDeviceToHost, c->stream));
    IVX_HIP_CHECK(ivx_stream_sync(c->stream));
    return IVX_OK;
}

void* ivx_cull_device_ptr(ivx_ctx* c, int which) {
    if (!c || !c->cull_state) return nullptr;
    CullState* st = static_cast<CullState*>(c->cull_state);
    switch (which) {
        case IVX_CULL_PTR_ARGS: return st->args.p;
        case IVX_CULL_PTR_COUNTS: return st->counts.p;  // (null only if the first enqueue could not make it)
        case IVX_CULL_PTR_FRUSTA: return st->frusta.p;
        default: return nullptr;
    }
}

}  // extern "C"
