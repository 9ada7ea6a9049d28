// Bounding volumes: the world-space boxes of a frame's objects, every intersecting pair of them, and region queries over them.
//
// Reference: impact_intersection/src/lib.rs (IntersectionManager: add_bounding_volume_to_hierarchy :39-54, total_bounding_volume, for_each_*),
//   impact_geometry/src/axis_aligned_box.rs:350-363 (aabb_of_transformed), :619-623 (box_lies_outside), sphere.rs:167-181, frustum.rs:456-471,
//   oriented_box.rs:129-143, impact_physics/src/collision.rs:215-262, 317-349 (which pairs a frame asks for), impact_voxel/src/object.rs:886-907 and
//   interaction.rs:202-222 (a voxel object's entry). The reference answers all of these from a bounding volume hierarchy; its tests and fuzz targets
//   use the `_brute_force` forms as ground truth. This file IS the brute-force form: no hierarchy, no sort, no atomics (the hierarchy: bvh.hip).
//
// WORLD — k_bv_world, one wave per 64 consecutive objects: a lane derives its object's world box (ivx_bv_world_aabb_of, the very function the host
//   export runs) or takes it as given, then a shuffle min / max tree in input order leaves the block's box. Minima and maxima are taken in the total
//   order of the bit patterns (-0.0 below +0.0), which keeps the block test below conservative under the sign-bit decision; a box with a NaN bound
//   intersects nothing and stays out of the block box. k_bv_total, one wave: the box around the block boxes.
// COUNT — k_bv_pair_walk<false>: a wave owns the row block of 64 objects (a row's box per lane, in registers) x one column segment of SEG_BLOCKS
//   column blocks. Per column block at or right of the diagonal: skipped when the two block boxes lie outside each other (wave-uniform, a scalar
//   branch); else the 64 column boxes are walked — their addresses depend on the block and the loop counter only, so they arrive by scalar loads, no
//   LDS — and each lane tests its row, with b > a and the mode's kind filter. Leaves count[segment][row].
// ROWS, SCAN — k_bv_rows, one lane per row: exclusive prefix over the row's segments in place, and the row's total. k_bv_scan, one workgroup:
//   exclusive prefix of the row totals, SCAN_ROUND rows a round with a carry. (row, segment) in row-major order IS the lexicographic order of (a, b).
//   The host reads the grand total (the call's one wait before the emit), grows the pair buffer and launches
// EMIT — k_bv_pair_walk<true>: the same walk; each lane writes its hits from its own offset in column order.
// QUERY — k_bv_query, one wave per 64 consecutive objects, a world box per lane: walks the queries (the record's address is wave-uniform: scalar
//   loads), __ballot is the mask word of (query, tile). k_bv_query_counts, one wave per query: the popcounts of its words. The call's two halves
//   (upload and buffers; counts, download and wait) are shared with bvh.hip's form, which fills the masks through the tree instead.
// LISTS — ivx_bv_query_lists: the resident masks of either form as per-query object lists; the four kernels are described where they stand.
#include <cmath>
#include <vector>

#include "bvol_internal.hpp"
#include "device_common.hpp"

namespace {

constexpr uint32_t SEG_BLOCKS = 8;     // column blocks per segment (512 columns)
constexpr uint32_t SCAN_ROUND = 1024;  // rows per round of k_bv_scan (its workgroup)

// ---- device side (the box rules: bvol_internal.hpp) ------------------------------------------------------------------------------------------
// ivx_bv_lies_outside's rule, as six differences into ivx_bv_any_negative (the form k_bv_pair_walk is measured with)
__device__ __forceinline__ bool lies_outside(const ivx_aabb& self, const ivx_aabb& other) {
    return ivx_bv_any_negative(other.upper[0] - self.lower[0], other.upper[1] - self.lower[1], other.upper[2] - self.lower[2], self.upper[0] - other.lower[0],
                               self.upper[1] - other.lower[1], self.upper[2] - other.lower[2]);
}
// ivx_bv_has_nan's rule, as three unordered pairs
__device__ __forceinline__ bool has_nan(const ivx_aabb& b) {
    return __builtin_isunordered(b.lower[0], b.lower[1]) || __builtin_isunordered(b.lower[2], b.upper[0]) || __builtin_isunordered(b.upper[1], b.upper[2]);
}
// (stays: k_bv_world's code differs when it calls ivx_bv_world_aabb_of without this forced-inline step in between)
__device__ __forceinline__ void world_aabb(const ivx_aabb& m, const ivx_similarity& s, ivx_aabb* out) { ivx_bv_world_aabb_of(m, s, out); }
// min / max over the wave, lane l with lane l ^ d, d = 1, 2, .. 32: every lane ends with the result
__device__ __forceinline__ ivx_aabb wave_union(ivx_aabb b) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            b.lower[k] = ivx_bv_order_min(b.lower[k], __shfl_xor(b.lower[k], d, 64));
            b.upper[k] = ivx_bv_order_max(b.upper[k], __shfl_xor(b.upper[k], d, 64));
        }
    return b;
}
__device__ __forceinline__ uint32_t wave_index() { return (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6))); }

template <bool DERIVE>
__global__ __launch_bounds__(256) void k_bv_world(const ivx_aabb* __restrict__ model, const ivx_similarity* __restrict__ sims, uint32_t n, ivx_aabb* __restrict__ world,
                                                  ivx_aabb* __restrict__ blocks) {
    const uint32_t lane = threadIdx.x & 63u, blk = wave_index();
    if (blk * 64u >= n) return;  // (whole waves)
    const uint32_t o = blk * 64u + lane;
    ivx_aabb b = ivx_bv_neutral_box();
    if (o < n) {
        if (DERIVE) world_aabb(model[o], sims[o], &b);
        else b = model[o];
    }
    world[o] = b;  // (the buffer holds whole blocks: the slots behind n get the neutral box, which the pair walk reads and finds outside)
    if (has_nan(b)) b = ivx_bv_neutral_box();
    b = wave_union(b);
    if (lane == 0u) blocks[blk] = b;
}

__global__ __launch_bounds__(64) void k_bv_total(const ivx_aabb* __restrict__ blocks, uint32_t n_blocks, ivx_aabb* __restrict__ total) {
    const uint32_t lane = threadIdx.x;
    ivx_aabb t = ivx_bv_neutral_box();
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += 64u)
        if (b0 + lane < n_blocks) ivx_bv_union(&t, blocks[b0 + lane]);
    t = wave_union(t);
    ivx_bv_frame_finish(&t);  // (no box without a NaN bound at all)
    if (lane == 0u) *total = t;
}

// counts: [n_seg][n]. EMIT: counts hold the exclusive prefix over a row's segments, row_base the exclusive prefix of the row totals
template <bool EMIT>
__global__ __launch_bounds__(256) void k_bv_pair_walk(const ivx_aabb* __restrict__ world, const uint32_t* __restrict__ kinds, const ivx_aabb* __restrict__ blocks, uint32_t n,
                                                      uint32_t n_blocks, uint32_t n_seg, uint32_t mode, uint32_t* __restrict__ counts, const uint32_t* __restrict__ row_base,
                                                      uint2* __restrict__ pairs) {
    const uint32_t lane = threadIdx.x & 63u, w = wave_index();
    if (w >= n_blocks * n_seg) return;  // (whole waves; n_blocks x n_seg <= 2^14 x 2^11)
    const uint32_t rb = w / n_seg, seg = w - rb * n_seg;
    const uint32_t cb_end = min(n_blocks, (seg + 1u) * SEG_BLOCKS);
    if (cb_end <= rb) return;  // wholly left of the diagonal: k_bv_rows starts behind these segments
    const uint32_t row = rb * 64u + lane;
    const bool live = row < n;
    ivx_aabb self = ivx_bv_neutral_box();
    uint32_t row_kind = 0u;
    if (live) self = world[row], row_kind = kinds[row];
    const bool row_ok = live & ((mode == 0u) | (row_kind != IVX_BV_PHANTOM));
    const size_t slot = (size_t)seg * n + row;
    uint32_t count = 0u, at = 0u;
    if (EMIT && live) at = row_base[row] + counts[slot];
    const ivx_aabb row_block = blocks[rb];
    for (uint32_t cb = max(seg * SEG_BLOCKS, rb); cb < cb_end; ++cb) {
        const ivx_aabb col_block = blocks[cb];
        if (lies_outside(row_block, col_block)) continue;  // wave-uniform
        const uint32_t b0 = cb * 64u;
#pragma unroll 8
        for (uint32_t j = 0; j < 64u; ++j) {  // (whole blocks: see k_bv_world)
            const uint32_t b = b0 + j;
            const ivx_aabb other = world[b];  // (uniform address)
            const uint32_t col_kind = kinds[b];
            const bool kinds_ok = (mode == 0u) | ((col_kind != IVX_BV_PHANTOM) & ((col_kind == IVX_BV_DYNAMIC) | (row_kind == IVX_BV_DYNAMIC)));
            const bool hit = (b > row) & row_ok & kinds_ok & !lies_outside(self, other);
            if (EMIT) {
                if (hit) pairs[at++] = make_uint2(row, b);
            } else {
                count += hit ? 1u : 0u;
            }
        }
    }
    if (!EMIT && live) counts[slot] = count;
}

__global__ __launch_bounds__(256) void k_bv_rows(uint32_t* __restrict__ counts, uint32_t n, uint32_t n_seg, uint32_t* __restrict__ row_total) {
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row >= n) return;
    uint32_t run = 0u;
    for (uint32_t seg = (row >> 6) / SEG_BLOCKS; seg < n_seg; ++seg) {
        const size_t slot = (size_t)seg * n + row;
        const uint32_t c = counts[slot];
        counts[slot] = run;
        run += c;
    }
    row_total[row] = run;
}

// in place: row_total -> exclusive prefix (mod 2^32; the host refuses a grand total of 2^31 or more before anything reads it)
__global__ __launch_bounds__(SCAN_ROUND) void k_bv_scan(uint32_t* __restrict__ row_total, uint32_t n, unsigned long long* __restrict__ grand_total) {
    __shared__ uint32_t wave_totals[SCAN_ROUND / 64u];
    const unsigned long long total = ivx_scan_rounds<SCAN_ROUND, unsigned long long>(row_total, row_total, n, wave_totals);
    if (threadIdx.x == 0u) *grand_total = total;
}

__global__ __launch_bounds__(256) void k_bv_query(const ivx_aabb* __restrict__ world, uint32_t n, const ivx_bv_query* __restrict__ queries, uint32_t n_queries,
                                                  unsigned long long* __restrict__ masks) {
    const uint32_t lane = threadIdx.x & 63u, tile = wave_index();
    const uint32_t n_words = (n + 63u) / 64u;
    if (tile >= n_words) return;  // (whole waves)
    const uint32_t o = tile * 64u + lane;
    const bool live = o < n;
    ivx_aabb b = ivx_bv_neutral_box();
    if (live) b = world[o];
    float c[3], h[3];
    ivx_bv_center_half(b, c, h);
    for (uint32_t q = 0; q < n_queries; ++q) {
        const bool hit = live && ivx_bv_query_hits(queries + q, b, c, h);  // (bvol_internal.hpp: the hierarchy's walk decides its leaves with it too)
        const unsigned long long mask = __ballot(hit);
        if (lane == 0u) masks[(size_t)q * n_words + tile] = mask;
    }
}

__global__ __launch_bounds__(64) void k_bv_query_counts(const unsigned long long* __restrict__ masks, uint32_t n_words, uint32_t* __restrict__ counts) {
    const uint32_t lane = threadIdx.x, q = blockIdx.x;
    const unsigned long long* __restrict__ m = masks + (size_t)q * n_words;
    uint32_t c = 0u;
    for (uint32_t w0 = 0; w0 < n_words; w0 += 64u)
        if (w0 + lane < n_words) c += (uint32_t)__popcll(m[w0 + lane]);
    c = ivx_wave_sum(c);
    if (lane == 0u) counts[q] = c;
}

// LISTS — the resident masks as hit lists, every position a prefix of popcounts (no sort, no atomic). k_bv_list_words, a lane per mask word: its
//   popcount. k_bv_list_rows, a workgroup per query: the exclusive prefix over the query's words in place, and the query's total. k_bv_list_offsets,
//   one workgroup: the exclusive prefix of the totals, offsets[n_queries] and the grand total. k_bv_list_emit, a lane per mask word again: the
//   objects of its set bits, ascending, from offsets[q] + the word's prefix.
__global__ __launch_bounds__(256) void k_bv_list_words(const unsigned long long* __restrict__ masks, uint32_t n_all_words, uint32_t* __restrict__ prefix) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_all_words) prefix[i] = (uint32_t)__popcll(masks[i]);
}

__global__ __launch_bounds__(SCAN_ROUND) void k_bv_list_rows(uint32_t* __restrict__ prefix, uint32_t n_words, uint32_t* __restrict__ totals) {
    __shared__ uint32_t wave_totals[SCAN_ROUND / 64u];
    uint32_t* row = prefix + (size_t)blockIdx.x * n_words;
    const uint32_t total = ivx_scan_rounds<SCAN_ROUND, uint32_t>(row, row, n_words, wave_totals);  // (at most 2^20 objects a query)
    if (threadIdx.x == 0u) totals[blockIdx.x] = total;
}

// offsets[n_queries + 1] (at most 2^10 queries of at most 2^20 objects: no 32-bit sum overflows)
__global__ __launch_bounds__(SCAN_ROUND) void k_bv_list_offsets(const uint32_t* __restrict__ totals, uint32_t n_queries, uint32_t* __restrict__ offsets) {
    __shared__ uint32_t wave_totals[SCAN_ROUND / 64u];
    const uint32_t total = ivx_scan_rounds<SCAN_ROUND, uint32_t>(totals, offsets, n_queries, wave_totals);
    if (threadIdx.x == 0u) offsets[n_queries] = total;
}

__global__ __launch_bounds__(256) void k_bv_list_emit(const unsigned long long* __restrict__ masks, uint32_t n_words, uint32_t n_all_words, const uint32_t* __restrict__ prefix,
                                                      const uint32_t* __restrict__ offsets, uint32_t n_hits, uint32_t* __restrict__ objects) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_all_words) return;
    const uint32_t q = i / n_words, w = i - q * n_words;
    unsigned long long word = masks[i];
    uint32_t at = offsets[q] + prefix[i];
    while (word != 0ull) {
        const uint32_t bit = (uint32_t)__ffsll((long long)word) - 1u;
        if (at < n_hits) objects[at] = w * 64u + bit;  // (always: the prefix came from these very words)
        ++at;
        word &= word - 1ull;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
// context-owned state: device buffers that only grow, a pinned staging block for the one upload of a call (device_common.hpp), and the set the context holds
struct BvState {
    ivx_buf set;      // input boxes | similarities || kinds | world boxes | block boxes | total  (the part before || is the upload's scratch)
    ivx_buf scratch;  // pairs: counts | row totals | grand total;  queries: records | counts
    ivx_buf pairs, masks;
    ivx_buf lists;  // ivx_bv_query_lists: per-word prefixes | per-query totals | offsets
    ivx_buf hits;   // ... and the objects
    ivx_staging staging;
    bool has_set = false;
    uint32_t n = 0;
    bool queried = false;      // a queries call (either form) has left masks of the set that stands
    uint32_t n_queried = 0;    // ... of this many queries
    size_t o_list_offsets = 0;  // where `lists` holds the offsets of the last ivx_bv_query_lists (n_listed != 0)
    uint32_t n_listed = 0;
    uint64_t serial = 0;  // counts the sets the context has held (ivx_bvol_set_serial)
    void* hierarchy = nullptr;  // bvh.hip's state: a tree over one of those sets
    size_t o_kinds = 0, o_world = 0, o_blocks = 0, o_total = 0;
};

int state_of(ivx_ctx* c, BvState** out) { return ivx_state_for(&c->bvol_state, "bounding volumes", out); }

int check_set_arguments(const char* who, const ivx_similarity* sims, const uint32_t* kinds, size_t n) {
    IVX_REQUIRE(n <= IVX_BV_MAX_OBJECTS, IVX_ERR_CAPACITY, "%s: %zu objects exceed %u", who, n, IVX_BV_MAX_OBJECTS);
    for (size_t o = 0; o < n && sims; ++o)
        IVX_REQUIRE(sims[o].scaling > 0.0f, IVX_ERR_INVALID, "%s: the scaling %g of object %zu is not positive", who, (double)sims[o].scaling, o);
    for (size_t o = 0; o < n && kinds; ++o)
        IVX_REQUIRE(kinds[o] <= IVX_BV_PHANTOM, IVX_ERR_INVALID, "%s: object %zu has kind %u (0 dynamic, 1 static, 2 phantom)", who, o, kinds[o]);
    return IVX_OK;
}

// the set buffer of n objects: the inputs of the world launch (boxes, similarities if any, kinds), then what the set keeps
struct SetLayout {
    size_t o_in = 0, o_sims = 0, o_kinds = 0, upload_bytes = 0, o_world = 0, o_blocks = 0, o_total = 0, bytes = 0;
};
SetLayout set_layout(size_t n, bool with_sims) {
    const size_t n_blocks = (n + 63u) / 64u;
    ivx_layout l;
    SetLayout s;
    s.o_in = l.take(n * sizeof(ivx_aabb)), s.o_sims = l.take(with_sims ? n * sizeof(ivx_similarity) : 0), s.o_kinds = l.take(n_blocks * 64u * 4);  // (kinds and world boxes: whole blocks)
    s.upload_bytes = l.bytes;
    s.o_world = l.take(n_blocks * 64u * sizeof(ivx_aabb)), s.o_blocks = l.take(n_blocks * sizeof(ivx_aabb)), s.o_total = l.take(sizeof(ivx_aabb));
    s.bytes = l.bytes;
    return s;
}

// the launches behind the inputs, wherever they came from (an upload: set_enqueue; a kernel of the caller: ivx_bvol_set_finish)
int set_launch(ivx_ctx* c, BvState* st, const SetLayout& l, size_t n, bool derive) {
    const size_t n_blocks = (n + 63u) / 64u;
    char* d = static_cast<char*>(st->set.p);
    const dim3 grid((uint32_t)((n_blocks + 3u) / 4u));
    ivx_aabb* d_world = reinterpret_cast<ivx_aabb*>(d + l.o_world);
    ivx_aabb* d_blocks = reinterpret_cast<ivx_aabb*>(d + l.o_blocks);
    if (derive)
        IVX_KLAUNCH(k_bv_world<true>, grid, dim3(256), 0, c->stream, reinterpret_cast<const ivx_aabb*>(d + l.o_in), reinterpret_cast<const ivx_similarity*>(d + l.o_sims), (uint32_t)n,
                    d_world, d_blocks);
    else
        IVX_KLAUNCH(k_bv_world<false>, grid, dim3(256), 0, c->stream, reinterpret_cast<const ivx_aabb*>(d + l.o_in), (const ivx_similarity*)nullptr, (uint32_t)n, d_world, d_blocks);
    IVX_KLAUNCH(k_bv_total, dim3(1), dim3(64), 0, c->stream, (const ivx_aabb*)d_blocks, (uint32_t)n_blocks, reinterpret_cast<ivx_aabb*>(d + l.o_total));
    IVX_HIP_CHECK(hipGetLastError());
    st->o_kinds = l.o_kinds, st->o_world = l.o_world, st->o_blocks = l.o_blocks, st->o_total = l.o_total;
    st->n = (uint32_t)n, st->has_set = true, ++st->serial;
    return IVX_OK;
}

int set_enqueue(ivx_ctx* c, const ivx_aabb* boxes, const ivx_similarity* sims, const uint32_t* kinds, size_t n) {
    BvState* st;
    if (int rc = state_of(c, &st)) return rc;
    st->has_set = false, st->n = 0, st->queried = false, st->n_listed = 0u;  // (until this call's set stands)
    if (n == 0) {
        st->has_set = true, ++st->serial;
        return IVX_OK;
    }
    const size_t n_blocks = (n + 63u) / 64u;
    const SetLayout l = set_layout(n, sims != nullptr);
    if (int rc = ivx_staging_for(&st->staging, l.upload_bytes)) return rc;
    if (int rc = ivx_buf_grow(c, &st->set, l.bytes, 1u << 16)) return rc;
    char* h = static_cast<char*>(st->staging.p);
    memcpy(h + l.o_in, boxes, n * sizeof(ivx_aabb));
    if (sims) memcpy(h + l.o_sims, sims, n * sizeof(ivx_similarity));
    memset(h + l.o_kinds, 0, n_blocks * 64u * 4);
    if (kinds) memcpy(h + l.o_kinds, kinds, n * 4);
    if (int rc = ivx_staging_upload(&st->staging, st->set.p, l.upload_bytes, c->stream)) return rc;
    return set_launch(c, st, l, n, sims != nullptr);
}

int model_aabb(ivx_grid* g, const char* who, ivx_aabb* out) {
    uint32_t occ[12];
    if (int rc = ivx_reference_occupied(g, who, occ)) return rc;
    bool empty = false;
    for (int d = 0; d < 3; ++d) empty = empty || occ[6 + 2 * d] >= occ[7 + 2 * d];
    for (int d = 0; d < 3; ++d) {
        out->lower[d] = empty ? 0.0f : (float)occ[6 + 2 * d] * g->extent;
        out->upper[d] = empty ? 0.0f : (float)occ[7 + 2 * d] * g->extent;
    }
    return IVX_OK;
}

int set_state(ivx_ctx* c, const char* who, BvState** out) {
    IVX_REQUIRE(c, IVX_ERR_INVALID, "%s: null context", who);
    BvState* st = static_cast<BvState*>(c->bvol_state);
    IVX_REQUIRE(st && st->has_set, IVX_ERR_STATE, "%s: the context holds no set of bounding volumes (call ivx_bv_set or ivx_bv_set_grids first)", who);
    *out = st;
    return IVX_OK;
}

}  // namespace

void ivx_bvol_release(ivx_ctx* c) {
    BvState* s = c ? ivx_state_take<BvState>(&c->bvol_state) : nullptr;
    if (!s) return;
    for (ivx_buf* b : {&s->set, &s->scratch, &s->pairs, &s->masks, &s->lists, &s->hits}) ivx_buf_free(b);
    ivx_staging_release(&s->staging);
    ivx_bvh_release(&s->hierarchy);
    delete s;
}

int ivx_bvol_view_of(ivx_ctx* c, const char* who, ivx_bvol_view* out) {
    BvState* st;
    if (int rc = set_state(c, who, &st)) return rc;
    const char* d = static_cast<const char*>(st->set.p);
    out->n = st->n, out->serial = st->serial, out->pairs = &st->pairs, out->hierarchy = &st->hierarchy;
    out->world = st->n ? reinterpret_cast<const ivx_aabb*>(d + st->o_world) : nullptr;
    out->kinds = st->n ? reinterpret_cast<const uint32_t*>(d + st->o_kinds) : nullptr;
    out->n_queried = st->queried ? st->n_queried : 0u;
    out->masks = st->queried && st->n ? static_cast<const unsigned long long*>(st->masks.p) : nullptr;
    return IVX_OK;
}

int ivx_bvol_set_begin(ivx_ctx* c, size_t n, ivx_aabb** d_boxes, uint32_t** d_kinds) {
    *d_boxes = nullptr, *d_kinds = nullptr;
    BvState* st;
    if (int rc = state_of(c, &st)) return rc;
    st->has_set = false, st->n = 0, st->queried = false, st->n_listed = 0u;  // (until ivx_bvol_set_finish)
    if (n == 0) return IVX_OK;
    const SetLayout l = set_layout(n, false);
    if (int rc = ivx_buf_grow(c, &st->set, l.bytes, 1u << 16)) return rc;
    char* d = static_cast<char*>(st->set.p);
    *d_boxes = reinterpret_cast<ivx_aabb*>(d + l.o_in), *d_kinds = reinterpret_cast<uint32_t*>(d + l.o_kinds);
    return IVX_OK;
}

int ivx_bvol_set_finish(ivx_ctx* c, size_t n) {
    BvState* st;
    if (int rc = state_of(c, &st)) return rc;
    if (n == 0) {
        st->has_set = true, ++st->serial;
        return IVX_OK;
    }
    return set_launch(c, st, set_layout(n, false), n, false);
}

uint64_t ivx_bvol_set_serial(const ivx_ctx* c) {
    const BvState* st = static_cast<const BvState*>(c->bvol_state);
    return st && st->has_set ? st->serial : 0u;
}

int ivx_bvol_pairs_enqueue(ivx_ctx* c, const char* who, uint32_t mode, bool check_cap, size_t cap, size_t* n_pairs) {
    *n_pairs = 0;
    BvState* st;
    if (int rc = set_state(c, who, &st)) return rc;
    const uint32_t n = st->n;
    if (n < 2u) return IVX_OK;
    const uint32_t n_blocks = (n + 63u) / 64u, n_seg = (n_blocks + SEG_BLOCKS - 1u) / SEG_BLOCKS;
    ivx_layout l;
    const size_t o_counts = l.take((size_t)n_seg * n * 4), o_rows = l.take((size_t)n * 4), o_grand = l.take(8);
    if (int rc = ivx_buf_grow(c, &st->scratch, l.bytes, 1u << 20)) return rc;
    char* s = static_cast<char*>(st->scratch.p);
    const char* d = static_cast<const char*>(st->set.p);
    const ivx_aabb* d_world = reinterpret_cast<const ivx_aabb*>(d + st->o_world);
    const ivx_aabb* d_blocks = reinterpret_cast<const ivx_aabb*>(d + st->o_blocks);
    const uint32_t* d_kinds = reinterpret_cast<const uint32_t*>(d + st->o_kinds);
    uint32_t* d_counts = reinterpret_cast<uint32_t*>(s + o_counts);
    uint32_t* d_rows = reinterpret_cast<uint32_t*>(s + o_rows);
    unsigned long long* d_grand = reinterpret_cast<unsigned long long*>(s + o_grand);
    const dim3 walk_grid((uint32_t)(((size_t)n_blocks * n_seg + 3u) / 4u));
    IVX_KLAUNCH(k_bv_pair_walk<false>, walk_grid, dim3(256), 0, c->stream, d_world, d_kinds, d_blocks, n, n_blocks, n_seg, mode, d_counts, (const uint32_t*)nullptr, (uint2*)nullptr);
    IVX_KLAUNCH(k_bv_rows, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, d_counts, n, n_seg, d_rows);
    IVX_KLAUNCH(k_bv_scan, dim3(1), dim3(SCAN_ROUND), 0, c->stream, d_rows, n, d_grand);
    IVX_HIP_CHECK(hipGetLastError());
    unsigned long long grand = 0;
    IVX_HIP_CHECK(ivx_memcpy_async(&grand, d_grand, 8, hipMemcpyDeviceToHost, c->stream));
    IVX_HIP_CHECK(ivx_stream_sync(c->stream));
    if (int rc = ivx_bvol_pairs_total(who, grand, check_cap, cap, n_pairs)) return rc;
    if (grand == 0) return IVX_OK;
    if (int rc = ivx_buf_grow(c, &st->pairs, (size_t)grand * 8, 1u << 16)) return rc;
    IVX_KLAUNCH(k_bv_pair_walk<true>, walk_grid, dim3(256), 0, c->stream, d_world, d_kinds, d_blocks, n, n_blocks, n_seg, mode, d_counts, (const uint32_t*)d_rows,
                static_cast<uint2*>(st->pairs.p));
    IVX_HIP_CHECK(hipGetLastError());
    return IVX_OK;
}

int ivx_bvol_pairs_check(const char* who, ivx_ctx* c, uint32_t mode, const uint32_t* pairs, size_t cap, size_t* n_out) {
    IVX_REQUIRE(n_out, IVX_ERR_INVALID, "%s: null argument", who);
    *n_out = 0;
    IVX_REQUIRE(c, IVX_ERR_INVALID, "%s: null context", who);
    IVX_REQUIRE(mode <= IVX_BV_DYNAMIC_PAIRS, IVX_ERR_INVALID, "%s: mode %u (0 = all pairs, 1 = no phantom and at least one dynamic member)", who, mode);
    IVX_REQUIRE(pairs || cap == 0, IVX_ERR_INVALID, "%s: null pair buffer of capacity %zu", who, cap);
    return IVX_OK;
}

int ivx_bvol_pairs_total(const char* who, unsigned long long grand, bool check_cap, size_t cap, size_t* n_pairs) {
    IVX_REQUIRE(grand < (1ull << 31), IVX_ERR_CAPACITY, "%s: %llu intersecting pairs: too many for one call", who, grand);
    *n_pairs = (size_t)grand;
    IVX_REQUIRE(!check_cap || grand <= cap, IVX_ERR_CAPACITY, "%s: %llu intersecting pairs, the buffer holds %zu", who, grand, cap);
    return IVX_OK;
}

int ivx_bvol_query_kinds_check(const char* who, const ivx_bv_query* queries, size_t n) {
    for (size_t q = 0; q < n; ++q)
        IVX_REQUIRE(queries[q].kind <= IVX_BV_QUERY_ORIENTED_BOX, IVX_ERR_INVALID, "%s: query %zu has kind %u (0 box, 1 sphere, 2 frustum, 3 oriented box)", who, q, queries[q].kind);
    return IVX_OK;
}

int ivx_bvol_queries_check(const char* who, ivx_ctx* c, const ivx_bv_query* queries, size_t n_queries) {
    IVX_REQUIRE(c, IVX_ERR_INVALID, "%s: null context", who);
    IVX_REQUIRE(n_queries <= IVX_BV_MAX_QUERIES, IVX_ERR_CAPACITY, "%s: %zu queries exceed %u per call", who, n_queries, IVX_BV_MAX_QUERIES);
    IVX_REQUIRE(queries || n_queries == 0, IVX_ERR_INVALID, "%s: null queries", who);
    return ivx_bvol_query_kinds_check(who, queries, n_queries);
}

int ivx_bvol_queries_begin(ivx_ctx* c, const char* who, const ivx_bv_query* queries, size_t n_queries, uint64_t* masks, ivx_bvol_query_run* run) {
    *run = ivx_bvol_query_run();
    BvState* st;
    if (int rc = set_state(c, who, &st)) return rc;
    run->n = st->n, run->n_words = (st->n + 63u) / 64u, run->n_queries = (uint32_t)n_queries;
    if (n_queries == 0 || st->n == 0) return IVX_OK;
    IVX_REQUIRE(masks, IVX_ERR_INVALID, "%s: null mask buffer", who);
    ivx_layout l;
    const size_t o_q = l.take(n_queries * sizeof(ivx_bv_query)), o_c = l.take(n_queries * 4);
    if (int rc = ivx_staging_for(&st->staging, n_queries * sizeof(ivx_bv_query))) return rc;
    if (int rc = ivx_buf_grow(c, &st->scratch, l.bytes, 1u << 20)) return rc;
    run->mask_bytes = n_queries * (size_t)run->n_words * 8;
    if (int rc = ivx_buf_grow(c, &st->masks, run->mask_bytes, 1u << 16)) return rc;
    st->queried = false, st->n_listed = 0u;  // (until this call's masks stand)
    char* s = static_cast<char*>(st->scratch.p);
    memcpy(st->staging.p, queries, n_queries * sizeof(ivx_bv_query));
    if (int rc = ivx_staging_upload(&st->staging, s + o_q, n_queries * sizeof(ivx_bv_query), c->stream)) return rc;
    run->d_queries = reinterpret_cast<const ivx_bv_query*>(s + o_q);
    run->d_masks = static_cast<unsigned long long*>(st->masks.p);
    run->d_counts = reinterpret_cast<uint32_t*>(s + o_c);
    return IVX_OK;
}

int ivx_bvol_queries_finish(ivx_ctx* c, const ivx_bvol_query_run& run, uint64_t* masks, uint32_t* counts) {
    BvState* st = static_cast<BvState*>(c->bvol_state);
    if (run.n_queries == 0u) return IVX_OK;
    if (run.n == 0u) {
        for (size_t q = 0; q < run.n_queries && counts; ++q) counts[q] = 0u;
        st->queried = true, st->n_queried = run.n_queries, st->n_listed = 0u;
        return IVX_OK;
    }
    IVX_KLAUNCH(k_bv_query_counts, dim3(run.n_queries), dim3(64), 0, c->stream, (const unsigned long long*)run.d_masks, run.n_words, run.d_counts);
    IVX_HIP_CHECK(hipGetLastError());
    IVX_HIP_CHECK(ivx_memcpy_async(masks, run.d_masks, run.mask_bytes, hipMemcpyDeviceToHost, c->stream));
    if (counts) IVX_HIP_CHECK(ivx_memcpy_async(counts, run.d_counts, (size_t)run.n_queries * 4, hipMemcpyDeviceToHost, c->stream));
    IVX_HIP_CHECK(ivx_stream_sync(c->stream));
    st->queried = true, st->n_queried = run.n_queries;
    return IVX_OK;
}

extern "C" {

int ivx_bv_world_aabb(const ivx_aabb* model, const ivx_similarity* similarity, ivx_aabb* out) {
    IVX_REQUIRE(model && similarity && out, IVX_ERR_INVALID, "ivx_bv_world_aabb: null argument");
    IVX_REQUIRE(similarity->scaling > 0.0f, IVX_ERR_INVALID, "ivx_bv_world_aabb: the scaling %g is not positive", (double)similarity->scaling);
    ivx_aabb b;
    ivx_bv_world_aabb_of(*model, *similarity, &b);
    *out = b;
    return IVX_OK;
}

int ivx_bv_frustum_query(const float planes[6][4], ivx_bv_query* out) {
    IVX_REQUIRE(planes && out, IVX_ERR_INVALID, "ivx_bv_frustum_query: null argument");
    memset(out, 0, sizeof(*out));
    out->kind = IVX_BV_QUERY_FRUSTUM;
    for (int p = 0; p < 6; ++p) {
        for (int k = 0; k < 4; ++k) out->u.frustum.planes[p][k] = planes[p][k];
        out->u.frustum.corners[p] = (((ivx_bv_bits(planes[p][0]) >> 31) ^ 1u) << 2) | (((ivx_bv_bits(planes[p][1]) >> 31) ^ 1u) << 1) | ((ivx_bv_bits(planes[p][2]) >> 31) ^ 1u);
    }
    return IVX_OK;
}

int ivx_grid_model_aabb(ivx_grid* g, ivx_aabb* out) {
    IVX_REQUIRE(g && out, IVX_ERR_INVALID, "ivx_grid_model_aabb: null argument");
    ivx_many_other_context other_(g->ctx);
    return model_aabb(g, "ivx_grid_model_aabb", out);
}

int ivx_bv_set(ivx_ctx* c, const ivx_aabb* model_boxes, const ivx_similarity* similarities, const uint32_t* kinds, size_t n) {
    IVX_REQUIRE(c, IVX_ERR_INVALID, "ivx_bv_set: null context");
    IVX_REQUIRE(model_boxes || n == 0, IVX_ERR_INVALID, "ivx_bv_set: null boxes");
    if (int rc = check_set_arguments("ivx_bv_set", similarities, kinds, n)) return rc;
    ivx_many_other_context other_(c);
    return set_enqueue(c, model_boxes, similarities, kinds, n);
}

int ivx_bv_set_grids(ivx_grid* const* grids, size_t n, const ivx_similarity* similarities, const uint32_t* kinds) {
    const char* who = "ivx_bv_set_grids";
    IVX_REQUIRE(grids || n == 0, IVX_ERR_INVALID, "%s: null object list", who);
    if (int rc = check_set_arguments(who, similarities, kinds, n)) return rc;
    if (n == 0) return IVX_OK;  // (no object names a context)
    for (size_t i = 0; i < n; ++i) {
        IVX_REQUIRE(grids[i], IVX_ERR_INVALID, "%s: object %zu is null", who, i);
        IVX_REQUIRE(grids[i]->ctx == grids[0]->ctx, IVX_ERR_INVALID, "%s: object %zu belongs to another context", who, i);
    }
    ivx_ctx* c = grids[0]->ctx;
    ivx_many_other_context other_(c);
    (void)ivx_many_break();  // the ranges below are the objects' after everything recorded so far
    if (int rc = ivx_many_error(c, false)) {
        ivx_set_error("%s: a flush of recorded launches failed on this context", who);
        return rc;
    }
    std::vector<ivx_aabb> boxes(n);
    for (size_t i = 0; i < n; ++i)
        if (int rc = model_aabb(grids[i], who, &boxes[i])) return rc;
    return set_enqueue(c, boxes.data(), similarities, kinds, n);
}

int ivx_bv_download(ivx_ctx* c, ivx_aabb* world_boxes, size_t cap, ivx_aabb* total) {
    BvState* st;
    if (int rc = set_state(c, "ivx_bv_download", &st)) return rc;
    IVX_REQUIRE(!world_boxes || cap >= st->n, IVX_ERR_CAPACITY, "ivx_bv_download: the set has %u boxes, the buffer holds %zu", st->n, cap);
    if (st->n == 0) {
        if (total) memset(total, 0, sizeof(*total));
        return IVX_OK;
    }
    ivx_many_other_context other_(c);
    const char* d = static_cast<const char*>(st->set.p);
    if (world_boxes) IVX_HIP_CHECK(ivx_memcpy_async(world_boxes, d + st->o_world, (size_t)st->n * sizeof(ivx_aabb), hipMemcpyDeviceToHost, c->stream));
    if (total) IVX_HIP_CHECK(ivx_memcpy_async(total, d + st->o_total, sizeof(ivx_aabb), hipMemcpyDeviceToHost, c->stream));
    IVX_HIP_CHECK(ivx_stream_sync(c->stream));
    return IVX_OK;
}

int ivx_bv_pairs(ivx_ctx* c, uint32_t mode, uint32_t* pairs, size_t cap, size_t* n_out) {
    const char* who = "ivx_bv_pairs";
    if (int rc = ivx_bvol_pairs_check(who, c, mode, pairs, cap, n_out)) return rc;
    BvState* st;
    if (int rc = set_state(c, who, &st)) return rc;
    if (st->n < 2u) return IVX_OK;
    ivx_many_other_context other_(c);
    if (int rc = ivx_bvol_pairs_enqueue(c, who, mode, pairs != nullptr, cap, n_out)) return rc;
    if (*n_out == 0) return IVX_OK;
    if (pairs) IVX_HIP_CHECK(ivx_memcpy_async(pairs, st->pairs.p, *n_out * 8, hipMemcpyDeviceToHost, c->stream));
    IVX_HIP_CHECK(ivx_stream_sync(c->stream));
    return IVX_OK;
}

int ivx_bv_queries(ivx_ctx* c, const ivx_bv_query* queries, size_t n_queries, uint64_t* masks, uint32_t* counts) {
    const char* who = "ivx_bv_queries";
    if (int rc = ivx_bvol_queries_check(who, c, queries, n_queries)) return rc;
    BvState* st;
    if (int rc = set_state(c, who, &st)) return rc;
    ivx_bvol_query_run run;
    if (n_queries == 0 || st->n == 0) {  // (nothing reaches the stream)
        if (int rc = ivx_bvol_queries_begin(c, who, queries, n_queries, masks, &run)) return rc;
        return ivx_bvol_queries_finish(c, run, masks, counts);
    }
    IVX_REQUIRE(masks, IVX_ERR_INVALID, "%s: null mask buffer", who);
    ivx_many_other_context other_(c);
    if (int rc = ivx_bvol_queries_begin(c, who, queries, n_queries, masks, &run)) return rc;
    IVX_KLAUNCH(k_bv_query, dim3((run.n_words + 3u) / 4u), dim3(256), 0, c->stream, reinterpret_cast<const ivx_aabb*>(static_cast<const char*>(st->set.p) + st->o_world), run.n,
                run.d_queries, run.n_queries, run.d_masks);
    return ivx_bvol_queries_finish(c, run, masks, counts);
}

int ivx_bv_query_lists(ivx_ctx* c, uint32_t* offsets, uint32_t* objects, size_t cap, size_t* n_out) {
    const char* who = "ivx_bv_query_lists";
    IVX_REQUIRE(n_out, IVX_ERR_INVALID, "%s: null argument", who);
    *n_out = 0;
    IVX_REQUIRE(objects || cap == 0, IVX_ERR_INVALID, "%s: null object buffer of capacity %zu", who, cap);
    BvState* st;
    if (int rc = set_state(c, who, &st)) return rc;
    IVX_REQUIRE(st->queried && st->n != 0u, IVX_ERR_STATE, "%s: no masks of the context's current set (call ivx_bv_queries or ivx_bv_queries_hierarchy after the set; an empty set has none)", who);
    const uint32_t nq = st->n_queried, n_words = (st->n + 63u) / 64u, n_all = nq * n_words;  // (at most 2^10 x 2^14)
    ivx_many_other_context other_(c);
    ivx_layout l;
    const size_t o_prefix = l.take((size_t)n_all * 4), o_totals = l.take((size_t)nq * 4), o_offsets = l.take(((size_t)nq + 1u) * 4);
    if (int rc = ivx_buf_grow(c, &st->lists, l.bytes, 1u << 16)) return rc;
    st->n_listed = 0u;  // (until this call's lists stand)
    char* d = static_cast<char*>(st->lists.p);
    const unsigned long long* d_masks = static_cast<const unsigned long long*>(st->masks.p);
    uint32_t* d_prefix = reinterpret_cast<uint32_t*>(d + o_prefix);
    uint32_t* d_totals = reinterpret_cast<uint32_t*>(d + o_totals);
    uint32_t* d_offsets = reinterpret_cast<uint32_t*>(d + o_offsets);
    const dim3 words_grid((n_all + 255u) / 256u);
    IVX_KLAUNCH(k_bv_list_words, words_grid, dim3(256), 0, c->stream, d_masks, n_all, d_prefix);
    IVX_KLAUNCH(k_bv_list_rows, dim3(nq), dim3(SCAN_ROUND), 0, c->stream, d_prefix, n_words, d_totals);
    IVX_KLAUNCH(k_bv_list_offsets, dim3(1), dim3(SCAN_ROUND), 0, c->stream, (const uint32_t*)d_totals, nq, d_offsets);
    IVX_HIP_CHECK(hipGetLastError());
    uint32_t total = 0;
    IVX_HIP_CHECK(ivx_memcpy_async(&total, d_offsets + nq, 4, hipMemcpyDeviceToHost, c->stream));
    IVX_HIP_CHECK(ivx_stream_sync(c->stream));
    *n_out = total;
    IVX_REQUIRE(!objects || total <= cap, IVX_ERR_CAPACITY, "%s: %u objects hit, the buffer holds %zu", who, total, cap);
    if (total != 0u) {
        if (int rc = ivx_buf_grow(c, &st->hits, (size_t)total * 4, 1u << 16)) return rc;
        IVX_KLAUNCH(k_bv_list_emit, words_grid, dim3(256), 0, c->stream, d_masks, n_words, n_all, (const uint32_t*)d_prefix, (const uint32_t*)d_offsets, total,
                    static_cast<uint32_t*>(st->hits.p));
        IVX_HIP_CHECK(hipGetLastError());
    }
    st->o_list_offsets = o_offsets, st->n_listed = nq + 1u;
    if (offsets) IVX_HIP_CHECK(ivx_memcpy_async(offsets, d_offsets, ((size_t)nq + 1u) * 4, hipMemcpyDeviceToHost, c->stream));
    if (objects && total != 0u) IVX_HIP_CHECK(ivx_memcpy_async(objects, st->hits.p, (size_t)total * 4, hipMemcpyDeviceToHost, c->stream));
    if (offsets || (objects && total != 0u)) IVX_HIP_CHECK(ivx_stream_sync(c->stream));
    return IVX_OK;
}

void* ivx_bv_device_ptr(ivx_ctx* c, int which) {
    if (!c || !c->bvol_state) return nullptr;
    BvState* st = static_cast<BvState*>(c->bvol_state);
    switch (which) {
        case IVX_BV_PTR_WORLD_BOXES: return st->has_set && st->n ? static_cast<char*>(st->set.p) + st->o_world : nullptr;
        case IVX_BV_PTR_PAIRS: return st->pairs.p;
        case IVX_BV_PTR_MASKS: return st->masks.p;
        case IVX_BV_PTR_NODES:
        case IVX_BV_PTR_LEAF_OBJECTS: return st->has_set ? ivx_bvh_device_ptr(st->hierarchy, st->serial, which) : nullptr;
        case IVX_BV_PTR_HIT_OFFSETS: return st->has_set && st->n_listed ? static_cast<char*>(st->lists.p) + st->o_list_offsets : nullptr;
        case IVX_BV_PTR_HIT_OBJECTS: return st->has_set && st->n_listed ? st->hits.p : nullptr;
        default: return nullptr;
    }
}

}  // extern "C"
