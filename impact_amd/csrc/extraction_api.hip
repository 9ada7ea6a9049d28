// Extraction host code of libimpact_voxel_hip.so: splitting disconnected regions off an object (one, or the whole loop in one call), the polyhedron
// clip (extract or copy) and the batched polyhedron copy, with the re-derivation of an object whose voxels changed. Host-side orchestration only:
// the kernels are those of split.hip and the step behind their ivx_launch_* functions. Every rule of the reference that these calls share has one
// body in the anonymous namespace below.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <vector>

#include "ivx_host.hpp"

// Derived state + regions of an object whose voxels changed, through the fused step path (ivx_voxel_step_enqueue: five launches and the
// results block instead of the stand-alone passes' ten launches and a blocking copy). `rederive_enqueue` only puts the work on the
// stream — a caller with results of its own still in flight waits for both with the one `rederive_collect`.
int rederive_enqueue(ivx_grid* g) { return step_enqueue_untimed(g, IVX_STAGE_DERIVE | IVX_STAGE_REGIONS); }
int rederive_collect(ivx_grid* g) {
    ivx_step_result res;
    const int rc = ivx_voxel_step_collect(g, &res);
    if (rc) return rc;
    g->mesh_valid = 0;
    return IVX_OK;
}
int rederive(ivx_grid* g) {
    const int rc = rederive_enqueue(g);
    return rc ? rc : rederive_collect(g);
}

namespace {
// the table of unit densities: with it an object's mass is its non-empty voxel count times the voxel volume
const float* unit_densities() {
    static const struct Ones {
        float v[256];
        Ones() {
            for (float& x : v) x = 1.0f;
        }
    } ones;
    return ones.v;
}
// ... as the object's resident table (one upload, one wait)
int set_unit_densities(ivx_grid* g) {
    const int rc = h2d(g, g->dens_dev, unit_densities(), sizeof(g->dens_host));
    if (rc) return rc;
    memcpy(g->dens_host, unit_densities(), sizeof(g->dens_host));
    g->has_dens = 1;
    return IVX_OK;
}

// The occupied ranges the object has NOW, by a reduction and a host read of their own. (Not ivx_reference_occupied: that one answers from
// ivx_grid::occ_ref while it is valid and launches nothing then, and these calls have always launched their reduction; nor does this fill the
// cache.)
int occupied_now(ivx_grid* g, uint32_t occ[12]) {
    uint32_t* d_occ = g->rscalar + 16;
    int rc;
    if ((rc = ivx_launch_occupied(g, d_occ))) return rc;
    uint32_t raw[12];
    if ((rc = d2h(g, raw, d_occ, sizeof(raw)))) return rc;
    ivx_occupied_from_raw(g, raw, occ);
    return IVX_OK;
}

// voxel_ranges_in_object_touching_aab (object/intersection.rs:693-782) of the AABB expanded by 2.54, as the box of chunks that holds them;
// false: the AABB misses the occupied ranges
bool aabb_chunk_box(const float aabb[6], const uint32_t occ[12], uint32_t lo[3], uint32_t cc[3]) {
    for (int q = 0; q < 3; ++q) {
        const float l = aabb[q] - 2.54f, h = aabb[3 + q] + 2.54f;
        const float fl = floorf(l);
        const long s = (long)(fl > 0.0f ? fl : 0.0f), e = (long)ceilf(h);
        const long vlo = std::max<long>((long)occ[6 + 2 * q], s), vhi = std::min<long>((long)occ[7 + 2 * q], std::max<long>(e, 0));
        if (vlo >= vhi) return false;
        lo[q] = (uint32_t)(vlo / 16);
        cc[q] = (uint32_t)((vhi + 15) / 16) - lo[q];
    }
    return true;
}

// find_two_disconnected_regions + the choice between them (extraction.rs:255-271), played over the descriptors of all regions: of the first two
// regions still there the one with fewer non-uniform chunks goes, ties by chunk count, then the second. -> the regions in the order they leave,
// at most `picks` of them (the single split-off is the loop's first iteration).
std::vector<uint32_t> extraction_order(const std::vector<ivx_region_desc>& d, size_t picks) {
    std::vector<uint32_t> order;
    order.reserve(std::min(picks, d.size()));
    uint32_t front = 0;  // the first region still there; `second`: the next one
    for (uint32_t second = 1; second < (uint32_t)d.size() && order.size() < picks; ++second) {
        const ivx_region_desc &a = d[front], &b = d[second];
        const bool take_first = a.non_uniform_chunk_count != b.non_uniform_chunk_count ? a.non_uniform_chunk_count < b.non_uniform_chunk_count : a.chunk_count < b.chunk_count;
        order.push_back(take_first ? front : second);
        if (take_first) front = second;
    }
    return order;
}

// What complete_extracted_voxel_object (extraction.rs:1902-2142) decides about a child of `cc` chunks from its uniform chunk count, its non-empty
// voxel count and the extents [lo, hi) of its non-empty voxels in its own grid (`ext`: lo, hi per axis, the layout of occupied[6..11]): a crumb
// gets no object; a child without uniform chunks, of more than one chunk, none of its extents above 14, goes into a single chunk, moved by `off`
// so that a voxel of padding stays in front of it.
struct ChildFate {
    bool crumb, one_chunk;
    uint32_t off[3];
};
ChildFate child_fate(uint32_t uniform_count, unsigned long long non_empty, const uint32_t cc[3], const uint32_t ext[6]) {
    ChildFate f;
    f.crumb = uniform_count == 0 && non_empty < 8;  // NON_EMPTY_VOXEL_THRESHOLD (object.rs:203)
    f.one_chunk = !f.crumb && uniform_count == 0 && cc[0] <= 2 && cc[1] <= 2 && cc[2] <= 2 && cc[0] * cc[1] * cc[2] > 1 && ext[1] - ext[0] <= 14 &&
                  ext[3] - ext[2] <= 14 && ext[5] - ext[4] <= 14;
    for (int q = 0; q < 3; ++q) f.off[q] = ext[2 * q] > 0 ? ext[2 * q] - 1u : 0u;
    return f;
}
// ... of a region that leaves its object, from its descriptor: the box of chunks it lies in, and its fate from its extents inside that box
struct RegionBox {
    uint32_t lo[3], cc[3];
    ChildFate fate;
};
RegionBox region_box(const ivx_region_desc& r) {
    RegionBox b;
    uint32_t ext[6];
    for (int q = 0; q < 3; ++q) {
        b.lo[q] = r.lo[q] >> 4;
        b.cc[q] = ((r.hi[q] - 1u) >> 4) - b.lo[q] + 1u;
        ext[2 * q] = r.lo[q] - b.lo[q] * 16u;
        ext[2 * q + 1] = r.hi[q] - b.lo[q] * 16u;
    }
    b.fate = child_fate(r.chunk_count - r.non_uniform_chunk_count, r.voxel_count, b.cc, ext);
    return b;
}

// A small child into a grid of ONE chunk (an allocation of its own), moved by -off. Done: the source is destroyed (which waits for the stream:
// the repack has read it), *pc is the new grid and `off` is added to `origin`. Failed: *pc still is the source, the caller's to release.
int repack_into_one_chunk(ivx_grid** pc, const uint32_t off[3], uint32_t origin[3]) {
    ivx_grid* c = *pc;
    const uint32_t one[3] = {1, 1, 1};
    ivx_grid* single = nullptr;
    int rc;
    if ((rc = ivx_grid_create(c->ctx, one, c->extent, 0, 0, &single))) return rc;
    if ((rc = ivx_launch_split_repack(c, single, off))) {
        ivx_grid_destroy(single);
        return rc;
    }
    ivx_grid_destroy(c);
    *pc = single;
    for (int q = 0; q < 3; ++q) origin[q] += off[q];
    return IVX_OK;
}

// `f(i)` for every object, RECORDED (many.hpp) so that one launch per chain position serves all of them: under a bracket of our own (many_phase:
// begin, the objects in order until the first error, flush), or — the caller's bracket is open — in order behind a break, unmerged, the flush
// left to the caller.
int recorded_for_all(ivx_grid* const* grids, size_t n, const std::function<int(size_t)>& f) {
    if (!ivx_many_recording()) return many_phase(grids, n, f);
    (void)ivx_many_break();
    for (size_t i = 0; i < n; ++i)
        if (int rc = f(i)) return rc;
    return IVX_OK;
}

// The end of a batched call that failed with children from a pooled block in flight: the stream is drained, the children go, the caller's
// `children` are nulled and, where given, its `outcomes` zeroed. -> code
int drop_pooled_children(ivx_ctx* ctx, std::vector<ivx_grid*>& kids, ivx_grid** children, int* outcomes, size_t n, int code) {
    (void)ivx_stream_sync(ctx->stream);
    for (ivx_grid*& c : kids)
        if (c) {
            c->pending_stages = 0, c->gather_launched = 0;
            ivx_grid_destroy(c);
            c = nullptr;
        }
    for (size_t k = 0; k < n; ++k) {
        children[k] = nullptr;
        if (outcomes) outcomes[k] = 0;
    }
    return code;
}

// the work counters of a child from a pooled block start at zero: recorded, or on the stream
int zero_work_counts(ivx_grid* c) {
    if (!ivx_many_zero(c->ctx, c, c->work_counts, 8 * sizeof(uint32_t))) IVX_HIP_CHECK(ivx_memset_async(c->work_counts, 0, 8 * sizeof(uint32_t), c->ctx->stream));
    return IVX_OK;
}
}  // namespace

int ivx_split_off_smallest_region(ivx_grid* parent, ivx_grid** child, uint32_t origin_offset_in_parent[3], int* outcome, ivx_region_desc* moved) {
    IVX_REQUIRE(parent && child && origin_offset_in_parent && outcome, IVX_ERR_INVALID, "ivx_split_off_smallest_region: null argument");
    *child = nullptr;
    *outcome = 0;
    int rc;
    if ((rc = require_whole_object(parent, "ivx_split_off_smallest_region", false))) return rc;
    if (parent->region_count < 2) return IVX_OK;
    if (!parent->has_dens && (rc = set_unit_densities(parent))) return rc;
    std::vector<ivx_region_desc> d;
    if ((rc = describe_regions_internal(parent, parent->dens_dev, d))) return rc;
    const uint32_t pick = extraction_order(d, 1)[0];
    const ivx_region_desc& r = d[pick];
    if (moved) *moved = r;
    const RegionBox b = region_box(r);
    ivx_grid* c = nullptr;
    if (!b.fate.crumb && (rc = ivx_grid_create(parent->ctx, b.cc, parent->extent, 0, 0, &c))) return rc;
    if ((rc = ivx_launch_split_move(parent, c, b.lo, b.cc, pick))) {
        ivx_grid_destroy(c);
        return rc;
    }
    for (int q = 0; q < 3; ++q) origin_offset_in_parent[q] = b.lo[q] * 16u;
    if (b.fate.one_chunk && (rc = repack_into_one_chunk(&c, b.fate.off, origin_offset_in_parent))) {
        ivx_grid_destroy(c);
        return rc;
    }
    if ((parent->occ_ref_valid = 0, rc = rederive(parent))) {
        ivx_grid_destroy(c);
        return rc;
    }
    if (c && (rc = rederive(c))) {
        ivx_grid_destroy(c);
        return rc;
    }
    *child = c;
    *outcome = c ? 1 : 2;
    return IVX_OK;
}

// The reference's split-off LOOP in one call (interaction.rs:256: `while let Some(..) = find_two_disconnected_regions` ->
// extract the smaller of the FIRST TWO regions in scan order, extraction.rs:255-271): the regions of the object are described once; what a
// region is — voxels, box, chunk counts — does not change when another region leaves (regions share no voxel, and a chunk that holds two of
// them stays NonUniform for the one that remains), nor does their scan order, so the loop's picks follow from the one description: the host
// plays the loop over the descriptors, every region that goes is moved out by its own launch into a grid from one shared block, the parent
// is re-derived ONCE and the children together (recorded, many.hpp). `children` / `origins3` / `outcomes` / `moved` in the order the loop
// extracts them (outcome 1: a child object, 2: discarded as a crumb); *n_out = number of split-offs (regions - 1).
int ivx_split_off_all(ivx_grid* parent, size_t cap, ivx_grid** children, uint32_t* origins3, int* outcomes, ivx_region_desc* moved, size_t* n_out) {
    IVX_REQUIRE(parent && n_out && (cap == 0 || (children && origins3 && outcomes)), IVX_ERR_INVALID, "ivx_split_off_all: null argument");
    *n_out = 0;
    int rc;
    if ((rc = require_whole_object(parent, "ivx_split_off_all", false))) return rc;
    if (parent->region_count < 2) return IVX_OK;
    const size_t n = parent->region_count - 1u;
    *n_out = n;
    IVX_REQUIRE(n <= cap, IVX_ERR_CAPACITY, "ivx_split_off_all: %zu split-offs exceed capacity %zu", n, cap);
    if (!parent->has_dens && (rc = set_unit_densities(parent))) return rc;
    std::vector<ivx_region_desc> d;
    if ((rc = describe_regions_internal(parent, parent->dens_dev, d))) return rc;
    const std::vector<uint32_t> order = extraction_order(d, n);
    // the children's boxes and grids (crumbs get none: their voxels are just emptied)
    std::vector<RegionBox> box(n);
    std::vector<uint32_t> ccs;
    std::vector<size_t> slot(n, (size_t)-1);
    for (size_t k = 0; k < n; ++k) {
        const ivx_region_desc& r = d[order[k]];
        if (moved) moved[k] = r;
        children[k] = nullptr;
        box[k] = region_box(r);
        for (int q = 0; q < 3; ++q) origins3[3 * k + q] = box[k].lo[q] * 16u;
        outcomes[k] = box[k].fate.crumb ? 2 : 1;
        if (box[k].fate.crumb) continue;
        slot[k] = ccs.size() / 3;
        for (int q = 0; q < 3; ++q) ccs.push_back(box[k].cc[q]);
    }
    const size_t n_kids = ccs.size() / 3;
    std::vector<ivx_grid*> kids(n_kids, nullptr);
    if ((rc = grid_create_pooled(parent->ctx, ccs.data(), n_kids, parent->extent, kids.data(), "ivx_split_off_all"))) return rc;
    auto fail = [&](int code) {
        parent->regions_valid = 0;  // (voxels may have left: the caller derives the object again)
        return drop_pooled_children(parent->ctx, kids, children, nullptr, n, code);
    };
    // every region that goes, by its own launch (they read the labelling the parent has now; none of them changes it)
    for (size_t k = 0; k < n; ++k)
        if ((rc = ivx_launch_split_move(parent, slot[k] == (size_t)-1 ? nullptr : kids[slot[k]], box[k].lo, box[k].cc, order[k]))) return fail(rc);
    // small children into one chunk
    for (size_t k = 0; k < n; ++k)
        if (box[k].fate.one_chunk && (rc = repack_into_one_chunk(&kids[slot[k]], box[k].fate.off, origins3 + 3 * k))) return fail(rc);
    // derived state and regions: the parent and every child, recorded and issued together; one wait
    parent->occ_ref_valid = 0;
    std::vector<ivx_grid*> all(kids);
    all.push_back(parent);
    if ((rc = recorded_for_all(all.data(), all.size(), [&](size_t i) -> int {
             ivx_grid* g = all[i];
             int r;
             // (a repacked child has an allocation of its own, zeroed at creation)
             if (g != parent && g->arena_block && (r = zero_work_counts(g))) return r;
             if ((r = rederive_enqueue(g))) return r;
             return ivx_step_collect_launch(g);
         })))
        return fail(rc);
    for (ivx_grid* g : all)
        if ((rc = rederive_collect(g))) return fail(rc);
    for (size_t k = 0; k < n; ++k)
        if (slot[k] != (size_t)-1) children[k] = kids[slot[k]];
    return IVX_OK;
}

// complete_extracted_voxel_object (extraction.rs:1901-2123) for a freshly filled child grid: discard rule, single-chunk
// repack, derived state. On return *pc is the final child (or nullptr when discarded).
static int complete_extracted(ivx_grid** pc, uint32_t origin[3]) {
    ivx_grid* c = *pc;
    int rc;
    std::vector<ivx_chunk_info> info(c->n_chunks);
    if ((rc = d2h(c, info.data(), c->info, sizeof(ivx_chunk_info) * c->n_chunks))) return rc;
    uint32_t uniform_count = 0;
    for (const ivx_chunk_info& i : info) uniform_count += i.gen_kind == KIND_UNIFORM;
    // non-empty voxel count and tight voxel box of the child: derive (flags + per-chunk boxes), unit-density mass
    if ((rc = ivx_launch_derive(c, 0))) return rc;
    uint32_t occ[12];
    if ((rc = occupied_now(c, occ))) return rc;
    if ((rc = set_unit_densities(c))) return rc;
    double* out_dev = c->partials + c->partial_blocks * 10;
    if ((rc = ivx_launch_inertia(c, c->dens_dev, out_dev, 0))) return rc;
    double m0 = 0.0;
    if ((rc = d2h(c, &m0, out_dev, sizeof(double)))) return rc;
    const double e = (double)c->extent;
    const ChildFate fate = child_fate(uniform_count, (unsigned long long)(m0 / (e * e * e) + 0.5), c->cc, occ + 6);
    if (fate.crumb) {
        ivx_grid_destroy(c);
        *pc = nullptr;
        return IVX_OK;
    }
    if (fate.one_chunk && occ[1] != 0 && (rc = repack_into_one_chunk(pc, fate.off, origin))) return rc;
    return rederive(*pc);
}

int ivx_clip_polyhedron(ivx_grid* parent, const float* planes4, size_t n_planes, const float aabb[6], int copy, ivx_grid** child,
                        uint32_t origin_offset_in_parent[3], int* outcome) {
    IVX_REQUIRE(parent && planes4 && aabb && child && origin_offset_in_parent && outcome, IVX_ERR_INVALID, "ivx_clip_polyhedron: null argument");
    *child = nullptr;
    *outcome = 0;
    IVX_REQUIRE(n_planes >= 1 && n_planes <= 64, IVX_ERR_CAPACITY, "ivx_clip_polyhedron: 1..64 planes supported, got %zu", n_planes);
    int rc;
    if ((rc = require_whole_object(parent, "ivx_clip_polyhedron", false))) return rc;
    uint32_t occ[12], lo[3], cc[3];
    if ((rc = occupied_now(parent, occ))) return rc;
    if (occ[1] == 0 || !aabb_chunk_box(aabb, occ, lo, cc)) return IVX_OK;
    ivx_grid* c = nullptr;
    if ((rc = ivx_grid_create(parent->ctx, cc, parent->extent, 0, 0, &c))) return rc;
    if ((rc = ivx_launch_clip(parent, c, lo, cc, planes4, (uint32_t)n_planes, copy ? 0 : 1))) {
        ivx_grid_destroy(c);
        return rc;
    }
    for (int q = 0; q < 3; ++q) origin_offset_in_parent[q] = lo[q] * 16u;
    if (!copy && (parent->occ_ref_valid = 0, rc = rederive(parent))) {
        ivx_grid_destroy(c);
        return rc;
    }
    if ((rc = complete_extracted(&c, origin_offset_in_parent))) {
        if (c) ivx_grid_destroy(c);
        return rc;
    }
    *child = c;
    *outcome = c ? 1 : 2;
    return IVX_OK;
}

// Batched polyhedron COPY: every fragment of one impact in one call (FracturingProcess::execute_in_parallel, fracturing.rs:1047-1189, runs
// copy_polyhedron_with_property_computer, extraction.rs:1301-1768, for all Voronoi cells of an impact over a thread pool; the object itself
// is not changed). The looped form pays per fragment: an occupied-range reduction with a host read, the child's record download, three more
// host reads for its voxel count / box / regions. Here the parent's ranges are reduced once, all clip kernels and all children's derive /
// range / voxel-count passes are enqueued back to back and read with ONE wait, the discard / repack decisions are taken on the host, then
// all region passes follow with a second wait. Per fragment the results are those of ivx_clip_polyhedron(copy = 1).
int ivx_copy_polyhedra(ivx_grid* parent, const float* planes4, const uint32_t* plane_counts, const float* aabbs6, size_t n_sets, ivx_grid** children,
                       uint32_t* origins3, int* outcomes) {
    IVX_REQUIRE(parent && planes4 && plane_counts && aabbs6 && children && origins3 && outcomes, IVX_ERR_INVALID, "ivx_copy_polyhedra: null argument");
    int rc;
    if ((rc = require_whole_object(parent, "ivx_copy_polyhedra", false))) return rc;
    for (size_t f = 0; f < n_sets; ++f) {
        children[f] = nullptr;
        outcomes[f] = 0;
        IVX_REQUIRE(plane_counts[f] >= 1 && plane_counts[f] <= 64, IVX_ERR_CAPACITY, "ivx_copy_polyhedra: 1..64 planes per polyhedron, set %zu has %u", f, plane_counts[f]);
    }
    if (n_sets == 0) return IVX_OK;
    hipStream_t s = parent->ctx->stream;
    uint32_t occ[12];
    if ((rc = occupied_now(parent, occ))) return rc;
    if (occ[1] == 0) return IVX_OK;
    // 1. the children's chunk boxes; their grids from ONE device block and ONE pinned block (grid_create_pooled)
    std::vector<uint32_t> live, ccs, los;
    size_t plane_off = 0;
    std::vector<size_t> plane_offs(n_sets);
    for (size_t f = 0; f < n_sets; plane_off += plane_counts[f], ++f) {
        plane_offs[f] = plane_off;
        uint32_t lo[3], cc[3];
        if (!aabb_chunk_box(aabbs6 + 6 * f, occ, lo, cc)) continue;
        live.push_back((uint32_t)f);
        for (int q = 0; q < 3; ++q) ccs.push_back(cc[q]), los.push_back(lo[q]), origins3[3 * f + q] = lo[q] * 16u;
    }
    const size_t n_live = live.size();
    if (n_live == 0) return IVX_OK;
    std::vector<ivx_grid*> kids(n_live, nullptr);
    if ((rc = grid_create_pooled(parent->ctx, ccs.data(), n_live, parent->extent, kids.data(), "ivx_copy_polyhedra"))) return rc;
    auto fail = [&](int code) { return drop_pooled_children(parent->ctx, kids, children, outcomes, n_sets, code); };
    if ((rc = ivx_ensure_dense(parent))) return fail(rc);  // (what the clips read; ahead of the recording: it may launch)
    // 2. per child, RECORDED (many.hpp) and issued as one launch per chain position for all of them: the clip, then a step of the child without
    // the sample and remesh stages — derived state, regions, occupied ranges, unit-density mass (= voxel count) — and the gather of its small
    // results into its host-mapped block. One wait for all. (No event records around the step's slots: they would cut the merged launches
    // between every two children.)
    const float* ones = unit_densities();
    const uint32_t child_stages = IVX_STAGE_DERIVE | IVX_STAGE_REGIONS | IVX_STAGE_OCCUPIED | IVX_STAGE_INERTIA;
    if ((rc = recorded_for_all(kids.data(), n_live, [&](size_t i) -> int {
             ivx_grid* c = kids[i];
             const size_t f = live[i];
             int r;
             if ((r = zero_work_counts(c))) return r;
             if ((r = ivx_launch_clip(parent, c, &los[3 * i], &ccs[3 * i], planes4 + 4 * plane_offs[f], plane_counts[f], 0))) return r;
             if (!ivx_many_upload(c->ctx, c, c->dens_dev, ones, sizeof(c->dens_host))) IVX_HIP_CHECK(ivx_memcpy_async(c->dens_dev, ones, sizeof(c->dens_host), hipMemcpyHostToDevice, s));
             memcpy(c->dens_host, ones, sizeof(c->dens_host));
             c->has_dens = 1;
             if ((r = step_enqueue_untimed(c, child_stages))) return r;
             return ivx_step_collect_launch(c);
         })))
        return fail(rc);
    std::vector<ivx_step_result> res(n_live);
    for (size_t i = 0; i < n_live; ++i)
        if ((rc = ivx_voxel_step_collect(kids[i], &res[i]))) return fail(rc);
    // 3. discard crumbs, repack small children into one chunk (complete_extracted_voxel_object, extraction.rs:1902-2142)
    for (size_t i = 0; i < n_live; ++i) {
        const size_t f = live[i];
        const uint32_t* cocc = res[i].occupied;
        const double e = (double)kids[i]->extent;
        // (the uniform chunk count is passed as zero: a chunk filled with one type — gen_kind Uniform — holds 4096 voxels and spans 16 along
        // every axis: neither the crumb test nor the one-chunk test can pass with one, which is what the reference's `uniform_chunk_count == 0`
        // conditions say)
        const ChildFate fate = child_fate(0, (unsigned long long)(res[i].moments.m64[0] / (e * e * e) + 0.5), kids[i]->cc, cocc + 6);
        if (fate.crumb) {
            ivx_grid_destroy(kids[i]);
            kids[i] = nullptr;
            outcomes[f] = 2;
            continue;
        }
        if (fate.one_chunk && cocc[1] != 0) {
            if ((rc = repack_into_one_chunk(&kids[i], fate.off, origins3 + 3 * f))) return fail(rc);
            ivx_step_result again;
            if ((rc = ivx_grid_set_densities(kids[i], ones)) || (rc = ivx_voxel_step(kids[i], child_stages, &again))) return fail(rc);
        }
        kids[i]->mesh_valid = 0;
        children[f] = kids[i];
        outcomes[f] = 1;
    }
    return IVX_OK;
}
