// Edit host code of libimpact_voxel_hip.so: a sphere or capsule absorbing voxels of an object (ivx_absorb_*_enqueue, ivx_absorb_collect and the
// calls that do both), the many-object forms, and the mutual absorption of two objects; the host state of an object's edits (ivx_edit_state,
// private to this unit) and the one statement of the result block an absorb kernel fills. Host-side orchestration only: the kernels are those of
// edit.hip and the step's, behind their ivx_launch_* functions. What the rest of the library asks of this unit is declared in ivx_host.hpp.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "ivx_host.hpp"
#include "voxel_ranges.hpp"

// ---- the result block --------------------------------------------------------------------------------------------------------------------
// What an absorb kernel accumulates for one object: [10 f64 removed moments][256 u32 emptied voxels by type][2 u32 counters: touched chunks,
// removed chunks; 2 spare words][u32 touched voxel ranges of `touched_words` chunks]. The single forms carry on, `grown` being the chunks of the
// touched box grown by one chunk each way: [uint4 needs records of the grown box's chunks], and in the host-mapped copy [their early twin]
// [the bell behind it].
struct EditBlock {
    size_t off_type, off_cnt, off_touch;
    size_t off_needs, total, off_early, off_bell;  // `off_needs`: behind the touched words; `total`: what the device block holds of one edit
    explicit EditBlock(size_t touched_words = 0, size_t grown = 0) {
        off_type = 80, off_cnt = off_type + 1024, off_touch = off_cnt + 16;
        off_needs = (off_touch + touched_words * 4 + 15) & ~(size_t)15;
        total = off_needs + grown * 16;
        off_early = (total + 63) & ~(size_t)63;
        off_bell = off_early + grown * 16;
    }
};
// A host copy `hb` of a block becomes the call's result: the moments in the object's units (sums over voxel indices times e^3, e^4 / 2, e^5 / 3,
// e^5 / 4), the emptied voxels summed over the types (`emptied_by_type` non-null: and each type's), the two counters.
static void edit_block_result(ivx_grid* g, const char* hb, const EditBlock& blk, ivx_absorb_result* out, uint32_t* emptied_by_type) {
    const double* rem = reinterpret_cast<const double*>(hb);
    const double ex = (double)g->extent, e3 = ex * ex * ex, e4 = e3 * ex, e5 = e4 * ex;
    const double f[10] = {e3, 0.5 * e4, 0.5 * e4, 0.5 * e4, e5 / 3.0, e5 / 3.0, e5 / 3.0, 0.25 * e5, 0.25 * e5, 0.25 * e5};
    for (int q = 0; q < 10; ++q) out->removed_moments[q] = rem[q] * f[q];
    const uint32_t* by_type = reinterpret_cast<const uint32_t*>(hb + blk.off_type);
    uint64_t emptied = 0;
    for (int t = 0; t < 256; ++t) {
        emptied += by_type[t];
        if (emptied_by_type) emptied_by_type[t] = by_type[t];
    }
    out->emptied_voxels = emptied;
    const uint32_t* cnt = reinterpret_cast<const uint32_t*>(hb + blk.off_cnt);
    out->touched_chunks = cnt[0];
    out->removed_chunks = cnt[1];
    if (cnt[1]) g->occ_ref_valid = 0;  // `if removed_chunks { self.update_occupied_ranges() }` (intersection.rs:255-257, 384-386, 520-522)
}

// ---- the edit path (§8f-2): ONE wait per edit, and only the chunks the edit can have changed are swept -------------------------------------
// ivx_absorb_*_enqueue puts on the stream: the edit kernel over the touched chunk box; the derive sweep over that box grown by one chunk
// each way (ivx_launch_derive_box: what the reference patches chunk by chunk, object/intersection.rs:255-262, 532-598) with the region
// forest of all other chunks reset; the global region resolve (interaction/absorption.rs:631); the count pass of the remesh for the chunks
// whose meshes the edit invalidates (ivx_launch_box_mesh_needs); one copy of all small results into pinned memory. ivx_absorb_collect waits
// for the doorbell behind them. Round 3 swept the whole object's active list (5 388 chunks of the 512^3 body for a bite that touches 80)
// and ivx_mesh_sync counted the whole object again and read its sizes back.
struct ivx_edit_state {
    // the edit in flight
    int pending = 0, nothing = 0, staged = 0;
    uint32_t bcc[3] = {0, 0, 0};  // the chunks of the grown box
    EditBlock blk;
    ivx_mapped pinned;          // results of the edit in flight: host-mapped, written by the step's gather launch ahead of the doorbell
    char* d_results = nullptr;  // the edit's accumulators on the device (its own allocation: zero between edits — cleared behind every collect)
    size_t d_results_bytes = 0;
    // what the meshes of the last edit's invalidated chunks need (chunk -> vertices, indices, kind | flags << 8): valid until voxels change again
    // (ascending by chunk — the grown box is walked in chunk-linear order —, looked up by binary search: a hash map's insertions were most of an
    // edit's collect for the small objects of a many-object frame)
    std::vector<std::array<uint32_t, 4>> needs;  // chunk, vertices, indices, kind | flags << 8
    // early delivery of what the invalidated meshes need (ivx_mesh_sync_enqueue with a null set while the edit is in flight): the role that
    // counts them writes its records into the pinned block behind the results and rings a bell there
    int early_armed = 0, early_taken = 0;
    uint32_t early_seq = 0;
};
void edit_free(ivx_grid* g) {
    ivx_edit_state* e = g->edit;
    g->edit = nullptr;
    if (!e) return;
    ivx_mapped_free(&e->pinned);
    if (e->d_results) (void)hipFree(e->d_results);
    delete e;
}
static ivx_edit_state* edit_state(ivx_grid* g) {
    if (!g->edit) g->edit = new (std::nothrow) ivx_edit_state();
    return g->edit;
}
bool edit_needs_lookup(ivx_grid* g, uint32_t chunk, uint32_t out3[3]) {
    if (!g->edit) return false;
    const auto& v = g->edit->needs;
    const auto it = std::lower_bound(v.begin(), v.end(), chunk, [](const std::array<uint32_t, 4>& a, uint32_t c) { return a[0] < c; });
    if (it == v.end() || (*it)[0] != chunk) return false;
    out3[0] = (*it)[1], out3[1] = (*it)[2], out3[2] = (*it)[3];
    return true;
}

// The edit's blocks hold an edit of these sizes (0: nothing is asked of that block). Both grow to max(2 * need, 64 KiB) and keep nothing; the
// device block starts zeroed (later it is cleared behind every collect), the pinned block is the caller's to clear. `wait`: what is in flight
// on the stream may use the old blocks and is waited for first. (false: the pre-allocation, which asks for one byte of each — no block is
// ever smaller than the 64 KiB floor, so only a block that does not exist yet grows there, and nothing in flight uses that one.)
static int edit_blocks_hold(ivx_edit_state* e, hipStream_t s, size_t dev_bytes, size_t pinned_bytes, bool wait) {
    if (e->d_results_bytes < dev_bytes) {
        if (wait) IVX_HIP_CHECK(ivx_stream_sync(s));
        if (e->d_results) (void)hipFree(e->d_results);
        e->d_results = nullptr, e->d_results_bytes = 0;
        const size_t cap = std::max<size_t>(2 * dev_bytes, 1 << 16);
        IVX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&e->d_results), cap));
        IVX_HIP_CHECK(ivx_memset_async(e->d_results, 0, cap, s));
        e->d_results_bytes = cap;
    }
    return ivx_mapped_grow(&e->pinned, pinned_bytes, std::max<size_t>(2 * pinned_bytes, 1 << 16), wait ? s : nullptr);
}

static int absorb_enqueue(ivx_grid* g, const char* who, int capsule, const float center[3], const float seg[3], float influence_radius, float shape_radius,
                          const float densities[256]) {
    IVX_REQUIRE(g && center && densities && (seg || !capsule), IVX_ERR_INVALID, "%s: null argument", who);
    ivx_many_other_context other_(g->ctx);
    IVX_REQUIRE(influence_radius >= 0.0f && shape_radius >= 0.0f, IVX_ERR_INVALID, "%s: negative radius", who);
    IVX_REQUIRE(g->regions_valid, IVX_ERR_STATE, "%s: derived state and regions must be current (ivx_derive_state + ivx_label_regions)", who);
    IVX_REQUIRE(g->x_off == 0 && g->gx == g->cc[0] && !g->has_ghost[0] && !g->has_ghost[1], IVX_ERR_STATE, "%s: not available on a slab of a decomposed grid",
                who);
    ivx_edit_state* e = edit_state(g);
    IVX_REQUIRE(e, IVX_ERR_CAPACITY, "%s: out of host memory", who);
    IVX_REQUIRE(!e->pending, IVX_ERR_STATE, "%s: an edit of this object is in flight (ivx_absorb_collect first)", who);
    int rc;
    // the touched voxel ranges start from the object's occupied ranges (voxel_ranges_touching_aab, intersection.rs:766-782)
    uint32_t occ[12];
    if ((rc = reference_occupied(g, occ))) return rc;
    float lo_f[3], hi_f[3];
    for (int d = 0; d < 3; ++d) {
        float a = center[d] - influence_radius, b = center[d] + influence_radius;  // Sphere::compute_aabb
        if (capsule) {  // Capsule::compute_aabb: the boxes of the two end spheres (capsule.rs:132-137)
            const float end = center[d] + seg[d];
            const float a1 = end - influence_radius, b1 = end + influence_radius;
            a = a1 < a ? a1 : a;
            b = b1 > b ? b1 : b;
        }
        lo_f[d] = a, hi_f[d] = b;
    }
    long rlo[3], rhi[3];
    int32_t vlo[3], vhi[3];
    uint32_t lo[3], cc[3];
    clamped_ranges(occ, lo_f, hi_f, true, rlo, rhi);
    e->nothing = 0;
    if (!chunk_box(rlo, rhi, vlo, vhi, lo, cc)) {
        e->nothing = 1;  // nothing touched: the collect reports zeros
        e->pending = 1;
        return IVX_OK;
    }
    uint32_t blo[3], bcc[3];  // the box the derive sweep goes over: one chunk more each way
    for (int d = 0; d < 3; ++d) {
        blo[d] = lo[d] > 0u ? lo[d] - 1u : 0u;
        const uint32_t bhi = std::min(lo[d] + cc[d] + 1u, g->cc[d]);
        e->bcc[d] = bcc[d] = bhi - blo[d];
    }
    const size_t grown = (size_t)bcc[0] * bcc[1] * bcc[2];
    e->blk = EditBlock((size_t)cc[0] * cc[1] * cc[2], grown);
    const EditBlock& blk = e->blk;
    hipStream_t s = g->ctx->stream;
    // (a density table other than the resident one rides in the block's LAST kilobyte — not right behind this edit's results: nothing clears it
    // there, and a later, larger edit would read its floats as the touched words of its box: 1.0f is "touched, voxels 0..0, 0..0, 0..8" — five
    // chunks invalidated for nothing in one of 3 600 random edit sequences, profiles/round5/README.md)
    if ((rc = edit_blocks_hold(e, s, ((blk.total + 255) & ~(size_t)255) + 1024, 0, true))) return rc;
    char* base = e->d_results;
    const size_t off_dens = e->d_results_bytes - 1024;
    const float* d_dens = g->dens_dev;
    if (!(g->has_dens && memcmp(g->dens_host, densities, sizeof(g->dens_host)) == 0)) {  // another table than the resident one
        if ((rc = h2d(g, base + off_dens, densities, 1024))) return rc;
        d_dens = reinterpret_cast<const float*>(base + off_dens);
    }
    // the edit; its first block also zeroes the region scalars the sweep behind it starts from
    if ((rc = ivx_launch_absorb(g, capsule, lo, cc, vlo, vhi, center, seg, influence_radius, shape_radius, d_dens, reinterpret_cast<double*>(base),
                                reinterpret_cast<uint32_t*>(base + blk.off_type), reinterpret_cast<uint32_t*>(base + blk.off_cnt),
                                reinterpret_cast<uint32_t*>(base + blk.off_touch), g->rscalar)))
        return rc;
    e->needs.clear();  // (voxels change: what an earlier edit's chunks needed is history)
    // derived state and chunk-local regions of the grown box, the other chunks' region nodes reset; then the global resolve, whose first
    // launch also counts what the invalidated chunks' meshes need, and whose last (the gather of ivx_absorb_collect) copies the edit's small
    // results to the host ahead of the doorbell: seven launches, no copy or fill operation on the stream
    if ((rc = ivx_launch_derive_box(g, IVX_PART_REGIONS, blo, bcc, nullptr))) return rc;
    e->staged = blk.total <= STAGED_COPY_MAX;
    if (e->staged) {
        const size_t had = e->pinned.bytes;
        if ((rc = edit_blocks_hold(e, s, 0, blk.off_bell + 64, true))) return rc;
        if (e->pinned.bytes != had) memset(e->pinned.p, 0, e->pinned.bytes);
    }
    char* const pinned_dev = static_cast<char*>(e->pinned.dev);
    e->early_armed = e->staged && g->early_needs_on;
    e->early_taken = 0;
    if (e->early_armed) {
        e->early_seq += 1u;
        // (the bell's place moves with the size of the box: whatever an earlier, larger edit left there must not read as this edit's number)
        *reinterpret_cast<volatile uint32_t*>(static_cast<char*>(e->pinned.p) + blk.off_bell) = 0u;
    }
    // (early delivery: the words [2], [3] behind the two counters are the block's spare: zero between edits like the rest)
    g->needs_role = ivx_needs_role{{lo[0], lo[1], lo[2], cc[0], cc[1], cc[2], blo[0], blo[1], blo[2], bcc[0], bcc[1], bcc[2]},
                                   reinterpret_cast<const uint32_t*>(base + blk.off_touch),
                                   reinterpret_cast<uint32_t*>(base + blk.off_needs),
                                   e->early_armed ? reinterpret_cast<uint32_t*>(pinned_dev + blk.off_early) : nullptr,
                                   e->early_armed ? reinterpret_cast<uint32_t*>(base + blk.off_cnt) + 2 : nullptr,
                                   e->early_armed ? reinterpret_cast<uint32_t*>(pinned_dev + blk.off_bell) : nullptr,
                                   e->early_armed ? e->early_seq : 0u};
    g->preset_fresh |= IVX_SCRATCH_REGIONS;  // (the region scalars were zeroed by the edit kernel, before the box sweep listed its multi-region chunks)
    g->regions_labelled_locally = 1;         // (... and the sweep labelled the box: no stand-alone local pass in front of the resolve)
    rc = step_enqueue_untimed(g, IVX_STAGE_REGIONS);  // (nobody reads this call's stage times)
    g->regions_labelled_locally = 0;
    if (rc) return rc;
    // (with early delivery the needs records are in the host-mapped block already: the gather copies the words in front of them only)
    if (e->staged)
        g->gather_copy = ivx_gather_copy{reinterpret_cast<const uint32_t*>(base), reinterpret_cast<uint32_t*>(pinned_dev),
                                         (uint32_t)(((e->early_armed ? blk.off_needs : blk.total) + 3) / 4)};
    e->pending = 1;
    return IVX_OK;
}

// The records of the edit's count role — a uint4 per chunk of the grown box: bit 31 | kind | flags << 8, vertices, indices, chunk — become
// e->needs, ascending by chunk; with `invalidated_chunks`, the chunks they name are marked there.
static void edit_take_needs(ivx_grid* g, const uint32_t* needs, uint8_t* invalidated_chunks) {
    ivx_edit_state* e = g->edit;
    const size_t grown = (size_t)e->bcc[0] * e->bcc[1] * e->bcc[2];
    e->needs.clear();
    for (size_t b = 0; b < grown; ++b) {
        const uint32_t w = needs[4 * b];
        if (!(w & 0x80000000u)) continue;
        const uint32_t c = needs[4 * b + 3];
        if (invalidated_chunks) invalidated_chunks[c] = 1;
        e->needs.push_back({c, needs[4 * b + 1], needs[4 * b + 2], w & 0xFFFFu});
    }
    if (!std::is_sorted(e->needs.begin(), e->needs.end(), [](const std::array<uint32_t, 4>& a, const std::array<uint32_t, 4>& b) { return a[0] < b[0]; }))
        std::sort(e->needs.begin(), e->needs.end(), [](const std::array<uint32_t, 4>& a, const std::array<uint32_t, 4>& b) { return a[0] < b[0]; });
    g->needs_current = 1;
}

static int absorb_collect(ivx_grid* g, const char* who, ivx_absorb_result* out, uint32_t* emptied_by_type, uint8_t* invalidated_chunks) {
    IVX_REQUIRE(g && out, IVX_ERR_INVALID, "%s: null argument", who);
    ivx_many_other_context other_(g->ctx);
    ivx_edit_state* e = g->edit;
    IVX_REQUIRE(e && e->pending, IVX_ERR_STATE, "%s: no edit of this object is in flight", who);
    e->pending = 0;
    memset(out, 0, sizeof(*out));
    if (emptied_by_type) memset(emptied_by_type, 0, 256 * sizeof(uint32_t));
    if (invalidated_chunks) memset(invalidated_chunks, 0, g->n_chunks);
    if (e->nothing) return IVX_OK;
    int rc;
    if ((rc = rederive_collect(g))) return rc;  // (the doorbell behind everything enqueued: one wait)
    mesh_sync_stream_drained(g);                // (... a sync enqueued while this edit was in flight included)
    const EditBlock& blk = e->blk;
    std::vector<char> hostbuf;
    const char* hb;
    if (e->staged) {
        hb = static_cast<const char*>(e->pinned.p);
    } else {
        hostbuf.resize(blk.total);
        if ((rc = d2h(g, hostbuf.data(), e->d_results, blk.total))) return rc;
        hb = hostbuf.data();
    }
    // (the accumulators and the touched words start the next edit from zero — and that edit's box may be larger than this one's: everything this
    // edit wrote is cleared now, off the next edit's path; the block beyond has never been written)
    if (!ivx_many_zero(g->ctx, g, e->d_results, (blk.total + 3) & ~(size_t)3)) IVX_HIP_CHECK(ivx_memset_async(e->d_results, 0, blk.total, g->ctx->stream));
    edit_block_result(g, hb, blk, out, emptied_by_type);
    // handle_chunk_voxels_modified (intersection.rs:560-598): the touched chunk, and a neighbour when the touched voxel range of the chunk
    // comes within two voxels of the face they share — decided on the device per chunk of the grown box, with what its mesh needs now
    const uint32_t* needs = reinterpret_cast<const uint32_t*>(e->early_armed ? static_cast<const char*>(e->pinned.p) + blk.off_early : hb + blk.off_needs);
    edit_take_needs(g, needs, invalidated_chunks);  // (an early sync may have taken them from the same records)
    return IVX_OK;
}

// an edit is in flight and has launches behind it (one that touched nothing has none)
static bool edit_has_launches(const ivx_grid* g) { return g->edit && g->edit->pending && !g->edit->nothing; }
void edit_abandon(ivx_grid* g) {
    ivx_absorb_result tmp;
    if (g->edit && g->edit->pending) (void)absorb_collect(g, "ivx_*_many (drain)", &tmp, nullptr, nullptr);
    if (g->edit) g->edit->pending = 0;
}

// what the edit in flight invalidates and what those meshes need, from the records its count role delivers early (ivx_edit_state::early_*):
// waits for the role's bell — a third of the way down the edit's chain —, not for the edit
int edit_early_needs(ivx_grid* g, const char* who, std::vector<uint32_t>& list) {
    ivx_edit_state* e = g->edit;
    IVX_REQUIRE(e && e->pending, IVX_ERR_STATE, "%s: a null set stands for the chunks of an edit in flight, and none is", who);
    if (e->nothing) return IVX_OK;
    IVX_REQUIRE(e->early_armed, IVX_ERR_STATE,
                "%s: the edit in flight does not deliver its mesh needs early (ivx_grid_set_early_mesh_needs before the edit; or its results do not fit the "
                "host-mapped block): collect it and pass its set",
                who);
    if (!e->early_taken) {
        (void)ivx_many_break();
        const char* pinned = static_cast<const char*>(e->pinned.p);
        bool rung = false;
        const int rc = doorbell_wait(reinterpret_cast<const volatile uint32_t*>(pinned + e->blk.off_bell), e->early_seq, 2000000u, g->ctx->stream, &rung);
        if (rc) return rc;
        IVX_REQUIRE(rung, IVX_ERR_HIP, "%s: the edit's mesh needs never arrived", who);
        edit_take_needs(g, reinterpret_cast<const uint32_t*>(pinned + e->blk.off_early), nullptr);
        e->early_taken = 1;
    }
    for (const auto& n : e->needs) list.push_back(n[0]);
    return IVX_OK;
}

int ivx_absorb_sphere_enqueue(ivx_grid* g, const float center[3], float influence_radius, float sphere_radius, const float densities[256]) {
    return absorb_enqueue(g, "ivx_absorb_sphere_enqueue", 0, center, nullptr, influence_radius, sphere_radius, densities);
}
int ivx_absorb_capsule_enqueue(ivx_grid* g, const float segment_start[3], const float segment_vector[3], float influence_radius, float capsule_radius,
                               const float densities[256]) {
    return absorb_enqueue(g, "ivx_absorb_capsule_enqueue", 1, segment_start, segment_vector, influence_radius, capsule_radius, densities);
}
int ivx_absorb_collect(ivx_grid* g, ivx_absorb_result* out, uint32_t* emptied_by_type, uint8_t* invalidated_chunks) {
    return absorb_collect(g, "ivx_absorb_collect", out, emptied_by_type, invalidated_chunks);
}

int ivx_absorb_sphere(ivx_grid* g, const float center[3], float influence_radius, float sphere_radius, const float densities[256], ivx_absorb_result* out,
                      uint32_t* emptied_by_type, uint8_t* invalidated_chunks) {
    IVX_REQUIRE(out, IVX_ERR_INVALID, "ivx_absorb_sphere: null argument");
    const int rc = absorb_enqueue(g, "ivx_absorb_sphere", 0, center, nullptr, influence_radius, sphere_radius, densities);
    return rc ? rc : absorb_collect(g, "ivx_absorb_sphere", out, emptied_by_type, invalidated_chunks);
}

int ivx_absorb_capsule(ivx_grid* g, const float segment_start[3], const float segment_vector[3], float influence_radius, float capsule_radius,
                       const float densities[256], ivx_absorb_result* out, uint32_t* emptied_by_type, uint8_t* invalidated_chunks) {
    IVX_REQUIRE(out, IVX_ERR_INVALID, "ivx_absorb_capsule: null argument");
    const int rc = absorb_enqueue(g, "ivx_absorb_capsule", 1, segment_start, segment_vector, influence_radius, capsule_radius, densities);
    return rc ? rc : absorb_collect(g, "ivx_absorb_capsule", out, emptied_by_type, invalidated_chunks);
}

// ---- many objects per call (many.hpp; the recorder phases are ivx_api.hip's) ---------------------------------------------------------------
// one absorber per object: spheres (segments3 == NULL) or capsules (segment vectors, 3 floats per object)
static int absorb_many(ivx_grid* const* grids, size_t n, const char* who, const float* points3, const float* segments3, const float* influence_radii,
                       const float* shape_radii, const float densities[256], ivx_absorb_result* out, uint8_t* const* invalidated_chunks) {
    if (n == 0) return IVX_OK;  // (a manager without voxel objects)
    int rc = many_check(grids, n, who);
    if (rc) return rc;
    ManyClock clk("absorb");
    IVX_REQUIRE(points3 && influence_radii && shape_radii && densities && out, IVX_ERR_INVALID, "%s: null argument", who);
    // (what an object's enqueue may have to wait for — its occupied ranges, a density table that is not the resident one — before the recording starts)
    for (size_t i = 0; i < n; ++i) {
        uint32_t occ[12];
        if (grids[i]->regions_valid && (rc = reference_occupied(grids[i], occ))) return rc;
        // (... and the object's edit buffers, which its first edit would otherwise allocate — with a wait on the stream — in the middle of the batch)
        ivx_edit_state* e = edit_state(grids[i]);
        IVX_REQUIRE(e, IVX_ERR_CAPACITY, "%s: out of host memory", who);
        if ((rc = edit_blocks_hold(e, grids[i]->ctx->stream, 1, 1, false))) return rc;
    }
    clk.lap("prepare");
    if ((rc = many_phase(grids, n, [&](size_t i) {
             return absorb_enqueue(grids[i], who, segments3 ? 1 : 0, points3 + 3 * i, segments3 ? segments3 + 3 * i : nullptr, influence_radii[i], shape_radii[i], densities);
         })))
        return many_fail(grids, n, rc);
    clk.lap("enqueue + flush");
    if ((rc = many_phase(grids, n, [&](size_t i) { return edit_has_launches(grids[i]) ? ivx_step_collect_launch(grids[i]) : IVX_OK; })))
        return many_fail(grids, n, rc);
    clk.lap("gathers");
    rc = many_phase(grids, n, [&](size_t i) { return absorb_collect(grids[i], who, &out[i], nullptr, invalidated_chunks ? invalidated_chunks[i] : nullptr); });
    clk.lap("collect");
    return many_fail(grids, n, rc);
}
int ivx_absorb_sphere_many(ivx_grid* const* grids, size_t n, const float* centers3, const float* influence_radii, const float* sphere_radii,
                           const float densities[256], ivx_absorb_result* out, uint8_t* const* invalidated_chunks) {
    return absorb_many(grids, n, "ivx_absorb_sphere_many", centers3, nullptr, influence_radii, sphere_radii, densities, out, invalidated_chunks);
}
int ivx_absorb_capsule_many(ivx_grid* const* grids, size_t n, const float* segment_starts3, const float* segment_vectors3, const float* influence_radii,
                            const float* capsule_radii, const float densities[256], ivx_absorb_result* out, uint8_t* const* invalidated_chunks) {
    IVX_REQUIRE(n == 0 || segment_vectors3, IVX_ERR_INVALID, "ivx_absorb_capsule_many: null argument");
    return absorb_many(grids, n, "ivx_absorb_capsule_many", segment_starts3, segment_vectors3, influence_radii, capsule_radii, densities, out, invalidated_chunks);
}

// ---- two objects absorbing each other ------------------------------------------------------------------------------------------------------
// apply_mutual_absorption (interaction/absorption.rs:891-1079). The overlap geometry is the collision unit's (host_intersection_ranges); the
// two result blocks live in A's device scratch, not in the edit state: the call waits for its results itself.
int ivx_absorb_mutual(ivx_grid* a, const float rotation_a[4], const float translation_a[3], const float densities_a[256], ivx_grid* b, const float rotation_b[4],
                      const float translation_b[3], const float densities_b[256], float smoothness, ivx_absorb_result* out_a, ivx_absorb_result* out_b,
                      uint8_t* invalidated_chunks_a, uint8_t* invalidated_chunks_b) {
    const char* who = "ivx_absorb_mutual";
    IVX_REQUIRE(a && b && rotation_a && translation_a && densities_a && rotation_b && translation_b && densities_b && out_a && out_b, IVX_ERR_INVALID,
                "%s: null argument", who);
    IVX_REQUIRE(a != b && a->ctx == b->ctx, IVX_ERR_INVALID, "%s: two different objects of one context are needed", who);
    IVX_REQUIRE(smoothness >= 0.0f, IVX_ERR_INVALID, "%s: negative smoothness", who);
    int rc;
    for (ivx_grid* g : {a, b})
        if ((rc = require_whole_object(g, who, false))) return rc;
    memset(out_a, 0, sizeof(*out_a));
    memset(out_b, 0, sizeof(*out_b));
    if (invalidated_chunks_a) memset(invalidated_chunks_a, 0, a->n_chunks);
    if (invalidated_chunks_b) memset(invalidated_chunks_b, 0, b->n_chunks);
    uint32_t occ_a[12], occ_b[12];
    if ((rc = ivx_reference_occupied(a, who, occ_a))) return rc;
    if ((rc = ivx_reference_occupied(b, who, occ_b))) return rc;
    long ra_lo[3], ra_hi[3], rb_lo[3], rb_hi[3];
    float q_ba[4], t_ba[3];
    if (!host_intersection_ranges(a, occ_a, rotation_a, translation_a, b, occ_b, rotation_b, translation_b, ra_lo, ra_hi, rb_lo, rb_hi, q_ba, t_ba)) return IVX_OK;
    // the snapshot of A's distances covers A's overlap ranges padded by one B voxel (in A voxels), inside A's grid
    const long pad = (long)std::ceil(b->extent * (1.0f / a->extent));
    for (int d = 0; d < 3; ++d) {
        ra_lo[d] = std::max<long>(0, ra_lo[d] - pad);
        ra_hi[d] = std::min<long>(ra_hi[d] + pad, (long)a->cc[d] * 16);
    }
    int32_t s_lo[3], s_hi[3], vb_lo[3], vb_hi[3];
    uint32_t lo_a[3], cc_a[3], lo_b[3], cc_b[3];
    const bool a_runs = chunk_box(ra_lo, ra_hi, s_lo, s_hi, lo_a, cc_a), b_runs = chunk_box(rb_lo, rb_hi, vb_lo, vb_hi, lo_b, cc_b);
    const size_t snap_bytes = a_runs ? (size_t)(s_hi[0] - s_lo[0]) * (size_t)(s_hi[1] - s_lo[1]) * (size_t)(s_hi[2] - s_lo[2]) : 0;
    if (!a_runs && !b_runs) return IVX_OK;
    // scratch (A's): a result block per object, then the two density tables, then the snapshot
    // (the touched ranges are indexed by the chunk's position in the object's chunk box; the boxes are known further down, a whole grid bounds them)
    const EditBlock blocks[2] = {EditBlock(a->n_chunks), EditBlock(b->n_chunks)};
    const size_t blk_a = (blocks[0].off_needs + 255) & ~(size_t)255, blk_b = (blocks[1].off_needs + 255) & ~(size_t)255;
    const size_t off_dens = blk_a + blk_b, off_snap = off_dens + 2048;
    if ((rc = ensure_dev_scratch(a, off_snap + snap_bytes + 256))) return rc;
    char* base = static_cast<char*>(a->dev_scratch);
    IVX_HIP_CHECK(ivx_memset_async(base, 0, off_dens, a->ctx->stream));
    if ((rc = h2d(a, base + off_dens, densities_a, 1024))) return rc;
    if ((rc = h2d(a, base + off_dens + 1024, densities_b, 1024))) return rc;
    int8_t* d_snap = reinterpret_cast<int8_t*>(base + off_snap);
    if (a_runs) {
        if ((rc = ivx_launch_sdf_snapshot(a, s_lo, s_hi, d_snap))) return rc;
        if ((rc = ivx_launch_absorb_mutual(a, 0, lo_a, cc_a, s_lo, s_hi, b, nullptr, s_lo, s_hi, q_ba, t_ba, smoothness, reinterpret_cast<float*>(base + off_dens),
                                           reinterpret_cast<double*>(base), reinterpret_cast<uint32_t*>(base + blocks[0].off_type),
                                           reinterpret_cast<uint32_t*>(base + blocks[0].off_cnt), reinterpret_cast<uint32_t*>(base + blocks[0].off_touch))))
            return rc;
    }
    if (b_runs) {
        char* bb = base + blk_a;
        if ((rc = ivx_launch_absorb_mutual(b, 1, lo_b, cc_b, vb_lo, vb_hi, a, d_snap, s_lo, s_hi, q_ba, t_ba, smoothness,
                                           reinterpret_cast<float*>(base + off_dens + 1024), reinterpret_cast<double*>(bb),
                                           reinterpret_cast<uint32_t*>(bb + blocks[1].off_type), reinterpret_cast<uint32_t*>(bb + blocks[1].off_cnt),
                                           reinterpret_cast<uint32_t*>(bb + blocks[1].off_touch))))
            return rc;
    }
    std::vector<char> hostbuf(off_dens);
    if ((rc = d2h(a, hostbuf.data(), base, off_dens))) return rc;
    if (a_runs && (rc = rederive(a))) return rc;
    if (b_runs && (rc = rederive(b))) return rc;
    for (int w = 0; w < 2; ++w) {
        ivx_grid* g = w ? b : a;
        if (!(w ? b_runs : a_runs)) continue;
        const char* hb = hostbuf.data() + (w ? blk_a : 0);
        uint8_t* inval = w ? invalidated_chunks_b : invalidated_chunks_a;
        const uint32_t* lo = w ? lo_b : lo_a;
        const uint32_t* cc = w ? cc_b : cc_a;
        edit_block_result(g, hb, blocks[w], w ? out_b : out_a, nullptr);
        if (!inval) continue;
        const uint32_t* touched = reinterpret_cast<const uint32_t*>(hb + blocks[w].off_touch);  // handle_chunk_voxels_modified (intersection.rs:560-598)
        for (uint32_t i = lo[0]; i < lo[0] + cc[0]; ++i)
            for (uint32_t j = lo[1]; j < lo[1] + cc[1]; ++j)
                for (uint32_t k = lo[2]; k < lo[2] + cc[2]; ++k) {
                    const uint32_t c = (i * g->cc[1] + j) * g->cc[2] + k;
                    const uint32_t wd = touched[((i - lo[0]) * cc[1] + (j - lo[1])) * cc[2] + (k - lo[2])];
                    if (!wd) continue;
                    inval[c] = 1;
                    const uint32_t idx[3] = {i, j, k};
                    for (int d = 0; d < 3; ++d) {
                        const uint32_t rlo = (wd >> (4 * d)) & 15u, rhi = ((wd >> (12 + 4 * d)) & 15u) + 1u;
                        uint32_t n3[3] = {i, j, k};
                        if (idx[d] > 0 && rlo < 2) {
                            n3[d] = idx[d] - 1;
                            inval[(n3[0] * g->cc[1] + n3[1]) * g->cc[2] + n3[2]] = 1;
                        }
                        if (idx[d] + 1 < g->cc[d] && 16u - rhi < 2) {
                            n3[d] = idx[d] + 1;
                            inval[(n3[0] * g->cc[1] + n3[1]) * g->cc[2] + n3[2]] = 1;
                        }
                    }
                }
    }
    return IVX_OK;
}
