// What the host units of the C ABI (ivx_api.hip, step_api.hip, edit_api.hip, voxel_collision_api.hip, extraction_api.hip, mesh_api.hip) share
// and nothing else links against: staged copies, the objects' device scratch, the cached occupied ranges, the bounded wait for a doorbell, the
// recorder phases of the many-object calls, what the extraction calls need of the grid life cycle, the regions and the step, what crosses
// between the edit unit, the mesh unit and the rest, the overlap ranges of two objects, and the host mirrors of the reference's range
// allocators. Defined in ivx_api.hip unless said otherwise (the functions hidden: the library exports what it exported before).
#pragma once
#include <atomic>
#include <chrono>
#include <functional>
#include <limits>
#include <map>
#include <unordered_map>
#include <vector>

#include "device_common.hpp"

#pragma GCC visibility push(hidden)

template <class T>
int dev_alloc(T** p, size_t count) {
    *p = nullptr;
    if (count == 0) return IVX_OK;
    IVX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T)));
    return IVX_OK;
}

// Host<->device copies through the grid's pinned staging buffer: ONE stream-ordered copy and ONE wait (larger than STAGED_COPY_MAX: plain
// blocking copies; an edit with larger results than that brings them back by such a copy)
constexpr size_t STAGED_COPY_MAX = 1u << 20;
int d2h(ivx_grid* g, void* dst, const void* src, size_t bytes);
int h2d(ivx_grid* g, void* dst, const void* src, size_t bytes);
// the object's device scratch (ivx_grid::dev_scratch) holds at least `bytes`; a growth waits for the stream and keeps nothing
int ensure_dev_scratch(ivx_grid* g, size_t bytes);
// a shared allocation (ivx_block, ivx_internal.hpp) let go of by one holder: freed with the last
void block_release(ivx_block* b);
// the occupied ranges in the reference's sense (ivx_grid::occ_ref), cached (ivx_reference_occupied: this behind a check that the object was derived)
int reference_occupied(ivx_grid* g, uint32_t occ[12]);

// A doorbell: a word of host-mapped memory that a kernel writes last (in-order stream: everything enqueued before it is complete too). A short
// chain is over before the runtime's blocking wait has gone to sleep and been woken again: the word is polled for at most `budget_ns` (0: never),
// then the stream is waited for. `rung`: the bell holds `want` (false behind a drained stream: its kernel never ran).
inline int doorbell_wait(const volatile uint32_t* bell, uint32_t want, uint64_t budget_ns, hipStream_t s, bool* rung) {
    *rung = false;
    if (budget_ns) {
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t it = 0; !(*rung = *bell == want); ++it) {
            __builtin_ia32_pause();
            if ((it & 255u) == 255u && (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count() > budget_ns) break;
        }
    }
    if (!*rung) IVX_HIP_CHECK(ivx_stream_sync(s));
    std::atomic_thread_fence(std::memory_order_acquire);
    *rung = *bell == want;
    return IVX_OK;
}

// box sweep + region stages after an edit that changed voxels, enqueued and collected (extraction_api.hip): both halves, and the two apart for a
// caller that has results of its own in flight behind the same doorbell
int rederive(ivx_grid* g);
int rederive_enqueue(ivx_grid* g);
int rederive_collect(ivx_grid* g);

// for extraction_api.hip: grids that come into being together, from one device block and one pinned block (`who`: the call, for messages) | the
// descriptors of all regions of a labelled object
int grid_create_pooled(ivx_ctx* c, const uint32_t* ccs, size_t n, float voxel_extent, ivx_grid** out, const char* who);
int describe_regions_internal(ivx_grid* g, const float* d_dens, std::vector<ivx_region_desc>& out);
// the step unit (step_api.hip): a step's launches with no slot timed, whatever ivx_grid_set_stage_timing asked for (the one place that masks
// timing) | the launch half of ivx_voxel_step_collect (many_fail calls the public half) | the stage clock's words and events given up
int step_enqueue_untimed(ivx_grid* g, uint32_t stages);
int ivx_step_collect_launch(ivx_grid* g);
void stage_clock_free(ivx_grid* g);

// What the collision and extraction calls ask of an object: derived state current, (needs_probes) probes picked from the current mesh, not a
// slab of a decomposed grid. `item` non-null names the object or pair of a batched call in the message ("object 3: ...").
inline int require_whole_object(const ivx_grid* g, const char* who, bool needs_probes, const char* item = nullptr, size_t index = 0) {
    const char* missing = nullptr;
    if (!g->regions_valid) missing = "derived state must be current (ivx_derive_state + ivx_label_regions)";
    else if (needs_probes && !(g->mesh_valid && g->probes_serial == g->mesh_serial)) missing = "collision probes must be current (ivx_collision_probes_recompute)";
    else if (!(g->x_off == 0 && g->gx == g->cc[0] && !g->has_ghost[0] && !g->has_ghost[1])) missing = "not available on a slab of a decomposed grid";
    if (!missing) return IVX_OK;
    if (item) ivx_set_error("%s: %s %zu: %s", who, item, index, missing);
    else ivx_set_error("%s: %s", who, missing);
    return IVX_ERR_STATE;
}

// many objects per call (many.hpp): the objects of one context, each listed once | `f(i)` for every object under the recorder, then the flush |
// the drain after a failure half way (the first two in many.cpp: they need nothing of a grid but its context)
int many_check(ivx_grid* const* grids, size_t n, const char* who);
int many_phase(ivx_grid* const* grids, size_t n, const std::function<int(size_t)>& f);
int many_fail(ivx_grid* const* grids, size_t n, int rc);

// developer aid: IVX_MANY_TRACE=1 prints the host time of every phase of the many-object calls (and, summed over a period, of a sync's enqueue)
inline bool many_trace() {
    static const bool on = getenv("IVX_MANY_TRACE") != nullptr;
    return on;
}
struct ManyClock {
    const char* what;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit ManyClock(const char* w) : what(w) {}
    double lap_us() {  // since the lap before
        const auto t1 = std::chrono::steady_clock::now();
        const double us = 1e-3 * (double)std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count();
        t0 = t1;
        return us;
    }
    void lap(const char* phase) {
        if (many_trace()) fprintf(stderr, "[ivx many] %s %s: %.1f us\n", what, phase, lap_us());
    }
};

// ---- the edit unit (edit_api.hip), the mesh unit (mesh_api.hip) and the rest (ivx_api.hip, step_api.hip, voxel_collision_api.hip) ----------------------
// grid -> edit: the edit state is given up (ivx_grid_destroy) | many -> edit: the edit in flight, if any, is collected, its results discarded (many_fail)
void edit_free(ivx_grid* g);
void edit_abandon(ivx_grid* g);
// edit -> collision (voxel_collision_api.hip): the voxel ranges that hold two objects' overlap, b's frame -> a's; false: the boxes do not meet
bool host_intersection_ranges(const ivx_grid* a, const uint32_t occ_a[12], const float rotation_a[4], const float translation_a[3], const ivx_grid* b,
                              const uint32_t occ_b[12], const float rotation_b[4], const float translation_b[3], long ra_lo[3], long ra_hi[3], long rb_lo[3],
                              long rb_hi[3], float q_ba[4], float t_ba[3]);
// mesh -> edit: what the mesh of `chunk` needs (vertices, indices, kind | flags << 8) when the last edit counted it | the chunks the edit in
// flight invalidates, from the records its count role delivers early (waits for the role's bell, not for the edit)
bool edit_needs_lookup(ivx_grid* g, uint32_t chunk, uint32_t out3[3]);
int edit_early_needs(ivx_grid* g, const char* who, std::vector<uint32_t>& list);
// edit / many -> mesh: the stream was drained behind the launches of the sync in flight, if there is one (its collect has nothing to wait for)
// | the sync in flight, if there is one, is given up: collected without a wait, its counts discarded (many_fail, after its own drain)
void mesh_sync_stream_drained(ivx_grid* g);
void mesh_sync_abandon(ivx_grid* g);
// step / many -> mesh. Capacities a growth gives for the needed counts (vertices, indices, submeshes): max(2 n + slack, 2 cap) when the mesh is
// rebuilt, max(n + n / 2 + slack, 2 cap) when it keeps what it holds; the slack 4096, 24576, 64. The caller takes those of the groups that grow.
void mesh_grown_capacities(const size_t need[3], const size_t cap[3], bool keep, size_t out[3]);
// ... room for a mesh rebuilt in full (contents are not kept) | the mesh arrays of several grids from ONE device allocation, `caps3`: the three
// capacities per grid | "a full mesh of these totals now stands here" | the arrays of a group given up (ivx_grid_destroy)
int ensure_mesh_capacity(ivx_grid* g, size_t nv, size_t ni, size_t ns);
int mesh_pool_assign(ivx_grid* const* grids, size_t n, const size_t* caps3);
void mesh_adopt_full(ivx_grid* g, const uint32_t totals[3]);
void mesh_group_free(ivx_grid* g, uint32_t group);
static inline void mesh_set_counts(ivx_grid* g, const uint32_t totals[3]) { g->mesh_counts = ivx_mesh_counts{totals[0], totals[1], totals[2], 0}; }

static inline uint32_t linear_chunk(const ivx_grid* g, const uint32_t c[3]) { return (c[0] * g->cc[1] + c[1]) * g->cc[2] + c[2]; }

// grow device arrays keeping what they hold: every array that has to grow gets its new block and its copy on the stream, then ONE wait by the
// caller, then the old blocks go (a wait per array was most of what a growth cost)
struct GrowKeep {
    void** slot;
    void* fresh;
    uint32_t group;  // the mesh group the array belongs to (mesh_group_free, mesh_api.hip); 0: none
};
template <class T>
int grow_keep_enqueue(ivx_grid* g, T** buf, size_t old_count, size_t new_count, std::vector<GrowKeep>& pending, uint32_t group) {
    T* fresh = nullptr;
    int rc = dev_alloc(&fresh, new_count);
    if (rc) return rc;
    if (*buf && old_count) IVX_HIP_CHECK(ivx_memcpy_async(fresh, *buf, old_count * sizeof(T), hipMemcpyDeviceToDevice, g->ctx->stream));
    pending.push_back(GrowKeep{reinterpret_cast<void**>(buf), fresh, group});
    return IVX_OK;
}

#pragma GCC visibility pop

// Host mirror of a RangeAllocator (impact_containers/src/range_allocator.rs)
struct ivx_range_allocator {
    std::map<size_t, size_t> free_ranges;  // start -> end; a second range with the same start is dropped, as BTreeSet::insert does
    void free_range(size_t a, size_t b) {
        if (a < b) free_ranges.emplace(a, b);
    }
    bool allocate(size_t len, size_t* start) {  // the smallest free range that fits, the first of equals
        auto best = free_ranges.end();
        size_t best_len = std::numeric_limits<size_t>::max();
        for (auto it = free_ranges.begin(); it != free_ranges.end(); ++it) {
            const size_t l = it->second - it->first;
            if (l < best_len && l >= len) best = it, best_len = l;
        }
        if (best == free_ranges.end()) return false;
        const size_t a = best->first, b = best->second;
        free_ranges.erase(best);
        if (a + len < b) free_ranges.emplace(a + len, b);
        *start = a;
        return true;
    }
    void merge_consecutive() {  // (in place: a range that starts where the one before it ends is folded into that one)
        if (free_ranges.size() < 2) return;
        auto prev = free_ranges.begin();
        for (auto it = std::next(prev); it != free_ranges.end();) {
            if (it->first == prev->second) {
                prev->second = it->second;
                it = free_ranges.erase(it);
            } else {
                prev = it;
                ++it;
            }
        }
    }
};
// Host mirror of the ChunkSubmeshManager (mesh.rs:699-849) with its two RangeAllocators: which slot of the submesh table a chunk owns and which
// ranges of the vertex / index buffers are free. The mesh data stays in HBM. (The probes' sync reads which chunks have a submesh from it.)
struct ivx_submesh_manager {
    std::vector<ivx_submesh> table;                   // slot order = the reference's chunk_submeshes order
    std::unordered_map<uint32_t, uint32_t> slot_of;   // linear chunk index -> slot
    ivx_range_allocator vertices, indices;
    size_t total_vertices = 0, total_indices = 0;     // buffer lengths (freed ranges inside them stay counted)
    std::vector<ivx_submesh_data_ranges> updated;     // VoxelMeshModifications (mesh.rs:113-123) since the last report
    bool chunks_were_removed = false;
    uint64_t serial = 0;                              // the mesh_serial this state describes
    // the sync in flight (no manager: none)
    int sync_pending = 0;
    int sync_drained = 0;          // an edit's collect has waited for a doorbell that was rung behind this sync's launches: nothing left to wait for
    ivx_mapped pinned_up;          // (host-mapped: the sync's kernels read their small lists in place)
    hipEvent_t up_done = nullptr;  // the last upload from pinned_up has been read
    int up_busy = 0;
};
// VoxelObjectCollisionProbes' bookkeeping (collidable.rs:97-101): chunk -> range of the point buffer, free ranges
struct ivx_probe_manager {
    std::unordered_map<uint32_t, std::pair<uint32_t, uint32_t>> range_of;  // linear chunk index -> [start, end)
    ivx_range_allocator points;
    size_t total = 0;  // length of the point buffer, freed ranges included
    bool built = true;  // false right after a recompute: the map is filled from the device entries when somebody needs it
};
