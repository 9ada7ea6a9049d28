// Mesh host code of libimpact_voxel_hip.so: where an object's mesh arrays live and how they grow, the full remesh, the incremental remesh
// (VoxelObjectMesh::sync_with_voxel_object) with its host mirror of the ChunkSubmeshManager, and what hands the arrays to a caller: download,
// device pointers, export and import. Host-side orchestration only: the kernels are the mesher's, behind the ivx_launch_* functions of
// surface_nets.hip. What the edit and step units (edit_api.hip, step_api.hip) and this unit ask of each other is declared in ivx_host.hpp.
#include <algorithm>
#include <array>
#include <cstring>
#include <new>
#include <vector>

#include <dlfcn.h>

#include "ivx_host.hpp"

namespace {
// The six mesh arrays of a grid, in the order of their parts in a pooled block. `group`: the bit of ivx_grid::mesh_pooled and the unit of a
// growth (1: per vertex, 2: per index, 4: per submesh); `bound`: the capacity that counts the array's elements (0 vcap, 1 icap, 2 scap);
// `kept`: a growth that keeps the mesh copies the contents (the vertex scratch holds nothing between launches).
struct MeshArray {
    void** slot;
    size_t elem;
    uint32_t group;
    int bound;
    bool kept;
};
std::array<MeshArray, 6> mesh_arrays(ivx_grid* g) {
    auto at = [](auto** p) { return reinterpret_cast<void**>(p); };
    return {{{at(&g->positions), 12, 1u, 0, true},
             {at(&g->normals), 12, 1u, 0, true},
             {at(&g->vertex_materials), 16, 1u, 0, false},
             {at(&g->indices), 4, 2u, 1, true},
             {at(&g->index_materials), 8, 2u, 1, true},
             {at(&g->submeshes), sizeof(ivx_submesh), 4u, 2, true}}};
}
// the arrays a caller can ask for (`which` of ivx_mesh_download's order, ivx_mesh_device_ptr and ivx_mesh_export): all but the vertex scratch
constexpr int N_HANDED_OUT = 5;
MeshArray handed_out(ivx_grid* g, int which) { return mesh_arrays(g)[which < 2 ? which : which + 1]; }

size_t* capacities(ivx_grid* g, int bound) { return bound == 0 ? &g->vcap : (bound == 1 ? &g->icap : &g->scap); }
void set_capacities(ivx_grid* g, const size_t caps[3]) { g->vcap = caps[0], g->icap = caps[1], g->scap = caps[2]; }
void give_up_all(ivx_grid* g) { mesh_group_free(g, 1u), mesh_group_free(g, 2u), mesh_group_free(g, 4u); }

int new_block(ivx_block** out) {
    ivx_block* blk = *out = new (std::nothrow) ivx_block();
    IVX_REQUIRE(blk, IVX_ERR_CAPACITY, "mesh buffers: out of host memory");
    blk->dev = blk->pinned = nullptr;
    blk->refs = 0;
    return IVX_OK;
}
}  // namespace

void mesh_grown_capacities(const size_t need[3], const size_t cap[3], bool keep, size_t out[3]) {
    // (slack: under the reference's range allocator an edited mesh's buffers grow — a re-meshed chunk that needs a little more than it had goes
    // to the end — by about as much again before freed ranges start to be reused; 2 x 48 B per vertex is nothing next to 288 GB. A growth by copy
    // costs allocations, device copies and a wait — the price of hundreds of small objects' syncs when each of them outgrows its buffers by a few
    // vertices per frame: double, and never by less than a few thousand elements.)
    static const size_t slack[3] = {4096, 24576, 64};
    for (int b = 0; b < 3; ++b) out[b] = std::max((keep ? need[b] + need[b] / 2 : 2 * need[b]) + slack[b], 2 * cap[b]);
}

// the mesh arrays of a group given up: freed, or — parts of a shared block — just let go, the block with its last part
void mesh_group_free(ivx_grid* g, uint32_t group) {
    const bool pooled = (g->mesh_pooled & group) != 0u;
    for (const MeshArray& a : mesh_arrays(g)) {
        if (a.group != group) continue;
        if (*a.slot && !pooled) (void)hipFree(*a.slot);
        *a.slot = nullptr;
    }
    if (pooled) {
        g->mesh_pooled &= ~group;
        if (!g->mesh_pooled) {
            block_release(g->mesh_block);
            g->mesh_block = nullptr;
        }
    }
}

// Mesh arrays for several grids from ONE device allocation (the fragments of an impact meet their first mesh together); whatever the grids held
// before is given up. Every array starts on a 256-byte boundary.
int mesh_pool_assign(ivx_grid* const* grids, size_t n, const size_t* caps3) {
    if (n == 0) return IVX_OK;
    ivx_layout sizes;
    for (size_t i = 0; i < n; ++i)
        for (const MeshArray& a : mesh_arrays(grids[i])) (void)sizes.take(caps3[3 * i + a.bound] * a.elem);
    ivx_block* blk;
    if (int rc = new_block(&blk)) return rc;
    if (hipMalloc(&blk->dev, sizes.bytes) != hipSuccess) {
        delete blk;
        ivx_set_error("mesh buffers: device allocation of %zu bytes for %zu objects failed", sizes.bytes, n);
        return IVX_ERR_HIP;
    }
    ivx_layout parts;
    for (size_t i = 0; i < n; ++i) {
        ivx_grid* g = grids[i];
        give_up_all(g);
        for (const MeshArray& a : mesh_arrays(g)) *a.slot = static_cast<char*>(blk->dev) + parts.take(caps3[3 * i + a.bound] * a.elem);
        set_capacities(g, caps3 + 3 * i);
        g->mesh_block = blk;
        g->mesh_pooled = 7u;
        g->mesh_generation += 1;
        blk->refs += 1;
    }
    return IVX_OK;
}

namespace {
// Developer experiment (IVX_MESH_ARENA=<mode>, IVX_MESH_PHASE=<bytes>): the mesher's four output arrays (+ the vertex scratch) carved from ONE
// allocation at chosen relative offsets — array k starts `k * phase` bytes past its 2 MiB-aligned place. mode 1: hipMalloc; 2: one physically
// contiguous block (hipExtMallocWithFlags(hipDeviceMallocContiguous)). What the mesher's run-to-run modes do NOT depend on.
int mesh_arena_mode() {
    static const int m = [] {
        const char* e = getenv("IVX_MESH_ARENA");
        return e ? atoi(e) : 0;
    }();
    return m;
}
int ensure_mesh_block(ivx_grid* g, size_t nv, size_t ni) {
    if (nv <= g->vcap && ni <= g->icap) return IVX_OK;
    IVX_HIP_CHECK(ivx_stream_sync(g->ctx->stream));
    static const size_t phase = [] {
        const char* e = getenv("IVX_MESH_PHASE");
        return (size_t)(e ? strtoull(e, nullptr, 0) : 0ull);
    }();
    const size_t need[3] = {nv, ni, 0}, have[3] = {g->vcap, g->icap, g->scap};
    size_t caps[3];
    mesh_grown_capacities(need, have, false, caps);
    caps[2] = g->scap;  // (the submeshes stay where they are)
    const std::array<MeshArray, 6> arrays = mesh_arrays(g);
    static const int order[5] = {0, 1, 3, 4, 2};  // k: positions, normals, indices, index materials, vertex scratch
    ivx_layout places;
    places.align = 2u << 20;
    size_t off[5], total = 0;
    for (int k = 0; k < 5; ++k) {
        const size_t bytes = caps[arrays[order[k]].bound] * arrays[order[k]].elem;
        off[k] = places.take((size_t)k * phase + bytes) + (size_t)k * phase;
        total = off[k] + bytes;
    }
    mesh_group_free(g, 1u), mesh_group_free(g, 2u);
    g->vcap = g->icap = 0;
    ivx_block* blk;
    if (int rc = new_block(&blk)) return rc;
    blk->refs = 1;
    if ((mesh_arena_mode() == 2 ? hipExtMallocWithFlags(&blk->dev, total, hipDeviceMallocContiguous) : hipMalloc(&blk->dev, total)) != hipSuccess) {
        delete blk;
        ivx_set_error("mesh buffers: device allocation of %zu bytes failed", total);
        return IVX_ERR_HIP;
    }
    for (int k = 0; k < 5; ++k) *arrays[order[k]].slot = static_cast<char*>(blk->dev) + off[k];
    set_capacities(g, caps);
    if (g->mesh_block) block_release(g->mesh_block);  // (only the submeshes of an earlier shared block can still be there: they move out below)
    g->mesh_block = blk;
    g->mesh_pooled = 3u;
    g->mesh_generation += 1;
    return IVX_OK;
}
}  // namespace

int ensure_mesh_capacity(ivx_grid* g, size_t nv, size_t ni, size_t ns) {
    if (mesh_arena_mode())
        if (int rc = ensure_mesh_block(g, nv, ni)) return rc;
    const size_t need[3] = {nv, ni, ns}, have[3] = {g->vcap, g->icap, g->scap};
    size_t caps[3];
    mesh_grown_capacities(need, have, false, caps);
    if (nv > g->vcap || ni > g->icap || ns > g->scap) g->mesh_generation += 1;
    for (int b = 0; b < 3; ++b) {
        if (need[b] <= have[b]) continue;
        mesh_group_free(g, 1u << b);
        *capacities(g, b) = 0;
        for (const MeshArray& a : mesh_arrays(g))
            if (a.bound == b) IVX_HIP_CHECK(hipMalloc(a.slot, caps[b] * a.elem));
        *capacities(g, b) = caps[b];
    }
    return IVX_OK;
}

namespace {
// grow the mesh buffers keeping what they hold (the full remesh may simply reallocate, a sync may not): grow_keep_enqueue, ivx_host.hpp
int ensure_mesh_capacity_keep(ivx_grid* g, size_t nv, size_t ni, size_t ns) {
    const size_t need[3] = {nv, ni, ns}, have[3] = {g->vcap, g->icap, g->scap};
    if (!(nv > g->vcap || ni > g->icap || ns > g->scap)) return IVX_OK;
    g->mesh_generation += 1;
    std::vector<GrowKeep> pending;
    struct FreeOnError {  // (a failed allocation further down must not leak the blocks made so far)
        std::vector<GrowKeep>& p;
        bool armed = true;
        ~FreeOnError() {
            if (armed)
                for (GrowKeep& k : p) (void)hipFree(k.fresh);
        }
    } guard{pending};
    size_t caps[3];
    mesh_grown_capacities(need, have, true, caps);
    uint32_t groups = 0;
    for (const MeshArray& a : mesh_arrays(g)) {
        if (need[a.bound] <= have[a.bound]) continue;
        groups |= a.group;
        if (int rc = grow_keep_enqueue(g, reinterpret_cast<char**>(a.slot), a.kept ? have[a.bound] * a.elem : 0, caps[a.bound] * a.elem, pending, a.group)) return rc;
    }
    IVX_HIP_CHECK(ivx_stream_sync(g->ctx->stream));
    guard.armed = false;
    for (int b = 0; b < 3; ++b)
        if (groups & (1u << b)) mesh_group_free(g, 1u << b);  // (the old arrays: freed, or let go of as parts of a shared block)
        else caps[b] = have[b];
    for (GrowKeep& k : pending) *k.slot = k.fresh;
    set_capacities(g, caps);
    return IVX_OK;
}
}  // namespace

void mesh_adopt_full(ivx_grid* g, const uint32_t totals[3]) {
    mesh_set_counts(g, totals);
    g->mesh_valid = 1;
    g->mesh_built = 1;
    g->mesh_serial += 1;
}

// ---- incremental remesh (row a7: VoxelObjectMesh::sync_with_voxel_object, mesh.rs:355-456) ---------------------------------------------
// (the host mirror of the ChunkSubmeshManager and its RangeAllocators, and the state of a sync in flight: ivx_submesh_manager, ivx_host.hpp)
void ivx_submesh_manager_free(ivx_submesh_manager* m) {
    if (!m) return;
    ivx_mapped_free(&m->pinned_up);
    if (m->up_done) (void)hipEventDestroy(m->up_done);
    delete m;
}

namespace {
void manager_remove(ivx_grid* g, ivx_submesh_manager* m, uint32_t chunk) {  // remove_chunk_if_present (mesh.rs:811-824)
    auto it = m->slot_of.find(chunk);
    if (it == m->slot_of.end()) return;
    const uint32_t slot = it->second;
    m->slot_of.erase(it);
    const ivx_submesh gone = m->table[slot];
    if (slot + 1 != m->table.size()) {
        m->table[slot] = m->table.back();
        m->slot_of[linear_chunk(g, m->table[slot].chunk_indices)] = slot;
    }
    m->table.pop_back();
    m->chunks_were_removed = true;
    m->vertices.free_range(gone.vertex_offset, (size_t)gone.vertex_offset + gone.vertex_count);
    m->indices.free_range(gone.index_offset, (size_t)gone.index_offset + gone.index_count);
}

bool sync_pending(const ivx_grid* g) { return g->submesh_manager && g->submesh_manager->sync_pending; }
// the sync's own host-mapped block, free (the event behind the last upload from it has passed) and at least `bytes`
int sync_block(ivx_submesh_manager* m, size_t bytes) {
    if (!m->up_done) IVX_HIP_CHECK(hipEventCreateWithFlags(&m->up_done, hipEventDisableTiming));
    if (m->up_busy) {
        IVX_HIP_CHECK(hipEventSynchronize(m->up_done));
        m->up_busy = 0;
    }
    return ivx_mapped_grow(&m->pinned_up, bytes, std::max<size_t>(bytes, 1 << 16), nullptr);
}
// host -> device from that block, asynchronously (the block is free again once the event behind the copy has passed)
int sync_upload(ivx_grid* g, const void* src, size_t bytes, void* d_dst) {
    if (ivx_many_upload(g->ctx, g, d_dst, src, (bytes + 3) & ~(size_t)3)) return IVX_OK;  // (a batch is being recorded: the words ride in its staging copy)
    ivx_submesh_manager* m = g->submesh_manager;
    int rc = sync_block(m, bytes);
    if (rc) return rc;
    memcpy(m->pinned_up.p, src, bytes);
    IVX_HIP_CHECK(ivx_memcpy_async(d_dst, m->pinned_up.p, bytes, hipMemcpyHostToDevice, g->ctx->stream));
    IVX_HIP_CHECK(ivx_event_record(m->up_done, g->ctx->stream));
    m->up_busy = 1;
    return IVX_OK;
}
// The sync's small lists where its kernels can read them WITHOUT a copy on the stream: into the block, *dev_view = the device's address of it.
// Null view: a batch is being recorded (the caller uploads as before). No event goes behind the readers: the block is next written by the
// object's next sync, which cannot be enqueued before this one's collect has waited for them — an event record there is a stream operation
// between the sync's launches and whatever follows them.
int sync_stage(ivx_grid* g, const void* src, size_t bytes, void** dev_view) {
    *dev_view = nullptr;
    if (ivx_many_recording()) return IVX_OK;
    ivx_submesh_manager* m = g->submesh_manager;
    int rc = sync_block(m, bytes);
    if (rc) return rc;
    memcpy(m->pinned_up.p, src, bytes);
    *dev_view = m->pinned_up.dev;
    return IVX_OK;
}

// VoxelObjectMesh::sync_with_voxel_object (mesh.rs:355-456) in two halves. ENQUEUE: the sizes the invalidated chunks' meshes need come from the
// last edit's result block when the set is that edit's (ivx_absorb_collect: no count pass, no read-back) — else from a count over just these
// chunks and one read-back —; the host mirror of the ChunkSubmeshManager places them; records and slots go up from pinned memory and the
// emit pass for the listed chunks follows on the stream. COLLECT: the wait. (Round 3 counted the whole object, read the sizes back, uploaded
// through a blocking copy and waited again: two round trips and ~25 us of counting for ~100 chunks.)
int mesh_sync_enqueue(ivx_grid* g, const uint8_t* invalidated_chunks, const char* who) {
    IVX_REQUIRE(g, IVX_ERR_INVALID, "%s: null argument", who);
    ivx_many_other_context other_(g->ctx);
    IVX_REQUIRE(!sync_pending(g), IVX_ERR_STATE, "%s: a sync of this object is in flight (ivx_mesh_sync_collect first)", who);
    IVX_REQUIRE(g->mesh_built, IVX_ERR_STATE, "ivx_mesh_sync: there is no mesh to synchronise (call ivx_remesh first)");
    IVX_REQUIRE(g->regions_valid, IVX_ERR_STATE, "ivx_mesh_sync: derived state must be current (the edit ops leave it so)");
    IVX_REQUIRE(g->x_off == 0 && g->gx == g->cc[0] && !g->has_ghost[0] && !g->has_ghost[1], IVX_ERR_STATE,
                "ivx_mesh_sync: not available on a slab of a decomposed grid");
    int rc;
    static thread_local double acc_[6];  // IVX_MANY_TRACE: host time per part of this function, summed over a period of calls
    static thread_local int calls_ = 0;
    ManyClock clk("sync enqueue");
    auto lap_ = [&](int slot) {
        if (many_trace()) acc_[slot] += clk.lap_us();
    };
    if (!g->submesh_manager) g->submesh_manager = new (std::nothrow) ivx_submesh_manager();
    IVX_REQUIRE(g->submesh_manager, IVX_ERR_HIP, "ivx_mesh_sync: out of host memory");
    ivx_submesh_manager* m = g->submesh_manager;
    if (m->serial != g->mesh_serial) {  // the mesh was rebuilt in full since: push_chunk for every submesh, no free ranges (mesh.rs:731-749)
        m->table.assign(g->mesh_counts.n_submeshes, ivx_submesh{});
        if ((rc = d2h(g, m->table.data(), g->submeshes, m->table.size() * sizeof(ivx_submesh)))) return rc;
        m->slot_of.clear();
        for (uint32_t s = 0; s < m->table.size(); ++s) m->slot_of[linear_chunk(g, m->table[s].chunk_indices)] = s;
        m->vertices.free_ranges.clear();
        m->indices.free_ranges.clear();
        m->total_vertices = g->mesh_counts.n_vertices;
        m->total_indices = g->mesh_counts.n_indices;
        m->updated.clear();  // (recreate -> ChunkSubmeshManager::clear, mesh.rs:843-851)
        m->chunks_were_removed = false;
        m->serial = g->mesh_serial;
    }
    lap_(0);
    // what the invalidated chunks' meshes need now and their records (exposure, obscuredness flags)
    // (the call's work lists live on across calls: with a hundred objects per frame their allocations were a third of the host's time here)
    static thread_local std::vector<uint32_t> list, needs, dirty_slots, rec_chunk, slots;
    static thread_local std::vector<char> stage;
    list.clear();
    if (!invalidated_chunks) {  // the set of the edit in flight
        if ((rc = edit_early_needs(g, who, list))) return rc;
    } else {   // chunk-linear order (the reference walks a hash set: unpinned); eight flags a look — nearly all of them are zero
        uint32_t c = 0;
        for (; c + 8u <= g->n_chunks; c += 8u) {
            uint64_t w;
            memcpy(&w, invalidated_chunks + c, 8);
            if (!w) continue;
            for (uint32_t b = 0; b < 8u; ++b)
                if (invalidated_chunks[c + b]) list.push_back(c + b);
        }
        for (; c < g->n_chunks; ++c)
            if (invalidated_chunks[c]) list.push_back(c);
    }
    needs.assign(3 * list.size(), 0u);
    bool cached = g->needs_current != 0;
    for (size_t e = 0; e < list.size() && cached; ++e) cached = edit_needs_lookup(g, list[e], &needs[3 * e]);
    if (!list.empty() && !cached) {
        const size_t off_out = (list.size() * 4 + 15) & ~(size_t)15;
        if ((rc = ensure_dev_scratch(g, off_out + list.size() * 16))) return rc;
        char* base = static_cast<char*>(g->dev_scratch);
        if ((rc = sync_upload(g, list.data(), list.size() * 4, base))) return rc;
        if ((rc = ivx_launch_list_mesh_needs(g, (uint32_t)list.size(), reinterpret_cast<const uint32_t*>(base), reinterpret_cast<uint32_t*>(base + off_out)))) return rc;
        std::vector<uint32_t> raw(4 * list.size());
        if ((rc = d2h(g, raw.data(), base + off_out, raw.size() * 4))) return rc;
        for (size_t e = 0; e < list.size(); ++e) needs[3 * e] = raw[4 * e + 1], needs[3 * e + 1] = raw[4 * e + 2], needs[3 * e + 2] = raw[4 * e] & 0xFFFFu;
    }
    lap_(1);
    dirty_slots.clear();  // slots of the device table that a removal rewrote (the emit pass writes the others)
    struct Rec {
        uint32_t chunk, voff, ioff, packed;
    };
    static thread_local std::vector<Rec> recs;
    recs.clear();
    rec_chunk.clear();
    for (size_t e = 0; e < list.size(); ++e) {
        const uint32_t c = list[e];
        const uint32_t nv = needs[3 * e], ni = needs[3 * e + 1], kind = needs[3 * e + 2] & 0xFFu, flags = (needs[3 * e + 2] >> 8) & 0xFFu;
        const bool exposed = kind == KIND_NONUNIFORM && (flags & CF_FULLY_OBSCURED) != CF_FULLY_OBSCURED;
        if (!exposed || ni == 0) {  // no longer exposed, or an empty mesh (mesh.rs:375-379, 447-451)
            auto gone = m->slot_of.find(c);
            if (gone != m->slot_of.end()) dirty_slots.push_back(gone->second);  // (the last entry moves here)
            manager_remove(g, m, c);
            continue;
        }
        // write_chunk (mesh.rs:751-809)
        auto it = m->slot_of.find(c);
        if (it != m->slot_of.end()) {
            const ivx_submesh& old = m->table[it->second];
            m->vertices.free_range(old.vertex_offset, (size_t)old.vertex_offset + old.vertex_count);
            m->indices.free_range(old.index_offset, (size_t)old.index_offset + old.index_count);
        }
        size_t v0, i0;
        if (!m->vertices.allocate(nv, &v0)) v0 = m->total_vertices, m->total_vertices += nv;
        if (!m->indices.allocate(ni, &i0)) i0 = m->total_indices, m->total_indices += ni;
        IVX_REQUIRE(m->total_vertices < 0xFFFFFFFFull && m->total_indices < 0xFFFFFFFFull, IVX_ERR_CAPACITY, "ivx_mesh_sync: mesh buffers exceed 2^32 elements");
        ivx_submesh sm;
        memset(&sm, 0, sizeof(sm));
        sm.chunk_indices[0] = c / (g->cc[1] * g->cc[2]);
        sm.chunk_indices[1] = (c / g->cc[2]) % g->cc[1];
        sm.chunk_indices[2] = c % g->cc[2];
        sm.index_offset = (uint32_t)i0;
        sm.index_count = ni;
        sm.vertex_offset = (uint32_t)v0;
        sm.vertex_count = nv;
        for (int a = 0; a < 2; ++a)  // ChunkSubmesh::new (mesh.rs:611-635): bits X_DN 0, Y_DN 1, Z_DN 2, X_UP 3, Y_UP 4, Z_UP 5
            for (int b = 0; b < 2; ++b)
                for (int d = 0; d < 2; ++d)
                    sm.is_obscured_from_direction[a][b][d] =
                        (((flags >> (3 * a)) & 1u) && ((flags >> (3 * b + 1)) & 1u) && ((flags >> (3 * d + 2)) & 1u)) ? 1u : 0u;
        if (it != m->slot_of.end()) {
            m->table[it->second] = sm;
        } else {
            m->slot_of[c] = (uint32_t)m->table.size();
            m->table.push_back(sm);
        }
        m->updated.push_back(ivx_submesh_data_ranges{(uint32_t)v0, (uint32_t)(v0 + nv), (uint32_t)i0, (uint32_t)(i0 + ni)});
        recs.push_back(Rec{c, (uint32_t)v0, (uint32_t)i0, nv | ((ni / 6u) << 16)});
        rec_chunk.push_back(c);
    }
    lap_(2);
    m->vertices.merge_consecutive();  // perform_maintainance
    m->indices.merge_consecutive();
    if ((rc = ensure_mesh_capacity_keep(g, m->total_vertices, m->total_indices, m->table.size()))) return rc;
    lap_(3);
    // the device table: the emit pass writes the re-meshed chunks' entries; entries a removal moved are patched from the host mirror — by the
    // emit pass's first workgroup when there is one (they ride in its upload), else by a small copy each
    size_t n_patch = 0;
    for (uint32_t slot : dirty_slots) n_patch += slot < m->table.size() ? 1u : 0u;
    if (!recs.empty()) {
        // (slots are final only now: a removal after a write may have moved the written entry)
        slots.resize(recs.size());
        for (size_t r = 0; r < recs.size(); ++r) slots[r] = m->slot_of.at(rec_chunk[r]);
        const size_t off_slots = 16 + recs.size() * sizeof(Rec), off_pslots = off_slots + recs.size() * 4;
        const size_t off_pent = (off_pslots + n_patch * 4 + 15) & ~(size_t)15, total = off_pent + n_patch * sizeof(ivx_submesh);
        if ((rc = ensure_dev_scratch(g, total))) return rc;
        stage.assign(total, 0);
        const uint32_t n = (uint32_t)recs.size();
        memcpy(stage.data(), &n, 4);
        memcpy(stage.data() + 16, recs.data(), recs.size() * sizeof(Rec));
        memcpy(stage.data() + off_slots, slots.data(), slots.size() * 4);
        size_t e = 0;
        for (uint32_t slot : dirty_slots)
            if (slot < m->table.size()) {
                memcpy(stage.data() + off_pslots + 4 * e, &slot, 4);
                memcpy(stage.data() + off_pent + e * sizeof(ivx_submesh), &m->table[slot], sizeof(ivx_submesh));
                e += 1;
            }
        // (records, slots and patches are a few KB the passes only read: from host-mapped memory in place — a copy ahead of the passes is a
        // stream operation of 4 us and a gap; a recorded batch carries them in its one staging copy instead)
        char* base = static_cast<char*>(g->dev_scratch);
        void* view = nullptr;
        if ((rc = sync_stage(g, stage.data(), total, &view))) return rc;
        if (view) base = static_cast<char*>(view);
        else if ((rc = sync_upload(g, stage.data(), total, base))) return rc;
        if ((rc = ivx_launch_sn_emit_list(g, n, reinterpret_cast<const uint32_t*>(base), base + 16, reinterpret_cast<const uint32_t*>(base + off_slots), (uint32_t)n_patch,
                                          base + off_pent, reinterpret_cast<const uint32_t*>(base + off_pslots))))
            return rc;
    }
    lap_(4);
    if (recs.empty())
        for (uint32_t slot : dirty_slots)
            if (slot < m->table.size() && !ivx_many_upload(g->ctx, g, g->submeshes + slot, &m->table[slot], sizeof(ivx_submesh)))
                IVX_HIP_CHECK(ivx_memcpy_async(g->submeshes + slot, &m->table[slot], sizeof(ivx_submesh), hipMemcpyHostToDevice, g->ctx->stream));
    g->mesh_counts.n_vertices = (uint32_t)m->total_vertices;
    g->mesh_counts.n_indices = (uint32_t)m->total_indices;
    g->mesh_counts.n_submeshes = (uint32_t)m->table.size();
    g->mesh_serial += 1;  // collision probes picked from the old mesh are stale
    m->serial = g->mesh_serial;
    m->sync_pending = 1;
    m->sync_drained = 0;
    lap_(5);
    static const int period_ = many_trace() && atoi(getenv("IVX_MANY_TRACE")) > 1 ? atoi(getenv("IVX_MANY_TRACE")) : 81;
    if (many_trace() && ++calls_ % period_ == 0) {
        fprintf(stderr, "[ivx many]   sync enqueue laps (us per period): setup %.1f list+needs %.1f allocator %.1f capacity %.1f upload+emit %.1f tail %.1f\n", acc_[0], acc_[1], acc_[2],
                acc_[3], acc_[4], acc_[5]);
        for (double& a : acc_) a = 0.0;
    }
    return IVX_OK;
}

int mesh_sync_collect(ivx_grid* g, ivx_mesh_counts* out, const char* who, bool stream_is_drained = false) {
    IVX_REQUIRE(g && out, IVX_ERR_INVALID, "%s: null argument", who);
    IVX_REQUIRE(sync_pending(g), IVX_ERR_STATE, "%s: no sync of this object is in flight", who);
    ivx_submesh_manager* m = g->submesh_manager;
    m->sync_pending = 0;
    if (m->sync_drained) stream_is_drained = true;  // (the edit's collect waited behind this sync's launches)
    m->sync_drained = 0;
    if (!stream_is_drained) IVX_HIP_CHECK(ivx_stream_sync(g->ctx->stream));
    g->mesh_valid = 1;
    *out = g->mesh_counts;
    return IVX_OK;
}
}  // namespace

void mesh_sync_stream_drained(ivx_grid* g) {
    if (sync_pending(g)) g->submesh_manager->sync_drained = 1;
}
void mesh_sync_abandon(ivx_grid* g) {
    ivx_mesh_counts mc;
    if (sync_pending(g)) (void)mesh_sync_collect(g, &mc, "ivx_*_many (drain)", true);
}

extern "C" {

int ivx_remesh(ivx_grid* g, ivx_mesh_counts* out) {
    IVX_REQUIRE(g && out, IVX_ERR_INVALID, "ivx_remesh: null argument");
    int rc;
    if ((rc = ivx_launch_sn_count(g))) return rc;
    if ((rc = ivx_launch_sn_scan(g))) return rc;
    uint32_t totals[3];
    if ((rc = d2h(g, totals, g->chunk_offsets + 2 * (size_t)g->n_chunks, sizeof(totals)))) return rc;
    if ((rc = ensure_mesh_capacity(g, totals[0], totals[1], totals[2]))) return rc;
    if (totals[1] > 0 && (rc = ivx_launch_sn_emit(g))) return rc;
    mesh_adopt_full(g, totals);
    *out = g->mesh_counts;
    IVX_HIP_CHECK(ivx_stream_sync(g->ctx->stream));
    return IVX_OK;
}

int ivx_mesh_sync_enqueue(ivx_grid* g, const uint8_t* invalidated_chunks) { return mesh_sync_enqueue(g, invalidated_chunks, "ivx_mesh_sync_enqueue"); }
int ivx_grid_set_early_mesh_needs(ivx_grid* g, int on) {
    IVX_REQUIRE(g, IVX_ERR_INVALID, "ivx_grid_set_early_mesh_needs: null grid");
    g->early_needs_on = on ? 1 : 0;
    return IVX_OK;
}
int ivx_mesh_sync_collect(ivx_grid* g, ivx_mesh_counts* out) { return mesh_sync_collect(g, out, "ivx_mesh_sync_collect"); }
int ivx_mesh_sync(ivx_grid* g, const uint8_t* invalidated_chunks, ivx_mesh_counts* out) {
    IVX_REQUIRE(out, IVX_ERR_INVALID, "ivx_mesh_sync: null argument");
    const int rc = mesh_sync_enqueue(g, invalidated_chunks, "ivx_mesh_sync");
    return rc ? rc : mesh_sync_collect(g, out, "ivx_mesh_sync");
}

int ivx_mesh_sync_many(ivx_grid* const* grids, size_t n, const uint8_t* const* invalidated_chunks, ivx_mesh_counts* out) {
    if (n == 0) return IVX_OK;  // (a manager without voxel objects)
    int rc = many_check(grids, n, "ivx_mesh_sync_many");
    if (rc) return rc;
    IVX_REQUIRE(invalidated_chunks && out, IVX_ERR_INVALID, "ivx_mesh_sync_many: null argument");
    ManyClock clk("sync");
    if ((rc = many_phase(grids, n, [&](size_t i) { return mesh_sync_enqueue(grids[i], invalidated_chunks[i], "ivx_mesh_sync_many"); }))) return many_fail(grids, n, rc);
    clk.lap("enqueue + flush");
    IVX_HIP_CHECK(ivx_stream_sync(grids[0]->ctx->stream));  // (one wait for all)
    clk.lap("wait");
    for (size_t i = 0; i < n; ++i)
        if ((rc = mesh_sync_collect(grids[i], &out[i], "ivx_mesh_sync_many", true))) return many_fail(grids, n, rc);
    return IVX_OK;
}

int ivx_mesh_modifications(ivx_grid* g, ivx_submesh_data_ranges* out, size_t cap, size_t* n_out, int* chunks_were_removed) {
    IVX_REQUIRE(g && n_out && chunks_were_removed && (out || cap == 0), IVX_ERR_INVALID, "ivx_mesh_modifications: null argument");
    const ivx_submesh_manager* m = g->submesh_manager;
    const bool current = m && m->serial == g->mesh_serial;  // (a full remesh since the last sync: nothing pending, the whole mesh is new)
    *n_out = current ? m->updated.size() : 0;
    *chunks_were_removed = current && m->chunks_were_removed ? 1 : 0;
    IVX_REQUIRE(*n_out <= cap || !out, IVX_ERR_CAPACITY, "ivx_mesh_modifications: %zu ranges exceed the capacity %zu", *n_out, cap);
    if (out && *n_out) memcpy(out, m->updated.data(), *n_out * sizeof(ivx_submesh_data_ranges));
    return IVX_OK;
}

int ivx_mesh_report_synchronized(ivx_grid* g) {
    IVX_REQUIRE(g, IVX_ERR_INVALID, "ivx_mesh_report_synchronized: null grid");
    if (g->submesh_manager) {
        g->submesh_manager->updated.clear();
        g->submesh_manager->chunks_were_removed = false;
    }
    return IVX_OK;
}

int ivx_mesh_download(ivx_grid* g, float* positions, float* normals, uint32_t* indices, uint8_t* index_materials, ivx_submesh* submeshes) {
    IVX_REQUIRE(g, IVX_ERR_INVALID, "ivx_mesh_download: null grid");
    IVX_REQUIRE(g->mesh_valid, IVX_ERR_STATE, "ivx_mesh_download: call ivx_remesh first");
    const size_t counts[3] = {g->mesh_counts.n_vertices, g->mesh_counts.n_indices, g->mesh_counts.n_submeshes};
    void* const dst[N_HANDED_OUT] = {positions, normals, indices, index_materials, submeshes};
    for (int which = 0; which < N_HANDED_OUT; ++which) {
        const MeshArray a = handed_out(g, which);
        if (!dst[which]) continue;
        if (int rc = d2h(g, dst[which], *a.slot, counts[a.bound] * a.elem)) return rc;
    }
    return IVX_OK;
}

void* ivx_mesh_device_ptr(ivx_grid* g, int which) {
    if (!g || !g->mesh_valid || which < 0 || which >= N_HANDED_OUT) return nullptr;
    return *handed_out(g, which).slot;
}

// §8f-4: handles of a mesh buffer another process or another API can import (gpu_resource.rs:498-530, 729-907 fill wgpu buffers from these
// arrays; mesh.rs:94-123). The buffers are plain hipMalloc allocations of their own, so the IPC handle names exactly the buffer.
int ivx_mesh_export(ivx_grid* g, int which, ivx_mesh_export_info* out) {
    IVX_REQUIRE(g && out && which >= 0 && which < N_HANDED_OUT, IVX_ERR_INVALID, "ivx_mesh_export: bad argument");
    IVX_REQUIRE(g->mesh_valid || g->mesh_built, IVX_ERR_STATE, "ivx_mesh_export: the grid has no mesh");
    memset(out, 0, sizeof(*out));
    out->dmabuf_fd = -1;
    const MeshArray a = handed_out(g, which);
    const size_t counts[3] = {g->mesh_counts.n_vertices, g->mesh_counts.n_indices, g->mesh_counts.n_submeshes};
    void* p = *a.slot;
    const size_t elem = a.elem, cap = *capacities(g, a.bound);
    // after an incremental sync the live ranges are scattered over the buffers: everything up to the capacity may be in use
    const size_t count = g->submesh_manager ? cap : counts[a.bound];
    IVX_REQUIRE(p && cap, IVX_ERR_STATE, "ivx_mesh_export: the buffer is empty");
    out->bytes = (uint64_t)count * elem;
    out->capacity_bytes = (uint64_t)cap * elem;
    out->element_bytes = (uint32_t)elem;
    out->generation = g->mesh_generation;
    out->device_ptr = (uint64_t)(uintptr_t)p;
    hipIpcMemHandle_t h;
    static_assert(sizeof(h) == sizeof(out->ipc_handle), "hipIpcMemHandle_t is 64 bytes");
    IVX_HIP_CHECK(hipIpcGetMemHandle(&h, p));
    memcpy(out->ipc_handle, &h, sizeof(h));
    // a dma-buf file descriptor for APIs that import those (Vulkan VK_EXT_external_memory_dma_buf under wgpu): optional, -1 where the
    // runtime cannot make one; the caller owns the descriptor (close it)
    int fd = -1;
    const size_t page = 4096;
    // The HSA runtime's export names the offset of the range inside the dma-buf object (the HIP call drops it): taken from there when the
    // symbol is in the process (it is wherever libamdhip64 is: libhsa-runtime64 is its dependency), page-aligned range around the buffer.
    typedef int (*export_fn)(const void*, size_t, int*, uint64_t*);
    static export_fn hsa_export = reinterpret_cast<export_fn>(dlsym(RTLD_DEFAULT, "hsa_amd_portable_export_dmabuf"));
    const uintptr_t lo = (uintptr_t)p & ~(uintptr_t)(page - 1), hi = ((uintptr_t)p + (size_t)out->capacity_bytes + page - 1) & ~(uintptr_t)(page - 1);
    uint64_t off = 0;
    if (hsa_export && hsa_export(reinterpret_cast<const void*>(lo), hi - lo, &fd, &off) == 0 && fd >= 0) {
        out->dmabuf_fd = fd;
        out->dmabuf_offset = off + ((uintptr_t)p - lo);
        out->dmabuf_bytes = hi - lo;
    } else if (hipMemGetHandleForAddressRange(&fd, reinterpret_cast<void*>(lo), hi - lo, hipMemRangeHandleTypeDmaBufFd, 0) == hipSuccess && fd >= 0) {
        out->dmabuf_fd = fd;
        out->dmabuf_offset = (uintptr_t)p - lo;  // (the range's own start: this call does not say where the range lies in the object)
        out->dmabuf_bytes = hi - lo;
    } else {
        const hipError_t e = hipGetLastError();
        ivx_set_error("ivx_mesh_export: no dma-buf descriptor for the buffer (%s); the hipIpc handle is valid", hipGetErrorString(e));
    }
    return IVX_OK;
}

// the importing side for a HIP process: the 64-byte handle of ivx_mesh_export -> a device pointer in THIS process (no context needed beyond
// the device being usable); ivx_mesh_import_close gives it back
int ivx_mesh_import_open(const uint8_t ipc_handle[64], int device, void** device_ptr) {
    IVX_REQUIRE(ipc_handle && device_ptr, IVX_ERR_INVALID, "ivx_mesh_import_open: null argument");
    IVX_HIP_CHECK(hipSetDevice(device));
    hipIpcMemHandle_t h;
    memcpy(&h, ipc_handle, sizeof(h));
    IVX_HIP_CHECK(hipIpcOpenMemHandle(device_ptr, h, hipIpcMemLazyEnablePeerAccess));
    return IVX_OK;
}
int ivx_mesh_import_close(void* device_ptr) {
    IVX_REQUIRE(device_ptr, IVX_ERR_INVALID, "ivx_mesh_import_close: null argument");
    IVX_HIP_CHECK(hipIpcCloseMemHandle(device_ptr));
    return IVX_OK;
}

int ivx_mesh_generation(ivx_grid* g, uint64_t* generation) {
    IVX_REQUIRE(g && generation, IVX_ERR_INVALID, "ivx_mesh_generation: null argument");
    *generation = g->mesh_generation;
    return IVX_OK;
}

}  // extern "C"
