// C ABI entry points of libimpact_voxel_hip.so (include/impact_voxel_hip.h has the contract and the reference interfaces each function
// replaces) that no unit of their own holds yet: contexts and the life cycle of grids, staged copies, upload and download, single-call sampling
// and deriving, inertia, regions, the resident SDF program and tables, halos, the recorder phases of the many-object calls. (The step, edits,
// meshes, split and clip, voxel collision: step_api, edit_api, mesh_api, extraction_api, voxel_collision_api.hip.) Host-side orchestration only.
#include <algorithm>
#include <functional>
#include <cmath>
#include <chrono>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "ivx_host.hpp"

static thread_local char g_error[512] = "";

void ivx_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

namespace {

int ensure_host_scratch(ivx_grid* g, size_t bytes) {
    if (g->host_scratch_bytes >= bytes) return IVX_OK;
    IVX_HIP_CHECK(ivx_stream_sync(g->ctx->stream));
    if (g->host_scratch) (void)hipHostFree(g->host_scratch);
    g->host_scratch = nullptr;
    g->host_scratch_bytes = 0;
    if (bytes < (64u << 10)) bytes = 64u << 10;
    IVX_HIP_CHECK(hipHostMalloc(&g->host_scratch, bytes, hipHostMallocDefault));
    g->host_scratch_bytes = bytes;
    return IVX_OK;
}

}  // namespace
// Host<->device copies. Small ones (the scalars and tables the entry points hand back: up to a few hundred KB, STAGED_COPY_MAX) go through
// the grid's pinned staging buffer as ONE stream-ordered copy and ONE wait (a blocking copy from pageable memory costs a wait for
// the stream, a staging copy inside the runtime and a second wait); large ones (whole planes) stay plain blocking copies.
int d2h(ivx_grid* g, void* dst, const void* src, size_t bytes) {
    if (bytes == 0) return IVX_OK;
    if (bytes <= STAGED_COPY_MAX) {
        int rc = ensure_host_scratch(g, bytes);
        if (rc) return rc;
        IVX_HIP_CHECK(ivx_memcpy_async(g->host_scratch, src, bytes, hipMemcpyDeviceToHost, g->ctx->stream));
        IVX_HIP_CHECK(ivx_stream_sync(g->ctx->stream));
        memcpy(dst, g->host_scratch, bytes);
        return IVX_OK;
    }
    IVX_HIP_CHECK(ivx_stream_sync(g->ctx->stream));
    IVX_HIP_CHECK(ivx_memcpy_sync(dst, src, bytes, hipMemcpyDeviceToHost));
    return IVX_OK;
}
int h2d(ivx_grid* g, void* dst, const void* src, size_t bytes) {
    if (bytes == 0) return IVX_OK;
    if (bytes <= STAGED_COPY_MAX) {
        int rc = ensure_host_scratch(g, bytes);
        if (rc) return rc;
        IVX_HIP_CHECK(ivx_stream_sync(g->ctx->stream));  // the staging buffer may still feed an earlier copy
        memcpy(g->host_scratch, src, bytes);
        IVX_HIP_CHECK(ivx_memcpy_async(dst, g->host_scratch, bytes, hipMemcpyHostToDevice, g->ctx->stream));
        IVX_HIP_CHECK(ivx_stream_sync(g->ctx->stream));
        return IVX_OK;
    }
    IVX_HIP_CHECK(ivx_stream_sync(g->ctx->stream));
    IVX_HIP_CHECK(ivx_memcpy_sync(dst, src, bytes, hipMemcpyHostToDevice));
    return IVX_OK;
}
int ensure_dev_scratch(ivx_grid* g, size_t bytes) {
    if (g->dev_scratch_bytes >= bytes) return IVX_OK;
    IVX_HIP_CHECK(ivx_stream_sync(g->ctx->stream));
    if (g->dev_scratch) (void)hipFree(g->dev_scratch);
    g->dev_scratch = nullptr;
    const size_t had = g->dev_scratch_bytes;
    g->dev_scratch_bytes = 0;
    bytes = std::max<size_t>(std::max<size_t>(bytes, 2 * had), 64u << 10);  // (a growth is a wait on the stream: rare by construction)
    IVX_HIP_CHECK(hipMalloc(&g->dev_scratch, bytes));
    g->dev_scratch_bytes = bytes;
    return IVX_OK;
}

// Shared allocations (ivx_block, ivx_internal.hpp): released by the last grid that holds a part.
void block_release(ivx_block* b) {
    if (!b || --b->refs > 0) return;
    if (b->dev) (void)hipFree(b->dev);
    if (b->pinned) (void)hipHostFree(b->pinned);
    delete b;
}

namespace {
__global__ __launch_bounds__(256) void k_halo_pack(GridView g, uint32_t side, int8_t* __restrict__ out_sdf, uint8_t* __restrict__ out_type,
                                                   ivx_chunk_info* __restrict__ out_info) {
    const uint32_t col = blockIdx.x;  // cj*cz + ck
    const uint32_t tid = threadIdx.x;
    const uint32_t ci = side ? g.cx - 1 : 0u;
    const uint32_t chunk = ci * g.cy * g.cz + col;
    const size_t src = (size_t)chunk * IVX_CHUNK_VOXELS + ((side ? 15u : 0u) << 8) + tid;
    const ivx_chunk_info rec = g.info[chunk];
    const bool dense = rec.kind == KIND_NONUNIFORM;  // else the chunk is its record (compact planes)
    out_sdf[(size_t)col * 256 + tid] = dense ? g.sdf[src] : (int8_t)ivx_uniform_sdf(rec.kind);
    out_type[(size_t)col * 256 + tid] = dense ? g.type[src] : (uint8_t)ivx_uniform_type(rec);
    if (tid == 0) out_info[col] = rec;
}

}  // namespace

int ivx_launch_halo_pack(ivx_grid* g, int side, void* buf) {
    const size_t cols = (size_t)g->cc[1] * g->cc[2];
    int8_t* o_sdf = static_cast<int8_t*>(buf);
    uint8_t* o_type = static_cast<uint8_t*>(buf) + cols * 256;
    ivx_chunk_info* o_info = reinterpret_cast<ivx_chunk_info*>(static_cast<uint8_t*>(buf) + cols * 512);
    GridView v = ivx_view(g);
    IVX_KLAUNCH(k_halo_pack, dim3((uint32_t)cols), dim3(256), 0, g->ctx->stream, v, (uint32_t)side, o_sdf, o_type, o_info);
    IVX_HIP_CHECK(hipGetLastError());
    return IVX_OK;
}

// the occupied ranges in the reference's sense (see ivx_grid::occ_ref): cached, recomputed only when something invalidated them
int reference_occupied(ivx_grid* g, uint32_t occ[12]) {
    if (!g->occ_ref_valid) {
        uint32_t* d_occ = g->rscalar + 16;
        int rc;
        if ((rc = ivx_launch_occupied(g, d_occ))) return rc;
        uint32_t raw[12];
        if ((rc = d2h(g, raw, d_occ, sizeof(raw)))) return rc;
        ivx_occupied_from_raw(g, raw, g->occ_ref);
        g->occ_ref_valid = 1;
    }
    memcpy(occ, g->occ_ref, sizeof(g->occ_ref));
    return IVX_OK;
}

int ivx_reference_occupied(ivx_grid* g, const char* who, uint32_t occ[12]) {
    IVX_REQUIRE(g->occ_ref_valid || g->bbox_valid, IVX_ERR_STATE, "%s: the object holds no occupied ranges yet (call ivx_derive_state or a step first)", who);
    return reference_occupied(g, occ);
}

extern "C" {

const char* ivx_last_error(void) { return g_error; }

int ivx_init(int device_id, void* stream, ivx_ctx** out) {
    IVX_REQUIRE(out, IVX_ERR_INVALID, "ivx_init: null output pointer");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0) {
        ivx_set_error("ivx_init: no HIP device available (%s); this library has no CPU fallback", e == hipSuccess ? "0 devices" : hipGetErrorString(e));
        return IVX_ERR_HIP;
    }
    IVX_REQUIRE(device_id >= 0 && device_id < count, IVX_ERR_INVALID, "ivx_init: device %d out of range (0..%d)", device_id, count - 1);
    IVX_HIP_CHECK(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    IVX_HIP_CHECK(hipGetDeviceProperties(&prop, device_id));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        ivx_set_error("ivx_init: device %d is %s; this library is built for gfx950 (MI355X) only", device_id, prop.gcnArchName);
        return IVX_ERR_HIP;
    }
    ivx_ctx* c = new (std::nothrow) ivx_ctx();
    IVX_REQUIRE(c, IVX_ERR_CAPACITY, "ivx_init: out of host memory");
    c->device = device_id;
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    {
        // the rate of the clock the kernels' stage stamps read (ivx_stage_stamp); 100 MHz on this part, assumed — and said — when the query fails
        int khz = 0;
        const hipError_t ce = hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device_id);
        if (ce != hipSuccess || khz <= 0) {
            ivx_set_error("ivx_init: the wall clock rate of device %d could not be queried (%s); stage times from clock stamps assume 100 MHz", device_id,
                          ce == hipSuccess ? "0 kHz reported" : hipGetErrorString(ce));
            khz = 100000;
        }
        c->wall_clock_khz = (double)khz;
    }
    if (stream) {
        c->stream = static_cast<hipStream_t>(stream);
        c->own_stream = false;
    } else {
        hipError_t se = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (se != hipSuccess) {
            ivx_set_error("ivx_init: hipStreamCreate failed: %s", hipGetErrorString(se));
            delete c;
            return IVX_ERR_HIP;
        }
        c->own_stream = true;
    }
    *out = c;
    return IVX_OK;
}

void ivx_shutdown(ivx_ctx* c) {
    if (!c) return;
    (void)ivx_stream_sync(c->stream);
    ivx_many_release(c);  // (the launch recorder of the many-object calls and its staging ring)
    ivx_mapped_free(&c->pinned_scratch);
    ivx_buf_free(&c->dev_scratch);
    ivx_buf_free(&c->drag_scratch);
    ivx_cull_release(c);
    ivx_bvol_release(c);
    ivx_fi_release(c);
    if (c->aux_stream) {
        (void)hipStreamSynchronize(c->aux_stream);
        (void)hipStreamDestroy(c->aux_stream);
    }
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int ivx_synchronize(ivx_ctx* c) {
    IVX_REQUIRE(c, IVX_ERR_INVALID, "ivx_synchronize: null context");
    IVX_HIP_CHECK(ivx_stream_sync(c->stream));
    return IVX_OK;
}

void* ivx_stream(ivx_ctx* c) { return c ? static_cast<void*>(c->stream) : nullptr; }

// ONE device allocation for everything of a grid whose size follows from the chunk counts, carved at 256-byte boundaries: a grid used to
// cost ~45 hipMalloc calls, which was most of the price of creating the small grids that split-off and polyhedron clips make (one per
// fragment). `arena` null: sizes only. Returns the arena's bytes.
static size_t grid_carve(ivx_grid* g, char* arena) {
    size_t arena_bytes = 0;
    const size_t cols = (size_t)g->cc[1] * g->cc[2];
    auto carve = [&](auto** p, size_t count) {
        using T = std::remove_pointer_t<std::remove_pointer_t<decltype(p)>>;
        const size_t bytes = (count * sizeof(T) + 255) & ~(size_t)255;
        if (arena) *p = reinterpret_cast<T*>(arena + arena_bytes);
        arena_bytes += bytes;
    };
    carve(&g->sdf, g->n_vox);
    carve(&g->type, g->n_vox);
    carve(&g->flags, g->n_vox);
    carve(&g->llabel, g->n_vox);
    carve(&g->info, (size_t)g->n_chunks);
    carve(&g->chunk_bbox, (size_t)g->n_chunks);
    for (int sd = 0; sd < 2; ++sd) {
        carve(&g->ghost_sdf[sd], cols * 256);
        carve(&g->ghost_type[sd], cols * 256);
        carve(&g->ghost_info[sd], cols);
    }
    carve(&g->chunk_counts, (size_t)g->n_chunks * 2);
    carve(&g->chunk_offsets, (size_t)g->n_chunks * 3 + 8);
    carve(&g->partials, g->partial_blocks * 10 + 16);
    carve(&g->rparent, (size_t)g->n_chunks * 256);
    carve(&g->rcompid, (size_t)g->n_chunks * 256);
    carve(&g->rscalar, (size_t)64);
    carve(&g->ccl_scratch, (size_t)g->n_chunks * 2);
    carve(&g->sn_list, (size_t)g->n_chunks * 4);  // one uint4 record per meshed chunk
    carve(&g->group_sums, (size_t)((g->n_chunks + 255u) / 256u) * (1u + IVX_SN_GROUP_WORDS) + IVX_SN_TAIL_WORDS);
    carve(&g->sn_hard, (size_t)g->n_chunks);
    carve(&g->sn_walk, (size_t)g->n_chunks * 5 + 2);  // the main pass's walk order: a uint4 record and a list index per meshed chunk, the two class counts (role_sn_scan)
    carve(&g->dens_dev, (size_t)256);
    carve(&g->work_counts, (size_t)8);
    carve(&g->occ_part, (size_t)((g->n_chunks + 255u) / 256u) * 12 + 12);
    carve(&g->active_list, (size_t)g->n_chunks);
    carve(&g->chunk_class, (size_t)g->n_chunks);
    carve(&g->chunk_touch, (size_t)g->n_chunks);
    carve(&g->chunk_signs, (size_t)g->n_chunks * 256);
    carve(&g->kface, (size_t)g->n_chunks * 1024);
    carve(&g->chunk_moments, (size_t)g->n_chunks * 10);
    return arena_bytes;
}
// the host side of a new grid (no device memory yet)
static int grid_new(ivx_ctx* c, const uint32_t cc[3], float voxel_extent, uint32_t x_chunk_offset, uint32_t global_x_chunks, ivx_grid** out) {
    IVX_REQUIRE(c && cc && out, IVX_ERR_INVALID, "ivx_grid_create: null argument");
    *out = nullptr;
    IVX_REQUIRE(cc[0] > 0 && cc[1] > 0 && cc[2] > 0, IVX_ERR_INVALID, "ivx_grid_create: empty chunk grid");
    IVX_REQUIRE(voxel_extent > 0.0f, IVX_ERR_INVALID, "ivx_grid_create: voxel extent must be positive");
    const uint64_t n64 = (uint64_t)cc[0] * cc[1] * cc[2];
    // GlobalRegionLabel packs the chunk index in 24 bits (split_detection.rs:1539-1571)
    IVX_REQUIRE(n64 <= (1u << 24), IVX_ERR_CAPACITY, "ivx_grid_create: more than 2^24 chunks");
    ivx_grid* g = new (std::nothrow) ivx_grid();
    IVX_REQUIRE(g, IVX_ERR_CAPACITY, "ivx_grid_create: out of host memory");
    memset(g, 0, sizeof(*g));
    g->scratch_dirty = IVX_SCRATCH_REGIONS;  // (the pool is not cleared: the region scalars' first user outside a step must zero them, ivx_launch_derive)
    g->ctx = c;
    for (int d = 0; d < 3; ++d) g->cc[d] = cc[d];
    g->n_chunks = (uint32_t)n64;
    g->n_vox = (size_t)n64 * IVX_CHUNK_VOXELS;
    g->extent = voxel_extent;
    g->x_off = x_chunk_offset;
    g->gx = global_x_chunks ? global_x_chunks : cc[0];
    g->partial_blocks = 2048;
    *out = g;
    return IVX_OK;
}

int ivx_grid_create(ivx_ctx* c, const uint32_t cc[3], float voxel_extent, uint32_t x_chunk_offset, uint32_t global_x_chunks, ivx_grid** out) {
    ivx_grid* g = nullptr;
    int rc = grid_new(c, cc, voxel_extent, x_chunk_offset, global_x_chunks, &g);
    if (rc) return rc;
    IVX_HIP_CHECK(hipSetDevice(c->device));
    const size_t arena_bytes = grid_carve(g, nullptr);
    char* arena = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&arena), arena_bytes) != hipSuccess) {
        ivx_set_error("ivx_grid_create: device allocation of %zu bytes failed", arena_bytes);
        delete g;
        return IVX_ERR_HIP;
    }
    g->arena = arena;
    (void)grid_carve(g, arena);
    if (ivx_memset_async(g->info, 0, sizeof(ivx_chunk_info) * g->n_chunks, c->stream) != hipSuccess ||
        ivx_memset_async(g->work_counts, 0, 8 * sizeof(uint32_t), c->stream) != hipSuccess) {
        ivx_set_error("ivx_grid_create: memset failed");
        ivx_grid_destroy(g);
        return IVX_ERR_HIP;
    }
    *out = g;
    return IVX_OK;
}

// Grids that come into being together (the fragments of an impact, fracturing.rs:1047-1189; docs/voxel_gpu_buffer_pooling.md:44-66): their
// arenas from ONE device allocation and their host-mapped result blocks from ONE pinned allocation, both released with the last of them.
// The chunk records and work counters start zeroed by ONE fill over the whole block. `ccs`: 3 chunk counts per grid; `who`: the call, for messages.
extern "C++" int grid_create_pooled(ivx_ctx* c, const uint32_t* ccs, size_t n, float voxel_extent, ivx_grid** out, const char* who) {
    for (size_t i = 0; i < n; ++i) out[i] = nullptr;
    if (n == 0) return IVX_OK;
    IVX_HIP_CHECK(hipSetDevice(c->device));
    auto fail = [&](int rc) {
        for (size_t i = 0; i < n; ++i) {
            if (out[i]) {  // (nothing of the blocks is theirs yet)
                out[i]->arena = nullptr, out[i]->arena_block = nullptr, out[i]->result_host = nullptr, out[i]->host_block = nullptr;
                delete out[i];
            }
            out[i] = nullptr;
        }
        return rc;
    };
    std::vector<size_t> off(n + 1, 0);
    for (size_t i = 0; i < n; ++i) {
        int rc = grid_new(c, ccs + 3 * i, voxel_extent, 0, 0, &out[i]);
        if (rc) return fail(rc);
        off[i + 1] = off[i] + ((grid_carve(out[i], nullptr) + 4095) & ~(size_t)4095);
    }
    ivx_block* blk = new (std::nothrow) ivx_block();
    if (!blk) return fail(IVX_ERR_CAPACITY);
    blk->dev = blk->pinned = nullptr;
    blk->refs = 0;
    if (hipMalloc(&blk->dev, off[n]) != hipSuccess || hipHostMalloc(&blk->pinned, n * IVX_RB_STRIDE_BYTES, hipHostMallocMapped) != hipSuccess) {
        ivx_set_error("%s: allocation of %zu bytes for %zu grids failed", who, off[n], n);
        blk->refs = 1;
        block_release(blk);
        return fail(IVX_ERR_HIP);
    }
    memset(blk->pinned, 0, n * IVX_RB_STRIDE_BYTES);
    void* pinned_dev = nullptr;
    if (hipHostGetDevicePointer(&pinned_dev, blk->pinned, 0) != hipSuccess) {
        blk->refs = 1;
        block_release(blk);
        return fail(IVX_ERR_HIP);
    }
    for (size_t i = 0; i < n; ++i) {
        ivx_grid* g = out[i];
        g->arena = static_cast<char*>(blk->dev) + off[i];
        (void)grid_carve(g, g->arena);
        g->arena_block = blk;
        g->result_host = reinterpret_cast<uint32_t*>(static_cast<char*>(blk->pinned) + i * IVX_RB_STRIDE_BYTES);
        g->result_host_dev = reinterpret_cast<uint32_t*>(static_cast<char*>(pinned_dev) + i * IVX_RB_STRIDE_BYTES);
        g->host_block = blk;
        blk->refs += 2;
    }
    return IVX_OK;
}

void ivx_grid_destroy(ivx_grid* g) {
    if (!g) return;
    (void)ivx_stream_sync(g->ctx->stream);
    ivx_sampler_free(g);  // (a pre-pass running ahead on the second stream is waited for)
    edit_free(g);
    ivx_submesh_manager_free(g->submesh_manager);  // (host mirrors of the incremental remesh and of the probes' ranges)
    ivx_probe_manager_free(g->probe_manager);
    g->submesh_manager = nullptr, g->probe_manager = nullptr;
    // (everything sized by the chunk counts lives in the arena; the rest grew on demand)
    if (g->dens_call) (void)hipFree(g->dens_call);
    mesh_group_free(g, 1u), mesh_group_free(g, 2u), mesh_group_free(g, 4u);  // (allocations of their own, or parts of a shared block)
    if (g->arena_block) {  // (the arena is a part of a block shared with the grids that came into being with this one)
        block_release(g->arena_block);
        g->arena = nullptr;
    }
    if (g->host_block) {
        block_release(g->host_block);
        g->result_host = nullptr;
    }
    void* ptrs[] = {g->arena, g->positions, g->normals, g->indices, g->index_materials, g->vertex_materials, g->submeshes, g->dev_scratch,
                    g->pairs_dev, g->probe_points, g->probe_chunk, g->probe_entries};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (g->host_scratch) (void)hipHostFree(g->host_scratch);
    if (g->result_host) (void)hipHostFree(g->result_host);
    stage_clock_free(g);
    delete g;
}

int ivx_grid_upload_dense(ivx_grid* g, const int8_t* sdf, const uint8_t* type, size_t n_voxels) {
    IVX_REQUIRE(g && sdf && type, IVX_ERR_INVALID, "ivx_grid_upload_dense: null argument");
    IVX_REQUIRE(n_voxels == g->n_vox, IVX_ERR_INVALID, "ivx_grid_upload_dense: expected %zu voxels, got %zu", g->n_vox, n_voxels);
    int rc;
    if ((rc = h2d(g, g->sdf, sdf, g->n_vox))) return rc;
    if ((rc = h2d(g, g->type, type, g->n_vox))) return rc;
    if ((rc = ivx_launch_classify(g))) return rc;
    ivx_voxels_replaced(g);
    IVX_HIP_CHECK(ivx_stream_sync(g->ctx->stream));
    return IVX_OK;
}

int ivx_grid_download_dense(ivx_grid* g, int8_t* sdf, uint8_t* type, uint8_t* flags, uint8_t* local_labels, ivx_chunk_info* info, size_t n_voxels) {
    IVX_REQUIRE(g, IVX_ERR_INVALID, "ivx_grid_download_dense: null grid");
    IVX_REQUIRE(n_voxels == g->n_vox, IVX_ERR_INVALID, "ivx_grid_download_dense: expected %zu voxels, got %zu", g->n_vox, n_voxels);
    int rc;
    if ((sdf || type || flags || local_labels) && (rc = ivx_ensure_dense(g))) return rc;  // Void / Uniform chunks are written out on demand
    if (sdf && (rc = d2h(g, sdf, g->sdf, g->n_vox))) return rc;
    if (type && (rc = d2h(g, type, g->type, g->n_vox))) return rc;
    if (flags && (rc = d2h(g, flags, g->flags, g->n_vox))) return rc;
    if (local_labels && (rc = d2h(g, local_labels, g->llabel, g->n_vox))) return rc;
    if (info && (rc = d2h(g, info, g->info, sizeof(ivx_chunk_info) * g->n_chunks))) return rc;
    return IVX_OK;
}

int ivx_grid_chunk_counts(ivx_grid* g, uint32_t out[3]) {
    IVX_REQUIRE(g && out, IVX_ERR_INVALID, "ivx_grid_chunk_counts: null argument");
    for (int d = 0; d < 3; ++d) out[d] = g->cc[d];
    return IVX_OK;
}

int ivx_grid_stage_counters(ivx_grid* g, uint32_t out[4]) {
    IVX_REQUIRE(g && out, IVX_ERR_INVALID, "ivx_grid_stage_counters: null argument");
    for (int i = 0; i < 4; ++i) out[i] = 0;
    int rc;
    if (ivx_eval_count(g)) {  // chunks evaluated per voxel by the sampler (three lists by LDS class)
        uint32_t ev[3];
        // (the live counters until the derive sweep has rolled them over into their statistics words, role_preset)
        if ((rc = d2h(g, ev, ivx_eval_count(g) + ((g->scratch_dirty & IVX_SCRATCH_EVAL) ? 0 : 8), sizeof(ev)))) return rc;
        out[0] = ev[0] + ev[1] + ev[2];
    }
    if ((rc = d2h(g, &out[1], g->rscalar + 2, sizeof(uint32_t)))) return rc;                            // chunks with several local regions
    if ((rc = d2h(g, &out[2], g->chunk_offsets + 2 * (size_t)g->n_chunks + 2, sizeof(uint32_t)))) return rc;  // chunks that emitted a mesh
    out[3] = g->n_chunks;
    return IVX_OK;
}

void* ivx_grid_device_ptr(ivx_grid* g, int which) {
    if (!g) return nullptr;
    if (which >= 0 && which < 4 && ivx_ensure_dense(g) != IVX_OK) return nullptr;  // whole planes for the caller (stream-ordered)
    if (which == 0 || which == 1 || which == 4) ivx_planes_touched(g);  // (the caller may write through the pointer)
    switch (which) {
        case 0: return g->sdf;
        case 1: return g->type;
        case 2: return g->flags;
        case 3: return g->llabel;
        case 4: return g->info;
        case 5: return g->rparent;
#ifdef IVX_WG_TRACE
        case 6: return g->chunk_moments;
#endif
        case 7: return g->smp.set[g->smp.cur].len;  // developer tools (tools/prog_stats.py): per-chunk compact program lengths, then the three list counters and lists
        case 8: return g->smp.set[g->smp.cur].ops;  // ... and the programs, OP_CAP (128) uint2 per chunk
        case 10: return g->sn_hard;  // ... and which (entries of the emit list)
        case 9: return ivx_sn_hard_count(g);  // developer tools: [0] how many chunks the mesher's last main pass handed to the general pass
        default: return nullptr;
    }
}

int ivx_sdf_sample(ivx_grid* g, const ivx_sdf_processed_node* nodes, size_t n_nodes, uint32_t stack_size, const uint32_t grid_shape[3],
                   const float shifted_grid_center[3], uint8_t voxel_type) {
    IVX_REQUIRE(g && grid_shape && shifted_grid_center, IVX_ERR_INVALID, "ivx_sdf_sample: null argument");
    IVX_REQUIRE(n_nodes == 0 || nodes, IVX_ERR_INVALID, "ivx_sdf_sample: null node array");
    for (int d = 0; d < 3; ++d) {
        const uint32_t cap = (d == 0 ? g->gx : g->cc[d]) * 16u;
        IVX_REQUIRE(grid_shape[d] <= cap, IVX_ERR_INVALID, "ivx_sdf_sample: grid shape %u exceeds the chunk grid (%u voxels) along axis %d", grid_shape[d], cap, d);
    }
    // validate the node program against the stack the kernel will use
    int depth = 0, max_depth = 0;
    for (size_t i = 0; i < n_nodes; ++i) {
        const uint32_t k = nodes[i].kind;
        IVX_REQUIRE(k <= 9, IVX_ERR_INVALID, "ivx_sdf_sample: unsupported node kind %u", k);
        IVX_REQUIRE(k != 6 || nodes[i].reserved[1] <= 255u, IVX_ERR_INVALID, "ivx_sdf_sample: noise node with more than 255 octaves");
        if (k <= 2) max_depth = std::max(max_depth, ++depth);
        else if (k >= 7) {
            IVX_REQUIRE(depth >= 2, IVX_ERR_INVALID, "ivx_sdf_sample: malformed node program (combination without two operands)");
            --depth;
        } else if (k == 5 || k == 6) {
            IVX_REQUIRE(depth >= 1, IVX_ERR_INVALID, "ivx_sdf_sample: malformed node program (scaling / noise without operand)");
        }
    }
    IVX_REQUIRE(n_nodes == 0 || depth == 1, IVX_ERR_INVALID, "ivx_sdf_sample: malformed node program (final stack depth %d)", depth);
    IVX_REQUIRE((uint32_t)max_depth <= stack_size || n_nodes == 0, IVX_ERR_INVALID, "ivx_sdf_sample: stack_size %u < required %d", stack_size, max_depth);
    int rc;
    if ((rc = ensure_dev_scratch(g, std::max<size_t>(n_nodes, 1) * sizeof(ivx_sdf_processed_node)))) return rc;
    {
        std::vector<ivx_sdf_processed_node> annotated(nodes, nodes + n_nodes);
        ivx_sdf_annotate_host(annotated.data(), n_nodes);
        if ((rc = h2d(g, g->dev_scratch, annotated.data(), n_nodes * sizeof(ivx_sdf_processed_node)))) return rc;
    }
    rc = ivx_launch_sdf_sample(g, static_cast<const ivx_sdf_processed_node*>(g->dev_scratch), (uint32_t)n_nodes, (uint32_t)max_depth, grid_shape,
                               shifted_grid_center, voxel_type, 0u, false, ivx_sdf_has_noise(nodes, n_nodes));
    if (rc) return rc;
    ivx_voxels_replaced(g);
    IVX_HIP_CHECK(ivx_stream_sync(g->ctx->stream));
    return IVX_OK;
}

int ivx_derive_state(ivx_grid* g) {
    IVX_REQUIRE(g, IVX_ERR_INVALID, "ivx_derive_state: null grid");
    int rc = ivx_launch_derive(g, 0);
    if (rc) return rc;
    g->mesh_valid = 0;
    g->regions_valid = 0;
    IVX_HIP_CHECK(ivx_stream_sync(g->ctx->stream));
    return IVX_OK;
}

int ivx_occupied_ranges(ivx_grid* g, uint32_t out[12]) {
    IVX_REQUIRE(g && out, IVX_ERR_INVALID, "ivx_occupied_ranges: null argument");
    IVX_REQUIRE(g->bbox_valid, IVX_ERR_STATE, "ivx_occupied_ranges: the chunk boxes come from the derive sweep (call ivx_derive_state first)");
    g->occ_ref_valid = 0;  // VoxelObject::update_occupied_ranges: reduced anew, and this is what the object holds from now on
    return reference_occupied(g, out);
}

// a density table for ONE call: the resident copy when it is the resident table (ivx_grid_set_densities), else a copy of its own behind the
// resident one — the object's resident table is what its steps and edits use and is never replaced on the side (round 3 overwrote the device
// copy here and left the host mirror saying otherwise: an edit handed the resident table again then ran on this call's)
static int densities_on_device(ivx_grid* g, const float densities[256], const float** d_out) {
    if (g->has_dens && memcmp(g->dens_host, densities, sizeof(g->dens_host)) == 0) {
        *d_out = g->dens_dev;
        return IVX_OK;
    }
    if (!g->dens_call) IVX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&g->dens_call), 256 * sizeof(float)));
    int rc = h2d(g, g->dens_call, densities, 256 * sizeof(float));
    if (rc) return rc;
    *d_out = g->dens_call;
    return IVX_OK;
}

int ivx_inertia(ivx_grid* g, const float densities[256], ivx_moments* out) {
    IVX_REQUIRE(g && densities && out, IVX_ERR_INVALID, "ivx_inertia: null argument");
    double* out_dev = g->partials + g->partial_blocks * 10;
    int rc;
    const float* d_dens = nullptr;
    if ((rc = densities_on_device(g, densities, &d_dens))) return rc;
    if ((rc = ivx_launch_inertia(g, d_dens, out_dev, 0))) return rc;
    if ((rc = d2h(g, out->m64, out_dev, 10 * sizeof(double)))) return rc;
    for (int i = 0; i < 10; ++i) out->m32[i] = (float)out->m64[i];
    out->reserved[0] = out->reserved[1] = 0;
    return IVX_OK;
}

int ivx_label_regions(ivx_grid* g, uint32_t* region_count) {
    IVX_REQUIRE(g && region_count, IVX_ERR_INVALID, "ivx_label_regions: null argument");
    int rc;
    if ((rc = ivx_launch_ccl_local(g, 0))) return rc;
    if ((rc = ivx_launch_ccl_merge(g))) return rc;
    if ((rc = ivx_launch_ccl_resolve(g))) return rc;
    uint32_t sc[IVX_RB_FLAGS + 1];  // (the region scalars: the head of what a step's result block holds)
    if ((rc = d2h(g, sc, g->rscalar, sizeof(sc)))) return rc;
    IVX_REQUIRE((sc[IVX_RB_FLAGS] & IVX_RB_FLAG_LOCAL_REGIONS) == 0, IVX_ERR_CAPACITY,
                "ivx_label_regions: a chunk has more than 254 local regions (the reference's CHUNK_MAX_REGIONS limit, split_detection.rs:145-157)");
    g->region_count = sc[IVX_RB_REGION_TOTAL];
    g->regions_valid = 1;
    *region_count = sc[IVX_RB_REGION_TOTAL];
    return IVX_OK;
}

int ivx_region_labels_download(ivx_grid* g, uint32_t* labels, size_t n_voxels) {
    IVX_REQUIRE(g && labels, IVX_ERR_INVALID, "ivx_region_labels_download: null argument");
    IVX_REQUIRE(g->regions_valid, IVX_ERR_STATE, "ivx_region_labels_download: call ivx_label_regions first");
    IVX_REQUIRE(n_voxels == g->n_vox, IVX_ERR_INVALID, "ivx_region_labels_download: expected %zu voxels, got %zu", g->n_vox, n_voxels);
    int rc;
    if ((rc = ensure_dev_scratch(g, g->n_vox * sizeof(uint32_t)))) return rc;
    if ((rc = ivx_launch_ccl_dense_labels(g, static_cast<uint32_t*>(g->dev_scratch)))) return rc;
    return d2h(g, labels, g->dev_scratch, g->n_vox * sizeof(uint32_t));
}

extern "C++" int describe_regions_internal(ivx_grid* g, const float* d_dens, std::vector<ivx_region_desc>& out) {
    const uint32_t n = g->region_count;
    out.assign(n, ivx_region_desc{});
    if (n == 0) return IVX_OK;
    const size_t bytes = ivx_region_stats_bytes(n);
    int rc;
    if ((rc = ensure_dev_scratch(g, bytes))) return rc;
    if ((rc = ivx_launch_region_stats(g, d_dens, g->dev_scratch, n))) return rc;
    std::vector<char> h(bytes);
    if ((rc = d2h(g, h.data(), g->dev_scratch, bytes))) return rc;
    const char* p = h.data();
    const unsigned long long* count = reinterpret_cast<const unsigned long long*>(p);
    p += 8 * (size_t)n;
    const double* mom = reinterpret_cast<const double*>(p);
    p += 80 * (size_t)n;
    const uint32_t* lo = reinterpret_cast<const uint32_t*>(p);
    p += 12 * (size_t)n;
    const uint32_t* hi = reinterpret_cast<const uint32_t*>(p);
    p += 12 * (size_t)n;
    const uint32_t* nu = reinterpret_cast<const uint32_t*>(p);
    p += 4 * (size_t)n;
    const uint32_t* ch = reinterpret_cast<const uint32_t*>(p);
    p += 4 * (size_t)n;
    const uint32_t* root = reinterpret_cast<const uint32_t*>(p);
    const double e = (double)g->extent, e2 = e * e, e3 = e2 * e, e4 = e2 * e2, e5 = e4 * e;
    for (uint32_t r = 0; r < n; ++r) {
        ivx_region_desc& o = out[r];
        o.root_chunk = root[r] >> 8;
        o.root_region = root[r] & 255u;
        o.voxel_count = count[r];
        for (int d3 = 0; d3 < 3; ++d3) {
            o.lo[d3] = lo[3 * r + d3];
            o.hi[d3] = hi[3 * r + d3];
        }
        o.non_uniform_chunk_count = nu[r];
        o.chunk_count = ch[r];
        for (int q = 0; q < 10; ++q) {
            const double f = q == 0 ? e3 : (q <= 3 ? 0.5 * e4 : (q <= 6 ? (1.0 / 3.0) * e5 : 0.25 * e5));
            o.moments[q] = mom[10 * (size_t)r + q] * f;
        }
    }
    return IVX_OK;
}

int ivx_regions_describe(ivx_grid* g, const float densities[256], ivx_region_desc* out, size_t cap, size_t* n_out) {
    IVX_REQUIRE(g && densities && out && n_out, IVX_ERR_INVALID, "ivx_regions_describe: null argument");
    IVX_REQUIRE(g->regions_valid, IVX_ERR_STATE, "ivx_regions_describe: call ivx_label_regions first");
    const uint32_t n = g->region_count;
    *n_out = n;
    IVX_REQUIRE(n <= cap, IVX_ERR_CAPACITY, "ivx_regions_describe: %u regions exceed capacity %zu", n, cap);
    int rc;
    const float* d_dens = nullptr;
    if ((rc = densities_on_device(g, densities, &d_dens))) return rc;
    std::vector<ivx_region_desc> d;
    if ((rc = describe_regions_internal(g, d_dens, d))) return rc;
    for (uint32_t r = 0; r < n; ++r) out[r] = d[r];
    return IVX_OK;
}

size_t ivx_region_face_bytes(ivx_grid* g) { return g ? (size_t)g->cc[1] * g->cc[2] * 256 * sizeof(uint16_t) : 0; }

int ivx_region_face_labels(ivx_grid* g, int side, void* device_buf) {
    IVX_REQUIRE(g && device_buf && (side == 0 || side == 1), IVX_ERR_INVALID, "ivx_region_face_labels: bad argument");
    IVX_REQUIRE(g->regions_valid, IVX_ERR_STATE, "ivx_region_face_labels: call ivx_label_regions first");
    int rc = ivx_launch_face_ids(g, side, static_cast<uint16_t*>(device_buf));
    if (rc) return rc;
    IVX_HIP_CHECK(ivx_stream_sync(g->ctx->stream));
    return IVX_OK;
}

int ivx_region_face_pairs(ivx_grid* g, int side, const void* neighbour_face_labels, uint32_t* pairs, size_t cap, size_t* n_out) {
    IVX_REQUIRE(g && neighbour_face_labels && n_out && (side == 0 || side == 1) && (pairs || cap == 0), IVX_ERR_INVALID,
                "ivx_region_face_pairs: bad argument");
    IVX_REQUIRE(g->regions_valid, IVX_ERR_STATE, "ivx_region_face_pairs: call ivx_label_regions first");
    const size_t face = (size_t)g->cc[1] * g->cc[2] * 256;
    int rc;
    if ((rc = ensure_dev_scratch(g, 16 + face * 8))) return rc;
    uint32_t* d_count = static_cast<uint32_t*>(g->dev_scratch);
    void* d_pairs = static_cast<char*>(g->dev_scratch) + 16;
    if ((rc = ivx_launch_face_pairs(g, side, static_cast<const uint16_t*>(neighbour_face_labels), d_count, d_pairs, (uint32_t)face, nullptr))) return rc;
    uint32_t n = 0;
    if ((rc = d2h(g, &n, d_count, sizeof(n)))) return rc;
    std::vector<uint64_t> h(n);
    if ((rc = d2h(g, h.data(), d_pairs, (size_t)n * 8))) return rc;
    // uint2{a,b} little-endian -> key a (low word) | b (high word); order by (a, b)
    for (auto& k : h) k = (k << 32) | (k >> 32);
    std::sort(h.begin(), h.end());
    h.erase(std::unique(h.begin(), h.end()), h.end());
    *n_out = h.size();
    IVX_REQUIRE(h.size() <= cap, IVX_ERR_CAPACITY, "ivx_region_face_pairs: %zu pairs exceed capacity %zu", h.size(), cap);
    for (size_t i = 0; i < h.size(); ++i) {
        pairs[2 * i] = (uint32_t)(h[i] >> 32);
        pairs[2 * i + 1] = (uint32_t)(h[i] & 0xFFFFFFFFu);
    }
    return IVX_OK;
}

int ivx_grid_set_sdf_program(ivx_grid* g, const ivx_sdf_processed_node* nodes, size_t n_nodes, uint32_t stack_size, const uint32_t grid_shape[3],
                             const float shifted_grid_center[3], uint8_t voxel_type) {
    IVX_REQUIRE(g && grid_shape && shifted_grid_center && (n_nodes == 0 || nodes), IVX_ERR_INVALID, "ivx_grid_set_sdf_program: null argument");
    int depth = 0, max_depth = 0;
    for (size_t i = 0; i < n_nodes; ++i) {
        const uint32_t k = nodes[i].kind;
        IVX_REQUIRE(k <= 9, IVX_ERR_INVALID, "ivx_grid_set_sdf_program: unsupported node kind %u", k);
        IVX_REQUIRE(k != 6 || nodes[i].reserved[1] <= 255u, IVX_ERR_INVALID, "ivx_grid_set_sdf_program: noise node with more than 255 octaves");
        if (k <= 2) max_depth = std::max(max_depth, ++depth);
        else if (k >= 7) {
            IVX_REQUIRE(depth >= 2, IVX_ERR_INVALID, "ivx_grid_set_sdf_program: malformed node program");
            --depth;
        } else if (k == 5 || k == 6) {
            IVX_REQUIRE(depth >= 1, IVX_ERR_INVALID, "ivx_grid_set_sdf_program: malformed node program");
        }
    }
    IVX_REQUIRE(n_nodes == 0 || depth == 1, IVX_ERR_INVALID, "ivx_grid_set_sdf_program: malformed node program (final stack depth %d)", depth);
    IVX_REQUIRE(n_nodes == 0 || (uint32_t)max_depth <= stack_size, IVX_ERR_INVALID, "ivx_grid_set_sdf_program: stack_size too small");
    for (int d = 0; d < 3; ++d) {
        const uint32_t cap = (d == 0 ? g->gx : g->cc[d]) * 16u;
        IVX_REQUIRE(grid_shape[d] <= cap, IVX_ERR_INVALID, "ivx_grid_set_sdf_program: grid shape exceeds the chunk grid along axis %d", d);
    }
    {  // a pre-pass that runs ahead reads the resident program: wait for it, drop what it wrote
        const int rc_a = ivx_sampler_ahead_cancel(g);
        if (rc_a) return rc_a;
    }
    auto& prog = g->smp.prog;
    if (n_nodes > prog.cap) {
        IVX_HIP_CHECK(ivx_stream_sync(g->ctx->stream));
        if (prog.nodes) (void)hipFree(prog.nodes);
        prog.nodes = nullptr;
        prog.cap = 0;
        int rc = dev_alloc(&prog.nodes, n_nodes);
        if (rc) return rc;
        prog.cap = (uint32_t)n_nodes;
    }
    std::vector<ivx_sdf_processed_node> annotated(nodes, nodes + n_nodes);
    ivx_sdf_annotate_host(annotated.data(), n_nodes);
    int rc = h2d(g, prog.nodes, annotated.data(), n_nodes * sizeof(ivx_sdf_processed_node));
    if (rc) return rc;
    ivx_sampler_set_program(g, (uint32_t)n_nodes, (uint32_t)max_depth, grid_shape, shifted_grid_center, voxel_type, ivx_sdf_has_noise(nodes, n_nodes));
    return IVX_OK;
}

int ivx_grid_set_voxel_type_noise(ivx_grid* g, uint32_t n_voxel_types, float noise_frequency, float voxel_type_frequency, uint32_t seed) {
    IVX_REQUIRE(g, IVX_ERR_INVALID, "ivx_grid_set_voxel_type_noise: null grid");
    IVX_REQUIRE(n_voxel_types <= 255u, IVX_ERR_INVALID, "ivx_grid_set_voxel_type_noise: %u voxel types (at most 255: 255 is the dummy type)", n_voxel_types);
    IVX_REQUIRE(std::isfinite(noise_frequency) && std::isfinite(voxel_type_frequency), IVX_ERR_INVALID, "ivx_grid_set_voxel_type_noise: non-finite frequency");
    if (g->smp.vt.n == 0u && n_voxel_types == 0u) return IVX_OK;  // (SameVoxelTypeGenerator before and after: the parameters say nothing)
    {  // the records a pre-pass that runs ahead has parked carry the type of the generator it ran under: wait for it, drop what it wrote
        const int rc_a = ivx_sampler_ahead_cancel(g);
        if (rc_a) return rc_a;
    }
    ivx_sampler_set_types(g, n_voxel_types, noise_frequency, voxel_type_frequency, seed);
    return IVX_OK;
}

int ivx_grid_set_densities(ivx_grid* g, const float densities[256]) {
    IVX_REQUIRE(g && densities, IVX_ERR_INVALID, "ivx_grid_set_densities: null argument");
    // (stream-ordered, no wait: the copy reads the grid's own host copy of the table, which lives as long as the grid — a table set again
    // before the copy has run may reach the device twice, in the right order. Setting the tables of the fragments of an impact used to cost a
    // pinned allocation and two waits each.)
    memcpy(g->dens_host, densities, sizeof(g->dens_host));
    if (!ivx_many_upload(g->ctx, g, g->dens_dev, g->dens_host, sizeof(g->dens_host)))
        IVX_HIP_CHECK(ivx_memcpy_async(g->dens_dev, g->dens_host, sizeof(g->dens_host), hipMemcpyHostToDevice, g->ctx->stream));
    g->has_dens = 1;
    return IVX_OK;
}

size_t ivx_halo_bytes(ivx_grid* g) {
    if (!g) return 0;
    const size_t cols = (size_t)g->cc[1] * g->cc[2];
    return cols * (256 + 256 + sizeof(ivx_chunk_info));
}

int ivx_halo_pack(ivx_grid* g, int side, void* device_buf) {
    IVX_REQUIRE(g && device_buf && (side == 0 || side == 1), IVX_ERR_INVALID, "ivx_halo_pack: bad argument");
    int rc = ivx_launch_halo_pack(g, side, device_buf);
    if (rc) return rc;
    IVX_HIP_CHECK(ivx_stream_sync(g->ctx->stream));
    return IVX_OK;
}

int ivx_halo_unpack(ivx_grid* g, int side, const void* device_buf) {
    IVX_REQUIRE(g && device_buf && (side == 0 || side == 1), IVX_ERR_INVALID, "ivx_halo_unpack: bad argument");
    const size_t cols = (size_t)g->cc[1] * g->cc[2];
    hipStream_t s = g->ctx->stream;
    const uint8_t* b = static_cast<const uint8_t*>(device_buf);
    IVX_HIP_CHECK(ivx_memcpy_async(g->ghost_sdf[side], b, cols * 256, hipMemcpyDeviceToDevice, s));
    IVX_HIP_CHECK(ivx_memcpy_async(g->ghost_type[side], b + cols * 256, cols * 256, hipMemcpyDeviceToDevice, s));
    IVX_HIP_CHECK(ivx_memcpy_async(g->ghost_info[side], b + cols * 512, cols * sizeof(ivx_chunk_info), hipMemcpyDeviceToDevice, s));
    g->has_ghost[side] = 1;
    g->ghost_ext[side] = nullptr;
    IVX_HIP_CHECK(ivx_stream_sync(s));
    return IVX_OK;
}

int ivx_halo_pack_enqueue(ivx_grid* g, int side, void* device_buf) {
    IVX_REQUIRE(g && device_buf && (side == 0 || side == 1), IVX_ERR_INVALID, "ivx_halo_pack_enqueue: bad argument");
    return ivx_launch_halo_pack(g, side, device_buf);
}

int ivx_halo_unpack_enqueue(ivx_grid* g, int side, const void* device_buf) {
    IVX_REQUIRE(g && device_buf && (side == 0 || side == 1), IVX_ERR_INVALID, "ivx_halo_unpack_enqueue: bad argument");
    IVX_REQUIRE((reinterpret_cast<uintptr_t>(device_buf) & 15u) == 0, IVX_ERR_INVALID, "ivx_halo_unpack_enqueue: the buffer must be 16-byte aligned");
    // no copy: the kernels read the ghost layer in place from the receive buffer (three copies per side and exchange were a
    // sixth of a multi-GPU step's launches); the caller keeps it untouched until it installs the next one
    g->ghost_ext[side] = static_cast<const uint8_t*>(device_buf);
    g->has_ghost[side] = 1;
    return IVX_OK;
}

int ivx_halo_pack_both_enqueue(ivx_grid* g, void* lower_buf, void* upper_buf, int with_face_labels) {
    IVX_REQUIRE(g && (lower_buf || upper_buf), IVX_ERR_INVALID, "ivx_halo_pack_both_enqueue: bad argument");
    return ivx_launch_halo_pack_both(g, lower_buf, upper_buf, with_face_labels);
}

int ivx_region_face_labels_enqueue(ivx_grid* g, int side, void* device_buf) {
    IVX_REQUIRE(g && device_buf && (side == 0 || side == 1), IVX_ERR_INVALID, "ivx_region_face_labels_enqueue: bad argument");
    return ivx_launch_face_ids(g, side, static_cast<uint16_t*>(device_buf));
}

// ---- many objects per call (many.hpp) ---------------------------------------------------------------------------------------------------
// The per-object host code runs object after object while the launches are recorded; one flush issues a launch per chain position for all of
// them; the results come back through every object's own host-mapped block, their gathers launched as one (many_check, many_phase: many.cpp).
// A many-object call that fails half way — an object's enqueue refused, a flush failed — must not leave the objects before it "in flight":
// the stream is drained, every object's collect half runs with its results discarded, and whatever flag still says "pending" is cleared, so
// that the next call on any of these objects starts clean (their derived state is what the launches that did run left: step them again).
extern "C++" int many_fail(ivx_grid* const* grids, size_t n, int rc) {
    if (!rc || !n) return rc;
    char keep[512];
    snprintf(keep, sizeof(keep), "%s", ivx_last_error());  // (the collects below may set messages of their own: the caller gets the first failure's)
    (void)ivx_stream_sync(grids[0]->ctx->stream);
    (void)ivx_many_error(grids[0]->ctx, true);
    for (size_t i = 0; i < n; ++i) {
        ivx_grid* g = grids[i];
        if (!g) continue;
        edit_abandon(g);
        mesh_sync_abandon(g);
        if (g->pending_stages || g->gather_launched) {
            ivx_step_result tmp;
            (void)ivx_voxel_step_collect(g, &tmp);
        }
        g->pending_stages = 0;
        g->gather_launched = 0;
        g->results_in_block = 0;
        g->defer_mesh_growth = 0;
        if (g->mesh_growth_pending) g->mesh_growth_pending = 0, g->mesh_valid = 0;
    }
    ivx_set_error("%s", keep);
    return rc;
}

int ivx_halo_clear(ivx_grid* g, int side) {
    IVX_REQUIRE(g && (side == 0 || side == 1), IVX_ERR_INVALID, "ivx_halo_clear: bad argument");
    g->has_ghost[side] = 0;
    g->ghost_ext[side] = nullptr;
    return IVX_OK;
}

}  // extern "C"
