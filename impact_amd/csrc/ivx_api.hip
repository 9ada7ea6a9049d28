// C ABI entry points of libimpact_voxel_hip.so (see include/impact_voxel_hip.h for the contract and
// the reference interfaces each function replaces). Host-side orchestration only: every compute call
// launches the HIP kernels in this directory on the context's stream.
#include <algorithm>
#include <array>
#include <functional>
#include <cmath>
#include <atomic>
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

// Host<->device copies. Small ones (the scalars and tables the entry points hand back: up to a few hundred KB) go through the
// grid's pinned staging buffer as ONE stream-ordered copy and ONE wait (a blocking copy from pageable memory costs a wait for
// the stream, a staging copy inside the runtime and a second wait); large ones (whole planes) stay plain blocking copies.
constexpr size_t STAGED_COPY_MAX = 1u << 20;
}  // namespace
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
static int reference_occupied(ivx_grid* g, uint32_t occ[12]) {
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
    if (hipMalloc(&blk->dev, off[n]) != hipSuccess || hipHostMalloc(&blk->pinned, n * 256, hipHostMallocMapped) != hipSuccess) {
        ivx_set_error("%s: allocation of %zu bytes for %zu grids failed", who, off[n], n);
        blk->refs = 1;
        block_release(blk);
        return fail(IVX_ERR_HIP);
    }
    memset(blk->pinned, 0, n * 256);
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
        g->result_host = reinterpret_cast<uint32_t*>(static_cast<char*>(blk->pinned) + i * 256);
        g->result_host_dev = reinterpret_cast<uint32_t*>(static_cast<char*>(pinned_dev) + i * 256);
        g->host_block = blk;
        blk->refs += 2;
    }
    return IVX_OK;
}

static void ivx_edit_state_free(struct ivx_edit_state* e);
void ivx_grid_destroy(ivx_grid* g) {
    if (!g) return;
    (void)ivx_stream_sync(g->ctx->stream);
    ivx_sampler_ahead_free(g);  // (a pre-pass running ahead on the second stream is waited for)
    ivx_edit_state_free(g->edit);
    g->edit = nullptr;
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
    void* ptrs[] = {g->arena, g->positions, g->normals, g->indices, g->index_materials, g->vertex_materials, g->submeshes, g->dev_scratch, g->prog_nodes,
                    g->samp_len, g->samp_ops, g->pairs_dev, g->samp_super, g->probe_points, g->probe_chunk, g->probe_entries};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (g->host_scratch) (void)hipHostFree(g->host_scratch);
    if (g->result_host) (void)hipHostFree(g->result_host);
    if (g->tick_dev) (void)hipFree(g->tick_dev);  // (the stage stamps' words: two small allocations of their own, made on first use)
    if (g->tick_host) (void)hipHostFree(g->tick_host);
    if (g->ev_ready)
        for (int i = 0; i < 2 * IVX_N_TIMED_STAGES; ++i) (void)hipEventDestroy(g->ev[i]);
    delete g;
}

int ivx_grid_upload_dense(ivx_grid* g, const int8_t* sdf, const uint8_t* type, size_t n_voxels) {
    IVX_REQUIRE(g && sdf && type, IVX_ERR_INVALID, "ivx_grid_upload_dense: null argument");
    IVX_REQUIRE(n_voxels == g->n_vox, IVX_ERR_INVALID, "ivx_grid_upload_dense: expected %zu voxels, got %zu", g->n_vox, n_voxels);
    int rc;
    if ((rc = h2d(g, g->sdf, sdf, g->n_vox))) return rc;
    if ((rc = h2d(g, g->type, type, g->n_vox))) return rc;
    if ((rc = ivx_launch_classify(g))) return rc;
    g->mesh_valid = 0;
    g->mesh_built = 0;
    g->occ_ref_valid = 0;
    g->bbox_valid = 0;
    g->regions_valid = 0;
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
    if (g->samp_len) {  // chunks evaluated per voxel by the sampler (three lists by LDS class)
        uint32_t ev[3];
        // (the live counters until the derive sweep has rolled them over into their statistics words, role_preset)
        if ((rc = d2h(g, ev, g->samp_len + g->n_chunks + ((g->scratch_dirty & IVX_SCRATCH_EVAL) ? 0 : 8), sizeof(ev)))) return rc;
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
        case 7: return g->samp_len;  // developer tools (tools/prog_stats.py): per-chunk compact program lengths, then the three list counters and lists
        case 8: return g->samp_ops;  // ... and the programs, OP_CAP (128) uint2 per chunk
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
    g->mesh_valid = 0;
    g->mesh_built = 0;
    g->occ_ref_valid = 0;
    g->bbox_valid = 0;
    g->regions_valid = 0;
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
    uint32_t* d = g->rscalar + 16;
    int rc;
    if ((rc = ivx_launch_occupied(g, d))) return rc;
    uint32_t raw[12];
    if ((rc = d2h(g, raw, d, 12 * sizeof(uint32_t)))) return rc;
    ivx_occupied_from_raw(g, raw, out);
    memcpy(g->occ_ref, out, sizeof(g->occ_ref));  // VoxelObject::update_occupied_ranges: this is what the object holds from now on
    g->occ_ref_valid = 1;
    return IVX_OK;
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
    uint32_t sc[2];
    if ((rc = d2h(g, sc, g->rscalar, sizeof(sc)))) return rc;
    IVX_REQUIRE((sc[1] & 1u) == 0, IVX_ERR_CAPACITY,
                "ivx_label_regions: a chunk has more than 254 local regions (the reference's CHUNK_MAX_REGIONS limit, split_detection.rs:145-157)");
    g->region_count = sc[0];
    g->regions_valid = 1;
    *region_count = sc[0];
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
    uint32_t lo[3] = {0, 0, 0}, cc[3] = {0, 0, 0}, blo[3] = {0, 0, 0}, bcc[3] = {0, 0, 0};
    size_t off_type = 0, off_cnt = 0, off_touch = 0, off_needs = 0, total = 0;
    void* pinned = nullptr;  // results of the edit in flight: host-mapped, written by the step's gather launch ahead of the doorbell
    void* pinned_dev = nullptr;
    size_t pinned_bytes = 0;
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
    size_t off_early = 0, off_bell = 0;
};
static void ivx_edit_state_free(ivx_edit_state* e) {
    if (!e) return;
    if (e->pinned) (void)hipHostFree(e->pinned);
    if (e->d_results) (void)hipFree(e->d_results);
    delete e;
}
static ivx_edit_state* edit_state(ivx_grid* g) {
    if (!g->edit) g->edit = new (std::nothrow) ivx_edit_state();
    return g->edit;
}
extern "C++" bool edit_needs_lookup(ivx_grid* g, uint32_t chunk, uint32_t out3[3]) {
    if (!g->edit) return false;
    const auto& v = g->edit->needs;
    const auto it = std::lower_bound(v.begin(), v.end(), chunk, [](const std::array<uint32_t, 4>& a, uint32_t c) { return a[0] < c; });
    if (it == v.end() || (*it)[0] != chunk) return false;
    out3[0] = (*it)[1], out3[1] = (*it)[2], out3[2] = (*it)[3];
    return true;
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
    int32_t vlo[3], vhi[3];
    uint32_t lo[3], cc[3];
    e->nothing = 0;
    for (int d = 0; d < 3; ++d) {
        float a = center[d] - influence_radius, b = center[d] + influence_radius;  // Sphere::compute_aabb
        if (capsule) {  // Capsule::compute_aabb: the boxes of the two end spheres (capsule.rs:132-137)
            const float end = center[d] + seg[d];
            const float a1 = end - influence_radius, b1 = end + influence_radius;
            a = a1 < a ? a1 : a;
            b = b1 > b ? b1 : b;
        }
        const float fl = std::floor(a), ce = std::ceil(b);
        // `as usize` saturates at 0; the occupied ranges bound the other side
        const long s_ = fl > 0.0f ? (fl < 2.0e9f ? (long)fl : 2000000000L) : 0, e_ = ce > 0.0f ? (ce < 2.0e9f ? (long)ce : 2000000000L) : 0;
        vlo[d] = (int32_t)std::max<long>((long)occ[6 + 2 * d], s_);
        vhi[d] = (int32_t)std::min<long>((long)occ[7 + 2 * d], e_);
        if (vlo[d] >= vhi[d]) {
            e->nothing = 1;  // nothing touched: the collect reports zeros
            e->pending = 1;
            return IVX_OK;
        }
        lo[d] = (uint32_t)vlo[d] / 16u;
        cc[d] = ((uint32_t)vhi[d] + 15u) / 16u - lo[d];
    }
    uint32_t blo[3], bcc[3];  // the box the derive sweep goes over: one chunk more each way
    for (int d = 0; d < 3; ++d) {
        blo[d] = lo[d] > 0u ? lo[d] - 1u : 0u;
        const uint32_t bhi = std::min(lo[d] + cc[d] + 1u, g->cc[d]);
        bcc[d] = bhi - blo[d];
        e->lo[d] = lo[d], e->cc[d] = cc[d], e->blo[d] = blo[d], e->bcc[d] = bcc[d];
    }
    // scratch: [10 f64 removed moments][256 u32 by type][2 u32 counters][pad][u32 touched ranges of the box's chunks][uint4 needs of the grown box's]
    const size_t box_chunks = (size_t)cc[0] * cc[1] * cc[2], grown = (size_t)bcc[0] * bcc[1] * bcc[2];
    e->off_type = 80, e->off_cnt = e->off_type + 1024, e->off_touch = e->off_cnt + 16;
    e->off_needs = (e->off_touch + box_chunks * 4 + 15) & ~(size_t)15;
    e->total = e->off_needs + grown * 16;
    hipStream_t s = g->ctx->stream;
    // (a density table other than the resident one rides in the block's LAST kilobyte — not right behind this edit's results: nothing clears it
    // there, and a later, larger edit would read its floats as the touched words of its box: 1.0f is "touched, voxels 0..0, 0..0, 0..8" — five
    // chunks invalidated for nothing in one of 3 600 random edit sequences, profiles/round5/README.md)
    const size_t need_bytes = ((e->total + 255) & ~(size_t)255) + 1024;
    if (e->d_results_bytes < need_bytes) {  // (grown on demand; a fresh block starts zeroed, later ones are cleared behind every collect)
        IVX_HIP_CHECK(ivx_stream_sync(s));
        if (e->d_results) (void)hipFree(e->d_results);
        e->d_results = nullptr, e->d_results_bytes = 0;
        const size_t cap = std::max<size_t>(2 * need_bytes, 1 << 16);
        IVX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&e->d_results), cap));
        IVX_HIP_CHECK(ivx_memset_async(e->d_results, 0, cap, s));
        e->d_results_bytes = cap;
    }
    char* base = e->d_results;
    const size_t off_dens = e->d_results_bytes - 1024;
    const float* d_dens = g->dens_dev;
    if (!(g->has_dens && memcmp(g->dens_host, densities, sizeof(g->dens_host)) == 0)) {  // another table than the resident one
        if ((rc = h2d(g, base + off_dens, densities, 1024))) return rc;
        d_dens = reinterpret_cast<const float*>(base + off_dens);
    }
    // the edit; its first block also zeroes the region scalars the sweep behind it starts from
    if ((rc = ivx_launch_absorb(g, capsule, lo, cc, vlo, vhi, center, seg, influence_radius, shape_radius, d_dens, reinterpret_cast<double*>(base),
                                reinterpret_cast<uint32_t*>(base + e->off_type), reinterpret_cast<uint32_t*>(base + e->off_cnt),
                                reinterpret_cast<uint32_t*>(base + e->off_touch), g->rscalar)))
        return rc;
    e->needs.clear();  // (voxels change: what an earlier edit's chunks needed is history)
    // derived state and chunk-local regions of the grown box, the other chunks' region nodes reset; then the global resolve, whose first
    // launch also counts what the invalidated chunks' meshes need, and whose last (the gather of ivx_absorb_collect) copies the edit's small
    // results to the host ahead of the doorbell: seven launches, no copy or fill operation on the stream
    if ((rc = ivx_launch_derive_box(g, IVX_PART_REGIONS, blo, bcc, nullptr))) return rc;
    e->staged = e->total <= STAGED_COPY_MAX;
    e->off_early = (e->total + 63) & ~(size_t)63;
    e->off_bell = e->off_early + grown * 16;
    const size_t pinned_need = e->off_bell + 64;
    if (e->staged && e->pinned_bytes < pinned_need) {
        IVX_HIP_CHECK(ivx_stream_sync(s));
        if (e->pinned) (void)hipHostFree(e->pinned);
        e->pinned = e->pinned_dev = nullptr, e->pinned_bytes = 0;
        const size_t cap = std::max<size_t>(2 * pinned_need, 1 << 16);
        IVX_HIP_CHECK(hipHostMalloc(&e->pinned, cap, hipHostMallocMapped));
        IVX_HIP_CHECK(hipHostGetDevicePointer(&e->pinned_dev, e->pinned, 0));
        memset(e->pinned, 0, cap);
        e->pinned_bytes = cap;
    }
    for (int d = 0; d < 3; ++d) g->post1_needs_box[d] = lo[d], g->post1_needs_box[3 + d] = cc[d], g->post1_needs_box[6 + d] = blo[d], g->post1_needs_box[9 + d] = bcc[d];
    g->post1_needs_touched = reinterpret_cast<const uint32_t*>(base + e->off_touch);
    g->post1_needs_out = reinterpret_cast<uint32_t*>(base + e->off_needs);
    e->early_armed = 0, e->early_taken = 0;
    if (e->staged && g->early_needs_on) {  // (the words [2], [3] behind the two counters are the block's spare: zero between edits like the rest)
        e->early_seq += 1u;
        g->post1_needs_early = reinterpret_cast<uint32_t*>(static_cast<char*>(e->pinned_dev) + e->off_early);
        g->post1_needs_counter = reinterpret_cast<uint32_t*>(base + e->off_cnt) + 2;
        g->post1_needs_bell = reinterpret_cast<uint32_t*>(static_cast<char*>(e->pinned_dev) + e->off_bell);
        g->post1_needs_seq = e->early_seq;
        // (the bell's place moves with the size of the box: whatever an earlier, larger edit left there must not read as this edit's number)
        *reinterpret_cast<volatile uint32_t*>(static_cast<char*>(e->pinned) + e->off_bell) = 0u;
        e->early_armed = 1;
    }
    g->preset_fresh |= IVX_SCRATCH_REGIONS;  // (the region scalars were zeroed by the edit kernel, before the box sweep listed its multi-region chunks)
    g->regions_labelled_locally = 1;         // (... and the sweep labelled the box: no stand-alone local pass in front of the resolve)
    rc = step_enqueue_untimed(g, IVX_STAGE_REGIONS);  // (nobody reads this call's stage times)
    g->regions_labelled_locally = 0;
    if (rc) return rc;
    if (e->staged) {
        g->gather_copy_src = reinterpret_cast<const uint32_t*>(base);
        g->gather_copy_dst = static_cast<uint32_t*>(e->pinned_dev);
        // (with early delivery the needs records are in the host-mapped block already: the gather copies the words in front of them only)
        g->gather_copy_words = (uint32_t)(((e->early_armed ? e->off_needs : e->total) + 3) / 4);
    }
    e->pending = 1;
    return IVX_OK;
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
    std::vector<char> hostbuf;
    const char* hb;
    if (e->staged) {
        hb = static_cast<const char*>(e->pinned);
    } else {
        hostbuf.resize(e->total);
        if ((rc = d2h(g, hostbuf.data(), e->d_results, e->total))) return rc;
        hb = hostbuf.data();
    }
    // (the accumulators and the touched words start the next edit from zero — and that edit's box may be larger than this one's: everything this
    // edit wrote is cleared now, off the next edit's path; the block beyond has never been written)
    if (!ivx_many_zero(g->ctx, g, e->d_results, (e->total + 3) & ~(size_t)3)) IVX_HIP_CHECK(ivx_memset_async(e->d_results, 0, e->total, g->ctx->stream));
    const double* rem = reinterpret_cast<const double*>(hb);
    const double ex = (double)g->extent, e3 = ex * ex * ex, e4 = e3 * ex, e5 = e4 * ex;
    const double f[10] = {e3, 0.5 * e4, 0.5 * e4, 0.5 * e4, e5 / 3.0, e5 / 3.0, e5 / 3.0, 0.25 * e5, 0.25 * e5, 0.25 * e5};
    for (int q = 0; q < 10; ++q) out->removed_moments[q] = rem[q] * f[q];
    const uint32_t* by_type = reinterpret_cast<const uint32_t*>(hb + e->off_type);
    uint64_t emptied = 0;
    for (int t = 0; t < 256; ++t) {
        emptied += by_type[t];
        if (emptied_by_type) emptied_by_type[t] = by_type[t];
    }
    out->emptied_voxels = emptied;
    const uint32_t* cnt = reinterpret_cast<const uint32_t*>(hb + e->off_cnt);
    out->touched_chunks = cnt[0];
    out->removed_chunks = cnt[1];
    if (cnt[1]) g->occ_ref_valid = 0;  // `if removed_chunks { self.update_occupied_ranges() }` (intersection.rs:384-386, 520-522)
    // handle_chunk_voxels_modified (intersection.rs:560-598): the touched chunk, and a neighbour when the touched voxel range of the chunk
    // comes within two voxels of the face they share — decided on the device per chunk of the grown box, with what its mesh needs now
    const uint32_t* needs = reinterpret_cast<const uint32_t*>(e->early_armed ? static_cast<const char*>(e->pinned) + e->off_early : hb + e->off_needs);
    const size_t grown = (size_t)e->bcc[0] * e->bcc[1] * e->bcc[2];
    e->needs.clear();  // (an early sync may have filled them from the same records)
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
    return IVX_OK;
}

// what the edit in flight invalidates and what those meshes need, from the records its count role delivers early (ivx_edit_state::early_*):
// waits for the role's bell — a third of the way down the edit's chain —, not for the edit
extern "C++" int edit_early_needs(ivx_grid* g, const char* who, std::vector<uint32_t>& list) {
    ivx_edit_state* e = g->edit;
    IVX_REQUIRE(e && e->pending, IVX_ERR_STATE, "%s: a null set stands for the chunks of an edit in flight, and none is", who);
    if (e->nothing) return IVX_OK;
    IVX_REQUIRE(e->early_armed, IVX_ERR_STATE,
                "%s: the edit in flight does not deliver its mesh needs early (ivx_grid_set_early_mesh_needs before the edit; or its results do not fit the "
                "host-mapped block): collect it and pass its set",
                who);
    if (!e->early_taken) {
        const volatile uint32_t* bell = reinterpret_cast<const volatile uint32_t*>(static_cast<const char*>(e->pinned) + e->off_bell);
        (void)ivx_many_break();
        bool rung = false;
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t it = 0;; ++it) {
            if (*bell == e->early_seq) {
                rung = true;
                break;
            }
            __builtin_ia32_pause();
            if ((it & 255u) == 255u && std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > 2000) break;
        }
        if (!rung) IVX_HIP_CHECK(ivx_stream_sync(g->ctx->stream));
        std::atomic_thread_fence(std::memory_order_acquire);
        IVX_REQUIRE(*bell == e->early_seq, IVX_ERR_HIP, "%s: the edit's mesh needs never arrived", who);
        const uint32_t* needs = reinterpret_cast<const uint32_t*>(static_cast<const char*>(e->pinned) + e->off_early);
        const size_t grown = (size_t)e->bcc[0] * e->bcc[1] * e->bcc[2];
        e->needs.clear();
        for (size_t b = 0; b < grown; ++b) {
            const uint32_t w = needs[4 * b];
            if (!(w & 0x80000000u)) continue;
            e->needs.push_back({needs[4 * b + 3], needs[4 * b + 1], needs[4 * b + 2], w & 0xFFFFu});
        }
        if (!std::is_sorted(e->needs.begin(), e->needs.end(), [](const std::array<uint32_t, 4>& a, const std::array<uint32_t, 4>& b) { return a[0] < b[0]; }))
            std::sort(e->needs.begin(), e->needs.end(), [](const std::array<uint32_t, 4>& a, const std::array<uint32_t, 4>& b) { return a[0] < b[0]; });
        g->needs_current = 1;
        e->early_taken = 1;
    }
    for (const auto& n : e->needs) list.push_back(n[0]);
    return IVX_OK;
}

extern "C" {
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
}  // extern "C"

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
    if (n_nodes > g->prog_cap) {
        IVX_HIP_CHECK(ivx_stream_sync(g->ctx->stream));
        if (g->prog_nodes) (void)hipFree(g->prog_nodes);
        g->prog_nodes = nullptr;
        g->prog_cap = 0;
        int rc = dev_alloc(&g->prog_nodes, n_nodes);
        if (rc) return rc;
        g->prog_cap = (uint32_t)n_nodes;
    }
    std::vector<ivx_sdf_processed_node> annotated(nodes, nodes + n_nodes);
    ivx_sdf_annotate_host(annotated.data(), n_nodes);
    int rc = h2d(g, g->prog_nodes, annotated.data(), n_nodes * sizeof(ivx_sdf_processed_node));
    if (rc) return rc;
    g->prog_n = (uint32_t)n_nodes;
    g->prog_stack = (uint32_t)max_depth;
    for (int d = 0; d < 3; ++d) {
        g->prog_shape[d] = grid_shape[d];
        g->prog_center[d] = shifted_grid_center[d];
    }
    g->prog_type = voxel_type;
    g->prog_noise = ivx_sdf_has_noise(nodes, n_nodes) ? 1 : 0;
    g->eval_len_valid = 0;
    g->eval_len_pending = 0;
    return IVX_OK;
}

int ivx_grid_set_voxel_type_noise(ivx_grid* g, uint32_t n_voxel_types, float noise_frequency, float voxel_type_frequency, uint32_t seed) {
    IVX_REQUIRE(g, IVX_ERR_INVALID, "ivx_grid_set_voxel_type_noise: null grid");
    IVX_REQUIRE(n_voxel_types <= 255u, IVX_ERR_INVALID, "ivx_grid_set_voxel_type_noise: %u voxel types (at most 255: 255 is the dummy type)", n_voxel_types);
    IVX_REQUIRE(std::isfinite(noise_frequency) && std::isfinite(voxel_type_frequency), IVX_ERR_INVALID, "ivx_grid_set_voxel_type_noise: non-finite frequency");
    if (g->vt_n == 0u && n_voxel_types == 0u) return IVX_OK;  // (SameVoxelTypeGenerator before and after: the parameters say nothing)
    {  // the records a pre-pass that runs ahead has parked carry the type of the generator it ran under: wait for it, drop what it wrote
        const int rc_a = ivx_sampler_ahead_cancel(g);
        if (rc_a) return rc_a;
    }
    g->vt_n = n_voxel_types;
    g->vt_noise_freq = noise_frequency;
    g->vt_type_freq = voxel_type_frequency;
    g->vt_seed = seed;
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

// Timed slots of a step (ivx_step_result::stage_ms): 0 sample (k_sdf_super, k_sdf_prepass, k_sdf_eval), 1 derive (k_chunk_pre, k_derive:
// flags, chunk state, chunk-local regions, chunk moments), 2 k_step_post1 (mesher count | region merge by columns | occupied slots
// | moment partial sums), 3 k_step_post2 (exact local numbering -> multi-region merge | mesher scan | moments and occupied ranges
// final), 4 k_step_emit (region forest flatten | mesher emit), 5 k_step_assign (component ids); 6..9 unused.
//
// How a timed slot is measured. On the step's fused path — a whole call (`part` 3) outside the slab protocol's remesh phase, on a grid
// the fused assign reaches, with the derive stage in it or nothing left for the stand-alone per-chunk kernels, not recorded into a batch —
// a slot costs the queue nothing: block 0 of the slot's first launch writes the device's constant-rate clock to a word on entry
// (ivx_stage_stamp), block 0 of the first launch enqueued BEHIND the slot writes the closing word, and the slot's time is the distance of
// the two: start to start, the launch boundary behind the slot included. Adjacent timed slots share the word between them. The closing word
// of a call's last slot goes to whatever stamping launch this grid makes next — the next call's first kernel, or k_step_gather (a launch
// of another object enqueued in between, the bench's k_free_step, falls into that boundary). The gather copies the words to host-mapped
// memory ahead of the doorbell and zeroes them. Every other call keeps two event records per slot, 2-3 us each on the queue — which is
// what the 6 us boundaries on either side of a timed k_step_emit were (profiles/stage_stamps) —, and IVX_STAGE_TIMING_EVENTS=1 (read once)
// forces that path everywhere. One call never mixes the two clocks. ivx_grid_set_stage_timing(g, 0) turns timing off.
static const bool g_stage_timing_events = [] {
    const char* e = getenv("IVX_STAGE_TIMING_EVENTS");
    return e && atoi(e) == 1;
}();
static int ensure_stage_events(ivx_grid* g) {
    if (g->ev_ready) return IVX_OK;
    for (int i = 0; i < 2 * IVX_N_TIMED_STAGES; ++i) IVX_HIP_CHECK(hipEventCreate(&g->ev[i]));
    g->ev_ready = 1;
    return IVX_OK;
}
static int ensure_stage_ticks(ivx_grid* g) {
    if (g->tick_dev && g->tick_host) return IVX_OK;
    if (!g->tick_dev) {
        IVX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&g->tick_dev), IVX_TICK_WORDS * sizeof(unsigned long long)));
        IVX_HIP_CHECK(hipMemset(g->tick_dev, 0, IVX_TICK_WORDS * sizeof(unsigned long long)));
    }
    if (!g->tick_host) {
        IVX_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&g->tick_host), IVX_TICK_WORDS * sizeof(unsigned long long), hipHostMallocMapped));
        memset(g->tick_host, 0, IVX_TICK_WORDS * sizeof(unsigned long long));
        IVX_HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&g->tick_host_dev), g->tick_host, 0));
    }
    return IVX_OK;
}
static int ensure_pairs(ivx_grid* g);
// `slab_nbr_ids` / `slab_record`: the slab protocol's remesh phase (ivx_slab_remesh_enqueue) — the pass over the neighbour's face ids and the
// slab's record ride in the phase's own launches instead of taking two more
// `part` (slab protocol, ivx_voxel_step_enqueue_part): bit 0 = the call's sample and derive sweeps, bit 1 = everything behind them; the two
// halves of ONE call enqueued apart, so that the slab's face planes can be packed and sent between them.
static int step_enqueue(ivx_grid* g, uint32_t stages, const uint16_t* slab_nbr_ids, void* slab_record, uint32_t part = 3u) {
    IVX_REQUIRE(g, IVX_ERR_INVALID, "ivx_voxel_step_enqueue: null grid");
    const bool front = (part & 1u) != 0u, back = (part & 2u) != 0u;
    ivx_many_other_context other_(g->ctx);
    IVX_REQUIRE(!(stages & IVX_STAGE_SAMPLE) || g->prog_n > 0, IVX_ERR_STATE, "ivx_voxel_step: no SDF program resident (ivx_grid_set_sdf_program)");
    IVX_REQUIRE(!(stages & IVX_STAGE_INERTIA) || g->has_dens, IVX_ERR_STATE, "ivx_voxel_step: no densities resident (ivx_grid_set_densities)");
    hipStream_t s = g->ctx->stream;
    g->ahead_unordered_ok = g->pending_stages == 0;  // (sample-ahead: whatever was enqueued before has been collected)
    // stages enqueued after a record change the step's results: the block the record role wrote is stale (this call sets the flag again
    // further down when it carries the slab record itself)
    g->results_in_block = 0;
    if (!g->result_host) {
        IVX_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&g->result_host), 64 * sizeof(uint32_t), hipHostMallocMapped));
        memset(g->result_host, 0, 64 * sizeof(uint32_t));
        IVX_HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&g->result_host_dev), g->result_host, 0));
    }
    int rc;
    if (stages & IVX_STAGE_SAMPLE)
        if ((rc = ivx_sampler_buffers(g))) return rc;
    // Scratch word groups the stages of this call start from. They are preset by the call's first kernel (k_sdf_super or
    // k_chunk_pre host that role); a call that starts with neither gets a preset launch of its own. Only the requested stages'
    // groups are touched: a phase of the multi-GPU protocol must not wipe what an earlier phase of the same step left.
    uint32_t preset_in_sample = 0, preset_in_derive = 0;
    if (front) {  // (the second half of a call enqueued in two parts finds its groups preset by the first half's kernels)
        uint32_t need = 0;
        if (stages & IVX_STAGE_SAMPLE) need |= IVX_SCRATCH_EVAL;
        if (stages & IVX_STAGE_REGIONS) need |= IVX_SCRATCH_REGIONS;
        if (stages & IVX_STAGE_REMESH) need |= IVX_SCRATCH_SN;
        // (ivx_step_preset_ahead: groups of the NEXT call, preset by this call's first kernel so that a call without one of its own — the
        // remesh phase of the slab protocol — needs no preset launch)
        const uint32_t fresh = g->preset_fresh;
        g->preset_fresh = 0;
        uint32_t ahead = 0;
        if (stages & (IVX_STAGE_SAMPLE | IVX_STAGE_DERIVE)) {
            ahead = g->preset_ahead & ~need;
            g->preset_ahead = 0;
        }
        if (stages & IVX_STAGE_SAMPLE) preset_in_sample = need | ahead;
        else if (stages & IVX_STAGE_DERIVE) preset_in_derive = need | ahead;
        else if ((rc = ivx_launch_step_preset(g, need & ~fresh))) return rc;
        g->preset_fresh = ahead;
    }
    // derive runs the chunk-local region labelling and the chunk moments in the same sweep when those stages are part of this call
    const uint32_t fused_parts = (stages & IVX_STAGE_DERIVE) ? (((stages & IVX_STAGE_REGIONS) ? IVX_PART_REGIONS : 0u) |
                                                                 ((stages & IVX_STAGE_INERTIA) ? IVX_PART_MOMENTS : 0u))
                                                              : 0u;
    const uint32_t post = back ? stages & (IVX_STAGE_OCCUPIED | IVX_STAGE_REGIONS | IVX_STAGE_REMESH | IVX_STAGE_INERTIA) : 0u;
    // (a call without the derive stage: stand-alone per-chunk kernels, which carry no stamp, run ahead of k_step_post1)
    const bool standalone_first = ((post & IVX_STAGE_REGIONS) && !(fused_parts & IVX_PART_REGIONS) && !g->regions_labelled_locally) ||
                                  ((post & IVX_STAGE_INERTIA) && !(fused_parts & IVX_PART_MOMENTS));
    const uint32_t timing = ~g->stage_timing_off;  // timed slots
    // stamps or events, for the whole call (see above); a call takes at most a word per slot and one more
    const bool stamps = timing != 0u && !g_stage_timing_events && !g->stage_events_only && part == 3u && !slab_record && ivx_step_assign_fits(g) && !standalone_first &&
                        !ivx_many_recording() && g->tick_used + IVX_N_TIMED_STAGES + 1u <= IVX_TICK_WORDS;
    if (stamps && (rc = ensure_stage_ticks(g))) return rc;
    if (timing != 0u && !stamps && (rc = ensure_stage_events(g))) return rc;
    // events: a slot's duration runs from the stop event of the slot enqueued just before it, when there is one
    hipEvent_t* last_stop = nullptr;
    // stamps: the word the open slot starts at, and whether the slot armed it itself (else it is the closing word of the slot before, still pending)
    int slot_word = -1;
    bool slot_fresh = false;
#define T0(i)                                                                            \
    if (!((timing >> (i)) & 1u)) last_stop = nullptr;                                    \
    else if (stamps) {                                                                   \
        slot_fresh = g->tick_next == nullptr;                                            \
        if (slot_fresh) {                                                                \
            g->tick_host[g->tick_used] = 0ull;                                           \
            g->tick_next = g->tick_dev + g->tick_used++;                                 \
        }                                                                                \
        slot_word = (int)(g->tick_next - g->tick_dev);                                   \
    } else {                                                                             \
        if (last_stop) g->ev_start_ref[i] = last_stop;                                   \
        else {                                                                           \
            IVX_HIP_CHECK(ivx_event_record(g->ev[2 * (i)], s));                          \
            g->ev_start_ref[i] = &g->ev[2 * (i)];                                        \
        }                                                                                \
    }
    // (stamps: a word that nobody took means the slot launched nothing — it reports 0, and a word it armed itself is given back)
#define T1(i)                                                                            \
    if ((timing >> (i)) & 1u) {                                                          \
        if (stamps) {                                                                    \
            g->stamp_mask |= 1u << (i), g->timed_mask &= ~(1u << (i));                   \
            if (g->tick_next == g->tick_dev + slot_word) {                               \
                g->tick_start_ref[i] = g->tick_end_ref[i] = -1;                          \
                if (slot_fresh) g->tick_next = nullptr, --g->tick_used;                  \
            } else {                                                                     \
                g->tick_start_ref[i] = (int8_t)slot_word;                                \
                g->tick_end_ref[i] = (int8_t)g->tick_used;                               \
                g->tick_host[g->tick_used] = 0ull;                                       \
                g->tick_next = g->tick_dev + g->tick_used++;                             \
            }                                                                            \
        } else {                                                                         \
            IVX_HIP_CHECK(ivx_event_record(g->ev[2 * (i) + 1], s));                      \
            last_stop = &g->ev[2 * (i) + 1];                                             \
            g->timed_mask |= 1u << (i), g->stamp_mask &= ~(1u << (i));                   \
        }                                                                                \
    }
    if (front && (stages & IVX_STAGE_SAMPLE)) {
        T0(0);
        if ((rc = ivx_launch_sdf_sample(g, g->prog_nodes, g->prog_n, g->prog_stack, g->prog_shape, g->prog_center, g->prog_type, preset_in_sample, true,
                                        g->prog_noise != 0))) return rc;
        T1(0);
        g->eval_len_pending = 1;  // (the list lengths reach the result block once a derive sweep has rolled the counters over)
        g->occ_ref_valid = 0;
        g->bbox_valid = 0;
        g->mesh_valid = 0;
        g->mesh_built = 0;  // a newly sampled object: whatever mesh the buffers hold is not a stale version of this one
        g->regions_valid = 0;
    }
    if (front && (stages & IVX_STAGE_DERIVE)) {
        T0(1);
        if ((rc = ivx_launch_derive(g, fused_parts, preset_in_derive))) return rc;
        T1(1);
        if (g->eval_len_pending == 1) g->eval_len_pending = 2;
    }
    if (post) {
        // stages that were not swept inside k_derive get their stand-alone per-chunk kernels first (a call without the derive stage)
        if ((stages & IVX_STAGE_REGIONS) && !(fused_parts & IVX_PART_REGIONS)) {
            // (level 1 over the active list; the exact numbering of multi-region chunks leads k_step_post2 below, so
            // only the list-driven labelling kernel is launched here: ivx_launch_ccl_local would run both)
            if (!g->regions_labelled_locally && (rc = ivx_launch_ccl_local_only(g))) return rc;
        }
        if ((stages & IVX_STAGE_INERTIA) && !(fused_parts & IVX_PART_MOMENTS))
            if ((rc = ivx_launch_inertia_dense(g))) return rc;
        const bool fused_assign = ivx_step_assign_fits(g);
        T0(2);
        if ((rc = ivx_launch_step_post1(g, post))) return rc;
        T1(2);
        T0(3);
        if (slab_record) {
            if ((rc = ensure_pairs(g))) return rc;
            if (slab_nbr_ids && !g->pairs_zeroed) IVX_HIP_CHECK(ivx_memset_async(g->pairs_dev, 0, (4 + 128) * sizeof(uint32_t), s));
            g->pairs_zeroed = 0;
        }
        if ((rc = ivx_launch_step_post2(g, post, slab_nbr_ids))) return rc;
        T1(3);
        // no host round trip for the mesh sizes: the emit pass writes into the buffers of the previous step and skips what
        // does not fit; ivx_voxel_step_collect grows the buffers and repeats the pass in that (rare) case
        if (post & (IVX_STAGE_REGIONS | IVX_STAGE_REMESH)) {
            T0(4);
            if (fused_assign) {
                if ((rc = ivx_launch_step_emit(g, post, (post & IVX_STAGE_REGIONS) != 0, slab_record, slab_nbr_ids != nullptr))) return rc;
                if (slab_record) g->results_in_block = 1;
            } else {  // more than 524 288 chunks: the region resolve takes its stand-alone path
                if ((post & IVX_STAGE_REMESH) && (rc = ivx_launch_step_emit(g, IVX_STAGE_REMESH))) return rc;
                if ((post & IVX_STAGE_REGIONS) && (rc = ivx_launch_ccl_resolve(g))) return rc;
            }
            T1(4);
        }
        // (sample-ahead: the next sample stage's pre-pass goes behind the step's last big launch, beside the small ones that follow)
        if (!g->ahead_unordered_ok && (rc = ivx_sampler_launch_ahead(g, true))) return rc;
        if ((post & IVX_STAGE_REGIONS) && fused_assign) {
            T0(5);
            if ((rc = ivx_launch_step_assign(g, (post & IVX_STAGE_REMESH) != 0))) return rc;
            T1(5);
        }
        if (post & IVX_STAGE_REMESH) {
            g->mesh_valid = 0;
            g->scratch_dirty |= IVX_SCRATCH_SN;
        }
        if (post & IVX_STAGE_REGIONS) g->scratch_dirty |= IVX_SCRATCH_REGIONS;
    }
#undef T0
#undef T1
    if (back && (rc = ivx_sampler_launch_ahead(g, !g->ahead_unordered_ok))) return rc;  // (a call without the stages behind the derive sweep)
    g->pending_stages |= stages;
    return IVX_OK;
}

int ivx_voxel_step_enqueue(ivx_grid* g, uint32_t stages) { return step_enqueue(g, stages, nullptr, nullptr); }
// ... without event records around the stage slots, whatever ivx_grid_set_stage_timing has asked for: for callers whose stage times nobody reads,
// and for recorded steps — an event is a stream operation of its own and would end the merging after every object
extern "C++" int step_enqueue_untimed(ivx_grid* g, uint32_t stages) {
    const uint32_t keep = g->stage_timing_off;
    g->stage_timing_off = 0xFFFFFFFFu;
    const int rc = step_enqueue(g, stages, nullptr, nullptr);
    g->stage_timing_off = keep;
    return rc;
}
}  // extern "C"
// (slab_comm.cpp) one call's launches in two parts: 1 = its sample and derive sweeps, 2 = what follows them
int ivx_voxel_step_enqueue_part(ivx_grid* g, uint32_t stages, uint32_t part) { return step_enqueue(g, stages, nullptr, nullptr, part); }
extern "C" {

// The remesh phase of the slab protocol in the step's own launches: count | — then scan | the component pairs across the upper x face (from
// `neighbour_face_ids`, the ids behind the neighbour's face planes of the second exchange; null for the last slab) — then emit | the slab's
// record into `device_record` and the step's small results into the grid's host-mapped block — then the mesher's general pass. Four launches
// where face pairs, the remesh stage and the record took six; ivx_voxel_step_collect then has its results without a launch of its own (the
// caller waits for the stream first: the slab protocol's doorbell).
int ivx_slab_remesh_enqueue(ivx_grid* g, const void* neighbour_face_ids, void* device_record) {
    IVX_REQUIRE(g && device_record, IVX_ERR_INVALID, "ivx_slab_remesh_enqueue: null argument");
    if (!ivx_step_assign_fits(g)) {  // (grids beyond the fused launches' reach: the separate passes)
        int rc;
        if (neighbour_face_ids && (rc = ivx_region_face_pairs_enqueue(g, 1, neighbour_face_ids))) return rc;
        if ((rc = step_enqueue(g, IVX_STAGE_REMESH, nullptr, nullptr))) return rc;
        if ((rc = ivx_step_record_enqueue(g, device_record))) return rc;
        if (g->record_head_copy)
            IVX_HIP_CHECK(ivx_memcpy_async(g->record_head_copy, device_record, (size_t)g->record_head_words * 8, hipMemcpyDeviceToDevice, g->ctx->stream));
        return IVX_OK;
    }
    g->pairs_enqueued = 0;
    return step_enqueue(g, IVX_STAGE_REMESH, static_cast<const uint16_t*>(neighbour_face_ids), device_record);
}

// Sample-ahead: with `on`, every sample stage under the resident program also enqueues the NEXT sample stage's pre-pass — on the context's
// second stream, behind its own evaluator —, and the next sample stage starts at its evaluator. For callers that sample the same program
// step after step (the bench's headline step); the results are the same bytes either way. Off (the default): the pre-pass is the stage's
// first kernel. Turning it off drops a pre-pass that is under way.
int ivx_grid_set_sample_ahead(ivx_grid* g, int on) {
    IVX_REQUIRE(g, IVX_ERR_INVALID, "ivx_grid_set_sample_ahead: null grid");
    g->ahead_on = on ? 1 : 0;
    if (!on) return ivx_sampler_ahead_cancel(g);
    return IVX_OK;
}

int ivx_grid_set_stage_timing(ivx_grid* g, uint32_t slot_mask) {
    IVX_REQUIRE(g, IVX_ERR_INVALID, "ivx_grid_set_stage_timing: null grid");
    g->stage_timing_off = ~slot_mask;
    return IVX_OK;
}

// Developer aid: the raw clock stamps behind the last collected step's stage_ms, start then end per slot (0: the slot was not stamped — not
// timed, without a launch, or timed by events), and the clock's rate in kHz.
int ivx_debug_stage_ticks(ivx_grid* g, unsigned long long ticks[2 * IVX_N_TIMED_STAGES], double* clock_khz) {
    IVX_REQUIRE(g && ticks, IVX_ERR_INVALID, "ivx_debug_stage_ticks: null argument");
    memcpy(ticks, g->tick_last, sizeof(g->tick_last));
    if (clock_khz) *clock_khz = g->ctx->wall_clock_khz;
    return IVX_OK;
}

// How long ivx_voxel_step_collect polls the doorbell before it falls back to hipStreamSynchronize (IVX_COLLECT_SPIN_US, default 2000;
// 0 = never poll).
static uint64_t collect_spin_ns() {
    static const uint64_t ns = [] {
        const char* e = getenv("IVX_COLLECT_SPIN_US");
        const long us = e ? strtol(e, nullptr, 10) : 2000;
        return (uint64_t)(us < 0 ? 0 : us) * 1000ull;
    }();
    return ns;
}

// the launch half of ivx_voxel_step_collect: the gather of the step's results (and whatever rides on it) goes on the stream — or into the
// batch being recorded —, the wait is left to the collect
extern "C++" int ivx_step_collect_launch(ivx_grid* g) {
    if (g->results_in_block || g->gather_launched) return IVX_OK;
    if (!g->result_host) {
        IVX_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&g->result_host), 64 * sizeof(uint32_t), hipHostMallocMapped));
        memset(g->result_host, 0, 64 * sizeof(uint32_t));
        IVX_HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&g->result_host_dev), g->result_host, 0));
    }
    g->gather_flush_id = ivx_many_flush_count();
    const int rc = ivx_launch_step_gather(g);
    if (!rc) g->gather_launched = 1;
    return rc;
}

int ivx_voxel_step_collect(ivx_grid* g, ivx_step_result* out) {
    IVX_REQUIRE(g && out, IVX_ERR_INVALID, "ivx_voxel_step_collect: null argument");
    ivx_many_other_context other_(g->ctx);
    hipStream_t s = g->ctx->stream;
    memset(out, 0, sizeof(*out));
    const uint32_t stages = g->pending_stages;
    // the small results of every stage (region scalars + occupied minima/maxima, mesh totals, moments) arrive in one
    // host-mapped block written by a last tiny kernel: one wait, no copies
    if (!g->result_host) {
        IVX_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&g->result_host), 64 * sizeof(uint32_t), hipHostMallocMapped));
        memset(g->result_host, 0, 64 * sizeof(uint32_t));
        IVX_HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&g->result_host_dev), g->result_host, 0));
    }
    const bool have_results = g->results_in_block != 0;  // (ivx_slab_remesh_enqueue: the block is written, the caller has waited for the stream)
    g->results_in_block = 0;
    if (!have_results) {
        if (!g->gather_launched) {  // (else ivx_step_collect_launch has put it on the stream: the many-object calls launch all objects' gathers as one)
            int rc = ivx_launch_step_gather(g);
            if (rc) return rc;
            (void)ivx_many_break();
        }
        // (a gather that was only recorded has to be on the stream before anybody polls its doorbell: flushed now unless a flush has gone by since)
        if (g->gather_launched && ivx_many_recording() && g->gather_flush_id == ivx_many_flush_count()) (void)ivx_many_break();
        g->gather_launched = 0;
    } else if (hipStreamQuery(s) != hipSuccess) {
        IVX_HIP_CHECK(ivx_stream_sync(s));
    }
    // A short step is over before the runtime's blocking wait has gone to sleep and been woken again: poll the doorbell word the
    // gather kernel writes last (in-order stream: everything enqueued before it is complete too) for a bounded time first.
    if (!have_results) {
        const volatile uint32_t* bell = g->result_host + 63;
        const uint32_t want = g->result_seq;
        const uint64_t budget_ns = collect_spin_ns();
        bool rung = false;
        if (budget_ns) {
            const auto t0 = std::chrono::steady_clock::now();
            for (uint32_t it = 0;; ++it) {
                if (*bell == want) {
                    rung = true;
                    break;
                }
                __builtin_ia32_pause();
                if ((it & 255u) == 255u && (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count() > budget_ns) break;
            }
            std::atomic_thread_fence(std::memory_order_acquire);
        }
        if (!rung) {
            IVX_HIP_CHECK(ivx_stream_sync(s));
            // the stream is empty and the doorbell has not rung: the gather never reached the stream (a flush of recorded launches failed and
            // dropped it, many.hpp) — what the block holds is an earlier step's
            std::atomic_thread_fence(std::memory_order_acquire);
            if (*bell != want) {
                const int dropped = ivx_many_error(g->ctx, true);
                g->pending_stages = 0;
                ivx_set_error("ivx_voxel_step_collect: the step's results never arrived (%s)", dropped ? "a flush of recorded launches failed" : "the gather did not run");
                return IVX_ERR_HIP;
            }
        }
    }
    if (have_results && g->stamp_mask && g->tick_dev) {
        // (stamped slots of a step that ended in ivx_step_record_enqueue instead of the gather — the slab protocol driven from outside the
        // library: the stream has been waited for, the words are fetched and cleared here)
        IVX_HIP_CHECK(ivx_memcpy_sync(g->tick_host, g->tick_dev, IVX_TICK_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        IVX_HIP_CHECK(hipMemset(g->tick_dev, 0, IVX_TICK_WORDS * sizeof(unsigned long long)));
    }
    const uint32_t* sc = g->result_host;
    if (sc[31]) g->last_active = sc[31];
    if (g->eval_len_pending == 2 && g->samp_len) {  // a sample stage and a derive sweep behind it have run under the resident program
        for (int c = 0; c < 3; ++c) g->eval_len[c] = sc[52 + c];
        g->eval_len_valid = 1;
    }
    g->eval_len_pending = 0;
    if (stages & IVX_STAGE_REGIONS) {
        IVX_REQUIRE((sc[1] & 1u) == 0, IVX_ERR_CAPACITY, "ivx_voxel_step: a chunk has more than 254 local regions");
        IVX_REQUIRE((sc[1] & 8u) == 0, IVX_ERR_HIP, "ivx_voxel_step: the region merge gave up waiting for the numbering of the multi-region chunks (k_step_post2)");
        g->region_count = sc[0];
        g->regions_valid = 1;
        out->region_count = sc[0];
    }
    if (stages & IVX_STAGE_OCCUPIED) {
        ivx_occupied_from_raw(g, sc + 16, out->occupied);
        memcpy(g->occ_ref, out->occupied, sizeof(g->occ_ref));
        g->occ_ref_valid = 1;
    }
    if (stages & IVX_STAGE_REMESH) {
        const uint32_t totals[3] = {sc[28], sc[29], sc[30]};
        const bool outgrown = totals[0] > g->vcap || totals[1] > g->icap || totals[2] > g->scap;
        // (ivx_voxel_step_many: the buffers of all objects that outgrew theirs from one allocation, their emit passes as one launch)
        g->mesh_growth_pending = outgrown && g->defer_mesh_growth ? 1 : 0;
        if (outgrown && !g->mesh_growth_pending) {
            int rc;
            if ((rc = ensure_mesh_capacity(g, totals[0], totals[1], totals[2]))) return rc;
            if ((rc = ivx_launch_sn_emit(g))) return rc;
            IVX_HIP_CHECK(ivx_stream_sync(s));
        }
        if (g->mesh_growth_pending) mesh_set_counts(g, totals);  // (valid, built and serial wait for the emit that ivx_voxel_step_many runs again)
        else mesh_adopt_full(g, totals);
    }
    if (stages & IVX_STAGE_INERTIA) {
        memcpy(out->moments.m64, sc + 32, 10 * sizeof(double));
        for (int i = 0; i < 10; ++i) out->moments.m32[i] = (float)out->moments.m64[i];
    }
    out->mesh = g->mesh_counts;
    for (int i = 0; i < IVX_N_TIMED_STAGES; ++i) {
        float ms = 0.0f;
        g->tick_last[2 * i] = g->tick_last[2 * i + 1] = 0ull;
        if ((g->stamp_mask >> i) & 1u) {  // clock stamps (step_enqueue): start to start, in ticks of the device's constant-rate clock
            if (g->tick_start_ref[i] >= 0 && g->tick_end_ref[i] >= 0) {
                const unsigned long long t0 = g->tick_host[g->tick_start_ref[i]], t1 = g->tick_host[g->tick_end_ref[i]];
                g->tick_last[2 * i] = t0, g->tick_last[2 * i + 1] = t1;
                if (t0 != 0ull && t1 > t0) ms = (float)((double)(t1 - t0) / g->ctx->wall_clock_khz);
            }
        } else if ((g->timed_mask >> i) & 1u) {
            if (hipEventElapsedTime(&ms, *g->ev_start_ref[i], g->ev[2 * i + 1]) != hipSuccess) ms = 0.0f;
        }
        out->stage_ms[i] = ms;
    }
    g->pending_stages = 0;
    g->timed_mask = 0;
    g->stamp_mask = 0;
    g->tick_used = 0;
    g->tick_next = nullptr;
    return IVX_OK;
}

int ivx_voxel_step(ivx_grid* g, uint32_t stages, ivx_step_result* out) {
    IVX_REQUIRE(g && out, IVX_ERR_INVALID, "ivx_voxel_step: null argument");
    int rc = ivx_voxel_step_enqueue(g, stages);
    if (rc) return rc;
    return ivx_voxel_step_collect(g, out);
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

static int ensure_pairs(ivx_grid* g) {
    if (g->pairs_dev) return IVX_OK;
    IVX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&g->pairs_dev), sizeof(uint32_t) * (4 + 128 + 2 * (size_t)IVX_MAX_FACE_PAIRS)));
    IVX_HIP_CHECK(ivx_memset_async(g->pairs_dev, 0, sizeof(uint32_t) * (4 + 128), g->ctx->stream));
    return IVX_OK;
}

int ivx_region_face_pairs_enqueue(ivx_grid* g, int side, const void* neighbour_face_labels) {
    IVX_REQUIRE(g && neighbour_face_labels && (side == 0 || side == 1), IVX_ERR_INVALID, "ivx_region_face_pairs_enqueue: bad argument");
    int rc = ensure_pairs(g);
    if (rc) return rc;
    rc = ivx_launch_face_pairs(g, side, static_cast<const uint16_t*>(neighbour_face_labels), g->pairs_dev, g->pairs_dev + 4 + 128, IVX_MAX_FACE_PAIRS,
                               g->pairs_dev + 4);
    if (rc) return rc;
    g->pairs_enqueued = 1;
    return IVX_OK;
}

size_t ivx_step_record_words(void) { return 28 + 2 * (size_t)IVX_MAX_FACE_PAIRS; }

int ivx_step_record_enqueue(ivx_grid* g, void* device_record) {
    IVX_REQUIRE(g && device_record, IVX_ERR_INVALID, "ivx_step_record_enqueue: null argument");
    int rc = ensure_pairs(g);
    if (rc) return rc;
    // (no face-pair pass since the last record: the record lists none — a null count, not a fill of the counter)
    rc = ivx_launch_step_record(g, g->pairs_enqueued ? g->pairs_dev : nullptr, g->pairs_dev + 4 + 128, IVX_MAX_FACE_PAIRS, device_record, g->result_host_dev != nullptr);
    if (!rc && g->result_host_dev) g->results_in_block = 1;
    g->pairs_enqueued = 0;
    return rc;
}

// ---- many objects per call (many.hpp) ---------------------------------------------------------------------------------------------------
// The per-object host code runs object after object while the launches are recorded; one flush issues a launch per chain position for all of
// them; the results come back through every object's own host-mapped block, their gathers launched as one.
int ivx_many_begin(ivx_ctx* c);
int ivx_many_flush(ivx_ctx* c);
extern "C++" int many_check(ivx_grid* const* grids, size_t n, const char* who) {
    IVX_REQUIRE(grids && grids[0], IVX_ERR_INVALID, "%s: null object list", who);
    static thread_local std::vector<const ivx_grid*> seen;  // (a thousand objects a call: no quadratic search for the duplicate)
    seen.assign(grids, grids + n);
    std::sort(seen.begin(), seen.end());
    for (size_t i = 0; i < n; ++i) {
        IVX_REQUIRE(grids[i] && grids[i]->ctx == grids[0]->ctx, IVX_ERR_INVALID, "%s: object %zu is null or belongs to another context", who, i);
        IVX_REQUIRE(i == 0 || seen[i] != seen[i - 1], IVX_ERR_INVALID, "%s: an object is listed twice", who);
    }
    return IVX_OK;
}
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
        if (g->edit && g->edit->pending) {
            ivx_absorb_result tmp;
            (void)absorb_collect(g, "ivx_*_many (drain)", &tmp, nullptr, nullptr);
        }
        mesh_sync_abandon(g);
        if (g->pending_stages || g->gather_launched) {
            ivx_step_result tmp;
            (void)ivx_voxel_step_collect(g, &tmp);
        }
        if (g->edit) g->edit->pending = 0;
        g->pending_stages = 0;
        g->gather_launched = 0;
        g->results_in_block = 0;
        g->defer_mesh_growth = 0;
        if (g->mesh_growth_pending) g->mesh_growth_pending = 0, g->mesh_valid = 0;
    }
    ivx_set_error("%s", keep);
    return rc;
}
// runs `f(i)` for every object under the recorder and flushes; the first error ends the batch (what was recorded still goes out; the caller
// drains: many_fail)
extern "C++" int many_phase(ivx_grid* const* grids, size_t n, const std::function<int(size_t)>& f) {
    ivx_ctx* c = grids[0]->ctx;
    int rc = ivx_many_begin(c);
    if (rc) return rc;
    int first = IVX_OK;
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t i = 0; i < n && !first; ++i) {
        ivx_many_object((uint32_t)i);
        first = f(i);
    }
    const auto t1 = std::chrono::steady_clock::now();
    rc = ivx_many_flush(c);
    static const bool trace_phase_ = getenv("IVX_MANY_TRACE") != nullptr;
    if (trace_phase_)
        fprintf(stderr, "[ivx many]   phase: objects %.1f us, flush %.1f us\n", 1e-3 * (double)std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count(),
                1e-3 * (double)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t1).count());
    return first ? first : rc;
}

int ivx_voxel_step_many(ivx_grid* const* grids, size_t n, uint32_t stages, ivx_step_result* out) {
    if (n == 0) return IVX_OK;  // (a manager without voxel objects)
    int rc = many_check(grids, n, "ivx_voxel_step_many");
    if (rc) return rc;
    IVX_REQUIRE(out, IVX_ERR_INVALID, "ivx_voxel_step_many: null result array");
    // (`stage_ms` of a merged step is zero — the launches are shared, their times are not an object's)
    if ((rc = many_phase(grids, n, [&](size_t i) { return step_enqueue_untimed(grids[i], stages); }))) return many_fail(grids, n, rc);
    if ((rc = many_phase(grids, n, [&](size_t i) { return ivx_step_collect_launch(grids[i]); }))) return many_fail(grids, n, rc);
    for (size_t i = 0; i < n; ++i) {
        grids[i]->defer_mesh_growth = 1;
        rc = ivx_voxel_step_collect(grids[i], &out[i]);
        grids[i]->defer_mesh_growth = 0;
        if (rc) return many_fail(grids, n, rc);
    }
    // Objects whose meshes outgrew their buffers (all of them, when the fragments of an impact are stepped for the first time): the new buffers
    // of all from ONE allocation at twice what each needs (docs/voxel_gpu_buffer_pooling.md:44-66), their emit passes again as one launch
    // each, one wait — where the single-object collect pays six allocations, a launch and a wait per object.
    static thread_local std::vector<ivx_grid*> grow;
    static thread_local std::vector<size_t> caps;
    grow.clear(), caps.clear();
    for (size_t i = 0; i < n; ++i)
        if (grids[i]->mesh_growth_pending) grow.push_back(grids[i]);
    if (!grow.empty()) {
        const size_t m = grow.size();
        caps.resize(3 * m);
        for (size_t k = 0; k < m; ++k) {
            const ivx_mesh_counts& mc = grow[k]->mesh_counts;
            const size_t need[3] = {mc.n_vertices, mc.n_indices, mc.n_submeshes}, have[3] = {grow[k]->vcap, grow[k]->icap, grow[k]->scap};
            mesh_grown_capacities(need, have, false, &caps[3 * k]);
        }
        if ((rc = mesh_pool_assign(grow.data(), m, caps.data()))) return many_fail(grids, n, rc);
        if ((rc = many_phase(grow.data(), m, [&](size_t k) -> int {
                 ivx_grid* g = grow[k];
                 if (!ivx_many_zero(g->ctx, g, ivx_sn_hard_count(g), IVX_SN_TAIL_WORDS * sizeof(uint32_t)))
                     IVX_HIP_CHECK(ivx_memset_async(ivx_sn_hard_count(g), 0, IVX_SN_TAIL_WORDS * sizeof(uint32_t), g->ctx->stream));
                 int r = ivx_launch_step_emit(g, IVX_STAGE_REMESH, true, nullptr, false);
                 if (r) return r;
                 return ivx_launch_step_assign(g, true, false);
             })))
            return many_fail(grids, n, rc);
        IVX_HIP_CHECK(ivx_stream_sync(grids[0]->ctx->stream));
        for (ivx_grid* g : grow) {
            const uint32_t totals[3] = {g->mesh_counts.n_vertices, g->mesh_counts.n_indices, g->mesh_counts.n_submeshes};
            g->mesh_growth_pending = 0;
            mesh_adopt_full(g, totals);
        }
    }
    return IVX_OK;
}

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
        if (!e->d_results) {
            const size_t cap = 1 << 16;
            IVX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&e->d_results), cap));
            IVX_HIP_CHECK(ivx_memset_async(e->d_results, 0, cap, grids[i]->ctx->stream));
            e->d_results_bytes = cap;
        }
        if (!e->pinned) {
            const size_t cap = 1 << 16;
            IVX_HIP_CHECK(hipHostMalloc(&e->pinned, cap, hipHostMallocMapped));
            IVX_HIP_CHECK(hipHostGetDevicePointer(&e->pinned_dev, e->pinned, 0));
            e->pinned_bytes = cap;
        }
    }
    clk.lap("prepare");
    if ((rc = many_phase(grids, n, [&](size_t i) {
             return absorb_enqueue(grids[i], who, segments3 ? 1 : 0, points3 + 3 * i, segments3 ? segments3 + 3 * i : nullptr, influence_radii[i], shape_radii[i], densities);
         })))
        return many_fail(grids, n, rc);
    clk.lap("enqueue + flush");
    if ((rc = many_phase(grids, n, [&](size_t i) { return (grids[i]->edit && grids[i]->edit->pending && !grids[i]->edit->nothing) ? ivx_step_collect_launch(grids[i]) : IVX_OK; })))
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

int ivx_halo_clear(ivx_grid* g, int side) {
    IVX_REQUIRE(g && (side == 0 || side == 1), IVX_ERR_INVALID, "ivx_halo_clear: bad argument");
    g->has_ghost[side] = 0;
    g->ghost_ext[side] = nullptr;
    return IVX_OK;
}

}  // extern "C"
