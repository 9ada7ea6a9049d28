/* impact_voxel_hip.h — C ABI of libimpact_voxel_hip.so
 *
 * MI355X (gfx950) implementation of the per-frame deformable-voxel physics step of
 * lars-frogner/Impact, exposed as a flat C ABI so that the reference's own Rust loader
 * `define_lib!` (interop/dynamic_lib/src/macros.rs:17-183) can bind it: FFI-primitive arguments
 * only, complex data as caller-allocated (ptr, len) buffers in the little-endian layouts documented
 * here, no heap ownership crosses the boundary, errors are status codes (0 = ok) with a message
 * available from ivx_last_error(). See INTEGRATION.md for the Rust-side binding.
 *
 * Every entry point cites the reference interface it stands in for (paths relative to
 * engine/crates/). There is NO CPU fallback: every compute entry point runs HIP kernels and fails
 * with IVX_ERR_HIP if no gfx950 device is usable.
 *
 * Device data layout ("dense chunk-tiled SoA"): the object's chunk grid (cx,cy,cz) is stored
 * completely (void and uniform chunks included); chunk c = (ci*cy + cj)*cz + ck owns 4096 bytes in
 * each plane at offset c*4096, voxel (i,j,k) at (i<<8)|(j<<4)|k — the reference's own chunk and
 * voxel index math (impact_voxel/src/object.rs:3140-3199). Planes: sdf (i8 quantised signed
 * distance, impact_voxel/src/lib.rs:154-222), type (u8 VoxelType), flags (u8 VoxelFlags,
 * lib.rs:75-101), local region label (u8, object/split_detection.rs:125,154).
 */
#ifndef IMPACT_VOXEL_HIP_H
#define IMPACT_VOXEL_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define IVX_OK 0
#define IVX_ERR_INVALID 1   /* bad argument / shape mismatch */
#define IVX_ERR_HIP 2       /* HIP runtime error or no usable device */
#define IVX_ERR_CAPACITY 3  /* caller buffer too small / internal limit exceeded */
#define IVX_ERR_STATE 4     /* call order violated (e.g. mesh download before remesh) */

typedef struct ivx_ctx ivx_ctx;
typedef struct ivx_grid ivx_grid;

/* SDFNode — impact_voxel/src/generation/sdf/atomic.rs:62-181. 32 bytes.
 * kind: 0 sphere{p0=radius} 1 capsule{p0=segment_length,p1=radius} 2 box{p0..2=extents}
 *       3 translation{child1,p0..2} 4 rotation{child1,p=quat xyzw} 5 scaling{child1,p0}
 *       6 multifractal noise{child1, child2=octaves, pad=seed, p=frequency,lacunarity,persistence,amplitude}
 *       7 union 8 subtraction 9 intersection {child1,child2,p0=smoothness}
 * Kind 6 (MultifractalNoiseSDFModifier, atomic.rs:165-181,1363-1571) follows the reference in its semantics, domains, margins,
 * noise positions and per-block early-out, but its noise is this library's own (impact_amd/csrc/noise.hpp: Gustavson simplex
 * noise summed over octaves, the construction of the reference's `simdnoise`, not simdnoise's values). */
typedef struct {
    uint32_t kind, child1, child2, pad;
    float p[4];
} ivx_sdf_node;

/* ProcessedSDFNode — atomic.rs:83-102 (+ constructor-derived parameters). 128 bytes. */
typedef struct {
    uint32_t kind, leaf_count;
    float transform[16]; /* column-major root->node space */
    float domain_lo[3], domain_hi[3]; /* domain_with_margin */
    float margin;
    float a, b, c; /* sphere a=r | capsule a=half_segment b=r | box half extents | scaling a=s | binary a=smoothness b=0.25/a
                      | noise a=noise_scale b=frequency c=lacunarity */
    uint32_t reserved[4]; /* noise: [0] persistence (f32 bits), [1] octaves, [2] seed */
} ivx_sdf_processed_node;

/* Per-chunk state (VoxelChunk / NonUniformVoxelChunk, object.rs:95-126,163-188; split_detection.rs:82-88). 8 bytes. */
typedef struct {
    uint8_t kind;      /* 0 void, 1 uniform, 2 non-uniform — after ivx_derive_state */
    uint8_t gen_kind;  /* kind right after generation/upload (object.rs:1890-1964) */
    uint8_t flags;     /* VoxelChunkFlags bits 0-5 IS_OBSCURED_{X,Y,Z}_DN,{X,Y,Z}_UP, bit 6 HAS_ONLY_EMPTY_VOXELS; 0 for void/uniform */
    uint8_t uniform_type;
    uint16_t face_dist; /* FaceVoxelDistribution, 2 bits per face at bit 2*(2*dim+side): 0 empty 1 full 2 mixed */
    uint8_t region_count, boundary_region_count; /* after ivx_label_regions. Inside a step, from the derive sweep to the exact numbering
                                                    (k_step_post2), a chunk on the multi-region list holds a provisional 2 / 0: what runs
                                                    between the two may test region_count against 0 and 1 only */
} ivx_chunk_info;

/* ChunkSubmesh (impact_voxel/src/mesh.rs:94-103) + the chunk's vertex range (mesh.rs:145). 64 bytes. */
typedef struct {
    uint32_t chunk_indices[3];
    uint32_t index_offset, index_count;
    uint32_t is_obscured_from_direction[2][2][2];
    uint32_t vertex_offset, vertex_count, reserved;
} ivx_submesh;

typedef struct {
    uint32_t n_vertices, n_indices, n_submeshes, reserved;
} ivx_mesh_counts;

/* VoxelObjectInertialPropertyManager (impact_voxel/src/object/inertia.rs:20-25): mass, first moments,
 * moments of inertia (xx,yy,zz), products (xy,yz,zx) about the grid origin. f64 is what the kernels
 * accumulate in; f32 is the value rounded for the reference's struct. */
typedef struct {
    double m64[10];
    float m32[10];
    uint32_t reserved[2];
} ivx_moments;

/* One connected region of the object (result of VoxelObject::count_regions /
 * find_two_disconnected_regions, object/split_detection.rs:193-301, plus what
 * extract_disconnected_region needs to pick and size a fragment, object/extraction.rs:121-295). */
typedef struct {
    uint32_t root_chunk, root_region; /* GlobalRegionLabel of the representative local region */
    uint64_t voxel_count;
    uint32_t lo[3], hi[3]; /* occupied voxel range [lo, hi) */
    uint32_t non_uniform_chunk_count, chunk_count;
    double moments[10];
} ivx_region_desc;

/* ---- context ------------------------------------------------------------------------------- */
/* One context per process and GPU (the engine holds the voxel / rigid-body managers behind one
 * write lock per stage, engine/src/tasks.rs:394-395,1040,1047 — calls on a ctx are serialised by
 * the caller). `stream` may be NULL (library-owned stream) or a hipStream_t to run on. */
int ivx_init(int device_id, void* stream, ivx_ctx** out);
void ivx_shutdown(ivx_ctx*);
const char* ivx_last_error(void); /* thread-local, library-owned string */
int ivx_synchronize(ivx_ctx*);
void* ivx_stream(ivx_ctx*); /* the hipStream_t kernels are launched on */

/* ---- grid (VoxelObject storage, object.rs:45-57) ---------------------------------------------- */
/* chunk_counts = ceil(grid_shape/16) (object.rs:321). x_chunk_offset / global_x_chunks describe an
 * x-slab of a larger grid for domain decomposition (0 and cx for a whole object). */
int ivx_grid_create(ivx_ctx*, const uint32_t chunk_counts[3], float voxel_extent, uint32_t x_chunk_offset,
                    uint32_t global_x_chunks, ivx_grid** out);
void ivx_grid_destroy(ivx_grid*);
/* dense chunk-tiled host planes -> device + classification of every chunk as the generator would
 * (generation.rs:336-355, object.rs:1890-1964). Replaces VoxelObject::generate_without_derived_state
 * for callers that bring their own voxels (ChunkedVoxelGenerator, generation.rs:41-67). */
int ivx_grid_upload_dense(ivx_grid*, const int8_t* sdf, const uint8_t* type, size_t n_voxels);
/* device -> host; any pointer may be NULL */
int ivx_grid_download_dense(ivx_grid*, int8_t* sdf, uint8_t* type, uint8_t* flags, uint8_t* local_labels, ivx_chunk_info* info,
                            size_t n_voxels);
int ivx_grid_chunk_counts(ivx_grid*, uint32_t out[3]);
/* diagnostics of the last step: chunks the sampler evaluated per voxel, chunks with several local regions, chunks that
 * emitted a mesh, total chunks */
int ivx_grid_stage_counters(ivx_grid*, uint32_t out[4]);
/* device pointers of the planes: 0 sdf, 1 type, 2 flags, 3 local labels, 4 chunk info, 5 global region parents. Between
 * steps the planes of Void / Uniform chunks are not kept up to date (such a chunk is its 8-byte record, as in the
 * reference's store, object.rs:96-119); asking for a plane pointer (0-3) enqueues the kernel that writes them out. */
void* ivx_grid_device_ptr(ivx_grid*, int which);

/* ---- a3: SDF sample ----------------------------------------------------------------------------- */
/* SDFGenerator::new_in (atomic.rs:228-596): host-side graph compile, no GPU work. */
int ivx_sdf_compile(const ivx_sdf_node* nodes, size_t n_nodes, uint32_t root, ivx_sdf_processed_node* out, size_t cap,
                    size_t* n_out, float domain[6], uint32_t* stack_size);
/* SDFVoxelGenerator::new (generation.rs:207-258): grid shape and shifted grid centre from the domain */
int ivx_sdf_grid_shape(const float domain[6], uint32_t grid_shape[3], float shifted_grid_center[3]);
/* VoxelObject::generate_without_derived_state with an SDFVoxelGenerator + SameVoxelTypeGenerator
 * (object.rs:267-404, generation.rs:293-371, atomic.rs:633-875). grid_shape is the GLOBAL shape. */
int ivx_sdf_sample(ivx_grid*, const ivx_sdf_processed_node* nodes, size_t n_nodes, uint32_t stack_size,
                   const uint32_t grid_shape[3], const float shifted_grid_center[3], uint8_t voxel_type);

/* ---- a4: derived state -------------------------------------------------------------------------- */
/* VoxelObject::compute_all_derived_state minus region labelling (object.rs:1136-1145): voxel adjacency
 * flags, face distributions, chunk obscuredness, uniform-chunk demotion. */
int ivx_derive_state(ivx_grid*);
/* VoxelObject::update_occupied_ranges (object.rs:1149-1198): out = chunk lo/hi x3, voxel lo/hi x3. Needs ivx_derive_state first (the ranges are reduced
 * from per-chunk boxes the derive sweep leaves). The object keeps these ranges the way the reference does: the edit, contact and probe entry points
 * use them as they were at the last update — an edit refreshes them only when it removed a chunk, split and clip always do. */
int ivx_occupied_ranges(ivx_grid*, uint32_t out[12]);

/* ---- a5-a7: remesh ------------------------------------------------------------------------------ */
/* VoxelObjectMesh::recreate (mesh.rs:286-354): padded chunk SDF + Surface Nets for every exposed chunk,
 * concatenated in chunk-linear order. Results stay on the device until downloaded. */
int ivx_remesh(ivx_grid*, ivx_mesh_counts* out);
/* positions/normals: 3 f32 per vertex; indices u32; index_materials 8 u8 per index
 * (VoxelMeshIndexMaterials, mesh.rs:77-82); any pointer may be NULL */
int ivx_mesh_download(ivx_grid*, float* positions, float* normals, uint32_t* indices, uint8_t* index_materials,
                      ivx_submesh* submeshes);
/* VoxelObjectMesh::sync_with_voxel_object (mesh.rs:355-456): re-mesh only the chunks marked in `invalidated_chunks` (one byte per chunk, e.g. what
 * ivx_absorb_* reported), placing their data through the ChunkSubmeshManager's best-fit reuse of freed buffer ranges (mesh.rs:699-849,
 * impact_containers/src/range_allocator.rs); chunks that are no longer exposed or whose mesh is empty lose their submesh (swap_remove).
 * Buffers only grow: counts.n_vertices / n_indices are the buffer lengths including freed ranges, the submesh table says what is live. The chunks
 * are visited in chunk-linear order (the reference walks a hash set, an unpinned order that decides which freed range a chunk lands in). */
int ivx_mesh_sync(ivx_grid*, const uint8_t* invalidated_chunks, ivx_mesh_counts* out);
/* ... in two halves: `_enqueue` places the invalidated chunks' meshes (their sizes come with the last edit's results when the set is that
 * edit's: no count pass, no read-back) and launches their emit pass; `_collect` waits and returns the buffer lengths.
 * invalidated_chunks = NULL: the set of the edit that is IN FLIGHT (ivx_absorb_*_enqueue without its ivx_absorb_collect yet). What that edit's
 * chunks need reaches the host a third of the way down the edit's launches (the count role rings a bell of its own); the call waits for that,
 * places the meshes while the edit's region stages still run, and puts its launches behind them:
 *   ivx_absorb_sphere_enqueue -> ivx_mesh_sync_enqueue(g, NULL) -> ivx_absorb_collect -> ivx_mesh_sync_collect
 * is the edit and its re-mesh with one idle moment for the GPU less than the four calls in their usual order (same results). The edit must
 * have been enqueued with early delivery switched on for the object (ivx_grid_set_early_mesh_needs(g, 1): off by default — the count role
 * then pays a system-scope fence per workgroup, ~4 us per edit). */
int ivx_grid_set_early_mesh_needs(ivx_grid*, int on);
int ivx_mesh_sync_enqueue(ivx_grid*, const uint8_t* invalidated_chunks);
int ivx_mesh_sync_collect(ivx_grid*, ivx_mesh_counts* out);
/* VoxelMeshModifications (mesh.rs:113-123, 826-841), the hand-off to the renderer's buffers: the vertex / index ranges ivx_mesh_sync wrote since the
 * last report, in the order written, and whether any chunk lost its submesh; ivx_mesh_report_synchronized = report_gpu_resources_synchronized. */
typedef struct {
    uint32_t vertex_start, vertex_end, index_start, index_end;
} ivx_submesh_data_ranges;
int ivx_mesh_modifications(ivx_grid*, ivx_submesh_data_ranges* out, size_t cap, size_t* n_out, int* chunks_were_removed);
int ivx_mesh_report_synchronized(ivx_grid*);
/* device pointers of the mesh buffers (hand-off to a renderer without a host round trip):
 * 0 positions, 1 normals, 2 indices, 3 index materials, 4 submeshes */
void* ivx_mesh_device_ptr(ivx_grid*, int which);
/* The same buffers as handles another process or another graphics / compute API can import, so that the renderer (gpu_resource.rs:498-530,
 * 729-907 fills wgpu vertex / index / storage buffers from exactly these arrays; mesh.rs:94-123) takes the mesh without a host round trip:
 * `ipc_handle` = hipIpcMemHandle_t of the buffer (another HIP process: hipIpcOpenMemHandle), `dmabuf_fd` = a dma-buf file descriptor of it
 * (Vulkan / wgpu external memory: VK_EXT_external_memory_dma_buf; -1 where the runtime cannot make one; the caller closes it). `bytes` = the
 * part in use (after ivx_mesh_sync: the capacity, the live ranges are scattered), `generation` changes whenever a buffer was reallocated
 * (growth in ivx_remesh / ivx_voxel_step_collect / ivx_mesh_sync): handles of an older generation name freed memory — ask
 * ivx_mesh_generation every frame (no device work) and export again when it moved. which: as ivx_mesh_device_ptr.
 * `dmabuf_offset` / `dmabuf_bytes`: where the buffer lies inside the exported dma-buf object and how many bytes of it the descriptor
 * covers — the runtime exports whole pages of the underlying allocation, so a consumer binds [dmabuf_offset, dmabuf_offset + capacity_bytes)
 * of the imported memory (VkBindBufferMemory's memoryOffset). */
typedef struct {
    uint8_t ipc_handle[64];
    int32_t dmabuf_fd;
    uint32_t element_bytes;
    uint64_t bytes, capacity_bytes, generation, device_ptr;
    uint64_t dmabuf_offset, dmabuf_bytes;
} ivx_mesh_export_info;
int ivx_mesh_export(ivx_grid*, int which, ivx_mesh_export_info* out);
int ivx_mesh_generation(ivx_grid*, uint64_t* generation);
/* the importing side for a HIP consumer in another process: handle -> device pointer valid in the calling process, and back */
int ivx_mesh_import_open(const uint8_t ipc_handle[64], int device, void** device_ptr);
int ivx_mesh_import_close(void* device_ptr);

/* ---- a8: mass / inertia ------------------------------------------------------------------------- */
/* VoxelObjectInertialPropertyManager::initialized_from (object/inertia.rs:125-136, 615-790) */
int ivx_inertia(ivx_grid*, const float densities[256], ivx_moments* out);

/* ---- a9-a11: connected regions / split ---------------------------------------------------------- */
/* update_local_connected_regions_for_all_chunks + resolve_connected_regions_between_all_chunks
 * (object/split_detection.rs:305-487); region_count = VoxelObject::count_regions (255-301) */
int ivx_label_regions(ivx_grid*, uint32_t* region_count);
/* dense u32 component id per voxel (chunk-tiled; 0xFFFFFFFF = empty), ids = rank of the component's
 * representative region in chunk scan order */
int ivx_region_labels_download(ivx_grid*, uint32_t* labels, size_t n_voxels);
/* per-region descriptors in id order (find_two_disconnected_regions = the first two) */
int ivx_regions_describe(ivx_grid*, const float densities[256], ivx_region_desc* out, size_t cap, size_t* n_out);

/* VoxelObject::extract_any_disconnected_region (object/extraction.rs:78-596, 1901-2123): if the object consists of
 * several regions, the smaller of the first two (fewest non-uniform chunks, ties by chunk count, then the second)
 * is moved into a NEW grid whose chunk grid is the region's chunk box (repacked into a single chunk when it is
 * at most 2x2x2 chunks and at most 14 voxels wide); the parent loses those voxels. Both grids come back with
 * derived state and regions recomputed. outcome: 0 = one region, nothing done; 1 = *child is the new object
 * (caller destroys it), origin_offset_in_parent in voxels; 2 = the region had fewer than 8 voxels and was removed
 * without creating an object. `moved` (optional) receives the descriptor of the removed region — voxel count, box and
 * the mass moments the reference's PropertyTransferrer would have carried over (object/inertia.rs:341-560), for the
 * densities last set with ivx_grid_set_densities / ivx_regions_describe (1.0 if never set). */
int ivx_split_off_smallest_region(ivx_grid* parent, ivx_grid** child, uint32_t origin_offset_in_parent[3], int* outcome, ivx_region_desc* moved);
/* The whole loop in one call — `while find_two_disconnected_regions { extract the smaller of the first two }` (impact_voxel/src/interaction.rs:256,
 * object/extraction.rs:255-271): the object's regions are described once, the host plays the loop over the descriptors (a region's voxel
 * count, box and chunk counts do not change when another region leaves, nor does the scan order), every region that goes is moved into a grid
 * of its own (all from one device block), and the parent and all children are re-derived together. Results in the order the loop extracts
 * them: children[k] (NULL for a discarded crumb), origins3 (3 per split-off), outcomes (1 object, 2 crumb), moved (optional descriptors);
 * *n_out = split-offs made = regions - 1 (IVX_ERR_CAPACITY when cap is smaller; nothing is changed then). Same objects, voxel for voxel, as
 * the loop over ivx_split_off_smallest_region. */
int ivx_split_off_all(ivx_grid* parent, size_t cap, ivx_grid** children, uint32_t* origins3, int* outcomes, ivx_region_desc* moved, size_t* n_out);

/* VoxelObject::extract_polyhedron / copy_polyhedron (object/extraction.rs:604-1768): the part of the object inside the convex
 * polyhedron given by `n_planes` face planes (planes4 = n x {unit normal x,y,z, displacement}, outward normals) and its AABB
 * (lower xyz, upper xyz), all in the object's normalized model space (voxel units, grid corner at the origin). copy = 0
 * removes the polyhedron from the parent (which keeps max(sdf, complement(d))), copy = 1 leaves the parent untouched.
 * Outcome and child conventions as for ivx_split_off_smallest_region; outcome 0 = the AABB misses the object. */
int ivx_clip_polyhedron(ivx_grid* parent, const float* planes4, size_t n_planes, const float aabb[6], int copy, ivx_grid** child,
                        uint32_t origin_offset_in_parent[3], int* outcome);
/* Batched COPY of several polyhedra out of one object — all fragments of one impact (FracturingProcess::execute_in_parallel,
 * fracturing.rs:1047-1189, over copy_polyhedron_with_property_computer, extraction.rs:1301-1768): `planes4` holds the plane sets one after the
 * other (plane_counts[f] planes of 4 floats each), `aabbs6` six floats per set. children[f] / origins3[3 f ..] / outcomes[f] are what
 * ivx_clip_polyhedron(copy = 1) returns for set f (outcome 0 = no overlap, 1 = object, 2 = fewer than 8 voxels: no object); the work of all
 * fragments is enqueued back to back and read with two host waits in all. */
int ivx_copy_polyhedra(ivx_grid* parent, const float* planes4, const uint32_t* plane_counts, const float* aabbs6, size_t n_sets, ivx_grid** children,
                       uint32_t* origins3, int* outcomes);

/* ---- whole voxel step (resident inputs, minimal host synchronisation) ---------------------------- */
/* The per-frame chain the engine runs for a voxel object — generate (engine/src/setup/scene/voxel.rs:33 ->
 * impact_voxel/src/setup.rs:555-579), derived state, mesh (engine/src/tasks.rs:376-399) and inertial
 * properties (setup.rs:581-616) — as ONE call over inputs that already live in HBM. `stages` selects
 * what runs; results come back in one small struct. Stage durations are measured with HIP events on
 * the context's stream (no extra synchronisation). */
#define IVX_STAGE_SAMPLE 1u
#define IVX_STAGE_DERIVE 2u
#define IVX_STAGE_OCCUPIED 4u
#define IVX_STAGE_REGIONS 8u
#define IVX_STAGE_REMESH 16u
#define IVX_STAGE_INERTIA 32u
#define IVX_STAGE_ALL 63u
/* timed slots of a step: 0 sample (k_sdf_super, k_sdf_prepass, k_sdf_eval), 1 derive (k_chunk_pre, k_derive: flags, chunk state, chunk-local
 * regions, chunk moments), 2 post1 (one launch: mesher count | region merge by chunk columns | occupied slots | moment partial sums),
 * 3 post2 (one launch: exact local numbering, then multi-region merge | mesher scan | moments and occupied ranges final), 4 emit (one launch:
 * region forest flatten | mesher emit), 5 assign (component ids), 6..9 unused */
#define IVX_N_TIMED_STAGES 10
typedef struct {
    ivx_mesh_counts mesh;
    uint32_t region_count;
    uint32_t occupied[12];
    uint32_t reserved[3];
    ivx_moments moments;
    float stage_ms[IVX_N_TIMED_STAGES];
    float reserved2[2];
} ivx_step_result;
/* ---- voxel edit ops --------------------------------------------------------------------------------------
 * apply_sphere_absorption (impact_voxel/src/interaction/absorption.rs:801-844) over modify_voxels_within_sphere
 * (object/intersection.rs:283-395): an absorbing sphere eats into the object. The sphere is given in the object's normalized space
 * (voxel units, lower grid corner at the origin): `influence_radius` = radius + 2 voxels bounds the voxels that are visited,
 * `sphere_radius` enters the new signed distance max(sd, -(|p - c| - R)). Needs current derived state and regions; leaves
 * them current (flags, chunk kinds, regions of the edited object). `removed_moments` are the ten moments (layout of
 * ivx_moments.m64) of the voxels that became empty — what VoxelObjectInertialPropertyUpdater::remove_voxel subtracts
 * (object/inertia.rs:377-394); `emptied_by_type` (256 counts, may be NULL) is what the absorbed-voxel tracker registers;
 * `invalidated_chunks` (one byte per chunk, may be NULL) is the set handle_chunk_voxels_modified registers for remeshing
 * (intersection.rs:532-598). */
typedef struct {
    double removed_moments[10];
    uint64_t emptied_voxels;
    uint32_t touched_chunks; /* chunks with a voxel centre inside the influence sphere */
    uint32_t removed_chunks; /* chunks that became Void */
} ivx_absorb_result;
int ivx_absorb_sphere(ivx_grid*, const float center[3], float influence_radius, float sphere_radius, const float densities[256],
                      ivx_absorb_result* out, uint32_t* emptied_by_type, uint8_t* invalidated_chunks);
/* apply_capsule_absorption (interaction/absorption.rs:846-889) over modify_voxels_within_capsule (object/intersection.rs:417-530):
 * the same with an absorbing capsule — segment start + vector in the object's normalized space, `influence_radius` = radius + 2
 * voxels. Per chunk the segment is clipped against the chunk box grown by the radius (Capsule::trim_segment_outside_aab,
 * impact_geometry/src/capsule.rs:144-164) and only the voxel ranges under the clipped capsule's box are visited; a voxel is inside
 * when its centre is within the radius of the whole segment, boundary included (capsule.rs:225-250). */
int ivx_absorb_capsule(ivx_grid*, const float segment_start[3], const float segment_vector[3], float influence_radius, float capsule_radius,
                       const float densities[256], ivx_absorb_result* out, uint32_t* emptied_by_type, uint8_t* invalidated_chunks);
/* The same edits in two halves, for a frame that has other work to put on the stream (or other objects to edit) before it waits:
 * `_enqueue` launches the edit, the sweep over the touched chunks and their neighbours, the region resolve and the count of what the
 * invalidated meshes need, and returns; ivx_absorb_collect waits ONCE and delivers what ivx_absorb_sphere / _capsule return. One edit per
 * object in flight; every other call on the object waits for the collect. */
int ivx_absorb_sphere_enqueue(ivx_grid*, const float center[3], float influence_radius, float sphere_radius, const float densities[256]);
int ivx_absorb_capsule_enqueue(ivx_grid*, const float segment_start[3], const float segment_vector[3], float influence_radius, float capsule_radius,
                               const float densities[256]);
int ivx_absorb_collect(ivx_grid*, ivx_absorb_result* out, uint32_t* emptied_by_type, uint8_t* invalidated_chunks);
/* apply_mutual_absorption (interaction/absorption.rs:891-1079): two objects eat into each other where they overlap. Every voxel of A's overlap
 * ranges (determine_voxel_ranges_encompassing_intersection, padded by one voxel of B) that is not maximally outside gets
 * sdf_subtraction(sd, max(sd, B's SDF at its centre), smoothness) with B's SDF sampled trilinearly (sample_voxel_object_sdf, object/sdf.rs:636-675);
 * every voxel of B's overlap ranges the same against A's SDF as it was before the call. rotation (xyzw) + translation = each object's world -> object
 * transform. Results per object as for ivx_absorb_sphere; both objects need current derived state and regions, and keep them current. */
int ivx_absorb_mutual(ivx_grid* a, const float rotation_a[4], const float translation_a[3], const float densities_a[256], ivx_grid* b,
                      const float rotation_b[4], const float translation_b[3], const float densities_b[256], float smoothness, ivx_absorb_result* out_a,
                      ivx_absorb_result* out_b, uint8_t* invalidated_chunks_a, uint8_t* invalidated_chunks_b);

/* ---- many objects per call ----------------------------------------------------------------------------------------------------------
 * The reference's per-frame unit is the manager, not the object: every voxel object's mesh is synced each frame (impact_voxel/src/lib.rs:729-733,
 * engine/src/tasks.rs:376-399), the fragments of an impact come into being together (interaction/fracturing.rs:1047-1189), its stress scene holds
 * a thousand small objects. One object's step, edit or sync is about ten launches of a few microseconds — for a small object all of its cost.
 * These calls run the same per-object work for N objects of one context in the launches of ONE: each launch of the chain is issued once for
 * all objects (csrc/many.hpp), their results arrive together, the host waits once. Same results per object as the single-object calls.
 *   ivx_voxel_step_many      ivx_voxel_step for every object (stages without IVX_STAGE_SAMPLE merge; a sample stage runs object by object)
 *   ivx_absorb_sphere_many   ivx_absorb_sphere, one sphere per object (centers3: 3 floats per object); `invalidated_chunks`: NULL, or one
 *                            array per object (entries may be NULL)
 *   ivx_absorb_capsule_many  ivx_absorb_capsule, one capsule per object (segment start and segment vector: 3 floats each per object)
 *   ivx_mesh_sync_many       ivx_mesh_sync for every object
 * A call that fails half way (an object refused, a launch failed) drains the stream and discards what the objects before it had in flight:
 * no object is left "pending"; step the objects again before using their derived state.
 * ivx_many_begin / ivx_many_flush expose the mechanism itself: between them the `_enqueue` calls of objects of the context are recorded — a
 * chain per object, in the order the objects first appear — and the flush issues them merged, front by front. A call on an object of another
 * context inside the bracket is issued on that context's stream, unrecorded. ivx_many_flush reports a failure of any flush since the begin
 * (launches that a failed flush dropped never run; `_collect` calls that wait for them fail with IVX_ERR_HIP). The recorder and its staging
 * blocks belong to the context and go with ivx_shutdown. A begin on a thread whose last bracket was never flushed (a caller that failed in
 * between) closes that bracket first: what it recorded goes out, the thread is not left refusing brackets. ivx_many_stats: out[0] launches recorded, [1] merged launches issued, [2] flushes
 * made on this context so far. */
int ivx_many_begin(ivx_ctx*);
int ivx_many_flush(ivx_ctx*);
int ivx_many_stats(ivx_ctx*, uint64_t out[3]);
int ivx_voxel_step_many(ivx_grid* const* grids, size_t n, uint32_t stages, ivx_step_result* out);
int ivx_absorb_sphere_many(ivx_grid* const* grids, size_t n, const float* centers3, const float* influence_radii, const float* sphere_radii,
                           const float densities[256], ivx_absorb_result* out, uint8_t* const* invalidated_chunks);
int ivx_absorb_capsule_many(ivx_grid* const* grids, size_t n, const float* segment_starts3, const float* segment_vectors3, const float* influence_radii,
                            const float* capsule_radii, const float densities[256], ivx_absorb_result* out, uint8_t* const* invalidated_chunks);
int ivx_mesh_sync_many(ivx_grid* const* grids, size_t n, const uint8_t* const* invalidated_chunks, ivx_mesh_counts* out);

/* make the compiled SDF program / the voxel-type densities resident on the device */
int ivx_grid_set_sdf_program(ivx_grid*, const ivx_sdf_processed_node* nodes, size_t n_nodes, uint32_t stack_size,
                             const uint32_t grid_shape[3], const float shifted_grid_center[3], uint8_t voxel_type);
int ivx_grid_set_densities(ivx_grid*, const float densities[256]);
/* voxel type generator of the grid's sampler: n_voxel_types = 0 -> SameVoxelTypeGenerator (the voxel_type argument of ivx_sdf_sample /
 * ivx_grid_set_sdf_program, the default); 1..255 -> GradientNoiseVoxelTypeGenerator (voxel_type.rs:97-169), the voxel_type argument is
 * then ignored. Holds for every later ivx_sdf_sample and sample stage of the grid until set again.
 * The type of a voxel is the index t < n_voxel_types of the greatest of the noise values simplex4(t * voxel_type_frequency, z * f, y * f,
 * x * f, seed), f = noise_frequency, (x, y, z) the voxel's indices relative to the shifted grid centre (the first maximum; the seed's bits
 * as the reference's `as i32` keeps them). The construction is the reference's, the noise values are this library's
 * (impact_amd/csrc/noise.hpp), whose coordinate range applies: |coordinate * frequency| < 2^31.
 * IVX_ERR_INVALID for n_voxel_types > 255 (255 is VoxelType::dummy()) or a non-finite frequency; the generator then stays as it was. */
int ivx_grid_set_voxel_type_noise(ivx_grid*, uint32_t n_voxel_types, float noise_frequency, float voxel_type_frequency, uint32_t seed);
int ivx_voxel_step(ivx_grid*, uint32_t stages, ivx_step_result* out);
/* The same in two halves: enqueue launches the kernels of `stages` and returns without waiting (several calls may follow
 * each other, e.g. the phases of the multi-GPU protocol with halo traffic in between); collect waits once, fetches the
 * results of everything enqueued since the last collect and, if the mesh outgrew the buffers kept from earlier steps,
 * grows them and repeats the emit pass. */
int ivx_voxel_step_enqueue(ivx_grid*, uint32_t stages);
int ivx_voxel_step_collect(ivx_grid*, ivx_step_result* out);
/* Stage timing (ivx_step_result::stage_ms): slot_mask bit i = time slot i. Default: every slot. 0 turns timing off (stage_ms reads 0).
 * A whole step on the fused path (ivx_voxel_step / _enqueue outside the slab protocol, on a grid of at most 524 288 chunks, with the derive
 * stage in the call or nothing left for the stand-alone per-chunk kernels) costs the queue nothing for it: the first workgroup of the
 * slot's first launch and of the first launch enqueued behind the slot write the device's constant-rate clock, and stage_ms[i] is the
 * distance of the two — START TO START, the launch boundary behind the slot included; the last slot of a call ends where the next launch
 * of this grid starts, which is the step's result gather unless another call was enqueued first (a launch of another object in between
 * falls into that boundary). A slot without a launch reads 0. Every other path — the slab protocol's phases, calls enqueued in parts,
 * larger grids, calls that run the stand-alone region / moment kernels — brackets a slot with two event records on the stream, about
 * 2-3 us each on the GPU's queue, and stage_ms[i] is the distance of those (the boundary in FRONT of the slot included). One call never
 * mixes the two. IVX_STAGE_TIMING_EVENTS=1 in the environment (read when the library is loaded) forces the event records everywhere. */
int ivx_grid_set_stage_timing(ivx_grid*, uint32_t slot_mask);
/* Developer aid: the raw clock stamps behind the last collected step's stage_ms, ticks[2 * i] = start and ticks[2 * i + 1] = end of slot i
 * (0: not stamped — not timed, no launch, or timed by events); *clock_khz (may be null) = the clock's rate. */
int ivx_debug_stage_ticks(ivx_grid*, unsigned long long ticks[2 * IVX_N_TIMED_STAGES], double* clock_khz);
/* Sample-ahead, for callers that sample the resident program step after step (the voxel generator of a streamed or re-generated object,
 * generation.rs:293-371 per chunk — the bench's headline step): with `on`, a sample stage also enqueues the NEXT sample stage's interval
 * pre-pass — it reads nothing but the program and the grid's geometry — on the context's second stream behind its own evaluator, and the next
 * sample stage starts at its evaluator. Same bytes either way. A step that never comes costs one unused pre-pass;
 * ivx_grid_set_sdf_program and ivx_grid_destroy wait for one that is under way. Off by default. */
int ivx_grid_set_sample_ahead(ivx_grid*, int on);

/* ---- multi-GPU: x-slab halos ----------------------------------------------------- */
/* Face planes of (sdf,type) and boundary chunk info, packed contiguously for torch.distributed /
 * RCCL send-recv: bytes = ivx_halo_bytes(). side 0 = lower x face, 1 = upper x face. The buffers are
 * device pointers owned by the caller (e.g. a torch tensor). */
size_t ivx_halo_bytes(ivx_grid*);
int ivx_halo_pack(ivx_grid*, int side, void* device_buf);
int ivx_halo_unpack(ivx_grid*, int side, const void* device_buf); /* install as ghost layer on `side` */
int ivx_halo_clear(ivx_grid*, int side);                          /* no neighbour: outside the grid */
/* stream-ordered variants (no host wait): for callers whose communication runs on the context's stream */
int ivx_halo_pack_enqueue(ivx_grid*, int side, void* device_buf);
/* installs the buffer itself as the ghost layer (no copy): it must be 16-byte aligned and stay untouched until the next
 * ivx_halo_unpack* / ivx_halo_clear of that side */
int ivx_halo_unpack_enqueue(ivx_grid*, int side, const void* device_buf);
/* both faces in one launch (either buffer may be NULL); with_face_labels != 0 appends the face planes of component ids
 * (ivx_region_face_bytes() bytes) right behind the ivx_halo_bytes() of each message */
int ivx_halo_pack_both_enqueue(ivx_grid*, void* lower_buf, void* upper_buf, int with_face_labels);

/* Cross-slab connected regions: after ivx_label_regions on every slab, exchange the face planes of
 * component ids with the x neighbours, list the distinct (own component, neighbour component) pairs
 * that touch across the face, all-gather the pairs and finish the union on the host. This carries the
 * reference's cross-chunk region connections (object/split_detection.rs:323-487, 1046-1325) across ranks.
 * ivx_region_face_labels writes cy*cz*256 u16 (0xFFFF = empty voxel; a slab holds fewer than 65 535 components) to a DEVICE buffer;
 * ivx_region_face_pairs takes the neighbour's plane (device) and returns sorted unique pairs
 * (pairs[2i] = own id, pairs[2i+1] = neighbour id) in HOST memory. */
size_t ivx_region_face_bytes(ivx_grid*);
int ivx_region_face_labels(ivx_grid*, int side, void* device_buf);
int ivx_region_face_pairs(ivx_grid*, int side, const void* neighbour_face_labels_device, uint32_t* pairs, size_t cap, size_t* n_out);
/* Stream-ordered form of the same exchange, ending in ONE fixed-size record per slab that is written on the device and can go
 * straight into an all-gather: ivx_step_record_words() 64-bit words = [0] components of the slab, [1] number of (own,
 * neighbour) pairs across the upper face, [2..14) occupied ranges, [14..17) mesh vertices / indices / submeshes, [17] error
 * flags, [18..28) the 10 moments (f64 bit patterns), [28..) the pairs (at most 4096). */
int ivx_region_face_labels_enqueue(ivx_grid*, int side, void* device_buf);
int ivx_region_face_pairs_enqueue(ivx_grid*, int side, const void* neighbour_face_labels_device);
size_t ivx_step_record_words(void);
int ivx_step_record_enqueue(ivx_grid*, void* device_record);
/* The three calls a slab's last phase makes — the pairs across its upper face (from the neighbour's face ids; null: no upper neighbour),
 * ivx_voxel_step_enqueue(IVX_STAGE_REMESH), the record — in the remesh stage's own four launches. The step's small results land in the
 * grid's host-mapped block on the way: once the stream is idle (the protocol's doorbell) ivx_voxel_step_collect returns them without a
 * launch of its own. (What ivx_slabs_step_enqueue calls) */
int ivx_slab_remesh_enqueue(ivx_grid*, const void* neighbour_face_ids_device, void* device_record);

/* ---- a13 / §8f-3: from an impact to fragment plane sets (host code: a few hundred points per impact) ------------------------------------
 * generate_impact_fracture_points (impact_voxel/src/interaction/fracturing.rs:1710-2015), DelaunayTetrahedralization
 * (impact_tesselation/src/delaunay.rs), VoronoiPolyhedron (impact_tesselation/src/voronoi.rs). The fragments of an impact are then
 *   region   = ivx_clip_polyhedron(object, ivx_delaunay_boundary_face_planes(Delaunay(boundary points)), its aabb, extract)   fracturing.rs:1537-1632
 *   cells    = for v in 4 .. vertices(Delaunay(fracture points - region origin)): ivx_voronoi_polyhedron(v), ivx_voronoi_bounded_aabb
 *   fragments= ivx_copy_polyhedra(region, planes displaced by -0.1, boxes)                                                   fracturing.rs:1190-1240
 * Vertex indices: 0..3 are the ad-hoc bounding tetrahedron, the points follow in input order (near-coincident points are skipped). */
typedef struct {                 /* VoxelImpactFracturingConfig (fracturing.rs:855-871: the defaults ivx_impact_fracturing_config_default fills in) */
    uint32_t boundary_polar_grid_size, boundary_azimuthal_grid_size;
    float boundary_angular_jitter, boundary_radial_jitter;
    uint64_t max_fragment_count;
    float radial_falloff_power, angular_falloff_power;
    uint32_t radial_grid_size, angular_grid_size;
    uint64_t max_position_rejections_per_sample;
    uint64_t seed;
} ivx_impact_fracturing_config;  /* 56 bytes */
typedef struct {                 /* FracturingProperties, #[repr(C)] Pod (fracturing.rs:61-86) */
    float fracturing_force, shattering_pressure, fragment_scale, min_fragment_extent, max_fragment_extent;
} ivx_fracturing_properties;     /* 20 bytes */
void ivx_impact_fracturing_config_default(ivx_impact_fracturing_config*);
/* Points in the object's normalized space (voxel units). rng_state: in/out state of the frame's generator (first impact: the seed). The
 * stream is fastrand 2.3.0's wyrand restated from its published source: the crate is not vendored, no reference test pins it. */
int ivx_generate_impact_fracture_points(const ivx_impact_fracturing_config*, const ivx_fracturing_properties*, float inverse_voxel_extent,
                                        const float world_to_object_rotation_xyzw[4], const float world_to_object_translation[3], const float object_aabb[6],
                                        const float force_position[3], const float force_unit_direction[3], float force_magnitude, uint64_t* rng_state,
                                        float* boundary_points3, size_t cap_boundary, size_t* n_boundary, float* fracture_points3, size_t cap_fracture,
                                        size_t* n_fracture);
typedef struct ivx_delaunay ivx_delaunay;
#define IVX_NO_TETRAHEDRON 0xFFFFFFFFu
int ivx_delaunay_construct(const float* points3, size_t n_points, ivx_delaunay** out);
void ivx_delaunay_destroy(ivx_delaunay*);
int ivx_delaunay_counts(const ivx_delaunay*, uint32_t counts[2] /* vertices incl. the 4 ad-hoc ones, tetrahedra */);
int ivx_delaunay_download(const ivx_delaunay*, float* vertices3, uint32_t* tet_vertices4, uint32_t* tet_neighbors4 /* across the face opposite corner c */);
/* displace_vertices (fracturing.rs:996-1002: the tetrahedralization built on the points as given is moved into the region object's frame) */
int ivx_delaunay_displace_vertices(ivx_delaunay*, const float offset[3]);
int ivx_delaunay_aabb(const ivx_delaunay*, float aabb[6]);
int ivx_delaunay_boundary_face_planes(const ivx_delaunay*, float* planes4 /* outward unit normal, displacement */, size_t cap, size_t* n_out);
int ivx_voronoi_polyhedron(const ivx_delaunay*, uint32_t vertex, float* vertices3, size_t cap_vertices, float* rays6 /* origin, unit direction */, size_t cap_rays,
                           float* planes4, size_t cap_planes, size_t n_out[3] /* vertices, rays, planes */);
int ivx_voronoi_bounded_aabb(const float* vertices3, size_t n_vertices, const float* rays6, size_t n_rays, const float bounding_aabb[6], float out_aabb[6], int* has);

/* ---- multi-GPU: the whole per-step protocol behind the C ABI ----------------------------------------------------------------------
 * One process per GPU owns one x-slab (an ivx_grid created with its chunk offset) and an RCCL communicator; ivx_slabs_step_enqueue
 * runs sample -> face exchange -> derive + regions + moments -> face exchange (+ component ids) -> remesh -> record all-gather, all
 * stream-ordered on the context's stream (grouped ncclSend / ncclRecv with the two x neighbours, one small ncclAllGather);
 * ivx_slabs_step_collect waits once, finishes the cross-slab union-find of the region equivalences and hands back the global results.
 * A Rust host binds these five entry points and keeps only the launcher (who is rank r, how the 128-byte unique id reaches the ranks).
 *   ivx_comm_unique_id   rank 0 makes the id (ncclGetUniqueId) and distributes it by its own means
 *   ivx_comm_init        ncclCommInitRank on the context's device; librccl is opened at run time (no link-time dependency)
 *   ivx_comm_init_local  an in-process communicator: all `nranks` slabs live in THIS process on one GPU and exchange by device copies —
 *                        the same driver code, used to check the decomposition on a single-GPU box
 * slabs: RCCL communicator -> exactly one slab (this rank's); in-process communicator -> all of them, in rank order. */
typedef struct ivx_comm ivx_comm;
typedef struct ivx_slab ivx_slab;
typedef struct {
    uint32_t region_count;           /* connected regions of the whole grid */
    uint32_t local_region_count;     /* components of this slab */
    uint32_t first_local_component;  /* index of this slab's component 0 in the concatenation over ranks */
    uint32_t reserved;
    double moments[10];              /* of the whole grid, summed in rank order */
    uint32_t occupied[12];           /* global occupied chunk / voxel ranges (layout of ivx_step_result::occupied) */
    ivx_mesh_counts mesh;            /* this slab's mesh */
    uint64_t vertex_offset, index_offset; /* of this slab's mesh in the concatenation over ranks */
    uint64_t total_triangles;
    float stage_ms[IVX_N_TIMED_STAGES];
    float reserved2[2];
} ivx_slab_result;
int ivx_comm_unique_id(void* out128);
int ivx_comm_init(ivx_ctx*, int nranks, int rank, const void* unique_id128, ivx_comm** out);
int ivx_comm_init_local(ivx_ctx*, int nranks, ivx_comm** out);
/* One PROCESS per rank on ONE device (RCCL refuses two ranks on a device): a rank copies its face planes straight into its neighbour's receive
 * buffer (hipIpcGetMemHandle / hipIpcOpenMemHandle), sequence numbers and the record gather go through the POSIX shared-memory block `name`
 * ("/..."; rank 0 creates it). The host waits at every exchange: a transport for running the protocol's driver as separate processes where
 * there is one GPU (tests/test_gpu_slabs_ipc.py), not for speed. ivx_slab_create is collective on such a communicator. */
int ivx_comm_init_ipc(ivx_ctx*, int nranks, int rank, const char* name, ivx_comm** out);
/* transport (0 RCCL, 1 in-process, 2 shared device), rank count and this process's rank as the communicator reports them (RCCL: ncclCommCount,
 * ncclCommUserRank) */
int ivx_comm_info(ivx_comm*, int* transport, int* nranks, int* rank);
/* Diagnostic (no reference counterpart): the in-process transport normally moves nothing (a slab reads its neighbour's send buffer in place).
 * on = 1: it moves its messages as the RCCL transport does — copies on the communicator's own stream behind the packing, the slabs' derive
 * sweep and mesher count split around their arrival (interior chunk planes first, the planes beside the ghost layers after the wait) — so
 * that a one-GPU box exercises the overlapped protocol; on = 2: the copies on the context's stream, sweeps unsplit; 0: back to in place. */
int ivx_comm_set_local_copies(ivx_comm*, int on);
void ivx_comm_destroy(ivx_comm*);
/* Diagnostic (no reference counterpart): runs every RCCL call the protocol makes — ncclGetUniqueId, ncclCommInitRank, a grouped
 * ncclSend / ncclRecv pair, ncclAllGather — on a ONE-rank communicator of this context's device and stream (the send goes to the rank
 * itself) and checks the bytes that come back. A single-GPU box can so prove that the run-time binding to librccl (dlopen, symbols,
 * argument layouts, the library's stream) works before a multi-rank job depends on it. IVX_OK = all of it worked. */
int ivx_comm_selftest(ivx_ctx*);
/* Diagnostic (no reference counterpart): the mesher divides decoded distances (surface_nets.rs:396-404, t = d1 / (d1 - d2)) and edge counts
 * with a short correctly-rounding sequence instead of the general f32 division; this runs both over the whole operand set (every pair of
 * decoded i8 distances of opposite sign, 1 / n for n = 1..256) on the device and returns the number of results that differ: must be 0. */
int ivx_selftest_mesher_division(ivx_ctx*, uint32_t* mismatches);
/* Developer export (tests): evaluates the library's noise functions (impact_amd/csrc/noise.hpp) at n given points — which = 0: fbm3 at
 * points (x, y, z), params = {frequency, lacunarity, gain, octaves (u32 bits), seed (u32 bits)}; which = 1: simplex4 at points (x, y, z, w),
 * params[4] = seed (u32 bits), the rest unused. Host arrays. On the device of `ctx`; ctx = NULL runs the host build of the same functions. */
int ivx_noise_eval(ivx_ctx* ctx, int which, const float* params, const float* points, size_t n, float* out);
/* Developer export (tests), beside ivx_noise_eval: the 4096 gradient-noise voxel types (ivx_grid_set_voxel_type_noise, n_voxel_types 1..255)
 * of the chunk whose root-space origin is given, i << 8 | j << 4 | k order. On the device of ctx; ctx = NULL runs the host build of the
 * same function. */
int ivx_voxel_types_eval(ivx_ctx* ctx, uint32_t n_voxel_types, float noise_frequency, float voxel_type_frequency, uint32_t seed,
                         const float chunk_origin[3], uint8_t out[4096]);
/* Developer export (tests): what a sample stage would launch, decided on the host alone — no device is touched, no context needed.
 * in[0] nodes, [1] stack size, [2] the program has a noise node, [3] it is the grid's resident program, [4] the list lengths are known,
 * [5..8) the lengths, [8] chunks, [9..12) chunk counts, [12] compute units, [13] the list counters are dirty, [14] scratch groups to preset,
 * [15] sample-ahead on, [16] its state (0 idle, 1 wanted, 2 pending), [17], [18] sample-ahead on and the resident program's nodes when a
 * later step acts on the wish.
 * out[0] program words, [1] super-block tables made inside the pre-pass, [2..5) super-blocks per axis, [5] the pending pre-pass is consumed,
 * [6] ... is cancelled, [7..10) groups preset by the super-block launch, the pre-pass, the first evaluator launch, [10] counters cleared by a
 * memset, [11] the next pre-pass may run ahead, [12] evaluator launches n <= 3; launch i at [13 + 10 i]: class (2 one-level, 1 two-level,
 * 0 general), noise form, grid, LDS bytes, scratch offset, list, with the long-entry split, with list 1 behind it, commits the shadow records.
 * [43] state after the stage, [44] state after a step acted on the wish, [45] that step launches the pre-pass, [46] state after a cancel
 * (from in[16]), [47] the cancel waits for a pre-pass. IVX_ERR_CAPACITY: the stack does not fit the LDS (as a sample call would report). */
#define IVX_SAMPLER_PLAN_IN_WORDS 19
#define IVX_SAMPLER_PLAN_OUT_WORDS 48
int ivx_sampler_plan(const uint32_t in[IVX_SAMPLER_PLAN_IN_WORDS], uint32_t out[IVX_SAMPLER_PLAN_OUT_WORDS]);
int ivx_slab_create(ivx_comm*, ivx_grid* slab_grid, int rank, ivx_slab** out);
void ivx_slab_destroy(ivx_slab*);
int ivx_slabs_step_enqueue(ivx_slab** slabs, size_t n);
int ivx_slabs_step_collect(ivx_slab** slabs, size_t n, ivx_slab_result* out /* n results */);
/* global region id of every slab-local component of `rank` (after a collect; `first_slab` = slabs[0] of that call) */
int ivx_slab_region_map(ivx_slab* first_slab, int rank, uint32_t* out, size_t cap, size_t* n_out);

/* ---- a15-a19: rigid bodies + sequential-impulses contact solve (engine/crates/impact_physics) ----- */
/* DynamicRigidBody, #[repr(C)], 152 bytes (src/rigid_body.rs:94-103). Matrices are Matrix3C (column-major),
 * orientation is UnitQuaternionC (x, y, z, w). */
typedef struct {
    float mass;
    float inertia[9], inv_inertia[9]; /* InertiaTensorC about the centre of mass, body frame (src/inertia.rs:41-47) */
    float position[3];
    float orientation[4];
    float momentum[3], angular_momentum[3];
    float total_force[3], total_torque[3];
} ivx_rigid_body;
/* KinematicRigidBody, 56 bytes (src/rigid_body.rs:108-117): AngularVelocityC = unit axis + angular speed */
typedef struct {
    float position[3];
    float orientation[4];
    float velocity[3];
    float angular_axis[3];
    float angular_speed;
} ivx_kinematic_body;
/* One ContactWithID of a collision (src/constraint/contact.rs:23-57) with the two rigid bodies it acts on.
 * body_a/body_b index the dynamic bodies; bit 31 set = index into the kinematic bodies. position =
 * ContactGeometry::position (point on B), normal = surface normal of B, depth = penetration depth; the
 * three response parameters are the already combined ones (src/material.rs:43-52). flags bit 0 marks the
 * first contact of a manifold (one Collision): interlock analysis works per manifold
 * (contact.rs:610-689). 64 bytes. */
typedef struct {
    uint64_t id; /* ContactID */
    uint32_t body_a, body_b;
    float position[3];
    float normal[3];
    float depth;
    float restitution, static_friction, dynamic_friction;
    uint32_t flags, reserved;
} ivx_contact;

/* ---- voxel contact generation (sphere collidables) -----------------------------------------------------------
 * for_each_sphere_voxel_object_contact (impact_voxel/src/collidable.rs:1098-1127) wrapped as generate_sphere_voxel_object_contact_manifold
 * does (collidable.rs:1051-1096): every surface voxel (non-empty, fewer than six neighbours) in the voxel ranges the sphere's box touches
 * is a sphere of radius -sd * extent tested against the collidable (determine_sphere_sphere_contact_geometry, impact_physics
 * collision/collidable/sphere.rs:105-136). `rotation_xyzw` + `translation` = transform_to_object_space (Isometry3: world -> the object's
 * model space), the sphere is in world space; `response` = the combined restitution, static and dynamic friction. Contacts come in the
 * reference's traversal order (chunks i,j,k then voxels i,j,k) with id = ContactID::from_two_u64_and_n_indices(collidable_id_a,
 * collidable_id_b, [i,j,k]) and the first one flagged IVX_CONTACT_MANIFOLD_START: ready for ivx_world_set_contacts. Needs current derived
 * state. *n_out is the number found even when it exceeds `cap` (IVX_ERR_CAPACITY then). */
int ivx_sphere_voxel_object_contacts(ivx_grid*, const float rotation_xyzw[4], const float translation[3], const float sphere_center[3],
                                     float sphere_radius, uint64_t collidable_id_a, uint64_t collidable_id_b, uint32_t body_a, uint32_t body_b,
                                     const float response[3], ivx_contact* out, size_t cap, size_t* n_out);
/* for_each_voxel_object_plane_contact (collidable.rs:1176-1208): the same for a plane collidable (unit normal + displacement, world space);
 * only Corner voxels (at most three neighbours) inside the voxel ranges of the plane's negative halfspace are tested
 * (determine_sphere_plane_contact_geometry, sphere.rs:138-160). The reference hashes the ids as (plane, voxel object) and the contact
 * normal is the plane's: pass the collidable ids in that order and the voxel object's body as body_a. */
int ivx_plane_voxel_object_contacts(ivx_grid*, const float rotation_xyzw[4], const float translation[3], const float plane_unit_normal[3],
                                    float plane_displacement, uint64_t collidable_id_a, uint64_t collidable_id_b, uint32_t body_a, uint32_t body_b,
                                    const float response[3], ivx_contact* out, size_t cap, size_t* n_out);
/* for_each_capsule_voxel_object_contact (collidable.rs:1257-1286): the same for a capsule collidable (segment start + vector + radius, world
 * space); surface voxels inside the capsule's box are tested with determine_capsule_sphere_contact_geometry
 * (impact_physics/src/collision/collidable/capsule.rs:212-270). Ids and bodies as for the sphere (collidable first). */
int ivx_capsule_voxel_object_contacts(ivx_grid*, const float rotation_xyzw[4], const float translation[3], const float segment_start[3],
                                      const float segment_vector[3], float capsule_radius, uint64_t collidable_id_a, uint64_t collidable_id_b,
                                      uint32_t body_a, uint32_t body_b, const float response[3], ivx_contact* out, size_t cap, size_t* n_out);
/* The same three generators for MANY objects in one call — the reference's collision pass visits every voxel object of the scene with the
 * collidables near it (impact_voxel/src/collidable.rs:1051-1286) —, one collidable per object: query i goes with grids[i]. The per-object
 * launches are merged (csrc/many.hpp) and the host waits twice for ALL objects (totals, then contacts) instead of twice per object.
 * out_offsets has n + 1 entries: object i's contacts are out[out_offsets[i] .. out_offsets[i + 1]), the very list the single-object call
 * returns (one manifold each). IVX_ERR_CAPACITY when the contacts of all objects exceed `cap` (out_offsets then holds the sizes needed). */
typedef struct ivx_collidable_query {
    int32_t mode;             /* 0 sphere, 1 plane, 2 capsule */
    float rotation_xyzw[4];   /* transform_to_object_space of the voxel object, as in the single-object calls */
    float translation[3];
    float shape3[3];          /* sphere centre | plane unit normal | capsule segment start (world space) */
    float shape3b[3];         /* capsule segment vector (unused otherwise) */
    float shape1;             /* sphere radius | plane displacement | capsule radius */
    uint32_t body_a, body_b;
    uint64_t collidable_id_a, collidable_id_b;
    float response[3];        /* restitution, static friction, dynamic friction */
    uint32_t reserved;
} ivx_collidable_query;
int ivx_voxel_object_contacts_many(ivx_grid* const* grids, size_t n, const ivx_collidable_query* queries, ivx_contact* out, size_t cap, uint32_t* out_offsets);

/* ---- contacts between two voxel objects (second part) -------------------------------------------------------------
 * VoxelObjectCollisionProbes::recompute_for_all_chunks (collidable.rs:361-392, 451-523, 614-731): per chunk submesh of the current mesh
 * (ivx_remesh), the mesh vertex of the most convex curvature in every block of 8^3 / 4^3 / 2^3 / 1 voxels (block size from the object's smallest
 * occupied extent). The probes stay on the device with the grid and go stale with the mesh. */
int ivx_collision_probes_recompute(ivx_grid*, size_t* n_points);
/* points: 3 floats each (the whole buffer; after a sync it may contain freed ranges), in submesh order then block order after a recompute; chunk_entries:
 * 5 u32 per chunk that has probes (ci, cj, ck, first point, end point) — the reference's chunk_point_ranges, sorted by first point. Either output may be
 * NULL; the counts are always returned. */
/* VoxelObjectCollisionProbes::sync_with_voxel_object_and_mesh (collidable.rs:394-433, 524-612): after ivx_mesh_sync, with the same invalidated chunks —
 * only their probes are picked again; the point buffer keeps its length or grows, a chunk's points go to the best-fitting range freed before or to
 * the end (RangeAllocator); chunks are visited in chunk-linear order (the reference's hash-set order is unpinned). n_points = length of the buffer,
 * freed ranges included. */
int ivx_collision_probes_sync(ivx_grid*, const uint8_t* invalidated_chunks, size_t* n_points);
/* ivx_collision_probes_sync for N objects of one context in merged launches (cf. ivx_mesh_sync_many, whose invalidated sets these are): the select
 * passes of all objects, one wait, the range allocators on the host, the gathers of all objects, one wait. n_points: one length per object. */
int ivx_collision_probes_sync_many(ivx_grid* const* grids, size_t n, const uint8_t* const* invalidated_chunks, size_t* n_points);
int ivx_collision_probes_download(ivx_grid*, float* points, size_t cap_points, uint32_t* chunk_entries, size_t cap_entries, size_t* n_points,
                                  size_t* n_entries);
/* for_each_mutual_voxel_object_contact (collidable.rs:859-1049): the probes of A inside the voxel ranges where the two occupied boxes can overlap
 * (determine_voxel_ranges_encompassing_intersection, object/intersection.rs:706-746) are sampled against B's signed distance field
 * (determine_sdf_value_and_normal_at_point_if_intersecting, collidable.rs:1288-1440), then B's probes against A. rotation (xyzw) + translation =
 * each object's transform_to_object_space (world -> object), center_of_mass_* = derive_center_of_mass() of the object's inertial properties
 * (object space, world units). Every contact hashes [0, i, j, k] of the probing object's voxel with the two collidable ids; normals point from B
 * to A. Both objects need current derived state and current probes, and must belong to the same context. The reference walks the chunks in the
 * iteration order of a hash map (unpinned, see oracle/src/orc_collide.cpp); here they come in submesh order, A's probes first. */
int ivx_mutual_voxel_object_contacts(ivx_grid* a, const float rotation_a[4], const float translation_a[3], const float center_of_mass_a[3], ivx_grid* b,
                                     const float rotation_b[4], const float translation_b[3], const float center_of_mass_b[3],
                                     uint64_t collidable_id_a, uint64_t collidable_id_b, uint32_t body_a, uint32_t body_b, const float response[3],
                                     ivx_contact* out, size_t cap, size_t* n_out);
/* The same for a list of pairs in merged launches with two waits for all (cf. ivx_voxel_object_contacts_many): the pairs the broad phase found
 * this frame. Pair i's manifold is out[out_offsets[i] .. out_offsets[i + 1]) (n + 1 offsets), the list the single-pair call returns. An object
 * may appear in any number of pairs; the probes of every object must be current. */
typedef struct ivx_mutual_query {
    ivx_grid* a;
    ivx_grid* b;
    float rotation_a[4], translation_a[3], center_of_mass_a[3];
    float rotation_b[4], translation_b[3], center_of_mass_b[3];
    uint64_t collidable_id_a, collidable_id_b;
    uint32_t body_a, body_b;
    float response[3];
    uint32_t reserved;
} ivx_mutual_query;
int ivx_mutual_voxel_object_contacts_many(const ivx_mutual_query* queries, size_t n, ivx_contact* out, size_t cap, uint32_t* out_offsets);

#define IVX_KINEMATIC_BODY 0x80000000u
#define IVX_CONTACT_MANIFOLD_START 1u
/* ConstraintSolverConfig (src/constraint/solver.rs:41-57; defaults 8, 0.4, 3, 0.2 at 374-384) */
typedef struct {
    uint32_t n_iterations;
    float old_impulse_weight;
    uint32_t n_positional_correction_iterations;
    float positional_correction_factor;
} ivx_solver_config;
typedef struct {
    uint32_t n_contacts;   /* prepared contacts (after interlock replacement and cache clean-up) */
    uint32_t n_bodies;     /* constrained bodies (touched by >= 1 contact) */
    uint32_t n_levels[2];  /* dependency levels of the velocity and the positional schedule */
    float stage_ms[5];     /* prepare, pre-solve (momenta + velocity sync), solve, write-back + configurations, total */
    uint32_t reserved[3];
} ivx_physics_result;

/* ---- a14: rigid bodies after voxels were removed (impact_voxel/src/interaction.rs:224-602) ----------------------------------------------
 * Host arithmetic, O(1) per object. `moments` are the ten f64 moments of a VoxelObjectInertialPropertyManager about the object's grid origin
 * (ivx_moments.m64 / ivx_region_desc.moments: mass, first moments, moments of inertia, products xy, yz, zx).
 * apply_updated_inertial_properties_to_rigid_body (interaction.rs:405-458; preserve_momentum = 1: ..._preserving_momentum, 460-487): new mass and
 * inertia tensor, position moved by the rotated shift of the local centre of mass, momenta re-synchronised for v + w x shift and the unchanged
 * angular velocity. */
/* VoxelObjectInertialPropertyManager::offset_reference_point_by (object/inertia.rs:257-267): the same moments about the point `offset` (e.g. a fragment's
 * moments from its own grid frame into the parent's: offset = -origin_offset_in_parent * voxel_extent) */
int ivx_offset_reference_point(double moments[10], const float offset[3]);
int ivx_apply_updated_inertial_properties(ivx_rigid_body* body, const double moments[10], const float original_local_center_of_mass[3],
                                          int preserve_momentum, float new_local_center_of_mass[3]);
/* determine_extracted_voxel_object_dynamics (interaction.rs:503-585): `moments` in = the fragment's moments in the PARENT's grid frame (what
 * ivx_split_off_smallest_region reports in `moved`), out = about the fragment's own grid origin (offset_reference_point_by, object/inertia.rs:257-267);
 * fragment_body = DynamicRigidBody::new(mass, inertia, position of its own centre of mass, parent orientation, v + w x shift, w). */
int ivx_extracted_object_dynamics(double moments[10], const uint32_t origin_offset_in_parent[3], float voxel_extent,
                                  const float original_local_center_of_mass[3], const ivx_rigid_body* parent_body, ivx_rigid_body* fragment_body,
                                  float new_local_center_of_mass[3]);
typedef struct {
    ivx_grid* grid; /* the new object; the caller destroys it */
    uint32_t origin_offset_in_parent[3];
    uint32_t reserved;
    ivx_rigid_body body;
    double moments[10]; /* its inertial property manager, about its own grid origin */
    float local_center_of_mass[3];
    float reserved2;
} ivx_extracted_object;
/* handle_voxel_object_after_removing_voxels (interaction.rs:224-403) without the anchor bookkeeping: while the object has disconnected regions the
 * smallest is split off (ivx_split_off_smallest_region), its moments leave `moments` and, if it is a new object, it gets its rigid body from the
 * parent body's state BEFORE this call; finally the parent body takes the remaining inertial properties (momentum re-synchronised unless
 * removed_mass_destroyed is set and nothing was split off). `moments` in = the object's manager after the removal that triggered the call.
 * original_object_empty = the object has fewer than 8 non-empty voxels left (is_effectively_empty, object.rs:803-845); its body is then left as is. */
int ivx_handle_voxel_object_after_removing_voxels(ivx_grid*, const float densities[256], double moments[10], ivx_rigid_body* body,
                                                  const float original_local_center_of_mass[3], int removed_mass_destroyed, ivx_extracted_object* out,
                                                  size_t cap, size_t* n_out, int* original_object_empty, float new_local_center_of_mass[3]);

/* RigidBodyManager + ConstraintManager of one simulation (src/rigid_body.rs:71-78, src/constraint.rs:33-39) */
typedef struct ivx_world ivx_world;
int ivx_world_create(ivx_ctx*, const ivx_solver_config*, ivx_world** out);
void ivx_world_destroy(ivx_world*);
int ivx_world_set_bodies(ivx_world*, const ivx_rigid_body* dynamic, size_t n_dynamic, const ivx_kinematic_body* kinematic, size_t n_kinematic);
int ivx_world_get_bodies(ivx_world*, ivx_rigid_body* dynamic, ivx_kinematic_body* kinematic); /* either may be NULL */
/* The collisions of this step (what CollisionWorld hands to ConstraintManager::prepare_constraints,
 * src/constraint.rs:193-265). Host side: interlock replacement, the ConstraintCache bookkeeping that fixes
 * the solve order and the warm-start source of every contact (solver.rs:386-452), and the dependency
 * schedule that lets the GPU run the reference's sequential sweeps in parallel with identical results. */
int ivx_world_set_contacts(ivx_world*, const ivx_contact*, size_t n, size_t* n_prepared);
/* SphericalJoint constraints (src/constraint/spherical_joint.rs, ConstraintManager::add_spherical_joint src/constraint.rs:183-190): two body
 * references per joint (IVX_KINEMATIC_BODY flag as in ivx_contact). The reference's joint is a placeholder that applies no impulse and no
 * positional correction (spherical_joint.rs:62-88); preparing it only registers its bodies as constrained bodies of the step, whose
 * velocities are written back after the solve — which is all this entry point makes happen. Stays in force until replaced; call it after
 * ivx_world_set_bodies. */
int ivx_world_set_spherical_joints(ivx_world*, const uint32_t* body_pairs, size_t n_joints);
/* perform_physics_step (src/lib.rs:31-110): prepare constraints ->
 * advance momenta -> synchronise velocities, warm start, n_iterations sweeps, positional correction,
 * write back -> advance configurations -> motion drivers at the new simulation time (when a set is installed,
 * ivx_world_set_motion_drivers) -> force generators and dynamic gravity (when either is installed,
 * ivx_world_set_force_generators / ivx_world_set_dynamic_gravity / ivx_world_set_detailed_drag).
 * A world with none of them keeps the total_force / total_torque the host gave its bodies. The stages are also exposed one by one. */
int ivx_world_step(ivx_world*, float dt, ivx_physics_result* out);
/* the same step, only enqueued on the context's stream (no wait, no result): lets the rigid-body step of a frame run
 * behind the voxel step of the same frame with a single wait for both (ivx_voxel_step_collect / ivx_synchronize);
 * the bodies are read back with ivx_world_get_bodies when they are needed */
int ivx_world_step_enqueue(ivx_world*, float dt);
int ivx_world_prepare(ivx_world*);
int ivx_world_advance_momenta(ivx_world*, float dt);
int ivx_world_solve(ivx_world*);
int ivx_world_advance_configurations(ivx_world*, float dt);
/* ContactIDs in solve order and their accumulated (normal, tangent, bitangent) impulses after the last solve */
/* How the solve walks the exact-order schedule. groups = 0 (default): chosen from the schedule — one workgroup with the bodies in LDS when the
 * widest dependency level fits it, else the chain-stationary solve (every chain of contacts keeps one lane of one wave for the whole phase with
 * its prepared contacts and accumulated impulses in registers; only the two bodies' state travels, through version-tagged records; both phases
 * in one launch), else tiles of the level schedule handed to up to 16 workgroups. 1: one workgroup. 2..16: the tile form on that many
 * workgroups. 255: the chain-stationary solve whatever the widths (tests). Same results whichever runs. ivx_world_solver_info: out[0]
 * workgroups used by the last solve, [1..2] levels of the velocity / positional schedule, [3..4] widest level of each, [5] chains (runs of
 * up to 4 contacts of one manifold), [6] contacts, [7] the kernel that ran (0 one workgroup, 1 tiles, 2 chain-stationary). */
int ivx_world_set_solver_groups(ivx_world*, uint32_t groups);
int ivx_world_solver_info(ivx_world*, uint32_t out[8]);
int ivx_world_contact_state(ivx_world*, uint64_t* ids, float* impulses3, size_t cap, size_t* n_out);

/* ---- detailed drag: drag load maps (impact_physics/src/force/detailed_drag.rs, detailed_drag/drag_load.rs, detailed_drag/equirectangular_map.rs) ----
 * The reference computes a map once per static TriangleMesh asset and caches it on disk; here the map comes from a triangle list or from the
 * mesh that is resident on the device, so a voxel object can have one after every bite. */
/* DragLoad: force on the centre of mass and torque about it, without the factors that do not depend on the triangles. 24 bytes. */
typedef struct {
    float force[3];
    float torque[3];
} ivx_drag_load;
/* the numeric fields of DragLoadMapConfig. 16 bytes. ivx_drag_map_config_default fills in 5000 / 64 / 2.0 (DragLoadMapConfig::default). */
typedef struct {
    uint32_t n_direction_samples, n_theta_coords;
    float smoothness;
    uint32_t reserved;
} ivx_drag_map_config;
void ivx_drag_map_config_default(ivx_drag_map_config*);
/* A map is n_theta x 2 n_theta loads, theta-major: cell = theta_idx * n_phi + phi_idx, n_phi = 2 n_theta.
 *
 * Host arithmetic (no device needed):
 * compute_uniformly_distributed_radial_directions (impact_geometry/src/lib.rs:59-91) in f32: z = 1 - 2 i / (n - 1) (the norm is 1 when n = 1),
 * r = sqrt(1 - z z), azimuth i pi (3 - sqrt 5), (r cos, r sin, z) normalised. Deliberate difference: 1 - z z is clamped at 0 (the last z can
 * round to just below -1, which makes the reference's direction NaN). */
int ivx_drag_directions(size_t n, float* dirs3);
/* EquirectangularMap::compute_phi_idx / compute_theta_idx (equirectangular_map.rs:86-98): rem_euclid(2 pi), theta above pi folded back,
 * floor(angle * (1 / cell)) with cell = pi / n_theta, theta clamped to n_theta - 1. Deliberate difference: phi is clamped to n_phi - 1 as
 * well (the reference indexes one past the row when the remainder of a tiny negative angle rounds to 2 pi). */
int ivx_drag_map_indices(uint32_t n_theta, float phi, float theta, uint32_t* phi_idx, uint32_t* theta_idx);
/* DetailedDragForce::apply + DragLoad::compute_world_space_drag_force_and_torque (detailed_drag.rs:200-243, drag_load.rs:42-67): v = momentum /
 * mass relative to the medium, s2 = |v_rel|^2; nothing happens when s2 <= 0; else the map cell at the body-space direction of v_rel (phi =
 * atan2(y, x), theta = acos z) scaled by fs = scaling^2 rho C_d s2 (torque: scaling fs), rotated to world space and ADDED to the body's
 * total_force / total_torque. */
int ivx_drag_force_and_torque(const ivx_drag_load* map, uint32_t n_theta, ivx_rigid_body* body, const float medium_velocity[3],
                              float medium_mass_density, float drag_coefficient, float scaling);
/* Device entry points (HIP kernels, drag.hip). Per triangle (drag_load.rs:212-245): c = e1 x e2, kept only if |c| > f32::EPSILON; normal = c / |c|,
 * area = |c| / 2, centre = (v1 + v2 + v3) / 3. Load of a direction d (drag_load.rs:174-208): over the triangles with cos = d . n > 0,
 * force += -(cos area) n, torque += (centre - com) x that force. f32 products, sums of 128 triangles in f32, everything above that in f64 in a
 * fixed order: results do not depend on timing (no float atomics). All arrays are host arrays.
 * ivx_drag_loads_triangles: a caller's triangle list (n_indices a multiple of 3, every index < n_vertices; an empty list gives zero loads).
 * ivx_drag_loads: the grid's resident mesh — the triangles of the live submeshes only (index_offset .. + index_count of every entry of the
 * submesh table; after ivx_mesh_sync the buffers also hold freed ranges with stale triangles). IVX_ERR_STATE without a current mesh. */
int ivx_drag_loads_triangles(ivx_ctx*, const float* positions3, size_t n_vertices, const uint32_t* indices, size_t n_indices, const float com[3],
                             const float* dirs3, size_t n_dirs, ivx_drag_load* out);
int ivx_drag_loads(ivx_grid*, const float com[3], const float* dirs3, size_t n_dirs, ivx_drag_load* out);
/* generate_map_from_drag_loads (detailed_drag.rs:401-471, equirectangular_map.rs:108-160), the smoothing stage alone. For sample s in order:
 * scaled = distance / (1 - 0.75 |d.z|), ext = max(scaled, cell / 2), n_across = ceil(2 ext / cell); rows theta_k = theta_s - ext + cell / 2 +
 * k cell, columns the same in phi, cell indices by ivx_drag_map_indices; angular distance = acos(sin theta_s sin theta_k + cos theta_s cos theta_k
 * cos(phi_j - phi_s)); w = max(0, 1 - (distance / scaled)^2)^2; the cell accumulates w load and w, every hit counting (near the poles a sample
 * meets a cell several times); afterwards each cell is sum / weight where weight > 0. One lane per cell gathers the samples in order, rows before
 * columns: the reference's summation order. Deliberate differences: the acos argument is clamped to [-1, 1] (the reference lets 1 + ulp become
 * NaN and then weight 0), and a distance above pi is refused (the region would wrap the map several times over). */
int ivx_drag_load_map_from_samples(ivx_ctx*, const float* dirs3, const ivx_drag_load* loads, size_t n, uint32_t n_theta,
                                   float angular_interpolation_distance, ivx_drag_load* map);
/* DragLoadMap::compute_from_mesh (detailed_drag.rs:362-398) over the resident mesh: directions, loads and map in one call, the samples never
 * leaving the device; angular_interpolation_distance = smoothness sqrt(4 pi / n_direction_samples). */
int ivx_drag_load_map(ivx_grid*, const float com[3], const ivx_drag_map_config*, ivx_drag_load* map);

/* ---- chunk culling: indirect draw arguments for all objects and views of a frame (impact_voxel/shaders/compute/voxel_chunk_culling.template.wgsl,
 * impact_voxel/src/render_commands.rs:392-598, mesh.rs:128-131, 638-696) ----
 * The reference records one dispatch with push constants and a bind group per object per view; here ONE call culls every chunk submesh of every
 * object against every view and leaves a region of draw arguments per view in a context-owned device buffer (csrc/cull.hip). */
/* CullingFrustum + the shader's instanceIdx (its push-constant block without chunkCount), in NORMALISED OBJECT SPACE: chunk extent 1, the lower
 * corner of chunk (i, j, k) at (i, j, k). planes: unit normal xyz, displacement. most_inside_corners: the low three bits select the corner, bit 2 / 1 / 0
 * = upper x / y / z (AxisAlignedBox::corner, the shader's CORNERS_OFFSETS). 136 bytes. */
typedef struct {
    float planes[6][4];
    uint32_t most_inside_corners[6];
    float apex[3];
    uint32_t instance_idx;
} ivx_culling_frustum;
#define IVX_CULL_VIEW_INDEXED 1u /* ivx_cull_view.flags: the view's pass draws indexed (shadow passes; the geometry pass does not) */
/* One view of the frame, in view space. kind 0: a frustum with its apex at the origin, the six planes in the order of Frustum (left, right, bottom,
 * top, near, far; unit normal xyz, displacement). kind 1: an orthographic frustum as an oriented box (centre, orientation quaternion xyzw, half
 * extents) looking along its negative depth axis, the apex emulated `apex_distance` chunks behind the centre (the reference passes 10 000).
 * 152 bytes. */
typedef struct {
    uint32_t kind, flags;
    float planes[6][4];
    float box_center[3];
    float box_orientation[4];
    float box_half_extents[3];
    float apex_distance;
    uint32_t reserved;
} ivx_cull_view;
#define IVX_CULL_PAIR_SKIP 1u /* ivx_cull_pair.flags: the object is not visible in this view, every one of its slots is culled */
/* One (view, object) pair, view-major (pair v * n_objects + o): the object-to-view similarity (rotation quaternion xyzw, translation, scaling), the
 * instance index the view's draws of this object carry, flags. 40 bytes. */
typedef struct {
    float rotation[4];
    float translation[3];
    float scaling;
    uint32_t instance_idx, flags;
} ivx_cull_pair;
/* Added to what the submesh says: 0 / 0 for per-object buffers, the object's arena offsets for a pooled renderer. 8 bytes. */
typedef struct {
    uint32_t first_index_base;
    int32_t base_vertex;
} ivx_cull_object;
/* wgpu's DrawIndirectArgs (the shader's non-indexed layout: index_count is `vertex_count`, first_index is `first_vertex`). 16 bytes. */
typedef struct {
    uint32_t index_count, instance_count, first_index, first_instance;
} ivx_draw_args;
/* wgpu's DrawIndexedIndirectArgs. 20 bytes. */
typedef struct {
    uint32_t index_count, instance_count, first_index;
    int32_t base_vertex;
    uint32_t first_instance;
} ivx_draw_indexed_args;
/* Where a view's region lies in the argument buffer: byte offset, 16 or 20 bytes per slot, slots (the submeshes of all objects). 16 bytes. */
typedef struct {
    uint64_t offset;
    uint32_t stride, n_slots;
} ivx_cull_region;
/* A view's record in the count buffer: draws (what multi_draw_indirect_count reads) and the sum of their index counts (mod 2^32). 8 bytes. */
typedef struct {
    uint32_t draws, indices;
} ivx_cull_count;
/* The derivation, host arithmetic (the device runs the same function and gives the same bytes): T = inverse of the similarity with its scaling
 * multiplied by chunk_extent (16 x the voxel extent); kind 0: every plane through Plane::transformed (point n d through T, normal through T's
 * rotation, displacement n' . p'), apex = T's translation; kind 1: the box through OrientedBox::transformed, planes in the order and with the signs of
 * compute_bounding_planes, apex = centre + apex_distance x depth axis; most_inside_corners[p]: bit 2 / 1 / 0 set where the normal's x / y / z does
 * NOT have its sign bit set. A restatement in f32 with a fixed operation order, not a bit-parity target (glam's is unpinned).
 * IVX_ERR_INVALID for a kind other than 0 / 1 and for a chunk_extent or scaling that is not positive. */
int ivx_culling_frustum_from_view(const ivx_cull_view*, const ivx_cull_pair*, float chunk_extent, ivx_culling_frustum* out);
/* The decision, per submesh s of object o under view v, from the record f of (v, o): with p = float(chunk_indices) + corner offset, plane q culls
 * when ((nx px + ny py) + nz pz) - d < -0.05f (strict, f32, no contraction); the chunk is obscured when is_obscured_from_direction[ix][iy][iz] > 0
 * with i* = (lower + 0.5 - apex).* < 0 ? 1 : 0; a NaN compares false both times (drawn). Culled = frustum-culled, or obscured, or IVX_CULL_PAIR_SKIP.
 * Slots: base[o] = exclusive prefix of the objects' submesh counts in call order, slot base[o] + s belongs to submesh s of object o; a view's
 * region holds that many slots of 16 or 20 bytes (IVX_CULL_VIEW_INDEXED); out_layout[v] says where it starts.
 * mode 0, zeroed in place (the reference's semantics): every slot is written; a drawn chunk gets index_count, instance_count 1, first_index =
 *   index_offset + first_index_base, base_vertex, first_instance = instance_idx; a culled one the same with index_count = instance_count = 0
 *   (the reference leaves the other fields stale).
 * mode 1, compacted: the drawn entries dense from slot 0 in (object, submesh) order, every slot from the count on all zero.
 * Both modes leave counts[v] in the count buffer. No atomics decide anything: two calls leave the same bytes.
 * At most 64 views per call (IVX_ERR_INVALID above); n_objects == 0 or n_views == 0 succeeds with empty regions.
 *   (ivx_cull_many* with n == 0, a frame without voxel objects, touch no context: out_layout gets offset 0, the view's stride and 0 slots, out_counts
 *   zeros, from the call itself; ivx_cull_download / ivx_cull_collect keep describing the context's last call that had objects or used the context.)
 * A call that fails leaves nothing to download (ivx_cull_download then refuses every view).
 * ivx_cull_submesh_tables: host tables, uploaded for the call (counts[o] entries each), chunk_extents[o] per object.
 * ivx_cull_many: the grids' RESIDENT submesh tables, the live mesh_counts.n_submeshes entries (what ivx_mesh_sync keeps current); chunk extent = 16 x
 *   the grid's voxel extent; `objects` may be NULL (all zero); a grid without a current mesh is IVX_ERR_STATE, a current mesh without submeshes
 *   contributes no slot. ivx_cull_many_enqueue does not wait and reads nothing back (the consumer is on the device); ivx_cull_collect waits and copies
 *   the counts of the last call's views; ivx_cull_many is both.
 * The *_frusta forms take ready records (frusta[v * n_objects + o], what VoxelChunkCullingPass::record computes today) with view_flags[v] and
 *   pair_flags[v * n_objects + o] (may be NULL) in place of views and pairs.
 * ivx_cull_frusta: the derivation stage alone on the device, records[v * n_objects + o] back to the host.
 * ivx_cull_download: one view's region (args_bytes >= n_slots x stride), its count record and its n_objects frustum records of the last call; each
 *   may be NULL.
 * ivx_cull_device_ptr: the argument buffer, the count buffer (64 records), the frustum records of the last call. The buffers belong to the context,
 *   only grow (a pointer is stale after a call that needed more) and go with ivx_shutdown. Export as ipc / dma-buf handles (cf. ivx_mesh_export) is
 *   not provided yet: this pointer is the hand-off. */
#define IVX_CULL_ZEROED 0u
#define IVX_CULL_COMPACTED 1u
#define IVX_CULL_PTR_ARGS 0
#define IVX_CULL_PTR_COUNTS 1
#define IVX_CULL_PTR_FRUSTA 2
int ivx_cull_frusta(ivx_ctx*, const ivx_cull_view* views, size_t n_views, const ivx_cull_pair* pairs, const float* chunk_extents, size_t n_objects,
                    ivx_culling_frustum* out);
int ivx_cull_submesh_tables(ivx_ctx*, const ivx_submesh* const* tables, const uint32_t* counts, size_t n_objects, const ivx_cull_object* objects,
                            const float* chunk_extents, const ivx_cull_view* views, size_t n_views, const ivx_cull_pair* pairs, uint32_t mode,
                            ivx_cull_region* out_layout, ivx_cull_count* out_counts);
int ivx_cull_submesh_tables_frusta(ivx_ctx*, const ivx_submesh* const* tables, const uint32_t* counts, size_t n_objects, const ivx_cull_object* objects,
                                   const ivx_culling_frustum* frusta, const uint32_t* view_flags, const uint32_t* pair_flags, size_t n_views, uint32_t mode,
                                   ivx_cull_region* out_layout, ivx_cull_count* out_counts);
int ivx_cull_many(ivx_grid* const* grids, size_t n, const ivx_cull_object* objects, const ivx_cull_view* views, size_t n_views, const ivx_cull_pair* pairs,
                  uint32_t mode, ivx_cull_region* out_layout, ivx_cull_count* out_counts);
int ivx_cull_many_enqueue(ivx_grid* const* grids, size_t n, const ivx_cull_object* objects, const ivx_cull_view* views, size_t n_views,
                          const ivx_cull_pair* pairs, uint32_t mode, ivx_cull_region* out_layout);
int ivx_cull_collect(ivx_ctx*, ivx_cull_count* out_counts, size_t n_views);
int ivx_cull_many_frusta(ivx_grid* const* grids, size_t n, const ivx_cull_object* objects, const ivx_culling_frustum* frusta, const uint32_t* view_flags,
                         const uint32_t* pair_flags, size_t n_views, uint32_t mode, ivx_cull_region* out_layout, ivx_cull_count* out_counts);
int ivx_cull_download(ivx_ctx*, uint32_t view, void* args, size_t args_bytes, ivx_cull_count* count, ivx_culling_frustum* frusta, size_t n_frusta);
void* ivx_cull_device_ptr(ivx_ctx*, int which);

/* ---- bounding volumes: world boxes, all intersecting pairs, region queries (impact_intersection/src/lib.rs IntersectionManager;
 * impact_geometry/src/axis_aligned_box.rs, sphere.rs, frustum.rs, oriented_box.rs; impact_physics/src/collision.rs:215-349) ----
 * What the batched calls above take as input and nothing else here produced: the pairs of ivx_*_contacts_many (ivx_bv_pairs), the objects an absorber
 * touches (ivx_bv_queries with a box or a sphere), the per-(view, object) IVX_CULL_PAIR_SKIP bit (ivx_bv_queries with frusta / oriented boxes).
 * Two forms of the pair pass that leave the same bytes: the exact upper triangle (the reference's own `_brute_force` form, csrc/bvol.hip; the
 * default everywhere) and a linear hierarchy built over the set on request (ivx_bv_build_hierarchy, csrc/bvh.hip; further down). Region queries
 * have the same two forms with the same bytes (ivx_bv_queries, the default; ivx_bv_queries_hierarchy), and their masks become hit lists on the
 * device (ivx_bv_query_lists). */
/* AxisAlignedBoxC. 24 bytes. */
typedef struct {
    float lower[3], upper[3];
} ivx_aabb;
/* A model-to-world similarity: rotation quaternion xyzw, translation, scaling — the leading fields of ivx_cull_pair, with the same meaning. 32 bytes. */
typedef struct {
    float rotation[4];
    float translation[3];
    float scaling;
} ivx_similarity;
/* CollidableKind (ivx_bv_set's `kinds`; NULL: all dynamic) */
#define IVX_BV_DYNAMIC 0u
#define IVX_BV_STATIC 1u
#define IVX_BV_PHANTOM 2u
/* ivx_bv_query.kind */
#define IVX_BV_QUERY_BOX 0u
#define IVX_BV_QUERY_SPHERE 1u
#define IVX_BV_QUERY_FRUSTUM 2u
#define IVX_BV_QUERY_ORIENTED_BOX 3u
/* One region of world space. 128 bytes: the kind, then 31 words of which the kind's member uses the leading ones (the rest is ignored).
 * frustum: planes in world space (unit normal xyz, displacement) and per plane the box corner with the largest signed distance, in the convention of
 * ivx_culling_frustum.most_inside_corners (bit 2 / 1 / 0 = upper x / y / z); ivx_bv_frustum_query fills both.
 * oriented_box: axes[a] = row a of the rotation from world space into the box frame, the box's centre in world space, its half extents. */
typedef struct {
    uint32_t kind;
    union {
        struct {
            float lower[3], upper[3];
        } box;
        struct {
            float center[3], radius;
        } sphere;
        struct {
            float planes[6][4];
            uint32_t corners[6];
        } frustum;
        struct {
            float axes[3][3], center[3], half_extents[3];
        } oriented_box;
        uint32_t words[31];
    } u;
} ivx_bv_query;
/* add_bounding_volume_to_hierarchy (lib.rs:39-54) = aabb_of_transformed (axis_aligned_box.rs:350-363) of the model box under the similarity's matrix.
 * Host arithmetic; the device runs the same function and gives the same bytes. All f32, this order, no contraction:
 *   c = 0.5 (lower + upper), h = 0.5 (upper - lower)                                        (center_of, half_extents)
 *   with q = rotation: n2 = ((x x + y y) + z z) + w w, and the nine numerators of the homogeneous rotation matrix
 *     N00 = ((w w + x x) - y y) - z z   N01 = 2 (x y - w z)             N02 = 2 (x z + w y)
 *     N10 = 2 (x y + w z)               N11 = ((w w - x x) + y y) - z z N12 = 2 (y z - w x)
 *     N20 = 2 (x z - w y)               N21 = 2 (y z + w x)             N22 = ((w w - x x) - y y) + z z
 *   M[i][j] = scaling (N[i][j] / n2)      (IEEE division: a quaternion that is unit only to rounding gives an exact 0 / 1 where the rotation has one)
 *   c'[i] = ((M[i][0] c.x + M[i][1] c.y) + M[i][2] c.z) + translation[i],   h'[i] = (|M[i][0]| h.x + |M[i][1]| h.y) + |M[i][2]| h.z
 *   out = (c' - h', c' + h').
 * The identity similarity returns the box's own bytes whenever lower + upper and upper - lower are exact in f32 (the operation order of the reference,
 * which has the same property); a restatement, not a bit-parity target (glam's order is unpinned).
 * IVX_ERR_INVALID for a scaling that is not positive (a NaN included). */
int ivx_bv_world_aabb(const ivx_aabb* model, const ivx_similarity* similarity, ivx_aabb* out);
/* A kind-2 record from six world-space planes: corners[p] has bit 2 / 1 / 0 set where the normal's x / y / z does NOT have its sign bit set
 * (-0.0 chooses the lower corner); the words behind `corners` are zeroed. */
int ivx_bv_frustum_query(const float planes[6][4], ivx_bv_query* out);
/* VoxelObject::compute_aabb (object.rs:886-907) as sync_voxel_object_bounding_volume stores it (interaction.rs:202-222): voxel_extent x (start, end)
 * of the occupied voxel ranges THE OBJECT CURRENTLY HOLDS — what ivx_occupied_ranges, a step, a split or a clip last left, refreshed first if an edit
 * that removed a chunk has invalidated them (the reference refreshes at that point) —, as float(start) x extent, float(end) x extent; the all-zero
 * box when a range is empty. An edit that empties voxels without making a chunk Void leaves the ranges, and so the box, as they were — even when
 * no voxel is left — until ivx_occupied_ranges is called, as in the reference. IVX_ERR_STATE when the grid holds no ranges yet (nothing has
 * derived its state). */
int ivx_grid_model_aabb(ivx_grid*, ivx_aabb* out);
/* The set of a context: n world boxes with their kinds, resident until the next ivx_bv_set* on the context.
 * ivx_bv_set: one upload from pinned staging, one launch (ivx_bv_world_aabb per object, and the box of every 64 consecutive objects) and one wave
 *   for the total; similarities == NULL: the boxes are in world space already and are stored as given. kinds == NULL: all IVX_BV_DYNAMIC. Refused
 *   (IVX_ERR_INVALID): a kind above 2, a scaling that is not positive; IVX_ERR_CAPACITY: n above IVX_BV_MAX_OBJECTS. n == 0 is a set (an empty
 *   one). A refused call leaves the context's set as it was; a call that fails later leaves none.
 * ivx_bv_set_grids: the same with model boxes from ivx_grid_model_aabb of every grid (one context); inside an ivx_many_begin bracket what has been
 *   recorded is flushed first, as by ivx_cull_many. n == 0 names no context and does nothing.
 * ivx_bv_download: the world boxes (cap >= n, else IVX_ERR_CAPACITY; may be NULL) and `total`, the box around all of them (total_bounding_volume:
 *   per component the minimum of the lowers and the maximum of the uppers, reduced 64 objects at a time in input order; the all-zero box for n == 0;
 *   may be NULL).
 * ivx_bv_pairs: every (a, b), a < b, whose world boxes intersect, as uint32_t[2], SORTED LEXICOGRAPHICALLY BY (a, b) — an order of our own (the
 *   reference's is an artefact of its tree) that no tiling shows through. mode 0: all pairs (cache_all_collisions); mode 1: only pairs with no phantom
 *   member and at least one dynamic member (collision.rs:317-349). *n_out is the number found even when it exceeds cap; the call then returns
 *   IVX_ERR_CAPACITY and writes nothing to `pairs`. The pairs also stay in the context's pair buffer; pairs == NULL with cap == 0 leaves them there
 *   only (the call succeeds). 2^31 pairs or more: IVX_ERR_CAPACITY. Device scratch: 4 n ceil(n / 512) bytes.
 * ivx_bv_queries: masks[q * W + w], W = ceil(n / 64): bit o % 64 of word o / 64 set when object o is hit by query q, bits past n zero; counts[q] the
 *   number hit (may be NULL). At most IVX_BV_MAX_QUERIES per call; a kind above 3 is IVX_ERR_INVALID. The masks also stay in the context's mask buffer.
 * ivx_bv_device_ptr: the world boxes (ivx_aabb[n]), the pair buffer (uint32_t[2] per pair of the last ivx_bv_pairs), the masks of the last
 *   ivx_bv_queries. Context-owned and grow-only, under the rules ivx_cull_device_ptr documents. NULL before the first call that fills the buffer.
 * Every call that produces results (download, pairs, queries) without a set on the context is IVX_ERR_STATE; n == 0 / n_queries == 0 succeed with
 * empty results.
 * The decisions — f32, this order, no contraction; d(x) below means "x has its sign bit set, or is a NaN":
 *   box against box (pairs, kind 0; box_lies_outside, axis_aligned_box.rs:619-623): outside when d() holds for any component of
 *     other.upper - self.lower or of self.upper - other.lower. The sign bit of the difference, not a `<`: touching faces intersect, and
 *     (-0.0) - (+0.0) = -0.0 does not. A box with a NaN bound intersects nothing.
 *   sphere (sphere.rs:167-181): s = 0; per axis x, y, z: if upper < c then s += (c - upper)^2, else if lower > c then s += (lower - c)^2; outside when
 *     s > radius x radius. A NaN compares false each time (a NaN bound adds nothing; a NaN sum or radius is a hit).
 *   frustum (frustum.rs:456-471): hit when ((nx px + ny py) + nz pz) - d >= 0 for all six planes, p the box corner corners[p] selects. A NaN is a miss.
 *   oriented box (oriented_box.rs:129-143), c and h of the world box as in ivx_bv_world_aabb, dx = c - center:
 *     e[a] = ((|A[a][0]| h.x + |A[a][1]| h.y) + |A[a][2]| h.z) + half[a],  l[a] = (A[a][0] dx.x + A[a][1] dx.y) + A[a][2] dx.z;
 *     hit when d(e[a] - |l[a]|) holds for no a. A NaN is a miss.
 * No atomic decides anything: two calls leave the same bytes. */
#define IVX_BV_MAX_OBJECTS (1u << 20)
#define IVX_BV_MAX_QUERIES 1024u
#define IVX_BV_ALL_PAIRS 0u
#define IVX_BV_DYNAMIC_PAIRS 1u
#define IVX_BV_PTR_WORLD_BOXES 0
#define IVX_BV_PTR_PAIRS 1
#define IVX_BV_PTR_MASKS 2
int ivx_bv_set(ivx_ctx*, const ivx_aabb* model_boxes, const ivx_similarity* similarities, const uint32_t* kinds, size_t n);
int ivx_bv_set_grids(ivx_grid* const* grids, size_t n, const ivx_similarity* similarities, const uint32_t* kinds);
int ivx_bv_download(ivx_ctx*, ivx_aabb* world_boxes, size_t cap, ivx_aabb* total);
int ivx_bv_pairs(ivx_ctx*, uint32_t mode, uint32_t* pairs, size_t cap, size_t* n_out);
int ivx_bv_queries(ivx_ctx*, const ivx_bv_query* queries, size_t n_queries, uint64_t* masks, uint32_t* counts);
void* ivx_bv_device_ptr(ivx_ctx*, int which);

/* The hierarchy over the context's set (hierarchy.rs, built by hierarchy/fast_bottom_up.rs in the reference; here a linear BVH in Morton order with
 * Karras's construction — the reference's tree shape is an artefact of its clustering and is not reproduced). csrc/bvh.hip; the host functions run
 * the very functions the kernels run and give the same bytes. All f32, this order, no contraction.
 * FRAME. A box is UNBOUNDED when one of its bounds has magnitude >= 1e30f (a plane's +-FLT_MAX box is). The frame is the union of the world boxes
 *   that have no NaN bound and are not unbounded, minima and maxima taken in the total order of the bit patterns (order_min / order_max: -0.0 below
 *   +0.0); the all-zero box when no world box qualifies.
 * KEY (ivx_bv_morton_key). For a box with no NaN bound that is not unbounded, per axis: c = 0.5f (lower + upper),
 *   t = (c - frame.lower) / (frame.upper - frame.lower), q = t < 1 ? (uint32_t)(t 1024.0f) : 1023; a t that is not greater than zero — a NaN, which a
 *   zero-extent axis gives, included — gives q = 0. code = the 30-bit interleave of qx, qy, qz, x above y above z (bit 3 k + 2 / + 1 / + 0 = bit k of
 *   qx / qy / qz). A NaN-bounded or unbounded box gets the code 0x3FFFFFFF. key = (code << 32) | index: unique, ties in the code fall in index
 *   order, and the tree is never deeper than 50 (30 code bits, 20 index bits).
 * LEAVES. leaf_objects[p] is the object at Morton position p, in ascending key order. A leaf's box is its object's world box, except for an object
 *   with a NaN bound: its leaf box is the neutral box (lower = +inf, upper = -inf), which meets nothing and adds nothing to a union.
 * NODES. For n >= 2 there are n - 1 internal nodes, node 0 the root. Node i is Karras's node i over the sorted keys: with
 *   delta(i, j) = clz(key_i ^ key_j) over the 64 bits, -1 when j lies past either end, its direction is the sign of delta(i, i + 1) - delta(i, i - 1),
 *   its range the longest run in that direction whose delta exceeds delta(i, i - d), its split the last position whose delta exceeds the range's
 *   own. left / right name an internal node by its index or a leaf by IVX_BV_LEAF | position. A node's box is the union of its two children's boxes
 *   in the bit order above — the order of the flat form's block boxes, for its reason: under the sign-bit decision an fminf union could reject a
 *   member pair that intersects. n == 1: no nodes (*n_nodes = 0), leaf_objects[0] = 0. n == 0: nothing.
 * ivx_bv_hierarchy_host: all of the above on the host for n world boxes (n <= IVX_BV_MAX_OBJECTS, else IVX_ERR_CAPACITY): nodes[n - 1],
 *   leaf_objects[n], *frame (may be NULL). nodes may be NULL for n < 2, leaf_objects for n == 0.
 * ivx_bv_build_hierarchy: the same over the context's set on its stream, nothing waits: frame, keys, a stable radix sort of the code bits (8 bits a
 *   pass, no atomic decides a position), a lane per node, and the boxes from the leaves up — a workgroup hands a box to another through an
 *   agent-scope release, a per-node ticket and an agent-scope acquire; the second arriver carries on, nobody waits, and the union does not depend
 *   on who came first: two builds leave the same bytes.
 * STATE. A hierarchy belongs to the set it was built from: after a new ivx_bv_set* (or ivx_cw_synchronize) ivx_bv_hierarchy_download and
 *   ivx_bv_pairs_hierarchy return IVX_ERR_STATE until ivx_bv_build_hierarchy has run again; without a set all three do. Inside an ivx_many_begin
 *   bracket what has been recorded is flushed first, as by ivx_bv_pairs.
 * ivx_bv_hierarchy_download: nodes (node_cap >= n - 1) and leaf objects (leaf_cap >= n), else IVX_ERR_CAPACITY; either may be NULL; *n_nodes (may be
 *   NULL). ivx_bv_device_ptr(IVX_BV_PTR_NODES / _LEAF_OBJECTS) names the resident arrays (NULL without a current hierarchy of two objects or more).
 * ivx_bv_pairs_hierarchy: THE CONTRACT AND THE BYTES OF ivx_bv_pairs — modes 0 and 1, (a, b) with a < b as object indices sorted lexicographically,
 *   *n_out beyond cap: IVX_ERR_CAPACITY and nothing written, pairs == NULL with cap == 0, 2^31 pairs or more: IVX_ERR_CAPACITY; the result also stays
 *   in the context's pair buffer (IVX_BV_PTR_PAIRS). A lane per leaf position p walks the tree to the right of p: a subtree is entered when its box
 *   does not lie outside the lane's (the box decision above) — a subtree whose leaf range ends at or before p is never entered, so each pair is
 *   found once, from its lower position; at a leaf the mode's kind filter applies. The walk runs twice (count, scan, the call's one wait, emit) and
 *   the pairs are then brought into (a, b) order by the same radix sort. A walk visits at most 2 n - 1 nodes and stops there: a hierarchy that is
 *   inconsistent ends the call with IVX_ERR_STATE and a message. Device scratch: O(n) for the tree, 8 bytes per pair for the sort.
 * ivx_cw_set_broad_phase (a collision world, below): IVX_CW_BROAD_FLAT (the default) or IVX_CW_BROAD_HIERARCHY; any other value is IVX_ERR_INVALID
 *   and leaves the setting as it was. With the hierarchy, ivx_cw_collide builds it over the set ivx_cw_synchronize installed and takes its pairs
 *   from the tree; contacts and deferred pairs are the same bytes under both settings.
 * ivx_bv_queries_hierarchy: THE CONTRACT AND THE BYTES OF ivx_bv_queries — the same masks (bits past n zero), counts, limits and refusals, the masks
 *   left in the context's mask buffer (IVX_BV_PTR_MASKS); n == 0 and n_queries == 0 as there. State as ivx_bv_pairs_hierarchy: IVX_ERR_STATE
 *   without a set or without a hierarchy of the current set; a bracket is flushed first; a walk past its 2 n steps ends the call with
 *   IVX_ERR_STATE and a message. A workgroup per query: it expands the top of the tree until it holds 256 subtrees or more, then a lane walks
 *   each without a stack. A leaf is decided by the decisions above on its object's world box; a hit is an OR into the mask, which the call
 *   zeroes first: two calls leave the same bytes. n == 1 has no nodes: the one object is decided directly.
 *   A NODE IS SKIPPED only if no leaf under it can be hit by those decisions in f32 (DESIGN.md section 4 has the arguments). This holds for
 *   PROPER boxes, lower <= upper on every axis, which a node's box contains bound by bound. An IRREGULAR object — a NaN bound (the sphere decision
 *   hits it), or lower > upper on an axis (a set stored as given may hold one) — is left out by the walk and decided by every query directly;
 *   the build keeps their list. With nb the node's box:
 *     box:      skipped when nb lies outside the query (the box decision above, self = the query).
 *     sphere:   the sphere expression on nb; skipped when s > radius x radius. A NaN compares false: entered.
 *     frustum:  not the leaf expression — corners[] is the caller's, and an unbounded member gives inf - inf. Per plane p and axis k
 *               m[k] = the larger of n[k] nb.lower[k] and n[k] nb.upper[k], a NaN if either is; skipped when ((m[0] + m[1]) + m[2]) - d < 0 for
 *               some plane. A NaN: entered.
 *     oriented: evaluated in f64 — e - |l| is not monotone in the box under f32 rounding. With H = 0.5 (nb.upper - nb.lower),
 *               dc = 0.5 (nb.lower + nb.upper) - center, M[k] = max(|nb.lower[k]|, |nb.upper[k]|), D[k] = |dc[k]| + H[k], per axis a of the query
 *               E = sum_k |A[a][k]| H[k] + half[a], L = sum_k A[a][k] dc[k], S = sum_k |A[a][k]| (D[k] + M[k]) + |half[a]|:
 *               skipped when |L| - E > 16 (2^-24 S + (sum_k |A[a][k]| + 1) 2^-126) for some a, provided S < 2^120 and
 *               M[k] + |center[k]| < 2^120 for every k. A NaN: entered.
 *   ivx_bv_query_skips_boxes: that decision for every query and every box, on the host (skips[q * n_boxes + b] = 1: skipped).
 * ivx_bv_queries_hierarchy_host: the same over a tree of the caller's (ivx_bv_hierarchy_host's output, say), with the same decision functions, on
 *   the host; n above IVX_BV_MAX_OBJECTS or n_queries above IVX_BV_MAX_QUERIES: IVX_ERR_CAPACITY; a tree that is none (a child out of range, a
 *   walk past 2 n steps): IVX_ERR_STATE. nodes may be NULL for n < 2.
 * ivx_bv_query_lists: the hit lists of the context's last queries call (either form), expanded on the device from the resident masks: a popcount per
 *   mask word, a prefix per query and over the queries, then every word emits its objects — no sort, no atomic. offsets[n_queries + 1] (may be
 *   NULL); query q's objects are objects[offsets[q] .. offsets[q + 1]) in ascending object index. *n_out is the total even when it exceeds cap; the
 *   call then returns IVX_ERR_CAPACITY and writes nothing. objects == NULL with cap == 0 leaves the lists on the device only:
 *   ivx_bv_device_ptr(IVX_BV_PTR_HIT_OFFSETS / _HIT_OBJECTS) names them (NULL until a call has made them, and again after the next queries call
 *   or set). IVX_ERR_STATE when no queries call with n_queries > 0 has run since the last set, or when the set is empty. */
#define IVX_BV_LEAF 0x80000000u /* child reference: bit 31 set = leaf, low bits = leaf position in Morton order */
typedef struct {
    float lower[3], upper[3];
    uint32_t left, right;
} ivx_bv_node; /* 32 bytes */
#define IVX_BV_PTR_NODES 3
#define IVX_BV_PTR_LEAF_OBJECTS 4
#define IVX_CW_BROAD_FLAT 0u
#define IVX_CW_BROAD_HIERARCHY 1u
int ivx_bv_morton_key(const ivx_aabb* frame, const ivx_aabb* box, uint32_t index, uint64_t* key);
int ivx_bv_hierarchy_host(const ivx_aabb* world, size_t n, ivx_bv_node* nodes, uint32_t* leaf_objects, ivx_aabb* frame);
int ivx_bv_build_hierarchy(ivx_ctx*);
int ivx_bv_hierarchy_download(ivx_ctx*, ivx_bv_node* nodes, size_t node_cap, uint32_t* leaf_objects, size_t leaf_cap, size_t* n_nodes);
int ivx_bv_pairs_hierarchy(ivx_ctx*, uint32_t mode, uint32_t* pairs, size_t cap, size_t* n_out);
#define IVX_BV_PTR_HIT_OFFSETS 5
#define IVX_BV_PTR_HIT_OBJECTS 6
int ivx_bv_queries_hierarchy(ivx_ctx*, const ivx_bv_query* queries, size_t n_queries, uint64_t* masks, uint32_t* counts);
int ivx_bv_queries_hierarchy_host(const ivx_aabb* world, size_t n, const ivx_bv_node* nodes, const uint32_t* leaf_objects, const ivx_bv_query* queries, size_t n_queries,
                                  uint64_t* masks, uint32_t* counts);
int ivx_bv_query_skips_boxes(const ivx_bv_query* queries, size_t n_queries, const ivx_aabb* boxes, size_t n_boxes, uint8_t* skips);
int ivx_bv_query_lists(ivx_ctx*, uint32_t* offsets, uint32_t* objects, size_t cap, size_t* n_out);
int ivx_cw_set_broad_phase(ivx_world*, uint32_t which);

/* ---- frame instances: kept sets, view transforms and cull pairs of every view of a frame (BufferModelInstancesAndBoundLights, engine/src/tasks.rs:779:
 * impact_scene/src/model.rs:171-297 buffer_model_instances_for_rendering; impact_scene/src/light.rs:85-284, 383-450, 465-641, 747-787, 827-848
 * bound_*_lights_and_buffer_shadow_casting_model_instances; impact_geometry/src/axis_aligned_box.rs:208-239; impact_math/src/transform/similarity.rs:278-284) ----
 * The reference loops per view over the hits of a region query: it filters a hit by the instance's flags and by the light's own entity, composes
 * model -> world -> view, appends to an instance range and reduces over the kept hits. Here ONE call does that for every view of a pass from
 * the context's resident world boxes (ivx_bv_set*, ivx_cw_synchronize) and the resident masks of its last queries call (ivx_bv_queries or
 * ivx_bv_queries_hierarchy), and leaves the ivx_cull_pair of every (view, object) where ivx_cull_many_resident reads it (csrc/instances.hip):
 * set -> queries -> instances -> cull on the context's stream, and only the reductions come back, because the light geometry needs them.
 * NOT here, it stays with the caller: the light geometry itself (cascade volumes, cubemap-face frusta, light-space orientation, texel snapping:
 * impact_light), material property buffering, scene-graph group transforms (the caller passes model-to-world), declare_visible_this_frame. */
/* One per object of the context's bounding-volume set, in the same index order. 48 bytes. */
#define IVX_FI_ABSENT 1u                  /* a bounding volume without a model instance node (get_node -> None): kept by no view */
#define IVX_FI_HIDDEN 2u                  /* ModelInstanceFlags::IS_HIDDEN */
#define IVX_FI_CASTS_NO_SHADOWS 4u        /* ::CASTS_NO_SHADOWS */
#define IVX_FI_SHADOWS_OFF_BY_DISTANCE 8u /* ::EXCEEDS_DIST_FOR_DISABLING_SHADOWING */
#define IVX_FI_NO_SHADOW_FEATURES 16u     /* feature_ids_for_shadow_mapping().is_empty() (light.rs:408-417 tests these four) */
#define IVX_FI_ALL_FLAGS 31u
#define IVX_FI_NONE 0xFFFFFFFFu /* ivx_fi_view.exclude_entity: excludes nothing; ivx_fi_view.and_view: no other view */
typedef struct {
    ivx_similarity model_to_world;
    uint32_t flags;  /* IVX_FI_* above; a view rejects by its reject_flags (IVX_FI_ABSENT is not implied: name it there) */
    uint32_t entity; /* what a light's exclude_entity is compared with */
    uint32_t reserved[2];
} ivx_fi_instance;
#define IVX_FI_VIEW_REACH 1u /* the reach filter and the two distance reductions from `point` and `squared_reach` (light.rs:419-436) */
#define IVX_FI_VIEW_BOX 2u   /* the view-space box reduction */
/* One view of a pass. 72 bytes. */
typedef struct {
    ivx_similarity world_to_view; /* the camera's view transform, camera-to-face o world-to-camera, or world-to-light: the caller computes it */
    uint32_t query;               /* the row of the context's last queries call (either form) */
    uint32_t reject_flags;        /* an instance with any of these flags is not kept */
    uint32_t exclude_entity;      /* an instance with this entity is not kept (self-shadowing, light.rs:395, 756); IVX_FI_NONE: nobody */
    uint32_t and_view;            /* IVX_FI_NONE, or a view of the context's PREVIOUS ivx_fi_views call: the object must have been kept by it too
                                     (a cubemap face takes only the light's shadowing_models, light.rs:258-261) */
    uint32_t instance_base;       /* the view's kept objects get instance indices instance_base, instance_base + 1, .. in ascending object index */
    uint32_t flags;               /* IVX_FI_VIEW_* */
    float point[3];               /* REACH: the light's position in world space */
    float squared_reach;          /* REACH: the light's squared max reach */
} ivx_fi_view;
/* The reductions over a view's kept set. 60 bytes. */
typedef struct {
    uint32_t count;
    ivx_aabb world_box;
    ivx_aabb view_box;
    float min_squared_distance, max_squared_distance;
} ivx_fi_view_result;
/* KEPT SET. With b the world box of object o, object o is kept by view v when ALL of:
 *   bit o of mask row v.query is set;  (flags[o] & v.reject_flags) == 0;  entity[o] != v.exclude_entity;
 *   v.and_view == IVX_FI_NONE, or bit o of kept row v.and_view of the context's previous ivx_fi_views call is set;
 *   no bound of b is a NaN;
 *   under IVX_FI_VIEW_REACH: NOT (d_close > v.squared_reach) — strict, so a box exactly at the reach is kept, and a NaN d_close is kept.
 * DISTANCES — all f32, this order, no contraction. With p = v.point, per axis k (closest_interior_point_to: max with lower, then min with upper):
 *     c[k] = b.lower[k] > p[k] ? b.lower[k] : p[k];   c[k] = b.upper[k] < c[k] ? b.upper[k] : c[k];   e[k] = p[k] - c[k]
 *   d_close = (e[0] e[0] + e[1] e[1]) + e[2] e[2].
 *   farthest_corner_from: m[k] = 0.5f (b.lower[k] + b.upper[k]);  f[k] = p[k] > m[k] ? b.lower[k] : b.upper[k]  (p at the centre takes the upper
 *   corner);  g[k] = p[k] - f[k];  d_far = (g[0] g[0] + g[1] g[1]) + g[2] g[2].
 * REDUCTIONS over the kept set: count; world_box = per component the minimum of the lowers and the maximum of the uppers of the world boxes;
 *   view_box (IVX_FI_VIEW_BOX) = the same merge over ivx_bv_world_aabb's arithmetic with the WORLD box as the model box and v.world_to_view as
 *   the similarity (aabb_of_transformed); min_squared_distance = the minimum of d_close, max_squared_distance = the maximum of d_far (REACH).
 *   Every minimum and maximum is order_min / order_max, the total order of the bit patterns with -0.0 below +0.0 that the block boxes of a set
 *   use: the result depends on no order of evaluation, +-0 and NaNs included (a positive NaN sorts above +inf, a negative one below -inf).
 *   The device reduces 64 objects by cross-lane steps, 256 objects in LDS, and the 256-object tiles of a view in one final pass; no float atomic.
 *   An empty kept set gives count 0, boxes with lower = +inf and upper = -inf, distances +inf / -inf; a reduction that was not asked for is
 *   stored with the same empty values.
 * COMPOSITION. For a kept pair, model_to_view = world_to_view * model_to_world by Similarity3 x Similarity3, a = world_to_view, b = model_to_world:
 *     scaling = a.s b.s;   u = (a.s b.t.x, a.s b.t.y, a.s b.t.z)
 *     translation = rotate(a.q, u) + a.t, with rotate(q, v) as the contact and collision kernels state it (glam's mul_vec3a): B = (q.x, q.y, q.z),
 *       b2 = (B.x B.x + B.y B.y) + B.z B.z, dv = (v.x B.x + v.y B.y) + v.z B.z, cross = (B.y v.z - v.y B.z, B.z v.x - v.z B.x, B.x v.y - v.x B.y),
 *       rotate = (v (q.w q.w - b2) + B (dv 2)) + cross (q.w 2), componentwise
 *     rotation = a.q b.q (glam's mul_quat, sums left to right):  x = ((a.w b.x + a.x b.w) + a.y b.z) - a.z b.y
 *       y = ((a.w b.y - a.x b.z) + a.y b.w) + a.z b.x    z = ((a.w b.z + a.x b.y) - a.y b.x) + a.z b.w    w = ((a.w b.w - a.x b.x) - a.y b.y) - a.z b.z
 *   A restatement in f32 with a fixed operation order, not a bit-parity target (glam's is unpinned). The product of two positive scalings may
 *   underflow to zero or overflow; the pair then carries that value, and ivx_cull_many_resident does not look at it.
 * OUTPUTS, all resident (ivx_fi_device_ptr) and each downloadable (ivx_fi_download); W = ceil(n / 64):
 *   pairs       ivx_cull_pair[n_views x n], view-major. A kept pair: the composed similarity, instance_idx = instance_base + its rank in the
 *               view's kept list, flags 0. Every other pair: the identity similarity (rotation 0 0 0 1, translation 0, scaling 1), instance_idx 0,
 *               IVX_CULL_PAIR_SKIP. Every byte is defined.
 *   lists       offsets[n_views + 1]; objects[total], ascending object index within a view; transforms[total], the composed ivx_similarity of
 *               each — the view's instance-transform range as the renderer's instance buffer wants it (InstanceModelViewTransform /
 *               InstanceModelLightTransform). The device buffers hold n_views x n entries, so that no call waits for the total.
 *   kept masks  uint64_t[n_views x W], bits past n zero. The context keeps them for the NEXT call's and_view; the set of the call before is
 *               dropped by a buffer swap. A new set of bounding volumes drops them too (the next call then has no previous views).
 *   results     ivx_fi_view_result[n_views].
 * ivx_fi_set_instances: one upload from pinned staging; the instances stay resident until the next call. IVX_ERR_INVALID: a scaling that is not
 *   positive (a NaN included), a flag bit outside IVX_FI_ALL_FLAGS; IVX_ERR_CAPACITY: n above IVX_BV_MAX_OBJECTS. A refused call leaves the
 *   instances as they were.
 * ivx_fi_views: a handful of launches on the context's stream, independent of n_views: decide (a wave per 64 objects walks the views), a
 *   workgroup per view (the final pass of the reductions; the prefix of the kept words' popcounts), the offsets, and the emit (a lane per pair,
 *   written out through LDS in whole lines). results == NULL: nothing waits and nothing comes back; else the n_views records, after one wait.
 *   IVX_ERR_INVALID: more than IVX_FI_MAX_VIEWS views (the cull limit), a world_to_view scaling that is not positive, a query not below the
 *   last queries call's count, an and_view that is neither IVX_FI_NONE nor below the previous call's view count, a reject_flags bit outside
 *   IVX_FI_ALL_FLAGS, a flags bit outside REACH | BOX. IVX_ERR_STATE: no set; no queries call since the set; no instances, or instances whose n
 *   is not the set's. n == 0 or n_views == 0 succeed with empty outputs (and count as the previous call of the next one). A refused call
 *   leaves the previous state — outputs and kept masks —; a call that fails later leaves none. Inside an ivx_many_begin bracket what has been
 *   recorded is flushed first.
 * ivx_fi_download: the outputs of the last call; each pointer may be NULL, each capacity is in elements (pairs: n_views x n; offsets: n_views + 1;
 *   objects and transforms share list_cap: the total; kept: n_views x W); too small: IVX_ERR_CAPACITY and nothing written. *n_listed (may be NULL)
 *   is the total. IVX_ERR_STATE before the first successful ivx_fi_views.
 * ivx_fi_device_ptr: the IVX_FI_PTR_* buffers. Context-owned and grow-only under the rules ivx_cull_device_ptr documents.
 * ivx_fi_views_host: the whole stage on the host with the same functions, for callers without a device and for the tests: n world boxes, n
 *   instances, masks[n_queries x W], previous_kept[n_previous_views x W] (may be NULL when that is 0). Same refusals as the two calls above for
 *   the records. Each output may be NULL; objects / transforms hold list_cap entries (IVX_ERR_CAPACITY when the total exceeds it, nothing written).
 *   The device leaves the same bytes. */
#define IVX_FI_MAX_VIEWS 64u
#define IVX_FI_PTR_INSTANCES 0
#define IVX_FI_PTR_PAIRS 1
#define IVX_FI_PTR_OFFSETS 2
#define IVX_FI_PTR_OBJECTS 3
#define IVX_FI_PTR_TRANSFORMS 4
#define IVX_FI_PTR_KEPT_MASKS 5
#define IVX_FI_PTR_RESULTS 6
int ivx_fi_set_instances(ivx_ctx*, const ivx_fi_instance* instances, size_t n);
int ivx_fi_views(ivx_ctx*, const ivx_fi_view* views, size_t n_views, ivx_fi_view_result* results);
int ivx_fi_download(ivx_ctx*, ivx_cull_pair* pairs, size_t pair_cap, uint32_t* offsets, size_t offset_cap, uint32_t* objects, ivx_similarity* transforms, size_t list_cap,
                    uint64_t* kept_masks, size_t kept_cap, size_t* n_listed);
void* ivx_fi_device_ptr(ivx_ctx*, int which);
int ivx_fi_views_host(const ivx_aabb* world_boxes, size_t n, const ivx_fi_instance* instances, const uint64_t* masks, size_t n_queries, const ivx_fi_view* views,
                      size_t n_views, const uint64_t* previous_kept, size_t n_previous_views, ivx_cull_pair* pairs, uint32_t* offsets, uint32_t* objects,
                      ivx_similarity* transforms, size_t list_cap, uint64_t* kept_masks, ivx_fi_view_result* results);
/* ivx_cull_many_enqueue with the pair of (view v, grid g) taken ON THE DEVICE from the frame-instance pairs of the grids' context at
 * (v, object_indices[g]) (object_indices == NULL: g itself): a small gather writes pairs and pair flags where the upload would have put them;
 * the rest of the call, its bytes and ivx_cull_collect / ivx_cull_download are those of ivx_cull_many_enqueue. IVX_ERR_STATE when the context's
 * last ivx_fi_views call had another n_views (or there was none); IVX_ERR_INVALID for an index not below that call's n. n == 0 touches no context. */
int ivx_cull_many_resident(ivx_grid* const* grids, size_t n, const ivx_cull_object* objects, const uint32_t* object_indices, const ivx_cull_view* views, size_t n_views,
                           uint32_t mode, ivx_cull_region* out_layout);

/* ---- primitive collidables: follow the bodies, narrow phase over the pairs (impact_physics/src/collision.rs:175-261, 317-373
 * synchronize_collidables_with_rigid_bodies and the collision pass; collision/collidable/basic.rs:57-151, sphere.rs:105-157, capsule.rs:142-303;
 * impact_geometry/src/line.rs:26-145; material.rs:43-51) ----
 * A frame of primitive bodies: ivx_cw_synchronize -> ivx_cw_collide -> ivx_world_set_contacts -> ivx_world_step. Only the contact list crosses
 * to the host (the constraint cache lives there); world boxes are never computed on the host. csrc/narrow.hip. */
#define IVX_CW_SPHERE 0u
#define IVX_CW_PLANE 1u
#define IVX_CW_CAPSULE 2u
#define IVX_CW_VOXEL_OBJECT 3u /* broad phase only: its pairs are deferred to ivx_voxel_object_contacts_many / ivx_mutual_voxel_object_contacts_many */
/* One collidable, in its body's frame (ivx_cw_set_collidables) or in world space (ivx_cw_download). 64 bytes. */
typedef struct {
    uint32_t shape;    /* IVX_CW_* */
    uint32_t kind;     /* IVX_BV_DYNAMIC / _STATIC / _PHANTOM */
    uint32_t body;     /* index of the dynamic body it follows; IVX_KINEMATIC_BODY bit set: of the kinematic body */
    uint32_t reserved;
    uint64_t id;       /* CollidableID */
    float a[3];        /* sphere centre | plane unit normal | capsule segment start | voxel object: model box lower (world space: world box lower) */
    float b[3];        /* capsule segment vector | voxel object: model box upper (world space: world box upper); unused otherwise */
    float s;           /* sphere radius | plane displacement | capsule radius; unused for a voxel object */
    float response[3]; /* restitution, static friction, dynamic friction of THIS collidable (ContactResponseParameters) */
} ivx_collidable;
#define IVX_CW_PTR_WORLD_COLLIDABLES 0
#define IVX_CW_PTR_CONTACTS 1
#define IVX_CW_PTR_DEFERRED_PAIRS 2
/* Host arithmetic; the kernels run the same functions and give the same bytes. All f32, the order below, no contraction.
 *   dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z;  u + v, u - v, u k component-wise;  cross(u, v) = (u.y v.z - v.y u.z, u.z v.x - v.z u.x, u.x v.y - v.x u.y)
 *   qrot(q, v), q = (x, y, z, w), b = (x, y, z): ((v (w w - dot(b, b))) + (b (dot(v, b) 2))) + (cross(b, v) (w 2))      (glam Quat::mul_vec3a)
 *   max0(x) = x > 0 ? x : 0 (f32::max(0.0, x): a NaN gives 0);  clamp01(x) = x < 0 ? 0 : (x > 1 ? 1 : x) (f32::clamp: a NaN and -0.0 pass through)
 *   EPS = 1e-8f
 * ivx_cw_transform — Collidable::from_descriptor under the body's isometry (position p, orientation q), and the world box:
 *   sphere:  a' = qrot(q, a) + p;  box = (a' - s, a' + s) per component
 *   capsule: a' = qrot(q, a) + p, b' = qrot(q, b);  e = a' + b';  box.lower = min(a' - s, e - s), box.upper = max(a' + s, e + s) with
 *            min(u, v) = v < u ? v : u, max(u, v) = v > u ? v : u (capsule.rs:132-137)
 *   plane (plane.rs:197-203):  a' = qrot(q, a);  s' = dot(a', qrot(q, a s) + p);  box = (-FLT_MAX, +FLT_MAX) on every axis — the reference gives a
 *            plane no bounding volume; here it pairs with every box that has no NaN bound. PLANES BELONG AT THE END OF THE LIST: a block of 64
 *            consecutive objects that holds one has an unbounded block box and is never rejected as a whole by the pair pass.
 *   voxel object: (lo, hi) = ivx_bv_world_aabb of the model box (a, b) under (q, p, scaling 1), then widened per axis k by
 *            pad_k = (((m_0 + m_1) + m_2) + |p_k|) 2^-19, m_j = |b_j| > |a_j| ? |b_j| : |a_j|:  a' = lo - pad, b' = hi + pad — also its box. The float32
 *            derivation alone can leave a corner of the rotated model box a few units in the last place OUTSIDE; the pad is several times the
 *            largest such loss, so the box holds the exact image of the model box. (a, b) is the model box in the BODY's frame: for a voxel
 *            object, ivx_grid_model_aabb minus the origin offset (the body frame's origin in model space, its centre of mass).
 *   Everything else of the record is copied. `box` may be NULL.
 * ivx_cw_contact — generate_contact_manifold (basic.rs:57-151) for one pair of WORLD-SPACE collidables A, B. *hit = 0: no contact (plane against
 *   plane always); 1: `out` holds it; 2: a member is a voxel object, nothing is tested. Where the reference answers CollidableOrder::Swapped —
 *   (sphere, capsule), (plane, sphere), (plane, capsule) — the two members swap first; "first / second" below are the members after the swap.
 *     id = splitmix(id_first ^ splitmix(id_second)) (random/splitmix.rs:4-15), body_a / body_b = the members' bodies, flags = IVX_CONTACT_MANIFOLD_START
 *     restitution = r2 > r1 ? r2 : r1;  static / dynamic friction = sqrt(f1 f2)                               (ContactResponseParameters::combined)
 *   sphere (c1, r1), sphere (c2, r2):  d = c1 - c2, d2 = dot(d, d), m = r1 + r2;  miss when d2 > m m;  dist = sqrt(d2);
 *     normal = dist > EPS ? d (1 / dist) : (0, 0, 1);  position = c2 + normal r2;  depth = max0(m - dist)
 *   sphere (c, r), plane (n, k):  sd = dot(n, c) - k, depth = r - sd;  miss when depth < 0;  position = c - n sd, normal = n
 *   capsule (a, v, rc), sphere (c, r):  l2 = dot(v, v);  t = l2 <= EPS ? 0 : clamp01(dot(v, c - a) / l2);  d = c - (a + v t), d2 = dot(d, d), m = r + rc;
 *     miss when d2 > m m;  dist = sqrt(d2);  dist > EPS: cn = d (1 / dist), depth = max0(m - dist);  else cn = ortho(v), depth = max0(m);
 *     normal = -cn, position = c + normal r
 *     ortho(v) (glam any_orthogonal_vector, normalized_from_if_above; parity with glam unpinned): o = |v.x| > |v.y| ? (-v.z, 0, v.x) : (0, v.z, -v.y),
 *       o2 = dot(o, o);  o2 > EPS EPS ? (o.x / sqrt(o2), o.y / sqrt(o2), o.z / sqrt(o2)) : (0, 0, 1)
 *   capsule (a1, v1, r1), capsule (a2, v2, r2) — parameters_of_closest_points_on_line_segments (line.rs:75-145):
 *     l1 = dot(v1, v1), l2 = dot(v2, v2);  both <= EPS: s = t = 0.  Else r = a1 - a2, f = dot(v2, r), and
 *       l1 <= EPS: s = 0, t = clamp01(f / l2);  else c = dot(v1, r) and
 *       l2 <= EPS: t = 0, s = clamp01(c / (-l1));  else g = dot(v1, v2), den = l1 l2 - g g,
 *         s = den != 0 ? clamp01((g f - c l2) / den) : 0;  t = (g s + f) / l2;
 *         t has its sign bit set (-0.0 included): t = 0, s = clamp01(c / (-l1));  else t > 1: t = 1, s = clamp01((g - c) / l1)
 *     p1 = a1 + v1 s, p2 = a2 + v2 t, d = p1 - p2, d2 = dot(d, d), m = r1 + r2;  miss when d2 > m m;  dist = sqrt(d2);
 *     dist > EPS: normal = d (1 / dist), depth = max0(m - dist);
 *     else (the segments intersect): normal = ortho(v2), w = dot(v1, normal), shift = w has no sign bit ? (1 - s) w : (-s) w, depth = max0(m + shift);
 *     position = p2 + normal r2
 *   capsule (a, v, r), plane (n, k):  e = a + v;  d0 = dot(n, a) - k, d1 = dot(n, e) - k;  (p, low) = d0 <= d1 ? (a, d0) : (e, d1);  depth = r - low;
 *     miss when depth < 0;  position = p - n low, normal = n */
int ivx_cw_transform(const ivx_collidable* local, const float position[3], const float orientation_xyzw[4], ivx_collidable* world, ivx_aabb* box);
int ivx_cw_contact(const ivx_collidable* a_world, const ivx_collidable* b_world, ivx_contact* out, int* hit);
/* The collidables of a world: n local records, resident until replaced (n == 0: an empty set). IVX_ERR_INVALID: a shape above 3, a kind above 2, a
 * body index past the world's body counts; IVX_ERR_CAPACITY: n above IVX_BV_MAX_OBJECTS. A refused call leaves the world's collidables as they were.
 * Index i of the set is object i of the bounding-volume set and of the pairs. */
int ivx_cw_set_collidables(ivx_world*, const ivx_collidable*, size_t n);
/* synchronize_collidables_with_rigid_bodies: one launch on the context's stream, a lane per collidable — ivx_cw_transform under the position and
 * orientation its body has in the world's resident arrays (behind ivx_world_step_enqueue it sees that step's bodies; nothing waits) — then the
 * launches of ivx_bv_set: the world boxes and kinds become the context's bounding-volume set without a host round trip, and ivx_bv_pairs,
 * ivx_bv_queries and ivx_bv_download work on it. IVX_ERR_STATE: no collidables set, or the world's bodies have been replaced by fewer since. */
int ivx_cw_synchronize(ivx_world*);
/* The world-space collidables of the last ivx_cw_synchronize (cap >= n, else IVX_ERR_CAPACITY). Waits for the stream. */
int ivx_cw_download(ivx_world*, ivx_collidable* world_space, size_t cap);
/* The pair pass of ivx_bv_pairs (same code, same modes) over the context's set, then ivx_cw_contact over the resident pair buffer, a lane per pair.
 * out: the contacts; deferred_pairs: uint32_t[2] = (a, b) of every pair with a voxel-object member, for the `_many` voxel generators. BOTH COMPACTED IN
 * PAIR ORDER, lexicographic in (a, b): wave ballots, a scan of the per-wave counts, no atomic — two calls leave the same bytes. The call waits twice:
 * for the pair pass's grand total and, at the end, for the two counts together with the results. *n_out / *n_deferred are the numbers found even
 * when one exceeds its capacity; the call then returns IVX_ERR_CAPACITY and writes neither list. out == NULL with cap == 0 (and likewise the
 * deferred list) leaves that list on the device only (ivx_cw_device_ptr). Inside an ivx_many_begin bracket what has been recorded is flushed first,
 * as by ivx_bv_pairs. IVX_ERR_STATE before ivx_cw_synchronize, or when the context's set has been replaced since. */
int ivx_cw_collide(ivx_world*, uint32_t mode, ivx_contact* out, size_t cap, size_t* n_out, uint32_t* deferred_pairs, size_t deferred_cap, size_t* n_deferred);
/* IVX_CW_PTR_*: the world collidables, the contacts and the deferred pairs of the last calls; world-owned and grow-only, NULL before they exist */
void* ivx_cw_device_ptr(ivx_world*, int which);

/* ---- collision frame: the deferred pairs' contacts in the same call (impact_voxel/src/collidable.rs:138-215 generate_contact_manifold,
 * 310-327 VoxelObjectCollidable::new; impact_math/src/transform/isometry.rs:112-134) ----
 * A frame with voxel objects among the collidables: ivx_cw_synchronize -> ivx_cw_collide_frame -> ivx_world_set_contacts -> ivx_world_step. The
 * voxel objects' world -> object transforms are derived on the device from the world's resident bodies; only the merged contact list and its
 * bookkeeping cross to the host. csrc/narrow.hip (k_cw_rows), csrc/cw_rows.hpp (the arithmetic), csrc/voxel_collision_api.hip (the host side). */
/* The voxel object behind a collidable of shape IVX_CW_VOXEL_OBJECT. 32 bytes: grid 0, origin_offset 8, center_of_mass 20. */
typedef struct ivx_cw_voxel_object {
    ivx_grid* grid;
    float origin_offset[3];  /* the body frame's origin in model space (the local centre of mass the body was seated on) */
    float center_of_mass[3]; /* the mutual generator's argument, model space */
} ivx_cw_voxel_object;
/* The dispatch of one deferred pair: which generator, and its arguments. 160 bytes, a multiple of 8. Offsets: generator 0, voxel 4, other 8,
 * reserved 12, collidable_id_a 16, collidable_id_b 24, body_a 32, body_b 36, response 40, shape1 52, shape3 56, shape3b 68, rotation_a 80,
 * translation_a 96, center_of_mass_a 108, rotation_b 120, translation_b 136, center_of_mass_b 148. It becomes an ivx_collidable_query
 * (generators 0 to 2: mode = generator, rotation_xyzw = rotation_a, translation = translation_a, the other fields by their names) or an
 * ivx_mutual_query (generator 3: every field by its name; the handles a / b are those of collidables `voxel` / `other`) by plain field copies.
 * What a generator does not take is zero. */
#define IVX_CW_ROW_MUTUAL 3u
struct ivx_cw_voxel_row { /* (no typedef: the function below has the name) */
    uint32_t generator;  /* 0 sphere, 1 plane, 2 capsule (ivx_collidable_query.mode), IVX_CW_ROW_MUTUAL */
    uint32_t voxel;      /* collidable index of the voxel object the generator runs on; mutual: of object A */
    uint32_t other;      /* collidable index of the other member; mutual: of object B */
    uint32_t reserved;
    uint64_t collidable_id_a, collidable_id_b;
    uint32_t body_a, body_b;
    float response[3];
    float shape1;
    float shape3[3], shape3b[3];
    float rotation_a[4], translation_a[3], center_of_mass_a[3]; /* transform_to_object_space of `voxel` */
    float rotation_b[4], translation_b[3], center_of_mass_b[3]; /* mutual only: of `other` */
};
#define IVX_CW_PTR_FRAME_CONTACTS 3 /* the merged list of the last ivx_cw_collide_frame (the buffer of IVX_CW_PTR_CONTACTS: the primitive part comes first) */
#define IVX_CW_PTR_VOXEL_ROWS 4     /* struct ivx_cw_voxel_row of every deferred pair of the last ivx_cw_collide_frame */
/* Host arithmetic; k_cw_rows runs the same two functions and gives the same bytes. All f32, the forms of ivx_cw_transform above, no contraction.
 * ivx_cw_to_object_space — VoxelObjectCollidable::new's transform_to_object_space for a body at position p with orientation q = (x, y, z, w) whose
 *   frame has its origin at o (model space): the inverse of transform_to_world_space.applied_to_translation(-o) in the reference's order,
 *     t_w = qrot(q, -o) + p;  rotation = conj(q) = (-x, -y, -z, w);  translation = -qrot(rotation, t_w)
 * ivx_cw_voxel_row — generate_contact_manifold (collidable.rs:138-215) for one deferred pair of WORLD-SPACE collidables (a, b), at least one a voxel
 *   object. pose_* = position[3] then orientation_xyzw[4] of the member's body, voxel_* = its ivx_cw_voxel_object (the grid is not read); both are
 *   read for voxel members only and may be NULL otherwise. combined(r1, r2) = (r2[0] > r1[0] ? r2[0] : r1[0], sqrt(r1[1] r2[1]), sqrt(r1[2] r2[2])).
 *     voxel, voxel:  generator 3; A = a, B = b: ids (a, b), bodies (a, b), response = combined(a, b); rotation / translation_a and _b =
 *       ivx_cw_to_object_space of each member, center_of_mass_a / _b theirs
 *     voxel v, plane c (either order):  generator 1; the voxel object is A: bodies (v, c), response = combined(v, c); the ids take the plane first:
 *       ids (c, v); shape3 = the plane's normal, shape1 = its displacement
 *     voxel v, sphere or capsule c (either order):  generator 0 / 2; c is A: bodies (c, v), ids (c, v), response = combined(c, v); shape3 = centre /
 *       segment start, shape1 = radius, capsule: shape3b = segment vector
 *     generators 0 to 2: rotation_a / translation_a = ivx_cw_to_object_space of v
 *   out->voxel / out->other are written as 0 for member a and 1 for member b (the kernel writes the pair's collidable indices). IVX_ERR_INVALID:
 *   no voxel member, a shape above 3, a voxel member without its pose or record. */
int ivx_cw_to_object_space(const float position[3], const float orientation_xyzw[4], const float origin_offset[3], float rotation_out[4], float translation_out[3]);
int ivx_cw_voxel_row(const ivx_collidable* a_world, const ivx_collidable* b_world, const float pose_a[7], const float pose_b[7], const ivx_cw_voxel_object* voxel_a,
                     const ivx_cw_voxel_object* voxel_b, struct ivx_cw_voxel_row* out);
/* Attaches objects[k] to collidable collidable_index[k] of the world's set; the n attachments REPLACE the ones before (n == 0: none). Resident
 * until replaced; ivx_cw_set_collidables drops them. The offsets and centres of mass are uploaded to a device array indexed by collidable; the
 * grids' occupied ranges, probes and buffers are read at every ivx_cw_collide_frame, so an edit needs no new call unless the origin offset or the
 * centre of mass moved. IVX_ERR_INVALID: an index past the set, an index whose shape is not a voxel object, a null grid, a grid of another
 * context than the world's, the same index twice; IVX_ERR_STATE: no collidables set. A refused call leaves the attachments as they were. */
int ivx_cw_set_voxel_objects(ivx_world*, const uint32_t* collidable_index, const ivx_cw_voxel_object* objects, size_t n);
/* The whole collision pass of a frame. The pair pass and the primitive narrow phase of ivx_cw_collide (same code, same modes, the broad phase
 * ivx_cw_set_broad_phase selected); right behind them k_cw_rows, a lane per deferred pair: ivx_cw_voxel_row over the world-space records, the
 * pose of each voxel member's body as the world's resident arrays hold it (behind ivx_world_step_enqueue: that step's bodies, with no wait) and
 * the attached offsets and centres of mass. The rows come to the host with the counts; the voxel generators of ivx_voxel_object_contacts_many
 * and ivx_mutual_voxel_object_contacts_many then run over them in merged launches (csrc/many.hpp), their emit passes writing behind the
 * primitive contacts. out: the primitive contacts (*n_primitive of them, what ivx_cw_collide returns), then one manifold per deferred pair IN
 * DEFERRED-LIST ORDER: manifold i is out[*n_primitive + manifold_offsets[i] .. *n_primitive + manifold_offsets[i + 1]) (n_deferred + 1 offsets),
 * the very list the single-pair generator returns for row i, first contact flagged IVX_CONTACT_MANIFOLD_START — ready for ivx_world_set_contacts.
 * deferred_pairs (2 x uint32_t each) and manifold_offsets share deferred_cap: room for deferred_cap pairs and deferred_cap + 1 offsets.
 * *n_out (all contacts), *n_primitive and *n_deferred are the numbers found even when a capacity is exceeded; the call then returns
 * IVX_ERR_CAPACITY and writes no list. out == NULL with cap == 0 leaves the merged list on the device only (IVX_CW_PTR_FRAME_CONTACTS), and
 * likewise the deferred list and the offsets. The call waits four times: the pair total; counts, deferred pairs and rows; the generators'
 * totals; the list (a growth of a buffer, or a deferred list more than twice the last call's, waits once more).
 * IVX_ERR_STATE: before ivx_cw_synchronize; the context's set replaced since; a deferred pair names a voxel collidable with no object attached;
 * inside an ivx_many_begin bracket (the call waits for its own phases). The generators' own preconditions report as they do in the `_many`
 * calls: current derived state, and current probes for both members of a voxel-voxel pair. */
int ivx_cw_collide_frame(ivx_world*, uint32_t mode, ivx_contact* out, size_t cap, size_t* n_out, size_t* n_primitive, uint32_t* deferred_pairs,
                         uint32_t* manifold_offsets, size_t deferred_cap, size_t* n_deferred);
/* The rows of the last ivx_cw_collide_frame, in deferred-list order (cap >= its *n_deferred, else IVX_ERR_CAPACITY). Waits for the stream. */
int ivx_cw_rows_download(ivx_world*, struct ivx_cw_voxel_row* rows, size_t cap, size_t* n_rows);

/* ---- motion drivers of kinematic bodies (impact_physics/src/driven_motion.rs and the files under driven_motion/; csrc/motion.hip) -----------
 * A kinematic body whose state is a function of the simulation time. One record per driver, 64 bytes: `body` indexes the world's kinematic
 * bodies (WITHOUT the IVX_KINEMATIC_BODY bit), `p` holds the reference's setup struct of that kind, field by field in its #[repr(C)] order:
 *   IVX_MD_CIRCULAR              CircularTrajectory            p[0] initial_time, p[1..4] orientation xyzw, p[5..7] center_position, p[8] radius, p[9] period
 *   IVX_MD_CONSTANT_ACCELERATION ConstantAccelerationTrajectory p[0] initial_time, p[1..3] initial_position, p[4..6] initial_velocity, p[7..9] acceleration
 *   IVX_MD_HARMONIC              HarmonicOscillatorTrajectory  p[0] center_time, p[1..3] center_position, p[4..6] direction, p[7] amplitude, p[8] period
 *   IVX_MD_ORBITAL               OrbitalTrajectory             p[0] periapsis_time, p[1..4] orientation xyzw, p[5..7] focal_position, p[8] semi_major_axis,
 *                                                              p[9] eccentricity, p[10] period
 *   IVX_MD_CONSTANT_ROTATION     ConstantRotation              p[0] initial_time, p[1..4] initial_orientation xyzw, p[5..7] unit axis, p[8] angular speed
 * The rest of `p` is ignored.
 *
 * Arithmetic: float32, uncontracted, in the reference's operation order (TWO_PI = 6.2831855f, PI = 3.1415927f; `%` is fmodf: the result has the
 * dividend's sign; sin, cos and tan are the double-precision functions rounded once; rotate_point / rotate_vector are glam's mul_vec3a):
 *   circular (circular.rs:134-194)    w = TWO_PI / period;  angle = (w * (t - initial_time)) % TWO_PI;  s, c = sin, cos(angle)
 *       position = center + rotate(q, (radius * c, radius * s, 0));  v = radius * w;  velocity = rotate(q, (-v * s, v * c, 0))
 *   constant acceleration (constant_acceleration.rs:143-157)    dt = t - initial_time
 *       position = (p0 + dt * v0) + (0.5 * (dt * dt)) * a;  velocity = v0 + dt * a
 *   harmonic (harmonic_oscillation.rs:139-159)    dt = t - center_time;  w = TWO_PI / period
 *       position = center + (amplitude * sin(w * dt)) * direction;  velocity = ((amplitude * w) * cos(w * dt)) * direction
 *   orbital (orbit.rs:149-365)    n = TWO_PI / period;  M = (n * (t - periapsis_time)) % TWO_PI
 *       E: Newton from E = M, E' = E - ((E - e * sin E) - M) / (1 - e * cos E), until |E' - E| <= 1e-4 or 100 iterations
 *       f2 = (1 + e) / (1 - e);  f = sqrt(f2);  th = tan(0.5 * E);  th2 = th * th;  tv2 = f2 * th2;  k = 1 / (1 + tv2)
 *       cos_v = (1 - tv2) * k;  dv_dE = (f * (1 + th2)) * k;  r = (a * (1 - e * e)) / (1 + e * cos_v)
 *       sin_v = sqrt(1 - cos_v * cos_v), negated unless E <= PI  (a time before periapsis_time has M < 0 and so E < PI: it takes the
 *       positive root, as in the reference)
 *       position = focus + rotate(q, (r * cos_v, r * sin_v, 0));  dv = (n * dv_dE) / (1 - e * cos E)
 *       vr = ((((dv * e) * a) * (1 - e * e)) * sin_v) / ((1 + e * cos_v) * (1 + e * cos_v));  vt = r * dv
 *       velocity = rotate(q, (vr * cos_v - vt * sin_v, vr * sin_v + vt * cos_v, 0))
 *   constant rotation (constant_rotation.rs:111-120)    orientation = advance_orientation(q0, axis, speed, t - initial_time), the very code of the
 *       step's advance of configurations (rigid_body.rs:1013-1034);  angular velocity = (axis, speed) as given
 *
 * Composition (MotionDriverManager::apply_motion, driven_motion.rs:50-82), the same code on the device and in ivx_md_apply_host:
 *   - a body with at least one trajectory driver (the first four kinds) has position and velocity reset to +0.0, then the contributions are
 *     added in the order circular, constant acceleration, harmonic, orbital and, within a kind, in the order of the caller's list. (The
 *     reference walks the drivers of a kind in the order of a hash map, which nothing pins; the list order is this library's choice.) The sum
 *     starts from the reset zero, so a lone -0.0 component comes out +0.0, as in the reference.
 *   - constant rotations come last; each sets orientation and angular velocity, the last one in list order wins.
 *   - a body with rotation drivers only keeps the position and velocity it has; one with trajectory drivers only keeps its orientation and
 *     angular velocity. Bodies without a driver are not written. */
#define IVX_MD_CIRCULAR 0u
#define IVX_MD_CONSTANT_ACCELERATION 1u
#define IVX_MD_HARMONIC 2u
#define IVX_MD_ORBITAL 3u
#define IVX_MD_CONSTANT_ROTATION 4u
typedef struct {
    uint32_t kind; /* IVX_MD_* */
    uint32_t body; /* index into the kinematic bodies */
    float p[14];
} ivx_motion_driver;
/* The world's driver set, resident until replaced (n == 0 removes it); call it after ivx_world_set_bodies. The set is stored sorted stably by
 * (body, kind, list index) with a compact list of the driven bodies, and uploaded once. IVX_ERR_INVALID, with a message that names the driver
 * (the set then stays as it was), for what the reference asserts when it applies a driver: a radius or semi-major axis that is not > 0, a period
 * with |period| <= FLT_EPSILON (circular, harmonic, orbital), an eccentricity outside [0, 1); and for an unknown kind or body >= the world's
 * kinematic bodies. With a set installed every ivx_world_step / ivx_world_step_enqueue ends by applying it at the new time (below): one launch
 * behind the advance of configurations on the same stream, a lane per driven body; nothing waits. A world without a set launches what it
 * launched before. If the world's bodies are replaced by fewer kinematic bodies than the set refers to, the next apply is IVX_ERR_STATE. */
int ivx_world_set_motion_drivers(ivx_world*, const ivx_motion_driver*, size_t n);
/* The world's simulation clock: 0 at creation; every ivx_world_step and ivx_world_step_enqueue sets time = time + dt in float32
 * (perform_physics_step's new_simulation_time, src/lib.rs:86-100). Host-side only. */
int ivx_world_set_time(ivx_world*, float time);
int ivx_world_time(ivx_world*, float* out);
/* MotionDriverManager::apply_motion at `time` on its own, like the other stages: enqueued, does not touch the clock. No set installed: nothing. */
int ivx_world_apply_motion(ivx_world*, float time);
/* One driver at `time`, the function the kernel runs, on the host (tests). Trajectory kinds: out[0..2] position, out[3..5] velocity, the rest 0;
 * constant rotation: out[0..3] orientation xyzw, out[4..6] axis, out[7] angular speed, the rest 0. Validates like ivx_world_set_motion_drivers
 * (the body index is not looked at). */
int ivx_md_eval(const ivx_motion_driver*, float time, float out[10]);
/* The composition above over host arrays, the code the kernel runs (tests). Validates like ivx_world_set_motion_drivers against n_kinematic. */
int ivx_md_apply_host(const ivx_motion_driver*, size_t n, ivx_kinematic_body* bodies, size_t n_kinematic, float time);

/* ---- force generators and dynamic gravity (impact_physics/src/force.rs and the files under force/; csrc/forces.hip) ---------------------------
 * ForceGeneratorManager::apply_forces_and_torques (force.rs:130-159) as the last stage of the step. One record per generator, 64 bytes: `body`
 * indexes the world's dynamic bodies; `body_b` is the second body of a spring — a dynamic index, or for the dynamic-kinematic spring a
 * kinematic index WITHOUT the IVX_KINEMATIC_BODY bit — and is ignored by the other kinds. An anchor is given resolved, as body index plus
 * body-space point; AnchorManager stays the host's business. `p`:
 *   IVX_FG_CONSTANT_ACCELERATION    constant_acceleration.rs:96-102   p[0..2] acceleration (world)
 *   IVX_FG_LOCAL_FORCE              local_force.rs:37-62              p[0..2] force (body frame), p[3..5] point (body frame)
 *   IVX_FG_SPRING_DYNAMIC_DYNAMIC   spring_force.rs:140-189, 317-331  p[0..2] attachment point 1, p[3..5] attachment point 2 (each in its body's frame),
 *                                                                     p[6] stiffness, p[7] damping, p[8] rest_length, p[9] slack_length
 *   IVX_FG_SPRING_DYNAMIC_KINEMATIC spring_force.rs:191-243           as above; body_b kinematic
 *   IVX_FG_ALIGNMENT_FIXED          alignment_torque.rs:107-241       p[0..2] axis_to_align (body frame, unit), p[3..5] alignment_direction (world, unit),
 *                                                                     p[6] settling_time, p[7] spin_damping, p[8] precession_damping
 *   IVX_FG_ALIGNMENT_GRAVITY        the same, AlignmentDirection::GravityForce   p[0..2] axis_to_align, p[6..8] as above
 * The rest of `p` is ignored.
 *
 * Arithmetic: float32, uncontracted, in the reference's operation order (EPSILON = f32::EPSILON; dot(a, b) = (ax bx + ay by) + az bz;
 * rotate(q, v) is glam's mul_vec3a; M v = (c0 vx + c1 vy) + c2 vz over the columns; rotated(M, q) = (R M) R^T with R = Mat3A::from_quat(q);
 * v / s on a Vec3A divides each component, on impact_math's vectors it multiplies by 1 / s — noted as `*recip` below):
 *   angular velocity of a dynamic body:  w0 = rotated(inv_inertia, q) L;  |w0|^2 > EPSILON^2 ? (w0 / |w0|) * |w0| : 0
 *   apply_force(f, at):  total_force += f;  total_torque += (at - position) x f
 *   constant acceleration    total_force += acceleration * mass
 *   local force              apply_force(rotate(q, force), position + rotate(q, point))
 *   spring (both kinds)      a1 = position_1 + rotate(q_1, point_1);  a2 likewise;  d = a2 - a1;  no force unless dot(d, d) > EPSILON^2
 *       length = sqrt(dot(d, d));  dir = d / length
 *       rate = 0 when |damping| <= EPSILON, else dot(v2, dir) - dot(v1, dir) with v = velocity + w x (a - position): for a dynamic body
 *       velocity = momentum *recip mass and w as above, for a kinematic body its velocity and axis * speed
 *       scalar = length <= slack_length ? 0 : (-stiffness) * (length - rest_length) + (-damping) * rate;  force_on_2 = scalar * dir
 *       body 1: apply_force(-force_on_2, a1);  body 2, if dynamic: apply_force(force_on_2, a2)
 *   gravity pair (i the lower rank; dynamic_gravity.rs:188-231, EPS = 1e-6; I = rotated(inertia, q))    r = p_j - p_i;  r2 = dot(r, r);  r1 = sqrt(r2)
 *       r3 = r2 * r1;  r5 = r3 * r2;  mono = (((G * m_i) * m_j) / (r3 + EPS)) * r;  qs = (1.5 * G) / (r5 + EPS)
 *       a = m_j * (I_i r);  b = m_i * (I_j r);  s = a + b;  trace = (xx + yy) + zz
 *       quad = qs * (((m_j * trace_i + m_i * trace_j) - (5 * dot(r, s)) / (r2 + EPS)) * r + 2 * s);  force_i = mono + quad
 *       torque_i = (2 * qs) * (r x a);  torque_j = (2 * qs) * (r x b)
 *       load_i.force += force_i, load_i.torque += torque_i;  load_j.force -= force_i, load_j.torque += torque_j
 *   alignment torque    direction = alignment_direction, or for the gravity kind load.force *recip |load.force| — nothing when the body is not in
 *       the field or when dot(load.force, load.force) <= 1e-9^2
 *       axis = rotate(q, axis_to_align);  c = direction x axis;  rot = dot(c, c) > 1e-8^2 ? c / sqrt(dot(c, c)) : orthogonal(axis), glam's
 *       any_orthonormal_vector: sign = copysign(1, z); a = -1 / (sign + z); (x * y * a, sign + y * y * a, -y)
 *       s_rot = dot(w, rot);  w_rot = s_rot * rot;  s_ax = dot(w, axis);  w_ax = s_ax * axis;  w_prec = (w - w_rot) - w_ax
 *       angle = acos(clamp(dot(direction, axis), -1, 1)), the double-precision function rounded once
 *       tc = 0.25 * settling_time;  nf = 1 / tc;  acc = (-(nf * nf)) * angle - (2 * nf) * s_rot
 *       alpha = (acc * rot - (spin_damping / settling_time) * w_ax) - (precession_damping / settling_time) * w_prec
 *       total_torque += rotated(inertia, q) alpha + w x L
 *
 * Composition, the same code on the device and in ivx_fg_apply_host:
 *   - total_force and total_torque of ALL dynamic bodies are reset to +0.0;
 *   - the contributions are added in the reference's phase order: constant accelerations, local forces, dynamic-dynamic springs, dynamic-kinematic
 *     springs, detailed drag (a set of its own, ivx_world_set_detailed_drag below), dynamic gravity, alignment torques (both kinds are one
 *     phase, as they are one registry);
 *   - inside a phase the order is that of the caller's list. (The reference walks a hash map there, which nothing pins; the list order is this
 *     library's choice, as for the motion drivers.)
 *   - dynamic gravity: the field is the caller's list of dynamic bodies (KeyIndexMapper order). Per body the reference's double loop adds the pairs
 *     in ascending partner rank; that order is kept. A field of fewer than two bodies gives zero loads.
 * Every body's sums are made by one lane in that order; there are no float atomics, so two runs leave the same bytes. */
#define IVX_FG_CONSTANT_ACCELERATION 0u
#define IVX_FG_LOCAL_FORCE 1u
#define IVX_FG_SPRING_DYNAMIC_DYNAMIC 2u
#define IVX_FG_SPRING_DYNAMIC_KINEMATIC 3u
#define IVX_FG_ALIGNMENT_FIXED 4u
#define IVX_FG_ALIGNMENT_GRAVITY 5u
typedef struct {
    uint32_t kind;   /* IVX_FG_* */
    uint32_t body;   /* index into the dynamic bodies */
    uint32_t body_b; /* springs: the second body (see above) */
    float p[13];
} ivx_force_generator;
/* The world's generator set, resident until replaced (n == 0 removes it); call it after ivx_world_set_bodies. IVX_ERR_INVALID, with a message that
 * names the generator (the set in force then stays): an unknown kind, a body index past the world's bodies, a dynamic-dynamic spring with
 * body == body_b (the reference's assert_ne!), a settling_time that is not > 0. With a set or a field installed every ivx_world_step /
 * ivx_world_step_enqueue ends with the force stage, behind the motion drivers on the same stream; nothing waits. Host-set totals are therefore
 * overwritten by the end of the first step (ivx_world_apply_forces primes them before it). A world with neither launches exactly what it launched
 * before and keeps host-set totals. If the world's bodies are later replaced by fewer than the sets refer to, the next apply or step is
 * IVX_ERR_STATE, before anything is launched; any other number of bodies gets a new plan at the next apply. */
int ivx_world_set_force_generators(ivx_world*, const ivx_force_generator*, size_t n);
/* DynamicGravityManager: the field's members in order and the gravitational constant (n == 0 removes the field; setting it again changes the
 * constant). IVX_ERR_INVALID: a body index out of range, a body listed twice (the reference panics in include_body). */
int ivx_world_set_dynamic_gravity(ivx_world*, const uint32_t* dynamic_bodies, size_t n, float gravitational_constant);
/* The stage on its own, enqueued on the context's stream: nothing when neither set is installed. */
int ivx_world_apply_forces(ivx_world*);
/* get_load_on_body for every field member in field order, as of the last apply (zero before the first one after a set call): 6 floats per member,
 * force then torque; `cap` counts members. Waits for the stream. Without a field nothing is written. */
int ivx_world_gravity_loads(ivx_world*, float* force3_torque3, size_t cap);
/* The stage over host arrays, the code the kernels run (tests). Validates like the two set calls. gravity_loads6 (6 floats per field member) may be NULL. */
int ivx_fg_apply_host(const ivx_force_generator*, size_t n, const uint32_t* gravity_bodies, size_t n_gravity, float gravitational_constant, ivx_rigid_body* dynamic,
                      size_t n_dynamic, const ivx_kinematic_body* kinematic, size_t n_kinematic, float* gravity_loads6);

/* ---- detailed drag inside the force stage (force.rs:146-147, detailed_drag.rs:200-243, drag_load.rs:42-67, medium.rs:11-16) -----------------------
 * The reference keeps drag load maps in a repository keyed by DragLoadMapID, a string hash; here a map lives in a numbered SLOT of the world's
 * table (at most 65 536 slots), resident on the device. Which name goes to which slot is the caller's business, as entity ids are elsewhere.
 * A detailed-drag generator names a dynamic body and a slot. The generators are a set of their own beside the force generators, as they are a
 * registry of their own in the reference (and ivx_fg_apply_host keeps refusing kind 6).
 *
 * Arithmetic, one function for the kernel and for ivx_fg_apply_host_drag, in the conventions stated above (float32, uncontracted):
 *   v      = momentum *recip mass
 *   v_rel  = v - medium.velocity;  s2 = dot(v_rel, v_rel);  nothing unless s2 > 0 (so nothing for a NaN)
 *   v_body = rotate(conjugate(q), v_rel);  d = v_body *recip sqrt(s2)
 *   phi    = atan2(d.y, d.x);  theta = acos(clamp(d.z, -1, 1)), each the double-precision function rounded once
 *   cell   = theta_idx * 2 n_theta + phi_idx, the indices those of ivx_drag_map_indices
 *   fs     = (((scaling * scaling) * mass_density) * drag_coefficient) * s2;  ts = scaling * fs
 *   total_force += fs * rotate(q, load.force);  total_torque += ts * rotate(q, load.torque)
 * Deliberate differences from the reference: the acos argument is clamped (as in ivx_drag_force_and_torque); phi's index is clamped (as in
 * ivx_drag_map_indices); a d with a non-finite component adds nothing — ivx_drag_force_and_torque refuses such a body, a stage cannot refuse
 * in the middle of a step. ivx_drag_force_and_torque itself stays as it was: it DIVIDES by mass and by the speed where the reference, and this
 * stage, multiply by the reciprocal (impact_math/src/vector.rs:679), sums its products without a stated association and takes atan2f / acosf;
 * the two agree to tolerance, not to the bit.
 * In the composition above the drag phase stands where the reference has it: behind the dynamic-kinematic springs and ahead of dynamic gravity;
 * inside the phase the generators apply in list order, and several may name one body. */
typedef struct {
    float mass_density;
    float velocity[3];
} ivx_uniform_medium; /* UniformMedium. 16 bytes. */
typedef struct {
    uint32_t body; /* index into the dynamic bodies */
    uint32_t map;  /* slot of the world's map table */
    float drag_coefficient, scaling;
} ivx_drag_generator; /* DetailedDragForce on one body. 16 bytes. */
typedef struct {
    const ivx_drag_load* loads; /* n_theta x 2 n_theta, theta-major; NULL: the slot holds no map */
    uint32_t n_theta, reserved;
} ivx_drag_map_view; /* one slot as ivx_fg_apply_host_drag reads it, in host memory. 16 bytes. */
/* The world's medium; a new world has UniformMedium::vacuum() (all zero). Takes effect at the next apply. */
int ivx_world_set_medium(ivx_world*, const ivx_uniform_medium*);
int ivx_world_medium(ivx_world*, ivx_uniform_medium*);
/* A host map into slot `slot` (n_theta in 1..2048); n_theta == 0 frees the slot. IVX_ERR_CAPACITY for a slot past 65 535; IVX_ERR_STATE when
 * the installed drag set names the slot that is to be freed (the set and the map stay). Replacing a map is ordered on the context's stream
 * behind an apply that still reads the old one. Maps and medium belong to the world: they outlive the sets. */
int ivx_world_set_drag_map(ivx_world*, uint32_t slot, const ivx_drag_load* map, uint32_t n_theta);
/* ivx_drag_load_map with the slot as destination: the same validation, passes and tiling; the map never crosses to the host. IVX_ERR_INVALID for
 * a grid of another context, IVX_ERR_STATE for a grid without a current mesh; a mesh of fewer than 3 indices gives a zero map. */
int ivx_world_set_drag_map_from_grid(ivx_world*, uint32_t slot, ivx_grid*, const float com[3], const ivx_drag_map_config*);
/* The slot's map as it is resident; cap_cells counts ivx_drag_load records. *n_theta is 0 for a slot without a map (nothing is written); map
 * NULL with cap_cells 0 asks for *n_theta alone. Waits for the stream. */
int ivx_world_drag_map_download(ivx_world*, uint32_t slot, ivx_drag_load* map, size_t cap_cells, uint32_t* n_theta);
/* The world's detailed-drag set, resident until replaced (n == 0 removes it). IVX_ERR_INVALID, with a message that names the generator (the set in
 * force then stays): a body past the world's dynamic bodies, a slot past the table, a slot that holds no map (the reference panics: "Tried to
 * obtain missing drag load map"). The set joins the other two: with any of the three installed every step ends with the force stage, and a world
 * whose bodies have been replaced by fewer than the set refers to gets IVX_ERR_STATE at the next apply or step. */
int ivx_world_set_detailed_drag(ivx_world*, const ivx_drag_generator*, size_t n);
/* ivx_fg_apply_host with the drag phase: the stage over host arrays, the code the kernels run (tests). Validates like the set calls. */
int ivx_fg_apply_host_drag(const ivx_force_generator*, size_t n, const uint32_t* gravity_bodies, size_t n_gravity, float gravitational_constant, ivx_rigid_body* dynamic,
                           size_t n_dynamic, const ivx_kinematic_body* kinematic, size_t n_kinematic, float* gravity_loads6, const ivx_drag_generator*, size_t n_drag,
                           const ivx_drag_map_view* maps, size_t n_maps, const ivx_uniform_medium*);

/* ---- SDF queries: distance, gradient and surface casts of a compiled program (csrc/sdf_query.hip) ------------------------------------------------
 * The value of a compiled atomic SDF program at arbitrary root-space points, and the three placements the reference's meta-SDF graph makes with it
 * (impact_voxel/src/generation/sdf/meta.rs): MetaClosestTranslationToSurface (:1620-1688, compute_translation_to_closest_point_on_surface :2411-2479),
 * MetaRayTranslationToSurface (:1690-1796, compute_spherecast_translation_to_surface :2534-2703) and MetaRotationToGradient (:1798-1863,
 * compute_rotation_to_gradient :2481-2532), all over sample_signed_distance_with_gradient (:2728-2770) and SDFGenerator::compute_signed_distance
 * (atomic.rs:877-1010): f32, uncontracted, one evaluation order per expression; NO domain test, early-out or clamp (the difference from ivx_sdf_sample).
 *   block positions (atomic.rs:1601-1660): origin = T * block_origin, position (i, j, k) = ((origin + i dx) + j dy), then += dz once for k = 1; a 2x2x2
 *   block's origin is p - 0.5, sample i*4 + j*2 + k; centre value = (((d0 + d1) + d2) ... + d7) * 0.125; gradient = 0.25 * the three bracketed
 *   differences of meta.rs:2763-2770. Leaves and combinations as in ivx_sdf_sample; scaling multiplies the top of the stack; translation and rotation are
 *   no-ops; a noise node adds noise * noise_scale at (o.z + k, o.y + j, o.x + i) in noise space, or at the per-voxel positions when its transform is
 *   rotated or scaled (atomic.rs:1423-1507), with the library's own noise (csrc/noise.hpp).
 *   similarities (impact_math/src/transform/similarity.rs:206-242): point -> rotate(scaling * p) + translation; vector -> rotate(scaling * v); the
 *   inverses rotate by the conjugate and multiply by 1 / scaling (impact_math's `/ f32` is `* recip`). normalized_from_if_above(v, 1e-8): norm squared
 *   > 1e-8 * 1e-8, then v / sqrt(norm squared). rotation_between_axes is glam's Quat::from_rotation_arc (DESIGN.md lists the glam forms whose bits
 *   are unpinned).
 * The program is the list, stack size and domain exactly as ivx_sdf_compile returns them (noise parameters in reserved[]); the query object keeps a
 * copy (and, with a context, a device copy) until it is destroyed. ctx == NULL: the object runs the host build of the functions the kernels run.
 * The kernels work eight lanes to an instance (one corner of the 2x2x2 block each) and keep one value-stack column per lane in LDS: 256 bytes per
 * stack level and wave. IVX_SDF_QUERY_MAX_STACK is bounded by that: 64 levels are 16 KiB per one-wave workgroup, which leaves ten waves on a
 * compute unit's 160 KiB; the host build holds the same number of levels on its call stack. */
#define IVX_SDF_QUERY_MAX_STACK 64u
#define IVX_SDF_QUERY_MAX_ITEMS (1u << 24) /* points or instances per call */
typedef struct ivx_sdf_query ivx_sdf_query;
/* The subject of a placement: its node-to-parent similarity and, for the cast only, the sphere in subject space (sphere_for_shape, meta.rs:1745-1765,
 * derived by the caller). 48 bytes. */
typedef struct {
    ivx_similarity subject_to_parent;
    float sphere_center[3];
    float sphere_radius;
} ivx_sdf_query_instance;
/* status: 0 where the reference returns Some, else the way it returned None */
#define IVX_SQ_OK 0u
#define IVX_SQ_ZERO_GRADIENT 1u         /* closest: gradient norm squared within 1e-8 of zero (meta.rs:2455) */
#define IVX_SQ_NO_GRADIENT_DIRECTION 2u /* cast, rotation: gradient direction below 1e-8 (meta.rs:2715, :2526) */
#define IVX_SQ_RAY_MISSES_DOMAIN 3u     /* cast: find_ray_intersection found none (meta.rs:2623, impact_geometry/src/axis_aligned_box.rs:420-455) */
#define IVX_SQ_DEGENERATE_DIRECTION 4u  /* cast: the direction in surface space is below 1e-8 (meta.rs:2579-2582) */
#define IVX_SQ_PENETRATING 5u           /* cast: the sphere starts below the surface (meta.rs:2644) */
#define IVX_SQ_LEFT_INTERVAL 6u         /* cast: the centre left the ray's domain interval (meta.rs:2682-2686) */
#define IVX_SQ_MAX_STEPS 7u             /* cast: max_steps without a crossing (meta.rs:2662-2667) */
#define IVX_SQ_DEGENERATE_Y_AXIS 8u     /* rotation: the subject's y-axis in parent space is below 1e-8 (meta.rs:2525) */
/* exit (status 0 only): which of the cast's two Some exits was taken */
#define IVX_SQ_EXIT_CONVERGED 0u /* within the tolerance (every closest and rotation result has this) */
#define IVX_SQ_EXIT_CROSSED 1u   /* max_steps reached after crossing the surface (meta.rs:2663-2664) */
/* 32 bytes. steps: closest: iteration_count when the loop ended; cast: step_count; rotation: 0. v: the translation in parent space (v[3] = 0), or the
 * rotation quaternion xyzw; all zero where status != 0. */
typedef struct {
    uint32_t status, steps;
    float v[4];
    uint32_t exit, reserved;
} ivx_sdf_query_result;
/* Walks the postfix list on the host (leaves push, kinds 3-6 need depth >= 1, kinds 7-9 need >= 2, the walk ends at depth 1). IVX_ERR_INVALID: a
 * list that does not reduce this way, a kind above 9, a depth above stack_size, a null argument; IVX_ERR_CAPACITY: stack_size above
 * IVX_SDF_QUERY_MAX_STACK. n_nodes == 0 is legal (nodes may be NULL): every distance is VoxelSignedDistance::MAX_F32 (0.02f * 127.0f), every gradient
 * zero. */
int ivx_sdf_query_create(ivx_ctx* ctx, const ivx_sdf_processed_node* nodes, size_t n_nodes, uint32_t stack_size, const float domain[6], ivx_sdf_query** out);
void ivx_sdf_query_destroy(ivx_sdf_query*); /* before ivx_shutdown of its context */
/* points: n x 3 floats in root space. which 0: compute_signed_distance, one float each; which 1: sample_signed_distance_with_gradient, four floats
 * each (centre value, gradient). Host arrays; one upload and one download through the object's pinned block; waits for the stream. */
int ivx_sdf_query_points(ivx_sdf_query*, int which, const float* points, size_t n, float* out);
/* surface_to_parent: the surface node's node_to_parent_transform. One result per instance, in order; two calls leave the same bytes. The reference's
 * constants (5 and 0.1; unit_y, 128, 0.1 and 0.5) are the Python mirror's defaults. IVX_ERR_INVALID for a safety_factor outside (0, 1] (the
 * reference asserts it). */
int ivx_sdf_query_closest(ivx_sdf_query*, const ivx_similarity* surface_to_parent, const ivx_sdf_query_instance* instances, size_t n, uint32_t max_iterations,
                          float max_distance, ivx_sdf_query_result* results);
int ivx_sdf_query_spherecast(ivx_sdf_query*, const ivx_similarity* surface_to_parent, const ivx_sdf_query_instance* instances, size_t n,
                             const float direction[3], uint32_t max_steps, float tolerance, float safety_factor, ivx_sdf_query_result* results);
int ivx_sdf_query_rotation(ivx_sdf_query*, const ivx_similarity* surface_to_parent, const ivx_sdf_query_instance* instances, size_t n,
                           ivx_sdf_query_result* results);

#ifdef __cplusplus
}
#endif
#endif
