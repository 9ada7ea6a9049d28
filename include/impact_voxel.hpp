// C++ host-side mirror of the reference's interface for the deformable-voxel path, header-only, above the C ABI of
// include/impact_voxel_hip.h. The reference is Rust; its types on this path are concrete structs, so the mirror
// keeps their names, method names and argument meaning (paths relative to /root/reference/engine/crates/):
//   SDFNode / SDFGraph / SDFGenerator        impact_voxel/src/generation/sdf/atomic.rs:55-181, 228-596, 1019-1148
//   SDFVoxelGenerator                        impact_voxel/src/generation.rs:204-258
//   VoxelObject                              impact_voxel/src/object.rs:239-404, 1136-1198; split_detection.rs:193-301; extraction.rs:78-119
//   VoxelObjectMesh                          impact_voxel/src/mesh.rs:286-456
//   VoxelObjectInertialPropertyManager       impact_voxel/src/object/inertia.rs:125-169
//   apply_sphere_absorption & co             impact_voxel/src/interaction/absorption.rs:801-1079
//   for_each_*_voxel_object_contact          impact_voxel/src/collidable.rs:859-1286
//   perform_physics_step / ConstraintSolver  impact_physics/src/lib.rs:31-110
//   CullingFrustum / VoxelChunkCullingPass   impact_voxel/src/mesh.rs:638-696, render_commands.rs:392-589
//   IntersectionManager (BoundingVolumeSet)  impact_intersection/src/lib.rs:39-150
// Errors: every C status other than IVX_OK becomes an impact_voxel::Error carrying ivx_last_error() — where the reference would
// return Err or panic on a violated precondition. Nothing here computes: it owns handles, sizes buffers and forwards.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "impact_voxel_hip.h"

namespace impact_voxel {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};
inline void check(int rc) {
    if (rc != IVX_OK) throw Error(rc, ivx_last_error());
}

class Context {
public:
    explicit Context(int device = 0, void* stream = nullptr) { check(ivx_init(device, stream, &ctx_)); }
    ~Context() {
        if (ctx_) ivx_shutdown(ctx_);
    }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    void synchronize() { check(ivx_synchronize(ctx_)); }
    ivx_ctx* handle() const { return ctx_; }

private:
    ivx_ctx* ctx_ = nullptr;
};

// ---- SDF graph ---------------------------------------------------------------------------------------------------------------
using SDFNodeID = uint32_t;
struct SDFNode {
    ivx_sdf_node rec{};
    static SDFNode make(uint32_t kind, uint32_t c1, uint32_t c2, std::array<float, 4> p) {
        SDFNode n;
        n.rec.kind = kind, n.rec.child1 = c1, n.rec.child2 = c2, n.rec.pad = 0;
        for (int i = 0; i < 4; ++i) n.rec.p[i] = p[i];
        return n;
    }
    static SDFNode new_sphere(float radius) { return make(0, 0, 0, {radius, 0, 0, 0}); }
    static SDFNode new_capsule(float segment_length, float radius) { return make(1, 0, 0, {segment_length, radius, 0, 0}); }
    static SDFNode new_box(std::array<float, 3> extents) { return make(2, 0, 0, {extents[0], extents[1], extents[2], 0}); }
    static SDFNode new_translation(SDFNodeID child, std::array<float, 3> t) { return make(3, child, 0, {t[0], t[1], t[2], 0}); }
    static SDFNode new_rotation(SDFNodeID child, std::array<float, 4> quaternion_xyzw) { return make(4, child, 0, quaternion_xyzw); }
    static SDFNode new_scaling(SDFNodeID child, float scaling) { return make(5, child, 0, {scaling, 0, 0, 0}); }
    static SDFNode new_union(SDFNodeID a, SDFNodeID b, float smoothness) { return make(7, a, b, {smoothness, 0, 0, 0}); }
    static SDFNode new_subtraction(SDFNodeID a, SDFNodeID b, float smoothness) { return make(8, a, b, {smoothness, 0, 0, 0}); }
    static SDFNode new_intersection(SDFNodeID a, SDFNodeID b, float smoothness) { return make(9, a, b, {smoothness, 0, 0, 0}); }
};
class SDFGraph {
public:
    SDFNodeID add_node(const SDFNode& n) {  // the last node added is the root (atomic.rs:1037-1046)
        nodes_.push_back(n.rec);
        root_ = (SDFNodeID)nodes_.size() - 1;
        return root_;
    }
    const std::vector<ivx_sdf_node>& nodes() const { return nodes_; }
    SDFNodeID root_node_id() const { return root_; }

private:
    std::vector<ivx_sdf_node> nodes_;
    SDFNodeID root_ = 0;
};
class SDFGenerator {  // SDFGraph::build (atomic.rs:228-596)
public:
    explicit SDFGenerator(const SDFGraph& g) {
        nodes_.resize(4 * g.nodes().size() + 64);
        size_t n = 0;
        check(ivx_sdf_compile(g.nodes().data(), g.nodes().size(), g.root_node_id(), nodes_.data(), nodes_.size(), &n, domain_, &stack_size_));
        nodes_.resize(n);
    }
    const std::vector<ivx_sdf_processed_node>& nodes() const { return nodes_; }
    uint32_t stack_size() const { return stack_size_; }
    const float* domain() const { return domain_; }

private:
    std::vector<ivx_sdf_processed_node> nodes_;
    float domain_[6] = {0, 0, 0, 0, 0, 0};
    uint32_t stack_size_ = 0;
};
// the two voxel type generators (generation/voxel_type.rs:18-36): what ivx_grid_set_voxel_type_noise is handed
struct SameVoxelTypeGenerator {
    uint8_t voxel_type = 0;
};
struct GradientNoiseVoxelTypeGenerator {  // (the reference's list of voxel types enters by its length alone)
    uint32_t n_voxel_types = 1;
    float noise_frequency = 0.0f;
    float voxel_type_frequency = 0.0f;
    uint32_t seed = 0;
};
class SDFVoxelGenerator {  // generation.rs:204-258
public:
    SDFVoxelGenerator(float voxel_extent, SDFGenerator generator, uint8_t voxel_type = 0)
        : extent_(voxel_extent), gen_(std::move(generator)), type_(voxel_type) {
        check(ivx_sdf_grid_shape(gen_.domain(), shape_, center_));
    }
    SDFVoxelGenerator(float voxel_extent, SDFGenerator generator, SameVoxelTypeGenerator types)
        : SDFVoxelGenerator(voxel_extent, std::move(generator), types.voxel_type) {}
    SDFVoxelGenerator(float voxel_extent, SDFGenerator generator, GradientNoiseVoxelTypeGenerator types)
        : SDFVoxelGenerator(voxel_extent, std::move(generator), (uint8_t)0) {
        noise_ = types;
        noise_on_ = true;
    }
    // n_voxel_types = 0: SameVoxelTypeGenerator(voxel_type())
    GradientNoiseVoxelTypeGenerator type_noise() const { return noise_on_ ? noise_ : GradientNoiseVoxelTypeGenerator{0, 0.0f, 0.0f, 0}; }
    float voxel_extent() const { return extent_; }
    std::array<uint32_t, 3> grid_shape() const { return {shape_[0], shape_[1], shape_[2]}; }
    std::array<uint32_t, 3> chunk_counts() const { return {(shape_[0] + 15) / 16, (shape_[1] + 15) / 16, (shape_[2] + 15) / 16}; }
    const SDFGenerator& sdf_generator() const { return gen_; }
    const uint32_t* shape() const { return shape_; }
    const float* shifted_grid_center() const { return center_; }
    uint8_t voxel_type() const { return type_; }

private:
    float extent_;
    SDFGenerator gen_;
    uint8_t type_;
    GradientNoiseVoxelTypeGenerator noise_;
    bool noise_on_ = false;
    uint32_t shape_[3] = {0, 0, 0};
    float center_[3] = {0, 0, 0};
};

// ---- voxel object -------------------------------------------------------------------------------------------------------------
struct Isometry3 {  // rotation (x, y, z, w) then translation
    std::array<float, 4> rotation{0, 0, 0, 1};
    std::array<float, 3> translation{0, 0, 0};
};
struct AbsorptionOutcome {
    ivx_absorb_result result{};
    std::vector<uint32_t> emptied_by_type;
    std::vector<uint8_t> invalidated_mesh_chunks;
};
class VoxelObject;
struct DisconnectedVoxelObject {  // extraction.rs:47-58
    std::unique_ptr<VoxelObject> voxel_object;
    std::array<uint32_t, 3> origin_offset_in_parent{0, 0, 0};
    ivx_region_desc moved{};
};

class VoxelObject {
public:
    VoxelObject(Context& ctx, std::array<uint32_t, 3> chunk_counts, float voxel_extent) : ctx_(&ctx), extent_(voxel_extent), cc_(chunk_counts) {
        check(ivx_grid_create(ctx.handle(), cc_.data(), voxel_extent, 0, cc_[0], &g_));
    }
    ~VoxelObject() {
        if (g_) ivx_grid_destroy(g_);
    }
    VoxelObject(const VoxelObject&) = delete;
    VoxelObject& operator=(const VoxelObject&) = delete;

    static std::unique_ptr<VoxelObject> generate_without_derived_state(Context& ctx, const SDFVoxelGenerator& gen) {
        auto o = std::make_unique<VoxelObject>(ctx, gen.chunk_counts(), gen.voxel_extent());
        const auto& n = gen.sdf_generator().nodes();
        const GradientNoiseVoxelTypeGenerator tn = gen.type_noise();
        check(ivx_grid_set_voxel_type_noise(o->g_, tn.n_voxel_types, tn.noise_frequency, tn.voxel_type_frequency, tn.seed));
        check(ivx_sdf_sample(o->g_, n.data(), n.size(), gen.sdf_generator().stack_size(), gen.shape(), gen.shifted_grid_center(), gen.voxel_type()));
        return o;
    }
    static std::unique_ptr<VoxelObject> generate(Context& ctx, const SDFVoxelGenerator& gen) {  // object.rs:239-244
        auto o = generate_without_derived_state(ctx, gen);
        o->compute_all_derived_state();       // (the reference updates the ranges first; here they are reduced from per-chunk boxes the derive
        o->update_occupied_voxel_ranges();    //  sweep leaves, the result is the same: emptiness does not change in between)
        return o;
    }
    void compute_all_derived_state() {  // object.rs:1136-1145
        check(ivx_derive_state(g_));
        check(ivx_label_regions(g_, &regions_));
    }
    std::array<uint32_t, 12> update_occupied_voxel_ranges() {
        std::array<uint32_t, 12> r{};
        check(ivx_occupied_ranges(g_, r.data()));
        return r;
    }
    uint32_t count_regions() {
        check(ivx_label_regions(g_, &regions_));
        return regions_;
    }
    std::optional<DisconnectedVoxelObject> extract_any_disconnected_region() {  // extraction.rs:78-119
        ivx_grid* child = nullptr;
        DisconnectedVoxelObject d;
        int outcome = 0;
        check(ivx_split_off_smallest_region(g_, &child, d.origin_offset_in_parent.data(), &outcome, &d.moved));
        if (outcome != 1) return std::nullopt;
        d.voxel_object = std::unique_ptr<VoxelObject>(new VoxelObject(*ctx_, child, extent_));
        return d;
    }
    // interaction/absorption.rs:801-889 with the shape in the object's normalized space
    AbsorptionOutcome absorb_sphere(std::array<float, 3> center, float influence_radius, float sphere_radius, const std::array<float, 256>& densities) {
        AbsorptionOutcome a = fresh_outcome();
        check(ivx_absorb_sphere(g_, center.data(), influence_radius, sphere_radius, densities.data(), &a.result, a.emptied_by_type.data(),
                                a.invalidated_mesh_chunks.data()));
        return a;
    }
    AbsorptionOutcome absorb_capsule(std::array<float, 3> segment_start, std::array<float, 3> segment_vector, float influence_radius, float capsule_radius,
                                     const std::array<float, 256>& densities) {
        AbsorptionOutcome a = fresh_outcome();
        check(ivx_absorb_capsule(g_, segment_start.data(), segment_vector.data(), influence_radius, capsule_radius, densities.data(), &a.result,
                                 a.emptied_by_type.data(), a.invalidated_mesh_chunks.data()));
        return a;
    }
    // collidable.rs:1098-1127 (sphere collidable in world space, transform_to_object_space of this object)
    std::vector<ivx_contact> sphere_contacts(const Isometry3& to_object, std::array<float, 3> center, float radius, uint64_t id_a, uint64_t id_b, uint32_t body_a,
                                             uint32_t body_b, std::array<float, 3> response, size_t capacity = 65536) {
        std::vector<ivx_contact> out(capacity);
        size_t n = 0;
        check(ivx_sphere_voxel_object_contacts(g_, to_object.rotation.data(), to_object.translation.data(), center.data(), radius, id_a, id_b, body_a, body_b,
                                               response.data(), out.data(), capacity, &n));
        out.resize(n);
        return out;
    }
    // collidable.rs:859-1049: contacts between this object (A) and `other` (B); both need current collision probes
    std::vector<ivx_contact> mutual_contacts(const Isometry3& to_object, std::array<float, 3> center_of_mass, VoxelObject& other, const Isometry3& other_to_object,
                                             std::array<float, 3> other_center_of_mass, uint64_t id_a, uint64_t id_b, uint32_t body_a, uint32_t body_b,
                                             std::array<float, 3> response, size_t capacity = 65536) {
        std::vector<ivx_contact> out(capacity);
        size_t n = 0;
        check(ivx_mutual_voxel_object_contacts(g_, to_object.rotation.data(), to_object.translation.data(), center_of_mass.data(), other.g_,
                                               other_to_object.rotation.data(), other_to_object.translation.data(), other_center_of_mass.data(), id_a, id_b,
                                               body_a, body_b, response.data(), out.data(), capacity, &n));
        out.resize(n);
        return out;
    }
    // VoxelObjectCollisionProbes (collidable.rs:361-433): recompute over the current mesh, or follow a mesh sync
    size_t recompute_collision_probes() {
        size_t n = 0;
        check(ivx_collision_probes_recompute(g_, &n));
        return n;
    }
    size_t sync_collision_probes(const std::vector<uint8_t>& invalidated_mesh_chunks) {
        size_t n = 0;
        check(ivx_collision_probes_sync(g_, invalidated_mesh_chunks.data(), &n));
        return n;
    }
    struct Dense {
        std::vector<int8_t> sdf;
        std::vector<uint8_t> type, flags, local_labels;
        std::vector<ivx_chunk_info> info;
    };
    Dense download() const {
        Dense d;
        const size_t nc = (size_t)cc_[0] * cc_[1] * cc_[2], nv = nc * 4096;
        d.sdf.resize(nv), d.type.resize(nv), d.flags.resize(nv), d.local_labels.resize(nv), d.info.resize(nc);
        check(ivx_grid_download_dense(g_, d.sdf.data(), d.type.data(), d.flags.data(), d.local_labels.data(), d.info.data(), nv));
        return d;
    }
    float voxel_extent() const { return extent_; }
    std::array<uint32_t, 3> chunk_counts() const { return cc_; }
    size_t n_chunks() const { return (size_t)cc_[0] * cc_[1] * cc_[2]; }
    ivx_grid* handle() const { return g_; }

private:
    VoxelObject(Context& ctx, ivx_grid* adopted, float extent) : ctx_(&ctx), g_(adopted), extent_(extent) {
        uint32_t c[3];
        check(ivx_grid_chunk_counts(g_, c));
        cc_ = {c[0], c[1], c[2]};
    }
    AbsorptionOutcome fresh_outcome() const {
        AbsorptionOutcome a;
        a.emptied_by_type.assign(256, 0);
        a.invalidated_mesh_chunks.assign(n_chunks(), 0);
        return a;
    }
    Context* ctx_;
    ivx_grid* g_ = nullptr;
    float extent_;
    std::array<uint32_t, 3> cc_{0, 0, 0};
    uint32_t regions_ = 0;
};

class VoxelObjectMesh {  // mesh.rs:44-58, 286-456; the buffers stay in HBM
public:
    static VoxelObjectMesh create(VoxelObject& o) {
        VoxelObjectMesh m(o);
        m.recreate();
        return m;
    }
    void recreate() { check(ivx_remesh(o_->handle(), &counts_)); }
    void sync_with_voxel_object(const std::vector<uint8_t>& invalidated_mesh_chunks) { check(ivx_mesh_sync(o_->handle(), invalidated_mesh_chunks.data(), &counts_)); }
    size_t n_vertices() const { return counts_.n_vertices; }
    size_t n_indices() const { return counts_.n_indices; }
    size_t n_chunks() const { return counts_.n_submeshes; }
    struct Buffers {
        std::vector<float> positions, normal_vectors;
        std::vector<uint32_t> indices;
        std::vector<uint8_t> index_materials;
        std::vector<ivx_submesh> chunk_submeshes;
    };
    Buffers download() const {
        Buffers b;
        b.positions.resize(3 * n_vertices()), b.normal_vectors.resize(3 * n_vertices()), b.indices.resize(n_indices());
        b.index_materials.resize(8 * n_indices()), b.chunk_submeshes.resize(n_chunks());
        check(ivx_mesh_download(o_->handle(), b.positions.data(), b.normal_vectors.data(), b.indices.data(), b.index_materials.data(), b.chunk_submeshes.data()));
        return b;
    }

private:
    explicit VoxelObjectMesh(VoxelObject& o) : o_(&o) {}
    VoxelObject* o_;
    ivx_mesh_counts counts_{};
};

class VoxelObjectInertialPropertyManager {  // object/inertia.rs:20-25, 125-169
public:
    static VoxelObjectInertialPropertyManager initialized_from(VoxelObject& o, const std::array<float, 256>& voxel_type_densities) {
        VoxelObjectInertialPropertyManager m;
        check(ivx_inertia(o.handle(), voxel_type_densities.data(), &m.moments_));
        return m;
    }
    double mass() const { return moments_.m64[0]; }
    std::array<double, 3> derive_center_of_mass() const { return {moments_.m64[1] / moments_.m64[0], moments_.m64[2] / moments_.m64[0], moments_.m64[3] / moments_.m64[0]}; }
    const ivx_moments& moments() const { return moments_; }

private:
    ivx_moments moments_{};
};

// ---- chunk culling (impact_voxel/src/mesh.rs:638-696, render_commands.rs:392-589): the draw arguments of every object under every view ----
struct CullingFrustum {
    // CullingFrustum::for_transformed_frustum / ::for_transformed_orthographic_frustum with the transform to normalised object space folded in
    static ivx_culling_frustum from_view(const ivx_cull_view& view, const ivx_cull_pair& object_to_view, float chunk_extent) {
        ivx_culling_frustum f{};
        check(ivx_culling_frustum_from_view(&view, &object_to_view, chunk_extent, &f));
        return f;
    }
};
class VoxelChunkCullingPass {
public:
    struct Result {
        std::vector<ivx_cull_region> layout;  // per view: where its region lies in the argument buffer
        std::vector<ivx_cull_count> counts;   // per view: draws, indices drawn (empty after `enqueue` until `collect`)
    };
    explicit VoxelChunkCullingPass(Context& ctx) : ctx_(&ctx) {}
    // pairs are view-major (views.size() x objects.size()); `offsets` empty: per-object buffers; mode IVX_CULL_ZEROED or IVX_CULL_COMPACTED
    Result record(const std::vector<VoxelObject*>& objects, const std::vector<ivx_cull_view>& views, const std::vector<ivx_cull_pair>& pairs, uint32_t mode,
                  const std::vector<ivx_cull_object>& offsets = {}) {
        Result r = sized(views.size(), true);
        const std::vector<ivx_grid*> g = handles(objects);
        check(ivx_cull_many(g.data(), g.size(), offsets.empty() ? nullptr : offsets.data(), views.data(), views.size(), pairs.data(), mode, r.layout.data(), r.counts.data()));
        return r;
    }
    Result enqueue(const std::vector<VoxelObject*>& objects, const std::vector<ivx_cull_view>& views, const std::vector<ivx_cull_pair>& pairs, uint32_t mode,
                   const std::vector<ivx_cull_object>& offsets = {}) {
        Result r = sized(views.size(), false);
        const std::vector<ivx_grid*> g = handles(objects);
        check(ivx_cull_many_enqueue(g.data(), g.size(), offsets.empty() ? nullptr : offsets.data(), views.data(), views.size(), pairs.data(), mode, r.layout.data()));
        return r;
    }
    void collect(Result& r) {
        r.counts.resize(r.layout.size());
        check(ivx_cull_collect(ctx_->handle(), r.counts.data(), r.counts.size()));
    }
    Result record_with_frusta(const std::vector<VoxelObject*>& objects, const std::vector<ivx_culling_frustum>& frusta, const std::vector<uint32_t>& view_flags, uint32_t mode,
                              const std::vector<uint32_t>& pair_flags = {}, const std::vector<ivx_cull_object>& offsets = {}) {
        Result r = sized(view_flags.size(), true);
        const std::vector<ivx_grid*> g = handles(objects);
        check(ivx_cull_many_frusta(g.data(), g.size(), offsets.empty() ? nullptr : offsets.data(), frusta.data(), view_flags.data(), pair_flags.empty() ? nullptr : pair_flags.data(),
                                   view_flags.size(), mode, r.layout.data(), r.counts.data()));
        return r;
    }
    std::vector<ivx_culling_frustum> frusta(const std::vector<ivx_cull_view>& views, const std::vector<ivx_cull_pair>& pairs, const std::vector<float>& chunk_extents) {
        std::vector<ivx_culling_frustum> out(views.size() * chunk_extents.size());
        check(ivx_cull_frusta(ctx_->handle(), views.data(), views.size(), pairs.data(), chunk_extents.data(), chunk_extents.size(), out.data()));
        return out;
    }
    // one view's region as raw bytes (ivx_draw_args or ivx_draw_indexed_args by the region's stride)
    std::vector<uint8_t> download(const Result& r, uint32_t view, ivx_cull_count* count = nullptr) {
        std::vector<uint8_t> args((size_t)r.layout.at(view).n_slots * r.layout.at(view).stride);
        check(ivx_cull_download(ctx_->handle(), view, args.data(), args.size(), count, nullptr, 0));
        return args;
    }
    void* device_ptr(int which) const { return ivx_cull_device_ptr(ctx_->handle(), which); }

private:
    static Result sized(size_t n_views, bool with_counts) {
        Result r;
        r.layout.resize(n_views);
        if (with_counts) r.counts.resize(n_views);
        return r;
    }
    static std::vector<ivx_grid*> handles(const std::vector<VoxelObject*>& objects) {
        std::vector<ivx_grid*> g;
        for (VoxelObject* o : objects) g.push_back(o->handle());
        return g;
    }
    Context* ctx_;
};

// ---- bounding volumes (impact_intersection/src/lib.rs): world boxes, all intersecting pairs, region queries --------------------------------
// add_bounding_volume_to_hierarchy's box: aabb_of_transformed of the model box under the similarity
inline ivx_aabb world_aabb(const ivx_aabb& model, const ivx_similarity& model_to_world) {
    ivx_aabb out{};
    check(ivx_bv_world_aabb(&model, &model_to_world, &out));
    return out;
}
// the flat form of the IntersectionManager: one set of world boxes per context, resident on the device until the next `set`
class BoundingVolumeSet {
public:
    explicit BoundingVolumeSet(Context& ctx) : ctx_(&ctx) {}
    // `similarities` empty: the boxes are world boxes already; `kinds` empty: all dynamic (IVX_BV_DYNAMIC / _STATIC / _PHANTOM)
    void set(const std::vector<ivx_aabb>& model_boxes, const std::vector<ivx_similarity>& similarities = {}, const std::vector<uint32_t>& kinds = {}) {
        check(ivx_bv_set(ctx_->handle(), model_boxes.data(), similarities.empty() ? nullptr : similarities.data(), kinds.empty() ? nullptr : kinds.data(), model_boxes.size()));
    }
    // sync_voxel_object_bounding_volume for every object, then the same
    void set(const std::vector<VoxelObject*>& objects, const std::vector<ivx_similarity>& similarities = {}, const std::vector<uint32_t>& kinds = {}) {
        std::vector<ivx_grid*> g;
        for (VoxelObject* o : objects) g.push_back(o->handle());
        check(ivx_bv_set_grids(g.data(), g.size(), similarities.empty() ? nullptr : similarities.data(), kinds.empty() ? nullptr : kinds.data()));
    }
    static ivx_aabb model_aabb(VoxelObject& object) {
        ivx_aabb out{};
        check(ivx_grid_model_aabb(object.handle(), &out));
        return out;
    }
    std::vector<ivx_aabb> world_boxes(size_t n) {
        std::vector<ivx_aabb> out(n);
        check(ivx_bv_download(ctx_->handle(), out.data(), out.size(), nullptr));
        return out;
    }
    ivx_aabb total_bounding_volume() {
        ivx_aabb out{};
        check(ivx_bv_download(ctx_->handle(), nullptr, 0, &out));
        return out;
    }
    // for_each_intersecting_bounding_volume_pair: (a, b), a < b, sorted; mode IVX_BV_ALL_PAIRS or IVX_BV_DYNAMIC_PAIRS
    std::vector<std::array<uint32_t, 2>> intersecting_pairs(uint32_t mode = IVX_BV_ALL_PAIRS) {
        std::vector<std::array<uint32_t, 2>> out;
        size_t n = 0;
        int rc = ivx_bv_pairs(ctx_->handle(), mode, nullptr, 0, &n);  // (counts, and leaves the pairs on the device)
        check(rc);
        out.resize(n);
        if (n) check(ivx_bv_pairs(ctx_->handle(), mode, &out[0][0], out.size(), &n));
        return out;
    }
    // the hierarchy over the set (hierarchy.rs): built on request, valid until the next `set`; its pair pass returns the bytes of the flat one
    void build_hierarchy() { check(ivx_bv_build_hierarchy(ctx_->handle())); }
    std::vector<ivx_bv_node> hierarchy(size_t n_objects, std::vector<uint32_t>* leaf_objects = nullptr) {
        std::vector<ivx_bv_node> nodes(n_objects ? n_objects - 1 : 0);
        if (leaf_objects) leaf_objects->resize(n_objects);
        size_t n_nodes = 0;
        check(ivx_bv_hierarchy_download(ctx_->handle(), nodes.data(), nodes.size(), leaf_objects ? leaf_objects->data() : nullptr, n_objects, &n_nodes));
        return nodes;
    }
    std::vector<std::array<uint32_t, 2>> intersecting_pairs_hierarchy(uint32_t mode = IVX_BV_ALL_PAIRS) {
        std::vector<std::array<uint32_t, 2>> out;
        size_t n = 0;
        check(ivx_bv_pairs_hierarchy(ctx_->handle(), mode, nullptr, 0, &n));  // (counts, and leaves the pairs on the device)
        out.resize(n);
        if (n) check(ivx_bv_pairs_hierarchy(ctx_->handle(), mode, &out[0][0], out.size(), &n));
        return out;
    }
    static uint64_t morton_key(const ivx_aabb& frame, const ivx_aabb& box, uint32_t index) {
        uint64_t key = 0;
        check(ivx_bv_morton_key(&frame, &box, index, &key));
        return key;
    }
    // for_each_bounding_volume_in_axis_aligned_box / _in_sphere / _maybe_in_frustum / _maybe_in_oriented_box: ceil(n / 64) mask words per query
    std::vector<uint64_t> query(const std::vector<ivx_bv_query>& queries, size_t n_objects, std::vector<uint32_t>* counts = nullptr) {
        std::vector<uint64_t> masks(queries.size() * ((n_objects + 63) / 64));
        if (counts) counts->resize(queries.size());
        check(ivx_bv_queries(ctx_->handle(), queries.data(), queries.size(), masks.data(), counts ? counts->data() : nullptr));
        return masks;
    }
    static ivx_bv_query frustum_query(const float planes[6][4]) {
        ivx_bv_query q{};
        check(ivx_bv_frustum_query(planes, &q));
        return q;
    }
    void* device_ptr(int which) const { return ivx_bv_device_ptr(ctx_->handle(), which); }

private:
    Context* ctx_;
};

// ---- frame instances (impact_scene/src/model.rs:171-297, light.rs:85-848): kept sets, view transforms and cull pairs of every view of a pass ----
// One instance per object of the context's BoundingVolumeSet; a pass after a `query` on that set. The light geometry, material buffering and
// scene-graph group transforms stay with the caller.
class FrameInstances {
public:
    struct Outputs {
        std::vector<ivx_cull_pair> pairs;  // view-major, views x objects
        std::vector<uint32_t> offsets;     // views + 1
        std::vector<uint32_t> objects;     // the kept objects of every view, ascending within a view
        std::vector<ivx_similarity> transforms;  // ... and their model-to-view transforms (the view's instance-transform range)
        std::vector<uint64_t> kept_masks;  // views x ceil(objects / 64)
    };
    explicit FrameInstances(Context& ctx) : ctx_(&ctx) {}
    void set_instances(const std::vector<ivx_fi_instance>& instances) { check(ivx_fi_set_instances(ctx_->handle(), instances.data(), instances.size())); }
    // enqueue only: nothing waits and nothing comes back
    void enqueue(const std::vector<ivx_fi_view>& views) { check(ivx_fi_views(ctx_->handle(), views.data(), views.size(), nullptr)); }
    // ... or with the reductions of every view
    std::vector<ivx_fi_view_result> views(const std::vector<ivx_fi_view>& views) {
        std::vector<ivx_fi_view_result> r(views.size());
        check(ivx_fi_views(ctx_->handle(), views.data(), views.size(), r.data()));
        return r;
    }
    Outputs download(size_t n_views, size_t n_objects) {
        Outputs o;
        o.pairs.resize(n_views * n_objects), o.offsets.resize(n_views + 1), o.kept_masks.resize(n_views * ((n_objects + 63) / 64));
        size_t total = 0;
        check(ivx_fi_download(ctx_->handle(), o.pairs.data(), o.pairs.size(), o.offsets.data(), o.offsets.size(), nullptr, nullptr, 0, o.kept_masks.data(), o.kept_masks.size(), &total));
        o.objects.resize(total), o.transforms.resize(total);
        check(ivx_fi_download(ctx_->handle(), nullptr, 0, nullptr, 0, o.objects.data(), o.transforms.data(), total, nullptr, 0, nullptr));
        return o;
    }
    void* device_ptr(int which) const { return ivx_fi_device_ptr(ctx_->handle(), which); }
    // the cull of voxel objects under the views of the last pass, their pairs taken on the device (`object_indices` empty: object g is instance g)
    std::vector<ivx_cull_region> enqueue_cull(const std::vector<VoxelObject*>& objects, const std::vector<uint32_t>& object_indices, const std::vector<ivx_cull_view>& views,
                                              uint32_t mode, const std::vector<ivx_cull_object>& offsets = {}) {
        std::vector<ivx_grid*> g;
        for (VoxelObject* o : objects) g.push_back(o->handle());
        std::vector<ivx_cull_region> layout(views.size());
        check(ivx_cull_many_resident(g.data(), g.size(), offsets.empty() ? nullptr : offsets.data(), object_indices.empty() ? nullptr : object_indices.data(), views.data(),
                                     views.size(), mode, layout.data()));
        return layout;
    }
    // the whole stage on the host, with the functions the kernels run
    static std::vector<ivx_fi_view_result> views_host(const std::vector<ivx_aabb>& world_boxes, const std::vector<ivx_fi_instance>& instances, const std::vector<uint64_t>& masks,
                                                      size_t n_queries, const std::vector<ivx_fi_view>& views, const std::vector<uint64_t>& previous_kept,
                                                      size_t n_previous_views, Outputs* out = nullptr) {
        const size_t n = world_boxes.size(), nv = views.size();
        std::vector<ivx_fi_view_result> r(nv);
        if (out) out->pairs.resize(nv * n), out->offsets.resize(nv + 1), out->objects.resize(nv * n), out->transforms.resize(nv * n), out->kept_masks.resize(nv * ((n + 63) / 64));
        check(ivx_fi_views_host(world_boxes.data(), n, instances.data(), masks.data(), n_queries, views.data(), nv, previous_kept.empty() ? nullptr : previous_kept.data(),
                                n_previous_views, out ? out->pairs.data() : nullptr, out ? out->offsets.data() : nullptr, out ? out->objects.data() : nullptr,
                                out ? out->transforms.data() : nullptr, nv * n, out ? out->kept_masks.data() : nullptr, r.data()));
        if (out) out->objects.resize(out->offsets.back()), out->transforms.resize(out->offsets.back());
        return r;
    }

private:
    Context* ctx_;
};

// ---- motion drivers of kinematic bodies (impact_physics/src/driven_motion/): the reference's setup structs in their #[repr(C)] layouts ------
// (all fields are f32: a record's parameters are the struct's bytes). `driver(kinematic_body_index)` gives the record ivx_world_set_motion_drivers takes.
namespace detail {
template <class T>
ivx_motion_driver motion_driver(uint32_t kind, uint32_t body, const T& setup) {
    static_assert(sizeof(T) <= sizeof(ivx_motion_driver::p) && sizeof(T) % sizeof(float) == 0, "a setup struct fits the record's parameters");
    ivx_motion_driver d{};
    d.kind = kind, d.body = body;
    const float* f = reinterpret_cast<const float*>(&setup);
    for (size_t i = 0; i < sizeof(T) / sizeof(float); ++i) d.p[i] = f[i];
    return d;
}
}  // namespace detail
struct CircularTrajectory {  // circular.rs:52-68
    float initial_time;
    float orientation[4];  // x, y, z, w
    float center_position[3];
    float radius, period;
    ivx_motion_driver driver(uint32_t body) const { return detail::motion_driver(IVX_MD_CIRCULAR, body, *this); }
};
struct ConstantAccelerationTrajectory {  // constant_acceleration.rs:52-61
    float initial_time;
    float initial_position[3], initial_velocity[3], acceleration[3];
    ivx_motion_driver driver(uint32_t body) const { return detail::motion_driver(IVX_MD_CONSTANT_ACCELERATION, body, *this); }
};
struct HarmonicOscillatorTrajectory {  // harmonic_oscillation.rs:55-64
    float center_time;
    float center_position[3], direction[3];
    float amplitude, period;
    ivx_motion_driver driver(uint32_t body) const { return detail::motion_driver(IVX_MD_HARMONIC, body, *this); }
};
struct OrbitalTrajectory {  // orbit.rs:52-70
    float periapsis_time;
    float orientation[4];  // x, y, z, w
    float focal_position[3];
    float semi_major_axis, eccentricity, period;
    ivx_motion_driver driver(uint32_t body) const { return detail::motion_driver(IVX_MD_ORBITAL, body, *this); }
};
struct ConstantRotation {  // constant_rotation.rs:51-59; AngularVelocityC = unit axis + angular speed
    float initial_time;
    float initial_orientation[4];  // x, y, z, w
    float axis_of_rotation[3];
    float angular_speed;
    ivx_motion_driver driver(uint32_t body) const { return detail::motion_driver(IVX_MD_CONSTANT_ROTATION, body, *this); }
};
static_assert(sizeof(CircularTrajectory) == 40 && sizeof(ConstantAccelerationTrajectory) == 40 && sizeof(HarmonicOscillatorTrajectory) == 36 &&
                  sizeof(OrbitalTrajectory) == 44 && sizeof(ConstantRotation) == 36 && sizeof(ivx_motion_driver) == 64,
              "motion driver layouts");

// ---- force generators of dynamic bodies (impact_physics/src/force/): the reference's setup structs ------------------------------------------
// `record(dynamic_body_index, ..)` gives the record ivx_world_set_force_generators takes. Entity ids and AnchorManager bookkeeping stay with the
// caller: a body is given by its index, an anchor as that index plus the body-space point.
namespace detail {
inline ivx_force_generator force_generator(uint32_t kind, uint32_t body, uint32_t body_b) {
    ivx_force_generator g{};
    g.kind = kind, g.body = body, g.body_b = body_b;
    return g;
}
inline void put3(float* p, const float v[3]) { p[0] = v[0], p[1] = v[1], p[2] = v[2]; }
}  // namespace detail
struct ConstantAcceleration {  // constant_acceleration.rs:52-103
    float acceleration[3];
    static constexpr float EARTH_DOWNWARD_ACCELERATION = 9.81f;
    static ConstantAcceleration downward(float acceleration) { return ConstantAcceleration{{0.0f, -acceleration, 0.0f}}; }
    static ConstantAcceleration earth() { return downward(EARTH_DOWNWARD_ACCELERATION); }
    ivx_force_generator record(uint32_t body) const {
        ivx_force_generator g = detail::force_generator(IVX_FG_CONSTANT_ACCELERATION, body, 0);
        detail::put3(g.p, acceleration);
        return g;
    }
};
struct LocalForce {  // local_force.rs:29-34
    float force[3];  // body frame
    float point[3];  // body frame
    ivx_force_generator record(uint32_t body) const {
        ivx_force_generator g = detail::force_generator(IVX_FG_LOCAL_FORCE, body, 0);
        detail::put3(g.p, force), detail::put3(g.p + 3, point);
        return g;
    }
};
struct Spring {  // spring_force.rs:125-138, 285-313
    float stiffness, damping, rest_length, slack_length;
    static Spring standard(float stiffness, float damping, float rest_length) { return Spring{stiffness, damping, rest_length, 0.0f}; }
    static Spring elastic_band(float stiffness, float damping, float slack_length) { return Spring{stiffness, damping, slack_length, slack_length}; }
};
namespace detail {
inline ivx_force_generator spring_generator(uint32_t kind, uint32_t body_1, uint32_t body_2, const float point_1[3], const float point_2[3], const Spring& s) {
    ivx_force_generator g = force_generator(kind, body_1, body_2);
    put3(g.p, point_1), put3(g.p + 3, point_2);
    g.p[6] = s.stiffness, g.p[7] = s.damping, g.p[8] = s.rest_length, g.p[9] = s.slack_length;
    return g;
}
}  // namespace detail
struct DynamicDynamicSpringForceProperties {  // spring_force.rs:83-102 (the two entities are the two body indices of record())
    float attachment_point_1[3], attachment_point_2[3];  // each in its body's frame
    Spring spring;
    ivx_force_generator record(uint32_t dynamic_body_1, uint32_t dynamic_body_2) const {
        return detail::spring_generator(IVX_FG_SPRING_DYNAMIC_DYNAMIC, dynamic_body_1, dynamic_body_2, attachment_point_1, attachment_point_2, spring);
    }
};
struct DynamicKinematicSpringForceProperties {  // spring_force.rs:104-123; the second body is kinematic (its index WITHOUT IVX_KINEMATIC_BODY)
    float attachment_point_1[3], attachment_point_2[3];
    Spring spring;
    ivx_force_generator record(uint32_t dynamic_body_1, uint32_t kinematic_body_2) const {
        return detail::spring_generator(IVX_FG_SPRING_DYNAMIC_KINEMATIC, dynamic_body_1, kinematic_body_2, attachment_point_1, attachment_point_2, spring);
    }
};
struct FixedDirectionAlignmentTorque {  // alignment_torque.rs:64-84
    float axis_to_align[3];        // body frame, unit
    float alignment_direction[3];  // world, unit
    float settling_time, spin_damping, precession_damping;
    ivx_force_generator record(uint32_t body) const {
        ivx_force_generator g = detail::force_generator(IVX_FG_ALIGNMENT_FIXED, body, 0);
        detail::put3(g.p, axis_to_align), detail::put3(g.p + 3, alignment_direction);
        g.p[6] = settling_time, g.p[7] = spin_damping, g.p[8] = precession_damping;
        return g;
    }
};
struct GravityAlignmentTorque {  // alignment_torque.rs:86-105: towards the gravitational force on the body (it must be in the gravity field)
    float axis_to_align[3];
    float settling_time, spin_damping, precession_damping;
    ivx_force_generator record(uint32_t body) const {
        ivx_force_generator g = detail::force_generator(IVX_FG_ALIGNMENT_GRAVITY, body, 0);
        detail::put3(g.p, axis_to_align);
        g.p[6] = settling_time, g.p[7] = spin_damping, g.p[8] = precession_damping;
        return g;
    }
};
struct DynamicGravityConfig {  // dynamic_gravity.rs:36-46, 170-176
    float gravitational_constant = 1.0f;
};
static_assert(sizeof(ivx_force_generator) == 64 && sizeof(Spring) == 16 && sizeof(LocalForce) == 24 && sizeof(FixedDirectionAlignmentTorque) == 36 &&
                  sizeof(GravityAlignmentTorque) == 24,
              "force generator layouts");

// ---- detailed drag inside the force stage: the medium and the generator (medium.rs:11-68, detailed_drag.rs:44-57) -------------------------------
struct UniformMedium {
    float mass_density;
    float velocity[3];
    static constexpr float SEA_LEVEL_AIR_MASS_DENSITY = 1.2f;
    static constexpr float WATER_MASS_DENSITY = 1e3f;
    static UniformMedium vacuum() { return UniformMedium{0.0f, {0.0f, 0.0f, 0.0f}}; }
    static UniformMedium moving_air(const float v[3]) { return UniformMedium{SEA_LEVEL_AIR_MASS_DENSITY, {v[0], v[1], v[2]}}; }
    static UniformMedium still_air() { return UniformMedium{SEA_LEVEL_AIR_MASS_DENSITY, {0.0f, 0.0f, 0.0f}}; }
    static UniformMedium moving_water(const float v[3]) { return UniformMedium{WATER_MASS_DENSITY, {v[0], v[1], v[2]}}; }
    static UniformMedium still_water() { return UniformMedium{WATER_MASS_DENSITY, {0.0f, 0.0f, 0.0f}}; }
    ivx_uniform_medium record() const { return ivx_uniform_medium{mass_density, {velocity[0], velocity[1], velocity[2]}}; }
};
struct DetailedDragForce {  // the map is a slot of the world's table (the reference's DragLoadMapID -> slot is the caller's mapping)
    uint32_t drag_load_map;
    float drag_coefficient;
    float scaling = 1.0f;
    ivx_drag_generator record(uint32_t body) const { return ivx_drag_generator{body, drag_load_map, drag_coefficient, scaling}; }
};
static_assert(sizeof(UniformMedium) == 16 && sizeof(ivx_uniform_medium) == 16 && sizeof(ivx_drag_generator) == 16 && sizeof(ivx_drag_map_view) == 16, "detailed drag layouts");

// ---- rigid bodies + constraint solver (impact_physics/src/lib.rs:31-110) --------------------------------------------------------------
class PhysicsWorld {
public:
    PhysicsWorld(Context& ctx, const ivx_solver_config& config) { check(ivx_world_create(ctx.handle(), &config, &w_)); }
    ~PhysicsWorld() {
        if (w_) ivx_world_destroy(w_);
    }
    PhysicsWorld(const PhysicsWorld&) = delete;
    PhysicsWorld& operator=(const PhysicsWorld&) = delete;
    void set_bodies(const std::vector<ivx_rigid_body>& dynamic, const std::vector<ivx_kinematic_body>& kinematic = {}) {
        n_dyn_ = dynamic.size(), n_kin_ = kinematic.size();
        check(ivx_world_set_bodies(w_, dynamic.data(), dynamic.size(), kinematic.data(), kinematic.size()));
    }
    ivx_physics_result perform_physics_step(const std::vector<ivx_contact>& contacts, float step_duration) {
        size_t prepared = 0;
        check(ivx_world_set_contacts(w_, contacts.data(), contacts.size(), &prepared));
        ivx_physics_result r{};
        check(ivx_world_step(w_, step_duration, &r));
        return r;
    }
    std::vector<ivx_rigid_body> dynamic_bodies() {
        std::vector<ivx_rigid_body> d(n_dyn_);
        check(ivx_world_get_bodies(w_, d.data(), nullptr));
        return d;
    }
    std::vector<ivx_kinematic_body> kinematic_bodies() {
        std::vector<ivx_kinematic_body> k(n_kin_);
        check(ivx_world_get_bodies(w_, nullptr, k.data()));
        return k;
    }
    // MotionDriverManager: the set replaces the one before (empty: none); with a set every step ends by applying it at the new simulation time
    void set_motion_drivers(const std::vector<ivx_motion_driver>& drivers) { check(ivx_world_set_motion_drivers(w_, drivers.data(), drivers.size())); }
    void apply_motion(float simulation_time) { check(ivx_world_apply_motion(w_, simulation_time)); }
    void set_simulation_time(float t) { check(ivx_world_set_time(w_, t)); }
    float simulation_time() {
        float t = 0.0f;
        check(ivx_world_time(w_, &t));
        return t;
    }
    // ForceGeneratorManager: each set replaces the one before (empty: none); with either installed every step ends with the force stage, which
    // resets the totals of all dynamic bodies first (apply_forces primes them before the first step)
    void set_force_generators(const std::vector<ivx_force_generator>& generators) { check(ivx_world_set_force_generators(w_, generators.data(), generators.size())); }
    void set_dynamic_gravity(const std::vector<uint32_t>& dynamic_bodies, const DynamicGravityConfig& config = {}) {
        n_gravity_ = dynamic_bodies.size();
        check(ivx_world_set_dynamic_gravity(w_, dynamic_bodies.data(), dynamic_bodies.size(), config.gravitational_constant));
    }
    void apply_forces() { check(ivx_world_apply_forces(w_)); }
    std::vector<float> gravity_loads() {  // force and torque, 6 floats per field member in field order
        std::vector<float> loads(6 * n_gravity_);
        check(ivx_world_gravity_loads(w_, loads.data(), n_gravity_));
        return loads;
    }

    // detailed drag: the medium and the maps belong to the world; the generators are a third set of the force stage
    void set_medium(const UniformMedium& medium) {
        const ivx_uniform_medium m = medium.record();
        check(ivx_world_set_medium(w_, &m));
    }
    UniformMedium medium() {
        ivx_uniform_medium m{};
        check(ivx_world_medium(w_, &m));
        return UniformMedium{m.mass_density, {m.velocity[0], m.velocity[1], m.velocity[2]}};
    }
    void set_drag_map(uint32_t slot, const std::vector<ivx_drag_load>& map, uint32_t n_theta) { check(ivx_world_set_drag_map(w_, slot, map.data(), n_theta)); }
    void free_drag_map(uint32_t slot) { check(ivx_world_set_drag_map(w_, slot, nullptr, 0)); }
    void set_drag_map_from_grid(uint32_t slot, ivx_grid* grid, const float center_of_mass[3], const ivx_drag_map_config& config) {
        check(ivx_world_set_drag_map_from_grid(w_, slot, grid, center_of_mass, &config));
    }
    std::vector<ivx_drag_load> drag_map(uint32_t slot, uint32_t* n_theta) {
        check(ivx_world_drag_map_download(w_, slot, nullptr, 0, n_theta));
        std::vector<ivx_drag_load> map(2u * size_t(*n_theta) * *n_theta);
        if (!map.empty()) check(ivx_world_drag_map_download(w_, slot, map.data(), map.size(), n_theta));
        return map;
    }
    void set_detailed_drag(const std::vector<ivx_drag_generator>& generators) { check(ivx_world_set_detailed_drag(w_, generators.data(), generators.size())); }

    // the collision world's broad phase: IVX_CW_BROAD_FLAT (the default) or IVX_CW_BROAD_HIERARCHY — where ivx_cw_collide takes its pairs from
    void set_broad_phase(uint32_t which) { check(ivx_cw_set_broad_phase(w_, which)); }

private:
    ivx_world* w_ = nullptr;
    size_t n_dyn_ = 0, n_kin_ = 0, n_gravity_ = 0;
};

}  // namespace impact_voxel
