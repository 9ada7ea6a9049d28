// SDF queries on the device: the value and gradient of a compiled atomic SDF program at arbitrary points, and the three placements of the
// reference's meta-SDF graph that sample it — the closest point on the surface (Newton steps), the sphere cast along a ray, the rotation onto
// the gradient. sdf_query_eval.hpp holds the arithmetic; the host exports (ctx == NULL) and the kernels run the same functions.
//
// k_sq<OP>, one-wave workgroups. EIGHT LANES TO AN INSTANCE: lane c of the eight evaluates corner c of the 2x2x2 sample block, the eight values go
//   round the group by lane exchange and every lane of the group forms the sums, the gradient and the step from them in the one fixed order — the
//   eight lanes hold the same state throughout, so a group's control flow is uniform within the group, and the 1x1x1 sample of the cast is computed
//   by all eight alike. Batches are hundreds to thousands of instances and a cast is up to 128 dependent steps of nine program evaluations: the
//   kernel is bound by latency and by the instances in flight, and eight lanes per instance put eight times as many waves in flight as one lane
//   looping over the corners would. (OP_VALUES, one 1x1x1 sample per point, has nothing to share: a lane per point.)
//   The value stack is a column per lane in LDS, [level][lane], 256 bytes per level: no runtime-indexed private array, no scratch. The node list
//   is read at wave-uniform indices (the node loop's trip count is the program's), so its loads are scalar. A group whose instance is finished
//   sits masked out until the last group of its wave is done; nothing is compacted. Lane 0 of a group writes the instance's 32-byte record with
//   two plain 16-byte stores; no atomics: two calls leave the same bytes.
#include <new>
#include <vector>

#include "device_common.hpp"
#include "sdf_query_eval.hpp"

namespace {

using namespace ivx_sq;

constexpr uint32_t WAVE = 64;  // lanes of a workgroup (one wave)
enum { OP_VALUES = 0, OP_GRADIENTS = 1, OP_CLOSEST = 2, OP_CAST = 3, OP_ROTATION = 4 };

struct SqParams {
    ivx_similarity surface;
    float domain[6];
    float direction[3];
    uint32_t max_count;  // closest: max_iterations; cast: max_steps
    float f0, f1;        // closest: max_distance; cast: tolerance, safety_factor
};

template <int OP>
__global__ __launch_bounds__(WAVE) void k_sq(Program pr, SqParams prm, const void* __restrict__ in, uint32_t n, void* __restrict__ out) {
    extern __shared__ float sq_stack[];  // [max(stack_size, 1)][WAVE]
    const uint32_t lane = threadIdx.x;
    constexpr uint32_t PER = OP == OP_VALUES ? 1u : 8u;
    const uint32_t slot = (blockIdx.x * WAVE + lane) / PER;
    const bool live = slot < n;
    const uint32_t item = live ? slot : n - 1u;  // (n > 0; a group past the end repeats the last instance and writes nothing)
    Sampler s;
    s.pr = pr, s.st = sq_stack + lane, s.stride = WAVE, s.corner = lane & 7u;
    if constexpr (OP == OP_VALUES) {
        const float* p = static_cast<const float*>(in) + (size_t)item * 3u;
        const float v = s.value(mk(p[0], p[1], p[2]));
        if (live) static_cast<float*>(out)[item] = v;
    } else if constexpr (OP == OP_GRADIENTS) {
        const float* p = static_cast<const float*>(in) + (size_t)item * 3u;
        float v;
        V3 g;
        s.gradient(mk(p[0], p[1], p[2]), &v, &g);
        if (live && s.corner == 0u) static_cast<float4*>(out)[item] = make_float4(v, g.x, g.y, g.z);
    } else {
        const ivx_sdf_query_instance inst = static_cast<const ivx_sdf_query_instance*>(in)[item];
        ivx_sdf_query_result r;
        if constexpr (OP == OP_CLOSEST) closest(s, prm.surface, inst, prm.max_count, prm.f0, &r);
        else if constexpr (OP == OP_CAST) spherecast(s, prm.domain, prm.surface, inst, mk(prm.direction[0], prm.direction[1], prm.direction[2]), prm.max_count, prm.f0, prm.f1, &r);
        else rotation(s, prm.surface, inst, &r);
        if (live && s.corner == 0u) {
            uint4* o = static_cast<uint4*>(out) + (size_t)item * 2u;
            o[0] = make_uint4(r.status, r.steps, __float_as_uint(r.v[0]), __float_as_uint(r.v[1]));
            o[1] = make_uint4(__float_as_uint(r.v[2]), __float_as_uint(r.v[3]), r.exit, r.reserved);
        }
    }
}

}  // namespace

struct ivx_sdf_query {
    ivx_ctx* ctx = nullptr;
    std::vector<ivx_sdf_processed_node> nodes;
    uint32_t stack_size = 0;
    float domain[6] = {0, 0, 0, 0, 0, 0};
    ivx_buf d_nodes, d_io;  // the resident program | a call's input and output
    ivx_staging staging;    // the pinned block a call's one upload and one download go through
};

namespace {

Program host_program(const ivx_sdf_query* q) { return {q->nodes.data(), (uint32_t)q->nodes.size(), q->stack_size}; }

// One call on the device: `in_bytes` from the pinned block up, the kernel, `out_bytes` back into the pinned block, the wait, the copy out.
template <int OP>
int run_device(ivx_sdf_query* q, const SqParams& prm, const void* in, size_t in_bytes, uint32_t n, void* out, size_t out_bytes) {
    ivx_ctx* c = q->ctx;
    ivx_many_other_context other_(c);
    ivx_layout l;
    const size_t o_in = l.take(in_bytes), o_out = l.take(out_bytes);
    if (int rc = ivx_buf_grow(c, &q->d_io, l.bytes, 1u << 16)) return rc;
    if (int rc = ivx_staging_for(&q->staging, l.bytes)) return rc;
    char* hs = static_cast<char*>(q->staging.p);
    char* ds = static_cast<char*>(q->d_io.p);
    memcpy(hs + o_in, in, in_bytes);
    IVX_HIP_CHECK(ivx_memcpy_async(ds + o_in, hs + o_in, in_bytes, hipMemcpyHostToDevice, c->stream));
    const Program pr{static_cast<const ivx_sdf_processed_node*>(q->d_nodes.p), (uint32_t)q->nodes.size(), q->stack_size};
    const uint32_t levels = q->stack_size ? q->stack_size : 1u;
    const uint32_t per = OP == OP_VALUES ? 1u : 8u;
    const uint32_t blocks = (uint32_t)(((size_t)n * per + WAVE - 1u) / WAVE);
    IVX_KLAUNCH(k_sq<OP>, dim3(blocks), dim3(WAVE), (size_t)levels * WAVE * sizeof(float), c->stream, pr, prm, (const void*)(ds + o_in), n, (void*)(ds + o_out));
    IVX_HIP_CHECK(hipGetLastError());
    IVX_HIP_CHECK(ivx_memcpy_async(hs + o_out, ds + o_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    IVX_HIP_CHECK(ivx_stream_sync(c->stream));
    memcpy(out, hs + o_out, out_bytes);
    return IVX_OK;
}

int check_call(const ivx_sdf_query* q, const char* who, const void* a, const void* b, const void* c, size_t n) {
    IVX_REQUIRE(q, IVX_ERR_INVALID, "%s: null query object", who);
    IVX_REQUIRE(a && (n == 0 || (b && c)), IVX_ERR_INVALID, "%s: null argument", who);
    IVX_REQUIRE(n <= IVX_SDF_QUERY_MAX_ITEMS, IVX_ERR_CAPACITY, "%s: %zu items exceed %u", who, n, IVX_SDF_QUERY_MAX_ITEMS);
    return IVX_OK;
}

}  // namespace

extern "C" {

int ivx_sdf_query_create(ivx_ctx* ctx, const ivx_sdf_processed_node* nodes, size_t n_nodes, uint32_t stack_size, const float domain[6], ivx_sdf_query** out) {
    const char* who = "ivx_sdf_query_create";
    IVX_REQUIRE(out && domain && (nodes || n_nodes == 0), IVX_ERR_INVALID, "%s: null argument", who);
    *out = nullptr;
    IVX_REQUIRE(n_nodes < (1u << 30), IVX_ERR_CAPACITY, "%s: %zu nodes", who, n_nodes);
    IVX_REQUIRE(stack_size <= IVX_SDF_QUERY_MAX_STACK, IVX_ERR_CAPACITY, "%s: stack size %u exceeds IVX_SDF_QUERY_MAX_STACK (%u)", who, stack_size,
                IVX_SDF_QUERY_MAX_STACK);
    size_t depth = 0;
    for (size_t i = 0; i < n_nodes; ++i) {
        const uint32_t kind = nodes[i].kind;
        IVX_REQUIRE(kind <= 9u, IVX_ERR_INVALID, "%s: node %zu has kind %u (0 .. 9)", who, i, kind);
        if (kind <= 2u) {
            ++depth;
            IVX_REQUIRE(depth <= stack_size, IVX_ERR_INVALID, "%s: node %zu brings the stack to depth %zu, stack_size is %u", who, i, depth, stack_size);
        } else if (kind <= 6u) {
            IVX_REQUIRE(depth >= 1, IVX_ERR_INVALID, "%s: node %zu (kind %u) has no operand on the stack", who, i, kind);
        } else {
            IVX_REQUIRE(depth >= 2, IVX_ERR_INVALID, "%s: node %zu (kind %u) has %zu operands on the stack, needs 2", who, i, kind, depth);
            --depth;
        }
    }
    IVX_REQUIRE(n_nodes == 0 || depth == 1, IVX_ERR_INVALID, "%s: the list leaves %zu values on the stack, not 1", who, depth);
    ivx_sdf_query* q = new (std::nothrow) ivx_sdf_query();
    IVX_REQUIRE(q, IVX_ERR_CAPACITY, "%s: out of host memory", who);
    q->ctx = ctx;
    q->nodes.assign(nodes, nodes + n_nodes);
    q->stack_size = stack_size;
    for (int k = 0; k < 6; ++k) q->domain[k] = domain[k];
    if (ctx && n_nodes) {
        ivx_many_other_context other_(ctx);
        int rc = ivx_buf_grow(ctx, &q->d_nodes, n_nodes * sizeof(ivx_sdf_processed_node), 0);
        if (rc == IVX_OK && ivx_memcpy_sync(q->d_nodes.p, nodes, n_nodes * sizeof(ivx_sdf_processed_node), hipMemcpyHostToDevice) != hipSuccess) {
            ivx_set_error("%s: the upload of the program failed", who);
            rc = IVX_ERR_HIP;
        }
        if (rc != IVX_OK) {
            ivx_buf_free(&q->d_nodes);
            delete q;
            return rc;
        }
    }
    *out = q;
    return IVX_OK;
}

void ivx_sdf_query_destroy(ivx_sdf_query* q) {
    if (!q) return;
    if (q->ctx) {
        ivx_many_other_context other_(q->ctx);
        (void)ivx_stream_sync(q->ctx->stream);
        ivx_buf_free(&q->d_nodes);
        ivx_buf_free(&q->d_io);
        ivx_staging_release(&q->staging);
    }
    delete q;
}

int ivx_sdf_query_points(ivx_sdf_query* q, int which, const float* points, size_t n, float* out) {
    const char* who = "ivx_sdf_query_points";
    if (int rc = check_call(q, who, q, points, out, n)) return rc;
    IVX_REQUIRE(which == 0 || which == 1, IVX_ERR_INVALID, "%s: which must be 0 (distance) or 1 (distance and gradient)", who);
    if (n == 0) return IVX_OK;
    if (q->ctx) {
        const SqParams prm{};
        if (which == 0) return run_device<OP_VALUES>(q, prm, points, n * 12, (uint32_t)n, out, n * 4);
        return run_device<OP_GRADIENTS>(q, prm, points, n * 12, (uint32_t)n, out, n * 16);
    }
    float st[IVX_SDF_QUERY_MAX_STACK];
    const Sampler s{host_program(q), st, 1u, 0u};
    for (size_t i = 0; i < n; ++i) {
        const V3 p = ld3(points + i * 3);
        if (which == 0) {
            out[i] = s.value(p);
        } else {
            V3 g;
            s.gradient(p, &out[i * 4], &g);
            st3(&out[i * 4 + 1], g);
        }
    }
    return IVX_OK;
}

int ivx_sdf_query_closest(ivx_sdf_query* q, const ivx_similarity* surface_to_parent, const ivx_sdf_query_instance* instances, size_t n, uint32_t max_iterations,
                          float max_distance, ivx_sdf_query_result* results) {
    const char* who = "ivx_sdf_query_closest";
    if (int rc = check_call(q, who, surface_to_parent, instances, results, n)) return rc;
    if (n == 0) return IVX_OK;
    if (q->ctx) {
        SqParams prm{};
        prm.surface = *surface_to_parent, prm.max_count = max_iterations, prm.f0 = max_distance;
        return run_device<OP_CLOSEST>(q, prm, instances, n * sizeof(ivx_sdf_query_instance), (uint32_t)n, results, n * sizeof(ivx_sdf_query_result));
    }
    float st[IVX_SDF_QUERY_MAX_STACK];
    const Sampler s{host_program(q), st, 1u, 0u};
    for (size_t i = 0; i < n; ++i) closest(s, *surface_to_parent, instances[i], max_iterations, max_distance, &results[i]);
    return IVX_OK;
}

int ivx_sdf_query_spherecast(ivx_sdf_query* q, const ivx_similarity* surface_to_parent, const ivx_sdf_query_instance* instances, size_t n,
                             const float direction[3], uint32_t max_steps, float tolerance, float safety_factor, ivx_sdf_query_result* results) {
    const char* who = "ivx_sdf_query_spherecast";
    if (int rc = check_call(q, who, surface_to_parent, instances, results, n)) return rc;
    IVX_REQUIRE(direction, IVX_ERR_INVALID, "%s: null direction", who);
    IVX_REQUIRE(safety_factor > 0.0f && safety_factor <= 1.0f, IVX_ERR_INVALID, "%s: safety_factor %g is not in (0, 1]", who, (double)safety_factor);
    if (n == 0) return IVX_OK;
    if (q->ctx) {
        SqParams prm{};
        prm.surface = *surface_to_parent, prm.max_count = max_steps, prm.f0 = tolerance, prm.f1 = safety_factor;
        for (int k = 0; k < 3; ++k) prm.direction[k] = direction[k];
        for (int k = 0; k < 6; ++k) prm.domain[k] = q->domain[k];
        return run_device<OP_CAST>(q, prm, instances, n * sizeof(ivx_sdf_query_instance), (uint32_t)n, results, n * sizeof(ivx_sdf_query_result));
    }
    float st[IVX_SDF_QUERY_MAX_STACK];
    const Sampler s{host_program(q), st, 1u, 0u};
    for (size_t i = 0; i < n; ++i) spherecast(s, q->domain, *surface_to_parent, instances[i], ld3(direction), max_steps, tolerance, safety_factor, &results[i]);
    return IVX_OK;
}

int ivx_sdf_query_rotation(ivx_sdf_query* q, const ivx_similarity* surface_to_parent, const ivx_sdf_query_instance* instances, size_t n,
                           ivx_sdf_query_result* results) {
    const char* who = "ivx_sdf_query_rotation";
    if (int rc = check_call(q, who, surface_to_parent, instances, results, n)) return rc;
    if (n == 0) return IVX_OK;
    if (q->ctx) {
        SqParams prm{};
        prm.surface = *surface_to_parent;
        return run_device<OP_ROTATION>(q, prm, instances, n * sizeof(ivx_sdf_query_instance), (uint32_t)n, results, n * sizeof(ivx_sdf_query_result));
    }
    float st[IVX_SDF_QUERY_MAX_STACK];
    const Sampler s{host_program(q), st, 1u, 0u};
    for (size_t i = 0; i < n; ++i) rotation(s, *surface_to_parent, instances[i], &results[i]);
    return IVX_OK;
}

}  // extern "C"
