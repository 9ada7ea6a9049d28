// C ABI of the rigid-body / contact-solver part (include/impact_voxel_hip.h, "a15-a19"): the world's device arrays, its two pinned upload
// blocks, and the entry points. What is inherently sequential and tiny per item in the reference — interlock analysis, the ConstraintCache
// order, the dependency schedule of the sweeps — is host-only code in contact_schedule.hpp (w->sched) and runs once per contact set;
// ivx_world_set_contacts here is the sequence of its stages with the uploads behind them. All arithmetic on body state runs in the kernels
// of physics.hip.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstring>
#include <new>

#include "physics_internal.hpp"

namespace {

// ONE table of the world's device arrays: which group an array belongs to, how large an element is, how many it needs now, and the host
// vector it is uploaded from (if any). ivx_world_ensure_form grows and uploads the arrays of a form from it, ivx_world_set_contacts the
// kinematic group, ivx_world_set_bodies walks the body group, contact_arrays_grow_keep the contact group, ivx_world_destroy frees them all.
enum WorldGroup : uint32_t {
    G_BODY,         // one capacity in bodies for all five; elem: bytes per body
    G_CONTACT,      // one capacity in contacts; elem: bytes per contact; keep: the previous state survives growth
    G_ITEMS,        // form 1, uploaded when there are items
    G_LEVELS,       // form 1, uploaded always
    G_STATIONARY,   // form 2, uploaded when there are slots
    G_CS_SLOT_OF,   // form 2, grown and uploaded only with kinematic items in the positional phase
    G_KIN_LISTS,    // grown with kinematic items, uploaded when the schedule changed
    G_KIN_SCRATCH,  // grown with kinematic items, device-only
    G_FIXED,        // allocated to size elsewhere; here to be freed
};
struct WorldArray {
    void** p;
    size_t* cap;  // in units of sizeof(T); null: G_FIXED
    size_t unit, elem;
    WorldGroup group;
    size_t need;       // elements
    const void* host;  // `need` elements, or null
    bool keep;
    size_t upload_bytes() const { return host ? need * elem : 0; }
};
template <class T>
WorldArray row(ivx_dev_array<T>& a, WorldGroup g, size_t need = 0, size_t elem = sizeof(T), bool keep = false) {
    return {reinterpret_cast<void**>(&a.p), &a.cap, sizeof(T), elem, g, need, nullptr, keep};
}
template <class T, class H>
WorldArray row(ivx_dev_array<T>& a, WorldGroup g, const std::vector<H>& host) {
    static_assert(sizeof(T) == sizeof(H), "a world array and its host vector have one element type");
    return {reinterpret_cast<void**>(&a.p), &a.cap, sizeof(T), sizeof(T), g, host.size(), host.data(), false};
}
template <class T>
WorldArray fixed(T*& p) {
    return {reinterpret_cast<void**>(&p), nullptr, sizeof(T), sizeof(T), G_FIXED, 0, nullptr, false};
}
std::array<WorldArray, 33> world_arrays(ivx_world* w) {
    ivx_contact_schedule& h = w->sched;
    const size_t n_pos_items = h.phase_items[1];
    return {{
        row(w->dyn, G_BODY), row(w->kin, G_BODY), row(w->cb, G_BODY), row(w->touched, G_BODY), row(w->dynst, G_BODY, 0, 2 * 64),
        row(w->contacts, G_CONTACT), row(w->prev_slot, G_CONTACT), row(w->pc[0], G_CONTACT, 0, sizeof(PhysContact), true),
        row(w->acc[0], G_CONTACT, 0, 4 * sizeof(float), true), row(w->pc[1], G_CONTACT, 0, sizeof(PhysContact), true),
        row(w->acc[1], G_CONTACT, 0, 4 * sizeof(float), true),
        row(w->items, G_ITEMS, h.items_host), row(w->item_bodies, G_ITEMS, h.item_bodies_host), row(w->item_tags, G_ITEMS, h.item_tags_host),
        row(w->level_start, G_LEVELS, h.level_start_host), row(w->tile_base, G_LEVELS, h.tile_base_host), row(w->tile_first, G_LEVELS, h.tile_first_host),
        row(w->cs_item, G_STATIONARY, h.cs_item_host), row(w->cs_bodies, G_STATIONARY, h.cs_bodies_host), row(w->cs_vers, G_STATIONARY, h.cs_vers_host),
        row(w->cs_round_start, G_STATIONARY, h.cs_round_start_host), row(w->cs_round_mask, G_STATIONARY, h.cs_round_mask_host),
        row(w->cs_round_level, G_STATIONARY, h.cs_round_level_host), row(w->cs_slot_of, G_CS_SLOT_OF, h.cs_slot_of_host),
        row(w->kin_offsets, G_KIN_LISTS, h.kin_offsets_host), row(w->kin_list, G_KIN_LISTS, h.kin_list_host),
        row(w->kin_applied, G_KIN_SCRATCH, n_pos_items), row(w->kin_qstart, G_KIN_SCRATCH, 8 * n_pos_items),  // float4 per (item, side)
        row(w->kin_snap, G_KIN_SCRATCH, (size_t)std::max<uint32_t>(w->n_dyn, 1u) * 8),
        fixed(w->barrier_words), fixed(w->joint_refs), fixed(w->packed[0]), fixed(w->packed[1]),
    }};
}
void world_array_free(const WorldArray& a) {
    if (*a.p) (void)hipFree(*a.p);
    *a.p = nullptr;
    if (a.cap) *a.cap = 0;
}

// The contact group holds at least nc contacts afterwards: max(nc, twice what it held, 256). The previous state (pc / acc of the last solve,
// n_prev contacts) survives the growth.
int contact_arrays_grow_keep(ivx_world* w, uint32_t nc) {
    if (nc <= w->acc[1].cap / 4) return IVX_OK;  // (the last of the group to grow)
    const size_t ncap = std::max<size_t>(nc, std::max<size_t>(w->acc[1].cap / 4 * 2, 256));
    IVX_HIP_CHECK(ivx_stream_sync(w->ctx->stream));
    for (const WorldArray& a : world_arrays(w)) {
        if (a.group != G_CONTACT || *a.cap * a.unit >= ncap * a.elem) continue;
        void* grown = nullptr;
        IVX_HIP_CHECK(hipMalloc(&grown, ncap * a.elem));
        if (a.keep && *a.p && w->n_prev) {
            const hipError_t e = ivx_memcpy_sync(grown, *a.p, w->n_prev * a.elem, hipMemcpyDeviceToDevice);
            if (e != hipSuccess) (void)hipFree(grown);
            IVX_HIP_CHECK(e);
        }
        world_array_free(a);
        *a.p = grown;
        *a.cap = ncap * a.elem / a.unit;
    }
    return IVX_OK;
}

void joint_refs_drop(ivx_world* w) {
    if (w->joint_refs) (void)hipFree(w->joint_refs);
    w->joint_refs = nullptr;
    w->n_joint_refs = 0;
    w->joint_refs_host.clear();
}

int fetch_body_position(ivx_world* w, uint32_t ref, float out[3]) {
    IVX_HIP_CHECK(ivx_stream_sync(w->ctx->stream));
    const void* src = (ref & IVX_KINEMATIC_BODY) ? static_cast<const void*>(w->kin.p[ref & 0x7FFFFFFFu].position) : static_cast<const void*>(w->dyn.p[ref].position);
    IVX_HIP_CHECK(ivx_memcpy_sync(out, src, 12, hipMemcpyDeviceToHost));
    return IVX_OK;
}

// device part of prepare_constraints: gather bodies, prepare every contact (null: every contact's previous slot is its own), warm-start
// bookkeeping, into the other half of the double-buffered state
int world_prepare_launches(ivx_world* w, const int32_t* d_prev_slot) {
    int rc;
    w->cur ^= 1;
    if ((rc = ivx_launch_phys_prepare_bodies(w))) return rc;
    if ((rc = ivx_launch_phys_prepare_contacts(w, d_prev_slot))) return rc;
    if ((rc = ivx_launch_phys_mark_joint_bodies(w))) return rc;
    w->prepared_fresh = 1;
    return IVX_OK;
}

}  // namespace

// The multi-workgroup solve's grid barrier is hand-rolled and bounded: a workgroup that never sees the others arrive gives up, sets this word
// and the phase goes on unsynchronised — the bodies of that step are wrong. Every entry point that waits on the world's stream looks at the
// word afterwards (it is host-mapped: no copy), reports the step as failed, clears the word, and keeps the world on the single-workgroup
// kernel from then on.
static int ivx_world_check_solve(ivx_world* w, const char* who) {
    if (!w->mg_err_host || w->mg_err_host[0] == 0u) return IVX_OK;
    w->mg_err_host[0] = 0u;
    w->mg_disabled = 1;
    ivx_set_error("%s: the solver's grid barrier timed out in an earlier step of this world (a workgroup of the solve was not resident): that step's "
                  "bodies are invalid; the world now solves on one workgroup", who);
    return IVX_ERR_HIP;
}

// Host arrays on their way to the device, all through ONE pinned staging block of the world (stage_sched) and asynchronous copies on its
// stream (the block is free again when the event behind the last copy has passed).
struct StagedUploads {
    ivx_world* w;
    struct Item {
        void* dst;
        const void* src;
        size_t bytes, off;
    };
    std::vector<Item> items;
    size_t total = 0;
    explicit StagedUploads(ivx_world* world) : w(world) {}
    void add(void* dst, const void* src, size_t bytes) {
        if (!bytes) return;
        items.push_back(Item{dst, src, bytes, total});
        total += (bytes + 63) & ~(size_t)63;
    }
    void add(const WorldArray& a) { add(*a.p, a.host, a.upload_bytes()); }
    int flush() {
        if (items.empty()) return IVX_OK;
        hipStream_t s = w->ctx->stream;
        ivx_staging* st = &w->stage_sched;
        if (int rc = ivx_staging_for(st, total)) return rc;
        char* block = static_cast<char*>(st->p);
        for (const Item& it : items) memcpy(block + it.off, it.src, it.bytes);
        for (const Item& it : items) IVX_HIP_CHECK(ivx_memcpy_async(it.dst, block + it.off, it.bytes, hipMemcpyHostToDevice, s));
        if (int rc = ivx_staging_sent(st, s)) return rc;
        items.clear();
        total = 0;
        return IVX_OK;
    }
};

// The schedule form the solve is about to use — 1: the level-ordered item list, tags and tiles (k_solve, k_solve_mg), 2: the chain-stationary
// tiles and rounds (k_solve_cs) — built from the levels and uploaded if this contact structure has not had it yet.
int ivx_world_ensure_form(ivx_world* w, uint32_t form) {
    ivx_contact_schedule& h = w->sched;
    if (h.forms_built & form) return IVX_OK;
    hipStream_t s = w->ctx->stream;
    h.build_form(form, w->cfg.n_iterations, w->cfg.n_positional_correction_iterations, w->n_dyn);
    const auto arrays = world_arrays(w);
    auto of_form = [&](const WorldArray& a) {
        if (form == 1u) return a.group == G_ITEMS || a.group == G_LEVELS;
        return a.group == G_STATIONARY || (a.group == G_CS_SLOT_OF && h.n_kin_items != 0);
    };
    for (const WorldArray& a : arrays)
        if (of_form(a))
            if (int rc = ivx_dev_grow(a.p, a.cap, a.unit, a.need, s)) return rc;
    StagedUploads up(w);
    for (const WorldArray& a : arrays) {
        if (!of_form(a)) continue;
        if (a.group == G_ITEMS && h.items_host.empty()) continue;
        if (a.group == G_STATIONARY && h.cs_item_host.empty()) continue;
        up.add(a);
    }
    if (int rc = up.flush()) return rc;
    h.forms_built |= form;
    return IVX_OK;
}

extern "C" {

int ivx_world_create(ivx_ctx* c, const ivx_solver_config* cfg, ivx_world** out) {
    IVX_REQUIRE(c && out, IVX_ERR_INVALID, "ivx_world_create: null argument");
    *out = nullptr;
    ivx_world* w = new (std::nothrow) ivx_world();
    IVX_REQUIRE(w, IVX_ERR_CAPACITY, "ivx_world_create: out of host memory");
    w->ctx = c;
    if (cfg) w->cfg = *cfg;
    else w->cfg = ivx_solver_config{8u, 0.4f, 3u, 0.2f};  // ConstraintSolverConfig::default (solver.rs:374-384)
    IVX_REQUIRE(w->cfg.n_iterations + w->cfg.n_positional_correction_iterations < 4096, IVX_ERR_INVALID, "ivx_world_create: too many iterations");
    if (hipMalloc(reinterpret_cast<void**>(&w->barrier_words), 128 * sizeof(uint32_t)) != hipSuccess ||
        ivx_memset_async(w->barrier_words, 0, 128 * sizeof(uint32_t), c->stream) != hipSuccess) {
        ivx_set_error("ivx_world_create: device allocation failed");
        delete w;
        return IVX_ERR_HIP;
    }
    if (hipHostMalloc(reinterpret_cast<void**>(&w->mg_err_host), 64, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void**>(&w->mg_err_dev), w->mg_err_host, 0) != hipSuccess) {
        ivx_set_error("ivx_world_create: host-mapped allocation failed");
        if (w->mg_err_host) (void)hipHostFree(w->mg_err_host);
        (void)hipFree(w->barrier_words);
        delete w;
        return IVX_ERR_HIP;
    }
    w->mg_err_host[0] = 0u;
    w->mg_disabled = 0;
    *out = w;
    return IVX_OK;
}

void ivx_world_destroy(ivx_world* w) {
    if (!w) return;
    (void)ivx_stream_sync(w->ctx->stream);
    if (w->side_stream) {  // the positional phase's stream and its fork / join events (created on the first multi-workgroup solve)
        (void)ivx_stream_sync(w->side_stream);
        (void)hipEventDestroy(w->ev_fork);
        (void)hipEventDestroy(w->ev_join);
        (void)hipStreamDestroy(w->side_stream);
    }
    ivx_cw_release(w);
    ivx_md_release(w);
    ivx_fg_release(w);
    ivx_staging_release(&w->stage_sched);
    ivx_staging_release(&w->stage_contacts);
    for (const WorldArray& a : world_arrays(w)) world_array_free(a);
    if (w->mg_err_host) (void)hipHostFree(w->mg_err_host);
    if (w->ev_ready)
        for (int i = 0; i < 5; ++i) (void)hipEventDestroy(w->ev[i]);
    delete w;
}

// ConstraintManager::add_spherical_joint + the joints' share of prepare_constraints (constraint.rs:183-190, 252-255). The reference's
// PreparedSphericalJoint is a placeholder: `compute_impulses` returns 0, `apply_impulses_to_body_pair` and
// `apply_positional_correction_to_body_pair` are empty (constraint/spherical_joint.rs:62-88), so a joint adds no item to the sweeps.
// What it does do is make its two bodies constrained bodies of the step (`prepare_spherical_joint` -> `add_body_pair`): their velocities
// are synchronised before the solve and written back after it — momentum = mass x (momentum / mass) — like those of bodies in contact.
int ivx_world_set_spherical_joints(ivx_world* w, const uint32_t* body_pairs, size_t n_joints) {
    IVX_REQUIRE(w && (body_pairs || n_joints == 0), IVX_ERR_INVALID, "ivx_world_set_spherical_joints: null argument");
    IVX_REQUIRE(n_joints < (1u << 24), IVX_ERR_CAPACITY, "ivx_world_set_spherical_joints: too many joints");
    for (size_t i = 0; i < 2 * n_joints; ++i) {
        const uint32_t r = body_pairs[i];
        IVX_REQUIRE((r & 0x7FFFFFFFu) < ((r & IVX_KINEMATIC_BODY) ? w->n_kin : w->n_dyn), IVX_ERR_INVALID,
                    "ivx_world_set_spherical_joints: anchor %zu refers to a missing body", i);
    }
    IVX_HIP_CHECK(ivx_stream_sync(w->ctx->stream));
    joint_refs_drop(w);
    w->sched.n_bodies_valid = false;
    if (n_joints) {
        IVX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&w->joint_refs), 2 * n_joints * sizeof(uint32_t)));
        IVX_HIP_CHECK(ivx_memcpy_sync(w->joint_refs, body_pairs, 2 * n_joints * sizeof(uint32_t), hipMemcpyHostToDevice));
        w->n_joint_refs = (uint32_t)(2 * n_joints);
        w->joint_refs_host.assign(body_pairs, body_pairs + 2 * n_joints);
    }
    return IVX_OK;
}

int ivx_world_set_bodies(ivx_world* w, const ivx_rigid_body* dyn, size_t n_dyn, const ivx_kinematic_body* kin, size_t n_kin) {
    IVX_REQUIRE(w && (dyn || n_dyn == 0) && (kin || n_kin == 0), IVX_ERR_INVALID, "ivx_world_set_bodies: null argument");
    IVX_REQUIRE(n_dyn < IVX_KINEMATIC_BODY && n_kin < IVX_KINEMATIC_BODY, IVX_ERR_CAPACITY, "ivx_world_set_bodies: too many bodies");
    for (size_t i = 0; i < n_dyn; ++i) IVX_REQUIRE(dyn[i].mass > 0.0f, IVX_ERR_INVALID, "ivx_world_set_bodies: body %zu has non-positive mass", i);
    hipStream_t s = w->ctx->stream;
    IVX_HIP_CHECK(ivx_stream_sync(s));
    const size_t need = n_dyn + n_kin;
    if (need > w->body_cap) {
        const auto arrays = world_arrays(w);
        for (const WorldArray& a : arrays)
            if (a.group == G_BODY) world_array_free(a);
        w->body_cap = 0;
        const size_t cap = std::max<size_t>(need, 64);
        for (const WorldArray& a : arrays) {
            if (a.group != G_BODY) continue;
            IVX_HIP_CHECK(hipMalloc(a.p, cap * a.elem));
            *a.cap = cap * a.elem / a.unit;
        }
        w->body_cap = cap;
    }
    if (n_dyn) IVX_HIP_CHECK(ivx_memcpy_sync(w->dyn.p, dyn, n_dyn * sizeof(ivx_rigid_body), hipMemcpyHostToDevice));
    if (n_kin) IVX_HIP_CHECK(ivx_memcpy_sync(w->kin.p, kin, n_kin * sizeof(ivx_kinematic_body), hipMemcpyHostToDevice));
    const bool resized = w->n_dyn != n_dyn || w->n_kin != n_kin;
    // joints name bodies by index and were validated against the old counts: a set that shrank drops them (the caller sets them again)
    if ((n_dyn < w->n_dyn || n_kin < w->n_kin) && w->n_joint_refs) joint_refs_drop(w);
    w->n_dyn = (uint32_t)n_dyn;
    w->n_kin = (uint32_t)n_kin;
    w->sched.n_bodies_valid = false;
    if (resized) w->schedule_valid = 0;
    w->prepared_fresh = 0;
    return IVX_OK;
}

int ivx_world_get_bodies(ivx_world* w, ivx_rigid_body* dyn, ivx_kinematic_body* kin) {
    IVX_REQUIRE(w, IVX_ERR_INVALID, "ivx_world_get_bodies: null world");
    IVX_HIP_CHECK(ivx_stream_sync(w->ctx->stream));
    if (int rc = ivx_world_check_solve(w, "ivx_world_get_bodies")) return rc;
    if (dyn && w->n_dyn) IVX_HIP_CHECK(ivx_memcpy_sync(dyn, w->dyn.p, w->n_dyn * sizeof(ivx_rigid_body), hipMemcpyDeviceToHost));
    if (kin && w->n_kin) IVX_HIP_CHECK(ivx_memcpy_sync(kin, w->kin.p, w->n_kin * sizeof(ivx_kinematic_body), hipMemcpyDeviceToHost));
    return IVX_OK;
}

// 0. The usual frame: the contacts of the frame before with new geometry — the same ids in the same order on the same body pairs, no manifold
// interlocked. Then everything the general path would compute is what it computed last time: every id keeps its slot (warm start from the
// same slot: prev_slot = identity), the chains and the dependency schedule stand. One pass over the input decides that and copies it into
// the pinned block; the upload is an asynchronous copy and nothing here waits for the GPU (46 080 contacts: 0.1 ms instead of 0.45).
// *done: the frame was that; otherwise the general path goes on (and overwrites the block).
static int set_contacts_fast(ivx_world* w, const ivx_contact* contacts, size_t n, bool* done) {
    const ivx_contact_schedule& h = w->sched;
    const size_t bytes = n * sizeof(ivx_contact);
    *done = false;
    if (!(w->schedule_valid && n > 0 && n == w->n_contacts && n == h.cache.size() && 2 * n == h.slot_bodies.size() && w->stage_contacts.bytes >= bytes)) return IVX_OK;
    if (int rc = ivx_staging_for(&w->stage_contacts, bytes)) return rc;  // (large enough: this waits for the previous frame's copy out of the block)
    if (!h.same_as_resident(contacts, n, static_cast<ivx_contact*>(w->stage_contacts.p))) return IVX_OK;
    hipStream_t s = w->ctx->stream;
    w->n_prev = w->n_contacts;
    if (int rc = ivx_staging_upload(&w->stage_contacts, w->contacts.p, bytes, s)) return rc;
    *done = true;
    return world_prepare_launches(w, nullptr);
}

int ivx_world_set_contacts(ivx_world* w, const ivx_contact* contacts, size_t n, size_t* n_prepared) {
    IVX_REQUIRE(w && (contacts || n == 0), IVX_ERR_INVALID, "ivx_world_set_contacts: null argument");
    if (int rc = ivx_world_check_solve(w, "ivx_world_set_contacts")) return rc;  // (no wait here: a flag that is already up)
    IVX_REQUIRE(n < (1u << 24), IVX_ERR_CAPACITY, "ivx_world_set_contacts: more than 2^24 contacts");
    ivx_contact_schedule& h = w->sched;
    int rc;
    bool done;
    if ((rc = set_contacts_fast(w, contacts, n, &done)) || done) {
        if (!rc && n_prepared) *n_prepared = n;
        return rc;
    }
    ivx_world_lap lap(1);
    if (ivx_world_trace_level() >= 1)  // developer aid (IVX_WORLD_TRACE=1): a frame that leaves the one-pass path says why
        fprintf(stderr, "[ivx world] set_contacts: general path (schedule_valid %d, n %zu, resident %u, cache %zu, staging cap %zu)\n", w->schedule_valid, n, w->n_contacts,
                h.cache.size(), w->stage_contacts.bytes / sizeof(ivx_contact));
    // 1. one pass over the input: the body references, and is any manifold interlocked? Only then is a copy of the list made, with those
    // manifolds replaced by their separating contact (needs the bodies' positions from the device)
    const ivx_contact_schedule::Verdict v = ivx_contact_schedule::validate(contacts, n, w->n_dyn, w->n_kin);
    IVX_REQUIRE(v.kind != ivx_contact_schedule::CONTACT_MISSING_BODY, IVX_ERR_INVALID, "ivx_world_set_contacts: contact %zu refers to a missing body", v.index);
    IVX_REQUIRE(v.kind != ivx_contact_schedule::CONTACT_SELF_PAIR, IVX_ERR_INVALID, "ivx_world_set_contacts: contact %zu joins a body with itself", v.index);
    const ivx_contact* eff = contacts;
    size_t n_eff = n;
    if (v.any_interlocked) {
        if ((rc = h.replace_interlocked(contacts, n, [w](uint32_t ref, float* out) { return fetch_body_position(w, ref, out); }))) return rc;
        eff = h.effective.data();
        n_eff = h.effective.size();
    }
    lap("validate + interlock");
    // 2. the ConstraintCache: every id keeps its slot; the contacts in slot order go straight into the pinned block their upload is made from
    const uint32_t nc = h.register_contacts(eff, n_eff);
    if ((rc = ivx_staging_for(&w->stage_contacts, (size_t)nc * sizeof(ivx_contact)))) return rc;
    h.write_slot_order(eff, static_cast<ivx_contact*>(w->stage_contacts.p));
    w->n_prev = w->n_contacts;  // size of the state arrays written by the previous prepare
    w->n_contacts = nc;
    lap("constraint cache");
    // 3. chains and the levels of the two phases' items
    h.build_chains();
    IVX_REQUIRE((uint64_t)h.n_chains() * (std::max(w->cfg.n_iterations + 1u, w->cfg.n_positional_correction_iterations)) < (1ull << 26), IVX_ERR_CAPACITY,
                "ivx_world_set_contacts: more than 2^26 schedule items in one phase");
    const bool same_schedule = h.build_levels(w->schedule_valid != 0, w->cfg.n_iterations, w->cfg.n_positional_correction_iterations, w->n_dyn, w->n_kin);
    lap("chains + levels");
    // 4. buffers and uploads
    hipStream_t s = w->ctx->stream;
    if ((rc = contact_arrays_grow_keep(w, nc))) return rc;
    const auto arrays = world_arrays(w);
    if (h.n_kin_items)
        for (const WorldArray& a : arrays)
            if (a.group == G_KIN_LISTS || a.group == G_KIN_SCRATCH)
                if ((rc = ivx_dev_grow(a.p, a.cap, a.unit, a.need, s))) return rc;
    // (no wait here: the copies below are stream-ordered behind whatever still reads these buffers; a buffer that grew was waited for as it grew)
    if (nc && (rc = ivx_staging_upload(&w->stage_contacts, w->contacts.p, (size_t)nc * sizeof(ivx_contact), s))) return rc;
    StagedUploads up(w);
    if (nc) up.add(w->prev_slot.p, h.prev_slot_host.data(), nc * sizeof(int32_t));
    if (!same_schedule && h.n_kin_items)
        for (const WorldArray& a : arrays)
            if (a.group == G_KIN_LISTS) up.add(a);
    lap("buffers");
    if ((rc = up.flush())) return rc;
    lap("staged uploads");
    w->schedule_valid = 1;
    // 5. device part of prepare_constraints
    if ((rc = world_prepare_launches(w, w->prev_slot.p))) return rc;
    lap("prepare launches");
    if (n_prepared) *n_prepared = nc;
    return IVX_OK;
}

// prepare_constraints again over the resident contact set: same ids, same order (every id is "known from
// the previous solve"), warm impulses from the last solve
int ivx_world_prepare(ivx_world* w) {
    IVX_REQUIRE(w, IVX_ERR_INVALID, "ivx_world_prepare: null world");
    IVX_REQUIRE(w->schedule_valid || w->n_contacts == 0, IVX_ERR_STATE, "ivx_world_prepare: call ivx_world_set_contacts after changing the bodies");
    w->n_prev = w->n_contacts;
    return world_prepare_launches(w, nullptr);
}

int ivx_world_advance_momenta(ivx_world* w, float dt) {
    IVX_REQUIRE(w, IVX_ERR_INVALID, "ivx_world_advance_momenta: null world");
    return ivx_launch_phys_pre_solve(w, dt);
}

int ivx_world_solve(ivx_world* w) {
    IVX_REQUIRE(w, IVX_ERR_INVALID, "ivx_world_solve: null world");
    IVX_REQUIRE(w->prepared_fresh, IVX_ERR_STATE, "ivx_world_solve: no prepared constraints (ivx_world_set_contacts / ivx_world_prepare)");
    int rc;
    if ((rc = ivx_launch_phys_solve(w))) return rc;
    if ((rc = ivx_launch_phys_post_solve(w, 0.0f, 1, 0))) return rc;
    w->prepared_fresh = 0;
    return IVX_OK;
}

int ivx_world_advance_configurations(ivx_world* w, float dt) {
    IVX_REQUIRE(w, IVX_ERR_INVALID, "ivx_world_advance_configurations: null world");
    return ivx_launch_phys_post_solve(w, dt, 0, 1);
}

// `timed`: bracket the phases with event records for stage_ms. Only the synchronous ivx_world_step asks for them: an event record
// is a packet of its own on the queue (~2-3 us each), and a frame that enqueues this step between other work has no use for them.
static int world_step_enqueue(ivx_world* w, float dt, bool timed) {
    hipStream_t s = w->ctx->stream;
    if (timed && !w->ev_ready) {
        for (int i = 0; i < 5; ++i) IVX_HIP_CHECK(hipEventCreate(&w->ev[i]));
        w->ev_ready = 1;
    }
    auto stamp = [&](int i) -> int {
        if (timed) IVX_HIP_CHECK(ivx_event_record(w->ev[i], s));
        return IVX_OK;
    };
    int rc;
    if (w->n_contacts == 0 && !w->prepared_fresh && w->n_joint_refs == 0) {
        // no constraints this step: prepare, advance momenta and advance configurations are element-wise per body — one launch
        w->cur ^= 1;
        w->n_prev = 0;
        for (int i = 0; i < 4; ++i)
            if ((rc = stamp(i))) return rc;
        if ((rc = ivx_launch_phys_free_step(w, dt))) return rc;
        return stamp(4);
    }
    if ((rc = stamp(0))) return rc;
    if (!w->prepared_fresh)
        if ((rc = ivx_world_prepare(w))) return rc;
    if ((rc = stamp(1))) return rc;
    if ((rc = ivx_launch_phys_pre_solve(w, dt))) return rc;
    if ((rc = stamp(2))) return rc;
    if ((rc = ivx_launch_phys_solve(w))) return rc;
    if ((rc = stamp(3))) return rc;
    if ((rc = ivx_launch_phys_post_solve(w, dt, 1, 1))) return rc;
    if ((rc = stamp(4))) return rc;
    w->prepared_fresh = 0;
    return IVX_OK;
}

// The tail of perform_physics_step (lib.rs:86-108): the clock moves on (new_simulation_time, host-side only) and the motion drivers, if the
// world has a set, are applied at the new time — one launch behind the advance of configurations; then the force generators and the gravity
// field, if the world has either, so that a spring sees a driven kinematic body at the new time. (stage_ms does not cover the tail.)
static int world_step_finish(ivx_world* w, float dt, const char* who) {
    w->time = w->time + dt;
    if (w->md_state)
        if (int rc = ivx_launch_motion_apply(w, w->time, who)) return rc;
    return w->fg_state ? ivx_launch_forces_apply(w, who) : IVX_OK;
}
// what the tail refuses, asked before the step launches anything
static int world_step_tail_ready(ivx_world* w, const char* who) {
    if (w->md_state)
        if (int rc = ivx_motion_ready(w, who)) return rc;
    return w->fg_state ? ivx_forces_ready(w, who) : IVX_OK;
}

int ivx_world_step_enqueue(ivx_world* w, float dt) {
    IVX_REQUIRE(w, IVX_ERR_INVALID, "ivx_world_step_enqueue: null world");
    if (int rc = ivx_world_check_solve(w, "ivx_world_step_enqueue")) return rc;  // (an earlier step's flag, if it is up by now)
    if (int rc = world_step_tail_ready(w, "ivx_world_step_enqueue")) return rc;
    if (int rc = world_step_enqueue(w, dt, false)) return rc;
    return world_step_finish(w, dt, "ivx_world_step_enqueue");
}

int ivx_world_step(ivx_world* w, float dt, ivx_physics_result* out) {
    IVX_REQUIRE(w, IVX_ERR_INVALID, "ivx_world_step: null world");
    int rc = world_step_tail_ready(w, "ivx_world_step");
    if (rc) return rc;
    if ((rc = world_step_enqueue(w, dt, out != nullptr))) return rc;
    if ((rc = world_step_finish(w, dt, "ivx_world_step"))) return rc;
    IVX_HIP_CHECK(ivx_stream_sync(w->ctx->stream));
    if ((rc = ivx_world_check_solve(w, "ivx_world_step"))) return rc;
    if (out) {
        memset(out, 0, sizeof(*out));
        out->n_contacts = w->n_contacts;
        out->n_levels[0] = w->sched.n_levels[0];
        out->n_levels[1] = w->sched.n_levels[1];
        out->n_bodies = w->sched.constrained_bodies(w->joint_refs_host, w->n_dyn, w->n_kin);
        for (int i = 0; i < 4; ++i)
            if (hipEventElapsedTime(&out->stage_ms[i], w->ev[i], w->ev[i + 1]) != hipSuccess) out->stage_ms[i] = 0.0f;
        if (hipEventElapsedTime(&out->stage_ms[4], w->ev[0], w->ev[4]) != hipSuccess) out->stage_ms[4] = 0.0f;
    }
    return IVX_OK;
}

int ivx_world_set_solver_groups(ivx_world* w, uint32_t groups) {
    IVX_REQUIRE(w && (groups <= 16u || groups == PHYS_SOLVER_STATIONARY), IVX_ERR_INVALID,
                "ivx_world_set_solver_groups: at most 16 workgroups (or 255: the chain-stationary solve)");
    w->solver_groups_forced = groups;
    return IVX_OK;
}

int ivx_world_solver_info(ivx_world* w, uint32_t out[8]) {
    IVX_REQUIRE(w && out, IVX_ERR_INVALID, "ivx_world_solver_info: null argument");
    out[0] = w->solver_groups_used;
    out[1] = w->sched.n_levels[0];
    out[2] = w->sched.n_levels[1];
    out[3] = w->sched.max_level_items[0];
    out[4] = w->sched.max_level_items[1];
    out[5] = w->sched.n_chains();
    out[6] = w->n_contacts;
    out[7] = w->solver_kind_used;
    return IVX_OK;
}

int ivx_world_contact_state(ivx_world* w, uint64_t* ids, float* impulses3, size_t cap, size_t* n_out) {
    IVX_REQUIRE(w && n_out, IVX_ERR_INVALID, "ivx_world_contact_state: null argument");
    *n_out = w->n_contacts;
    IVX_REQUIRE(w->n_contacts <= cap, IVX_ERR_CAPACITY, "ivx_world_contact_state: %u contacts exceed capacity %zu", w->n_contacts, cap);
    if (ids)
        for (uint32_t s = 0; s < w->n_contacts; ++s) ids[s] = w->sched.cache[s].id;
    if (impulses3 && w->n_contacts) {
        IVX_HIP_CHECK(ivx_stream_sync(w->ctx->stream));
        if (int rc = ivx_world_check_solve(w, "ivx_world_contact_state")) return rc;
        std::vector<float> a((size_t)w->n_contacts * 4);
        IVX_HIP_CHECK(ivx_memcpy_sync(a.data(), w->acc[w->cur].p, a.size() * 4, hipMemcpyDeviceToHost));
        for (uint32_t s = 0; s < w->n_contacts; ++s)
            for (int q = 0; q < 3; ++q) impulses3[3 * (size_t)s + q] = a[4 * (size_t)s + q];
    }
    return IVX_OK;
}

}  // extern "C"
