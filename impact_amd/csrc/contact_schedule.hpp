// Host-side bookkeeping of a world's contact set, with no HIP in it: everything that is inherently sequential and tiny per item in the reference —
//   * interlock analysis of a manifold and its separating contact     constraint/contact.rs:610-780
//   * ConstraintCache order + warm-start source of every contact      constraint/solver.rs:386-452
//   * chains, dependency levels and the two schedule forms the solve kernels read (physics.hip)
// ivx_world_set_contacts (physics_api.hip) calls the operations in order and owns every device array, stream operation and wait;
// tools/contact_schedule_check.cpp drives the same operations without a GPU.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "../../include/impact_voxel_hip.h"

#define PHYS_ITEM_WARM 0u
#define PHYS_ITEM_VELOCITY 1u
#define PHYS_ITEM_POSITIONAL 2u
// A chain is at most this many contacts: what the chain-stationary solve keeps of a chain in one lane's registers (longer manifolds are
// consecutive chains on the same pair; the dependency schedule orders them like any two items that share a body)
#define PHYS_CHAIN_MAX 4u
// the chain-stationary solve (physics.hip, k_solve_cs): waves per workgroup, and the most workgroups one phase may ask for (its working
// workgroups share one XCD: 32 CUs, one workgroup of 12 x 64 threads — three waves per SIMD at up to 168 registers — on each)
#define PHYS_CS_WAVES 12u
#define PHYS_CS_MAX_GROUPS 32u

// IVX_WORLD_TRACE, read once: 0 unset, 1 the paths and stages of ivx_world_set_contacts, 2 the passes inside the schedule builders as well
inline int ivx_world_trace_level() {
    static const int level = [] {
        const char* e = getenv("IVX_WORLD_TRACE");
        return e ? std::max(1, atoi(e)) : 0;
    }();
    return level;
}
// a lap clock of that trace: prints the time since the lap before when the trace level is at least its own
struct ivx_world_lap {
    int level;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit ivx_world_lap(int lvl) : level(lvl) {}
    void operator()(const char* what) {
        if (ivx_world_trace_level() < level) return;
        const auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "[ivx world] %s%s: %.1f us\n", level >= 2 ? "    " : "  ", what, 1e-3 * (double)std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count());
        t0 = t1;
    }
};

struct ivx_contact_schedule {
    // host-side ConstraintCache<ContactID, _> bookkeeping (constraint/solver.rs:60-66, 386-452)
    struct Entry {
        uint64_t id;
        int32_t prev_slot;
        uint32_t src;
        bool prepared;
    };
    std::vector<Entry> cache;
    // id -> slot: open addressing, linear probing, deletion by backward shift; a value of ~0 marks an empty entry. (The std::unordered_map it
    // replaces cost 0.7-1.0 ms per frame at 41 472 contacts of which a tenth had changed: a node allocation per insert, a pointer chase per find.)
    std::vector<uint64_t> id_keys;
    std::vector<uint32_t> id_vals;
    size_t id_used = 0;
    std::vector<ivx_contact> effective;   // contacts of this step after interlock replacement (only when a manifold is interlocked)
    std::vector<uint32_t> slot_bodies;    // (body_a, body_b) of every resident contact in slot order
    std::vector<int32_t> prev_slot_host;  // the slot every resident contact had in the set before (-1: new): its warm-start source
    // chains: maximal runs (<= PHYS_CHAIN_MAX) of contacts that are consecutive in the solve order and act on the same (body_a, body_b);
    // last frame's chains (an unchanged contact structure keeps its schedule)
    std::vector<uint32_t> chain_start, chain_bodies, prev_chain_start, prev_chain_bodies;
    // what build_levels makes of the schedule: per phase the level of every item (pass-major, chains in solve order), the levels' extents and
    // whether the chain-stationary form exists; the forms the kernels read are built on demand (build_form: bit 0 the level-ordered items and
    // tiles, bit 1 the chain-stationary tiles)
    std::vector<uint32_t> lvl_host[2], level_start_host;
    uint32_t n_levels[2] = {0, 0}, max_level_items[2] = {0, 0};  // levels and the widest level of each phase's schedule
    uint32_t phase_items[2] = {0, 0}, item_offset[2] = {0, 0}, level_offset[2] = {0, 0};
    uint32_t n_tiles[2] = {0, 0}, tile_offset[2] = {0, 0};
    int cs_feasible[2] = {0, 0};
    uint32_t forms_built = 0;
    // form 1 (k_solve, k_solve_mg): the level-ordered item list; per item the constrained-body indices of its pair and four tags: the versions
    // it finds its bodies a and b at (a body's record carries the number of items that have touched it this phase), the sweep tag it finds on
    // its contacts' accumulated impulses, the tag it leaves there. Tiles of 64 consecutive items of a level: tile_base per level (indexed like
    // level_start) the phase-relative index of its first tile; tile_first per tile the phase-relative index of its first item | (items - 1) << 26
    std::vector<uint32_t> items_host, item_bodies_host, item_tags_host, tile_base_host, tile_first_host;
    // form 2 (k_solve_cs): every chain lives in a pair of lanes of one wave for the whole phase (even lane: body A's side, odd: B's). Per phase:
    // tiles of 32 chains in the order of their first level; per slot (tile * 64 + lane) the chain word (first contact | length << 24, ~0 = empty),
    // the lane's own body and the other one (constrained-body indices), and degree | rank << 16 of the chain on the own body — the version that
    // body's record has when sweep s of the chain starts is s * degree + rank; per tile its rounds in level order (64-bit lane masks, the level
    // beside each). cs_slot_of: positional phase with kinematic bodies only, [(tile * 32 + pair) * passes + sweep] -> the item's index in the
    // level schedule (what ReplayView is indexed by).
    struct CsSchedule {
        uint32_t n_tiles = 0;  // 0: this phase cannot run chain-stationary (too many chains, a body with more than 65535 chains)
        uint32_t slot_offset = 0, round_start_offset = 0, round_offset = 0;  // into cs_item / cs_bodies / cs_vers, cs_round_start, cs_round_mask
    } cs[2];
    std::vector<uint32_t> cs_item_host, cs_bodies_host, cs_vers_host, cs_round_start_host, cs_round_level_host, cs_slot_of_host;
    std::vector<uint64_t> cs_round_mask_host;
    // kinematic orientations in the positional phase (physics.hip, ReplayView): the positional chains of every kinematic body in solve order
    // (CSR: kin_offsets[n_kin + 1], kin_list: phase-relative item | side << 31)
    std::vector<uint32_t> kin_offsets_host, kin_list_host, cs_slot_of_level;
    uint32_t n_kin_items = 0;  // positional items that involve a kinematic body (0: the phase runs once, as without kinematic bodies)
    std::vector<uint32_t> scratch_count, scratch_last, scratch_rank, scratch_order, scratch_first;
    std::vector<uint64_t> scratch_mask, scratch_bits;
    uint32_t n_bodies = 0;  // constrained bodies of the resident contacts and joints (ivx_physics_result::n_bodies), while `n_bodies_valid`
    bool n_bodies_valid = false;  // (a function of the contact list, the joints and the body counts: whoever changes one of them clears it)

    uint32_t n_chains() const { return chain_start.empty() ? 0u : (uint32_t)chain_start.size() - 1u; }

    // the one walk over manifolds: f(first, count) for every run from a manifold start to the next, until f answers false
    template <class F>
    static void for_each_manifold(const ivx_contact* contacts, size_t n, F f) {
        size_t i = 0;
        while (i < n) {
            size_t j = i + 1;
            while (j < n && !(contacts[j].flags & IVX_CONTACT_MANIFOLD_START)) ++j;
            if (!f(i, j - i)) return;
            i = j;
        }
    }

    // The usual frame: the contacts of the frame before with new geometry — the same ids in the same order on the same body pairs, no manifold
    // interlocked? One pass, which copies every contact it has looked at into `out` (the caller's upload block) as it goes. The caller has made
    // sure that n is the resident count. (The resident body references were validated when they came in.)
    bool same_as_resident(const ivx_contact* contacts, size_t n, ivx_contact* out) const;
    // the body references of every contact, and is any manifold interlocked (constraint.rs:237-249)?
    enum { CONTACT_OK = 0, CONTACT_MISSING_BODY, CONTACT_SELF_PAIR };
    struct Verdict {
        int kind;      // of the first bad contact, CONTACT_OK if there is none
        size_t index;  // ... and which it is
        bool any_interlocked;
    };
    static Verdict validate(const ivx_contact* contacts, size_t n, uint32_t n_dyn, uint32_t n_kin);
    // `effective`: the list with every interlocked manifold replaced by its separating contact. body_position(ref, float[3]) -> error code
    // supplies the bodies' positions (on the device: rare, and slow).
    int replace_interlocked(const ivx_contact* contacts, size_t n, const std::function<int(uint32_t, float*)>& body_position);
    static uint32_t id_hash(uint64_t id) { return (uint32_t)((id * 0x9E3779B97F4A7C15ull) >> 32); }
    void id_table_reset(size_t want);
    size_t id_find_pos(uint64_t id) const {  // position of the id's entry, or of the empty entry its probe ends at
        const size_t mask = id_keys.size() - 1;
        size_t h = id_hash(id) & mask;
        while (id_vals[h] != 0xFFFFFFFFu && id_keys[h] != id) h = (h + 1) & mask;
        return h;
    }
    void id_erase(uint64_t id);
    // ConstraintCache::register_prepared_constraint + remove_unprepared_constraints (solver.rs:406-452): every id keeps its slot, new ids are
    // appended, ids that did not come are swap-removed in slot order. An id is looked for at the slot behind the one its predecessor in the
    // input had first (a run of contacts that stayed together costs a comparison each), then in the id table. Returns the resident count.
    uint32_t register_contacts(const ivx_contact* eff, size_t n_eff);
    // ... and the registered contacts in slot order into `out` (the block their upload is made from: one copy of each contact on the host),
    // their body pairs and warm-start sources beside them
    void write_slot_order(const ivx_contact* eff, ivx_contact* out);
    void build_chains();
    // The levels of the two phases' items, (warm pass + velocity sweeps) and (positional sweeps), unless the chains and their body pairs are
    // last frame's and `keep` allows it: the schedule depends on nothing else, so an unchanged contact structure keeps its schedule, host and
    // device copies. Answers whether it was kept.
    bool build_levels(bool keep, uint32_t n_iterations, uint32_t n_positional, uint32_t n_dyn, uint32_t n_kin);
    // The schedule form the solve is about to use, from the levels — 1: the level-ordered item list, tags and tiles (k_solve, k_solve_mg),
    // 2: the chain-stationary tiles and rounds (k_solve_cs). Only the one in use is built and uploaded: a frame whose contact set changed used
    // to build and upload both, 1.4 of its 2.6 ms on the host at 41 472 contacts.
    void build_form(uint32_t form, uint32_t n_iterations, uint32_t n_positional, uint32_t n_dyn);
    // The step's constrained bodies: the dynamic bodies the device marks (k_prepare_contacts: both bodies of every contact; k_mark_bodies: the
    // joints' dynamic anchors) and the kinematic bodies of the contacts — counted from the host's copies of the same lists, once per contact
    // list (a read-back of the marks and a walk over 46 080 contacts every step were 60 us of a 1 ms step)
    uint32_t constrained_bodies(const std::vector<uint32_t>& joint_refs, uint32_t n_dyn, uint32_t n_kin);

private:
    bool stationary_feasible(uint32_t nch, uint32_t passes, uint32_t n_dyn);
    void build_phase_levels(uint32_t n_first, uint32_t n_passes, int phase, uint32_t n_dyn, uint32_t n_kin);
    void build_items(uint32_t first_type, uint32_t n_first, uint32_t type, uint32_t n_passes, int phase, uint32_t n_dyn);
    void build_stationary(int phase, uint32_t nch, uint32_t passes, uint32_t n_dyn);
};
