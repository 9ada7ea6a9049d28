// The solver launcher's host-side decisions, free of HIP: which of the three solve forms a step runs and the operations it enqueues, in
// order (solve_plan), and the developer switches. ivx_launch_phys_solve (physics.hip) executes the plan; tools/solve_plan_check.cpp holds it
// to sequences written out by hand, without a GPU (tests/test_solve_plan_cpu.py).
#pragma once
#include <cassert>
#include <cstdint>
#include <cstdlib>

#include "contact_schedule.hpp"

#define PHYS_SOLVER_STATIONARY 255u  // ivx_world_set_solver_groups: force the chain-stationary solve where the schedule allows it

namespace ivx_solve {

// Developer switches, never set in production; read from the environment once:
//   IVX_SOLVER_DRY     bit 0 = walk the levels without running the chains, bit 1 = without the grid barrier — how tools/time_pile.py splits a
//                      level's time into arithmetic and synchronisation (results are garbage with either)
//   IVX_SOLVER_NAP     tenths of a level a wave of k_solve_cs wakes ahead of its round (default 20); 0 = never sleeps
//   IVX_SOLVER_SPREAD  8 (default) = a launch holds 8 blocks per working workgroup, which then share one XCD under round-robin placement;
//                      1 = consecutive blocks (see k_solve_mg, k_solve_cs)
//   IVX_SOLVER_SERIAL  non-zero = the tile-dataflow phases one after the other on the context's stream
//   IVX_SOLVER_TRACE   <file> = every round's four clock stamps of the first k_solve_cs launch of each step, dumped as [phase][round][4] u64
//                      behind a header of {rounds of phase 0, rounds of phase 1} (tools/solver_trace.py reads it); the step then waits
struct SolveSwitches {
    uint32_t dry, nap;
    int spread;
    bool serial;
    const char* trace_path;
    // k_solve_mg works on every spread-th block, whatever the stride: 1..8
    uint32_t spread_mg() const { return (uint32_t)(spread < 1 ? 1 : (spread > 8 ? 8 : spread)); }
    // k_solve_cs takes block b % spread as the phase, and its feasibility counts an eighth of the CUs per phase: 8 or nothing
    uint32_t spread_cs() const { return spread < 2 ? 1u : 8u; }
};
inline const SolveSwitches& solve_switches() {
    static const SolveSwitches s = [] {
        const auto num = [](const char* name, int unset) {
            const char* e = getenv(name);
            return e ? atoi(e) : unset;
        };
        return SolveSwitches{(uint32_t)num("IVX_SOLVER_DRY", 0), (uint32_t)num("IVX_SOLVER_NAP", 20), num("IVX_SOLVER_SPREAD", 8), num("IVX_SOLVER_SERIAL", 0) != 0,
                             getenv("IVX_SOLVER_TRACE")};
    }();
    return s;
}
// ... and the device buffer IVX_SOLVER_TRACE's stamps are written to, grown to the rounds of the largest schedule met (`cap` in u64 words)
struct SolveTrace {
    unsigned long long* dev = nullptr;
    size_t cap = 0;
};

constexpr uint32_t LDS_BODY_BYTES = 143360u;    // 140 KiB: a phase's mutable body state goes to LDS when it fits one CU beside the level table
constexpr uint32_t BODY_BYTES[2] = {24u, 28u};  // ... per dynamic body: velocity phase (v, w), positional phase (position, orientation)
constexpr uint32_t ONE_GROUP_ITEMS = 256u;      // a level that fits one workgroup at one wave per SIMD gains nothing from more
constexpr uint32_t GROUP_ITEMS = 160u;  // a few more waves than the widest level has tiles: measured on the 4096-body pile, 8 workgroups 0.85 ms, 5: 0.89, 16: 0.86
constexpr uint32_t MAX_GROUPS = 16u;    // all resident: 256 CUs
constexpr uint32_t STATIONARY_LEVELS = 48u;  // from here on the chain-stationary solve wins whatever the width (solve_plan)
constexpr uint32_t BLOCK_STRIDE = 8u;        // every eighth block works (k_solve_mg, k_solve_cs): an eighth of the CUs is one XCD's worth
constexpr uint32_t MAX_STEPS = 16u;

struct SolvePlanIn {
    uint32_t n_contacts, n_dyn, n_kin;
    uint32_t n_levels[2], max_level_items[2];
    bool cs_feasible[2];
    uint32_t n_chains, n_kin_items;
    uint32_t forced;  // ivx_world_set_solver_groups: 0 automatic, 1..16 that many workgroups, 255 chain-stationary where the schedule allows it
    bool mg_disabled;
    uint32_t n_cu;
    int mg_blocks_per_cu, cs_blocks_per_cu;  // occupancy answers: the smaller of the two k_solve_mg phases', k_solve_cs's
    bool serial, tracing;
};
enum Op : uint8_t { PACK_ITEMS, FORK, JOIN_RECORD, JOIN_WAIT, CLEAR_FLAG, SNAPSHOT, SOLVE, KIN_PREFIX, RESTORE, CS_INIT, CS_SOLVE, CS_FINISH, TRACE_CLEAR, TRACE_DUMP };
struct Step {
    uint8_t op;
    uint8_t phase;   // PACK_ITEMS, SOLVE: which phase's; 0 elsewhere
    uint8_t stream;  // 0 the context's, 1 the world's side stream
    uint8_t pass;    // of the positional phase. SOLVE of phase 1, CS_SOLVE: 1 the pass that counts (or the only one), 2 the replay under the
                     // flag; CS_INIT: 0 both halves, 2 the positional half under the flag; 0 elsewhere
};
struct SolvePlan {
    uint32_t kind;    // 0 one workgroup (k_solve), 1 tile dataflow (k_solve_mg), 2 chain-stationary (k_solve_cs)
    uint32_t form;    // of the schedule (ivx_world_ensure_form): 1 level-ordered items, 2 chain-stationary tiles; 0 with nothing to do
    uint32_t groups;  // working workgroups; chain-stationary: of both phases together
    uint32_t lds_bytes[2];  // kind 0, per phase: the bodies' LDS bytes, 0 = bodies in global memory ...
    bool in_lds[2];         // ... except without dynamic bodies, where the LDS form runs on 0 bytes
    bool replay;            // the positional phase runs twice
    uint32_t n_steps;
    Step step[MAX_STEPS];  // in enqueue order
};

inline SolvePlan solve_plan(const SolvePlanIn& in) {
    SolvePlan pl{};
    if (in.n_contacts == 0u) return pl;
    const bool has[2] = {in.n_levels[0] != 0u, in.n_levels[1] != 0u};
    const uint32_t widest = in.max_level_items[0] > in.max_level_items[1] ? in.max_level_items[0] : in.max_level_items[1];
    // the positional phase runs twice when kinematic bodies take part in it (ReplayView, physics.hip): pass 1 counts, k_kin_prefix raises the
    // flag where an orientation moves, pass 2 — under the flag, from the state pass 1 began with — runs on the orientations it tabulated
    pl.replay = has[1] && in.n_kin_items > 0u;
    auto add = [&pl](Op op, uint32_t phase = 0u, uint32_t stream = 0u, uint32_t pass = 0u) {
        assert(pl.n_steps < MAX_STEPS);
        pl.step[pl.n_steps++] = Step{(uint8_t)op, (uint8_t)phase, (uint8_t)stream, (uint8_t)pass};
    };
    // The chain-stationary solve: can this schedule run on it, and should it? Needs every phase that has levels in stationary form, one
    // workgroup per CU and an eighth of the CUs per phase for its workgroups. One workgroup with the bodies in LDS walks a level in ~4-5 us
    // whatever its width — a barrier and the contacts' trip from memory —, the chain-stationary solve in ~2.3 (velocity) / ~3.5 (positional)
    // plus ~25 us of launches and census around it: it wins wherever the chain of levels is long, wide or not (81 bodies of 48 contacts each
    // on a ground plane: 297 + 99 levels of at most 79 chains, 0.55 -> 0.21 ms; tools/time_world_frames.py). A handful of levels stays
    // with the one workgroup.
    const uint32_t cs_groups = ((in.n_chains + 31u) / 32u + PHYS_CS_WAVES - 1u) / PHYS_CS_WAVES;  // per phase: tiles of 32 chains, a wave each
    const bool groups_forced = in.forced >= 1u && in.forced <= MAX_GROUPS;
    if (!in.mg_disabled && !groups_forced && (has[0] || has[1]) && (!has[0] || in.cs_feasible[0]) && (!has[1] || in.cs_feasible[1]) &&
        in.cs_blocks_per_cu >= 1 && cs_groups <= in.n_cu / BLOCK_STRIDE &&
        (in.forced == PHYS_SOLVER_STATIONARY || widest > ONE_GROUP_ITEMS || in.n_levels[0] + in.n_levels[1] >= STATIONARY_LEVELS)) {
        pl.kind = 2u, pl.form = 2u, pl.groups = cs_groups * ((has[0] ? 1u : 0u) + (has[1] ? 1u : 0u));
        if (pl.replay) add(CLEAR_FLAG);
        if (in.tracing) add(TRACE_CLEAR);
        if (in.n_dyn) add(CS_INIT);
        add(CS_SOLVE, 0u, 0u, 1u);  // the velocity phase and positional pass 1 in one launch
        if (pl.replay) {            // the positional phase again: its bodies' records from the untouched body array
            add(KIN_PREFIX);
            if (in.n_dyn) add(CS_INIT, 0u, 0u, 2u);
            add(CS_SOLVE, 0u, 0u, 2u);
        }
        if (in.tracing) add(TRACE_DUMP);
        if (in.n_dyn) add(CS_FINISH);
        return pl;
    }
    // Workgroups of the tile-dataflow solve: as many as the widest level fills, all co-resident — the grid barrier rests on that, so
    // groups x BLOCK_STRIDE blocks must fit the device (the occupancy answer); a world whose barrier ever timed out stays on one workgroup
    const uint32_t fit = (uint32_t)(in.mg_blocks_per_cu > 0 ? in.mg_blocks_per_cu : 0) * in.n_cu / BLOCK_STRIDE;
    const auto least = [](uint32_t a, uint32_t b) { return a < b ? a : b; };
    if (in.mg_disabled || fit < 2u) pl.groups = 1u;
    else if (groups_forced) pl.groups = least(in.forced, fit);
    else if (widest <= ONE_GROUP_ITEMS) pl.groups = 1u;
    else pl.groups = least(least((widest + GROUP_ITEMS - 1u) / GROUP_ITEMS, MAX_GROUPS), fit);
    pl.kind = pl.groups > 1u ? 1u : 0u, pl.form = 1u;
    for (int p = 0; p < 2 && pl.kind == 0u; ++p) {
        const uint64_t bytes = (uint64_t)in.n_dyn * BODY_BYTES[p];
        pl.in_lds[p] = bytes <= LDS_BODY_BYTES;
        pl.lds_bytes[p] = pl.in_lds[p] ? (uint32_t)bytes : 0u;
    }
    // THE positional sequence, on stream st
    const auto positional = [&](uint32_t st) {
        if (pl.replay) add(CLEAR_FLAG, 0u, st), add(SNAPSHOT, 0u, st);
        add(SOLVE, 1u, st, 1u);  // (without a replay: the only pass, on empty views)
        if (pl.replay) add(KIN_PREFIX, 0u, st), add(RESTORE, 0u, st), add(SOLVE, 1u, st, 2u);
    };
    // Tile dataflow, THE TWO PHASES SIDE BY SIDE. The velocity phase reads and writes velocities (and the accumulated impulses); the
    // positional phase reads and writes positions and orientations; what either reads of the other's — the configuration the velocity items
    // are linearised about, inverse masses and inertia — is in its packed records, taken from the body array before either starts (the
    // reference runs the positional correction on the configuration the step began with, solver.rs:496-602, and integrates afterwards). Each
    // phase is a chain of dependent tiles a handful of waves deep — 183 and 147 levels on the 4096-body pile, of which 135 are the fill of
    // one sweep over the lattice —, so one after the other they cost the sum, on two streams the longer one.
    if (pl.kind == 1u && has[0]) add(PACK_ITEMS, 0u);
    if (pl.kind == 1u && has[1]) add(PACK_ITEMS, 1u);
    if (pl.kind == 1u && has[0] && has[1] && !in.serial) {
        add(FORK);
        positional(1u);  // (the side stream first: its launches are in flight while the host enqueues the velocity phase)
        add(JOIN_RECORD, 0u, 1u);
        add(SOLVE);
        add(JOIN_WAIT);
    } else {  // one workgroup, or one stream
        if (has[0]) add(SOLVE);
        if (has[1]) positional(0u);
    }
    return pl;
}

}  // namespace ivx_solve
