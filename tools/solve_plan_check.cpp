// The solver launcher's plan (impact_amd/csrc/solve_plan.hpp) checked on the host, without the HIP runtime:
//   solve_plan_check table            inputs with the expected form, workgroups, LDS bytes and exact step sequence, written out by hand from the
//                                     rules (tests/test_solve_plan_cpu.py)
//   solve_plan_check random N [seed]  N random inputs: the choice against a transcription of what the plan replaced — solver_stationary,
//                                     solver_groups and the LDS conditions of physics.hip as they stood, on a plain struct with the field names
//                                     they had — and the invariants of the step sequence
// Build: g++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/solve_plan_check.cpp -o solve_plan_check
#include <cstdio>
#include <cstring>
#include <random>
#include <string>

#include "../impact_amd/csrc/solve_plan.hpp"

using namespace ivx_solve;

static std::string steps_text(const SolvePlan& pl) {
    static const char* const names[] = {"pack", "fork", "jrec", "jwait", "clear", "snap", "solve", "prefix", "restore", "csinit", "cssolve", "csfinish", "trclear", "trdump"};
    std::string s;
    for (uint32_t i = 0; i < pl.n_steps; ++i) {
        const Step& st = pl.step[i];
        if (i) s += ' ';
        s += names[st.op];
        if (st.op == PACK_ITEMS || st.op == SOLVE) s += ':', s += (char)('0' + st.phase);
        else if (st.phase) s += ":?";  // (a phase where none belongs)
        if (st.pass) s += '/', s += (char)('0' + st.pass);
        if (st.stream) s += "@1";
    }
    return s;
}

// ---- the table -----------------------------------------------------------------------------------------------------------------------------
// 256 CUs, two k_solve_mg blocks and one k_solve_cs block per CU: fit = 64 workgroups, at most 32 chain-stationary workgroups per phase
// (12 288 chains); 50 dynamic bodies (1200 / 1400 bytes of LDS), 30 chains (one chain-stationary workgroup per phase), 10 + 5 levels of at
// most 20 items: one workgroup unless a row says otherwise
static SolvePlanIn base() { return SolvePlanIn{100, 50, 0, {10, 5}, {20, 20}, {true, true}, 30, 0, 0, false, 256, 2, 1, false, false}; }
typedef void (*Change)(SolvePlanIn&);
struct Row {
    const char* what;
    Change change;
    uint32_t kind, form, groups;
    long lds[2];  // bytes, -1: the bodies in global memory
    const char* steps;
};
static const Row rows[] = {
    {"no contacts", [](SolvePlanIn& in) { in.n_contacts = 0; }, 0, 0, 0, {0, 0}, ""},
    // one workgroup
    {"one workgroup", [](SolvePlanIn&) {}, 0, 1, 1, {1200, 1400}, "solve:0 solve:1/1"},
    {"one workgroup, velocity only", [](SolvePlanIn& in) { in.n_levels[1] = 0; }, 0, 1, 1, {1200, 1400}, "solve:0"},
    {"one workgroup, positional only", [](SolvePlanIn& in) { in.n_levels[0] = 0; }, 0, 1, 1, {1200, 1400}, "solve:1/1"},
    {"one workgroup, replay", [](SolvePlanIn& in) { in.n_kin = 2, in.n_kin_items = 3; }, 0, 1, 1, {1200, 1400}, "solve:0 clear snap solve:1/1 prefix restore solve:1/2"},
    {"one workgroup, positional only, replay", [](SolvePlanIn& in) { in.n_levels[0] = 0, in.n_kin = 2, in.n_kin_items = 3; }, 0, 1, 1, {1200, 1400}, "clear snap solve:1/1 prefix restore solve:1/2"},
    {"kinematic items, no positional levels: no replay", [](SolvePlanIn& in) { in.n_levels[1] = 0, in.n_kin = 2, in.n_kin_items = 3; }, 0, 1, 1, {1200, 1400}, "solve:0"},
    {"one workgroup, serial and tracing change nothing", [](SolvePlanIn& in) { in.serial = in.tracing = true; }, 0, 1, 1, {1200, 1400}, "solve:0 solve:1/1"},
    {"no dynamic bodies: the LDS form on 0 bytes", [](SolvePlanIn& in) { in.n_dyn = 0, in.n_kin = 2, in.n_kin_items = 3; }, 0, 1, 1, {0, 0}, "solve:0 clear snap solve:1/1 prefix restore solve:1/2"},
    {"5120 bodies: both phases in LDS", [](SolvePlanIn& in) { in.n_dyn = 5120, in.n_kin = 2, in.n_kin_items = 3; }, 0, 1, 1, {122880, 143360}, "solve:0 clear snap solve:1/1 prefix restore solve:1/2"},
    {"5121 bodies: the positional phase in global memory", [](SolvePlanIn& in) { in.n_dyn = 5121, in.n_kin = 2, in.n_kin_items = 3; }, 0, 1, 1, {122904, -1}, "solve:0 clear snap solve:1/1 prefix restore solve:1/2"},
    {"5973 bodies: the velocity phase still in LDS", [](SolvePlanIn& in) { in.n_dyn = 5973, in.n_kin = 2, in.n_kin_items = 3; }, 0, 1, 1, {143352, -1}, "solve:0 clear snap solve:1/1 prefix restore solve:1/2"},
    {"5974 bodies: both phases in global memory", [](SolvePlanIn& in) { in.n_dyn = 5974, in.n_kin = 2, in.n_kin_items = 3; }, 0, 1, 1, {-1, -1}, "solve:0 clear snap solve:1/1 prefix restore solve:1/2"},
    // tile dataflow
    {"forced 2", [](SolvePlanIn& in) { in.forced = 2; }, 1, 1, 2, {0, 0}, "pack:0 pack:1 fork solve:1/1@1 jrec@1 solve:0 jwait"},
    {"forced 2, replay", [](SolvePlanIn& in) { in.forced = 2, in.n_kin = 2, in.n_kin_items = 3; }, 1, 1, 2, {0, 0},
     "pack:0 pack:1 fork clear@1 snap@1 solve:1/1@1 prefix@1 restore@1 solve:1/2@1 jrec@1 solve:0 jwait"},
    {"forced 2, serial", [](SolvePlanIn& in) { in.forced = 2, in.serial = true; }, 1, 1, 2, {0, 0}, "pack:0 pack:1 solve:0 solve:1/1"},
    {"forced 2, serial, replay", [](SolvePlanIn& in) { in.forced = 2, in.serial = true, in.n_kin = 2, in.n_kin_items = 3; }, 1, 1, 2, {0, 0},
     "pack:0 pack:1 solve:0 clear snap solve:1/1 prefix restore solve:1/2"},
    {"forced 2, velocity only: no fork", [](SolvePlanIn& in) { in.forced = 2, in.n_levels[1] = 0; }, 1, 1, 2, {0, 0}, "pack:0 solve:0"},
    {"forced 2, positional only: no fork", [](SolvePlanIn& in) { in.forced = 2, in.n_levels[0] = 0; }, 1, 1, 2, {0, 0}, "pack:1 solve:1/1"},
    {"forced 2, positional only, replay", [](SolvePlanIn& in) { in.forced = 2, in.n_levels[0] = 0, in.n_kin = 2, in.n_kin_items = 3; }, 1, 1, 2, {0, 0},
     "pack:1 clear snap solve:1/1 prefix restore solve:1/2"},
    {"forced 16, fit 64", [](SolvePlanIn& in) { in.forced = 16; }, 1, 1, 16, {0, 0}, "pack:0 pack:1 fork solve:1/1@1 jrec@1 solve:0 jwait"},
    {"forced 16, fit 4", [](SolvePlanIn& in) { in.forced = 16, in.n_cu = 32, in.mg_blocks_per_cu = 1; }, 1, 1, 4, {0, 0}, "pack:0 pack:1 fork solve:1/1@1 jrec@1 solve:0 jwait"},
    {"forced 2, fit 1: one workgroup", [](SolvePlanIn& in) { in.forced = 2, in.n_cu = 8, in.mg_blocks_per_cu = 1; }, 0, 1, 1, {1200, 1400}, "solve:0 solve:1/1"},
    {"forced 2, no occupancy answer: one workgroup", [](SolvePlanIn& in) { in.forced = 2, in.mg_blocks_per_cu = -1; }, 0, 1, 1, {1200, 1400}, "solve:0 solve:1/1"},
    {"forced 1 on a wide, long schedule", [](SolvePlanIn& in) { in.forced = 1, in.max_level_items[0] = 1000, in.n_levels[0] = 100; }, 0, 1, 1, {1200, 1400}, "solve:0 solve:1/1"},
    {"a world whose barrier timed out", [](SolvePlanIn& in) { in.mg_disabled = true, in.max_level_items[0] = 1000, in.n_levels[0] = 100; }, 0, 1, 1, {1200, 1400}, "solve:0 solve:1/1"},
    {"a world whose barrier timed out, forced 255", [](SolvePlanIn& in) { in.mg_disabled = true, in.forced = 255; }, 0, 1, 1, {1200, 1400}, "solve:0 solve:1/1"},
    {"widest 256, not stationary: one workgroup", [](SolvePlanIn& in) { in.cs_feasible[0] = false, in.max_level_items[1] = 256; }, 0, 1, 1, {1200, 1400}, "solve:0 solve:1/1"},
    {"widest 257, not stationary: 2 workgroups", [](SolvePlanIn& in) { in.cs_feasible[0] = false, in.max_level_items[1] = 257; }, 1, 1, 2, {0, 0},
     "pack:0 pack:1 fork solve:1/1@1 jrec@1 solve:0 jwait"},
    {"widest 1000, not stationary: 7 workgroups", [](SolvePlanIn& in) { in.cs_feasible[1] = false, in.max_level_items[0] = 1000; }, 1, 1, 7, {0, 0},
     "pack:0 pack:1 fork solve:1/1@1 jrec@1 solve:0 jwait"},
    {"widest 5000, not stationary: at most 16", [](SolvePlanIn& in) { in.cs_feasible[1] = false, in.max_level_items[0] = 5000; }, 1, 1, 16, {0, 0},
     "pack:0 pack:1 fork solve:1/1@1 jrec@1 solve:0 jwait"},
    {"forced 255, not stationary, fit 64", [](SolvePlanIn& in) { in.forced = 255, in.cs_feasible[1] = false, in.max_level_items[0] = 1000; }, 1, 1, 7, {0, 0},
     "pack:0 pack:1 fork solve:1/1@1 jrec@1 solve:0 jwait"},
    {"forced 255, not stationary, fit 4", [](SolvePlanIn& in) { in.forced = 255, in.cs_feasible[1] = false, in.max_level_items[0] = 1000, in.n_cu = 32, in.mg_blocks_per_cu = 1; },
     1, 1, 4, {0, 0}, "pack:0 pack:1 fork solve:1/1@1 jrec@1 solve:0 jwait"},
    {"forced 255, no k_solve_cs block fits a CU", [](SolvePlanIn& in) { in.forced = 255, in.cs_blocks_per_cu = 0; }, 0, 1, 1, {1200, 1400}, "solve:0 solve:1/1"},
    // chain-stationary
    {"forced 255", [](SolvePlanIn& in) { in.forced = 255; }, 2, 2, 2, {0, 0}, "csinit cssolve/1 csfinish"},
    {"forced 255, fit 1", [](SolvePlanIn& in) { in.forced = 255, in.n_cu = 8, in.mg_blocks_per_cu = 1; }, 2, 2, 2, {0, 0}, "csinit cssolve/1 csfinish"},
    {"forced 255, velocity only (the empty phase's feasibility is not asked)", [](SolvePlanIn& in) { in.forced = 255, in.n_levels[1] = 0, in.cs_feasible[1] = false; }, 2, 2, 1,
     {0, 0}, "csinit cssolve/1 csfinish"},
    {"forced 255, positional only", [](SolvePlanIn& in) { in.forced = 255, in.n_levels[0] = 0, in.cs_feasible[0] = false; }, 2, 2, 1, {0, 0}, "csinit cssolve/1 csfinish"},
    {"forced 255, no levels at all", [](SolvePlanIn& in) { in.forced = 255, in.n_levels[0] = in.n_levels[1] = 0; }, 0, 1, 1, {1200, 1400}, ""},
    {"forced 255, replay", [](SolvePlanIn& in) { in.forced = 255, in.n_kin = 2, in.n_kin_items = 3; }, 2, 2, 2, {0, 0},
     "clear csinit cssolve/1 prefix csinit/2 cssolve/2 csfinish"},
    {"forced 255, tracing", [](SolvePlanIn& in) { in.forced = 255, in.tracing = true; }, 2, 2, 2, {0, 0}, "trclear csinit cssolve/1 trdump csfinish"},
    {"forced 255, replay, tracing", [](SolvePlanIn& in) { in.forced = 255, in.tracing = true, in.n_kin = 2, in.n_kin_items = 3; }, 2, 2, 2, {0, 0},
     "clear trclear csinit cssolve/1 prefix csinit/2 cssolve/2 trdump csfinish"},
    {"forced 255, no dynamic bodies", [](SolvePlanIn& in) { in.forced = 255, in.n_dyn = 0; }, 2, 2, 2, {0, 0}, "cssolve/1"},
    {"forced 255, no dynamic bodies, replay", [](SolvePlanIn& in) { in.forced = 255, in.n_dyn = 0, in.n_kin = 2, in.n_kin_items = 3; }, 2, 2, 2, {0, 0},
     "clear cssolve/1 prefix cssolve/2"},
    {"47 levels: one workgroup", [](SolvePlanIn& in) { in.n_levels[0] = 30, in.n_levels[1] = 17; }, 0, 1, 1, {1200, 1400}, "solve:0 solve:1/1"},
    {"48 levels: chain-stationary", [](SolvePlanIn& in) { in.n_levels[0] = 30, in.n_levels[1] = 18; }, 2, 2, 2, {0, 0}, "csinit cssolve/1 csfinish"},
    {"widest 256: one workgroup", [](SolvePlanIn& in) { in.max_level_items[0] = 256; }, 0, 1, 1, {1200, 1400}, "solve:0 solve:1/1"},
    {"widest 257: chain-stationary", [](SolvePlanIn& in) { in.max_level_items[0] = 257; }, 2, 2, 2, {0, 0}, "csinit cssolve/1 csfinish"},
    {"12288 chains: 32 workgroups per phase, the limit", [](SolvePlanIn& in) { in.max_level_items[0] = 300, in.n_chains = 12288; }, 2, 2, 64, {0, 0}, "csinit cssolve/1 csfinish"},
    {"12289 chains: one workgroup too many", [](SolvePlanIn& in) { in.max_level_items[0] = 300, in.n_chains = 12289; }, 1, 1, 2, {0, 0},
     "pack:0 pack:1 fork solve:1/1@1 jrec@1 solve:0 jwait"},
    {"12289 chains, forced 255", [](SolvePlanIn& in) { in.forced = 255, in.n_chains = 12289; }, 0, 1, 1, {1200, 1400}, "solve:0 solve:1/1"},
};

static int run_table() {
    int bad = 0;
    for (const Row& r : rows) {
        SolvePlanIn in = base();
        r.change(in);
        const SolvePlan pl = solve_plan(in);
        const std::string got = steps_text(pl);
        bool ok = pl.kind == r.kind && pl.form == r.form && pl.groups == r.groups && got == r.steps;
        if (r.kind == 0 && r.form != 0)
            for (int p = 0; p < 2; ++p) ok = ok && pl.in_lds[p] == (r.lds[p] >= 0) && pl.lds_bytes[p] == (uint32_t)(r.lds[p] > 0 ? r.lds[p] : 0);
        if (!ok) {
            ++bad;
            printf("%s:\n  expected kind %u form %u groups %u lds %ld %ld steps [%s]\n  got      kind %u form %u groups %u lds %ld %ld steps [%s]\n", r.what, r.kind, r.form,
                   r.groups, r.lds[0], r.lds[1], r.steps, pl.kind, pl.form, pl.groups, pl.in_lds[0] ? (long)pl.lds_bytes[0] : -1L, pl.in_lds[1] ? (long)pl.lds_bytes[1] : -1L,
                   got.c_str());
        }
    }
    printf("solve plan table: %s (%zu rows)\n", bad ? "FAILED" : "ok", sizeof rows / sizeof rows[0]);
    return bad ? 1 : 0;
}

// ---- what the plan replaced, with its field and function names ----------------------------------------------------------------------------
namespace old {
struct Sched {
    uint32_t n_levels[2], max_level_items[2];
    int cs_feasible[2];
    size_t chain_start_size;  // chain_start.size()
    uint32_t n_kin_items;
};
struct Ctx {
    int n_cu;
};
struct ivx_world {
    Ctx* ctx;
    int mg_disabled;
    uint32_t solver_groups_forced, n_dyn;
    Sched sched;
};
static int resident, per_cu;  // the occupancy answers (function-local statics there)
static uint32_t solver_groups(const ivx_world* w) {
    if (w->mg_disabled) return 1u;
    const uint32_t fit = (uint32_t)(resident > 0 ? resident : 0) * (uint32_t)w->ctx->n_cu / 8u;
    if (fit < 2u) return 1u;
    if (w->solver_groups_forced && w->solver_groups_forced <= 16u) return w->solver_groups_forced < fit ? w->solver_groups_forced : fit;
    const uint32_t widest = w->sched.max_level_items[0] > w->sched.max_level_items[1] ? w->sched.max_level_items[0] : w->sched.max_level_items[1];
    if (widest <= 256u) return 1u;
    uint32_t g = (widest + 159u) / 160u;
    g = g < 16u ? g : 16u;
    return g < fit ? g : fit;
}
static bool solver_stationary(const ivx_world* w) {
    if (w->mg_disabled || w->solver_groups_forced == 1u || (w->solver_groups_forced >= 2u && w->solver_groups_forced <= 16u)) return false;
    for (int p = 0; p < 2; ++p)
        if (w->sched.n_levels[p] && !w->sched.cs_feasible[p]) return false;
    if (!w->sched.n_levels[0] && !w->sched.n_levels[1]) return false;
    if (per_cu < 1) return false;
    for (int p = 0; p < 2; ++p)
        if (w->sched.n_levels[p] && (((uint32_t)w->sched.chain_start_size - 1u + 31u) / 32u + PHYS_CS_WAVES - 1u) / PHYS_CS_WAVES > (uint32_t)w->ctx->n_cu / 8u) return false;
    if (w->solver_groups_forced == PHYS_SOLVER_STATIONARY) return true;
    const uint32_t widest = w->sched.max_level_items[0] > w->sched.max_level_items[1] ? w->sched.max_level_items[0] : w->sched.max_level_items[1];
    return widest > 256u || w->sched.n_levels[0] + w->sched.n_levels[1] >= 48u;
}
}  // namespace old

#define REQUIRE(cond)                                                                     \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            printf("input %zu: %s fails; steps [%s]\n", i, #cond, steps_text(pl).c_str()); \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

static int run_random(size_t n, uint64_t seed) {
    std::mt19937_64 rng(seed);
    auto pick = [&](std::initializer_list<uint32_t> v) { return v.begin()[rng() % v.size()]; };
    auto upto = [&](uint32_t hi) { return (uint32_t)(rng() % ((uint64_t)hi + 1u)); };
    size_t kinds[3] = {0, 0, 0}, replays = 0, forks = 0;
    for (size_t i = 0; i < n; ++i) {
        SolvePlanIn in{};
        in.n_contacts = rng() % 50 ? 1u + upto(50000) : 0u;
        in.n_dyn = rng() % 3 ? pick({0, 1, 63, 4096, 5119, 5120, 5121, 5972, 5973, 5974, 6000, 200000000}) : upto(8000);
        in.n_kin = upto(4);
        for (int p = 0; p < 2; ++p) {
            in.n_levels[p] = rng() % 4 ? pick({1, 2, 23, 24, 25, 46, 47, 48, 300}) : 0u;
            in.max_level_items[p] = rng() % 2 ? pick({1, 64, 160, 255, 256, 257, 320, 321, 2400, 2401, 2560, 2561, 40000}) : 1u + upto(3000);
            in.cs_feasible[p] = rng() % 5 != 0;
        }
        in.n_cu = pick({1, 8, 15, 16, 32, 64, 256, 304});
        const uint32_t chains_at_limit = in.n_cu / 8u * PHYS_CS_WAVES * 32u;
        in.n_chains = rng() % 2 ? 1u + upto(20000) : chains_at_limit + upto(2) - (chains_at_limit ? 1u : 0u);
        in.n_kin_items = in.n_kin && rng() % 2 ? 1u + upto(5) : 0u;
        in.forced = rng() % 2 ? 0u : (rng() % 4 ? upto(16) : 255u);
        in.mg_disabled = rng() % 10 == 0;
        in.mg_blocks_per_cu = (int)pick({0, 1, 1, 2, 2, 8}) - (rng() % 20 == 0 ? 1 : 0);
        in.cs_blocks_per_cu = (int)pick({0, 1, 1, 1, 2});
        in.serial = rng() % 4 == 0;
        in.tracing = rng() % 8 == 0;
        const SolvePlan pl = solve_plan(in);
        if (!in.n_contacts) {
            REQUIRE(pl.form == 0u && pl.n_steps == 0u);
            continue;
        }
        // the choice, against the transcription
        old::Ctx ctx{(int)in.n_cu};
        old::ivx_world w{&ctx, in.mg_disabled ? 1 : 0, in.forced, in.n_dyn,
                         {{in.n_levels[0], in.n_levels[1]}, {in.max_level_items[0], in.max_level_items[1]}, {in.cs_feasible[0] ? 1 : 0, in.cs_feasible[1] ? 1 : 0},
                          (size_t)in.n_chains + 1u, in.n_kin_items}};
        old::resident = in.mg_blocks_per_cu, old::per_cu = in.cs_blocks_per_cu;
        const bool replay = w.sched.n_levels[1] && w.sched.n_kin_items > 0;
        REQUIRE(pl.replay == replay);
        if (old::solver_stationary(&w)) {
            uint32_t n_groups = 0;  // (v.n_groups + p1.n_groups of launch_solve_cs: cs[p].n_tiles is (chains + 31) / 32 for a phase with levels)
            for (int p = 0; p < 2; ++p)
                if (w.sched.n_levels[p]) n_groups += ((in.n_chains + 31u) / 32u + PHYS_CS_WAVES - 1u) / PHYS_CS_WAVES;
            REQUIRE(pl.kind == 2u && pl.form == 2u && pl.groups == n_groups);
        } else {
            const uint32_t groups = old::solver_groups(&w);
            REQUIRE(pl.form == 1u && pl.groups == groups && pl.kind == (groups > 1u ? 1u : 0u));
            if (groups == 1u) {
                const size_t lds0 = (size_t)w.n_dyn * 24, lds1 = (size_t)w.n_dyn * 28;
                REQUIRE(pl.in_lds[0] == (lds0 <= 140 * 1024) && pl.lds_bytes[0] == (lds0 <= 140 * 1024 ? lds0 : 0));
                REQUIRE(pl.in_lds[1] == (lds1 <= 140 * 1024) && pl.lds_bytes[1] == (lds1 <= 140 * 1024 ? lds1 : 0));
            }
        }
        // the sequence's invariants
        REQUIRE(pl.n_steps <= MAX_STEPS);
        int fork = -1, jrec = -1, jwait = -1, pass1 = -1, pass2 = -1, prefix = -1, n_prefix = 0;
        for (int k = 0; k < (int)pl.n_steps; ++k) {
            const Step& st = pl.step[k];
            if (st.op == FORK) {
                REQUIRE(fork < 0);
                fork = k;
            }
            if (st.op == JOIN_RECORD) {
                REQUIRE(fork >= 0 && jrec < 0 && st.stream == 1u);
                jrec = k;
            }
            if (st.op == JOIN_WAIT) {
                REQUIRE(jrec >= 0 && jwait < 0 && st.stream == 0u);
                jwait = k;
            }
            if (st.stream) REQUIRE(st.stream == 1u && fork >= 0 && k > fork && (jrec < 0 || k == jrec));  // stream 1 only from the fork to its join-record
            if (st.pass == 2u) REQUIRE(pl.replay);
            const bool solve = (st.op == SOLVE && st.phase == 1u) || st.op == CS_SOLVE;
            if (solve && st.pass == 1u) {
                REQUIRE(pass1 < 0 && pass2 < 0);
                pass1 = k;
            }
            if (solve && st.pass == 2u) {
                REQUIRE(pass1 >= 0 && prefix > pass1 && pass2 < 0);
                pass2 = k;
            }
            if (solve) REQUIRE(st.pass == 1u || st.pass == 2u);
            if (st.op == KIN_PREFIX) {
                REQUIRE(pass1 >= 0 && pass2 < 0 && pl.step[pass1].stream == st.stream);
                prefix = k, ++n_prefix;
            }
            REQUIRE((st.op == SOLVE || st.op == SNAPSHOT || st.op == RESTORE) ? pl.kind != 2u : true);
            REQUIRE((st.op >= CS_INIT && st.op <= TRACE_DUMP) ? pl.kind == 2u : true);
            REQUIRE((st.op == PACK_ITEMS || st.op == FORK) ? pl.kind == 1u : true);
        }
        REQUIRE((fork >= 0) == (jrec >= 0) && (fork >= 0) == (jwait >= 0));
        REQUIRE(n_prefix == (pl.replay ? 1 : 0) && (pass2 >= 0) == pl.replay);
        REQUIRE((pass1 >= 0) == (pl.kind == 2u || in.n_levels[1] != 0u));
        ++kinds[pl.kind], replays += pl.replay, forks += fork >= 0;
    }
    printf("solve plan random: ok (%zu inputs: %zu one workgroup, %zu tile dataflow, %zu chain-stationary; %zu with a replay, %zu forked)\n", n, kinds[0], kinds[1], kinds[2],
           replays, forks);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "table")) return run_table();
    if (argc >= 3 && !strcmp(argv[1], "random")) return run_random((size_t)atoll(argv[2]), argc >= 4 ? (uint64_t)atoll(argv[3]) : 1u);
    fprintf(stderr, "usage: solve_plan_check table | random N [seed]\n");
    return 2;
}
