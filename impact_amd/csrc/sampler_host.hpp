// The sampler's host-side decisions, free of HIP calls: what a sample stage launches (sample_plan) and the transitions of sample-ahead's
// state (ivx_sampler::ahead, ivx_internal.hpp). sdf_sample.hip executes the plan; ivx_sampler_plan exports it to tests that run without a GPU.
#pragma once
#include "ivx_internal.hpp"

namespace ivx_smp {

constexpr int SUPER = 4;  // super-blocks of 4 x 4 x 4 chunks (k_sdf_super)
constexpr uint32_t SUPER_MAX_WORDS = 64;  // programs of up to 2048 nodes get their super-block tables inside the pre-pass (k_sdf_super beyond)
constexpr uint32_t MAX_LDS_BYTES = 150u * 1024u;  // the general class's forward stack: at most 9 blocks of 16 KiB fit the 160 KiB LDS

struct SamplePlanIn {
    uint32_t n_nodes, stack_size;
    bool noise, resident;  // (`resident`: the step path, under the grid's resident program — the remembered lengths and sample-ahead are that program's)
    bool eval_len_valid;
    uint32_t eval_len[3];
    uint32_t n_chunks, cc[3], n_cu;
    bool eval_dirty;  // IVX_SCRATCH_EVAL of the grid's scratch_dirty: the list counters are not known to be zero
    uint32_t preset_groups;
    bool ahead_on, ahead_pending;
};
struct EvalLaunch {
    uint8_t mode;  // k_sdf_eval<mode>: 2 the one-level class, 1 the two-level class (or both), 0 the general class
    bool noise;    // ... k_sdf_eval<0, true>
    uint32_t grid, lds_bytes, scratch_off;
    uint8_t list;         // which of the three counters and lists it walks
    bool long_count;      // ... with the long / short split of the first list (counter 3)
    bool first;           // ... behind counter and list 1, as first_count / first_list (the merged launch)
    bool commits_shadow;  // the stage's first launch when its pre-pass ran ahead: commits the parked records and hosts the presets
};
struct SuperGrid {
    uint32_t words;       // 32-node words of the program's far bits
    uint32_t sx, sy, sz;  // super-blocks along the axes
    uint32_t blocks() const { return sx * sy * sz; }
};
inline SuperGrid super_grid(uint32_t n_nodes, const uint32_t cc[3]) {
    const uint32_t words = (n_nodes + 31u) / 32u;
    return SuperGrid{words > 0u ? words : 1u, (cc[0] + SUPER - 1) / SUPER, (cc[1] + SUPER - 1) / SUPER, (cc[2] + SUPER - 1) / SUPER};
}
struct SamplePlan {
    SuperGrid sb;
    bool fused_super;
    bool consume, cancel;  // the pre-pass that ran ahead is this stage's / is waited for and dropped
    // scratch groups preset by k_sdf_super, by the stage's own pre-pass, by the first evaluator launch (whichever is the stage's first kernel)
    uint32_t super_presets, prepass_presets, first_presets;
    bool clear_counters;  // the eight list counters are cleared by a memset ahead of the stage
    bool ahead_wanted;    // the NEXT stage's pre-pass may run ahead
    uint32_t n_launches;
    EvalLaunch launch[3];  // in launch order: one-level, two-level or merged, general
};

inline SamplePlan sample_plan(const SamplePlanIn& in) {
    SamplePlan pl{};
    // Programs of up to SUPER_MAX_WORDS * 32 nodes get their super-block tables inside the pre-pass (no launch of their own); the
    // pre-pass is then the call's first kernel and hosts the presets of the later stages' scratch words. The sampler's own list
    // counters are zero already when the derive sweep of the step before rolled them over (role_preset), else cleared here.
    pl.sb = super_grid(in.n_nodes, in.cc);
    pl.fused_super = pl.sb.words <= SUPER_MAX_WORDS;
    // One evaluator launch per LDS class (see k_sdf_prepass); a class the program cannot reach is not launched, nor one whose list the last step
    // under this program found empty (the lists are a function of the program and the grid). Two launches one after the other each pay
    // their own ramp and tail: when both of the first two classes have work and one of them is too short to fill the chip a few times
    // over, the two-level kernel takes both lists in one launch (the one-level programs run there as well, five workgroups per CU).
    // (`resident`: the remembered lengths are the RESIDENT program's; ivx_sdf_sample runs any program through this plan and must launch
    // every class that program can reach)
    const uint32_t* len = in.eval_len;
    const bool noise = in.noise, known = in.resident && in.eval_len_valid;
    const uint32_t fill = 4u * 5u * in.n_cu;
    // (a program with a noise node lists every chunk for the general class and runs in k_sdf_eval<0, true> alone)
    const bool merge01 = !noise && known && len[0] && len[1] && (len[0] < fill || len[1] < fill);
    const bool launch2 = !noise && !merge01 && !(known && len[0] == 0u);               // k_sdf_eval<2>: the one-level class
    const bool launch1 = !noise && (merge01 || !(known && len[1] == 0u));              // k_sdf_eval<1>: the two-level class (or both)
    const bool launch0 = (noise || in.stack_size >= 3u) && !(known && len[2] == 0u);  // k_sdf_eval<0>: the general class
    // Sample-ahead: this stage's pre-pass may have run already, behind the evaluator of the step before; the stage then starts at its first
    // evaluator launch, which commits the parked records and hosts the presets. Only with an evaluator launch to host them.
    const bool ahead_fits = in.resident && pl.fused_super && (launch0 || launch1 || launch2);
    pl.consume = in.resident && in.ahead_pending && ahead_fits;
    pl.cancel = in.resident && in.ahead_pending && !ahead_fits;
    pl.ahead_wanted = in.ahead_on && ahead_fits;
    const uint32_t host_presets = in.preset_groups & ~IVX_SCRATCH_EVAL;  // what the stage's first kernel presets for the later stages
    if (pl.consume) pl.first_presets = host_presets;
    else {
        pl.super_presets = pl.fused_super ? 0u : in.preset_groups;
        pl.prepass_presets = pl.fused_super ? host_presets : 0u;
        pl.clear_counters = in.eval_dirty && !(pl.super_presets & IVX_SCRATCH_EVAL);
        if (!in.eval_dirty) pl.super_presets &= ~IVX_SCRATCH_EVAL;
    }
    // (grids: a whole number of list entries per workgroup once the lists' lengths are known — a launch's last wave of workgroups costs as
    // much as a full one, see ivx_launch_derive)
    auto fit = [&](uint32_t n) {
        const uint32_t cap = in.n_chunks < 16384u ? in.n_chunks : 16384u;  // (measured on 512^3: 4 096 and 32 768 are both slower on the all-surface grid)
        if (!known || n == 0u) return cap;
        const uint32_t each = (n + cap - 1u) / cap;
        return (n + each - 1u) / each;
    };
    auto add = [&](uint8_t mode, uint32_t n, uint32_t scratch_off, uint32_t lds_words, uint8_t list, bool long_count, bool first) {
        pl.launch[pl.n_launches] = EvalLaunch{mode, mode == 0u && noise, fit(n), lds_words * (uint32_t)sizeof(float), scratch_off, list, long_count, first,
                                              pl.consume && pl.n_launches == 0u};
        ++pl.n_launches;
    };
    // one level + 64 words of scratch: 16 640 bytes = 13 LDS granules, eight workgroups per CU (the waves a SIMD holds)
    if (launch2) add(2, len[0], IVX_CHUNK_VOXELS, IVX_CHUNK_VOXELS + 64u, 0, true, false);
    // two levels, the second one 15 rows long + 64 words of scratch: 32 000 bytes = 25 LDS granules, five workgroups per CU
    if (launch1) {
        const uint32_t scratch_off = IVX_CHUNK_VOXELS + 15u * 256u;
        if (merge01) add(1, len[0] + len[1], scratch_off, scratch_off + 64u, 0, true, true);
        else add(1, len[1], scratch_off, scratch_off + 64u, 1, false, false);
    }
    // (the scratch words are the last sixteen of the stack: rows 15 of the last level's threads 240..255, dead when they are used
    // — the votes — and never used as published test voxels, which only the trimmed launch has)
    if (launch0) {
        const uint32_t lv = in.stack_size ? in.stack_size : 1u;
        add(0, len[2], lv * IVX_CHUNK_VOXELS - 16u, lv * IVX_CHUNK_VOXELS, 2, false, false);
    }
    return pl;
}

// ---- sample-ahead's state: every change of ivx_sampler::ahead.state is one of these -----------------------------------------------------
// end of a sample stage: the next stage's pre-pass may run ahead (a pre-pass still pending — a stage that was not the resident program's — stays)
inline void ahead_want(ivx_sampler& s, bool wanted) {
    if (s.ahead.state != AHEAD_PENDING) s.ahead.state = wanted ? AHEAD_WANTED : AHEAD_IDLE;
}
// the step acts on the wish: true = launch the pre-pass now. The wish is as old as the last sample stage; whatever has changed since
// (sample-ahead turned off, another program) is looked at again here.
inline bool ahead_take_wish(ivx_sampler& s) {
    if (s.ahead.state != AHEAD_WANTED) return false;
    s.ahead.state = AHEAD_IDLE;
    return s.ahead.on && s.prog.n > 0u && (s.prog.n + 31u) / 32u <= SUPER_MAX_WORDS;
}
inline void ahead_launched(ivx_sampler& s) { s.ahead.state = AHEAD_PENDING; }
// the pending pre-pass becomes this stage's: the sets trade places (`eval_dirty`: the set that steps back has live counters unless a
// derive sweep rolled them over)
inline void ahead_consume(ivx_sampler& s, bool eval_dirty) {
    s.cur ^= 1;
    s.ahead.other_dirty = eval_dirty ? 1 : 0;
    s.ahead.state = AHEAD_IDLE;
}
// true: a pre-pass is under way — the caller waits for it; what it wrote into the other set is dropped
inline bool ahead_cancel(ivx_sampler& s) {
    const bool pending = s.ahead.state == AHEAD_PENDING;
    s.ahead.state = AHEAD_IDLE;
    if (pending) s.ahead.other_dirty = 1;
    return pending;
}

}  // namespace ivx_smp
