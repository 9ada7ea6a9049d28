// The step of the C ABI: ivx_voxel_step_enqueue / _collect and what rides on them — the slab protocol's remesh phase, a slab's face pairs and
// step record, ivx_voxel_step_many — and the driving of the stage clock (stage_clock.hpp). Host-side orchestration only, no kernel of its own;
// what this unit and the other host units ask of each other is declared in ivx_host.hpp.
#include "ivx_host.hpp"

extern "C" {

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
static const bool g_stage_timing_events = getenv("IVX_STAGE_TIMING_EVENTS") && atoi(getenv("IVX_STAGE_TIMING_EVENTS")) == 1;
// the HIP runtime behind the stage clock: its two allocations, event records on the context's stream, the time between two events
namespace {
struct StageRt {
    hipStream_t s;
    int make_events(ivx_stage_timing& t) {
        if (t.ev_ready) return IVX_OK;
        for (int i = 0; i < 2 * IVX_N_TIMED_STAGES; ++i) IVX_HIP_CHECK(hipEventCreate(reinterpret_cast<hipEvent_t*>(&t.ev[i])));
        t.ev_ready = 1;
        return IVX_OK;
    }
    int make_ticks(ivx_stage_timing& t) {
        if (!t.tick_dev) {
            IVX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&t.tick_dev), IVX_TICK_WORDS * sizeof(unsigned long long)));
            IVX_HIP_CHECK(hipMemset(t.tick_dev, 0, IVX_TICK_WORDS * sizeof(unsigned long long)));
        }
        if (!t.tick_host) {
            IVX_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&t.tick_host), IVX_TICK_WORDS * sizeof(unsigned long long), hipHostMallocMapped));
            memset(t.tick_host, 0, IVX_TICK_WORDS * sizeof(unsigned long long));
            IVX_HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&t.tick_host_dev), t.tick_host, 0));
        }
        return IVX_OK;
    }
    int record(void* e) {
        IVX_HIP_CHECK(ivx_event_record(static_cast<hipEvent_t>(e), s));
        return IVX_OK;
    }
    bool elapsed(void* from, void* to, float* ms) { return hipEventElapsedTime(ms, static_cast<hipEvent_t>(from), static_cast<hipEvent_t>(to)) == hipSuccess; }
};
}  // namespace
// (ivx_grid_destroy: the stage stamps' words — two small allocations of their own, made on first use — and the events)
extern "C++" void stage_clock_free(ivx_grid* g) {
    ivx_stage_timing& t = g->timing;
    if (t.tick_dev) (void)hipFree(t.tick_dev);
    if (t.tick_host) (void)hipHostFree(t.tick_host);
    if (t.ev_ready)
        for (void* e : t.ev) (void)hipEventDestroy(static_cast<hipEvent_t>(e));
}
// the grid's host-mapped result block (IVX_RB_*, ivx_internal.hpp), made on first use unless the grid came with a part of a shared one
static int ensure_result_block(ivx_grid* g) {
    if (g->result_host) return IVX_OK;
    IVX_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&g->result_host), IVX_RB_WORDS * sizeof(uint32_t), hipHostMallocMapped));
    memset(g->result_host, 0, IVX_RB_WORDS * sizeof(uint32_t));
    IVX_HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&g->result_host_dev), g->result_host, 0));
    return IVX_OK;
}
static int ensure_pairs(ivx_grid* g) {
    if (g->pairs_dev) return IVX_OK;
    IVX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&g->pairs_dev), sizeof(uint32_t) * (size_t)IVX_PAIRS_WORDS));
    IVX_HIP_CHECK(ivx_memset_async(g->pairs_dev, 0, sizeof(uint32_t) * IVX_PAIRS_HEAD_WORDS, g->ctx->stream));
    return IVX_OK;
}
// `slab_nbr_ids` / `slab_record`: the slab protocol's remesh phase (ivx_slab_remesh_enqueue) — the pass over the neighbour's face ids and the
// slab's record ride in the phase's own launches instead of taking two more
// `part` (slab protocol, ivx_voxel_step_enqueue_part): bit 0 = the call's sample and derive sweeps, bit 1 = everything behind them; the two
// halves of ONE call enqueued apart, so that the slab's face planes can be packed and sent between them.
static int step_enqueue(ivx_grid* g, uint32_t stages, const uint16_t* slab_nbr_ids, void* slab_record, uint32_t part = 3u) {
    IVX_REQUIRE(g, IVX_ERR_INVALID, "ivx_voxel_step_enqueue: null grid");
    const bool front = (part & 1u) != 0u, back = (part & 2u) != 0u;
    ivx_many_other_context other_(g->ctx);
    IVX_REQUIRE(!(stages & IVX_STAGE_SAMPLE) || g->smp.prog.n > 0, IVX_ERR_STATE, "ivx_voxel_step: no SDF program resident (ivx_grid_set_sdf_program)");
    IVX_REQUIRE(!(stages & IVX_STAGE_INERTIA) || g->has_dens, IVX_ERR_STATE, "ivx_voxel_step: no densities resident (ivx_grid_set_densities)");
    hipStream_t s = g->ctx->stream;
    const bool ahead_unordered_ok = g->pending_stages == 0;  // (sample-ahead: whatever was enqueued before has been collected)
    // stages enqueued after a record change the step's results: the block the record role wrote is stale (this call sets the flag again
    // further down when it carries the slab record itself)
    g->results_in_block = 0;
    int rc;
    if ((rc = ensure_result_block(g))) return rc;
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
    // stamps or events, for the whole call (see above)
    ivx_stage_timing& clk = g->timing;
    StageRt rt{s};
    if ((rc = clk.begin(rt, ivx_stage_call{part, g_stage_timing_events, slab_record != nullptr, ivx_step_assign_fits(g), standalone_first, ivx_many_recording()}))) return rc;
    if (front && (stages & IVX_STAGE_SAMPLE)) {
        if ((rc = clk.open(rt, 0))) return rc;
        const auto& prog = g->smp.prog;
        if ((rc = ivx_launch_sdf_sample(g, prog.nodes, prog.n, prog.stack, prog.shape, prog.center, prog.type, preset_in_sample, true, prog.noise != 0, ahead_unordered_ok)))
            return rc;
        if ((rc = clk.close(rt, 0))) return rc;
        g->smp.lens.pending = 1;  // (the list lengths reach the result block once a derive sweep has rolled the counters over)
        ivx_voxels_replaced(g);
    }
    if (front && (stages & IVX_STAGE_DERIVE)) {
        if ((rc = clk.open(rt, 1))) return rc;
        if ((rc = ivx_launch_derive(g, fused_parts, preset_in_derive))) return rc;
        if ((rc = clk.close(rt, 1))) return rc;
        if (g->smp.lens.pending == 1) g->smp.lens.pending = 2;
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
        if ((rc = clk.open(rt, 2))) return rc;
        if ((rc = ivx_launch_step_post1(g, post))) return rc;
        if ((rc = clk.close(rt, 2))) return rc;
        if ((rc = clk.open(rt, 3))) return rc;
        if (slab_record) {
            if ((rc = ensure_pairs(g))) return rc;
            if (slab_nbr_ids && !g->pairs_zeroed) IVX_HIP_CHECK(ivx_memset_async(g->pairs_dev, 0, IVX_PAIRS_HEAD_WORDS * sizeof(uint32_t), s));
            g->pairs_zeroed = 0;
        }
        if ((rc = ivx_launch_step_post2(g, post, slab_nbr_ids))) return rc;
        if ((rc = clk.close(rt, 3))) return rc;
        // no host round trip for the mesh sizes: the emit pass writes into the buffers of the previous step and skips what
        // does not fit; ivx_voxel_step_collect grows the buffers and repeats the pass in that (rare) case
        if (post & (IVX_STAGE_REGIONS | IVX_STAGE_REMESH)) {
            if ((rc = clk.open(rt, 4))) return rc;
            if (fused_assign) {
                if ((rc = ivx_launch_step_emit(g, post, (post & IVX_STAGE_REGIONS) != 0, slab_record, slab_nbr_ids != nullptr))) return rc;
                if (slab_record) g->results_in_block = 1;
            } else {  // more than 524 288 chunks: the region resolve takes its stand-alone path
                if ((post & IVX_STAGE_REMESH) && (rc = ivx_launch_step_emit(g, IVX_STAGE_REMESH))) return rc;
                if ((post & IVX_STAGE_REGIONS) && (rc = ivx_launch_ccl_resolve(g))) return rc;
            }
            if ((rc = clk.close(rt, 4))) return rc;
        }
        // (sample-ahead: the next sample stage's pre-pass goes behind the step's last big launch, beside the small ones that follow)
        if (!ahead_unordered_ok && (rc = ivx_sampler_launch_ahead(g, true))) return rc;
        if ((post & IVX_STAGE_REGIONS) && fused_assign) {
            if ((rc = clk.open(rt, 5))) return rc;
            if ((rc = ivx_launch_step_assign(g, (post & IVX_STAGE_REMESH) != 0))) return rc;
            if ((rc = clk.close(rt, 5))) return rc;
        }
        if (post & IVX_STAGE_REMESH) {
            g->mesh_valid = 0;
            g->scratch_dirty |= IVX_SCRATCH_SN;
        }
        if (post & IVX_STAGE_REGIONS) g->scratch_dirty |= IVX_SCRATCH_REGIONS;
    }
    if (back && (rc = ivx_sampler_launch_ahead(g, !ahead_unordered_ok))) return rc;  // (a call without the stages behind the derive sweep)
    g->pending_stages |= stages;
    return IVX_OK;
}

int ivx_voxel_step_enqueue(ivx_grid* g, uint32_t stages) { return step_enqueue(g, stages, nullptr, nullptr); }
// ... without event records around the stage slots, whatever ivx_grid_set_stage_timing has asked for: for callers whose stage times nobody reads,
// and for recorded steps — an event is a stream operation of its own and would end the merging after every object
extern "C++" int step_enqueue_untimed(ivx_grid* g, uint32_t stages) {
    const uint32_t keep = g->timing.off;
    g->timing.off = 0xFFFFFFFFu;
    const int rc = step_enqueue(g, stages, nullptr, nullptr);
    g->timing.off = keep;
    return rc;
}
// (slab_comm.cpp) one call's launches in two parts: 1 = its sample and derive sweeps, 2 = what follows them
extern "C++" int ivx_voxel_step_enqueue_part(ivx_grid* g, uint32_t stages, uint32_t part) { return step_enqueue(g, stages, nullptr, nullptr, part); }

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

int ivx_grid_set_stage_timing(ivx_grid* g, uint32_t slot_mask) {
    IVX_REQUIRE(g, IVX_ERR_INVALID, "ivx_grid_set_stage_timing: null grid");
    g->timing.off = ~slot_mask;
    return IVX_OK;
}

// Developer aid: the raw clock stamps behind the last collected step's stage_ms, start then end per slot (0: the slot was not stamped — not
// timed, without a launch, or timed by events), and the clock's rate in kHz.
int ivx_debug_stage_ticks(ivx_grid* g, unsigned long long ticks[2 * IVX_N_TIMED_STAGES], double* clock_khz) {
    IVX_REQUIRE(g && ticks, IVX_ERR_INVALID, "ivx_debug_stage_ticks: null argument");
    memcpy(ticks, g->timing.tick_last, sizeof(g->timing.tick_last));
    if (clock_khz) *clock_khz = g->ctx->wall_clock_khz;
    return IVX_OK;
}

// How long ivx_voxel_step_collect polls the doorbell before it falls back to hipStreamSynchronize (IVX_COLLECT_SPIN_US, default 2000;
// 0 = never poll).
static uint64_t collect_spin_ns() {
    static const long us = getenv("IVX_COLLECT_SPIN_US") ? strtol(getenv("IVX_COLLECT_SPIN_US"), nullptr, 10) : 2000;
    return (uint64_t)(us < 0 ? 0 : us) * 1000ull;
}

// the launch half of ivx_voxel_step_collect: the gather of the step's results (and whatever rides on it) goes on the stream — or into the
// batch being recorded —, the wait is left to the collect
extern "C++" int ivx_step_collect_launch(ivx_grid* g) {
    if (g->results_in_block || g->gather_launched) return IVX_OK;
    if (int rc_b = ensure_result_block(g)) return rc_b;
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
    if (int rc_b = ensure_result_block(g)) return rc_b;
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
        // the doorbell word the gather kernel writes last: polled for a bounded time, then the stream is waited for
        bool rung = false;
        if (int rc = doorbell_wait(g->result_host + IVX_RB_BELL, g->result_seq, collect_spin_ns(), s, &rung)) return rc;
        // the stream is empty and the doorbell has not rung: the gather never reached the stream (a flush of recorded launches failed and
        // dropped it, many.hpp) — what the block holds is an earlier step's
        if (!rung) {
            const int dropped = ivx_many_error(g->ctx, true);
            g->pending_stages = 0;
            ivx_set_error("ivx_voxel_step_collect: the step's results never arrived (%s)", dropped ? "a flush of recorded launches failed" : "the gather did not run");
            return IVX_ERR_HIP;
        }
    } else if (hipStreamQuery(s) != hipSuccess) {
        IVX_HIP_CHECK(ivx_stream_sync(s));
    }
    ivx_stage_timing& clk = g->timing;
    if (have_results && clk.stamp_mask && clk.tick_dev) {
        // (stamped slots of a step that ended in ivx_step_record_enqueue instead of the gather — the slab protocol driven from outside the
        // library: the stream has been waited for, the words are fetched and cleared here)
        IVX_HIP_CHECK(ivx_memcpy_sync(clk.tick_host, clk.tick_dev, IVX_TICK_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        IVX_HIP_CHECK(hipMemset(clk.tick_dev, 0, IVX_TICK_WORDS * sizeof(unsigned long long)));
    }
    const uint32_t* sc = g->result_host;
    if (sc[IVX_RB_ACTIVE]) g->last_active = sc[IVX_RB_ACTIVE];
    auto& lens = g->smp.lens;
    if (lens.pending == 2 && ivx_eval_count(g)) {  // a sample stage and a derive sweep behind it have run under the resident program
        for (int c = 0; c < 3; ++c) lens.len[c] = sc[IVX_RB_EVAL_LEN + c];
        lens.valid = 1;
    }
    lens.pending = 0;
    if (stages & IVX_STAGE_REGIONS) {
        IVX_REQUIRE((sc[IVX_RB_FLAGS] & IVX_RB_FLAG_LOCAL_REGIONS) == 0, IVX_ERR_CAPACITY, "ivx_voxel_step: a chunk has more than 254 local regions");
        IVX_REQUIRE((sc[IVX_RB_FLAGS] & IVX_RB_FLAG_MERGE_GAVE_UP) == 0, IVX_ERR_HIP, "ivx_voxel_step: the region merge gave up waiting for the numbering of the multi-region chunks (k_step_post2)");
        g->region_count = sc[IVX_RB_REGION_TOTAL];
        g->regions_valid = 1;
        out->region_count = sc[IVX_RB_REGION_TOTAL];
    }
    if (stages & IVX_STAGE_OCCUPIED) {
        ivx_occupied_from_raw(g, sc + IVX_RB_OCCUPIED, out->occupied);
        memcpy(g->occ_ref, out->occupied, sizeof(g->occ_ref));
        g->occ_ref_valid = 1;
    }
    if (stages & IVX_STAGE_REMESH) {
        const uint32_t totals[3] = {sc[IVX_RB_MESH_TOTALS], sc[IVX_RB_MESH_TOTALS + 1], sc[IVX_RB_MESH_TOTALS + 2]};
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
        memcpy(out->moments.m64, sc + IVX_RB_MOMENTS, 10 * sizeof(double));
        for (int i = 0; i < 10; ++i) out->moments.m32[i] = (float)out->moments.m64[i];
    }
    out->mesh = g->mesh_counts;
    StageRt rt{s};
    for (int i = 0; i < IVX_N_TIMED_STAGES; ++i) out->stage_ms[i] = clk.read(rt, i, g->ctx->wall_clock_khz);
    g->pending_stages = 0;
    clk.reset();
    return IVX_OK;
}

int ivx_voxel_step(ivx_grid* g, uint32_t stages, ivx_step_result* out) {
    IVX_REQUIRE(g && out, IVX_ERR_INVALID, "ivx_voxel_step: null argument");
    int rc = ivx_voxel_step_enqueue(g, stages);
    if (rc) return rc;
    return ivx_voxel_step_collect(g, out);
}

int ivx_region_face_pairs_enqueue(ivx_grid* g, int side, const void* neighbour_face_labels) {
    IVX_REQUIRE(g && neighbour_face_labels && (side == 0 || side == 1), IVX_ERR_INVALID, "ivx_region_face_pairs_enqueue: bad argument");
    int rc = ensure_pairs(g);
    if (rc) return rc;
    rc = ivx_launch_face_pairs(g, side, static_cast<const uint16_t*>(neighbour_face_labels), g->pairs_dev, g->pairs_dev + IVX_PAIRS_HEAD_WORDS, IVX_MAX_FACE_PAIRS,
                               g->pairs_dev + 4);
    if (rc) return rc;
    g->pairs_enqueued = 1;
    return IVX_OK;
}

size_t ivx_step_record_words(void) { return IVX_RECORD_HEAD_WORDS + 2 * (size_t)IVX_MAX_FACE_PAIRS; }

int ivx_step_record_enqueue(ivx_grid* g, void* device_record) {
    IVX_REQUIRE(g && device_record, IVX_ERR_INVALID, "ivx_step_record_enqueue: null argument");
    int rc = ensure_pairs(g);
    if (rc) return rc;
    // (no face-pair pass since the last record: the record lists none — a null count, not a fill of the counter)
    rc = ivx_launch_step_record(g, g->pairs_enqueued ? g->pairs_dev : nullptr, g->pairs_dev + IVX_PAIRS_HEAD_WORDS, IVX_MAX_FACE_PAIRS, device_record, g->result_host_dev != nullptr);
    if (!rc && g->result_host_dev) g->results_in_block = 1;
    g->pairs_enqueued = 0;
    return rc;
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

}  // extern "C"
