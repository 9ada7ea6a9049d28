// The stage clock of a step (ivx_grid::timing): which timed slots of the calls since the last collect are measured by clock stamps and which by
// event records, and how they become ivx_step_result::stage_ms; what a slot is and how it is measured is told where the clock is driven
// (step_api.hip). Bookkeeping only, plain data that starts as zero bytes: event records and the two allocations enter through `Rt` — int
// make_ticks(clock), int make_events(clock), int record(void* event), bool elapsed(void* from, void* to, float* ms) —, so it also compiles, and is
// checked against what it replaced, without the HIP runtime (tools/stage_clock_check.cpp, tests/test_stage_clock_cpu.py).
#pragma once
#include <cstdint>

#include "../../include/impact_voxel_hip.h"

#define IVX_TICK_WORDS 32  // clock words of a grid between two collects; a call takes at most a word per slot and one more

// What begin() asks of the call being enqueued: `part` 3 = a whole call (ivx_voxel_step_enqueue_part: 1, 2 = its halves) | IVX_STAGE_TIMING_EVENTS=1
// | the call ends in the slab's record, not in the gather | the fused assign reaches the grid | stand-alone per-chunk kernels, which carry no
// stamp, run ahead of k_step_post1 | the launches are recorded into a batch of several objects
struct ivx_stage_call {
    uint32_t part;
    bool force_events, slab_record, assign_fits, standalone_first, recording;
};

struct ivx_stage_timing {
    uint32_t off;     // slots that are NOT timed (ivx_grid_set_stage_timing; zero-initialised: every slot is timed)
    int events_only;  // this grid's timed slots always take event records (a slab of the slab protocol, ivx_slab_create)
    void* ev[2 * IVX_N_TIMED_STAGES];  // events: start/stop per slot (hipEvent_t, made on first use: ev_ready)
    int ev_ready;
    int8_t ev_start_ref[IVX_N_TIMED_STAGES];  // the event a slot's duration starts from (the stop of the slot before when adjacent)
    uint32_t timed_mask;                      // slots whose events were recorded since the last collect
    // stamps: words are handed out in stream order since the last collect
    unsigned long long* tick_dev;   // [IVX_TICK_WORDS] device words the launches stamp; k_step_gather copies them out and zeroes them
    unsigned long long* tick_host;  // [IVX_TICK_WORDS] host-mapped copy, written by the gather ahead of the doorbell
    unsigned long long* tick_host_dev;
    unsigned long long* tick_next;  // the word the next stamping launch on this grid writes (take), or null
    uint32_t tick_used;             // words handed out since the last collect
    uint32_t stamp_mask;            // slots whose words were armed since the last collect (their times come from tick_host)
    int8_t tick_start_ref[IVX_N_TIMED_STAGES], tick_end_ref[IVX_N_TIMED_STAGES];  // word indices of a stamped slot's two ends (-1: the slot had no launch)
    unsigned long long tick_last[2 * IVX_N_TIMED_STAGES];  // the last collect's raw stamps, start then end per slot (ivx_debug_stage_ticks)
    // the call being enqueued: its timed slots | stamps or events, for the whole call | events: the stop of the slot enqueued just before (-1: none),
    // where the next slot starts | stamps: the word the open slot starts at, and whether the slot armed it itself (else it is the closing word of
    // the slot before, still pending)
    uint32_t call_mask;
    bool call_stamps, slot_fresh;
    int8_t last_stop, slot_word;

    void arm() { tick_host[tick_used] = 0ull, tick_next = tick_dev + tick_used++; }
    // stamps or events for a whole call: stamps on the step's fused path while the words last
    template <class Rt>
    int begin(Rt& rt, const ivx_stage_call& c) {
        call_mask = ~off, last_stop = slot_word = -1, slot_fresh = false;
        call_stamps = call_mask != 0u && !c.force_events && !events_only && c.part == 3u && !c.slab_record && c.assign_fits && !c.standalone_first && !c.recording &&
                      tick_used + IVX_N_TIMED_STAGES + 1u <= IVX_TICK_WORDS;
        return call_stamps ? rt.make_ticks(*this) : call_mask != 0u ? rt.make_events(*this) : 0;
    }
    template <class Rt>
    int open(Rt& rt, int i) {
        if (!((call_mask >> i) & 1u)) last_stop = -1;
        else if (call_stamps) {
            slot_fresh = tick_next == nullptr;
            if (slot_fresh) arm();
            slot_word = (int8_t)(tick_next - tick_dev);
        } else if (last_stop >= 0) ev_start_ref[i] = last_stop;
        else {
            if (int rc = rt.record(ev[2 * i])) return rc;
            ev_start_ref[i] = (int8_t)(2 * i);
        }
        return 0;
    }
    // (stamps: a word that nobody took means the slot launched nothing — it reports 0, and a word it armed itself is given back)
    template <class Rt>
    int close(Rt& rt, int i) {
        if (!((call_mask >> i) & 1u)) return 0;
        if (!call_stamps) {
            if (int rc = rt.record(ev[2 * i + 1])) return rc;
            last_stop = (int8_t)(2 * i + 1);
            timed_mask |= 1u << i, stamp_mask &= ~(1u << i);
            return 0;
        }
        stamp_mask |= 1u << i, timed_mask &= ~(1u << i);
        if (tick_next == tick_dev + slot_word) {
            tick_start_ref[i] = tick_end_ref[i] = -1;
            if (slot_fresh) tick_next = nullptr, --tick_used;
        } else {
            tick_start_ref[i] = slot_word, tick_end_ref[i] = (int8_t)tick_used;
            arm();
        }
        return 0;
    }
    // The clock word the launch being made stamps: the pending one, handed out once. A launch that is only recorded into a batch of several
    // objects (its twin does not stamp) leaves the word to the next launch made directly.
    unsigned long long* take(bool recording) {
        unsigned long long* t = recording ? nullptr : tick_next;
        if (t) tick_next = nullptr;
        return t;
    }
    // k_step_gather: the words of the stamped slots since the last collect go out with the results; a word still pending is that launch's own
    void hand_to_gather(unsigned long long** dev, unsigned long long** host_dev, uint32_t* n, unsigned long long** own) {
        if (!tick_used) return;
        *dev = tick_dev, *host_dev = tick_host_dev, *n = tick_used, *own = tick_next;
        tick_next = nullptr;
    }
    // slot i of the calls since the last collect in ms (0: not timed, or without a launch), the raw stamps kept; stamps run start to start, in
    // ticks of the device's constant-rate clock
    template <class Rt>
    float read(Rt& rt, int i, double clock_khz) {
        float ms = 0.0f;
        tick_last[2 * i] = tick_last[2 * i + 1] = 0ull;
        if ((stamp_mask >> i) & 1u) {
            if (tick_start_ref[i] >= 0 && tick_end_ref[i] >= 0) {
                const unsigned long long t0 = tick_host[tick_start_ref[i]], t1 = tick_host[tick_end_ref[i]];
                tick_last[2 * i] = t0, tick_last[2 * i + 1] = t1;
                if (t0 != 0ull && t1 > t0) ms = (float)((double)(t1 - t0) / clock_khz);
            }
        } else if (((timed_mask >> i) & 1u) && !rt.elapsed(ev[ev_start_ref[i]], ev[2 * i + 1], &ms)) ms = 0.0f;
        return ms;
    }
    void reset() { timed_mask = stamp_mask = tick_used = 0u, tick_next = nullptr; }  // (behind a collect)
};
