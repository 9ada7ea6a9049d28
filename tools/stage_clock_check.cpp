// The stage clock's bookkeeping (impact_amd/csrc/stage_clock.hpp) checked on the host, without the HIP runtime:
//   stage_clock_check scenarios        scenarios written out by hand (tests/test_stage_clock_cpu.py runs this)
//   stage_clock_check random N [seed]  N random sequences through the clock and through a transcription of what it replaced — the T0 / T1
//                                      macros of step_enqueue, ivx_take_tick, the gather's hand-over and the tail of the collect as they stood
//                                      before the step became a unit of its own — compared after every operation
// Build: g++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/stage_clock_check.cpp -o stage_clock_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../impact_amd/csrc/stage_clock.hpp"

typedef unsigned long long ull;
static const int N = IVX_N_TIMED_STAGES;
static const double KHZ = 100000.0;  // 100 ticks = 1 us

// Events are their indices; a record notes the index and the time; the two allocations are noted as -1 (words) and -2 (events).
struct FakeRt {
    std::vector<int> log;
    int ids[2 * N];
    ull when[2 * N] = {}, now = 0;
    ull dev[IVX_TICK_WORDS] = {}, host[IVX_TICK_WORDS] = {};
    int make_ticks(ivx_stage_timing& t) {
        log.push_back(-1);
        t.tick_dev = dev, t.tick_host = t.tick_host_dev = host;
        return 0;
    }
    int make_events(ivx_stage_timing& t) {
        log.push_back(-2);
        for (int i = 0; i < 2 * N; ++i) ids[i] = i, t.ev[i] = &ids[i];
        t.ev_ready = 1;
        return 0;
    }
    int record(void* e) {
        const int i = *static_cast<int*>(e);
        log.push_back(i), when[i] = now;
        return 0;
    }
    bool elapsed(void* from, void* to, float* ms) {
        *ms = (float)((double)(when[*static_cast<int*>(to)] - when[*static_cast<int*>(from)]) / KHZ);
        return true;
    }
};

// ---- what the clock replaced, with its field and local names --------------------------------------------------------------------------
struct Old {
    uint32_t stage_timing_off = 0;
    int stage_events_only = 0;
    int ev[2 * N];
    const int* ev_start_ref[N] = {};
    uint32_t timed_mask = 0, stamp_mask = 0;
    ull dev_[IVX_TICK_WORDS] = {}, host_[IVX_TICK_WORDS] = {};
    ull *tick_dev = dev_, *tick_host = host_, *tick_next = nullptr;
    uint32_t tick_used = 0;
    int8_t tick_start_ref[N] = {}, tick_end_ref[N] = {};
    ull tick_last[2 * N] = {};
    // record keeping of the transcription
    std::vector<int> log;
    ull when[2 * N] = {}, now = 0;
    // the locals of step_enqueue
    uint32_t timing = 0;
    bool stamps = false;
    const int* last_stop = nullptr;
    int slot_word = -1;
    bool slot_fresh = false;
    Old() {
        for (int i = 0; i < 2 * N; ++i) ev[i] = i;
    }
    void event_record(int e) { log.push_back(e), when[e] = now; }
    void begin(const ivx_stage_call& c) {
        timing = ~stage_timing_off;
        stamps = timing != 0u && !c.force_events && !stage_events_only && c.part == 3u && !c.slab_record && c.assign_fits && !c.standalone_first && !c.recording &&
                 tick_used + IVX_N_TIMED_STAGES + 1u <= IVX_TICK_WORDS;
        if (stamps) log.push_back(-1);
        if (timing != 0u && !stamps) log.push_back(-2);
        last_stop = nullptr, slot_word = -1, slot_fresh = false;
    }
    void T0(int i) {
        if (!((timing >> (i)) & 1u)) last_stop = nullptr;
        else if (stamps) {
            slot_fresh = tick_next == nullptr;
            if (slot_fresh) {
                tick_host[tick_used] = 0ull;
                tick_next = tick_dev + tick_used++;
            }
            slot_word = (int)(tick_next - tick_dev);
        } else {
            if (last_stop) ev_start_ref[i] = last_stop;
            else {
                event_record(ev[2 * (i)]);
                ev_start_ref[i] = &ev[2 * (i)];
            }
        }
    }
    void T1(int i) {
        if ((timing >> (i)) & 1u) {
            if (stamps) {
                stamp_mask |= 1u << (i), timed_mask &= ~(1u << (i));
                if (tick_next == tick_dev + slot_word) {
                    tick_start_ref[i] = tick_end_ref[i] = -1;
                    if (slot_fresh) tick_next = nullptr, --tick_used;
                } else {
                    tick_start_ref[i] = (int8_t)slot_word;
                    tick_end_ref[i] = (int8_t)tick_used;
                    tick_host[tick_used] = 0ull;
                    tick_next = tick_dev + tick_used++;
                }
            } else {
                event_record(ev[2 * (i) + 1]);
                last_stop = &ev[2 * (i) + 1];
                timed_mask |= 1u << (i), stamp_mask &= ~(1u << (i));
            }
        }
    }
    ull* take_tick(bool recording) {
        if (!tick_next || recording) return nullptr;
        ull* t = tick_next;
        tick_next = nullptr;
        return t;
    }
    bool gather(ull** a_ticks_dev, ull** a_ticks_host, uint32_t* a_n_ticks, ull** a_tick) {
        if (tick_used) {
            *a_ticks_dev = tick_dev, *a_ticks_host = tick_host, *a_n_ticks = tick_used;
            *a_tick = tick_next;
            tick_next = nullptr;
            return true;
        }
        return false;
    }
    void collect_tail(float stage_ms[N]) {
        for (int i = 0; i < N; ++i) {
            float ms = 0.0f;
            tick_last[2 * i] = tick_last[2 * i + 1] = 0ull;
            if ((stamp_mask >> i) & 1u) {
                if (tick_start_ref[i] >= 0 && tick_end_ref[i] >= 0) {
                    const ull t0 = tick_host[tick_start_ref[i]], t1 = tick_host[tick_end_ref[i]];
                    tick_last[2 * i] = t0, tick_last[2 * i + 1] = t1;
                    if (t0 != 0ull && t1 > t0) ms = (float)((double)(t1 - t0) / KHZ);
                }
            } else if ((timed_mask >> i) & 1u) {
                ms = (float)((double)(when[2 * i + 1] - when[*ev_start_ref[i]]) / KHZ);
            }
            stage_ms[i] = ms;
        }
        timed_mask = 0;
        stamp_mask = 0;
        tick_used = 0;
        tick_next = nullptr;
    }
};

// ---- the clock under a driver of its own -----------------------------------------------------------------------------------------------
struct New {
    ivx_stage_timing t;
    FakeRt rt;
    New() { memset(&t, 0, sizeof(t)); }
    int next() const { return t.tick_next ? (int)(t.tick_next - t.tick_dev) : -1; }
    // a launch made directly at time `now`: stamps the pending word, if there is one
    void launch(ull now, bool recording = false) {
        if (ull* w = t.take(recording)) *w = now;
    }
    // k_step_gather at time `now`: the words go to the host copy, the launch's own word from its register; the device words are zeroed
    void gather(ull now) {
        ull *d = nullptr, *h = nullptr, *own = nullptr;
        uint32_t n = 0;
        t.hand_to_gather(&d, &h, &n, &own);
        for (uint32_t w = 0; w < n; ++w) h[w] = d + w == own ? now : d[w], d[w] = 0ull;
    }
    float read(int i) { return t.read(rt, i, KHZ); }
};

static const ivx_stage_call FUSED = {3u, false, false, true, false, false};
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                             \
        }                                                         \
    } while (0)
static bool near_ms(float ms, double us) { return ms > 0.0f && (double)ms > 1e-3 * us * 0.999 && (double)ms < 1e-3 * us * 1.001; }

// one call over slots [first, last], a launch of 1 us in every slot but `idle`
static int call(New& c, ull& now, int first, int last, int idle = -1, const ivx_stage_call& how = FUSED) {
    if (c.t.begin(c.rt, how)) return 1;
    for (int i = first; i <= last; ++i) {
        c.rt.now = now;
        if (c.t.open(c.rt, i)) return 1;
        if (i != idle) c.launch(now), now += 100;
        c.rt.now = now;
        if (c.t.close(c.rt, i)) return 1;
    }
    return 0;
}

static int scenarios() {
    {  // all slots timed on the fused path: seven words, each shared between neighbours
        New c;
        ull now = 1000;
        CHECK(!call(c, now, 0, 5));
        CHECK(c.t.call_stamps && c.t.tick_used == 7u && c.next() == 6 && c.t.stamp_mask == 0x3Fu && c.t.timed_mask == 0u);
        for (int i = 0; i < 6; ++i) CHECK(c.t.tick_start_ref[i] == i && c.t.tick_end_ref[i] == i + 1);
        CHECK(c.rt.log == std::vector<int>{-1});  // (the words made, no event)
        c.gather(now);
        for (int i = 0; i < N; ++i) CHECK(i < 6 ? near_ms(c.read(i), 1.0) : c.read(i) == 0.0f);
        CHECK(c.t.tick_last[0] == 1000ull && c.t.tick_last[1] == 1100ull && c.t.tick_last[11] == 1600ull);
        c.t.reset();
        CHECK(c.t.tick_used == 0u && c.next() == -1 && c.t.stamp_mask == 0u);
    }
    {  // a mask with gaps: no sharing across an untimed slot, whose launch closes the slot before it
        New c;
        ull now = 1000;
        c.t.off = ~0x15u;  // slots 0, 2, 4
        CHECK(!call(c, now, 0, 5));
        CHECK(c.t.tick_used == 6u && c.t.stamp_mask == 0x15u);
        for (int k = 0; k < 3; ++k) CHECK(c.t.tick_start_ref[2 * k] == 2 * k && c.t.tick_end_ref[2 * k] == 2 * k + 1);
        CHECK(c.next() == -1);  // (slot 5's launch took slot 4's closing word)
        c.gather(now);
        for (int i = 0; i < 6; ++i) CHECK(i % 2 == 0 ? near_ms(c.read(i), 1.0) : c.read(i) == 0.0f);
    }
    {  // a slot without a launch reports 0; the word it opened at stays pending for the next slot
        New c;
        ull now = 1000;
        CHECK(!call(c, now, 0, 3, 2));
        CHECK(c.t.tick_start_ref[2] == -1 && c.t.tick_end_ref[2] == -1 && c.t.tick_start_ref[3] == 2 && c.t.tick_end_ref[1] == 2 && c.t.tick_used == 4u);
        c.gather(now);
        CHECK(near_ms(c.read(1), 1.0) && c.read(2) == 0.0f && near_ms(c.read(3), 1.0));
        // ... and a word it armed itself is given back
        New d;
        d.t.off = ~4u;
        CHECK(!call(d, now, 0, 3, 2));
        CHECK(d.t.stamp_mask == 4u && d.t.tick_used == 0u && d.next() == -1 && d.t.tick_start_ref[2] == -1);
        d.gather(now);
        CHECK(d.read(2) == 0.0f);
    }
    {  // two enqueues before one collect: the second call's first launch closes the first call's last slot
        New c;
        ull now = 1000;
        CHECK(!call(c, now, 0, 1));
        CHECK(c.t.tick_used == 3u && c.next() == 2);
        now += 700;  // (host time between the calls falls into slot 1: start to start)
        CHECK(!call(c, now, 2, 5));
        CHECK(c.t.tick_used == 7u && c.t.tick_start_ref[2] == 2 && c.t.tick_end_ref[1] == 2 && c.t.stamp_mask == 0x3Fu);
        c.gather(now);
        CHECK(near_ms(c.read(0), 1.0) && near_ms(c.read(1), 8.0) && near_ms(c.read(5), 1.0));
    }
    {  // the word budget exhausted: the call falls to events as a whole; the pending word still goes to its first launch
        New c;
        ull now = 1000;
        for (int k = 0; k < 4; ++k) CHECK(!call(c, now, 0, 5) && c.t.call_stamps && c.t.tick_used == 7u + 6u * k);
        CHECK(!call(c, now, 0, 5));
        CHECK(!c.t.call_stamps && c.t.tick_used == 25u && c.next() == -1 && c.t.stamp_mask == 0u && c.t.timed_mask == 0x3Fu);
        CHECK(c.rt.log == (std::vector<int>{-1, -1, -1, -1, -2, 0, 1, 3, 5, 7, 9, 11}));
        c.gather(now);
        for (int i = 0; i < 6; ++i) CHECK(near_ms(c.read(i), 1.0));
        CHECK(c.t.tick_last[0] == 0ull);  // (no raw stamps behind an event-timed slot)
    }
    {  // a call that may not stamp — a part of a call, a slab's record, a recorded batch, a grid of the slab protocol — takes events
        const ivx_stage_call part1 = {1u, false, false, true, false, false}, record = {3u, false, true, true, false, false}, batch = {3u, false, false, true, false, true};
        for (const ivx_stage_call* how : {&part1, &record, &batch}) {
            New c;
            ull now = 1000;
            CHECK(!call(c, now, 0, 1, -1, *how) && !c.t.call_stamps && c.t.tick_used == 0u && c.t.timed_mask == 3u);
        }
        New c;
        ull now = 1000;
        c.t.events_only = 1;
        CHECK(!call(c, now, 0, 1) && !c.t.call_stamps);
        c.t.off = 0xFFFFFFFFu;  // no slot timed: neither clock, nothing made
        c.rt.log.clear();
        CHECK(!call(c, now, 0, 5) && c.rt.log.empty());
    }
    printf("stage clock scenarios: ok\n");
    return 0;
}

// ---- random sequences through both -----------------------------------------------------------------------------------------------------
static int mismatch(const New& a, const Old& b, const char* where, long seq) {
    const int nb = b.tick_next ? (int)(b.tick_next - b.tick_dev) : -1;
    bool ok = a.t.stamp_mask == b.stamp_mask && a.t.timed_mask == b.timed_mask && a.t.tick_used == b.tick_used && a.next() == nb && a.rt.log == b.log;
    for (int i = 0; i < N && ok; ++i) {
        if ((b.stamp_mask >> i) & 1u) ok = a.t.tick_start_ref[i] == b.tick_start_ref[i] && a.t.tick_end_ref[i] == b.tick_end_ref[i];
        if ((b.timed_mask >> i) & 1u) ok = ok && a.t.ev_start_ref[i] == *b.ev_start_ref[i];
    }
    if (a.t.tick_host) ok = ok && memcmp(a.rt.host, b.host_, sizeof(b.host_)) == 0 && memcmp(a.rt.dev, b.dev_, sizeof(b.dev_)) == 0;
    if (!ok) printf("MISMATCH in sequence %ld %s\n", seq, where);
    return ok ? 0 : 1;
}

static int random_sequences(long n_seq, unsigned seed) {
    std::mt19937 rng(seed);
    auto coin = [&](double p) { return std::uniform_real_distribution<double>(0.0, 1.0)(rng) < p; };
    auto upto = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    long calls = 0, stamp_calls = 0, event_calls = 0, untimed_calls = 0, idle_slots = 0, unstamped_first = 0, exhausted = 0, collects = 0, compared = 0;
    for (long seq = 0; seq < n_seq; ++seq) {
        New a;
        Old b;
        ull now = 1000 + upto(1000);
        const int n_collects = 1 + (int)upto(3);
        for (int col = 0; col < n_collects; ++col) {
            const int n_enq = coin(0.9) ? 1 + (int)upto(3) : 4 + (int)upto(3);
            const bool heavy = n_enq >= 4;  // (whole timed calls one behind the other: the words run out)
            bool any_record = false;
            for (int e = 0; e < n_enq; ++e) {
                // the call, as step_enqueue sees it
                const uint32_t mask = heavy || coin(0.3) ? 0x3FFu : (coin(0.1) ? 0u : upto(1024));
                const uint32_t stages = heavy || coin(0.4) ? 31u : 1u + upto(31);  // sample, derive, occupied, regions, remesh (inertia rides with derive here)
                const uint32_t part = heavy || coin(0.7) ? 3u : 1u + upto(3);
                const bool front = part & 1u, back = part & 2u;
                const bool has_sample = stages & 1u, has_derive = stages & 2u, has_regions = stages & 8u, has_remesh = stages & 16u;
                const uint32_t post = back ? stages & 28u : 0u;
                ivx_stage_call c;
                c.part = part;
                c.force_events = coin(0.03);
                c.slab_record = post && coin(0.08);
                c.assign_fits = !coin(0.05);
                c.standalone_first = (post & 8u) && !has_derive && coin(0.8);
                c.recording = coin(0.15);
                a.t.off = b.stage_timing_off = ~mask;
                a.t.events_only = b.stage_events_only = coin(0.1) ? 1 : 0;
                const uint32_t used_before = b.tick_used;
                a.t.begin(a.rt, c), b.begin(c);
                if (a.t.call_stamps != b.stamps) return printf("MISMATCH in sequence %ld: stamps or events\n", seq), 1;
                ++calls;
                if (!mask) ++untimed_calls;
                else if (b.stamps) ++stamp_calls;
                else {
                    ++event_calls;
                    if (used_before + N + 1u > IVX_TICK_WORDS) ++exhausted;
                }
                any_record |= c.slab_record;
                int slots[6], n_slots = 0;
                if (front && has_sample) slots[n_slots++] = 0;
                if (front && has_derive) slots[n_slots++] = 1;
                if (post) {
                    slots[n_slots++] = 2, slots[n_slots++] = 3;
                    if (has_regions || has_remesh) slots[n_slots++] = 4;
                    if (has_regions && c.assign_fits) slots[n_slots++] = 5;
                }
                for (int k = 0; k < n_slots; ++k) {
                    const int i = slots[k];
                    a.rt.now = b.now = now;
                    a.t.open(a.rt, i), b.T0(i);
                    if (mismatch(a, b, "after an open", seq)) return 1;
                    // the slot's launches: none, or a few of which the first may be one that carries no stamp
                    const int n_launch = coin(0.15) ? 0 : 1 + (int)upto(3);
                    if (!n_launch) ++idle_slots;
                    for (int l = 0; l < n_launch; ++l) {
                        now += 50 + upto(400);
                        if (l == 0 && coin(0.15)) {
                            ++unstamped_first;
                            continue;
                        }
                        ull *wa = a.t.take(c.recording), *wb = b.take_tick(c.recording);
                        if ((wa ? wa - a.t.tick_dev : -1) != (wb ? wb - b.tick_dev : -1)) return printf("MISMATCH in sequence %ld: the word taken\n", seq), 1;
                        if (wa) *wa = *wb = coin(0.02) ? 0ull : now;
                    }
                    now += upto(200);
                    a.rt.now = b.now = now;
                    a.t.close(a.rt, i), b.T1(i);
                    if (mismatch(a, b, "after a close", seq)) return 1;
                    ++compared;
                }
                now += upto(2000);
            }
            // the collect: the gather brings the words home — or, behind a slab's record, the host fetches them all
            if (!any_record || coin(0.5)) {
                ull *da = nullptr, *ha = nullptr, *oa = nullptr, *db = nullptr, *hb = nullptr, *ob = nullptr;
                uint32_t na = 0, nb = 0;
                a.t.hand_to_gather(&da, &ha, &na, &oa), b.gather(&db, &hb, &nb, &ob);
                if (na != nb || (oa ? oa - a.t.tick_dev : -1) != (ob ? ob - b.tick_dev : -1)) return printf("MISMATCH in sequence %ld: the gather's hand-over\n", seq), 1;
                for (uint32_t w = 0; w < na; ++w) {
                    ha[w] = da + w == oa ? now : da[w], da[w] = 0ull;
                    hb[w] = db + w == ob ? now : db[w], db[w] = 0ull;
                }
            } else if (b.stamp_mask && a.t.tick_dev) {
                memcpy(a.rt.host, a.rt.dev, sizeof(a.rt.dev)), memset(a.rt.dev, 0, sizeof(a.rt.dev));
                memcpy(b.host_, b.dev_, sizeof(b.dev_)), memset(b.dev_, 0, sizeof(b.dev_));
            }
            if (mismatch(a, b, "before the read", seq)) return 1;
            float ms_b[N];
            b.collect_tail(ms_b);
            for (int i = 0; i < N; ++i) {
                const float ms_a = a.read(i);
                if (memcmp(&ms_a, &ms_b[i], sizeof(float)) != 0) return printf("MISMATCH in sequence %ld: stage_ms[%d] %g vs %g\n", seq, i, ms_a, ms_b[i]), 1;
            }
            a.t.reset();
            if (memcmp(a.t.tick_last, b.tick_last, sizeof(b.tick_last)) != 0 || mismatch(a, b, "after the reset", seq)) return printf("MISMATCH in sequence %ld: raw ticks\n", seq), 1;
            ++collects;
            now += upto(5000);
        }
    }
    printf("stage clock against the transcribed macros: %ld sequences (seed %u), %ld collects, %ld calls — %ld with stamps, %ld with events (%ld of them because "
           "the words ran out), %ld untimed —, %ld slots compared, %ld slots without a launch, %ld first launches without a stamp: all equal\n",
           n_seq, seed, collects, calls, stamp_calls, event_calls, exhausted, untimed_calls, compared, idle_slots, unstamped_first);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "scenarios")) return scenarios();
    if (argc >= 3 && !strcmp(argv[1], "random")) return random_sequences(atol(argv[2]), argc >= 4 ? (unsigned)atol(argv[3]) : 1u);
    fprintf(stderr, "usage: %s scenarios | random N [seed]\n", argv[0]);
    return 2;
}
