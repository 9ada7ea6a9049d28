// The launch recorder's flush plan (impact_amd/csrc/many_plan.hpp) checked on the host, without the HIP runtime:
//   many_plan_check table            recorded batches with the expected launches, members, running block counts, totals and staging offsets
//                                    written out by hand from the rules (tests/test_many_plan_cpu.py)
//   many_plan_check random N [seed]  N random batches over the real kernel ids: the plan against a transcription of the loops it replaced —
//                                    flush_recorded_checked of many.cpp as it stood, on plain structs with the field names it had — and the
//                                    invariants of a plan
// Build: g++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/many_plan_check.cpp -o many_plan_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

#include "../impact_amd/csrc/many_plan.hpp"

using namespace ivx_many;

static const char* const names[IVX_MK_COUNT] = {"ABSORB",     "DERIVE_PLANES",     "DERIVE_SIGNS",      "CHUNK_PRE",    "LIST_REBUILD", "POST1",      "POST2",
                                                "EMIT",       "ASSIGN",            "GATHER",            "SN_EMIT",      "SN_EMIT_GEN",  "INERTIA",    "CLIP",
                                                "SVC_COUNT",  "SVC_SCAN",          "SVC_EMIT",          "SCAN_COUNTS",  "MUT_COUNT",    "MUT_EMIT",   "SELECT_SMALL",
                                                "SELECT_FULL", "PROBE_GATHER",     "ZERO",              "UPLOAD"};

// launch by launch: KERNEL[object.entry:running-count^payload-offset ...]=total@off_args/off_ends, `!` behind the total of a launch that is
// not issued, the payload offset for uploads only; the size of the staging block at the end
static std::string plan_text(const Plan& pl) {
    std::string s;
    for (size_t p = 0; p < pl.n_launches(); ++p) {
        s += names[pl.kernel[p]];
        s += '[';
        for (uint32_t m = pl.first[p]; m < pl.first[p + 1]; ++m) {
            if (m != pl.first[p]) s += ' ';
            s += std::to_string(pl.members[m].first) + '.' + std::to_string(pl.members[m].second) + ':' + std::to_string(pl.ends[m]);
            if (is_upload(pl.kernel[p])) s += '^' + std::to_string(pl.off_payload[m]);
        }
        s += "]=" + std::to_string(pl.totals[p]) + (pl.issued(p) ? "" : "!") + '@' + std::to_string(pl.off_args[p]) + '/' + std::to_string(pl.off_ends[p]) + ' ';
    }
    return s + "bytes=" + std::to_string(pl.bytes);
}

// ---- the table -----------------------------------------------------------------------------------------------------------------------------
// argument blocks of 48 bytes, but IVX_MK_GATHER's of 8 and the range operations' of 32
static void table_arg_bytes(uint32_t ab[IVX_MK_COUNT]) {
    for (int k = 0; k < IVX_MK_COUNT; ++k) ab[k] = 48u;
    ab[IVX_MK_GATHER] = 8u;
    ab[IVX_MK_ZERO] = ab[IVX_MK_UPLOAD] = 32u;
}
struct E {
    int kernel;
    uint32_t blocks, payload;
};
static const int A = IVX_MK_POST1, B = IVX_MK_POST2, C = IVX_MK_EMIT, G = IVX_MK_GATHER, Z = IVX_MK_ZERO, U = IVX_MK_UPLOAD;
struct Row {
    const char* what;
    std::vector<std::vector<E>> chains;
    const char* plan;
};
static const Row rows[] = {
    {"an empty batch", {}, "bytes=0"},
    {"objects that recorded nothing", {{}, {}, {}}, "bytes=0"},
    {"one object", {{{A, 3, 0}, {B, 2, 0}, {G, 1, 0}}}, "POST1[0.0:3]=3@0/48 POST2[0.1:2]=2@64/112 GATHER[0.2:1]=1@128/144 bytes=160"},
    {"three identical chains: as many launches as a chain has entries",
     {{{A, 2, 0}, {B, 1, 0}}, {{A, 2, 0}, {B, 1, 0}}, {{A, 2, 0}, {B, 1, 0}}},
     "POST1[0.0:2 1.0:4 2.0:6]=6@0/144 POST2[0.1:1 1.1:2 2.1:3]=3@160/304 bytes=320"},
    {"the middle object skips a stage: the others merge at equal kernels",
     {{{A, 1, 0}, {B, 1, 0}, {C, 1, 0}}, {{A, 2, 0}, {C, 2, 0}}, {{A, 3, 0}, {B, 3, 0}, {C, 3, 0}}},
     "POST1[0.0:1 1.0:3 2.0:6]=6@0/144 POST2[0.1:1 2.1:4]=4@160/256 EMIT[0.2:1 1.1:3 2.2:6]=6@272/416 bytes=432"},
    {"the first object skips a stage: its next kernel goes first, the other object's entries stay in order",
     {{{A, 1, 0}, {C, 1, 0}}, {{A, 1, 0}, {B, 1, 0}, {C, 1, 0}}},
     "POST1[0.0:1 1.0:2]=2@0/96 EMIT[0.1:1]=1@112/160 POST2[1.1:1]=1@176/224 EMIT[1.2:1]=1@240/288 bytes=304"},
    {"one object, the same kernel twice in a row: two launches", {{{A, 1, 0}, {A, 2, 0}}}, "POST1[0.0:1]=1@0/48 POST1[0.1:2]=2@64/112 bytes=128"},
    {"one object, three range operations in a row: one launch", {{{Z, 1, 0}, {Z, 2, 0}, {Z, 3, 0}}}, "ZERO[0.0:1 0.1:3 0.2:6]=6@0/96 bytes=112"},
    {"range operations of two objects: all in one launch, objects ascending", {{{Z, 1, 0}, {Z, 1, 0}}, {{Z, 2, 0}}}, "ZERO[0.0:1 0.1:2 1.0:4]=4@0/96 bytes=112"},
    {"a fill, an upload, a fill: two kernels, three launches; the upload's words ahead of everything",
     {{{Z, 1, 0}, {U, 1, 8}, {Z, 1, 0}}},
     "ZERO[0.0:1]=1@16/48 UPLOAD[0.1:1^0]=1@64/96 ZERO[0.2:1]=1@112/144 bytes=160"},
    {"uploads of 4, 12, 16 and 20 bytes: each on a 16-byte boundary",
     {{{U, 1, 4}, {U, 1, 12}}, {{U, 1, 16}, {U, 1, 20}}},
     "UPLOAD[0.0:1^0 0.1:2^16 1.0:3^32 1.1:4^48]=4@80/208 bytes=224"},
    {"an upload behind a kernel: its words still come first", {{{A, 1, 0}, {U, 1, 20}}}, "POST1[0.0:1]=1@32/80 UPLOAD[0.1:1^0]=1@96/128 bytes=144"},
    {"entries without blocks: planned, a launch whose total is 0 not issued",
     {{{A, 0, 0}, {B, 2, 0}}, {{A, 0, 0}, {B, 0, 0}}},
     "POST1[0.0:0 1.0:0]=0!@0/96 POST2[0.1:2 1.1:2]=2@112/208 bytes=224"},
    {"object 0 recorded nothing", {{}, {{A, 1, 0}}, {{A, 1, 0}, {B, 1, 0}}}, "POST1[1.0:1 2.0:2]=2@0/96 POST2[2.1:1]=1@112/160 bytes=176"},
    {"object 0 finishes first: the next kernel is object 1's",
     {{{A, 1, 0}}, {{A, 1, 0}, {B, 1, 0}, {C, 1, 0}}, {{A, 1, 0}, {C, 1, 0}}},
     "POST1[0.0:1 1.0:2 2.0:3]=3@0/144 POST2[1.1:1]=1@160/208 EMIT[1.2:1 2.1:2]=2@224/320 bytes=336"},
};

static Chains to_chains(const std::vector<std::vector<E>>& in) {
    Chains chains(in.size());
    for (size_t i = 0; i < in.size(); ++i)
        for (const E& e : in[i]) chains[i].push_back(Entry{e.kernel, e.blocks, e.payload, 0u, 0u});
    return chains;
}

static int run_table() {
    uint32_t ab[IVX_MK_COUNT];
    table_arg_bytes(ab);
    int bad = 0;
    Plan pl;  // (one plan for all rows, as the recorder keeps one for all flushes)
    for (const Row& r : rows) {
        plan_flush(to_chains(r.chains), ab, pl);
        const std::string got = plan_text(pl);
        if (got != r.plan) {
            ++bad;
            printf("%s:\n  expected %s\n  got      %s\n", r.what, r.plan, got.c_str());
        }
    }
    printf("many plan table: %s (%zu rows)\n", bad ? "FAILED" : "ok", sizeof rows / sizeof rows[0]);
    return bad ? 1 : 0;
}

// ---- what the plan replaced, with its field and function names ----------------------------------------------------------------------------
namespace old {
struct Entry {
    int kernel;
    uint32_t blocks, off, bytes;
    uint32_t payload_off, payload_bytes;
};
struct ivx_many_reg {
    void* fn;
    uint32_t arg_bytes;
};
static ivx_many_reg g_regs[IVX_MK_COUNT];
struct Recorder {
    std::vector<std::vector<Entry>> chains;
    size_t n_entries = 0;
    std::vector<uint32_t> cursor;
};
struct Plan {
    std::vector<int> kernel;
    std::vector<uint32_t> first;
    std::vector<std::pair<uint32_t, uint32_t>> members;
    std::vector<size_t> off_args, off_ends, off_payload;
    std::vector<uint32_t> totals;
    std::vector<std::vector<uint32_t>> ends;  // (what the fill loop wrote at off_ends[p] of the pinned block)
    size_t bytes = 0;
};
static void flush_recorded_checked(Recorder* r, Plan& plan) {
    const size_t n_obj = r->chains.size();
    r->cursor.assign(n_obj, 0u);
    size_t left = r->n_entries;
    size_t lowest = 0;
    while (left) {
        while (lowest < n_obj && r->cursor[lowest] >= r->chains[lowest].size()) ++lowest;
        const int k = r->chains[lowest][r->cursor[lowest]].kernel;
        plan.kernel.push_back(k);
        plan.first.push_back((uint32_t)plan.members.size());
        for (size_t i = lowest; i < n_obj; ++i) {
            while (r->cursor[i] < r->chains[i].size() && r->chains[i][r->cursor[i]].kernel == k) {
                plan.members.emplace_back((uint32_t)i, r->cursor[i]);
                r->cursor[i] += 1u;
                left -= 1;
                if (k != IVX_MK_ZERO && k != IVX_MK_UPLOAD) break;
            }
        }
    }
    const size_t n_launch = plan.kernel.size();
    plan.first.push_back((uint32_t)plan.members.size());
    size_t bytes = 0;
    plan.off_args.resize(n_launch), plan.off_ends.resize(n_launch), plan.totals.resize(n_launch);
    plan.off_payload.assign(plan.members.size(), 0);
    for (size_t p = 0; p < n_launch; ++p) {
        if (plan.kernel[p] != IVX_MK_UPLOAD) continue;
        for (uint32_t m = plan.first[p]; m < plan.first[p + 1]; ++m) {
            const Entry& e = r->chains[plan.members[m].first][plan.members[m].second];
            plan.off_payload[m] = bytes;
            bytes += (e.payload_bytes + 15u) & ~15u;
        }
    }
    for (size_t p = 0; p < n_launch; ++p) {
        const uint32_t ab = g_regs[plan.kernel[p]].arg_bytes, nm = plan.first[p + 1] - plan.first[p];
        plan.off_args[p] = bytes;
        bytes += (size_t)ab * nm;
        bytes = (bytes + 15) & ~(size_t)15;
        plan.off_ends[p] = bytes;
        bytes += 4 * (size_t)nm;
        bytes = (bytes + 15) & ~(size_t)15;
    }
    plan.bytes = bytes;
    plan.ends.resize(n_launch);
    for (size_t p = 0; p < n_launch; ++p) {
        uint32_t run = 0;
        for (uint32_t m = plan.first[p]; m < plan.first[p + 1]; ++m) {
            const Entry& e = r->chains[plan.members[m].first][plan.members[m].second];
            run += e.blocks;
            plan.ends[p].push_back(run);
        }
        plan.totals[p] = run;
    }
}
}  // namespace old

// the twin's search (ivx_many_find, many.hpp): first i with block_end[i] > b
static uint32_t many_find(const uint32_t* block_end, uint32_t n, uint32_t b) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (block_end[mid] > b) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}

#define REQUIRE(cond)                                                               \
    do {                                                                            \
        if (!(cond)) {                                                              \
            printf("batch %zu: %s fails; plan %s\n", i, #cond, plan_text(pl).c_str()); \
            return 1;                                                               \
        }                                                                           \
    } while (0)

static int run_random(size_t n, uint64_t seed) {
    std::mt19937_64 rng(seed);
    auto upto = [&](uint32_t hi) { return (uint32_t)(rng() % ((uint64_t)hi + 1u)); };
    size_t n_entries_all = 0, n_launches_all = 0, n_idle = 0, n_range_merges = 0;
    Plan pl;
    Chains chains;
    std::vector<std::vector<uint32_t>> launch_of;
    struct Range {
        size_t off, len;
    };
    std::vector<Range> ranges;
    for (size_t i = 0; i < n; ++i) {
        // the sizes of the argument blocks: multiples of 8, the range operations' as they are
        uint32_t ab[IVX_MK_COUNT];
        for (int k = 0; k < IVX_MK_COUNT; ++k) ab[k] = 8u * (1u + upto(149));
        ab[IVX_MK_ZERO] = ab[IVX_MK_UPLOAD] = 32u;
        // a program of up to 12 kernels that the objects follow, each with entries left out, doubled or replaced: chains that merge in part
        int program[12];
        const uint32_t n_prog = upto(12);
        for (uint32_t k = 0; k < n_prog; ++k) program[k] = rng() % 3 == 0 ? (rng() % 2 ? (int)IVX_MK_ZERO : (int)IVX_MK_UPLOAD) : (int)upto(IVX_MK_COUNT - 1);
        const uint32_t n_obj = upto(64);
        chains.assign(n_obj, {});
        size_t n_entries = 0;
        for (auto& chain : chains) {
            for (uint32_t k = 0; k < n_prog && chain.size() < 12u; ++k) {
                const uint32_t what = upto(9);
                if (what == 0) continue;
                const int kernel = what == 1 ? (int)upto(IVX_MK_COUNT - 1) : program[k];
                for (uint32_t rep = 0; rep < (what == 2 ? 2u : 1u) && chain.size() < 12u; ++rep)
                    chain.push_back(Entry{kernel, rng() % 5 ? upto(300) : 0u, is_upload(kernel) ? 4u * upto(1024) : 0u, 0u, 0u});
            }
            n_entries += chain.size();
        }
        plan_flush(chains, ab, pl);

        // against the transcription
        old::Recorder r;
        r.chains.resize(n_obj);
        for (uint32_t o = 0; o < n_obj; ++o)
            for (const Entry& e : chains[o]) r.chains[o].push_back(old::Entry{e.kernel, e.blocks, 0u, ab[e.kernel], 0u, e.payload_bytes});
        r.n_entries = n_entries;
        for (int k = 0; k < IVX_MK_COUNT; ++k) old::g_regs[k].arg_bytes = ab[k];
        old::Plan op;
        old::flush_recorded_checked(&r, op);
        REQUIRE(pl.kernel == op.kernel && pl.first == op.first && pl.members == op.members);
        REQUIRE(pl.off_args == op.off_args && pl.off_ends == op.off_ends && pl.off_payload == op.off_payload && pl.totals == op.totals && pl.bytes == op.bytes);
        const size_t n_launch = pl.n_launches();
        for (size_t p = 0; p < n_launch; ++p)
            REQUIRE(pl.n_members(p) == op.ends[p].size() && std::equal(op.ends[p].begin(), op.ends[p].end(), pl.ends.begin() + pl.first[p]));

        // the invariants: every entry a member exactly once, of a launch of its kernel
        REQUIRE(pl.members.size() == n_entries && pl.ends.size() == n_entries && pl.first.size() == n_launch + 1u && pl.first[n_launch] == n_entries);
        launch_of.assign(n_obj, {});
        for (uint32_t o = 0; o < n_obj; ++o) launch_of[o].assign(chains[o].size(), UINT32_MAX);
        ranges.clear();
        for (size_t p = 0; p < n_launch; ++p) {
            REQUIRE(pl.n_members(p) >= 1u);
            uint32_t run = 0;
            for (uint32_t m = pl.first[p]; m < pl.first[p + 1]; ++m) {
                const uint32_t o = pl.members[m].first, e = pl.members[m].second;
                REQUIRE(o < n_obj && e < chains[o].size() && launch_of[o][e] == UINT32_MAX);
                launch_of[o][e] = (uint32_t)p;
                REQUIRE(chains[o][e].kernel == pl.kernel[p]);
                // inside a launch: objects ascending, an object's merged entries in chain order
                if (m != pl.first[p]) REQUIRE(pl.members[m - 1] < pl.members[m]);
                // the running counts and the total
                run += chains[o][e].blocks;
                REQUIRE(pl.ends[m] == run);
                if (is_upload(pl.kernel[p])) ranges.push_back(Range{pl.off_payload[m], chains[o][e].payload_bytes});
                else REQUIRE(pl.off_payload[m] == 0u);
            }
            REQUIRE(pl.totals[p] == run && pl.issued(p) == (run != 0u));
            n_idle += !pl.issued(p);
            ranges.push_back(Range{pl.off_args[p], (size_t)ab[pl.kernel[p]] * pl.n_members(p)});
            ranges.push_back(Range{pl.off_ends[p], 4u * (size_t)pl.n_members(p)});
            // what the twin's search makes of the counts: block b belongs to the member whose blocks are [end before it, its end)
            const uint32_t* ends = pl.ends.data() + pl.first[p];
            for (uint32_t t = 0; t < 4u && run; ++t) {
                const uint32_t b = t == 0 ? 0u : (t == 1 ? run - 1u : upto(run - 1u)), at = many_find(ends, pl.n_members(p), b);
                REQUIRE(at < pl.n_members(p) && b < ends[at] && (at ? ends[at - 1u] : 0u) <= b);
                REQUIRE(chains[pl.members[pl.first[p] + at].first][pl.members[pl.first[p] + at].second].blocks > b - (at ? ends[at - 1u] : 0u));
            }
        }
        // an object's entries reach the stream in chain order: one launch after the other, range operations also in the same one
        for (uint32_t o = 0; o < n_obj; ++o)
            for (size_t e = 0; e < chains[o].size(); ++e) {
                REQUIRE(launch_of[o][e] != UINT32_MAX);
                if (!e) continue;
                REQUIRE(launch_of[o][e - 1] <= launch_of[o][e]);
                if (launch_of[o][e - 1] != launch_of[o][e]) continue;
                REQUIRE(is_range_op(chains[o][e].kernel));
                ++n_range_merges;
            }
        // the pieces of the staging block: on 16-byte boundaries, apart from one another, inside the block
        std::sort(ranges.begin(), ranges.end(), [](const Range& a, const Range& b) { return a.off != b.off ? a.off < b.off : a.len < b.len; });
        for (size_t k = 0; k < ranges.size(); ++k) {
            REQUIRE(ranges[k].off % 16u == 0u && ranges[k].off + ranges[k].len <= pl.bytes);
            if (k + 1 < ranges.size()) REQUIRE(ranges[k].off + ranges[k].len <= ranges[k + 1].off);
        }
        REQUIRE(pl.bytes % 16u == 0u);
        n_entries_all += n_entries, n_launches_all += n_launch;
    }
    printf("many plan random: ok (%zu batches: %zu entries in %zu launches, %zu of them without blocks; %zu range operations merged into their object's launch)\n", n,
           n_entries_all, n_launches_all, n_idle, n_range_merges);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "table")) return run_table();
    if (argc >= 3 && !strcmp(argv[1], "random")) return run_random((size_t)atoll(argv[2]), argc >= 4 ? (uint64_t)atoll(argv[3]) : 1u);
    fprintf(stderr, "usage: many_plan_check table | random N [seed]\n");
    return 2;
}
