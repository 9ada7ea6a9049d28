// The flush's host-side decisions (many.hpp, many.cpp), free of HIP: which recorded entries of which objects go into which launch of a twin,
// in which order, and where every launch's argument blocks, running block counts and upload words stand in the one staging block.
// flush_recorded_checked (many.cpp) executes the plan; tools/many_plan_check.cpp holds it to plans written out by hand, without a GPU
// (tests/test_many_plan_cpu.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

// kernels with a twin
enum ivx_many_kernel : int {
    IVX_MK_ABSORB = 0,
    IVX_MK_DERIVE_PLANES,
    IVX_MK_DERIVE_SIGNS,
    IVX_MK_CHUNK_PRE,
    IVX_MK_LIST_REBUILD,
    IVX_MK_POST1,
    IVX_MK_POST2,
    IVX_MK_EMIT,
    IVX_MK_ASSIGN,
    IVX_MK_GATHER,
    IVX_MK_SN_EMIT_SLOTS,
    IVX_MK_SN_EMIT_GENERAL_SLOTS,
    IVX_MK_INERTIA_DENSE,
    IVX_MK_CLIP,
    IVX_MK_SVC_COUNT,  // collidable-against-voxel-object contacts: count | scan | emit (contacts.hip)
    IVX_MK_SVC_SCAN,
    IVX_MK_SVC_EMIT,
    IVX_MK_SCAN_COUNTS,  // contacts between two voxel objects: count (probes of one against the other's field) | scan | emit (collide.hip)
    IVX_MK_MUT_COUNT,
    IVX_MK_MUT_EMIT,
    IVX_MK_PROBE_SELECT_SMALL,  // collision probes of the listed chunk submeshes: select (two LDS sizes) | gather (collide.hip)
    IVX_MK_PROBE_SELECT_FULL,
    IVX_MK_PROBE_GATHER,
    IVX_MK_ZERO,    // fill a device range with one word (the twin of a hipMemsetAsync of 0x00 or 0xFF bytes)
    IVX_MK_UPLOAD,  // host words to a device range (the twin of a small hipMemcpyAsync host -> device): the words ride in the flush's one staging copy
    IVX_MK_COUNT
};

namespace ivx_many {

// A range operation writes a device range and nothing else: consecutive ones of ONE object may share a launch (every other kernel of an object
// reads what the object's previous launch wrote: one entry per launch, in chain order) | an upload's words travel in the staging block
constexpr bool is_range_op(int k) { return k == IVX_MK_ZERO || k == IVX_MK_UPLOAD; }
constexpr bool is_upload(int k) { return k == IVX_MK_UPLOAD; }
// every piece of the staging block starts on a 16-byte boundary
constexpr size_t round16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

// a captured launch, as it stands in its object's chain
struct Entry {
    int kernel;
    uint32_t blocks;
    uint32_t payload_bytes;     // IVX_MK_UPLOAD: the host words
    uint32_t off, payload_off;  // (the recorder's: where its arena keeps the argument block and the words until the flush; the plan reads neither)
};
typedef std::vector<std::vector<Entry>> Chains;  // per object of the batch

// The merged launches of a flush, in issue order: launch p takes the members [first[p], first[p + 1]) of `members` ((object, entry index)
// pairs). Flat vectors kept from flush to flush: the same chains recur frame after frame and nothing is allocated after the first.
struct Plan {
    std::vector<int> kernel;
    std::vector<uint32_t> first;
    std::vector<std::pair<uint32_t, uint32_t>> members;
    std::vector<uint32_t> ends;                           // per member: the blocks of its launch up to and including its own (what the twin searches)
    std::vector<size_t> off_args, off_ends, off_payload;  // offsets into the staging block (off_payload: per member, uploads only)
    std::vector<uint32_t> totals;
    size_t bytes = 0;  // of the staging block
    std::vector<uint32_t> cursor;  // (scratch: per object, the entries planned so far)
    void clear() {
        kernel.clear(), first.clear(), members.clear(), ends.clear(), off_args.clear(), off_ends.clear(), off_payload.clear(), totals.clear();
        bytes = 0;
    }
    size_t n_launches() const { return kernel.size(); }
    uint32_t n_members(size_t p) const { return first[p + 1] - first[p]; }
    bool issued(size_t p) const { return totals[p] != 0; }  // a launch without blocks is planned (its members are spent) and never issued
};

// `arg_bytes`: the size of an argument block, per kernel id
inline void plan_flush(const Chains& chains, const uint32_t* arg_bytes, Plan& plan) {
    plan.clear();
    const size_t n_obj = chains.size();
    plan.cursor.assign(n_obj, 0u);
    std::vector<uint32_t>& cursor = plan.cursor;
    size_t left = 0;
    for (const auto& c : chains) left += c.size();
    // the front of the chains, position by position: the first unfinished object's next kernel, and everybody whose next entry is that kernel.
    // `lowest`: no object below it has entries left (the scan for the next kernel starts there instead of at object 0)
    size_t lowest = 0;
    while (left) {
        while (cursor[lowest] >= chains[lowest].size()) ++lowest;
        const int k = chains[lowest][cursor[lowest]].kernel;
        plan.kernel.push_back(k);
        plan.first.push_back((uint32_t)plan.members.size());
        uint32_t run = 0;
        for (size_t i = lowest; i < n_obj; ++i) {
            while (cursor[i] < chains[i].size() && chains[i][cursor[i]].kernel == k) {
                plan.members.emplace_back((uint32_t)i, cursor[i]);
                plan.ends.push_back(run += chains[i][cursor[i]].blocks);
                cursor[i] += 1u;
                left -= 1;
                if (!is_range_op(k)) break;
            }
        }
        plan.totals.push_back(run);
    }
    const size_t n_launch = plan.kernel.size();
    plan.first.push_back((uint32_t)plan.members.size());
    // the staging block: the words of the uploads first, then per launch its argument blocks and its running block counts
    size_t bytes = 0;
    plan.off_args.resize(n_launch), plan.off_ends.resize(n_launch);
    plan.off_payload.assign(plan.members.size(), 0);
    for (size_t p = 0; p < n_launch; ++p) {
        if (!is_upload(plan.kernel[p])) continue;
        for (uint32_t m = plan.first[p]; m < plan.first[p + 1]; ++m) {
            plan.off_payload[m] = bytes;
            bytes += round16(chains[plan.members[m].first][plan.members[m].second].payload_bytes);
        }
    }
    for (size_t p = 0; p < n_launch; ++p) {
        const uint32_t nm = plan.n_members(p);
        plan.off_args[p] = bytes;
        bytes = round16(bytes + (size_t)arg_bytes[plan.kernel[p]] * nm);
        plan.off_ends[p] = bytes;
        bytes = round16(bytes + 4 * (size_t)nm);
    }
    plan.bytes = bytes;
}

}  // namespace ivx_many
