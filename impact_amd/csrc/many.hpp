// Many objects per launch. The reference's per-frame unit is the manager, not the object: every voxel object is
// synced each frame (impact_voxel/src/lib.rs:729-733, engine/src/tasks.rs:376-399), the fragments of an impact come into being together
// (interaction/fracturing.rs:1047-1189), its own stress scene holds a thousand small objects. One object's step, edit or sync is ~10 launches
// of a few microseconds each — for a small object all of its cost — so N objects looped are N x that, and what has to go is the launches,
// not the work.
//
// The mechanism is a RECORDER in front of the kernel launches. Between ivx_many_begin and ivx_many_flush a launch of a kernel that has a
// `_many` twin is not issued: its argument block and its block count are written down at the object's position in the chain. The per-object
// host code (stage logic, scratch bookkeeping, the submesh manager) runs unchanged, object after object. The flush then issues, chain position
// by chain position, ONE launch for all objects: the twin finds the object of a block by a search over the running block counts (scalar
// loads: the block index is uniform), fetches that object's argument block and runs the very body of the single-object kernel with the
// block index counted from the object's first block. Objects whose chains differ (a stage one of them skips) still merge wherever the same
// kernel stands at the same position; a launch or a stream operation WITHOUT a twin first flushes what has been recorded (ivx_many_break, in
// front of every such call): order on the stream is that of the recorded program in every case, merging is only ever an optimisation.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "many_plan.hpp"  // the kernel ids (ivx_many_kernel)

struct ivx_ctx;

// the twin's launcher: `d_argv` n argument blocks back to back, `d_block_end` the running block counts, `total` blocks in all
typedef int (*ivx_many_launch_fn)(hipStream_t s, const void* d_argv, const uint32_t* d_block_end, uint32_t n, uint32_t total);
// (IVX_MANY_REGISTER below, once per kernel id; `arg_bytes`: the size of an argument block)
void ivx_many_register(int kernel, ivx_many_launch_fn fn, uint32_t arg_bytes);

// recording state of the calling thread: null = launches are issued as they come
bool ivx_many_recording();
// at the top of every entry point that enqueues work for an object: see many.cpp
struct ivx_many_other_context {
    explicit ivx_many_other_context(const ivx_ctx* c);
    ~ivx_many_other_context();
    bool suspended;
};
// true: written down (nothing was launched); false: not recording, or `c` is not the context the batch is recorded for (what has been
// recorded goes out first; the launch belongs on c's stream) — the caller launches
// `owner`: the object the launch belongs to (its grid). A batch recorded through the bare bracket (ivx_many_begin ... _flush, no
// ivx_many_object) keeps a chain per owner, in the order the owners first appear, so that its objects merge front by front as well.
bool ivx_many_capture(const ivx_ctx* c, const void* owner, int kernel, uint32_t blocks, const void* args, uint32_t arg_bytes);
// in front of every launch / stream operation that has no twin: what has been recorded goes out first. A flush that fails is remembered on
// the batch's context (ivx_many_error): the launches it dropped never reach the stream, and whoever waits for their results must say so
int ivx_many_break();
// the sticky error of a failed flush on this context (IVX_OK if none); `clear`: reported now, forget it
int ivx_many_error(ivx_ctx* c, bool clear);
// the context's recorder and its staging ring (ivx_shutdown)
void ivx_many_release(ivx_ctx* c);
// how many flushes (explicit or by a break) this thread's recorder has made: whoever recorded something and later needs it ON the stream
// compares the count at recording time with the count now instead of forcing a flush that may have happened long ago
uint64_t ivx_many_flush_count();
// the next captures belong to object `i` of the batch (chain positions count per object)
void ivx_many_object(uint32_t i);

// zero `bytes` (a multiple of 4) at d_ptr / copy `bytes` (a multiple of 4) from host memory to d_dst: recorded when a batch is being recorded
// on context `c` (true), else the caller issues the stream operation itself
bool ivx_many_zero(const ivx_ctx* c, const void* owner, void* d_ptr, size_t bytes);
bool ivx_many_fill(const ivx_ctx* c, const void* owner, void* d_ptr, uint32_t word, size_t bytes);  // (every 4-byte word of the range = `word`)
bool ivx_many_upload(const ivx_ctx* c, const void* owner, void* d_dst, const void* h_src, size_t bytes);

template <typename A>
static inline bool ivx_many_try(const ivx_ctx* c, const void* owner, int kernel, uint32_t blocks, const A& a) {
    static_assert(sizeof(A) % 8 == 0, "argument blocks are copied as 8-byte words");
    return ivx_many_capture(c, owner, kernel, blocks, &a, (uint32_t)sizeof(A));
}

// (what stands in front of every launch and asynchronous stream operation of the library that has no twin)
#define IVX_KLAUNCH(k, grid, block, shmem, stream, ...)               \
    do {                                                              \
        (void)ivx_many_break();                                       \
        hipLaunchKernelGGL(k, grid, block, shmem, stream, __VA_ARGS__); \
    } while (0)

#ifdef __HIPCC__
// first i with block_end[i] > b (uniform: scalar loads and a scalar loop)
__device__ __forceinline__ uint32_t ivx_many_find(const uint32_t* __restrict__ block_end, uint32_t n, uint32_t b) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (block_end[mid] > b) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}
// A twin is declared ONCE, by its kernel id: the launcher, the registration under that id, the size rule of its argument block and the thread
// count, which the launcher and IVX_MANY_LAUNCH below both read (a twin launched with other threads than its body was written for compiles, runs
// and gives wrong bytes only inside a batch). This form for a twin kernel written by hand (k_clip_many, k_range_many) ...
#define IVX_MANY_REGISTER(ID, twin, ARGS, threads)                                                                                 \
    static_assert(sizeof(ARGS) % 8 == 0, "argument blocks travel as 8-byte words");                                                \
    [[maybe_unused]] constexpr uint32_t ivx_many_threads_##ID = threads;                                                           \
    static int ivx_many_launch_##ID(hipStream_t s, const void* d_argv, const uint32_t* d_block_end, uint32_t n, uint32_t total) {  \
        hipLaunchKernelGGL(twin, dim3(total), dim3(threads), 0, s, static_cast<const ARGS*>(d_argv), d_block_end, n);              \
        return hipGetLastError() == hipSuccess ? 0 : -3;                                                                           \
    }                                                                                                                              \
    static const int ivx_many_registered_##ID = (ivx_many_register(ID, ivx_many_launch_##ID, sizeof(ARGS)), 0);
// ... and the whole of it for a kernel whose body is `BODY(const ARGS&, bid, nb)` (further attributes of the twin behind the thread count).
// The argument block comes by 8-byte words through the scalar cache.
#define IVX_MANY_DECLARE(ID, twin, ARGS, BODY, threads, ...)                                                                               \
    __global__ __launch_bounds__(threads) __VA_ARGS__ void twin(const ARGS* __restrict__ argv, const uint32_t* __restrict__ block_end, uint32_t n) { \
        const uint32_t i = ivx_many_find(block_end, n, blockIdx.x);                                                                        \
        const uint32_t b0 = i ? block_end[i - 1u] : 0u;                                                                                    \
        const ARGS a = argv[i];                                                                                                            \
        BODY(a, blockIdx.x - b0, block_end[i] - b0);                                                                                       \
    }                                                                                                                                      \
    IVX_MANY_REGISTER(ID, twin, ARGS, threads)
// Launch or record: the plain kernel `k` on the context's stream with the thread count declared for ID, unless the launch was written down for
// the flush. For the sites of exactly this shape; the others keep their own code and say why.
#define IVX_MANY_LAUNCH(c, owner, ID, blocks, k, args)                                                                                                       \
    do {                                                                                                                                                     \
        if (!ivx_many_try(c, owner, ID, blocks, args)) IVX_KLAUNCH(k, dim3(blocks), dim3(ivx_many_threads_##ID), 0, (c)->stream, args);                      \
    } while (0)
#endif
