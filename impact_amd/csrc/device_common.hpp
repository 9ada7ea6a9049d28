// Host-side pieces the device subsystems (drag.hip, cull.hip, bvol.hip, narrow.hip) and the host units of the C ABI build their state from:
// device buffers that only grow, host-mapped blocks that only grow, the pinned staging block a call's one upload or download goes through, and
// the layout of the parts of one allocation.
#pragma once
#include <new>

#include "ivx_internal.hpp"

// `b` holds at least `bytes` afterwards. A buffer that has to grow waits for the stream first (what is in flight may still read the old one) and
// does not keep its contents; it grows to 3/2 of what was asked for, at least `floor_bytes`.
static inline int ivx_buf_grow(ivx_ctx* c, ivx_buf* b, size_t bytes, size_t floor_bytes) {
    if (b->bytes >= bytes) return IVX_OK;
    IVX_HIP_CHECK(ivx_stream_sync(c->stream));
    if (b->p) (void)hipFree(b->p);
    b->p = nullptr, b->bytes = 0;
    bytes = bytes + bytes / 2;
    if (bytes < floor_bytes) bytes = floor_bytes;
    IVX_HIP_CHECK(hipMalloc(&b->p, bytes));
    b->bytes = bytes;
    return IVX_OK;
}
static inline void ivx_buf_free(ivx_buf* b) {
    if (b->p) (void)hipFree(b->p);
    b->p = nullptr, b->bytes = 0;
}

// A typed device array that only grows: a pointer and a capacity in elements. `grow`: at least `need` elements afterwards; an array that has
// to grow waits for the stream first, does not keep its contents and becomes max(need, twice what it was). (ivx_dev_grow is the same on an
// array known by its element size only: a table of arrays of several types walks them with it.)
static inline int ivx_dev_grow(void** p, size_t* cap, size_t elem_bytes, size_t need, hipStream_t s) {
    if (need <= *cap) return IVX_OK;
    const size_t ncap = need > *cap * 2 ? need : *cap * 2;
    IVX_HIP_CHECK(ivx_stream_sync(s));
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    IVX_HIP_CHECK(hipMalloc(p, ncap * elem_bytes));
    *cap = ncap;
    return IVX_OK;
}
template <class T>
struct ivx_dev_array {
    T* p = nullptr;
    size_t cap = 0;
    int grow(hipStream_t s, size_t need) { return ivx_dev_grow(reinterpret_cast<void**>(&p), &cap, sizeof(T), need, s); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr, cap = 0;
    }
};

// `m` holds at least `bytes` afterwards. A block that has to grow does not keep its contents and is made `want` bytes (the owner's growth
// rule, at least `bytes`); `wait` non-null: what is in flight on that stream may still use the old block and is waited for first.
static inline void ivx_mapped_free(ivx_mapped* m) {
    if (m->p) (void)hipHostFree(m->p);
    *m = ivx_mapped();
}
static inline int ivx_mapped_grow(ivx_mapped* m, size_t bytes, size_t want, hipStream_t wait) {
    if (m->bytes >= bytes) return IVX_OK;
    if (wait) IVX_HIP_CHECK(ivx_stream_sync(wait));
    ivx_mapped_free(m);
    IVX_HIP_CHECK(hipHostMalloc(&m->p, want, hipHostMallocMapped));
    IVX_HIP_CHECK(hipHostGetDevicePointer(&m->dev, m->p, 0));
    m->bytes = want;
    return IVX_OK;
}

// parts of one allocation, each on a 256-byte boundary (or another power of two: `align`): take all, then add the base
struct ivx_layout {
    size_t bytes = 0;
    size_t align = 256;
    size_t take(size_t n) {
        const size_t at = bytes;
        bytes += (n + align - 1) & ~(align - 1);
        return at;
    }
};

// A pinned host block that only grows, and the two ways an owner uses it:
//   asynchronous  ivx_staging_for, fill the block, ivx_staging_upload (one copy from the block's start) — or copies of the owner's own from offsets
//                 of the block and ivx_staging_sent behind the last of them. The next ivx_staging_for waits until that upload has left the block.
//   synchronous   ivx_staging_for alone: the owner waits for the stream itself before it touches the block again, and never calls `sent`.
// `staged` and `pending` belong to ivx_staging_sent and ivx_staging_for; no owner writes them.
struct ivx_staging {
    void* p = nullptr;
    size_t bytes = 0;
    hipEvent_t staged = nullptr;
    bool pending = false;
};
static inline int ivx_staging_for(ivx_staging* st, size_t bytes) {
    if (st->pending) {
        IVX_HIP_CHECK(hipEventSynchronize(st->staged));
        st->pending = false;
    }
    if (st->bytes >= bytes) return IVX_OK;
    if (st->p) (void)hipHostFree(st->p);
    st->p = nullptr, st->bytes = 0;
    bytes = bytes + bytes / 2;
    if (bytes < (1u << 16)) bytes = 1u << 16;
    IVX_HIP_CHECK(hipHostMalloc(&st->p, bytes, hipHostMallocDefault));
    st->bytes = bytes;
    return IVX_OK;
}
// the copies out of the block have just been enqueued on `s`: the event behind them (made on first use) says when the block is free again
static inline int ivx_staging_sent(ivx_staging* st, hipStream_t s) {
    if (!st->staged) IVX_HIP_CHECK(hipEventCreateWithFlags(&st->staged, hipEventDisableTiming));
    IVX_HIP_CHECK(ivx_event_record(st->staged, s));
    st->pending = true;
    return IVX_OK;
}
// the first `bytes` of the block to `dst` on the device
static inline int ivx_staging_upload(ivx_staging* st, void* dst, size_t bytes, hipStream_t s) {
    IVX_HIP_CHECK(ivx_memcpy_async(dst, st->p, bytes, hipMemcpyHostToDevice, s));
    return ivx_staging_sent(st, s);
}
static inline void ivx_staging_release(ivx_staging* st) {
    if (st->p) (void)hipHostFree(st->p);
    if (st->staged) (void)hipEventDestroy(st->staged);
    *st = ivx_staging();
}

// The record a subsystem hangs off a `void*` slot of the context or the world. `for`: the record in the slot, made (value-initialised) on first
// use; `what` names the owner in the one out-of-memory message. `take`: the record leaves the slot (null: there was none) — the owner's release
// function frees its members and deletes it.
template <class S>
static inline int ivx_state_for(void** slot, const char* what, S** out) {
    if (!*slot) {
        S* s = new (std::nothrow) S();
        IVX_REQUIRE(s, IVX_ERR_CAPACITY, "%s: out of host memory", what);
        *slot = s;
    }
    *out = static_cast<S*>(*slot);
    return IVX_OK;
}
template <class S>
static inline S* ivx_state_take(void** slot) {
    S* s = static_cast<S*>(*slot);
    *slot = nullptr;
    return s;
}

// ---- store forms of the device code -------------------------------------------------------------------------------------------------------
// What a store says about the line it writes (gfx950; MI355X_MICROARCH.md, visibility): a PLAIN store leaves it dirty in the XCD's L2 until
// something writes it back — at the latest the end of the launch, when the chip waits for every dirty line of every L2 —; NT marks it as
// streaming but still leaves it in the L2 ("nt is not write-through"); WT (sc1) writes it through as it is made and drops it from the L2, so
// a reader on the same XCD fetches it from the memory side again; WT_NT is both. A kernel's output stream takes ONE policy, a -D macro at its
// store site (tools/build_variant.sh builds the variants side by side); the values stored are the same under every policy.
//
// Forms. Plain and NT are the compiler's own stores. WT of 8 bytes or fewer is the relaxed agent-scope atomic store (global_store ... sc1,
// counted by the compiler's waits like any store). WT of 16 bytes has no builtin on a global address: it is the instruction itself, which
// costs no scalar registers (a buffer resource is four per plane; the evaluator has none to spare) but is NOT counted by the compiler's
// s_waitcnt — use it only for bytes that nobody reads again in the same launch. (`s_nop 1`: the data registers of a store wider than 64 bits
// may not be overwritten in the two states after it.) The buffer form, for code that holds a resource anyway, is counted; its offset is 32 bits
// and a store beyond the resource's range is dropped, so the host sizes the resource and keeps planes that do not fit it on the global forms.
#define IVX_ST_PLAIN 0
#define IVX_ST_NT 1
#define IVX_ST_WT 2
#define IVX_ST_WT_NT 3
typedef unsigned int ivx_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int ivx_u32x2 __attribute__((ext_vector_type(2)));

template <int POL>
__device__ __forceinline__ void ivx_st16(void* p, uint4 v) {
    ivx_u32x4 x;
    x.x = v.x, x.y = v.y, x.z = v.z, x.w = v.w;
    if constexpr (POL == IVX_ST_PLAIN) *reinterpret_cast<uint4*>(p) = v;
    else if constexpr (POL == IVX_ST_NT) __builtin_nontemporal_store(x, reinterpret_cast<ivx_u32x4*>(p));
    else if constexpr (POL == IVX_ST_WT) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(x) : "memory");
    else asm volatile("global_store_dwordx4 %0, %1, off sc1 nt\n\ts_nop 1" ::"v"(p), "v"(x) : "memory");
}
template <int POL>
__device__ __forceinline__ void ivx_st8(void* p, uint2 v) {
    ivx_u32x2 x;
    x.x = v.x, x.y = v.y;
    const unsigned long long u = (unsigned long long)v.x | ((unsigned long long)v.y << 32);
    if constexpr (POL == IVX_ST_PLAIN) *reinterpret_cast<uint2*>(p) = v;
    else if constexpr (POL == IVX_ST_NT) __builtin_nontemporal_store(x, reinterpret_cast<ivx_u32x2*>(p));
    else if constexpr (POL == IVX_ST_WT) __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else asm volatile("global_store_dwordx2 %0, %1, off sc1 nt" ::"v"(p), "v"(x) : "memory");
}
template <int POL>
__device__ __forceinline__ void ivx_st4(void* p, uint32_t v) {
    if constexpr (POL == IVX_ST_PLAIN) *reinterpret_cast<uint32_t*>(p) = v;
    else if constexpr (POL == IVX_ST_NT) __builtin_nontemporal_store(v, reinterpret_cast<uint32_t*>(p));
    else if constexpr (POL == IVX_ST_WT) __hip_atomic_store(reinterpret_cast<uint32_t*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else asm volatile("global_store_dword %0, %1, off sc1 nt" ::"v"(p), "v"(v) : "memory");
}
template <int POL>
__device__ __forceinline__ void ivx_st4(float* p, float v) { ivx_st4<POL>(static_cast<void*>(p), __float_as_uint(v)); }
template <int POL>
__device__ __forceinline__ void ivx_st4(uint32_t* p, uint32_t v) { ivx_st4<POL>(static_cast<void*>(p), v); }
template <int POL>
__device__ __forceinline__ void ivx_st2(void* p, uint16_t v) {
    if constexpr (POL == IVX_ST_PLAIN) *reinterpret_cast<uint16_t*>(p) = v;
    else if constexpr (POL == IVX_ST_NT) __builtin_nontemporal_store(v, reinterpret_cast<uint16_t*>(p));
    else if constexpr (POL == IVX_ST_WT) __hip_atomic_store(reinterpret_cast<uint16_t*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else asm volatile("global_store_short %0, %1, off sc1 nt" ::"v"(p), "v"((uint32_t)v) : "memory");
}
// the buffer form: `aux` 2 = nt, 16 = sc1
template <int POL>
__device__ __forceinline__ void ivx_st16_buf(__amdgpu_buffer_rsrc_t rs, uint32_t byte_off, ivx_u32x4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(v, rs, (int)byte_off, 0, (POL & 1 ? 2 : 0) | (POL & 2 ? 16 : 0));
}
// (the solver's hand-off store, physics.hip: write-through, so that another workgroup anywhere on the chip reads it back with an sc1 load)
__device__ __forceinline__ void st16_sc1(__amdgpu_buffer_rsrc_t rs, uint32_t byte_off, float4 f) {
    ivx_u32x4 v;
    v.x = __float_as_uint(f.x), v.y = __float_as_uint(f.y), v.z = __float_as_uint(f.z), v.w = __float_as_uint(f.w);
    ivx_st16_buf<IVX_ST_WT>(rs, byte_off, v);
}
