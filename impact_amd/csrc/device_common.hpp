// Host-side pieces the device subsystems (drag.hip, cull.hip, bvol.hip, narrow.hip) and the host units of the C ABI build their state from:
// device buffers that only grow, host-mapped blocks that only grow, the pinned staging block a call's one upload or download goes through, and
// the layout of the parts of one allocation.
#pragma once
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

// parts of one allocation, each on a 256-byte boundary: take all, then add the base
struct ivx_layout {
    size_t bytes = 0;
    size_t take(size_t n) {
        const size_t at = bytes;
        bytes += (n + 255u) & ~(size_t)255u;
        return at;
    }
};

// A pinned host block that only grows. An owner that uploads from it asynchronously creates `staged`, records it behind the upload and sets
// `pending`: the next ivx_staging_for then waits until that upload has left the block. An owner that waits for the stream itself leaves both alone.
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
static inline void ivx_staging_release(ivx_staging* st) {
    if (st->p) (void)hipHostFree(st->p);
    if (st->staged) (void)hipEventDestroy(st->staged);
    *st = ivx_staging();
}
