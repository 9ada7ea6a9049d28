// The hierarchy over a context's bounding-volume set: a linear BVH in Morton order (Karras's construction), and the pair pass through it that leaves
// the bytes of bvol.hip's flat pass.
//
// Reference: impact_intersection/src/bounding_volume/hierarchy.rs (built by hierarchy/fast_bottom_up.rs, driven by
//   impact_physics/src/collision.rs CollisionWorld::cache_all_collisions). The reference clusters bottom-up; its tree shape is unpinned and is not
//   reproduced — what is kept is what it answers: every intersecting pair. include/impact_voxel_hip.h states the rules (frame, key, leaves, nodes);
//   bvol_internal.hpp holds their functions, which ivx_bv_hierarchy_host runs in a loop and the kernels below run a lane each: the same bytes.
//
// FRAME, KEYS — k_bvh_frame, one workgroup: the union (bit order) of the boxes that take a key. k_bvh_keys, a lane per object: (code << 32) | index.
// SORT — a stable LSD radix sort of 64-bit words by chosen bytes, three launches a pass: k_bvh_sort_count (a wave owns SORT_TILE consecutive
//   words and leaves its histogram of the byte), k_bvh_sort_scan (one workgroup: exclusive prefix over [digit][tile], which IS the stable order),
//   k_bvh_sort_scatter (the same wave again: a word's place is its digit's base plus its rank among the wave's equal digits — ballots, in input
//   order). No atomic anywhere. The keys take the four bytes of the code (the input is in index order already); the pairs, read as (b << 32) | a,
//   take the bytes of b and then those of a.
// NODES — k_bvh_nodes, a lane per position: the leaf's object, box and kind in Morton order; Karras's node i: children, parents, and the two
//   skip links of the stackless walk (where a walk goes on behind node i's, or leaf p's, subtree: the node or leaf that starts at the next position).
// REFIT — k_bvh_refit, a lane per leaf, climbs: release, the parent's ticket; the first arriver leaves, the second acquires, loads the sibling's
//   box (vector loads that bypass the L1), stores the union (written through) and climbs on. Nobody waits. The union in the bit order does not
//   depend on who was second.
// WALK — k_bvh_walk<false / true>, a lane per leaf position p: starts at leaf p's skip link — the first subtree to the right of p, so every subtree
//   it sees ends beyond p — and goes on in preorder: into a node whose box does not lie outside the lane's, over it otherwise; at a leaf the kind
//   filter and the box decision. Counts, then k_bvh_scan and the call's one wait, then emits (min, max) of the two objects; the sort above brings
//   the pairs into (a, b) order. A walk takes at most 2 n steps, a climb 64: beyond that the launch sets the error word and the call fails.
// QUERIES — k_bvh_query (described at the kernel): the four kinds of region query through the tree, with the bytes of bvol.hip's flat k_bv_query.
//   Leaves are decided by the flat kernel's own function; a node is skipped only where bvol_internal.hpp's node decision proves that no proper
//   leaf below can be hit in f32; the irregular objects (a NaN bound, lower > upper) are listed by k_bvh_nodes and decided outside the walk.
#include <algorithm>
#include <vector>

#include "bvol_internal.hpp"
#include "device_common.hpp"

namespace {

constexpr uint32_t SORT_TILE = 1024;   // words per wave of the sort
constexpr uint32_t SCAN_ROUND = 1024;  // entries per round of the one-workgroup scans
constexpr uint32_t NONE = 0xFFFFFFFFu;  // a skip link past the last leaf; the root's parent
constexpr uint32_t ERR_REFIT = 1u, ERR_WALK = 2u, ERR_SORT = 4u;

struct Status {  // 16 bytes at the start of the tree buffer, zeroed with the tickets by every build
    unsigned long long grand;
    uint32_t error, n_irregular;  // (n_irregular: the length of the build's list of irregular objects)
};
constexpr uint32_t QUERY_FRONT = 512;   // subtree roots the top expansion of a query holds in LDS (it stops at 256 or more: at most 510)
constexpr uint32_t QUERY_STACK = 1024;  // entries of a workgroup's stack in LDS: the front's share and 256 more per level below it, then lanes walk alone
constexpr uint32_t QUERY_GROUP_LEAVES = 16384, QUERY_MAX_GROUPS = 16;  // workgroups per query: one per so many leaves, at most so many

typedef uint64_t u64;

// ---- device side -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void flag(Status* status, uint32_t what) { __hip_atomic_fetch_or(&status->error, what, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(1024) void k_bvh_frame(const ivx_aabb* __restrict__ world, uint32_t n, ivx_aabb* __restrict__ frame) {
    __shared__ ivx_aabb part[16];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    ivx_aabb f = ivx_bv_neutral_box();
    for (uint32_t i = t; i < n; i += 1024u) {
        const ivx_aabb b = world[i];
        if (!ivx_bv_unkeyed(b)) ivx_bv_union(&f, b);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            f.lower[k] = ivx_bv_order_min(f.lower[k], __shfl_xor(f.lower[k], d, 64));
            f.upper[k] = ivx_bv_order_max(f.upper[k], __shfl_xor(f.upper[k], d, 64));
        }
    if (lane == 0u) part[wv] = f;
    __syncthreads();
    if (t == 0u) {
        for (uint32_t w = 1; w < 16u; ++w) ivx_bv_union(&f, part[w]);
        ivx_bv_frame_finish(&f);
        *frame = f;
    }
}

__global__ __launch_bounds__(256) void k_bvh_keys(const ivx_aabb* __restrict__ world, uint32_t n, const ivx_aabb* __restrict__ frame, u64* __restrict__ keys) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) keys[i] = ivx_bv_key_of(*frame, world[i], i);
}

// the live lanes of the wave that hold the same byte as this one
__device__ __forceinline__ u64 same_digit(uint32_t d, bool live) {
    u64 m = __ballot(live);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = ((d >> b) & 1u) != 0u;
        const u64 with = __ballot(live && bit);
        m &= bit ? with : ~with;
    }
    return m;
}

// hist: [256][n_tiles]
__global__ __launch_bounds__(256) void k_bvh_sort_count(const u64* __restrict__ in, uint32_t n, uint32_t shift, uint32_t n_tiles, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[4][256];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, tile = blockIdx.x * 4u + wv;
    if (tile >= n_tiles) return;  // (whole waves; no workgroup barrier below)
    for (uint32_t k = 0; k < 4u; ++k) h[wv][lane + 64u * k] = 0u;
    __builtin_amdgcn_wave_barrier();
    for (uint32_t r = 0; r < SORT_TILE / 64u; ++r) {
        const uint32_t i = tile * SORT_TILE + r * 64u + lane;
        const bool live = i < n;
        const uint32_t d = live ? (uint32_t)(in[i] >> shift) & 255u : 0u;
        const u64 m = same_digit(d, live);
        if (live && lane == (uint32_t)__ffsll((long long)m) - 1u) h[wv][d] += (uint32_t)__popcll(m);  // (one lane per digit)
        __builtin_amdgcn_wave_barrier();
    }
    for (uint32_t k = 0; k < 4u; ++k) hist[(size_t)(lane + 64u * k) * n_tiles + tile] = h[wv][lane + 64u * k];
}

__global__ __launch_bounds__(SCAN_ROUND) void k_bvh_sort_scan(uint32_t* __restrict__ hist, uint32_t n_entries) {
    __shared__ uint32_t wave_totals[SCAN_ROUND / 64u];
    (void)ivx_scan_rounds<SCAN_ROUND, uint32_t>(hist, hist, n_entries, wave_totals);
}

// base: the scanned histogram. A place past n cannot come from a histogram of the same words: it is dropped and flagged.
__global__ __launch_bounds__(256) void k_bvh_sort_scatter(const u64* __restrict__ in, uint32_t n, uint32_t shift, uint32_t n_tiles, const uint32_t* __restrict__ base,
                                                          u64* __restrict__ out, Status* __restrict__ status) {
    __shared__ uint32_t at[4][256];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, tile = blockIdx.x * 4u + wv;
    if (tile >= n_tiles) return;
    for (uint32_t k = 0; k < 4u; ++k) at[wv][lane + 64u * k] = base[(size_t)(lane + 64u * k) * n_tiles + tile];
    __builtin_amdgcn_wave_barrier();
    const u64 below = (1ull << lane) - 1ull;
    for (uint32_t r = 0; r < SORT_TILE / 64u; ++r) {
        const uint32_t i = tile * SORT_TILE + r * 64u + lane;
        const bool live = i < n;
        const u64 word = live ? in[i] : 0ull;
        const uint32_t d = (uint32_t)(word >> shift) & 255u;
        const u64 m = same_digit(d, live);
        const uint32_t first = live ? at[wv][d] : 0u;
        __builtin_amdgcn_wave_barrier();  // (every lane has read its digit's place before one lane moves it)
        if (live && lane == (uint32_t)__ffsll((long long)m) - 1u) at[wv][d] = first + (uint32_t)__popcll(m);
        __builtin_amdgcn_wave_barrier();
        if (live) {
            const uint32_t place = first + (uint32_t)__popcll(m & below);
            if (place < n) out[place] = word;
            else flag(status, ERR_SORT);
        }
    }
}

// where a preorder walk goes on behind a subtree whose last leaf is `last`: the right child that starts at last + 1 — internal node last + 1 when
// that node's range runs upwards (its index is then the first of its range), else the leaf
__device__ __forceinline__ uint32_t skip_behind(const u64* keys, int n, int last) {
    const int j = last + 1;
    if (j >= n) return NONE;
    if (j <= n - 2 && ivx_bv_delta(keys, n, j, j + 1) - ivx_bv_delta(keys, n, j, j - 1) >= 0) return (uint32_t)j;
    return IVX_BV_LEAF | (uint32_t)j;
}

struct TreeArrays {
    ivx_bv_node* nodes;
    uint32_t *leaf_objects, *leaf_kinds, *leaf_skip, *leaf_parent, *node_skip, *node_parent, *tickets, *irregular;
    ivx_aabb* leaf_boxes;
};

__global__ __launch_bounds__(256) void k_bvh_nodes(const u64* __restrict__ keys, uint32_t n, const ivx_aabb* __restrict__ world, const uint32_t* __restrict__ kinds, TreeArrays t,
                                                   Status* __restrict__ status) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t o = (uint32_t)keys[i];  // (o < n: the keys are a permutation of what k_bvh_keys wrote; checked all the same)
    ivx_aabb b = ivx_bv_neutral_box();
    if (o < n) {
        b = world[o];
        if (ivx_bv_irregular(b)) {  // the queries decide these outside their walk. The list's order is whoever came first: it decides no byte
            const uint32_t at = __hip_atomic_fetch_add(&status->n_irregular, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (at < n) t.irregular[at] = o;
        }
        if (ivx_bv_has_nan(b)) b = ivx_bv_neutral_box();
    }
    t.leaf_objects[i] = o, t.leaf_boxes[i] = b, t.leaf_kinds[i] = o < n ? kinds[o] : IVX_BV_PHANTOM;
    t.leaf_skip[i] = skip_behind(keys, (int)n, (int)i);
    if (i + 1u >= n) return;
    uint32_t left, right, first, last;
    ivx_bv_karras(keys, (int)n, (int)i, &left, &right, &first, &last);
    t.nodes[i].left = left, t.nodes[i].right = right;
    t.node_skip[i] = skip_behind(keys, (int)n, (int)last);
    // (Karras's split lies inside the node's range, so both children lie in [0, n); a link that does not is left out and the refit flags it)
    if ((left & ~IVX_BV_LEAF) < n) (left & IVX_BV_LEAF ? t.leaf_parent[left & ~IVX_BV_LEAF] : t.node_parent[left]) = i;
    if ((right & ~IVX_BV_LEAF) < n) (right & IVX_BV_LEAF ? t.leaf_parent[right & ~IVX_BV_LEAF] : t.node_parent[right]) = i;
    if (i == 0u) t.node_parent[0] = NONE;
}

// The one place where workgroups hand data to each other inside a launch. Producer: the box's stores (written through), an agent-scope release,
// the wait for the stores, then the parent's ticket. Consumer (the second arriver only): an agent-scope acquire, then vector loads of the
// sibling's box that bypass the L1. The first arriver returns: no lane waits for another.
__global__ __launch_bounds__(256) void k_bvh_refit(uint32_t n, TreeArrays t, Status* status) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    ivx_aabb box = t.leaf_boxes[p];  // (written by the launch before: not handed off here)
    uint32_t me = IVX_BV_LEAF | p, cur = t.leaf_parent[p];
    for (int climb = 0; climb < 64; ++climb) {
        if (cur >= n - 1u) break;  // (an inconsistent link: flagged below)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t before = __hip_atomic_fetch_add(&t.tickets[cur], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (before == 0u) return;
        if (before != 1u) break;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        ivx_bv_node* node = t.nodes + cur;
        const uint32_t left = node->left, right = node->right;  // (k_bvh_nodes wrote them)
        const uint32_t sibling = left == me ? right : left;
        ivx_aabb other;
        if (sibling & IVX_BV_LEAF) {
            const uint32_t q = sibling & ~IVX_BV_LEAF;
            if (q >= n) break;
            other = t.leaf_boxes[q];
        } else {
            if (sibling >= n - 1u) break;
            uint32_t* src = reinterpret_cast<uint32_t*>(t.nodes + sibling);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                other.lower[k] = __uint_as_float(__hip_atomic_load(src + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                other.upper[k] = __uint_as_float(__hip_atomic_load(src + 3 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            }
        }
        ivx_bv_union(&box, other);
        uint32_t* dst = reinterpret_cast<uint32_t*>(node);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            __hip_atomic_store(dst + k, __float_as_uint(box.lower[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(dst + 3 + k, __float_as_uint(box.upper[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (cur == 0u) return;
        me = cur, cur = t.node_parent[cur];
    }
    flag(status, ERR_REFIT);
}

// counts: per leaf position; EMIT: its exclusive prefix
template <bool EMIT>
__global__ __launch_bounds__(256) void k_bvh_walk(uint32_t n, uint32_t mode, const ivx_bv_node* __restrict__ nodes, const uint32_t* __restrict__ node_skip,
                                                  const ivx_aabb* __restrict__ leaf_boxes, const uint32_t* __restrict__ leaf_kinds, const uint32_t* __restrict__ leaf_skip,
                                                  const uint32_t* __restrict__ leaf_objects, uint32_t* __restrict__ counts, uint32_t n_pairs, uint2* __restrict__ pairs,
                                                  Status* __restrict__ status) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const ivx_aabb self = leaf_boxes[p];
    const uint32_t row_kind = leaf_kinds[p], row_object = leaf_objects[p];
    const bool row_ok = (mode == 0u) | (row_kind != IVX_BV_PHANTOM);
    uint32_t count = 0u, at = EMIT ? counts[p] : 0u;
    uint32_t cur = row_ok ? leaf_skip[p] : NONE;
    bool sound = true;
    for (uint32_t steps = 0; cur != NONE; ++steps) {
        if (steps >= 2u * n) {
            sound = false;
            break;
        }
        if (cur & IVX_BV_LEAF) {
            const uint32_t q = cur & ~IVX_BV_LEAF;
            if (q >= n) {
                sound = false;
                break;
            }
            const ivx_aabb other = leaf_boxes[q];
            const uint32_t col_kind = leaf_kinds[q];
            const bool kinds_ok = (mode == 0u) | ((col_kind != IVX_BV_PHANTOM) & ((col_kind == IVX_BV_DYNAMIC) | (row_kind == IVX_BV_DYNAMIC)));
            if (kinds_ok && !ivx_bv_lies_outside(self, other)) {
                if (EMIT) {
                    const uint32_t col_object = leaf_objects[q];
                    if (at < n_pairs) pairs[at] = make_uint2(min(row_object, col_object), max(row_object, col_object));
                    else sound = false;
                    ++at;
                } else {
                    ++count;
                }
            }
            cur = leaf_skip[q];
        } else {
            if (cur >= n - 1u) {
                sound = false;
                break;
            }
            const ivx_bv_node node = nodes[cur];
            ivx_aabb box;
            for (int k = 0; k < 3; ++k) box.lower[k] = node.lower[k], box.upper[k] = node.upper[k];
            cur = ivx_bv_lies_outside(self, box) ? node_skip[cur] : node.left;
        }
    }
    if (!sound) flag(status, ERR_WALK);
    if (!EMIT) counts[p] = count;
}

// in place: counts -> exclusive prefix (mod 2^32; the host refuses a grand total of 2^31 or more before anything reads it)
__global__ __launch_bounds__(SCAN_ROUND) void k_bvh_scan(uint32_t* __restrict__ counts, uint32_t n, Status* __restrict__ status) {
    __shared__ uint32_t wave_totals[SCAN_ROUND / 64u];
    const unsigned long long total = ivx_scan_rounds<SCAN_ROUND, unsigned long long>(counts, counts, n, wave_totals);
    if (threadIdx.x == 0u) status->grand = total;
}

__device__ __forceinline__ ivx_aabb box_of(const ivx_bv_node& node) {
    ivx_aabb box;
    for (int k = 0; k < 3; ++k) box.lower[k] = node.lower[k], box.upper[k] = node.upper[k];
    return box;
}
__device__ __forceinline__ void set_hit(unsigned long long* __restrict__ row, uint32_t object) {
    __hip_atomic_fetch_or(row + (object >> 6), 1ull << (object & 63u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void decide_directly(const ivx_bv_query* __restrict__ q, const ivx_aabb* __restrict__ world, uint32_t object, unsigned long long* __restrict__ row) {
    const ivx_aabb b = world[object];
    float c[3], h[3];
    ivx_bv_center_half(b, c, h);
    if (ivx_bv_query_hits(q, b, c, h)) set_hit(row, object);
}

struct QueryTree {  // what a query's walk reads of the tree
    const ivx_bv_node* __restrict__ nodes;
    const uint32_t* __restrict__ node_skip;
    const ivx_aabb* __restrict__ leaf_boxes;
    const uint32_t* __restrict__ leaf_skip;
    const uint32_t* __restrict__ leaf_objects;
};

// the leaf decision at position p < n. The leaf's box is its object's world box, or the neutral box of a NaN-bounded object: an irregular box is
// left to the pass over the build's list. false: the leaf names no object
__device__ __forceinline__ bool query_leaf(uint32_t n, const ivx_bv_query* __restrict__ q, const QueryTree& t, uint32_t p, unsigned long long* __restrict__ row) {
    const ivx_aabb box = t.leaf_boxes[p];
    if (ivx_bv_irregular(box)) return true;
    float c[3], h[3];
    ivx_bv_center_half(box, c, h);
    if (!ivx_bv_query_hits(q, box, c, h)) return true;
    const uint32_t object = t.leaf_objects[p];
    if (object >= n) return false;
    set_hit(row, object);
    return true;
}

// one lane walks the subtree of `start` in preorder without a stack, by k_bvh_walk's skip links, and stops at start's own skip link: every link
// inside a subtree leads to a place inside it or to that one. At most 2 n steps. false: a link points nowhere, or the steps ran out
__device__ bool query_subtree(uint32_t n, const ivx_bv_query* __restrict__ q, const QueryTree& t, uint32_t start, unsigned long long* __restrict__ row) {
    const uint32_t at0 = start & ~IVX_BV_LEAF;
    if (start & IVX_BV_LEAF ? at0 >= n : at0 >= n - 1u) return false;
    const uint32_t end = start & IVX_BV_LEAF ? t.leaf_skip[at0] : t.node_skip[at0];
    uint32_t at = start;
    for (uint32_t steps = 0; at != end && at != NONE; ++steps) {
        if (steps >= 2u * n) return false;
        if (at & IVX_BV_LEAF) {
            const uint32_t p = at & ~IVX_BV_LEAF;
            if (p >= n || !query_leaf(n, q, t, p, row)) return false;
            at = t.leaf_skip[p];
        } else {
            if (at >= n - 1u) return false;
            const ivx_bv_node node = t.nodes[at];
            at = ivx_bv_query_skips_node(q, box_of(node)) ? t.node_skip[at] : node.left;
        }
    }
    return true;
}

// QUERIES — k_bvh_query, `groups` workgroups per query over (query, subtree) items; the masks are zeroed on the stream beforehand and a hit is an
//   agent-scope OR into its word: idempotent and commutative, so the bytes do not depend on who came first, and no workgroup waits for another.
//   The query's record has a workgroup-uniform address (scalar loads).
//   TOP: every workgroup of the query expands the tree from the root breadth-first in LDS, a lane per front entry: a leaf stays, a node the
//     node decision (ivx_bv_query_skips_node) skips is dropped, any other node is replaced by its two children (undecided); places come from a
//     workgroup prefix sum, so the groups hold the same front in the same order. Until the front holds 256 entries or more (at most
//     510 < QUERY_FRONT), or no node. Group g takes entries g, g + groups, ...
//   STACK: the group's entries become a stack in LDS that its 256 lanes work off together, up to 256 entries from the top a round: a leaf is
//     decided (the leaf decision of the flat kernel, ivx_bv_query_hits), a node is dropped or replaced by its children as above. Every entry is
//     popped once and a round pops one at least: at most 2 n rounds, else ERR_WALK. A fully covered subtree is so shared by all lanes, however
//     the front fell. When a round's children would not fit (QUERY_STACK), nothing is pushed and each lane walks the subtree of its node
//     by itself (query_subtree): the stack holds 256 more entries per level it has gone down, so these are the small subtrees at the bottom.
//   IRREGULAR: the objects of the build's list (a NaN bound, lower > upper), which the node decisions do not cover and the walk leaves alone,
//     are decided by every query from their world boxes, shared among its groups. n == 1 has no tree: the one object is decided this way.
__global__ __launch_bounds__(256) void k_bvh_query(uint32_t n, uint32_t groups, const ivx_bv_query* __restrict__ queries, const ivx_aabb* __restrict__ world, QueryTree tree,
                                                   const uint32_t* __restrict__ irregular, uint32_t n_words, unsigned long long* __restrict__ masks,
                                                   Status* __restrict__ status) {
    __shared__ uint32_t front[2][QUERY_FRONT];
    __shared__ uint32_t stack[QUERY_STACK];
    __shared__ uint32_t wave_sums[4];
    const uint32_t t = threadIdx.x, query = blockIdx.x / groups, g = blockIdx.x - query * groups;
    const ivx_bv_query* __restrict__ q = queries + query;
    unsigned long long* __restrict__ row = masks + (size_t)query * n_words;
    if (n == 1u) {
        if (t == 0u && g == 0u) decide_directly(q, world, 0u, row);
        return;
    }
    bool sound = true;
    if (t == 0u) front[0][0] = 0u;  // the root
    __syncthreads();
    uint32_t cur = 0u, m = 1u;
    for (uint32_t round = 0; round < 64u && m < 256u; ++round) {  // (m and every exit are workgroup-uniform)
        const uint32_t ref = t < m ? front[cur][t] : NONE;
        const bool is_node = t < m && !(ref & IVX_BV_LEAF);
        uint32_t keep = t < m ? 1u : 0u, a = ref, b = NONE;
        if (is_node) {
            keep = 0u;
            if (ref < n - 1u) {
                const ivx_bv_node node = tree.nodes[ref];
                if (!ivx_bv_query_skips_node(q, box_of(node))) keep = 2u, a = node.left, b = node.right;
            } else {
                sound = false;
            }
        }
        uint32_t total;  // low half: the entries kept; high half: the nodes this round looked at
        const uint32_t at = ivx_block_prefix(keep | (is_node ? 1u << 16 : 0u), wave_sums, t, total) & 0xFFFFu;
        if (keep >= 1u) front[cur ^ 1u][at] = a;
        if (keep == 2u) front[cur ^ 1u][at + 1u] = b;
        __syncthreads();
        cur ^= 1u, m = total & 0xFFFFu;
        if ((total >> 16) == 0u) break;  // leaves only: nothing left to expand
    }
    uint32_t size = m > g ? (m - g + groups - 1u) / groups : 0u;  // (at most 510 <= QUERY_STACK)
    for (uint32_t i = t; i < size; i += 256u) stack[i] = front[cur][g + i * groups];
    __syncthreads();
    for (uint32_t round = 0; size != 0u; ++round) {  // (size and every exit are workgroup-uniform)
        if (round >= 2u * n) {
            sound = false;
            break;
        }
        const uint32_t take = min(size, 256u), base = size - take;
        const uint32_t ref = t < take ? stack[base + t] : NONE;
        uint32_t keep = 0u, a = NONE, b = NONE;
        if (t < take) {
            const uint32_t at = ref & ~IVX_BV_LEAF;
            if (ref & IVX_BV_LEAF) {
                if (at >= n || !query_leaf(n, q, tree, at, row)) sound = false;
            } else if (at < n - 1u) {
                const ivx_bv_node node = tree.nodes[at];
                if (!ivx_bv_query_skips_node(q, box_of(node))) keep = 2u, a = node.left, b = node.right;
            } else {
                sound = false;
            }
        }
        uint32_t total;
        const uint32_t at = ivx_block_prefix(keep, wave_sums, t, total);  // (its barriers: every lane has read its entry before one is written)
        if (base + total <= QUERY_STACK) {
            if (keep == 2u) stack[base + at] = a, stack[base + at + 1u] = b;
            size = base + total;
        } else {
            if (keep == 2u && !query_subtree(n, q, tree, ref, row)) sound = false;
            size = base;
        }
        __syncthreads();
    }
    const uint32_t n_irregular = min(status->n_irregular, n);
    for (uint32_t i = g * 256u + t; i < n_irregular; i += groups * 256u) {
        const uint32_t object = irregular[i];
        if (object < n) decide_directly(q, world, object, row);
        else sound = false;
    }
    if (!sound) flag(status, ERR_WALK);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
struct BvhState {
    ivx_buf tree;     // status | tickets || frame | keys | keys (the sort's other side) | histogram | nodes | the leaf and node side arrays | irregular objects
    ivx_buf walk;     // counts per leaf position
    ivx_buf sorting;  // the pair sort's other side | its histogram
    bool built = false;
    uint32_t n = 0;
    uint64_t set_serial = 0;  // the set the tree was built from
};

struct TreeLayout {
    size_t o_status = 0, o_tickets = 0, zero_bytes = 0, o_frame = 0, o_keys = 0, o_keys2 = 0, o_hist = 0, o_nodes = 0, o_leaf_objects = 0, o_leaf_boxes = 0, o_leaf_kinds = 0,
           o_leaf_skip = 0, o_leaf_parent = 0, o_node_skip = 0, o_node_parent = 0, o_irregular = 0, bytes = 0;
};
uint32_t tiles_of(size_t n) { return (uint32_t)((n + SORT_TILE - 1u) / SORT_TILE); }
TreeLayout tree_layout(size_t n) {
    ivx_layout l;
    TreeLayout t;
    t.o_status = l.take(sizeof(Status)), t.o_tickets = l.take(n * 4);
    t.zero_bytes = l.bytes;  // (one block from the allocation's start, a multiple of 256 bytes: the build's one memset)
    t.o_frame = l.take(sizeof(ivx_aabb)), t.o_keys = l.take(n * 8), t.o_keys2 = l.take(n * 8), t.o_hist = l.take((size_t)tiles_of(n) * 256u * 4);
    t.o_nodes = l.take(n * sizeof(ivx_bv_node)), t.o_leaf_objects = l.take(n * 4), t.o_leaf_boxes = l.take(n * sizeof(ivx_aabb)), t.o_leaf_kinds = l.take(n * 4);
    t.o_leaf_skip = l.take(n * 4), t.o_leaf_parent = l.take(n * 4), t.o_node_skip = l.take(n * 4), t.o_node_parent = l.take(n * 4);
    t.o_irregular = l.take(n * 4);  // (behind everything the pair pass knows)
    t.bytes = l.bytes;
    return t;
}
TreeArrays tree_arrays(const BvhState* st, const TreeLayout& l) {
    char* d = static_cast<char*>(st->tree.p);
    TreeArrays t;
    t.nodes = reinterpret_cast<ivx_bv_node*>(d + l.o_nodes);
    t.leaf_objects = reinterpret_cast<uint32_t*>(d + l.o_leaf_objects), t.leaf_kinds = reinterpret_cast<uint32_t*>(d + l.o_leaf_kinds);
    t.leaf_skip = reinterpret_cast<uint32_t*>(d + l.o_leaf_skip), t.leaf_parent = reinterpret_cast<uint32_t*>(d + l.o_leaf_parent);
    t.node_skip = reinterpret_cast<uint32_t*>(d + l.o_node_skip), t.node_parent = reinterpret_cast<uint32_t*>(d + l.o_node_parent);
    t.tickets = reinterpret_cast<uint32_t*>(d + l.o_tickets), t.leaf_boxes = reinterpret_cast<ivx_aabb*>(d + l.o_leaf_boxes);
    t.irregular = reinterpret_cast<uint32_t*>(d + l.o_irregular);
    return t;
}

// one pass per entry of `shifts` (an even number of them: the result is back in `a`)
int sort_enqueue(ivx_ctx* c, u64* a, u64* b, uint32_t n, uint32_t* hist, const uint32_t* shifts, int n_shifts, Status* status) {
    const uint32_t n_tiles = tiles_of(n);
    const dim3 grid((n_tiles + 3u) / 4u);
    for (int s = 0; s < n_shifts; ++s) {
        IVX_KLAUNCH(k_bvh_sort_count, grid, dim3(256), 0, c->stream, (const u64*)a, n, shifts[s], n_tiles, hist);
        IVX_KLAUNCH(k_bvh_sort_scan, dim3(1), dim3(SCAN_ROUND), 0, c->stream, hist, n_tiles * 256u);
        IVX_KLAUNCH(k_bvh_sort_scatter, grid, dim3(256), 0, c->stream, (const u64*)a, n, shifts[s], n_tiles, (const uint32_t*)hist, b, status);
        std::swap(a, b);
    }
    IVX_HIP_CHECK(hipGetLastError());
    return IVX_OK;
}

// the context's set and the tree that stands over it (IVX_ERR_STATE: none, or one of an earlier set)
int current_tree(ivx_ctx* c, const char* who, ivx_bvol_view* view, BvhState** out) {
    if (int rc = ivx_bvol_view_of(c, who, view)) return rc;
    BvhState* st = static_cast<BvhState*>(*view->hierarchy);
    IVX_REQUIRE(st && st->built && st->set_serial == view->serial, IVX_ERR_STATE,
                "%s: no hierarchy over the context's current set of bounding volumes (call ivx_bv_build_hierarchy after the set)", who);
    *out = st;
    return IVX_OK;
}

int check_status(const Status& s, const char* who) {
    IVX_REQUIRE(s.error == 0u, IVX_ERR_STATE, "%s: the hierarchy is inconsistent (%s%s%s): a bounded loop ran out or a link points nowhere", who,
                s.error & ERR_REFIT ? "refit " : "", s.error & ERR_WALK ? "walk " : "", s.error & ERR_SORT ? "sort" : "");
    return IVX_OK;
}

// n boxes on the host: the functions of bvol_internal.hpp in a loop
void hierarchy_host(const ivx_aabb* world, size_t n, ivx_bv_node* nodes, uint32_t* leaf_objects, ivx_aabb* frame_out) {
    ivx_aabb frame = ivx_bv_neutral_box();
    for (size_t o = 0; o < n; ++o)
        if (!ivx_bv_unkeyed(world[o])) ivx_bv_union(&frame, world[o]);
    ivx_bv_frame_finish(&frame);
    if (frame_out) *frame_out = frame;
    if (n == 0) return;
    std::vector<uint64_t> keys(n);
    for (size_t o = 0; o < n; ++o) keys[o] = ivx_bv_key_of(frame, world[o], (uint32_t)o);
    std::sort(keys.begin(), keys.end());  // (unique keys: ascending order is the stable order of the codes)
    std::vector<ivx_aabb> leaf_boxes(n);
    for (size_t p = 0; p < n; ++p) {
        leaf_objects[p] = (uint32_t)keys[p];
        leaf_boxes[p] = ivx_bv_has_nan(world[leaf_objects[p]]) ? ivx_bv_neutral_box() : world[leaf_objects[p]];
    }
    if (n < 2) return;
    std::vector<uint32_t> leaf_parent(n), node_parent(n - 1, NONE), tickets(n - 1, 0u);
    for (size_t i = 0; i + 1 < n; ++i) {
        uint32_t left, right, first, last;
        ivx_bv_karras(keys.data(), (int)n, (int)i, &left, &right, &first, &last);
        nodes[i].left = left, nodes[i].right = right;
        for (uint32_t child : {left, right}) (child & IVX_BV_LEAF ? leaf_parent[child & ~IVX_BV_LEAF] : node_parent[child]) = (uint32_t)i;
    }
    // the climb of k_bvh_refit, a leaf after the other: the first arriver at a node leaves, the second stores the union
    for (size_t p = 0; p < n; ++p) {
        ivx_aabb box = leaf_boxes[p];
        uint32_t me = IVX_BV_LEAF | (uint32_t)p, cur = leaf_parent[p];
        for (int climb = 0; climb < 64 && cur != NONE; ++climb) {
            if (tickets[cur]++ == 0u) break;
            const uint32_t sibling = nodes[cur].left == me ? nodes[cur].right : nodes[cur].left;
            ivx_aabb other;
            if (sibling & IVX_BV_LEAF) other = leaf_boxes[sibling & ~IVX_BV_LEAF];
            else
                for (int k = 0; k < 3; ++k) other.lower[k] = nodes[sibling].lower[k], other.upper[k] = nodes[sibling].upper[k];
            ivx_bv_union(&box, other);
            for (int k = 0; k < 3; ++k) nodes[cur].lower[k] = box.lower[k], nodes[cur].upper[k] = box.upper[k];
            me = cur, cur = node_parent[cur];
        }
    }
}

// the queries over a tree the caller brings, with the decisions the kernel runs: a descent from the root with a stack of its own in place of the
// skip links (which are not part of ivx_bv_node), the irregular objects found by a loop. false: the tree is no tree over n leaves
bool queries_host(const ivx_aabb* world, size_t n, const ivx_bv_node* nodes, const uint32_t* leaf_objects, const ivx_bv_query* queries, size_t n_queries, uint64_t* masks) {
    const size_t n_words = (n + 63u) / 64u;
    auto decide_directly = [&](const ivx_bv_query* q, size_t object, uint64_t* row) {
        float c[3], h[3];
        ivx_bv_center_half(world[object], c, h);
        if (ivx_bv_query_hits(q, world[object], c, h)) row[object >> 6] |= 1ull << (object & 63u);
    };
    std::vector<uint32_t> irregular, stack;
    for (size_t o = 0; o < n; ++o)
        if (ivx_bv_irregular(world[o])) irregular.push_back((uint32_t)o);
    for (size_t qi = 0; qi < n_queries; ++qi) {
        const ivx_bv_query* q = queries + qi;
        uint64_t* row = masks + qi * n_words;
        std::fill(row, row + n_words, (uint64_t)0);
        if (n == 1) {
            decide_directly(q, 0, row);
            continue;
        }
        stack.assign(1, 0u);
        for (size_t steps = 0; !stack.empty(); ++steps) {
            if (steps >= 2 * n) return false;
            const uint32_t at = stack.back();
            stack.pop_back();
            if (at & IVX_BV_LEAF) {
                const uint32_t p = at & ~IVX_BV_LEAF;
                if (p >= n || leaf_objects[p] >= n) return false;
                const uint32_t object = leaf_objects[p];
                if (!ivx_bv_irregular(world[object])) decide_directly(q, object, row);
            } else {
                if (at >= n - 1) return false;
                ivx_aabb box;
                for (int k = 0; k < 3; ++k) box.lower[k] = nodes[at].lower[k], box.upper[k] = nodes[at].upper[k];
                if (!ivx_bv_query_skips_node(q, box)) stack.push_back(nodes[at].right), stack.push_back(nodes[at].left);
            }
        }
        for (uint32_t object : irregular) decide_directly(q, object, row);
    }
    return true;
}

}  // namespace

void ivx_bvh_release(void** hierarchy) {
    BvhState* s = ivx_state_take<BvhState>(hierarchy);
    if (!s) return;
    for (ivx_buf* b : {&s->tree, &s->walk, &s->sorting}) ivx_buf_free(b);
    delete s;
}

void* ivx_bvh_device_ptr(void* hierarchy, uint64_t set_serial, int which) {
    BvhState* st = static_cast<BvhState*>(hierarchy);
    if (!st || !st->built || st->set_serial != set_serial || st->n < 2u) return nullptr;
    const TreeLayout l = tree_layout(st->n);
    char* d = static_cast<char*>(st->tree.p);
    return which == IVX_BV_PTR_NODES ? d + l.o_nodes : (which == IVX_BV_PTR_LEAF_OBJECTS ? d + l.o_leaf_objects : nullptr);
}

int ivx_bvh_build_enqueue(ivx_ctx* c, const char* who) {
    ivx_bvol_view view;
    if (int rc = ivx_bvol_view_of(c, who, &view)) return rc;
    BvhState* st;
    if (int rc = ivx_state_for(view.hierarchy, who, &st)) return rc;
    st->built = false;  // (until this call's tree stands)
    const uint32_t n = view.n;
    if (n >= 2u) {
        const TreeLayout l = tree_layout(n);
        if (int rc = ivx_buf_grow(c, &st->tree, l.bytes, 1u << 16)) return rc;
        char* d = static_cast<char*>(st->tree.p);
        const TreeArrays t = tree_arrays(st, l);
        Status* status = reinterpret_cast<Status*>(d + l.o_status);
        ivx_aabb* frame = reinterpret_cast<ivx_aabb*>(d + l.o_frame);
        u64* keys = reinterpret_cast<u64*>(d + l.o_keys);
        const dim3 lanes((n + 255u) / 256u);
        IVX_HIP_CHECK(ivx_memset_async(d, 0, l.zero_bytes, c->stream));
        IVX_KLAUNCH(k_bvh_frame, dim3(1), dim3(1024), 0, c->stream, view.world, n, frame);
        IVX_KLAUNCH(k_bvh_keys, lanes, dim3(256), 0, c->stream, view.world, n, (const ivx_aabb*)frame, keys);
        static const uint32_t code_bytes[4] = {32u, 40u, 48u, 56u};
        if (int rc = sort_enqueue(c, keys, reinterpret_cast<u64*>(d + l.o_keys2), n, reinterpret_cast<uint32_t*>(d + l.o_hist), code_bytes, 4, status)) return rc;
        IVX_KLAUNCH(k_bvh_nodes, lanes, dim3(256), 0, c->stream, (const u64*)keys, n, view.world, view.kinds, t, status);
        IVX_KLAUNCH(k_bvh_refit, lanes, dim3(256), 0, c->stream, n, t, status);
        IVX_HIP_CHECK(hipGetLastError());
    }
    st->n = n, st->set_serial = view.serial, st->built = true;
    return IVX_OK;
}

int ivx_bvh_pairs_enqueue(ivx_ctx* c, const char* who, uint32_t mode, bool check_cap, size_t cap, size_t* n_pairs) {
    *n_pairs = 0;
    ivx_bvol_view view;
    BvhState* st;
    if (int rc = current_tree(c, who, &view, &st)) return rc;
    const uint32_t n = st->n;
    if (n < 2u) return IVX_OK;
    const TreeLayout l = tree_layout(n);
    const TreeArrays t = tree_arrays(st, l);
    Status* d_status = reinterpret_cast<Status*>(static_cast<char*>(st->tree.p) + l.o_status);
    if (int rc = ivx_buf_grow(c, &st->walk, (size_t)n * 4, 1u << 16)) return rc;
    uint32_t* d_counts = static_cast<uint32_t*>(st->walk.p);
    const dim3 lanes((n + 255u) / 256u);
    IVX_KLAUNCH(k_bvh_walk<false>, lanes, dim3(256), 0, c->stream, n, mode, (const ivx_bv_node*)t.nodes, (const uint32_t*)t.node_skip, (const ivx_aabb*)t.leaf_boxes,
                (const uint32_t*)t.leaf_kinds, (const uint32_t*)t.leaf_skip, (const uint32_t*)t.leaf_objects, d_counts, 0u, (uint2*)nullptr, d_status);
    IVX_KLAUNCH(k_bvh_scan, dim3(1), dim3(SCAN_ROUND), 0, c->stream, d_counts, n, d_status);
    IVX_HIP_CHECK(hipGetLastError());
    Status status = {};
    IVX_HIP_CHECK(ivx_memcpy_async(&status, d_status, sizeof(Status), hipMemcpyDeviceToHost, c->stream));
    IVX_HIP_CHECK(ivx_stream_sync(c->stream));
    if (int rc = check_status(status, who)) return rc;
    const unsigned long long grand = status.grand;
    if (int rc = ivx_bvol_pairs_total(who, grand, check_cap, cap, n_pairs)) return rc;
    if (grand == 0) return IVX_OK;
    ivx_layout s;
    const size_t o_other = s.take((size_t)grand * 8), o_hist = s.take((size_t)tiles_of((size_t)grand) * 256u * 4);
    if (int rc = ivx_buf_grow(c, view.pairs, (size_t)grand * 8, 1u << 16)) return rc;
    if (int rc = ivx_buf_grow(c, &st->sorting, s.bytes, 1u << 16)) return rc;
    IVX_KLAUNCH(k_bvh_walk<true>, lanes, dim3(256), 0, c->stream, n, mode, (const ivx_bv_node*)t.nodes, (const uint32_t*)t.node_skip, (const ivx_aabb*)t.leaf_boxes,
                (const uint32_t*)t.leaf_kinds, (const uint32_t*)t.leaf_skip, (const uint32_t*)t.leaf_objects, d_counts, (uint32_t)grand, static_cast<uint2*>(view.pairs->p), d_status);
    // a pair in memory is the word (b << 32) | a: the bytes of b first, then those of a (as many as n - 1 has)
    uint32_t shifts[8];
    int n_shifts = 0, index_bytes = 1;
    while (index_bytes < 4 && ((n - 1u) >> (8 * index_bytes)) != 0u) ++index_bytes;
    for (int k = 0; k < index_bytes; ++k) shifts[n_shifts++] = 32u + 8u * (uint32_t)k;
    for (int k = 0; k < index_bytes; ++k) shifts[n_shifts++] = 8u * (uint32_t)k;
    char* sd = static_cast<char*>(st->sorting.p);
    return sort_enqueue(c, static_cast<u64*>(view.pairs->p), reinterpret_cast<u64*>(sd + o_other), (uint32_t)grand, reinterpret_cast<uint32_t*>(sd + o_hist), shifts, n_shifts, d_status);
}

extern "C" {

int ivx_bv_morton_key(const ivx_aabb* frame, const ivx_aabb* box, uint32_t index, uint64_t* key) {
    IVX_REQUIRE(frame && box && key, IVX_ERR_INVALID, "ivx_bv_morton_key: null argument");
    *key = ivx_bv_key_of(*frame, *box, index);
    return IVX_OK;
}

int ivx_bv_hierarchy_host(const ivx_aabb* world, size_t n, ivx_bv_node* nodes, uint32_t* leaf_objects, ivx_aabb* frame) {
    const char* who = "ivx_bv_hierarchy_host";
    IVX_REQUIRE(n <= IVX_BV_MAX_OBJECTS, IVX_ERR_CAPACITY, "%s: %zu objects exceed %u", who, n, IVX_BV_MAX_OBJECTS);
    IVX_REQUIRE((world && leaf_objects) || n == 0, IVX_ERR_INVALID, "%s: null argument", who);
    IVX_REQUIRE(nodes || n < 2, IVX_ERR_INVALID, "%s: null node buffer", who);
    hierarchy_host(world, n, nodes, leaf_objects, frame);
    return IVX_OK;
}

int ivx_bv_build_hierarchy(ivx_ctx* c) {
    const char* who = "ivx_bv_build_hierarchy";
    IVX_REQUIRE(c, IVX_ERR_INVALID, "%s: null context", who);
    ivx_many_other_context other_(c);
    return ivx_bvh_build_enqueue(c, who);
}

int ivx_bv_hierarchy_download(ivx_ctx* c, ivx_bv_node* nodes, size_t node_cap, uint32_t* leaf_objects, size_t leaf_cap, size_t* n_nodes) {
    const char* who = "ivx_bv_hierarchy_download";
    if (n_nodes) *n_nodes = 0;
    IVX_REQUIRE(c, IVX_ERR_INVALID, "%s: null context", who);
    ivx_bvol_view view;
    BvhState* st;
    if (int rc = current_tree(c, who, &view, &st)) return rc;
    const uint32_t n = st->n, nn = n >= 2u ? n - 1u : 0u;
    if (n_nodes) *n_nodes = nn;
    IVX_REQUIRE(!nodes || node_cap >= nn, IVX_ERR_CAPACITY, "%s: the hierarchy has %u nodes, the buffer holds %zu", who, nn, node_cap);
    IVX_REQUIRE(!leaf_objects || leaf_cap >= n, IVX_ERR_CAPACITY, "%s: the hierarchy has %u leaves, the buffer holds %zu", who, n, leaf_cap);
    if (n == 1u && leaf_objects) leaf_objects[0] = 0u;
    if (n < 2u) return IVX_OK;
    ivx_many_other_context other_(c);
    const TreeLayout l = tree_layout(n);
    const char* d = static_cast<const char*>(st->tree.p);
    Status status = {};
    if (nodes) IVX_HIP_CHECK(ivx_memcpy_async(nodes, d + l.o_nodes, (size_t)nn * sizeof(ivx_bv_node), hipMemcpyDeviceToHost, c->stream));
    if (leaf_objects) IVX_HIP_CHECK(ivx_memcpy_async(leaf_objects, d + l.o_leaf_objects, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    IVX_HIP_CHECK(ivx_memcpy_async(&status, d + l.o_status, sizeof(Status), hipMemcpyDeviceToHost, c->stream));
    IVX_HIP_CHECK(ivx_stream_sync(c->stream));
    return check_status(status, who);
}

int ivx_bv_pairs_hierarchy(ivx_ctx* c, uint32_t mode, uint32_t* pairs, size_t cap, size_t* n_out) {
    const char* who = "ivx_bv_pairs_hierarchy";
    if (int rc = ivx_bvol_pairs_check(who, c, mode, pairs, cap, n_out)) return rc;
    ivx_bvol_view view;
    BvhState* st;
    if (int rc = current_tree(c, who, &view, &st)) return rc;
    if (st->n < 2u) return IVX_OK;
    ivx_many_other_context other_(c);
    if (int rc = ivx_bvh_pairs_enqueue(c, who, mode, pairs != nullptr, cap, n_out)) return rc;
    if (*n_out == 0) return IVX_OK;
    const TreeLayout l = tree_layout(st->n);
    Status status = {};
    if (pairs) IVX_HIP_CHECK(ivx_memcpy_async(pairs, view.pairs->p, *n_out * 8, hipMemcpyDeviceToHost, c->stream));
    IVX_HIP_CHECK(ivx_memcpy_async(&status, static_cast<const char*>(st->tree.p) + l.o_status, sizeof(Status), hipMemcpyDeviceToHost, c->stream));
    IVX_HIP_CHECK(ivx_stream_sync(c->stream));
    return check_status(status, who);
}

int ivx_bv_query_skips_boxes(const ivx_bv_query* queries, size_t n_queries, const ivx_aabb* boxes, size_t n_boxes, uint8_t* skips) {
    const char* who = "ivx_bv_query_skips_boxes";
    IVX_REQUIRE((queries && boxes && skips) || n_queries == 0 || n_boxes == 0, IVX_ERR_INVALID, "%s: null argument", who);
    if (n_boxes != 0)
        if (int rc = ivx_bvol_query_kinds_check(who, queries, n_queries)) return rc;
    for (size_t q = 0; q < n_queries; ++q)
        for (size_t b = 0; b < n_boxes; ++b) skips[q * n_boxes + b] = ivx_bv_query_skips_node(queries + q, boxes[b]) ? 1u : 0u;
    return IVX_OK;
}

int ivx_bv_queries_hierarchy_host(const ivx_aabb* world, size_t n, const ivx_bv_node* nodes, const uint32_t* leaf_objects, const ivx_bv_query* queries, size_t n_queries,
                                  uint64_t* masks, uint32_t* counts) {
    const char* who = "ivx_bv_queries_hierarchy_host";
    IVX_REQUIRE(n <= IVX_BV_MAX_OBJECTS, IVX_ERR_CAPACITY, "%s: %zu objects exceed %u", who, n, IVX_BV_MAX_OBJECTS);
    IVX_REQUIRE(n_queries <= IVX_BV_MAX_QUERIES, IVX_ERR_CAPACITY, "%s: %zu queries exceed %u per call", who, n_queries, IVX_BV_MAX_QUERIES);
    IVX_REQUIRE(queries || n_queries == 0, IVX_ERR_INVALID, "%s: null queries", who);
    if (int rc = ivx_bvol_query_kinds_check(who, queries, n_queries)) return rc;
    IVX_REQUIRE((world && leaf_objects) || n == 0, IVX_ERR_INVALID, "%s: null argument", who);
    IVX_REQUIRE(nodes || n < 2, IVX_ERR_INVALID, "%s: null node buffer", who);
    if (n_queries == 0) return IVX_OK;
    if (n == 0) {
        for (size_t q = 0; q < n_queries && counts; ++q) counts[q] = 0u;
        return IVX_OK;
    }
    IVX_REQUIRE(masks, IVX_ERR_INVALID, "%s: null mask buffer", who);
    IVX_REQUIRE(queries_host(world, n, nodes, leaf_objects, queries, n_queries, masks), IVX_ERR_STATE,
                "%s: the hierarchy is inconsistent: a walk ran past its %zu steps or a link points nowhere", who, 2 * n);
    const size_t n_words = (n + 63u) / 64u;
    for (size_t q = 0; q < n_queries && counts; ++q) {
        uint32_t hit = 0u;
        for (size_t w = 0; w < n_words; ++w) hit += (uint32_t)__builtin_popcountll(masks[q * n_words + w]);
        counts[q] = hit;
    }
    return IVX_OK;
}

int ivx_bv_queries_hierarchy(ivx_ctx* c, const ivx_bv_query* queries, size_t n_queries, uint64_t* masks, uint32_t* counts) {
    const char* who = "ivx_bv_queries_hierarchy";
    if (int rc = ivx_bvol_queries_check(who, c, queries, n_queries)) return rc;
    ivx_bvol_view view;
    BvhState* st;
    if (int rc = current_tree(c, who, &view, &st)) return rc;
    ivx_bvol_query_run run;
    if (n_queries == 0 || st->n == 0u) {  // (nothing reaches the stream)
        if (int rc = ivx_bvol_queries_begin(c, who, queries, n_queries, masks, &run)) return rc;
        return ivx_bvol_queries_finish(c, run, masks, counts);
    }
    IVX_REQUIRE(masks, IVX_ERR_INVALID, "%s: null mask buffer", who);
    ivx_many_other_context other_(c);
    if (int rc = ivx_bvol_queries_begin(c, who, queries, n_queries, masks, &run)) return rc;
    IVX_HIP_CHECK(ivx_memset_async(run.d_masks, 0, run.mask_bytes, c->stream));
    const uint32_t n = st->n;
    TreeArrays t = {};
    Status* d_status = nullptr;
    if (n >= 2u) {
        const TreeLayout l = tree_layout(n);
        t = tree_arrays(st, l);
        d_status = reinterpret_cast<Status*>(static_cast<char*>(st->tree.p) + l.o_status);
    }
    const QueryTree tree = {t.nodes, t.node_skip, t.leaf_boxes, t.leaf_skip, t.leaf_objects};
    const uint32_t groups = std::min(std::max(n / QUERY_GROUP_LEAVES, 1u), QUERY_MAX_GROUPS);
    IVX_KLAUNCH(k_bvh_query, dim3(run.n_queries * groups), dim3(256), 0, c->stream, n, groups, run.d_queries, view.world, tree, (const uint32_t*)t.irregular, run.n_words, run.d_masks,
                d_status);
    IVX_HIP_CHECK(hipGetLastError());
    Status status = {};
    if (d_status) IVX_HIP_CHECK(ivx_memcpy_async(&status, d_status, sizeof(Status), hipMemcpyDeviceToHost, c->stream));
    if (int rc = ivx_bvol_queries_finish(c, run, masks, counts)) return rc;  // (the call's one wait)
    return check_status(status, who);
}

}  // extern "C"
