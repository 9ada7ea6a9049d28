// The world's host bookkeeping (impact_amd/csrc/contact_schedule.hpp) checked on the host, without the HIP runtime:
//   contact_schedule_check scenarios        small cases with the expected arrays written out by hand (tests/test_contact_schedule_cpu.py)
//   contact_schedule_check random N [seed]  N random sequences of frames through the struct and through a transcription of what it replaced —
//                                           the functions of physics_api.hip and the host part of ivx_world_set_contacts, ivx_world_ensure_form
//                                           and ivx_world_step as they stood before the world became a unit of its own, on a plain struct
//                                           with the field names they had — compared after every operation
// Build: g++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/contact_schedule_check.cpp impact_amd/csrc/contact_schedule.cpp -o contact_schedule_check
// -DSEED_FAULT=1..4 plants a fault in the TRANSCRIPTION (1: swap-remove without the id table's fix-up, 2: a chain cap of 5, 3: a kinematic
// body raises a level, 4: the rank not shifted in cs_vers); `random` must then report a difference.
#include <cstring>
#include <initializer_list>
#include <random>

#include "../impact_amd/csrc/contact_schedule.hpp"

#ifndef SEED_FAULT
#define SEED_FAULT 0
#endif

typedef std::vector<uint32_t> U32s;
typedef void (*PositionOf)(uint32_t ref, float out[3]);
static void position_of(uint32_t ref, float out[3]) {  // synthetic body positions: a function of the reference alone
    const uint32_t i = ref & 0x7FFFFFFFu, k = (ref >> 31) * 17u;
    out[0] = 0.37f * (float)(i % 7u) - 0.5f * (float)k, out[1] = 0.21f * (float)(i % 5u) + 0.1f * (float)k, out[2] = 0.11f * (float)i - 1.0f;
}
enum { SET_OK = 0, SET_MISSING_BODY, SET_SELF_PAIR };
struct SetResult {
    int code = SET_OK;
    size_t bad = 0;
    bool fast = false;
    uint32_t nc = 0;
};
inline bool operator==(const ivx_contact& a, const ivx_contact& b) { return memcmp(&a, &b, sizeof a) == 0; }

// ---- what the struct replaced, with its field and function names ------------------------------------------------------------------------
namespace old {
struct World {
    ivx_solver_config cfg{};
    uint32_t n_dyn = 0, n_kin = 0, n_contacts = 0, n_prev = 0;
    int schedule_valid = 0;
    struct Entry {
        uint64_t id;
        int32_t prev_slot;
        uint32_t src;
        bool prepared;
    };
    std::vector<Entry> cache;
    std::vector<uint64_t> id_keys;
    U32s id_vals;
    size_t id_used = 0;
    std::vector<ivx_contact> effective, stage_contacts;
    size_t stage_contacts_cap = 0;
    std::vector<int32_t> prev_slot_host;
    U32s slot_bodies, chain_start, chain_bodies, prev_chain_start, prev_chain_bodies, lvl_host[2], level_start_host, cs_slot_of_level;
    U32s items_host, item_bodies_host, item_tags_host, tile_base_host, tile_first_host, kin_offsets_host, kin_list_host;
    U32s cs_item_host, cs_bodies_host, cs_vers_host, cs_round_start_host, cs_round_level_host, cs_slot_of_host;
    std::vector<uint64_t> cs_round_mask_host, scratch_mask, scratch_bits;
    U32s scratch_count, scratch_last, scratch_rank, scratch_order, scratch_first, joint_refs_host;
    uint32_t n_levels[2] = {}, item_offset[2] = {}, level_offset[2] = {}, max_level_items[2] = {}, n_tiles[2] = {}, tile_offset[2] = {}, phase_items[2] = {};
    int cs_feasible[2] = {};
    uint32_t forms_built = 0, n_kin_items = 0, n_bodies_stat = 0;
    int n_bodies_stat_valid = 0;
    struct CsSchedule {
        uint32_t n_tiles = 0, slot_offset = 0, round_start_offset = 0, round_offset = 0;
    } cs[2];
};
typedef World ivx_world;
#if SEED_FAULT == 2
static const uint32_t CHAIN_MAX = 5u;
#else
static const uint32_t CHAIN_MAX = PHYS_CHAIN_MAX;
#endif

struct H3 {
    float x, y, z;
};
inline H3 h3(const float* p) { return {p[0], p[1], p[2]}; }
inline H3 operator+(H3 a, H3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline H3 operator-(H3 a, H3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline H3 operator-(H3 a) { return {-a.x, -a.y, -a.z}; }
inline H3 operator*(H3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
inline float hdot(H3 a, H3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
inline H3 hcross(H3 a, H3 b) { return {a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }
inline uint64_t splitmix(uint64_t state) {  // (vec3.hpp)
    state += 0x9E3779B97F4A7C15ull;
    uint64_t z = state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline uint64_t splitmix2(uint64_t a, uint64_t b) { return splitmix(a ^ splitmix(b)); }

bool manifold_interlocked(const ivx_contact* c, size_t n) {
    float abs_sum = 0.0f;
    H3 vec{0, 0, 0};
    for (size_t i = 0; i < n; ++i) {
        if (c[i].depth <= 0.0f) continue;
        abs_sum += c[i].depth;
        vec = vec + h3(c[i].normal) * c[i].depth;
    }
    if (abs_sum < 1e-6f) return false;
    return hdot(vec, vec) / (abs_sum * abs_sum) < 0.1f;
}
template <class F>
H3 max_displacement(const ivx_contact* c, size_t n, F map) {
    float best = -INFINITY;
    size_t bi = n, bj = n;
    for (size_t i = 0; i + 1 < n; ++i)
        for (size_t j = i + 1; j < n; ++j) {
            const H3 d = map(h3(c[i].position)) - map(h3(c[j].position));
            const float s = hdot(d, d);
            if (s > best) {
                best = s;
                bi = i;
                bj = j;
            }
        }
    if (bi == n) return {0, 0, 0};
    return map(h3(c[bj].position)) - map(h3(c[bi].position));
}
bool unit_if_above(H3 v, float min_norm, H3& out) {
    const float n2 = hdot(v, v);
    if (!(n2 > min_norm * min_norm)) return false;
    const float n = std::sqrt(n2);
    out = {v.x / n, v.y / n, v.z / n};
    return true;
}
bool separate_along(H3 com_a_minus_b, const ivx_contact* c, size_t n, H3 axis, ivx_contact& out) {
    if (hdot(axis, com_a_minus_b) < 0.0f) axis = -axis;
    float lo = INFINITY, hi = -INFINITY;
    size_t i0 = n, i1 = n;
    for (size_t i = 0; i < n; ++i) {
        const float d = hdot(h3(c[i].position), axis);
        if (d < lo) {
            lo = d;
            i0 = i;
        }
        if (d > hi) {
            hi = d;
            i1 = i;
        }
    }
    if (i0 == i1) return false;
    out = c[i0];
    out.normal[0] = axis.x;
    out.normal[1] = axis.y;
    out.normal[2] = axis.z;
    out.depth = hi - lo;
    out.restitution = 0.0f;
    out.static_friction = INFINITY;
    out.dynamic_friction = INFINITY;
    out.id = splitmix2(c[i0].id, c[i1].id);
    return true;
}
bool separating_contact(H3 com_a_minus_b, const ivx_contact* c, size_t n, ivx_contact& out) {
    if (n == 0) return false;
    H3 major, middle, minor;
    if (!unit_if_above(max_displacement(c, n, [](H3 p) { return p; }), 1e-6f, major)) return false;
    const H3 md = max_displacement(c, n, [&](H3 p) { return p - major * hdot(p, major); });
    if (!unit_if_above(md, 1e-6f, middle)) return separate_along(com_a_minus_b, c, n, major, out);
    if (!unit_if_above(hcross(major, middle), 1e-4f, minor)) return separate_along(com_a_minus_b, c, n, major, out);
    if (separate_along(com_a_minus_b, c, n, minor, out)) return true;
    return separate_along(com_a_minus_b, c, n, middle, out);
}

void build_chains(ivx_world* w) {
    w->chain_start.clear();
    w->chain_bodies.clear();
    const uint32_t n = w->n_contacts;
    uint32_t s = 0;
    while (s < n) {
        uint32_t e = s + 1;
        while (e < n && e - s < CHAIN_MAX && w->slot_bodies[2 * (size_t)e] == w->slot_bodies[2 * (size_t)s] && w->slot_bodies[2 * (size_t)e + 1] == w->slot_bodies[2 * (size_t)s + 1]) ++e;
        w->chain_start.push_back(s);
        w->chain_bodies.push_back(w->slot_bodies[2 * (size_t)s]);
        w->chain_bodies.push_back(w->slot_bodies[2 * (size_t)s + 1]);
        s = e;
    }
    w->chain_start.push_back(n);
}
bool stationary_feasible(ivx_world* w, uint32_t nch, uint32_t passes) {
    const uint32_t n_tiles = (nch + 31u) / 32u;
    if (nch == 0 || passes == 0 || n_tiles > PHYS_CS_WAVES * PHYS_CS_MAX_GROUPS) return false;
    U32s& deg = w->scratch_count;
    deg.assign(w->n_dyn, 0u);
    for (uint32_t ch = 0; ch < nch; ++ch)
        for (int side = 0; side < 2; ++side) {
            const uint32_t b = w->chain_bodies[2 * (size_t)ch + side];
            if (!(b & IVX_KINEMATIC_BODY)) deg[b] += 1u;
        }
    for (uint32_t b = 0; b < w->n_dyn; ++b)
        if (deg[b] > 0xFFFFu) return false;
    return true;
}
void build_stationary(ivx_world* w, int phase, uint32_t nch, uint32_t passes, const U32s& lvl) {
    ivx_world::CsSchedule& cs = w->cs[phase];
    cs = ivx_world::CsSchedule();
    cs.slot_offset = (uint32_t)w->cs_item_host.size();
    cs.round_start_offset = (uint32_t)w->cs_round_start_host.size();
    cs.round_offset = (uint32_t)w->cs_round_mask_host.size();
    const uint32_t n_tiles = (nch + 31u) / 32u;
    if (!w->cs_feasible[phase]) return;
    U32s& deg = w->scratch_count;
    deg.assign(w->n_dyn, 0u);
    U32s& rank = w->scratch_rank;
    rank.resize(2 * (size_t)nch);
    for (uint32_t ch = 0; ch < nch; ++ch)
        for (int side = 0; side < 2; ++side) {
            const uint32_t b = w->chain_bodies[2 * (size_t)ch + side];
            rank[2 * (size_t)ch + side] = (b & IVX_KINEMATIC_BODY) ? 0u : deg[b]++;
        }
    const uint32_t max_level = w->n_levels[phase];
    U32s& order = w->scratch_order;
    order.resize(nch);
    {
        U32s& first = w->scratch_first;
        first.assign(max_level + 2u, 0u);
        for (uint32_t ch = 0; ch < nch; ++ch) first[lvl[ch] + 1u] += 1u;
        for (uint32_t l = 1; l <= max_level + 1u; ++l) first[l] += first[l - 1u];
        for (uint32_t ch = 0; ch < nch; ++ch) order[first[lvl[ch]]++] = ch;
    }
    const size_t slot0 = cs.slot_offset;
    w->cs_item_host.resize(slot0 + (size_t)n_tiles * 64u, 0xFFFFFFFFu);
    w->cs_bodies_host.resize(2 * (slot0 + (size_t)n_tiles * 64u), 0u);
    w->cs_vers_host.resize(slot0 + (size_t)n_tiles * 64u, 0u);
    std::vector<uint64_t>& mask_of = w->scratch_mask;
    mask_of.assign(max_level + 1u, 0ull);
    std::vector<uint64_t>& bits = w->scratch_bits;
    bits.assign((max_level + 64u) / 64u, 0ull);
    for (uint32_t t = 0; t < n_tiles; ++t) {
        const uint32_t first = t * 32u, cnt = std::min(32u, nch - first);
        uint32_t lo_w = 0xFFFFFFFFu, hi_w = 0u;
        for (uint32_t l = 0; l < cnt; ++l) {
            const uint32_t ch = order[first + l];
            const uint32_t s0 = w->chain_start[ch], len = w->chain_start[ch + 1] - s0;
            uint32_t body[2];
            for (int side = 0; side < 2; ++side) {
                const uint32_t b = w->chain_bodies[2 * (size_t)ch + side];
                body[side] = (b & IVX_KINEMATIC_BODY) ? w->n_dyn + (b & 0x7FFFFFFFu) : b;
            }
            for (int side = 0; side < 2; ++side) {
                const size_t slot = slot0 + (size_t)t * 64u + 2u * l + side;
                const uint32_t b = w->chain_bodies[2 * (size_t)ch + side];
                w->cs_item_host[slot] = s0 | (len << 24);
                w->cs_bodies_host[2 * slot] = body[side];
                w->cs_bodies_host[2 * slot + 1] = body[side ^ 1];
#if SEED_FAULT == 4
                w->cs_vers_host[slot] = (b & IVX_KINEMATIC_BODY) ? 0u : (deg[b] | rank[2 * (size_t)ch + side]);
#else
                w->cs_vers_host[slot] = (b & IVX_KINEMATIC_BODY) ? 0u : (deg[b] | (rank[2 * (size_t)ch + side] << 16));
#endif
            }
            const uint64_t lanes = 3ull << (2u * l);
            for (uint32_t p = 0; p < passes; ++p) {
                const uint32_t lv = lvl[(size_t)p * nch + ch];
                mask_of[lv] |= lanes;
                bits[lv >> 6] |= 1ull << (lv & 63u);
                lo_w = std::min(lo_w, lv >> 6);
                hi_w = std::max(hi_w, lv >> 6);
            }
        }
        w->cs_round_start_host.push_back((uint32_t)(w->cs_round_mask_host.size() - cs.round_offset));
        for (uint32_t wd = lo_w; wd <= hi_w && lo_w != 0xFFFFFFFFu; ++wd) {
            uint64_t m = bits[wd];
            bits[wd] = 0ull;
            while (m) {
                const uint32_t lv = wd * 64u + (uint32_t)__builtin_ctzll(m);
                m &= m - 1ull;
                w->cs_round_mask_host.push_back(mask_of[lv]);
                w->cs_round_level_host.push_back(lv);
                mask_of[lv] = 0ull;
            }
        }
    }
    w->cs_round_start_host.push_back((uint32_t)(w->cs_round_mask_host.size() - cs.round_offset));
    if (phase == 1 && !w->cs_slot_of_level.empty()) {
        w->cs_slot_of_host.assign((size_t)n_tiles * 32u * passes, 0u);
        for (uint32_t i = 0; i < nch; ++i)
            for (uint32_t p = 0; p < passes; ++p) w->cs_slot_of_host[(size_t)i * passes + p] = w->cs_slot_of_level[(size_t)p * nch + order[i]];
    }
    cs.n_tiles = n_tiles;
}
void build_levels(ivx_world* w, uint32_t n_first, uint32_t n_passes, int phase) {
    const uint32_t nch = (uint32_t)w->chain_start.size() - 1u, nb = w->n_dyn;
    const uint32_t total_passes = n_first + n_passes;
    const size_t total = (size_t)total_passes * nch;
    w->phase_items[phase] = (uint32_t)total;
    w->item_offset[phase] = phase ? w->phase_items[0] : 0u;
    w->level_offset[phase] = (uint32_t)w->level_start_host.size();
    w->n_levels[phase] = 0;
    w->max_level_items[phase] = 0;
    w->cs_feasible[phase] = 0;
    U32s& lvl = w->lvl_host[phase];
    lvl.clear();
    if (phase == 1) {
        w->kin_offsets_host.assign((size_t)w->n_kin + 1, 0u);
        w->kin_list_host.clear();
        w->cs_slot_of_level.clear();
        w->n_kin_items = 0;
    }
    if (total == 0) {
        w->level_start_host.push_back(0);
        return;
    }
    U32s& last = w->scratch_last;
    lvl.resize(total);
    last.assign(nb, 0u);
    uint32_t max_level = 0;
    size_t k = 0;
    for (uint32_t pass = 0; pass < total_passes; ++pass)
        for (uint32_t ch = 0; ch < nch; ++ch, ++k) {
            const uint32_t ba = w->chain_bodies[2 * (size_t)ch], bb = w->chain_bodies[2 * (size_t)ch + 1];
            uint32_t l = 0;
            if (!(ba & IVX_KINEMATIC_BODY)) l = std::max(l, last[ba]);
            if (!(bb & IVX_KINEMATIC_BODY)) l = std::max(l, last[bb]);
#if SEED_FAULT == 3
            if ((ba | bb) & IVX_KINEMATIC_BODY) l += 1;
#endif
            l += 1;
            if (!(ba & IVX_KINEMATIC_BODY)) last[ba] = l;
            if (!(bb & IVX_KINEMATIC_BODY)) last[bb] = l;
            lvl[k] = l;
            max_level = std::max(max_level, l);
        }
    const size_t ls0 = w->level_start_host.size();
    w->level_start_host.resize(ls0 + max_level + 1, 0u);
    uint32_t* start = w->level_start_host.data() + ls0;
    for (size_t i = 0; i < total; ++i) start[lvl[i]] += 1;
    uint32_t run = 0, widest = 0;
    for (uint32_t l = 1; l <= max_level; ++l) {
        const uint32_t c = start[l];
        widest = std::max(widest, c);
        run += c;
        start[l] = run;
    }
    w->n_levels[phase] = max_level;
    w->max_level_items[phase] = widest;
    w->cs_feasible[phase] = stationary_feasible(w, nch, total_passes) ? 1 : 0;
    if (phase == 1 && w->n_kin) {
        U32s cursor(start, start + max_level);
        std::vector<U32s> kin_items(w->n_kin);
        w->cs_slot_of_level.assign(total, 0u);
        k = 0;
        for (uint32_t pass = 0; pass < total_passes; ++pass)
            for (uint32_t ch = 0; ch < nch; ++ch, ++k) {
                const uint32_t slot = cursor[lvl[k] - 1]++;
                w->cs_slot_of_level[k] = slot;
                const uint32_t ba = w->chain_bodies[2 * (size_t)ch], bb = w->chain_bodies[2 * (size_t)ch + 1];
                if (ba & IVX_KINEMATIC_BODY) kin_items[ba & 0x7FFFFFFFu].push_back(slot);
                if (bb & IVX_KINEMATIC_BODY) kin_items[bb & 0x7FFFFFFFu].push_back(slot | 0x80000000u);
            }
        w->kin_offsets_host.assign(1, 0u);
        for (const auto& v : kin_items) {
            w->kin_list_host.insert(w->kin_list_host.end(), v.begin(), v.end());
            w->kin_offsets_host.push_back((uint32_t)w->kin_list_host.size());
        }
        w->n_kin_items = (uint32_t)w->kin_list_host.size();
        if (w->n_kin_items == 0) w->cs_slot_of_level.clear();
    }
}
void build_items(ivx_world* w, uint32_t first_type, uint32_t n_first, uint32_t type, uint32_t n_passes, int phase) {
    const uint32_t nch = (uint32_t)w->chain_start.size() - 1u, nb = w->n_dyn;
    const uint32_t total_passes = n_first + n_passes;
    const size_t total = (size_t)total_passes * nch;
    const U32s& lvl = w->lvl_host[phase];
    const uint32_t max_level = w->n_levels[phase];
    const size_t ls0 = w->level_offset[phase];
    w->tile_offset[phase] = (uint32_t)w->tile_first_host.size();
    w->n_tiles[phase] = 0;
    w->tile_base_host.resize(ls0 + max_level + 1, 0u);
    if (total == 0) return;
    const uint32_t* start = w->level_start_host.data() + ls0;
    const size_t it0 = w->items_host.size();
    w->items_host.resize(it0 + total);
    w->item_bodies_host.resize(2 * (it0 + total));
    w->item_tags_host.resize(4 * (it0 + total));
    U32s& seen = w->scratch_count;
    seen.assign(nb, 0u);
    U32s cursor(start, start + max_level);
    size_t k = 0;
    for (uint32_t pass = 0; pass < total_passes; ++pass) {
        const uint32_t ty = pass < n_first ? first_type : type;
        for (uint32_t ch = 0; ch < nch; ++ch, ++k) {
            const uint32_t s0 = w->chain_start[ch], len = w->chain_start[ch + 1] - s0;
            const size_t slot = it0 + cursor[lvl[k] - 1]++;
            w->items_host[slot] = s0 | (len << 24) | (ty << 28);
            const uint32_t ba = w->chain_bodies[2 * (size_t)ch], bb = w->chain_bodies[2 * (size_t)ch + 1];
            w->item_bodies_host[2 * slot] = (ba & IVX_KINEMATIC_BODY) ? w->n_dyn + (ba & 0x7FFFFFFFu) : ba;
            w->item_bodies_host[2 * slot + 1] = (bb & IVX_KINEMATIC_BODY) ? w->n_dyn + (bb & 0x7FFFFFFFu) : bb;
            uint32_t* tg = &w->item_tags_host[4 * slot];
            tg[0] = (ba & IVX_KINEMATIC_BODY) ? 0u : seen[ba]++;
            tg[1] = (bb & IVX_KINEMATIC_BODY) ? 0u : seen[bb]++;
            const uint32_t sweep = pass < n_first ? 0u : pass - n_first;
            tg[2] = sweep;
            tg[3] = sweep + 1u;
        }
    }
    uint32_t n_tiles = 0;
    for (uint32_t l = 0; l < max_level; ++l) {
        w->tile_base_host[ls0 + l] = n_tiles;
        for (uint32_t i = start[l]; i < start[l + 1]; i += 64u) {
            w->tile_first_host.push_back(i | ((std::min(64u, start[l + 1] - i) - 1u) << 26));
            n_tiles += 1;
        }
    }
    w->tile_base_host[ls0 + max_level] = n_tiles;
    w->n_tiles[phase] = n_tiles;
}
inline uint32_t id_hash(uint64_t id) { return (uint32_t)((id * 0x9E3779B97F4A7C15ull) >> 32); }
void id_table_reset(ivx_world* w, size_t want) {
    size_t cap = 1024;
    while (cap < 2 * want) cap *= 2;
    w->id_keys.assign(cap, 0ull);
    w->id_vals.assign(cap, 0xFFFFFFFFu);
    w->id_used = 0;
    for (uint32_t s = 0; s < w->cache.size(); ++s) {
        size_t h = id_hash(w->cache[s].id) & (cap - 1);
        while (w->id_vals[h] != 0xFFFFFFFFu) h = (h + 1) & (cap - 1);
        w->id_keys[h] = w->cache[s].id;
        w->id_vals[h] = s;
        w->id_used += 1;
    }
}
inline size_t id_find_pos(const ivx_world* w, uint64_t id) {
    const size_t mask = w->id_keys.size() - 1;
    size_t h = id_hash(id) & mask;
    while (w->id_vals[h] != 0xFFFFFFFFu && w->id_keys[h] != id) h = (h + 1) & mask;
    return h;
}
inline void id_erase(ivx_world* w, uint64_t id) {
    const size_t mask = w->id_keys.size() - 1;
    size_t h = id_find_pos(w, id);
    if (w->id_vals[h] == 0xFFFFFFFFu) return;
    size_t hole = h;
    for (size_t j = (h + 1) & mask; w->id_vals[j] != 0xFFFFFFFFu; j = (j + 1) & mask) {
        const size_t home = id_hash(w->id_keys[j]) & mask;
        const bool stays = hole <= j ? (home > hole && home <= j) : (home > hole || home <= j);
        if (!stays) {
            w->id_keys[hole] = w->id_keys[j];
            w->id_vals[hole] = w->id_vals[j];
            hole = j;
        }
    }
    w->id_vals[hole] = 0xFFFFFFFFu;
    w->id_used -= 1;
}

void ensure_form(ivx_world* w, uint32_t form) {  // ivx_world_ensure_form without its growth and uploads
    if (w->forms_built & form) return;
    if (form == 1u) {
        w->items_host.clear();
        w->item_bodies_host.clear();
        w->item_tags_host.clear();
        w->tile_base_host.clear();
        w->tile_first_host.clear();
        build_items(w, PHYS_ITEM_WARM, 1u, PHYS_ITEM_VELOCITY, w->cfg.n_iterations, 0);
        build_items(w, PHYS_ITEM_POSITIONAL, 0u, PHYS_ITEM_POSITIONAL, w->cfg.n_positional_correction_iterations, 1);
    } else {
        w->cs_item_host.clear();
        w->cs_bodies_host.clear();
        w->cs_vers_host.clear();
        w->cs_round_start_host.clear();
        w->cs_round_mask_host.clear();
        w->cs_round_level_host.clear();
        w->cs_slot_of_host.clear();
        const uint32_t nch = (uint32_t)w->chain_start.size() - 1u;
        build_stationary(w, 0, nch, w->cfg.n_iterations + 1u, w->lvl_host[0]);
        build_stationary(w, 1, nch, w->cfg.n_positional_correction_iterations, w->lvl_host[1]);
    }
    w->forms_built |= form;
}

// ivx_world_set_contacts without its device arrays, uploads and launches (the pinned block is a vector with the old growth rule)
SetResult set_contacts(ivx_world* w, const ivx_contact* contacts, size_t n, PositionOf fetch_body_position) {
    SetResult r;
    if (w->schedule_valid && n > 0 && n == w->n_contacts && n == w->cache.size() && 2 * n == w->slot_bodies.size() && w->stage_contacts_cap >= n) {
        bool same = true;
        size_t i = 0;
        while (i < n && same) {
            size_t j = i + 1;
            while (j < n && !(contacts[j].flags & IVX_CONTACT_MANIFOLD_START)) ++j;
            if (manifold_interlocked(contacts + i, j - i)) same = false;
            for (size_t k = i; k < j && same; ++k) {
                const ivx_contact& c = contacts[k];
                same = c.id == w->cache[k].id && c.body_a == w->slot_bodies[2 * k] && c.body_b == w->slot_bodies[2 * k + 1];
                w->stage_contacts[k] = c;
            }
            i = j;
        }
        if (same) {
            w->n_prev = w->n_contacts;
            r.fast = true;
            r.nc = (uint32_t)n;
            return r;
        }
    }
    bool any_interlocked = false;
    {
        size_t i = 0;
        while (i < n) {
            size_t j = i;
            do {
                const ivx_contact& c = contacts[j];
                const uint32_t la = (c.body_a & IVX_KINEMATIC_BODY) ? w->n_kin : w->n_dyn, lb = (c.body_b & IVX_KINEMATIC_BODY) ? w->n_kin : w->n_dyn;
                if (!((c.body_a & 0x7FFFFFFFu) < la && (c.body_b & 0x7FFFFFFFu) < lb)) return r.code = SET_MISSING_BODY, r.bad = j, r;
                if (!(c.body_a != c.body_b)) return r.code = SET_SELF_PAIR, r.bad = j, r;
                ++j;
            } while (j < n && !(contacts[j].flags & IVX_CONTACT_MANIFOLD_START));
            if (manifold_interlocked(contacts + i, j - i)) any_interlocked = true;
            i = j;
        }
    }
    const ivx_contact* eff = contacts;
    size_t n_eff = n;
    if (any_interlocked) {
        w->effective.clear();
        size_t i = 0;
        while (i < n) {
            size_t j = i + 1;
            while (j < n && !(contacts[j].flags & IVX_CONTACT_MANIFOLD_START)) ++j;
            const ivx_contact* m = contacts + i;
            const size_t cnt = j - i;
            bool replaced = false;
            if (manifold_interlocked(m, cnt)) {
                float pa[3], pb[3];
                fetch_body_position(m[0].body_a, pa);
                fetch_body_position(m[0].body_b, pb);
                ivx_contact sep;
                if (separating_contact(h3(pa) - h3(pb), m, cnt, sep)) {
                    sep.body_a = m[0].body_a;
                    sep.body_b = m[0].body_b;
                    w->effective.push_back(sep);
                    replaced = true;
                }
            }
            if (!replaced) w->effective.insert(w->effective.end(), m, m + cnt);
            i = j;
        }
        eff = w->effective.data();
        n_eff = w->effective.size();
    }
    if (w->id_keys.empty() || 2 * (w->cache.size() + n_eff) > w->id_keys.size()) id_table_reset(w, w->cache.size() + n_eff);
    {
        const size_t old_len = w->cache.size();
        size_t cursor = 0;
        w->cache.reserve(old_len + n_eff);
        for (uint32_t e = 0; e < n_eff; ++e) {
            const uint64_t id = eff[e].id;
            if (cursor < old_len && w->cache[cursor].id == id) {
                w->cache[cursor].src = e;
                w->cache[cursor].prepared = true;
                cursor += 1;
                continue;
            }
            const size_t h = id_find_pos(w, id);
            if (w->id_vals[h] != 0xFFFFFFFFu) {
                ivx_world::Entry& en = w->cache[w->id_vals[h]];
                en.src = e;
                en.prepared = true;
                cursor = (size_t)w->id_vals[h] + 1;
            } else {
                w->id_keys[h] = id;
                w->id_vals[h] = (uint32_t)w->cache.size();
                w->id_used += 1;
                w->cache.push_back(ivx_world::Entry{id, -1, e, true});
            }
        }
        size_t idx = 0, len = w->cache.size();
        while (idx < len) {
            if (w->cache[idx].prepared) {
                ++idx;
            } else {
                id_erase(w, w->cache[idx].id);
                w->cache[idx] = w->cache[len - 1];
                w->cache.pop_back();
                --len;
#if SEED_FAULT != 1
                if (idx < len) w->id_vals[id_find_pos(w, w->cache[idx].id)] = (uint32_t)idx;
#endif
            }
        }
    }
    const uint32_t nc = (uint32_t)w->cache.size();
    w->n_bodies_stat_valid = 0;
    if (nc > w->stage_contacts_cap) {
        const size_t cap2 = (size_t)nc + nc / 4 + 64;
        w->stage_contacts.assign(cap2, ivx_contact{});
        w->stage_contacts_cap = cap2;
    }
    w->prev_slot_host.resize(nc);
    w->slot_bodies.resize(2 * (size_t)nc);
    for (uint32_t sl = 0; sl < nc; ++sl) {
        ivx_world::Entry& en = w->cache[sl];
        const ivx_contact& c = eff[en.src];
        w->stage_contacts[sl] = c;
        w->slot_bodies[2 * (size_t)sl] = c.body_a;
        w->slot_bodies[2 * (size_t)sl + 1] = c.body_b;
        w->prev_slot_host[sl] = en.prev_slot;
        en.prev_slot = (int32_t)sl;
        en.prepared = false;
    }
    w->n_prev = w->n_contacts;
    w->n_contacts = nc;
    build_chains(w);
    const bool same_schedule = w->schedule_valid && w->chain_start == w->prev_chain_start && w->chain_bodies == w->prev_chain_bodies;
    if (!same_schedule) {
        w->level_start_host.clear();
        build_levels(w, 1u, w->cfg.n_iterations, 0);
        build_levels(w, 0u, w->cfg.n_positional_correction_iterations, 1);
        w->forms_built = 0;
        w->prev_chain_start = w->chain_start;
        w->prev_chain_bodies = w->chain_bodies;
    }
    w->schedule_valid = 1;
    r.nc = nc;
    return r;
}
uint32_t step_body_count(ivx_world* w) {  // the count inside ivx_world_step
    if (!w->n_bodies_stat_valid) {
        std::vector<uint8_t> t((size_t)w->n_dyn + w->n_kin, 0);
        for (size_t sl = 0; sl + 1 < w->slot_bodies.size(); sl += 2) {
            const uint32_t a = w->slot_bodies[sl], b = w->slot_bodies[sl + 1];
            if (a & IVX_KINEMATIC_BODY) t[w->n_dyn + (a & 0x7FFFFFFFu)] = 1;
            else if (a < w->n_dyn) t[a] = 1;
            if (b & IVX_KINEMATIC_BODY) t[w->n_dyn + (b & 0x7FFFFFFFu)] = 1;
            else if (b < w->n_dyn) t[b] = 1;
        }
        for (uint32_t r : w->joint_refs_host)
            if (!(r & IVX_KINEMATIC_BODY) && r < w->n_dyn) t[r] = 1;
        uint32_t nb = 0;
        for (uint8_t x : t) nb += x;
        w->n_bodies_stat = nb;
        w->n_bodies_stat_valid = 1;
    }
    return w->n_bodies_stat;
}
}  // namespace old

// ---- the struct, driven the way ivx_world_set_contacts and ivx_world_ensure_form drive it ------------------------------------------------
struct New {
    ivx_solver_config cfg{};
    uint32_t n_dyn = 0, n_kin = 0, n_contacts = 0, n_prev = 0;
    int schedule_valid = 0;
    ivx_contact_schedule sched;
    std::vector<ivx_contact> block;  // the pinned block (size rule of ivx_staging_for, in contacts)
    U32s joint_refs_host;
    SetResult set_contacts(const ivx_contact* contacts, size_t n) {
        SetResult r;
        ivx_contact_schedule& h = sched;
        if (schedule_valid && n > 0 && n == n_contacts && n == h.cache.size() && 2 * n == h.slot_bodies.size() && block.size() >= n && h.same_as_resident(contacts, n, block.data())) {
            n_prev = n_contacts;
            r.fast = true;
            r.nc = (uint32_t)n;
            return r;
        }
        const ivx_contact_schedule::Verdict v = ivx_contact_schedule::validate(contacts, n, n_dyn, n_kin);
        if (v.kind != ivx_contact_schedule::CONTACT_OK) return r.code = v.kind == ivx_contact_schedule::CONTACT_MISSING_BODY ? SET_MISSING_BODY : SET_SELF_PAIR, r.bad = v.index, r;
        const ivx_contact* eff = contacts;
        size_t n_eff = n;
        if (v.any_interlocked) {
            h.replace_interlocked(contacts, n, [](uint32_t ref, float* out) { return position_of(ref, out), 0; });
            eff = h.effective.data(), n_eff = h.effective.size();
        }
        const uint32_t nc = h.register_contacts(eff, n_eff);
        if (nc > block.size()) block.assign(std::max<size_t>((size_t)nc + nc / 2, 1024), ivx_contact{});
        h.write_slot_order(eff, block.data());
        n_prev = n_contacts;
        n_contacts = nc;
        h.build_chains();
        h.build_levels(schedule_valid != 0, cfg.n_iterations, cfg.n_positional_correction_iterations, n_dyn, n_kin);
        schedule_valid = 1;
        r.nc = nc;
        return r;
    }
    void ensure_form(uint32_t form) {
        if (sched.forms_built & form) return;
        sched.build_form(form, cfg.n_iterations, cfg.n_positional_correction_iterations, n_dyn);
        sched.forms_built |= form;
    }
};

// ---- comparison ---------------------------------------------------------------------------------------------------------------------------
static int n_diff = 0;
static void differ(const char* what) {
    if (n_diff++ < 20) printf("DIFFERENT: %s\n", what);
}
#define SAME(a, b) \
    if (!((a) == (b))) differ(#a)
#define SAME2(a, b) \
    if (!((a)[0] == (b)[0] && (a)[1] == (b)[1])) differ(#a)

static void compare(old::World& o, New& n, const SetResult& ro, const SetResult& rn, std::mt19937_64& rng) {
    ivx_contact_schedule& h = n.sched;
    SAME(ro.code, rn.code);
    SAME(ro.bad, rn.bad);
    SAME(ro.fast, rn.fast);
    SAME(ro.nc, rn.nc);
    SAME(o.n_contacts, n.n_contacts);
    SAME(o.n_prev, n.n_prev);
    SAME(o.schedule_valid, n.schedule_valid);
    SAME(o.cache.size(), h.cache.size());
    for (size_t s = 0; s < o.cache.size() && s < h.cache.size(); ++s) {
        const old::World::Entry& a = o.cache[s];
        const ivx_contact_schedule::Entry& b = h.cache[s];
        if (a.id != b.id || a.prev_slot != b.prev_slot || a.src != b.src || a.prepared != b.prepared) differ("cache entry");
        if (o.id_vals[old::id_find_pos(&o, a.id)] != h.id_vals[h.id_find_pos(a.id)]) differ("id table: an id present");
        if (h.id_vals[h.id_find_pos(a.id)] != s) differ("id table: slot of an id present");
    }
    if (!o.id_keys.empty())
        for (int i = 0; i < 8; ++i) {
            const uint64_t id = rng();
            if (o.id_vals[old::id_find_pos(&o, id)] != h.id_vals[h.id_find_pos(id)]) differ("id table: an id absent");
        }
    SAME(o.id_used, h.id_used);
    SAME(o.prev_slot_host, h.prev_slot_host);
    SAME(o.slot_bodies, h.slot_bodies);
    if (o.n_contacts && memcmp(o.stage_contacts.data(), n.block.data(), o.n_contacts * sizeof(ivx_contact)) != 0) differ("contacts in slot order");
    SAME(o.chain_start, h.chain_start);
    SAME(o.chain_bodies, h.chain_bodies);
    SAME(o.prev_chain_start, h.prev_chain_start);
    SAME(o.prev_chain_bodies, h.prev_chain_bodies);
    SAME2(o.lvl_host, h.lvl_host);
    SAME(o.level_start_host, h.level_start_host);
    SAME2(o.n_levels, h.n_levels);
    SAME2(o.max_level_items, h.max_level_items);
    SAME2(o.phase_items, h.phase_items);
    SAME2(o.item_offset, h.item_offset);
    SAME2(o.level_offset, h.level_offset);
    SAME2(o.cs_feasible, h.cs_feasible);
    SAME(o.forms_built, h.forms_built);
    SAME(o.n_kin_items, h.n_kin_items);
    SAME(o.kin_offsets_host, h.kin_offsets_host);
    SAME(o.kin_list_host, h.kin_list_host);
    SAME(o.cs_slot_of_level, h.cs_slot_of_level);
    if (o.forms_built & 1u) {
        SAME2(o.n_tiles, h.n_tiles);
        SAME2(o.tile_offset, h.tile_offset);
        SAME(o.items_host, h.items_host);
        SAME(o.item_bodies_host, h.item_bodies_host);
        SAME(o.item_tags_host, h.item_tags_host);
        SAME(o.tile_base_host, h.tile_base_host);
        SAME(o.tile_first_host, h.tile_first_host);
    }
    if (o.forms_built & 2u) {
        for (int p = 0; p < 2; ++p)
            if (o.cs[p].n_tiles != h.cs[p].n_tiles || o.cs[p].slot_offset != h.cs[p].slot_offset || o.cs[p].round_start_offset != h.cs[p].round_start_offset ||
                o.cs[p].round_offset != h.cs[p].round_offset)
                differ("cs[p]");
        SAME(o.cs_item_host, h.cs_item_host);
        SAME(o.cs_bodies_host, h.cs_bodies_host);
        SAME(o.cs_vers_host, h.cs_vers_host);
        SAME(o.cs_round_start_host, h.cs_round_start_host);
        SAME(o.cs_round_mask_host, h.cs_round_mask_host);
        SAME(o.cs_round_level_host, h.cs_round_level_host);
        SAME(o.cs_slot_of_host, h.cs_slot_of_host);
    }
}

// ---- random sequences ----------------------------------------------------------------------------------------------------------------------
struct Manifold {
    uint32_t a, b;
    std::vector<uint64_t> ids;
    bool interlocked;
};
struct Gen {
    std::mt19937_64 rng;
    uint32_t n_dyn = 1, n_kin = 0;
    uint32_t below(uint32_t n) { return (uint32_t)(rng() % n); }
    float unit() { return (float)(rng() % 10000u) / 10000.0f; }
    uint32_t body() {
        const uint32_t i = below(n_dyn + n_kin);
        return i < n_dyn ? i : ((i - n_dyn) | IVX_KINEMATIC_BODY);
    }
    bool pair(uint32_t& a, uint32_t& b) {  // two different bodies, at least one dynamic
        if (n_dyn + n_kin < 2) return false;
        do a = body(), b = body();
        while (a == b || (a & b & IVX_KINEMATIC_BODY));
        return true;
    }
    Manifold manifold() {
        Manifold m{};
        pair(m.a, m.b);
        const uint32_t k = 1u + below(9u);
        for (uint32_t i = 0; i < k; ++i) m.ids.push_back(rng());
        m.interlocked = k >= 2 && below(8u) == 0;
        return m;
    }
    void emit(const Manifold& m, std::vector<ivx_contact>& out) {  // fresh geometry every time: the ids and pairs are what stays
        for (size_t i = 0; i < m.ids.size(); ++i) {
            ivx_contact c{};
            c.id = m.ids[i], c.body_a = m.a, c.body_b = m.b;
            for (int q = 0; q < 3; ++q) c.position[q] = 4.0f * unit() - 2.0f;
            c.normal[0] = (m.interlocked && (i & 1)) ? -1.0f : 1.0f;
            c.depth = m.interlocked ? 0.01f : 0.02f * unit() - 0.002f;
            c.restitution = unit(), c.static_friction = unit(), c.dynamic_friction = unit();
            c.flags = i == 0 ? IVX_CONTACT_MANIFOLD_START : 0u;
            out.push_back(c);
        }
    }
};

static int run_random(unsigned long long n_seq, unsigned long long seed) {
    Gen g;
    g.rng.seed(seed);
    unsigned long long n_frames = 0, n_contacts = 0, n_fast = 0, n_rejected = 0, n_interlocked = 0, n_two_tiles = 0;
    for (unsigned long long q = 0; q < n_seq && !n_diff; ++q) {
        old::World o;
        New n;
        g.n_dyn = 1u + g.below(40u), g.n_kin = g.below(5u);
        o.n_dyn = n.n_dyn = g.n_dyn, o.n_kin = n.n_kin = g.n_kin;
        o.cfg.n_iterations = n.cfg.n_iterations = g.below(10u);
        o.cfg.n_positional_correction_iterations = n.cfg.n_positional_correction_iterations = g.below(5u);
        std::vector<Manifold> live, gone;
        std::vector<ivx_contact> list;
        const uint32_t frames = 4u + g.below(12u);
        for (uint32_t f = 0; f < frames && !n_diff; ++f) {
            const bool can = g.n_dyn + g.n_kin >= 2;
            const uint32_t mode = f == 0 ? 3u : g.below(12u);
            bool bad = false;
            switch (mode) {
            case 0: break;     // the same list again (the fast path unless something is interlocked)
            case 1: break;     // ... emit() gives it other depths anyway
            case 2:            // ids leave from the middle
                for (uint32_t k = 0, m = 1u + g.below(3u); k < m && !live.empty(); ++k) {
                    const size_t at = g.below((uint32_t)live.size());
                    if (live[at].ids.size() > 1 && g.below(2u)) live[at].ids.erase(live[at].ids.begin() + g.below((uint32_t)live[at].ids.size()));
                    else gone.push_back(live[at]), live.erase(live.begin() + at);
                }
                break;
            case 3:            // new manifolds; some that had left come back
                for (uint32_t k = 0, m = 1u + g.below(12u); k < m && can; ++k) live.push_back(g.manifold());
                while (!gone.empty() && g.below(2u)) live.insert(live.begin() + g.below((uint32_t)live.size() + 1u), gone.back()), gone.pop_back();
                break;
            case 4:            // all new
                live.clear();
                for (uint32_t k = 0, m = 1u + g.below(12u); k < m && can; ++k) live.push_back(g.manifold());
                break;
            case 5: std::reverse(live.begin(), live.end()); break;  // the same ids, reversed
            case 6: gone.insert(gone.end(), live.begin(), live.end()), live.clear(); break;  // the empty list
            case 7:            // consecutive manifolds on one pair
                if (!live.empty()) {
                    const size_t at = g.below((uint32_t)live.size());
                    Manifold m = g.manifold();
                    m.a = live[at].a, m.b = live[at].b;
                    live.insert(live.begin() + at + 1, m);
                }
                break;
            case 8:            // more than 32 chains: a second tile
                for (uint32_t k = 0; k < 36u && can; ++k) live.push_back(g.manifold());
                break;
            case 9: bad = true; break;  // a list that must be refused
            case 10: {         // other body counts between frames: the schedule is invalid, the references stay good
                g.n_dyn += g.below(3u), g.n_kin += g.below(2u);
                o.n_dyn = n.n_dyn = g.n_dyn, o.n_kin = n.n_kin = g.n_kin;
                o.n_bodies_stat_valid = 0, n.sched.n_bodies_valid = false;
                o.schedule_valid = n.schedule_valid = 0;
                break;
            }
            default:           // a manifold becomes interlocked or stops being so
                if (!live.empty()) {
                    Manifold& m = live[g.below((uint32_t)live.size())];
                    m.interlocked = !m.interlocked && m.ids.size() >= 2;
                }
            }
            list.clear();
            for (const Manifold& m : live) g.emit(m, list), n_interlocked += m.interlocked;
            if (bad && !list.empty()) {
                ivx_contact& c = list[g.below((uint32_t)list.size())];
                if (g.below(2u)) c.body_b = c.body_a;
                else (g.below(2u) ? c.body_a : c.body_b) = g.below(2u) ? g.n_dyn : (g.n_kin | IVX_KINEMATIC_BODY);
            }
            const SetResult ro = old::set_contacts(&o, list.data(), list.size(), position_of), rn = n.set_contacts(list.data(), list.size());
            n_frames += 1, n_contacts += list.size(), n_fast += rn.fast, n_rejected += rn.code != SET_OK;
            compare(o, n, ro, rn, g.rng);
            if (rn.code != SET_OK) continue;
            for (uint32_t form = 1; form <= 2; ++form)
                if (g.below(3u)) {
                    old::ensure_form(&o, form), n.ensure_form(form);
                    compare(o, n, ro, rn, g.rng);
                }
            n_two_tiles += n.sched.n_chains() > 32u;
            if (g.below(2u)) {
                o.joint_refs_host.assign(1, g.body()), n.joint_refs_host = o.joint_refs_host;
                o.n_bodies_stat_valid = 0, n.sched.n_bodies_valid = false;
            }
            for (int twice = 0; twice < 2; ++twice)
                if (old::step_body_count(&o) != n.sched.constrained_bodies(n.joint_refs_host, n.n_dyn, n.n_kin)) differ("constrained bodies");
        }
    }
    printf("seed %llu: %llu sequences, %llu frames (%llu on the fast path, %llu refused, %llu with more than 32 chains), %llu contacts, %llu interlocked manifolds: %s\n", seed, n_seq,
           n_frames, n_fast, n_rejected, n_two_tiles, n_contacts, n_interlocked, n_diff ? "DIFFERENT" : "all equal");
    return n_diff ? 1 : 0;
}

// ---- scenarios -----------------------------------------------------------------------------------------------------------------------------
static int n_wrong = 0;
template <class T>
static void expect(const char* scenario, const char* what, const std::vector<T>& got, std::initializer_list<typename std::common_type<T>::type> want) {
    if (got == std::vector<T>(want)) return;
    n_wrong += 1;
    printf("WRONG %s: %s =", scenario, what);
    for (const T& x : got) printf(" %lld", (long long)x);
    printf("\n");
}
static void expect2(const char* scenario, const char* what, const uint32_t got[2], uint32_t w0, uint32_t w1) { expect(scenario, what, U32s{got[0], got[1]}, {w0, w1}); }
#define EXPECT(v, ...) expect(S, #v, v, {__VA_ARGS__})
#define EXPECT2(v, a, b) expect2(S, #v, v, a, b)
static const uint32_t K = IVX_KINEMATIC_BODY;
static ivx_contact contact(uint64_t id, uint32_t a, uint32_t b, bool start = true) {
    ivx_contact c{};
    c.id = id, c.body_a = a, c.body_b = b, c.normal[1] = 1.0f, c.depth = 0.01f, c.flags = start ? IVX_CONTACT_MANIFOLD_START : 0u;
    return c;
}
static New world(uint32_t n_dyn, uint32_t n_kin, uint32_t iterations, uint32_t positional) {
    New n;
    n.n_dyn = n_dyn, n.n_kin = n_kin, n.cfg.n_iterations = iterations, n.cfg.n_positional_correction_iterations = positional;
    return n;
}
static U32s head(const U32s& v, size_t n) { return U32s(v.begin(), v.begin() + std::min(n, v.size())); }

static int run_scenarios() {
    {
        const char* S = "two bodies, one contact";
        New n = world(2, 0, 1, 1);
        const ivx_contact c[] = {contact(7, 0, 1)};
        n.set_contacts(c, 1), n.ensure_form(1), n.ensure_form(2);
        ivx_contact_schedule& h = n.sched;
        EXPECT(h.prev_slot_host, -1);
        EXPECT(h.slot_bodies, 0u, 1u);
        EXPECT(h.chain_start, 0u, 1u);
        EXPECT(h.chain_bodies, 0u, 1u);
        EXPECT(h.lvl_host[0], 1u, 2u);
        EXPECT(h.lvl_host[1], 1u);
        EXPECT(h.level_start_host, 0u, 1u, 2u, 0u, 1u);
        EXPECT2(h.n_levels, 2u, 1u);
        EXPECT2(h.max_level_items, 1u, 1u);
        EXPECT2(h.phase_items, 2u, 1u);
        EXPECT2(h.item_offset, 0u, 2u);
        EXPECT2(h.level_offset, 0u, 3u);
        EXPECT(h.items_host, 0x01000000u, 0x11000000u, 0x21000000u);
        EXPECT(h.item_bodies_host, 0u, 1u, 0u, 1u, 0u, 1u);
        EXPECT(h.item_tags_host, 0u, 0u, 0u, 1u, 1u, 1u, 0u, 1u, 0u, 0u, 0u, 1u);
        EXPECT(h.tile_base_host, 0u, 1u, 2u, 0u, 1u);
        EXPECT(h.tile_first_host, 0u, 1u, 0u);
        EXPECT2(h.n_tiles, 2u, 1u);
        EXPECT2(h.tile_offset, 0u, 2u);
        EXPECT((U32s{h.cs[0].n_tiles, h.cs[0].slot_offset, h.cs[1].n_tiles, h.cs[1].slot_offset, h.cs[1].round_start_offset, h.cs[1].round_offset}), 1u, 0u, 1u, 64u, 2u, 2u);
        EXPECT((U32s{(uint32_t)h.cs_item_host.size(), h.cs_item_host[0], h.cs_item_host[1], h.cs_item_host[2], h.cs_item_host[64], h.cs_item_host[66]}), 128u, 0x01000000u, 0x01000000u, 0xFFFFFFFFu,
               0x01000000u, 0xFFFFFFFFu);
        EXPECT(head(h.cs_bodies_host, 4), 0u, 1u, 1u, 0u);
        EXPECT(head(h.cs_vers_host, 3), 1u, 1u, 0u);
        EXPECT(h.cs_round_start_host, 0u, 2u, 0u, 1u);
        EXPECT(h.cs_round_mask_host, 3ull, 3ull, 3ull);
        EXPECT(h.cs_round_level_host, 1u, 2u, 1u);
        EXPECT((U32s{h.constrained_bodies(n.joint_refs_host, 2, 0)}), 2u);
    }
    {
        const char* S = "one manifold of five contacts on one pair";
        New n = world(2, 0, 1, 1);
        ivx_contact c[5];
        for (uint32_t i = 0; i < 5; ++i) c[i] = contact(100 + i, 0, 1, i == 0);
        n.set_contacts(c, 5), n.ensure_form(1);
        ivx_contact_schedule& h = n.sched;
        EXPECT(h.chain_start, 0u, 4u, 5u);
        EXPECT(h.chain_bodies, 0u, 1u, 0u, 1u);
        EXPECT(h.lvl_host[0], 1u, 2u, 3u, 4u);
        EXPECT(h.lvl_host[1], 1u, 2u);
        EXPECT2(h.n_levels, 4u, 2u);
        EXPECT2(h.max_level_items, 1u, 1u);
        EXPECT(h.items_host, 0x04000000u, 0x01000004u, 0x14000000u, 0x11000004u, 0x24000000u, 0x21000004u);
    }
    {
        const char* S = "three bodies in a row";
        New n = world(3, 0, 1, 0);
        const ivx_contact c[] = {contact(1, 0, 1), contact(2, 1, 2)};
        n.set_contacts(c, 2), n.ensure_form(1);
        ivx_contact_schedule& h = n.sched;
        EXPECT(h.lvl_host[0], 1u, 2u, 3u, 4u);
        EXPECT(h.level_start_host, 0u, 1u, 2u, 3u, 4u, 0u);
        EXPECT2(h.n_levels, 4u, 0u);
        EXPECT(h.item_tags_host, 0u, 0u, 0u, 1u, 1u, 0u, 0u, 1u, 1u, 2u, 0u, 1u, 3u, 1u, 0u, 1u);
        EXPECT(h.item_bodies_host, 0u, 1u, 1u, 2u, 0u, 1u, 1u, 2u);
    }
    {
        const char* S = "an id leaves from the middle of four";
        New n = world(8, 0, 1, 1);
        const ivx_contact c[] = {contact(10, 0, 1), contact(11, 2, 3), contact(12, 4, 5), contact(13, 6, 7)};
        n.set_contacts(c, 4);
        const ivx_contact d[] = {c[0], c[2], c[3]};
        n.set_contacts(d, 3);
        ivx_contact_schedule& h = n.sched;
        EXPECT((std::vector<uint64_t>{h.cache[0].id, h.cache[1].id, h.cache[2].id}), 10ull, 13ull, 12ull);
        EXPECT(h.prev_slot_host, 0, 3, 2);
        EXPECT(h.slot_bodies, 0u, 1u, 6u, 7u, 4u, 5u);
        EXPECT((std::vector<uint64_t>{n.block[0].id, n.block[1].id, n.block[2].id}), 10ull, 13ull, 12ull);
        EXPECT((U32s{h.id_vals[h.id_find_pos(10)], h.id_vals[h.id_find_pos(13)], h.id_vals[h.id_find_pos(12)], h.id_vals[h.id_find_pos(11)], (uint32_t)h.id_used}), 0u, 1u, 2u, 0xFFFFFFFFu, 3u);
        EXPECT((U32s{n.n_prev, n.n_contacts}), 4u, 3u);
    }
    {
        const char* S = "33 independent chains";
        New n = world(66, 0, 0, 0);
        std::vector<ivx_contact> c;
        for (uint32_t i = 0; i < 33; ++i) c.push_back(contact(500 + i, 2 * i, 2 * i + 1));
        n.set_contacts(c.data(), c.size()), n.ensure_form(2);
        ivx_contact_schedule& h = n.sched;
        EXPECT2(h.n_levels, 1u, 0u);
        EXPECT2(h.max_level_items, 33u, 0u);
        EXPECT((U32s{(uint32_t)h.cs_feasible[0], (uint32_t)h.cs_feasible[1], h.cs[0].n_tiles, h.cs[1].n_tiles, (uint32_t)h.cs_item_host.size()}), 1u, 0u, 2u, 0u, 128u);
        EXPECT(h.cs_round_start_host, 0u, 1u, 2u);
        EXPECT(h.cs_round_mask_host, ~0ull, 3ull);
        EXPECT(h.cs_round_level_host, 1u, 1u);
        EXPECT((U32s{h.cs_item_host[63], h.cs_item_host[64], h.cs_item_host[65], h.cs_item_host[66]}), 0x0100001Fu, 0x01000020u, 0x01000020u, 0xFFFFFFFFu);
    }
    {
        const char* S = "one kinematic body, two positional passes";
        New n = world(2, 1, 0, 2);
        const ivx_contact c[] = {contact(1, 0, K | 0u), contact(2, 1, K | 0u)};
        n.set_contacts(c, 2), n.ensure_form(2);
        ivx_contact_schedule& h = n.sched;
        EXPECT(h.lvl_host[1], 1u, 1u, 2u, 2u);
        EXPECT(h.level_start_host, 0u, 2u, 0u, 2u, 4u);
        EXPECT(h.cs_slot_of_level, 0u, 1u, 2u, 3u);
        EXPECT(h.kin_offsets_host, 0u, 4u);
        EXPECT(h.kin_list_host, K | 0u, K | 1u, K | 2u, K | 3u);
        EXPECT((U32s{h.n_kin_items, (uint32_t)h.cs_slot_of_host.size()}), 4u, 64u);
        EXPECT(head(h.cs_slot_of_host, 5), 0u, 2u, 1u, 3u, 0u);
        EXPECT(U32s(h.cs_bodies_host.begin() + 128, h.cs_bodies_host.begin() + 136), 0u, 2u, 2u, 0u, 1u, 2u, 2u, 1u);
        EXPECT(U32s(h.cs_vers_host.begin() + 64, h.cs_vers_host.begin() + 69), 1u, 0u, 1u, 0u, 0u);
        EXPECT((U32s{h.constrained_bodies(n.joint_refs_host, 2, 1)}), 3u);
    }
    {
        const char* S = "zero iterations of either kind";
        New n = world(2, 0, 0, 0);
        const ivx_contact c[] = {contact(7, 0, 1)};
        n.set_contacts(c, 1), n.ensure_form(1), n.ensure_form(2);
        ivx_contact_schedule& h = n.sched;
        EXPECT2(h.n_levels, 1u, 0u);
        EXPECT2(h.phase_items, 1u, 0u);
        EXPECT(h.level_start_host, 0u, 1u, 0u);
        EXPECT(h.items_host, 0x01000000u);
        EXPECT(h.tile_base_host, 0u, 1u, 0u);
        EXPECT((U32s{(uint32_t)h.cs_feasible[0], (uint32_t)h.cs_feasible[1], h.cs[0].n_tiles, h.cs[1].n_tiles}), 1u, 0u, 1u, 0u);
    }
    {
        const char* S = "the empty list after a full one";
        New n = world(4, 0, 2, 1);
        const ivx_contact c[] = {contact(1, 0, 1), contact(2, 2, 3)};
        n.set_contacts(c, 2);
        const SetResult r = n.set_contacts(nullptr, 0);
        n.ensure_form(1), n.ensure_form(2);
        ivx_contact_schedule& h = n.sched;
        EXPECT((U32s{r.nc, n.n_prev, n.n_contacts, (uint32_t)h.cache.size(), (uint32_t)h.id_used, h.n_chains()}), 0u, 2u, 0u, 0u, 0u, 0u);
        EXPECT(h.chain_start, 0u);
        EXPECT(h.level_start_host, 0u, 0u);
        EXPECT2(h.n_levels, 0u, 0u);
        EXPECT2(h.phase_items, 0u, 0u);
        EXPECT((U32s{(uint32_t)h.items_host.size(), (uint32_t)h.cs_item_host.size(), h.cs[0].n_tiles}), 0u, 0u, 0u);
        EXPECT(h.tile_base_host, 0u, 0u);
        EXPECT((U32s{h.constrained_bodies(n.joint_refs_host, 4, 0)}), 0u);
    }
    {
        const char* S = "lists that are refused";
        New n = world(2, 1, 1, 1);
        const ivx_contact c[] = {contact(1, 0, 1), contact(2, 1, 2), contact(3, 1, 1)};
        const SetResult r = n.set_contacts(c, 3);
        EXPECT((U32s{(uint32_t)r.code, (uint32_t)r.bad}), (uint32_t)SET_MISSING_BODY, 1u);
        const ivx_contact d[] = {contact(1, 0, K | 0u), contact(3, K | 0u, K | 0u)};
        const SetResult q = n.set_contacts(d, 2);
        EXPECT((U32s{(uint32_t)q.code, (uint32_t)q.bad, n.n_contacts}), (uint32_t)SET_SELF_PAIR, 1u, 0u);
    }
    printf("contact schedule scenarios: %s\n", n_wrong ? "WRONG" : "ok");
    return n_wrong ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "scenarios")) return run_scenarios();
    if (argc >= 3 && !strcmp(argv[1], "random")) return run_random(strtoull(argv[2], nullptr, 10), argc >= 4 ? strtoull(argv[3], nullptr, 10) : 1ull);
    fprintf(stderr, "usage: %s scenarios | random N [seed]\n", argv[0]);
    return 2;
}
