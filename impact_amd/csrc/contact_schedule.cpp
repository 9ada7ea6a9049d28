// The bodies of contact_schedule.hpp: plain C++, no HIP.
#include "contact_schedule.hpp"

#include <cmath>
#include <cstring>

namespace {
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

// impact_math/src/random/splitmix.rs:4-10 (vec3.hpp has the same for device code)
inline uint64_t splitmix(uint64_t state) {
    state += 0x9E3779B97F4A7C15ull;
    uint64_t z = state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline uint64_t splitmix2(uint64_t a, uint64_t b) { return splitmix(a ^ splitmix(b)); }

// objects_in_contact_are_interlocked (contact.rs:610-636)
inline bool manifold_interlocked(const ivx_contact* c, size_t n) {
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
H3 max_displacement(const ivx_contact* c, size_t n, F map) {  // contact.rs:691-712
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
inline bool unit_if_above(H3 v, float min_norm, H3& out) {
    const float n2 = hdot(v, v);
    if (!(n2 > min_norm * min_norm)) return false;
    const float n = std::sqrt(n2);
    out = {v.x / n, v.y / n, v.z / n};
    return true;
}
// create_contact_separating_along_axis (contact.rs:714-780)
inline bool separate_along(H3 com_a_minus_b, const ivx_contact* c, size_t n, H3 axis, ivx_contact& out) {
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
// create_separating_contact_for_interlocked_objects (contact.rs:638-689)
inline bool separating_contact(H3 com_a_minus_b, const ivx_contact* c, size_t n, ivx_contact& out) {
    if (n == 0) return false;
    H3 major, middle, minor;
    if (!unit_if_above(max_displacement(c, n, [](H3 p) { return p; }), 1e-6f, major)) return false;
    const H3 md = max_displacement(c, n, [&](H3 p) { return p - major * hdot(p, major); });
    if (!unit_if_above(md, 1e-6f, middle)) return separate_along(com_a_minus_b, c, n, major, out);
    if (!unit_if_above(hcross(major, middle), 1e-4f, minor)) return separate_along(com_a_minus_b, c, n, major, out);
    if (separate_along(com_a_minus_b, c, n, minor, out)) return true;
    return separate_along(com_a_minus_b, c, n, middle, out);
}
}  // namespace

bool ivx_contact_schedule::same_as_resident(const ivx_contact* contacts, size_t n, ivx_contact* out) const {
    bool same = true;
    for_each_manifold(contacts, n, [&](size_t i, size_t cnt) {
        if (manifold_interlocked(contacts + i, cnt)) same = false;
        for (size_t k = i; k < i + cnt && same; ++k) {
            const ivx_contact& c = contacts[k];
            same = c.id == cache[k].id && c.body_a == slot_bodies[2 * k] && c.body_b == slot_bodies[2 * k + 1];
            out[k] = c;
        }
        return same;
    });
    return same;
}

ivx_contact_schedule::Verdict ivx_contact_schedule::validate(const ivx_contact* contacts, size_t n, uint32_t n_dyn, uint32_t n_kin) {
    Verdict v{CONTACT_OK, 0, false};
    for_each_manifold(contacts, n, [&](size_t i, size_t cnt) {
        for (size_t j = i; j < i + cnt; ++j) {
            const ivx_contact& c = contacts[j];
            const uint32_t la = (c.body_a & IVX_KINEMATIC_BODY) ? n_kin : n_dyn, lb = (c.body_b & IVX_KINEMATIC_BODY) ? n_kin : n_dyn;
            v.index = j;
            if (!((c.body_a & 0x7FFFFFFFu) < la && (c.body_b & 0x7FFFFFFFu) < lb)) v.kind = CONTACT_MISSING_BODY;
            else if (c.body_a == c.body_b) v.kind = CONTACT_SELF_PAIR;
            if (v.kind != CONTACT_OK) return false;
        }
        if (manifold_interlocked(contacts + i, cnt)) v.any_interlocked = true;
        return true;
    });
    return v;
}

int ivx_contact_schedule::replace_interlocked(const ivx_contact* contacts, size_t n, const std::function<int(uint32_t, float*)>& body_position) {
    effective.clear();
    int rc = 0;
    for_each_manifold(contacts, n, [&](size_t i, size_t cnt) {
        const ivx_contact* m = contacts + i;
        bool replaced = false;
        if (manifold_interlocked(m, cnt)) {
            float pa[3], pb[3];
            if ((rc = body_position(m[0].body_a, pa))) return false;
            if ((rc = body_position(m[0].body_b, pb))) return false;
            ivx_contact sep;
            if (separating_contact(h3(pa) - h3(pb), m, cnt, sep)) {
                sep.body_a = m[0].body_a;
                sep.body_b = m[0].body_b;
                effective.push_back(sep);
                replaced = true;
            }
        }
        if (!replaced) effective.insert(effective.end(), m, m + cnt);
        return true;
    });
    return rc;
}

void ivx_contact_schedule::id_table_reset(size_t want) {
    size_t cap = 1024;
    while (cap < 2 * want) cap *= 2;
    id_keys.assign(cap, 0ull);
    id_vals.assign(cap, 0xFFFFFFFFu);
    id_used = 0;
    for (uint32_t s = 0; s < cache.size(); ++s) {
        size_t h = id_hash(cache[s].id) & (cap - 1);
        while (id_vals[h] != 0xFFFFFFFFu) h = (h + 1) & (cap - 1);
        id_keys[h] = cache[s].id;
        id_vals[h] = s;
        id_used += 1;
    }
}

void ivx_contact_schedule::id_erase(uint64_t id) {
    const size_t mask = id_keys.size() - 1;
    size_t h = id_find_pos(id);
    if (id_vals[h] == 0xFFFFFFFFu) return;
    size_t hole = h;
    for (size_t j = (h + 1) & mask; id_vals[j] != 0xFFFFFFFFu; j = (j + 1) & mask) {
        const size_t home = id_hash(id_keys[j]) & mask;
        // the entry at j may move into the hole unless its home lies (cyclically) in (hole, j]
        const bool stays = hole <= j ? (home > hole && home <= j) : (home > hole || home <= j);
        if (!stays) {
            id_keys[hole] = id_keys[j];
            id_vals[hole] = id_vals[j];
            hole = j;
        }
    }
    id_vals[hole] = 0xFFFFFFFFu;
    id_used -= 1;
}

uint32_t ivx_contact_schedule::register_contacts(const ivx_contact* eff, size_t n_eff) {
    if (id_keys.empty() || 2 * (cache.size() + n_eff) > id_keys.size()) id_table_reset(cache.size() + n_eff);
    const size_t old_len = cache.size();
    size_t cursor = 0;
    cache.reserve(old_len + n_eff);
    for (uint32_t e = 0; e < n_eff; ++e) {
        const uint64_t id = eff[e].id;
        if (cursor < old_len && cache[cursor].id == id) {
            cache[cursor].src = e;
            cache[cursor].prepared = true;
            cursor += 1;
            continue;
        }
        const size_t h = id_find_pos(id);
        if (id_vals[h] != 0xFFFFFFFFu) {
            Entry& en = cache[id_vals[h]];
            en.src = e;
            en.prepared = true;
            cursor = (size_t)id_vals[h] + 1;
        } else {
            id_keys[h] = id;
            id_vals[h] = (uint32_t)cache.size();
            id_used += 1;
            cache.push_back(Entry{id, -1, e, true});
        }
    }
    size_t idx = 0, len = cache.size();
    while (idx < len) {
        if (cache[idx].prepared) {
            ++idx;
        } else {
            id_erase(cache[idx].id);
            cache[idx] = cache[len - 1];
            cache.pop_back();
            --len;
            if (idx < len) id_vals[id_find_pos(cache[idx].id)] = (uint32_t)idx;
        }
    }
    n_bodies_valid = false;
    return (uint32_t)cache.size();
}

void ivx_contact_schedule::write_slot_order(const ivx_contact* eff, ivx_contact* out) {
    const uint32_t nc = (uint32_t)cache.size();
    prev_slot_host.resize(nc);
    slot_bodies.resize(2 * (size_t)nc);
    for (uint32_t sl = 0; sl < nc; ++sl) {
        Entry& en = cache[sl];
        const ivx_contact& c = eff[en.src];
        out[sl] = c;
        slot_bodies[2 * (size_t)sl] = c.body_a;
        slot_bodies[2 * (size_t)sl + 1] = c.body_b;
        prev_slot_host[sl] = en.prev_slot;
        en.prev_slot = (int32_t)sl;
        en.prepared = false;
    }
}

void ivx_contact_schedule::build_chains() {
    chain_start.clear();
    chain_bodies.clear();
    const uint32_t n = (uint32_t)(slot_bodies.size() / 2);
    uint32_t s = 0;
    while (s < n) {
        uint32_t e = s + 1;
        while (e < n && e - s < PHYS_CHAIN_MAX && slot_bodies[2 * (size_t)e] == slot_bodies[2 * (size_t)s] && slot_bodies[2 * (size_t)e + 1] == slot_bodies[2 * (size_t)s + 1]) ++e;
        chain_start.push_back(s);
        chain_bodies.push_back(slot_bodies[2 * (size_t)s]);
        chain_bodies.push_back(slot_bodies[2 * (size_t)s + 1]);
        s = e;
    }
    chain_start.push_back(n);
}

bool ivx_contact_schedule::build_levels(bool keep, uint32_t n_iterations, uint32_t n_positional, uint32_t n_dyn, uint32_t n_kin) {
    if (keep && chain_start == prev_chain_start && chain_bodies == prev_chain_bodies) return true;
    level_start_host.clear();
    build_phase_levels(1u, n_iterations, 0, n_dyn, n_kin);
    build_phase_levels(0u, n_positional, 1, n_dyn, n_kin);
    forms_built = 0;
    prev_chain_start = chain_start;
    prev_chain_bodies = chain_bodies;
    return false;
}

void ivx_contact_schedule::build_form(uint32_t form, uint32_t n_iterations, uint32_t n_positional, uint32_t n_dyn) {
    if (form == 1u) {
        items_host.clear();
        item_bodies_host.clear();
        item_tags_host.clear();
        tile_base_host.clear();
        tile_first_host.clear();
        build_items(PHYS_ITEM_WARM, 1u, PHYS_ITEM_VELOCITY, n_iterations, 0, n_dyn);
        build_items(PHYS_ITEM_POSITIONAL, 0u, PHYS_ITEM_POSITIONAL, n_positional, 1, n_dyn);
    } else {
        cs_item_host.clear();
        cs_bodies_host.clear();
        cs_vers_host.clear();
        cs_round_start_host.clear();
        cs_round_mask_host.clear();
        cs_round_level_host.clear();
        cs_slot_of_host.clear();
        build_stationary(0, n_chains(), n_iterations + 1u, n_dyn);
        build_stationary(1, n_chains(), n_positional, n_dyn);
    }
}

uint32_t ivx_contact_schedule::constrained_bodies(const std::vector<uint32_t>& joint_refs, uint32_t n_dyn, uint32_t n_kin) {
    if (n_bodies_valid) return n_bodies;
    std::vector<uint8_t> t((size_t)n_dyn + n_kin, 0);
    for (size_t sl = 0; sl + 1 < slot_bodies.size(); sl += 2) {
        const uint32_t a = slot_bodies[sl], b = slot_bodies[sl + 1];
        if (a & IVX_KINEMATIC_BODY) t[n_dyn + (a & 0x7FFFFFFFu)] = 1;
        else if (a < n_dyn) t[a] = 1;
        if (b & IVX_KINEMATIC_BODY) t[n_dyn + (b & 0x7FFFFFFFu)] = 1;
        else if (b < n_dyn) t[b] = 1;
    }
    for (uint32_t r : joint_refs)
        if (!(r & IVX_KINEMATIC_BODY) && r < n_dyn) t[r] = 1;
    uint32_t nb = 0;
    for (uint8_t x : t) nb += x;
    n_bodies = nb;
    n_bodies_valid = true;
    return nb;
}

// can this phase run chain-stationary at all? (its tiles fit the working workgroups, no body with more than 65535 chains)
bool ivx_contact_schedule::stationary_feasible(uint32_t nch, uint32_t passes, uint32_t n_dyn) {
    const uint32_t n_tiles = (nch + 31u) / 32u;
    if (nch == 0 || passes == 0 || n_tiles > PHYS_CS_WAVES * PHYS_CS_MAX_GROUPS) return false;
    std::vector<uint32_t>& deg = scratch_count;
    deg.assign(n_dyn, 0u);
    for (uint32_t ch = 0; ch < nch; ++ch)
        for (int side = 0; side < 2; ++side) {
            const uint32_t b = chain_bodies[2 * (size_t)ch + side];
            if (!(b & IVX_KINEMATIC_BODY)) deg[b] += 1u;
        }
    for (uint32_t b = 0; b < n_dyn; ++b)
        if (deg[b] > 0xFFFFu) return false;
    return true;
}

// Dependency levels of a phase's item sequence (pass-major, chains in cache order inside a pass); items of one level touch pairwise
// different dynamic bodies: the level of every item (`lvl_host`), the levels' extents (`level_start_host`) and what the launcher needs to
// choose a kernel (levels, widest level, whether the chain-stationary form exists).
void ivx_contact_schedule::build_phase_levels(uint32_t n_first, uint32_t n_passes, int phase, uint32_t n_dyn, uint32_t n_kin) {
    ivx_world_lap slap(2);
    const uint32_t nch = (uint32_t)chain_start.size() - 1u, nb = n_dyn;
    const uint32_t total_passes = n_first + n_passes;
    const size_t total = (size_t)total_passes * nch;
    phase_items[phase] = (uint32_t)total;
    item_offset[phase] = phase ? phase_items[0] : 0u;
    level_offset[phase] = (uint32_t)level_start_host.size();
    n_levels[phase] = 0;
    max_level_items[phase] = 0;
    cs_feasible[phase] = 0;
    std::vector<uint32_t>& lvl = lvl_host[phase];
    lvl.clear();
    if (phase == 1) {
        kin_offsets_host.assign((size_t)n_kin + 1, 0u);
        kin_list_host.clear();
        cs_slot_of_level.clear();
        n_kin_items = 0;
    }
    if (total == 0) {
        level_start_host.push_back(0);
        return;
    }
    std::vector<uint32_t>& last = scratch_last;
    lvl.resize(total);
    last.assign(nb, 0u);
    uint32_t max_level = 0;
    size_t k = 0;
    for (uint32_t pass = 0; pass < total_passes; ++pass)
        for (uint32_t ch = 0; ch < nch; ++ch, ++k) {
            const uint32_t ba = chain_bodies[2 * (size_t)ch], bb = chain_bodies[2 * (size_t)ch + 1];
            uint32_t l = 0;
            if (!(ba & IVX_KINEMATIC_BODY)) l = std::max(l, last[ba]);
            if (!(bb & IVX_KINEMATIC_BODY)) l = std::max(l, last[bb]);
            l += 1;
            if (!(ba & IVX_KINEMATIC_BODY)) last[ba] = l;
            if (!(bb & IVX_KINEMATIC_BODY)) last[bb] = l;
            lvl[k] = l;
            max_level = std::max(max_level, l);
        }
    slap("schedule: levels");
    // counting sort by level (stable): level l (from 1) holds the items [start[l - 1], start[l])
    const size_t ls0 = level_start_host.size();
    level_start_host.resize(ls0 + max_level + 1, 0u);
    uint32_t* start = level_start_host.data() + ls0;
    for (size_t i = 0; i < total; ++i) start[lvl[i]] += 1;  // start[l] = count of level l (l >= 1), start[0] = 0
    uint32_t run = 0, widest = 0;
    for (uint32_t l = 1; l <= max_level; ++l) {
        const uint32_t c = start[l];
        widest = std::max(widest, c);
        run += c;
        start[l] = run;  // end of level l = begin of level l + 1
    }
    n_levels[phase] = max_level;
    max_level_items[phase] = widest;
    cs_feasible[phase] = stationary_feasible(nch, total_passes, n_dyn) ? 1 : 0;
    if (phase == 1 && n_kin) {
        // positional phase with kinematic bodies (ReplayView): every kinematic body's chains in solve order, by the items' places in the level order
        std::vector<uint32_t> cursor(start, start + max_level);
        std::vector<std::vector<uint32_t>> kin_items(n_kin);
        cs_slot_of_level.assign(total, 0u);
        k = 0;
        for (uint32_t pass = 0; pass < total_passes; ++pass)
            for (uint32_t ch = 0; ch < nch; ++ch, ++k) {
                const uint32_t slot = cursor[lvl[k] - 1]++;
                cs_slot_of_level[k] = slot;
                const uint32_t ba = chain_bodies[2 * (size_t)ch], bb = chain_bodies[2 * (size_t)ch + 1];
                if (ba & IVX_KINEMATIC_BODY) kin_items[ba & 0x7FFFFFFFu].push_back(slot);
                if (bb & IVX_KINEMATIC_BODY) kin_items[bb & 0x7FFFFFFFu].push_back(slot | 0x80000000u);
            }
        kin_offsets_host.assign(1, 0u);
        for (const auto& v : kin_items) {
            kin_list_host.insert(kin_list_host.end(), v.begin(), v.end());
            kin_offsets_host.push_back((uint32_t)kin_list_host.size());
        }
        n_kin_items = (uint32_t)kin_list_host.size();
        if (n_kin_items == 0) cs_slot_of_level.clear();
    }
    slap("schedule: extents");
}

// the level-ordered item list of a phase, its hand-off tags and tiles (k_solve, k_solve_mg); appends to the host arrays (phase 0 first)
void ivx_contact_schedule::build_items(uint32_t first_type, uint32_t n_first, uint32_t type, uint32_t n_passes, int phase, uint32_t n_dyn) {
    ivx_world_lap slap(2);
    const uint32_t nch = (uint32_t)chain_start.size() - 1u, nb = n_dyn;
    const uint32_t total_passes = n_first + n_passes;
    const size_t total = (size_t)total_passes * nch;
    const std::vector<uint32_t>& lvl = lvl_host[phase];
    const uint32_t max_level = n_levels[phase];
    const size_t ls0 = level_offset[phase];
    tile_offset[phase] = (uint32_t)tile_first_host.size();
    n_tiles[phase] = 0;
    tile_base_host.resize(ls0 + max_level + 1, 0u);
    if (total == 0) return;
    const uint32_t* start = level_start_host.data() + ls0;
    const size_t it0 = items_host.size();
    items_host.resize(it0 + total);
    item_bodies_host.resize(2 * (it0 + total));
    item_tags_host.resize(4 * (it0 + total));
    std::vector<uint32_t>& seen = scratch_count;  // per dynamic body: items of this phase that have touched it so far
    seen.assign(nb, 0u);
    std::vector<uint32_t> cursor(start, start + max_level);
    size_t k = 0;
    for (uint32_t pass = 0; pass < total_passes; ++pass) {
        const uint32_t ty = pass < n_first ? first_type : type;
        for (uint32_t ch = 0; ch < nch; ++ch, ++k) {
            const uint32_t s0 = chain_start[ch], len = chain_start[ch + 1] - s0;
            const size_t slot = it0 + cursor[lvl[k] - 1]++;
            items_host[slot] = s0 | (len << 24) | (ty << 28);
            const uint32_t ba = chain_bodies[2 * (size_t)ch], bb = chain_bodies[2 * (size_t)ch + 1];
            item_bodies_host[2 * slot] = (ba & IVX_KINEMATIC_BODY) ? n_dyn + (ba & 0x7FFFFFFFu) : ba;
            item_bodies_host[2 * slot + 1] = (bb & IVX_KINEMATIC_BODY) ? n_dyn + (bb & 0x7FFFFFFFu) : bb;
            // the hand-off tags (k_solve_mg): the versions of the two bodies' records this item waits for (it leaves them one higher), and the
            // sweep tag on the accumulated impulses — written by the velocity sweeps only: sweep q finds q (0: as prepared) and leaves q + 1
            uint32_t* tg = &item_tags_host[4 * slot];
            tg[0] = (ba & IVX_KINEMATIC_BODY) ? 0u : seen[ba]++;
            tg[1] = (bb & IVX_KINEMATIC_BODY) ? 0u : seen[bb]++;
            const uint32_t sweep = pass < n_first ? 0u : pass - n_first;
            tg[2] = sweep;
            tg[3] = sweep + 1u;
        }
    }
    slap("schedule: items");
    // tiles of 64 consecutive items of a level (the packed records of the multi-workgroup solve); tile_base runs parallel to level_start
    uint32_t nt = 0;
    for (uint32_t l = 0; l < max_level; ++l) {
        tile_base_host[ls0 + l] = nt;
        for (uint32_t i = start[l]; i < start[l + 1]; i += 64u) {
            tile_first_host.push_back(i | ((std::min(64u, start[l + 1] - i) - 1u) << 26));
            nt += 1;
        }
    }
    tile_base_host[ls0 + max_level] = nt;
    n_tiles[phase] = nt;
    slap("schedule: tiles");
}

// The chain-stationary form of a phase's schedule (physics.hip, k_solve_cs): every chain gets a pair of lanes of one wave for the whole
// phase. Tiles are 32 consecutive chains in the order (level of the chain's first item, solve order) — the chains of a level are mutually
// independent and tend to stay so in every sweep —, a workgroup is PHYS_CS_WAVES consecutive tiles. A tile's rounds are the distinct levels
// its items lie on, in level order, each a mask of the lanes whose next item it is: a round's items are of one level, so they depend on
// lower levels only and every wave walks its rounds in level order — the lowest unfinished level can always run while all workgroups are
// resident. lvl_host[phase]: level (from 1) of item pass * nch + chain.
void ivx_contact_schedule::build_stationary(int phase, uint32_t nch, uint32_t passes, uint32_t n_dyn) {
    ivx_world_lap slap(2);
    const std::vector<uint32_t>& lvl = lvl_host[phase];
    CsSchedule& c = cs[phase];
    c = CsSchedule();
    c.slot_offset = (uint32_t)cs_item_host.size();
    c.round_start_offset = (uint32_t)cs_round_start_host.size();
    c.round_offset = (uint32_t)cs_round_mask_host.size();
    const uint32_t nt = (nch + 31u) / 32u;
    if (!cs_feasible[phase]) return;
    // degree of every dynamic body (chains that touch it) and a chain's rank among them: before sweep s of the chain the body's record has
    // been written s * degree + rank times (every sweep walks the chains in the same order)
    std::vector<uint32_t>& deg = scratch_count;
    deg.assign(n_dyn, 0u);
    std::vector<uint32_t>& rank = scratch_rank;
    rank.resize(2 * (size_t)nch);
    for (uint32_t ch = 0; ch < nch; ++ch)
        for (int side = 0; side < 2; ++side) {
            const uint32_t b = chain_bodies[2 * (size_t)ch + side];
            rank[2 * (size_t)ch + side] = (b & IVX_KINEMATIC_BODY) ? 0u : deg[b]++;
        }
    slap("stationary: degrees");
    // the chains by the level of their first item, solve order inside a level: a counting sort (levels are small integers)
    const uint32_t max_level = n_levels[phase];
    std::vector<uint32_t>& order = scratch_order;
    order.resize(nch);
    {
        std::vector<uint32_t>& first = scratch_first;
        first.assign(max_level + 2u, 0u);
        for (uint32_t ch = 0; ch < nch; ++ch) first[lvl[ch] + 1u] += 1u;
        for (uint32_t l = 1; l <= max_level + 1u; ++l) first[l] += first[l - 1u];
        for (uint32_t ch = 0; ch < nch; ++ch) order[first[lvl[ch]]++] = ch;
    }
    slap("stationary: order");
    const size_t slot0 = c.slot_offset;
    cs_item_host.resize(slot0 + (size_t)nt * 64u, 0xFFFFFFFFu);
    cs_bodies_host.resize(2 * (slot0 + (size_t)nt * 64u), 0u);
    cs_vers_host.resize(slot0 + (size_t)nt * 64u, 0u);
    // a tile's rounds: the lanes of every level its items lie on — a table of lane masks over the levels and a bitmap of the levels touched,
    // walked in ascending order afterwards (no sort: the levels are small integers)
    std::vector<uint64_t>& mask_of = scratch_mask;
    mask_of.assign(max_level + 1u, 0ull);
    std::vector<uint64_t>& bits = scratch_bits;
    bits.assign((max_level + 64u) / 64u, 0ull);
    cs_round_mask_host.reserve(cs_round_mask_host.size() + (size_t)nt * 64u);
    cs_round_level_host.reserve(cs_round_level_host.size() + (size_t)nt * 64u);
    for (uint32_t t = 0; t < nt; ++t) {
        const uint32_t first = t * 32u, cnt = std::min(32u, nch - first);
        uint32_t lo_w = 0xFFFFFFFFu, hi_w = 0u;
        for (uint32_t l = 0; l < cnt; ++l) {
            const uint32_t ch = order[first + l];
            const uint32_t s0 = chain_start[ch], len = chain_start[ch + 1] - s0;
            uint32_t body[2];
            for (int side = 0; side < 2; ++side) {
                const uint32_t b = chain_bodies[2 * (size_t)ch + side];
                body[side] = (b & IVX_KINEMATIC_BODY) ? n_dyn + (b & 0x7FFFFFFFu) : b;
            }
            for (int side = 0; side < 2; ++side) {
                const size_t slot = slot0 + (size_t)t * 64u + 2u * l + side;
                const uint32_t b = chain_bodies[2 * (size_t)ch + side];
                cs_item_host[slot] = s0 | (len << 24);
                cs_bodies_host[2 * slot] = body[side];
                cs_bodies_host[2 * slot + 1] = body[side ^ 1];
                cs_vers_host[slot] = (b & IVX_KINEMATIC_BODY) ? 0u : (deg[b] | (rank[2 * (size_t)ch + side] << 16));
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
        cs_round_start_host.push_back((uint32_t)(cs_round_mask_host.size() - c.round_offset));
        for (uint32_t wd = lo_w; wd <= hi_w && lo_w != 0xFFFFFFFFu; ++wd) {
            uint64_t m = bits[wd];
            bits[wd] = 0ull;
            while (m) {
                const uint32_t lv = wd * 64u + (uint32_t)__builtin_ctzll(m);
                m &= m - 1ull;
                cs_round_mask_host.push_back(mask_of[lv]);
                cs_round_level_host.push_back(lv);
                mask_of[lv] = 0ull;
            }
        }
    }
    cs_round_start_host.push_back((uint32_t)(cs_round_mask_host.size() - c.round_offset));
    slap("stationary: tiles");
    if (phase == 1 && !cs_slot_of_level.empty()) {  // ReplayView's item indices, by pair of lanes and sweep instead of by pass and chain
        cs_slot_of_host.assign((size_t)nt * 32u * passes, 0u);
        for (uint32_t i = 0; i < nch; ++i)
            for (uint32_t p = 0; p < passes; ++p) cs_slot_of_host[(size_t)i * passes + p] = cs_slot_of_level[(size_t)p * nch + order[i]];
    }
    c.n_tiles = nt;
}
