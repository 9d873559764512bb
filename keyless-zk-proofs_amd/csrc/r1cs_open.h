// r1cs_open.h -- host side of the open-set solve (r1cs_scan.hip, k16_r1cs_open_system / k16_r1cs_open_direction; DESIGN.md
// section 10h): the kinds of the constraints, the components of the outside wires and the work list of the elimination kernel.
// Pure C++ (no HIP): compiled into libk16.so and, on its own, into tests/cpp/r1cs_open_check.cpp.
//
// Given the incidence list (r1cs_pairs.h), a mask of FIXED wires (wire 0 always is) and the verdicts of the last check:
//   an OUTSIDE wire is one that is not fixed
//   a constraint the check found broken is DROPPED: no equation, no connectivity
//   an unbroken constraint with an outside incidence is LINEAR when its outside wires with A^ != 0 or its outside wires with
//   B^ != 0 are none -- moving the outside wires by t then moves its residual by exactly sum lin t -- and CROSS otherwise
//   the COMPONENTS are those of the bipartite graph of outside wires and unbroken constraints, LINEAR and CROSS alike; a
//   component's id is its lowest wire.  An outside wire whose incidences all lie in dropped constraints is a component of its own
// A component of at most R1CS_OPEN_MAX_WIRES wires is ELIMINATED: the work list holds its wires, ascending -- the columns of its
// matrix -- and a CSR of its LINEAR rows, ascending by constraint, each entry (column, incidence).  The components are grouped
// by size class (<= 16, <= 32, <= 64 wires: one launch each) and ordered by id inside a class.  A larger component is SKIPPED.
// The builder and the walk from one wire take the cap as `max_wires`, R1CS_OPEN_MAX_WIRES .. R1CS_OPEN_MAX_WIRES_EX: two more
// classes (<= 128, <= 256 wires: k_r1cs_open_rref_wide) follow the three, in the same layout; with the
// cap at R1CS_OPEN_MAX_WIRES they are empty and the work list is byte for byte what it was without them.
// Everything here is one linear walk over the outside wires' incidences; nothing iterates to a fixed point except the
// union-find's path halving.
#pragma once
#include <algorithm>
#include "r1cs_pairs.h"

namespace k16 {

constexpr uint32_t R1CS_OPEN_MAX_WIRES    = 64;
constexpr uint32_t R1CS_OPEN_MAX_WIRES_EX = 256;
constexpr uint32_t R1CS_OPEN_NARROW       = 3; // the classes of one wave: <= 16, <= 32, <= 64 wires
constexpr uint32_t R1CS_OPEN_CLASSES      = 5; // and the wide ones: <= 128, <= 256 wires
constexpr uint32_t R1CS_OPEN_NONE         = 0xffffffffu;
constexpr uint32_t r1cs_open_class_wires(uint32_t k) { return 16u << k; }

// what the host alone decides of a wire's class; ELIMINATED wires get theirs from the kernel
enum : uint8_t { R1CS_OPEN_FIXED = 0, R1CS_OPEN_ABSENT = 1, R1CS_OPEN_ELIMINATED = 2, R1CS_OPEN_SKIPPED = 5 };
enum : uint8_t { R1CS_KIND_NONE = 0, R1CS_KIND_LINEAR = 1, R1CS_KIND_CROSS = 2 };

// The constraint-side index over the whole host list: inc[start[c] .. start[c + 1]) are the incidences of constraint c, by wire.
struct R1csOpenIndex {
    std::vector<uint32_t> start, inc;
};
inline void r1cs_open_index(const R1csPairs& P, uint32_t M, R1csOpenIndex* X)
{
    const size_t n = P.pair.size();
    X->start.assign((size_t)M + 1, 0);
    X->inc.assign(n, 0);
    for (size_t i = 0; i < n; i++)
        if (P.pair[i].constraint < M) X->start[P.pair[i].constraint + 1]++;
    for (size_t c = 0; c < M; c++) X->start[c + 1] += X->start[c];
    std::vector<uint32_t> cur(X->start.begin(), X->start.end() - 1);
    for (size_t i = 0; i < n; i++) // (a counting sort keeps the list's order: by wire)
        if (P.pair[i].constraint < M) X->inc[cur[P.pair[i].constraint]++] = (uint32_t)i;
}

// An eliminated component as the kernel reads it.
struct R1csOpenComp {
    uint32_t wire0, n_wires; // its wires: wires[wire0 .. wire0 + n_wires)
    uint32_t row0, n_rows;   // its LINEAR rows: row_start[row0 .. row0 + n_rows], entries ent[row_start[.] ..)
    uint32_t n_cross;        // its CROSS constraints
    uint32_t id;             // its lowest wire
};
struct R1csOpenEntry {
    uint32_t column, inc; // inc: the incidence's index in the host list minus `skip` (the device list leaves wire 0's column out)
};

struct R1csOpenWork {
    std::vector<uint8_t>       kind;       // [M]
    std::vector<uint8_t>       cls;        // [n_wires]: R1CS_OPEN_FIXED / _ABSENT / _ELIMINATED / _SKIPPED
    std::vector<uint32_t>      comp;       // [n_wires]: the component's id, R1CS_OPEN_NONE for FIXED / ABSENT
    std::vector<R1csOpenComp>  comps;      // the eliminated components, by size class, then by id
    uint32_t                   n_class[R1CS_OPEN_CLASSES] = {0, 0, 0, 0, 0};
    std::vector<uint32_t>      wires;      // the eliminated components' wires
    std::vector<uint32_t>      row;        // the constraint of every row
    std::vector<uint32_t>      row_start;  // [rows + 1]
    std::vector<R1csOpenEntry> ent;
    uint64_t                   n_components = 0, n_skipped = 0, n_absent = 0;
};

inline bool r1cs_open_bit(const uint64_t* mask, uint32_t i) { return (mask[i >> 6] >> (i & 63u)) & 1ull; }

// The kind of constraint c.  fixed: n_wires bytes; verdict: bit c = the check found c broken.
inline uint8_t r1cs_open_kind(const R1csPairs& P, const R1csOpenIndex& X, const uint8_t* fixed, const uint64_t* verdict, uint32_t c)
{
    if (r1cs_open_bit(verdict, c)) return R1CS_KIND_NONE;
    bool on_a = false, on_b = false, any = false;
    for (uint32_t k = X.start[c]; k < X.start[c + 1]; k++) {
        const uint32_t i = X.inc[k], w = P.wire[i];
        if (w == 0 || fixed[w]) continue;
        any  = true;
        on_a = on_a || P.pair[i].a != R1CS_PAIR_NONE;
        on_b = on_b || P.pair[i].b != R1CS_PAIR_NONE;
    }
    return !any ? R1CS_KIND_NONE : on_a && on_b ? R1CS_KIND_CROSS : R1CS_KIND_LINEAR;
}

namespace r1cs_open_detail {

// Slots for the components in `ids` (ascending) of at most max_wires wires, grouped by size class; their wires, rows and
// entries.  size[id]: the component's wires; comp[w]: the id of wire w's component; slot: scratch, n_wires words.
inline void fill(const R1csPairs& P, const R1csOpenIndex& X, const uint8_t* fixed, const std::vector<uint32_t>& ids,
                 const std::vector<uint32_t>& size, const std::vector<uint32_t>& members, const std::vector<uint32_t>& rows,
                 std::vector<uint32_t>& slot, uint32_t max_wires, R1csOpenWork* W)
{
    const uint32_t skip = P.start[1];
    // slots by class, then by id
    for (uint32_t k = 0; k < R1CS_OPEN_CLASSES; k++)
        for (uint32_t id : ids) {
            const uint32_t n = size[id];
            if (n > max_wires || n > r1cs_open_class_wires(k) || (k && n <= r1cs_open_class_wires(k - 1))) continue;
            slot[id] = (uint32_t)W->comps.size();
            W->comps.push_back(R1csOpenComp{0, 0, 0, 0, 0, id});
            W->n_class[k]++;
        }
    // wires: `members` lists the outside wires of the components ascending
    for (uint32_t w : members)
        if (W->cls[w] == R1CS_OPEN_ELIMINATED) W->comps[slot[W->comp[w]]].n_wires++;
    uint32_t at = 0;
    for (R1csOpenComp& c : W->comps) {
        c.wire0   = at;
        at += c.n_wires;
        c.n_wires = 0;
    }
    W->wires.assign(at, 0);
    std::vector<uint32_t> column(members.size(), 0); // the column of members[k]
    for (size_t k = 0; k < members.size(); k++) {
        const uint32_t w = members[k];
        if (W->cls[w] != R1CS_OPEN_ELIMINATED) continue;
        R1csOpenComp& c = W->comps[slot[W->comp[w]]];
        column[k]       = c.n_wires;
        W->wires[c.wire0 + c.n_wires++] = w;
    }
    // rows: `rows` lists the unbroken constraints with an outside incidence, ascending.  The first outside wire names the component.
    auto first_outside = [&](uint32_t c) {
        for (uint32_t k = X.start[c]; k < X.start[c + 1]; k++) {
            const uint32_t w = P.wire[X.inc[k]];
            if (w != 0 && !fixed[w]) return w;
        }
        return R1CS_OPEN_NONE;
    };
    std::vector<uint32_t> ents(W->comps.size(), 0);
    for (uint32_t c : rows) {
        const uint32_t w = first_outside(c);
        if (w == R1CS_OPEN_NONE || W->cls[w] != R1CS_OPEN_ELIMINATED) continue;
        R1csOpenComp& k = W->comps[slot[W->comp[w]]];
        if (W->kind[c] == R1CS_KIND_CROSS) {
            k.n_cross++;
            continue;
        }
        k.n_rows++;
        for (uint32_t j = X.start[c]; j < X.start[c + 1]; j++) {
            const uint32_t x = P.wire[X.inc[j]];
            if (x != 0 && !fixed[x]) ents[&k - W->comps.data()]++;
        }
    }
    uint32_t row_at = 0, ent_at = 0;
    std::vector<uint32_t> ent0(W->comps.size(), 0);
    for (size_t s = 0; s < W->comps.size(); s++) {
        R1csOpenComp& k = W->comps[s];
        k.row0   = row_at;
        row_at += k.n_rows;
        k.n_rows = 0;
        ent0[s]  = ent_at;
        ent_at += ents[s];
    }
    W->row.assign(row_at, 0);
    W->row_start.assign((size_t)row_at + 1, 0);
    W->ent.assign(ent_at, R1csOpenEntry{0, 0});
    // the column of a wire: its position among its component's wires -- found through `members`, which is ascending
    auto column_of = [&](uint32_t w) {
        const size_t k = (size_t)(std::lower_bound(members.begin(), members.end(), w) - members.begin());
        return column[k];
    };
    for (uint32_t c : rows) {
        if (W->kind[c] != R1CS_KIND_LINEAR) continue;
        const uint32_t w = first_outside(c);
        if (w == R1CS_OPEN_NONE || W->cls[w] != R1CS_OPEN_ELIMINATED) continue;
        const size_t  s = slot[W->comp[w]];
        R1csOpenComp& k = W->comps[s];
        const uint32_t r = k.row0 + k.n_rows++;
        W->row[r]       = c;
        W->row_start[r] = ent0[s];
        for (uint32_t j = X.start[c]; j < X.start[c + 1]; j++) {
            const uint32_t i = X.inc[j], x = P.wire[i];
            if (x == 0 || fixed[x]) continue;
            W->ent[ent0[s]++] = R1csOpenEntry{column_of(x), i - skip};
        }
        W->row_start[r + 1] = ent0[s];
    }
}

} // namespace r1cs_open_detail

// Every component of the circuit.  fixed: n_wires bytes, non-zero = held fixed; verdict: the check's mask; max_wires: the cap,
// R1CS_OPEN_MAX_WIRES .. R1CS_OPEN_MAX_WIRES_EX (the callers check it).
inline void r1cs_open_build(const R1csPairs& P, const R1csOpenIndex& X, uint32_t n_wires, uint32_t M, const uint8_t* fixed,
                            const uint64_t* verdict, R1csOpenWork* W, uint32_t max_wires = R1CS_OPEN_MAX_WIRES)
{
    *W = R1csOpenWork();
    W->kind.assign(M, R1CS_KIND_NONE);
    W->cls.assign(n_wires, R1CS_OPEN_FIXED);
    W->comp.assign(n_wires, R1CS_OPEN_NONE);
    std::vector<uint32_t> parent(n_wires), size(n_wires, 0), rows, members, ids;
    std::vector<uint8_t>  seen(M, 0);
    auto find = [&](uint32_t x) {
        while (parent[x] != x) {
            parent[x] = parent[parent[x]];
            x         = parent[x];
        }
        return x;
    };
    for (uint32_t w = 1; w < n_wires; w++) { // the outside wires that are in some term
        if (fixed[w]) continue;
        if (P.start[w + 1] == P.start[w]) {
            W->cls[w] = R1CS_OPEN_ABSENT;
            W->n_absent++;
            continue;
        }
        parent[w] = w;
        members.push_back(w);
    }
    // only the constraints an outside wire is in are looked at, each once: the walk is linear in the outside wires' incidences
    for (uint32_t w : members)
        for (uint32_t i = P.start[w]; i < P.start[w + 1]; i++) {
            const uint32_t c = P.pair[i].constraint;
            if (c >= M || seen[c]) continue;
            seen[c] = 1;
            if ((W->kind[c] = r1cs_open_kind(P, X, fixed, verdict, c)) == R1CS_KIND_NONE) continue;
            rows.push_back(c);
            uint32_t root = find(w);
            for (uint32_t k = X.start[c]; k < X.start[c + 1]; k++) {
                const uint32_t y = P.wire[X.inc[k]];
                if (y == 0 || fixed[y]) continue;
                const uint32_t x = find(y);
                if (x != root) { // the lower root stays: a component's root is its lowest wire
                    parent[std::max(x, root)] = std::min(x, root);
                    root                      = std::min(x, root);
                }
            }
        }
    if (rows.size() > M / 16) { // ascending: one pass over the kinds where most constraints are in, a sort where few are
        rows.clear();
        for (uint32_t c = 0; c < M; c++)
            if (W->kind[c] != R1CS_KIND_NONE) rows.push_back(c);
    } else {
        std::sort(rows.begin(), rows.end());
    }
    for (uint32_t w : members) {
        const uint32_t id = find(w);
        W->comp[w]        = id;
        if (!size[id]++) ids.push_back(id); // (id is the component's lowest wire: met first)
    }
    W->n_components = ids.size();
    for (uint32_t w : members) {
        const bool skipped = size[W->comp[w]] > max_wires;
        W->cls[w]          = skipped ? R1CS_OPEN_SKIPPED : R1CS_OPEN_ELIMINATED;
        W->n_skipped += skipped;
    }
    r1cs_open_detail::fill(P, X, fixed, ids, size, members, rows, parent, max_wires, W); // (parent serves as the slot table from here on)
}

// The component of ONE outside wire, by a walk from it: the same work list with that component alone (none when it is SKIPPED).
// *n_wires_out / *n_rows_out / *n_cross_out: the component's wires, LINEAR rows and CROSS constraints, SKIPPED or not.  Returns
// the wire's host class (R1CS_OPEN_FIXED and _ABSENT: no component, the counts are 0).
inline uint8_t r1cs_open_one(const R1csPairs& P, const R1csOpenIndex& X, uint32_t n_wires, uint32_t M, const uint8_t* fixed,
                             const uint64_t* verdict, uint32_t wire, R1csOpenWork* W, uint32_t* n_wires_out, uint32_t* n_rows_out,
                             uint32_t* n_cross_out, uint32_t max_wires = R1CS_OPEN_MAX_WIRES)
{
    *W = R1csOpenWork();
    *n_wires_out = *n_rows_out = *n_cross_out = 0;
    if (wire == 0 || fixed[wire]) return R1CS_OPEN_FIXED;
    if (P.start[wire + 1] == P.start[wire]) return R1CS_OPEN_ABSENT;
    W->kind.assign(M, R1CS_KIND_NONE);
    W->cls.assign(n_wires, R1CS_OPEN_FIXED);
    W->comp.assign(n_wires, R1CS_OPEN_NONE);
    std::vector<uint8_t>  seen_c(M, 0);
    std::vector<uint32_t> members{wire}, rows;
    W->cls[wire] = R1CS_OPEN_ELIMINATED;
    for (size_t at = 0; at < members.size(); at++) { // every wire enters once, every constraint is judged once
        const uint32_t w = members[at];
        for (uint32_t i = P.start[w]; i < P.start[w + 1]; i++) {
            const uint32_t c = P.pair[i].constraint;
            if (c >= M || seen_c[c]) continue;
            seen_c[c] = 1;
            if ((W->kind[c] = r1cs_open_kind(P, X, fixed, verdict, c)) == R1CS_KIND_NONE) continue;
            rows.push_back(c);
            for (uint32_t k = X.start[c]; k < X.start[c + 1]; k++) {
                const uint32_t x = P.wire[X.inc[k]];
                if (x == 0 || fixed[x] || W->cls[x] == R1CS_OPEN_ELIMINATED) continue;
                W->cls[x] = R1CS_OPEN_ELIMINATED;
                members.push_back(x);
            }
        }
    }
    std::sort(members.begin(), members.end());
    std::sort(rows.begin(), rows.end());
    const uint32_t id = members[0];
    *n_wires_out      = (uint32_t)members.size();
    for (uint32_t c : rows) (W->kind[c] == R1CS_KIND_CROSS ? *n_cross_out : *n_rows_out)++;
    const bool skipped = members.size() > max_wires;
    for (uint32_t w : members) {
        W->comp[w] = id;
        W->cls[w]  = skipped ? R1CS_OPEN_SKIPPED : R1CS_OPEN_ELIMINATED;
    }
    W->n_components = 1;
    if (skipped) {
        W->n_skipped = members.size();
        return R1CS_OPEN_SKIPPED;
    }
    std::vector<uint32_t> size(n_wires, 0), slot(n_wires, 0);
    size[id] = (uint32_t)members.size();
    r1cs_open_detail::fill(P, X, fixed, std::vector<uint32_t>{id}, size, members, rows, slot, max_wires, W);
    return R1CS_OPEN_ELIMINATED;
}

} // namespace k16
