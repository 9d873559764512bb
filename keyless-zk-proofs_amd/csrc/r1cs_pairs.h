// r1cs_pairs.h -- host side of the unbound-wire scan (r1cs_check.hip, k16_r1cs_unbound_wires): the (wire, constraint)
// incidences of a circuit.  Pure C++ (no HIP): compiled into libk16.so and, on its own, into tests/cpp/r1cs_pairs_check.cpp.
//
// An INCIDENCE is a pair (wire i, constraint c) in which at least one of the three MERGED coefficients A^_ci, B^_ci, C^_ci is
// non-zero: the terms of wire i in a combination add modulo r, as the check treats a wire listed twice (r1cs_file.h), and a sum
// of zero is no coefficient.  The list is ordered by wire, then by constraint; start[i] .. start[i + 1] is the column of wire i
// (what k16_r1cs_wire_constraints reads), and bit i of `present` says that the column is not empty -- the static half of a
// wire's class: a wire without a column is ABSENT whatever the witness holds.
//
// An incidence does not carry its coefficients, it NAMES them (20 bytes instead of 100): a position below n_entries is an entry
// of the check's own coefficient array (R1csPlan::pos of the one term the wire has in that combination), a position
// n_entries + k is side[k], the merged sum of a wire listed more than once, and R1CS_PAIR_NONE stands for zero.  `side` is kept in
// standard form; the caller scales it the way it scaled the entries.
#pragma once
#include "r1cs_file.h"

namespace k16 {

constexpr uint32_t R1CS_PAIR_NONE = 0xffffffffu;

struct R1csPair {
    uint32_t constraint, a, b, c; // positions of A^, B^, C^ (see above)
};

struct R1csPairs {
    std::vector<uint32_t> start;   // [n_wires + 1]
    std::vector<uint32_t> wire;    // [n_pairs]: the wire of each incidence (ascending)
    std::vector<R1csPair> pair;    // [n_pairs]
    std::vector<R1csFr>   side;    // merged sums of duplicated wires, standard form, non-zero
    std::vector<uint64_t> present; // [ceil(n_wires / 64)]
    uint32_t              n_entries = 0; // of the plan the positions refer to
    uint64_t n_pairs() const { return pair.size(); }
};

// R1CS_OK, or R1CS_ERR_ARG for 2^32 incidences or more, or when entries and side table together leave no room for the sentinel.
inline int r1cs_pairs_build(const R1csFile& f, const R1csPlan& plan, R1csPairs* out)
{
    const uint64_t M = f.n_constraints;
    struct Term {
        uint32_t wire, matrix;
        uint64_t t;
    };
    struct Found {
        uint32_t wire;
        R1csPair p;
    };
    std::vector<Term>  terms;
    std::vector<Found> found; // in the order of the constraints
    out->side.clear();
    out->n_entries = (uint32_t)plan.plan.n_entries;
    out->start.assign((size_t)f.n_wires + 1, 0);
    for (uint64_t c = 0; c < M; c++) {
        terms.clear();
        for (uint32_t m = 0; m < 3; m++)
            for (uint64_t t = f.row_start[m * M + c]; t < f.row_start[m * M + c + 1]; t++) terms.push_back({f.wire[t], m, t});
        std::sort(terms.begin(), terms.end(), [](const Term& x, const Term& y) {
            return x.wire != y.wire ? x.wire < y.wire : (x.matrix != y.matrix ? x.matrix < y.matrix : x.t < y.t);
        });
        for (size_t i = 0; i < terms.size();) {
            Found fd = {terms[i].wire, {(uint32_t)c, R1CS_PAIR_NONE, R1CS_PAIR_NONE, R1CS_PAIR_NONE}};
            bool  any = false;
            while (i < terms.size() && terms[i].wire == fd.wire) { // one (wire, matrix) group after the other
                const uint32_t m     = terms[i].matrix;
                const size_t   first = i;
                R1csFr         sum   = f.coef[terms[i++].t];
                while (i < terms.size() && terms[i].wire == fd.wire && terms[i].matrix == m) sum = r1cs_fr_add(sum, f.coef[terms[i++].t]);
                if (r1cs_fr_is_zero(sum)) continue;
                uint32_t pos;
                if (i - first == 1) {
                    pos = plan.pos[terms[first].t];
                } else {
                    if ((uint64_t)out->n_entries + out->side.size() >= R1CS_PAIR_NONE) return R1CS_ERR_ARG;
                    pos = out->n_entries + (uint32_t)out->side.size();
                    out->side.push_back(sum);
                }
                (m == 0 ? fd.p.a : m == 1 ? fd.p.b : fd.p.c) = pos;
                any = true;
            }
            if (!any) continue;
            if (found.size() >= 0xffffffffull) return R1CS_ERR_ARG; // (2^32 - 1 incidences at the most)
            found.push_back(fd);
            out->start[(size_t)fd.wire + 1]++;
        }
    }
    // by wire, the constraints of a wire ascending: a counting sort keeps the order they were found in
    for (size_t i = 0; i < f.n_wires; i++) out->start[i + 1] += out->start[i];
    out->wire.assign(found.size(), 0);
    out->pair.assign(found.size(), R1csPair{0, R1CS_PAIR_NONE, R1CS_PAIR_NONE, R1CS_PAIR_NONE});
    {
        std::vector<uint32_t> cur(out->start.begin(), out->start.end() - 1);
        for (const Found& fd : found) {
            const uint32_t at = cur[fd.wire]++;
            out->wire[at]     = fd.wire;
            out->pair[at]     = fd.p;
        }
    }
    out->present.assign(((size_t)f.n_wires + 63) / 64, 0);
    for (size_t i = 0; i < f.n_wires; i++)
        if (out->start[i + 1] != out->start[i]) out->present[i >> 6] |= 1ull << (i & 63);
    return R1CS_OK;
}

} // namespace k16
