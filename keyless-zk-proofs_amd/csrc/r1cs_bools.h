// r1cs_bools.h -- host side of the witness completion's bit rule (r1cs_scan.hip, k16_r1cs_boolean_wires): which wires does the
// circuit itself constrain to {0, 1}?  Pure C++ (no HIP): compiled into libk16.so and, on its own, into
// tests/cpp/r1cs_bools_check.cpp.
//
// A wire x >= 1 is BOOLEAN when some constraint c
//   - has a non-zero MERGED coefficient (r1cs_pairs.h: the terms of a wire in a combination add modulo r) on no wire other than
//     x and wire 0, and
//   - with wire 0 = 1 and A = a1 x + a0, B = b1 x + b0, C = c1 x + c0 has the residual quad x^2 + lin x + k with
//         quad = a1 b1 != 0,   k = a0 b0 - c0 = 0,   lin + quad = 0   (lin = a1 b0 + a0 b1 - c1):
//     quad x (x - 1), whose roots are exactly 0 and 1 (r is prime).
// b (b - 1) = 0, b (1 - b) = 0, b b = b and every scaled form of them qualify.  The marks are a function of the circuit alone.
// Such a constraint is a MARKING ROW of x.  The rows and their wires are handed out too, ascending by constraint: the determinism
// closure's bit rule (k16_r1cs_held_wires) asks which of them a witness leaves unbroken.
// Products are Montgomery products (x y / 2^256): every term of a comparison carries the same factor, the C terms through a
// product with 1, and every operand and result is canonical, so equality of words is equality modulo r.
#pragma once
#include <algorithm>
#include "r1cs_file.h"

namespace k16 {

struct R1csBools {
    std::vector<uint64_t> mark; // [ceil(n_wires / 64)] bit i = wire i is BOOLEAN
    uint64_t              n = 0;
    std::vector<uint32_t> row;      // the marking rows, ascending
    std::vector<uint32_t> row_wire; // [row.size()] the wire each of them marks
};

inline void r1cs_bools_build(const R1csFile& f, R1csBools* out)
{
    const uint64_t M = f.n_constraints;
    struct Term {
        uint32_t wire, matrix;
        uint64_t t;
    };
    std::vector<Term> terms;
    const R1csFr      zero = {{0, 0, 0, 0}}, one = {{1, 0, 0, 0}};
    out->mark.assign(((size_t)f.n_wires + 63) / 64, 0);
    out->n = 0;
    out->row.clear();
    out->row_wire.clear();
    for (uint64_t c = 0; c < M; c++) {
        terms.clear();
        for (uint32_t m = 0; m < 3; m++)
            for (uint64_t t = f.row_start[m * M + c]; t < f.row_start[m * M + c + 1]; t++) terms.push_back({f.wire[t], m, t});
        std::sort(terms.begin(), terms.end(), [](const Term& x, const Term& y) { return x.wire != y.wire ? x.wire < y.wire : x.t < y.t; });
        // k[0]: the merged coefficients of wire 0, k[1]: of the one other wire x
        R1csFr   k[2][3] = {{zero, zero, zero}, {zero, zero, zero}};
        uint32_t x       = 0;
        bool     single  = true;
        for (size_t i = 0; i < terms.size() && single;) {
            const uint32_t w      = terms[i].wire;
            R1csFr         s[3]   = {zero, zero, zero};
            for (; i < terms.size() && terms[i].wire == w; i++) s[terms[i].matrix] = r1cs_fr_add(s[terms[i].matrix], f.coef[terms[i].t]);
            if (r1cs_fr_is_zero(s[0]) && r1cs_fr_is_zero(s[1]) && r1cs_fr_is_zero(s[2])) continue; // (coefficients that cancel name no wire)
            if (w != 0 && x != 0) single = false; // a second wire beside wire 0
            if (w != 0) x = w;
            for (int m = 0; m < 3; m++) k[w != 0][m] = s[m];
        }
        if (!single || x == 0 || x >= f.n_wires) continue;
        const R1csFr *k0 = k[0], *k1 = k[1];
        if (r1cs_fr_is_zero(k1[0]) || r1cs_fr_is_zero(k1[1])) continue;                              // quad = 0
        if (!r1cs_fr_eq(r1cs_fr_mont_mul(k0[0], k0[1]), r1cs_fr_mont_mul(k0[2], one))) continue;     // k != 0
        const R1csFr lhs = r1cs_fr_add(r1cs_fr_add(r1cs_fr_mont_mul(k1[0], k0[1]), r1cs_fr_mont_mul(k0[0], k1[1])), r1cs_fr_mont_mul(k1[0], k1[1]));
        if (!r1cs_fr_eq(lhs, r1cs_fr_mont_mul(k1[2], one))) continue;                                // lin + quad != 0
        uint64_t& word = out->mark[x >> 6];
        out->n += !((word >> (x & 63)) & 1);
        word |= 1ull << (x & 63);
        out->row.push_back((uint32_t)c);
        out->row_wire.push_back(x);
    }
}

} // namespace k16
