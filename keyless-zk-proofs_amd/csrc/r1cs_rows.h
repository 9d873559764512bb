// r1cs_rows.h -- host side of the witness completion (r1cs_scan.hip, k16_r1cs_complete_witness): the terms of a circuit by ROW.
// Pure C++ (no HIP): compiled into libk16.so and, on its own, into tests/cpp/r1cs_rows_check.cpp.
//
// The check's own layout places the 3 M rows A | B | C by LENGTH (r1cs_file.h R1csPlan: slices of 64 rows): good for a pass over
// every row, useless for "the terms of constraint c".  The row view is a CSR over the same rows in the file's order: the terms of
// row id = matrix * M + constraint are term[row_start[id] .. row_start[id + 1]), each one its wire and the POSITION of its
// coefficient in the check's coefficient array (R1csPlan::pos) -- 8 bytes a term, the coefficients are not stored twice.  A wire
// listed twice in a row has two terms here, as in the file: a sum over the row adds them.
#pragma once
#include "r1cs_file.h"

namespace k16 {

struct R1csRowRef {
    uint32_t wire, pos;
};

struct R1csRows {
    std::vector<uint32_t>   row_start; // [3 M + 1]
    std::vector<R1csRowRef> term;      // [n_terms]
};

// R1CS_OK, or R1CS_ERR_ARG for 2^32 terms or more.
inline int r1cs_rows_build(const R1csFile& f, const R1csPlan& plan, R1csRows* out)
{
    const size_t n_rows = f.row_start.size() - 1;
    if (f.n_terms() >= (1ull << 32) || plan.pos.size() != f.n_terms()) return R1CS_ERR_ARG;
    out->row_start.resize(n_rows + 1);
    for (size_t i = 0; i <= n_rows; i++) out->row_start[i] = (uint32_t)f.row_start[i];
    out->term.resize(f.n_terms());
    for (uint64_t t = 0; t < f.n_terms(); t++) out->term[t] = R1csRowRef{f.wire[t], plan.pos[t]};
    return R1CS_OK;
}

} // namespace k16
