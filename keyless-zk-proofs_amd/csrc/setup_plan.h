// setup_plan.h -- host side of the set-up from a trapdoor (setup.hip, include/k16.h k16_r1cs_setup*): the shape and exact size
// of the zkey a circuit gets, the TRANSPOSED layout of its three matrices for the column kernel, and the writer of everything
// in the key that is no curve point (container, section 1, the header's integers, section 4, section 10).  Pure C++ (no HIP):
// compiled into libk16.so and, on its own, into tests/cpp/setup_plan_check.cpp.
//
// The key (snarkjs Groth16 zkey, the layout the prover's parser reads; formulas in DESIGN.md section 11):
//   magic "zkey", u32 version = 1, u32 nSections = 10, then the sections 1 .. 10 in this order, { u32 type, u64 size, payload }
//   1   u32 protocol = 1 (Groth16)
//   2   u32 n8q = 32, q, u32 n8r = 32, r, u32 nVars, u32 nPublic, u32 domain N, alpha1, beta1, beta2, gamma2, delta1, delta2
//   3   IC: nPublic + 1 G1 points            4   u32 count, then 44-byte records { u32 m, u32 c, u32 wire, coef * 2^512 mod r }
//   5   A: nVars G1      6   B1: nVars G1    7   B2: nVars G2      8   C: nVars - nPublic - 1 G1      9   H: N G1
//   10  64-byte circuit hash (written as zeros: nothing here computes snarkjs's hash), u32 nContributions = 0
// G1 points are 64 bytes, G2 points 128 bytes, affine Montgomery, (0,0) = infinity.
// Section 4, pinned by the reference-made tests/golden/toy/toy_1.zkey: for every constraint c its A terms (m = 0), then its B
// terms (m = 1), in the file's order and unmerged; behind the last constraint the rows { 0, M + s, s, 2^512 mod r } for
// s = 0 .. nPublic.  (The toy's order is this order: A of a constraint before its B, public rows last.)
// Domain: N = the smallest power of two >= M + nPublic + 1.
//
// Columns.  The QAP value of wire i in matrix m at tau is sum over the terms (c, i, k) of k * L_c(tau): a sparse
// matrix-vector product with the TRANSPOSED matrices.  Row id = m * nWires + wire (m: 0 = A, 1 = B, 2 = C), its entries
// (constraint, coefficient); row wire of A also holds (M + wire, 1) for wire <= nPublic, the row snarkjs appends.  The rows
// go through spmv_plan_rows like the prover's and the witness check's: the gathered vector is L(tau) in the witness's place.
#pragma once
#include "r1cs_file.h"

namespace k16 {

struct SetupShape {
    uint32_t n_wires = 0, n_public = 0, M = 0, N = 0, log_n = 0;
    uint64_t n_records = 0; // section 4
    // payload offset and size of section s (1 .. 10) in the file
    uint64_t off[11] = {0}, size[11] = {0};
    uint64_t total = 0;
};
constexpr uint64_t SETUP_HEADER_INTS = 4 + 32 + 4 + 32 + 12; // section 2 up to alpha1

// R1CS_ERR_ARG for a circuit with no constraint, with 3 * nWires >= 2^32 (row numbers of the column plan) or with a domain
// above 2^27 (Fr has no 2^29-th root of unity)
inline int setup_shape(const R1csFile& f, SetupShape* s, const char** why = nullptr)
{
    const char* dummy;
    if (!why) why = &dummy;
    *why = "";
    if (f.n_constraints == 0) {
        *why = "setup: the circuit has no constraint";
        return R1CS_ERR_ARG;
    }
    if (3 * (uint64_t)f.n_wires >= (1ull << 32)) {
        *why = "setup: too many wires for 32-bit row numbers";
        return R1CS_ERR_ARG;
    }
    s->n_wires  = f.n_wires;
    s->n_public = f.n_public();
    s->M        = f.n_constraints;
    const uint64_t need = (uint64_t)s->M + s->n_public + 1; // < 2^32 / 3 + 2^32 / 3: N <= 2^31
    s->log_n = 0;
    while ((1ull << s->log_n) < need) s->log_n++;
    if (s->log_n > 27) { // r - 1 = 2^28 * odd: the transforms need a primitive 2N-th root of unity
        *why = "setup: the domain would exceed 2^27";
        return R1CS_ERR_ARG;
    }
    s->N         = 1u << s->log_n;
    s->n_records = f.row_start[2 * (uint64_t)s->M] + s->n_public + 1; // the terms of A and B
    const uint64_t nw = s->n_wires, np1 = (uint64_t)s->n_public + 1;
    s->size[1]  = 4;
    s->size[2]  = SETUP_HEADER_INTS + 3 * 64 + 3 * 128;
    s->size[3]  = np1 * 64;
    s->size[4]  = 4 + 44 * s->n_records;
    s->size[5]  = nw * 64;
    s->size[6]  = nw * 64;
    s->size[7]  = nw * 128;
    s->size[8]  = (nw - np1) * 64;
    s->size[9]  = (uint64_t)s->N * 64;
    s->size[10] = 64 + 4;
    uint64_t pos = 12;
    for (int k = 1; k <= 10; k++) {
        s->off[k] = pos + 12;
        pos += 12 + s->size[k];
    }
    s->total = pos;
    return R1CS_OK;
}

// Everything of the key that is no curve point, into out[0 .. s.total): the container's frame, section 1, the integers of
// section 2, section 4 and section 10.  The point fields are left as they are.
inline void setup_write_frame(const R1csFile& f, const SetupShape& s, uint8_t* out)
{
    auto u32 = [&](uint64_t at, uint32_t v) { memcpy(out + at, &v, 4); };
    auto u64 = [&](uint64_t at, uint64_t v) { memcpy(out + at, &v, 8); };
    memcpy(out, "zkey", 4);
    u32(4, 1);
    u32(8, 10);
    for (uint32_t k = 1; k <= 10; k++) {
        u32(s.off[k] - 12, k);
        u64(s.off[k] - 8, s.size[k]);
    }
    u32(s.off[1], 1);
    static const uint64_t Q[4] = {0x3c208c16d87cfd47ull, 0x97816a916871ca8dull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
    uint64_t              h    = s.off[2];
    u32(h, 32);
    memcpy(out + h + 4, Q, 32);
    u32(h + 36, 32);
    memcpy(out + h + 40, R1CS_R, 32);
    u32(h + 72, s.n_wires);
    u32(h + 76, s.n_public);
    u32(h + 80, s.N);
    // section 4
    uint64_t at = s.off[4];
    u32(at, (uint32_t)s.n_records);
    at += 4;
    const R1csScale to_key(512);
    auto            rec = [&](uint32_t m, uint32_t c, uint32_t wire, const R1csFr& v) {
        u32(at, m);
        u32(at + 4, c);
        u32(at + 8, wire);
        memcpy(out + at + 12, v.v, 32);
        at += 44;
    };
    for (uint64_t c = 0; c < s.M; c++)
        for (uint32_t m = 0; m < 2; m++)
            for (uint64_t t = f.row_start[(uint64_t)m * s.M + c]; t < f.row_start[(uint64_t)m * s.M + c + 1]; t++)
                rec(m, (uint32_t)c, f.wire[t], to_key(f.coef[t]));
    const R1csFr one_key = r1cs_fr_pow2(512);
    for (uint32_t i = 0; i <= s.n_public; i++) rec(0, s.M + i, i, one_key);
    memset(out + s.off[10], 0, s.size[10]);
}

// The column plan: cons[e] / coef[e] = constraint (index into L(tau)) and coefficient (standard form) of entry e; padding
// entries are (0, 0).  R1CS_ERR_ARG for 2^32 or more padded entries.
struct SetupColumns {
    SpmvPlan              plan;
    std::vector<uint32_t> cons;
    std::vector<R1csFr>   coef;
};
inline int setup_columns_build(const R1csFile& f, const SetupShape& s, SetupColumns* out)
{
    const uint64_t        nw = s.n_wires, M = s.M;
    std::vector<uint32_t> len(3 * nw, 0);
    for (uint64_t m = 0; m < 3; m++)
        for (uint64_t t = f.row_start[m * M]; t < f.row_start[(m + 1) * M]; t++) {
            if (len[m * nw + f.wire[t]] == 0xffffffffu) return R1CS_ERR_ARG;
            len[m * nw + f.wire[t]]++;
        }
    for (uint32_t i = 0; i <= s.n_public; i++) len[i]++;
    SpmvPlacer pl;
    if (spmv_plan_rows(len, [](size_t i) -> size_t { return i; }, &out->plan, &pl)) return R1CS_ERR_ARG;
    const uint64_t n_entries = std::max<uint64_t>(out->plan.n_entries, 1);
    out->cons.assign(n_entries, 0);
    out->coef.assign(n_entries, R1csFr{{0, 0, 0, 0}});
    std::vector<uint32_t> fill(3 * nw, 0);
    for (uint64_t m = 0; m < 3; m++)
        for (uint64_t c = 0; c < M; c++)
            for (uint64_t t = f.row_start[m * M + c]; t < f.row_start[m * M + c + 1]; t++) {
                const uint32_t row = (uint32_t)(m * nw + f.wire[t]);
                const uint32_t e   = pl.pos(row, fill[row]++);
                out->cons[e]       = (uint32_t)c;
                out->coef[e]       = f.coef[t];
            }
    for (uint32_t i = 0; i <= s.n_public; i++) {
        const uint32_t e = pl.pos(i, fill[i]++);
        out->cons[e]     = s.M + i;
        out->coef[e]     = R1csFr{{1, 0, 0, 0}};
    }
    return R1CS_OK;
}

} // namespace k16
