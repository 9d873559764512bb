// r1cs_file.h -- host side of the R1CS witness check (r1cs_check.hip): the iden3 `r1cs` container, the layout of its
// 3 M rows A | B | C for the row kernel, and the comparison of a circuit with a Groth16 zkey.  Pure C++ (no HIP): compiled
// into libk16.so and, on its own, into tests/cpp/r1cs_file_check.cpp.
//
// Container (the zkey's: binfile_utils.cpp:13-58): magic "r1cs", u32 version = 1, u32 nSections, then per section
// { u32 type, u64 size, payload } in any order; the first occurrence of a type wins.
//   section 1 (header)       u32 fieldSize, prime (fieldSize bytes LE), u32 nWires, u32 nPubOut, u32 nPubIn, u32 nPrvIn,
//                            u64 nLabels, u32 mConstraints
//   section 2 (constraints)  per constraint three linear combinations A, B, C, each u32 n and n x { u32 wire, 32-byte
//                            coefficient }, little-endian STANDARD form (not Montgomery)
//   section 3 (wire -> label) and every other section are ignored.
// Constraint c holds for an assignment w when <A_c, w> * <B_c, w> = <C_c, w> mod r.  A wire may be listed more than once in
// a combination: its coefficients add.  nPublic = nPubOut + nPubIn.
// The test fixtures hold no .r1cs file written by circom: the files this reader is tested with come from
// tests/r1cs_builder.py, written from the format description above; the one pin that is not of our
// own making is r1cs_match_zkey against the reference-made tests/golden/toy/toy_1.zkey.
//
// Errors are the library's status codes (include/k16.h; r1cs_check.hip asserts the values):
//   R1CS_ERR_FORMAT  truncation, a section shorter than its counts imply, a count that runs past the section, a wire >=
//                    nWires, a coefficient >= r, bytes left over in section 2, a header with nWires = 0 or with
//                    nPubOut + nPubIn >= nWires (wire 0 is the constant: it is never a public wire)
//   R1CS_ERR_CURVE   fieldSize != 32 or prime != BN254 r
//   R1CS_ERR_ARG     3 * mConstraints >= 2^32, or (r1cs_plan_build) 2^32 or more entries with padding
// Nothing here reads outside [base, base + size).
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "spmv_plan.h"

namespace k16 {

enum { R1CS_OK = 0, R1CS_ERR_ARG = -3, R1CS_ERR_FORMAT = -5, R1CS_ERR_CURVE = -6 };

// ---------------------------------------------------------------- 256-bit integers mod r (four 64-bit words, little-endian)
struct R1csFr {
    uint64_t v[4];
};
static const uint64_t R1CS_R[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};

inline R1csFr r1cs_fr_load(const uint8_t* p)
{
    R1csFr x;
    memcpy(x.v, p, 32);
    return x;
}
inline bool r1cs_fr_geq_r(const R1csFr& x)
{
    for (int i = 3; i >= 0; i--)
        if (x.v[i] != R1CS_R[i]) return x.v[i] > R1CS_R[i];
    return true;
}
inline bool r1cs_fr_is_zero(const R1csFr& x) { return (x.v[0] | x.v[1] | x.v[2] | x.v[3]) == 0; }
inline bool r1cs_fr_eq(const R1csFr& a, const R1csFr& b) { return memcmp(a.v, b.v, 32) == 0; }
// a + b mod r for a, b < r
inline R1csFr r1cs_fr_add(const R1csFr& a, const R1csFr& b)
{
    R1csFr            s;
    unsigned __int128 c = 0;
    for (int i = 0; i < 4; i++) {
        c += (unsigned __int128)a.v[i] + b.v[i];
        s.v[i] = (uint64_t)c;
        c >>= 64;
    }
    if (c || r1cs_fr_geq_r(s)) { // (a + b < 2r < 2^255: no carry out in fact)
        unsigned __int128 br = 0;
        for (int i = 0; i < 4; i++) {
            const unsigned __int128 d = (unsigned __int128)s.v[i] - R1CS_R[i] - (uint64_t)br;
            s.v[i]                    = (uint64_t)d;
            br                        = (d >> 64) & 1;
        }
    }
    return s;
}
// a * b / 2^256 mod r (Montgomery product, CIOS) for a, b < r
inline R1csFr r1cs_fr_mont_mul(const R1csFr& a, const R1csFr& b)
{
    uint64_t n0 = 1; // -r^-1 mod 2^64 by Newton's iteration
    for (int i = 0; i < 6; i++) n0 *= 2 - R1CS_R[0] * n0;
    n0 = 0 - n0;
    uint64_t t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
        unsigned __int128 c = 0;
        for (int j = 0; j < 4; j++) {
            c += (unsigned __int128)a.v[j] * b.v[i] + t[j];
            t[j] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[4] = (uint64_t)c;
        t[5] = (uint64_t)(c >> 64);
        const uint64_t m = t[0] * n0;
        c                = ((unsigned __int128)m * R1CS_R[0] + t[0]) >> 64;
        for (int j = 1; j < 4; j++) {
            c += (unsigned __int128)m * R1CS_R[j] + t[j];
            t[j - 1] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[3] = (uint64_t)c;
        t[4] = t[5] + (uint64_t)(c >> 64);
    }
    R1csFr r = {{t[0], t[1], t[2], t[3]}};
    if (t[4] || r1cs_fr_geq_r(r)) {
        unsigned __int128 br = 0;
        for (int i = 0; i < 4; i++) {
            const unsigned __int128 d = (unsigned __int128)r.v[i] - R1CS_R[i] - (uint64_t)br;
            r.v[i]                    = (uint64_t)d;
            br                        = (d >> 64) & 1;
        }
    }
    return r;
}
// 2^k mod r
inline R1csFr r1cs_fr_pow2(unsigned k)
{
    R1csFr x = {{1, 0, 0, 0}};
    for (unsigned i = 0; i < k; i++) x = r1cs_fr_add(x, x);
    return x;
}
// x -> x * 2^k mod r: one Montgomery product with 2^(k + 256)
struct R1csScale {
    R1csFr f;
    explicit R1csScale(unsigned k) : f(r1cs_fr_pow2(k + 256)) {}
    R1csFr operator()(const R1csFr& x) const { return r1cs_fr_mont_mul(x, f); }
};

// ---------------------------------------------------------------- the container
struct R1csSection {
    const uint8_t* p    = nullptr;
    uint64_t       size = 0;
};
// sections 0..15 of an iden3 binfile; R1CS_ERR_FORMAT for a wrong magic / version or a section that leaves the file
inline int r1cs_binfile_sections(const uint8_t* base, size_t size, const char* magic, R1csSection sec[16])
{
    if (!base || size < 12 || memcmp(base, magic, 4) != 0) return R1CS_ERR_FORMAT;
    uint32_t version, nsec;
    memcpy(&version, base + 4, 4);
    memcpy(&nsec, base + 8, 4);
    if (version != 1) return R1CS_ERR_FORMAT;
    size_t pos = 12;
    for (uint32_t i = 0; i < nsec; i++) {
        if (size - pos < 12) return R1CS_ERR_FORMAT;
        uint32_t st;
        uint64_t ss;
        memcpy(&st, base + pos, 4);
        memcpy(&ss, base + pos + 4, 8);
        pos += 12;
        if (ss > size - pos) return R1CS_ERR_FORMAT;
        if (st < 16 && sec[st].p == nullptr) {
            sec[st].p    = base + pos;
            sec[st].size = ss;
        }
        pos += (size_t)ss;
    }
    return R1CS_OK;
}

// A parsed circuit: the terms of row id = matrix * M + constraint (matrix 0 = A, 1 = B, 2 = C) are
// [row_start[id], row_start[id + 1]) of wire / coef, in the file's order.
struct R1csFile {
    uint32_t              n_wires = 0, n_pub_out = 0, n_pub_in = 0, n_prv_in = 0, n_constraints = 0;
    uint64_t              n_labels = 0;
    std::vector<uint64_t> row_start; // [3 M + 1]
    std::vector<uint32_t> wire;
    std::vector<R1csFr>   coef;      // standard form, < r
    uint32_t n_public() const { return n_pub_out + n_pub_in; }
    uint64_t n_terms() const { return wire.size(); }
    uint32_t row_len(size_t id) const { return (uint32_t)(row_start[id + 1] - row_start[id]); }
};

inline int r1cs_parse(const uint8_t* base, size_t size, R1csFile* out, const char** why = nullptr)
{
    const char* dummy;
    if (!why) why = &dummy;
    *why = "";
    R1csSection sec[16];
    if (r1cs_binfile_sections(base, size, "r1cs", sec)) {
        *why = "r1cs: not an iden3 r1cs container (magic / version / sections)";
        return R1CS_ERR_FORMAT;
    }
    if (!sec[1].p || !sec[2].p) {
        *why = "r1cs: header or constraint section missing";
        return R1CS_ERR_FORMAT;
    }
    const uint8_t* h = sec[1].p;
    uint32_t       fs;
    if (sec[1].size < 4) {
        *why = "r1cs: header section too short";
        return R1CS_ERR_FORMAT;
    }
    memcpy(&fs, h, 4);
    if (fs != 32) {
        *why = "r1cs: field size is not 32 bytes";
        return R1CS_ERR_CURVE;
    }
    if (sec[1].size < 4 + 32 + 4 * 4 + 8 + 4) {
        *why = "r1cs: header section too short";
        return R1CS_ERR_FORMAT;
    }
    if (memcmp(h + 4, R1CS_R, 32) != 0) { // (x86 / gfx host: little-endian words = the file's bytes)
        *why = "r1cs: prime is not BN254 r";
        return R1CS_ERR_CURVE;
    }
    memcpy(&out->n_wires, h + 36, 4);
    memcpy(&out->n_pub_out, h + 40, 4);
    memcpy(&out->n_pub_in, h + 44, 4);
    memcpy(&out->n_prv_in, h + 48, 4);
    memcpy(&out->n_labels, h + 52, 8);
    memcpy(&out->n_constraints, h + 60, 4);
    const uint64_t M = out->n_constraints;
    if (3 * M >= (1ull << 32)) {
        *why = "r1cs: too many constraints for 32-bit row numbers";
        return R1CS_ERR_ARG;
    }
    if (out->n_wires == 0 || (uint64_t)out->n_pub_out + out->n_pub_in >= out->n_wires) {
        *why = "r1cs: bad header sizes";
        return R1CS_ERR_FORMAT;
    }
    const uint8_t* p   = sec[2].p;
    const uint64_t len = sec[2].size;
    if (M > len / 12) { // three counts per constraint at the least: nothing below is sized by an unchecked M
        *why = "r1cs: constraint section shorter than the header implies";
        return R1CS_ERR_FORMAT;
    }
    // pass 1: bounds, wires, coefficients, row lengths
    out->row_start.assign(3 * M + 1, 0);
    uint64_t pos = 0, total = 0;
    for (uint64_t c = 0; c < M; c++) {
        for (int m = 0; m < 3; m++) {
            if (len - pos < 4) {
                *why = "r1cs: constraint section truncated";
                return R1CS_ERR_FORMAT;
            }
            uint32_t n;
            memcpy(&n, p + pos, 4);
            pos += 4;
            if ((uint64_t)n > (len - pos) / 36) {
                *why = "r1cs: a term count runs past the constraint section";
                return R1CS_ERR_FORMAT;
            }
            for (uint32_t k = 0; k < n; k++, pos += 36) {
                uint32_t w;
                memcpy(&w, p + pos, 4);
                if (w >= out->n_wires) {
                    *why = "r1cs: wire number out of range";
                    return R1CS_ERR_FORMAT;
                }
                if (r1cs_fr_geq_r(r1cs_fr_load(p + pos + 4))) {
                    *why = "r1cs: coefficient not below r";
                    return R1CS_ERR_FORMAT;
                }
            }
            out->row_start[(uint64_t)m * M + c + 1] = n;
            total += n;
        }
    }
    if (pos != len) {
        *why = "r1cs: bytes left over behind the last constraint";
        return R1CS_ERR_FORMAT;
    }
    for (uint64_t i = 0; i < 3 * M; i++) out->row_start[i + 1] += out->row_start[i];
    out->wire.assign(total, 0);
    out->coef.assign(total, R1csFr{{0, 0, 0, 0}});
    // pass 2: the terms, row by row
    pos = 0;
    for (uint64_t c = 0; c < M; c++) {
        for (int m = 0; m < 3; m++) {
            uint32_t n;
            memcpy(&n, p + pos, 4);
            pos += 4;
            uint64_t at = out->row_start[(uint64_t)m * M + c];
            for (uint32_t k = 0; k < n; k++, pos += 36, at++) {
                memcpy(&out->wire[at], p + pos, 4);
                out->coef[at] = r1cs_fr_load(p + pos + 4);
            }
        }
    }
    return R1CS_OK;
}

// ---------------------------------------------------------------- layout for the row kernel
// The 3 M rows through spmv_plan.h's core: rows of <= SPMV_LONG terms in length-sorted slices, longer rows a wave each, no
// bit-reversed placement -- row id lands at index id of the output.  pos[t] = entry of term t (the order of R1csFile's
// arrays); every other entry of a slice is padding (wire 0, coefficient 0).
struct R1csPlan {
    SpmvPlan              plan;
    std::vector<uint32_t> pos; // [n_terms]
};
inline int r1cs_plan_build(const R1csFile& f, R1csPlan* out)
{
    const size_t          n_rows = f.row_start.size() - 1;
    std::vector<uint32_t> len(n_rows);
    for (size_t r = 0; r < n_rows; r++) {
        if (f.row_start[r + 1] - f.row_start[r] >= (1ull << 32)) return R1CS_ERR_ARG;
        len[r] = f.row_len(r);
    }
    SpmvPlacer pl;
    if (spmv_plan_rows(len, [](size_t i) -> size_t { return i; }, &out->plan, &pl)) return R1CS_ERR_ARG;
    out->pos.assign(f.n_terms(), 0);
    for (size_t r = 0; r < n_rows; r++)
        for (uint32_t k = 0; k < len[r]; k++) out->pos[f.row_start[r] + k] = pl.pos((uint32_t)r, k);
    return R1CS_OK;
}

// ---------------------------------------------------------------- circuit <-> proving key
// Section 4 of a snarkjs Groth16 zkey is derived from the circuit: for every constraint c and every term of A (matrix 0) or
// B (1) a record { u32 m, u32 c, u32 wire, coef * 2^512 mod r }, plus, for s = 0 .. nPublic, { 0, M + s, s, 2^512 mod r }.
// Both sides are compared as multisets per (matrix, constraint) after the coefficients of a wire listed twice have been
// added (a sum of zero counts as no term).  Also: nVars == nWires, equal nPublic, domain a power of two >= M + nPublic + 1.
enum { R1CS_MATCH = 0, R1CS_DIFF_HEADER = 1, R1CS_DIFF_A = 2, R1CS_DIFF_B = 3, R1CS_DIFF_PUBLIC = 4 };
struct R1csMismatch {
    uint32_t kind = R1CS_MATCH, constraint = 0, wire = 0; // the first difference, in the order header, A, B, public rows
};
struct R1csRowTerm {
    uint32_t wire;
    R1csFr   coef;
    bool     canonical = true; // coef < r; a zkey's record may not be: it then equals no coefficient of a circuit
};
// sorts by wire, adds the coefficients of equal wires, drops sums of zero
inline void r1cs_row_canonical(std::vector<R1csRowTerm>& row)
{
    std::stable_sort(row.begin(), row.end(), [](const R1csRowTerm& a, const R1csRowTerm& b) { return a.wire < b.wire; });
    size_t n = 0;
    for (size_t i = 0; i < row.size();) {
        R1csRowTerm t = row[i++];
        while (i < row.size() && row[i].wire == t.wire) t.coef = r1cs_fr_add(t.coef, row[i++].coef);
        if (!r1cs_fr_is_zero(t.coef)) row[n++] = t;
    }
    row.resize(n);
}
// Returns R1CS_OK with *out filled, or R1CS_ERR_FORMAT / R1CS_ERR_CURVE for a zkey that cannot be read.
inline int r1cs_match_zkey(const R1csFile& f, const uint8_t* zkey, size_t size, R1csMismatch* out, const char** why = nullptr)
{
    const char* dummy;
    if (!why) why = &dummy;
    *why = "";
    *out = R1csMismatch();
    R1csSection sec[16];
    if (r1cs_binfile_sections(zkey, size, "zkey", sec) || !sec[2].p || !sec[4].p) {
        *why = "zkey: not an iden3 zkey container with sections 2 and 4";
        return R1CS_ERR_FORMAT;
    }
    const uint8_t* h = sec[2].p;
    uint32_t       n8;
    if (sec[2].size < 4) return R1CS_ERR_FORMAT;
    memcpy(&n8, h, 4);
    if (n8 != 32) return R1CS_ERR_CURVE;
    if (sec[2].size < 4 + 32 + 4 + 32 + 12) return R1CS_ERR_FORMAT;
    memcpy(&n8, h + 36, 4);
    if (n8 != 32 || memcmp(h + 40, R1CS_R, 32) != 0) {
        *why = "zkey curve not supported";
        return R1CS_ERR_CURVE;
    }
    uint32_t n_vars, n_public, domain;
    memcpy(&n_vars, h + 72, 4);
    memcpy(&n_public, h + 76, 4);
    memcpy(&domain, h + 80, 4);
    if (sec[4].size < 4) return R1CS_ERR_FORMAT;
    uint32_t n_rec;
    memcpy(&n_rec, sec[4].p, 4);
    if ((uint64_t)n_rec > (sec[4].size - 4) / 44) {
        *why = "zkey: section 4 shorter than its count implies";
        return R1CS_ERR_FORMAT;
    }
    const uint8_t* cf = sec[4].p + 4;
    const uint64_t M = f.n_constraints, need = M + f.n_public() + 1;
    if (n_vars != f.n_wires || n_public != f.n_public() || domain == 0 || (domain & (domain - 1)) || domain < need) {
        out->kind = R1CS_DIFF_HEADER;
        *why      = "the zkey's nVars / nPublic / domain are not this circuit's";
        return R1CS_OK;
    }
    // the zkey's records by row: id = m * need + c; a record outside these rows is a difference of its own
    std::vector<uint64_t> start(2 * need + 1, 0);
    for (uint32_t i = 0; i < n_rec; i++) {
        uint32_t m, c, s;
        memcpy(&m, cf + (size_t)i * 44, 4);
        memcpy(&c, cf + (size_t)i * 44 + 4, 4);
        memcpy(&s, cf + (size_t)i * 44 + 8, 4);
        if (m > 1 || c >= need || (m == 1 && c >= M)) {
            out->kind       = m == 0 ? R1CS_DIFF_PUBLIC : R1CS_DIFF_B;
            out->constraint = c;
            out->wire       = s;
            *why            = "the zkey has a coefficient outside the circuit's rows";
            return R1CS_OK;
        }
        start[(uint64_t)m * need + c + 1]++;
    }
    for (uint64_t i = 0; i < 2 * need; i++) start[i + 1] += start[i];
    std::vector<uint32_t> order(n_rec ? n_rec : 1);
    {
        std::vector<uint64_t> cur(start.begin(), start.end() - 1);
        for (uint32_t i = 0; i < n_rec; i++) {
            uint32_t m, c;
            memcpy(&m, cf + (size_t)i * 44, 4);
            memcpy(&c, cf + (size_t)i * 44 + 4, 4);
            order[cur[(uint64_t)m * need + c]++] = i;
        }
    }
    const R1csScale          to_key(512);
    std::vector<R1csRowTerm> want, got;
    auto zkey_row = [&](uint64_t id) {
        got.clear();
        for (uint64_t k = start[id]; k < start[id + 1]; k++) {
            const uint8_t* rec = cf + (size_t)order[k] * 44;
            R1csRowTerm    t;
            memcpy(&t.wire, rec + 8, 4);
            t.coef      = r1cs_fr_load(rec + 12);
            t.canonical = !r1cs_fr_geq_r(t.coef);
            if (t.canonical && r1cs_fr_is_zero(t.coef)) continue;
            got.push_back(t);
        }
        bool canon = true;
        for (const auto& t : got) canon = canon && t.canonical;
        if (canon) r1cs_row_canonical(got); // (a row with a value >= r is not summed: it differs whatever the sum)
        else std::stable_sort(got.begin(), got.end(), [](const R1csRowTerm& a, const R1csRowTerm& b) { return a.wire < b.wire; });
    };
    auto differ = [&](uint32_t kind, uint64_t c) -> bool {
        const size_t n = std::min(want.size(), got.size());
        for (size_t i = 0; i < n; i++) {
            if (want[i].wire != got[i].wire || !got[i].canonical || !r1cs_fr_eq(want[i].coef, got[i].coef)) {
                out->kind       = kind;
                out->constraint = (uint32_t)c;
                out->wire       = std::min(want[i].wire, got[i].wire);
                return true;
            }
        }
        if (want.size() != got.size()) {
            out->kind       = kind;
            out->constraint = (uint32_t)c;
            out->wire       = want.size() > n ? want[n].wire : got[n].wire;
            return true;
        }
        return false;
    };
    for (int m = 0; m < 2; m++) {
        for (uint64_t c = 0; c < M; c++) {
            want.clear();
            for (uint64_t t = f.row_start[m * M + c]; t < f.row_start[m * M + c + 1]; t++) want.push_back({f.wire[t], f.coef[t]});
            r1cs_row_canonical(want);
            for (auto& t : want) t.coef = to_key(t.coef);
            zkey_row((uint64_t)m * need + c);
            if (differ(m == 0 ? R1CS_DIFF_A : R1CS_DIFF_B, c)) {
                *why = m == 0 ? "matrix A of the zkey differs from the circuit's" : "matrix B of the zkey differs from the circuit's";
                return R1CS_OK;
            }
        }
    }
    const R1csFr one_key = r1cs_fr_pow2(512);
    for (uint64_t s = 0; s <= f.n_public(); s++) {
        want.assign(1, R1csRowTerm{(uint32_t)s, one_key});
        zkey_row(M + s);
        if (differ(R1CS_DIFF_PUBLIC, M + s)) {
            *why = "the zkey's public-input rows are not those snarkjs appends for this circuit";
            return R1CS_OK;
        }
    }
    return R1CS_OK;
}

} // namespace k16
