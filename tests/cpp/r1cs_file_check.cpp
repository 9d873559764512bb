// tests/cpp/r1cs_file_check.cpp -- CPU check of keyless-zk-proofs_amd/csrc/r1cs_file.h (the .r1cs reader, the 3 M-row layout
// plan and r1cs_match_zkey), driven by tests/test_r1cs_host.py.  Built with -fsanitize=address,undefined: every input is
// copied into a heap block of exactly its size, so a read past the end is reported.
//   dump FILE        parse; print "rc=<code>" and, when 0, the header, every row and the verdict of the plan check
//   mutate FILE      every truncation length and single-byte corruptions of every byte: each parses (and then plans) or is
//                    refused with a documented code
//   match R1CS ZKEY  print "rc=<code> kind=<k> constraint=<c> wire=<w>"
//   selftest         what needs no file: the 2^32-entry limit of the plan, the field helpers
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "r1cs_file.h"

using namespace k16;

static std::vector<uint8_t> slurp(const char* path)
{
    std::vector<uint8_t> out;
    FILE*                f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(2);
    }
    uint8_t buf[65536];
    size_t  n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
    fclose(f);
    return out;
}
// parse a copy that ends exactly where the input ends
static int parse_exact(const uint8_t* p, size_t n, R1csFile* f)
{
    uint8_t* heap = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(heap, p, n);
    const int rc = r1cs_parse(n ? heap : nullptr, n, f);
    free(heap);
    return rc;
}
static std::string hex(const R1csFr& x)
{
    char b[65];
    snprintf(b, sizeof b, "%016llx%016llx%016llx%016llx", (unsigned long long)x.v[3], (unsigned long long)x.v[2],
             (unsigned long long)x.v[1], (unsigned long long)x.v[0]);
    return b;
}
// what k_r1cs_rows does with the plan: every row is walked once and sees exactly its own terms, in the file's order; every
// other entry of a slice is (wire 0, coefficient 0); every term has an entry of its own.  0 or the number of the failed check.
static int plan_check(const R1csFile& f)
{
    R1csPlan p;
    if (r1cs_plan_build(f, &p)) return 1;
    const SpmvPlan&       pl = p.plan;
    const uint64_t        n  = pl.n_entries;
    std::vector<int64_t>  term_at(n ? n : 1, -1);
    for (uint64_t t = 0; t < f.n_terms(); t++) {
        if (p.pos[t] >= n || term_at[p.pos[t]] >= 0) return 2;
        term_at[p.pos[t]] = (int64_t)t;
    }
    const size_t         n_rows = f.row_start.size() - 1;
    std::vector<uint8_t> seen(n_rows ? n_rows : 1, 0);
    uint32_t             prev = ~0u;
    uint64_t             used = 0;
    for (uint32_t s = 0; s < pl.n_slices; s++) {
        const SpmvSlice sl = pl.slices[s];
        if (sl.len > SPMV_LONG || sl.len > prev) return 3;
        prev = sl.len;
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint32_t row = pl.row_of[64ull * s + lane];
            const uint32_t len = row == 0xffffffffu ? 0 : f.row_len(row);
            if (row != 0xffffffffu && (row >= n_rows || seen[row]++ || len > sl.len)) return 4;
            for (uint32_t k = 0; k < sl.len; k++) {
                const uint64_t e = (uint64_t)sl.off + 64ull * k + lane;
                if (e >= n) return 5;
                used++;
                if (k < len ? term_at[e] != (int64_t)(f.row_start[row] + k) : term_at[e] != -1) return 6;
            }
        }
    }
    for (uint32_t k = 0; k < pl.n_long; k++) {
        const SpmvLong L = pl.longs[k];
        if (L.row >= n_rows || seen[L.row]++ || L.len != f.row_len(L.row) || L.len <= SPMV_LONG) return 7;
        for (uint32_t j = 0; j < L.len; j++, used++)
            if ((uint64_t)L.off + j >= n || term_at[L.off + j] != (int64_t)(f.row_start[L.row] + j)) return 8;
    }
    for (size_t r = 0; r < n_rows; r++)
        if (!seen[r]) return 9;
    if (used != n) return 10; // nothing outside slices and long rows
    return 0;
}
static bool documented(int rc) { return rc == R1CS_OK || rc == R1CS_ERR_FORMAT || rc == R1CS_ERR_CURVE || rc == R1CS_ERR_ARG; }

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "dump" && argc == 3) {
        const std::vector<uint8_t> in = slurp(argv[2]);
        R1csFile                   f;
        const int                  rc = parse_exact(in.data(), in.size(), &f);
        printf("rc=%d\n", rc);
        if (rc) return 0;
        printf("wires=%u pub_out=%u pub_in=%u prv_in=%u labels=%llu constraints=%u public=%u terms=%llu\n", f.n_wires, f.n_pub_out,
               f.n_pub_in, f.n_prv_in, (unsigned long long)f.n_labels, f.n_constraints, f.n_public(), (unsigned long long)f.n_terms());
        const uint64_t M = f.n_constraints;
        for (int m = 0; m < 3; m++)
            for (uint64_t c = 0; c < M; c++) {
                printf("%c %llu :", "ABC"[m], (unsigned long long)c);
                for (uint64_t t = f.row_start[m * M + c]; t < f.row_start[m * M + c + 1]; t++) printf(" %u:%s", f.wire[t], hex(f.coef[t]).c_str());
                printf("\n");
            }
        printf("plan=%d\n", plan_check(f));
        return 0;
    }
    if (mode == "mutate" && argc == 3) {
        const std::vector<uint8_t> in = slurp(argv[2]);
        unsigned long              n_ok = 0, n_refused = 0;
        auto one = [&](const uint8_t* p, size_t n) -> int {
            R1csFile  f;
            const int rc = parse_exact(p, n, &f);
            if (!documented(rc)) return 1;
            if (rc == R1CS_OK) {
                if (plan_check(f)) return 2;
                n_ok++;
            } else {
                n_refused++;
            }
            return 0;
        };
        for (size_t n = 0; n <= in.size(); n++)
            if (int e = one(in.data(), n)) {
                printf("truncation to %zu bytes: failure %d\n", n, e);
                return 1;
            }
        std::vector<uint8_t> m = in;
        const uint8_t        flips[] = {0x01, 0x80, 0xff};
        for (size_t i = 0; i < in.size(); i++)
            for (uint8_t x : flips) {
                m[i] = in[i] ^ x;
                if (int e = one(m.data(), m.size())) {
                    printf("byte %zu ^ %02x: failure %d\n", i, x, e);
                    return 1;
                }
                m[i] = in[i];
            }
        printf("ok parsed=%lu refused=%lu\n", n_ok, n_refused);
        return 0;
    }
    if (mode == "match" && argc == 4) {
        const std::vector<uint8_t> in = slurp(argv[2]), zk = slurp(argv[3]);
        R1csFile                   f;
        if (parse_exact(in.data(), in.size(), &f)) {
            printf("r1cs does not parse\n");
            return 1;
        }
        uint8_t* heap = (uint8_t*)malloc(zk.size() ? zk.size() : 1);
        memcpy(heap, zk.data(), zk.size());
        R1csMismatch mm;
        const int    rc = r1cs_match_zkey(f, heap, zk.size(), &mm);
        free(heap);
        printf("rc=%d kind=%u constraint=%u wire=%u\n", rc, mm.kind, mm.constraint, mm.wire);
        return 0;
    }
    if (mode == "selftest") {
        // padded term count >= 2^32: two rows of 2^31 terms (nothing but the lengths is looked at before the limit)
        R1csFile f;
        f.n_wires = 1;
        f.n_constraints = 1;
        f.row_start = {0, 1ull << 31, 1ull << 32, (1ull << 32) + 5};
        R1csPlan p;
        if (r1cs_plan_build(f, &p) != R1CS_ERR_ARG) {
            printf("plan limit not refused\n");
            return 1;
        }
        f.row_start = {0, (1ull << 32) + 1, (1ull << 32) + 1, (1ull << 32) + 1}; // one row too long for a 32-bit length
        if (r1cs_plan_build(f, &p) != R1CS_ERR_ARG) {
            printf("row length limit not refused\n");
            return 1;
        }
        // field helpers: (r - 1) + (r - 1) = r - 2; x * 2^0 = x; 2^256 * 2^256 / 2^256 = 2^256 mod r; (r - 1) * 2^512 twice = + 2^1024
        R1csFr m1 = {{R1CS_R[0] - 1, R1CS_R[1], R1CS_R[2], R1CS_R[3]}}, m2 = {{R1CS_R[0] - 2, R1CS_R[1], R1CS_R[2], R1CS_R[3]}};
        if (!r1cs_fr_eq(r1cs_fr_add(m1, m1), m2) || !r1cs_fr_geq_r(r1cs_fr_load((const uint8_t*)R1CS_R)) || r1cs_fr_geq_r(m1)) {
            printf("add / compare\n");
            return 1;
        }
        const R1csFr x = {{0x123456789abcdef0ull, 0xfedcba9876543210ull, 0x0f1e2d3c4b5a6978ull, 0x1122334455667788ull}};
        if (!r1cs_fr_eq(R1csScale(0)(x), x) || !r1cs_fr_eq(R1csScale(7)(m1), r1cs_fr_add(R1csFr{{0, 0, 0, 0}}, R1csScale(3)(R1csScale(4)(m1))))) {
            printf("scale\n");
            return 1;
        }
        R1csFr d = x; // x * 2^9 by doubling
        for (int i = 0; i < 9; i++) d = r1cs_fr_add(d, d);
        if (!r1cs_fr_eq(R1csScale(9)(x), d) || !r1cs_fr_eq(R1csScale(512)(R1csFr{{1, 0, 0, 0}}), r1cs_fr_pow2(512))) {
            printf("scale vs doubling\n");
            return 1;
        }
        printf("ok\n");
        return 0;
    }
    fprintf(stderr, "usage: r1cs_file_check dump FILE | mutate FILE | match R1CS ZKEY | selftest\n");
    return 2;
}
