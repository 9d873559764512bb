// tests/cpp/setup_plan_check.cpp -- CPU check of keyless-zk-proofs_amd/csrc/setup_plan.h (the set-up's shape and exact size,
// the transposed column plan, and the writer of everything in the key that is no curve point), driven by
// tests/test_setup_host.py.  Built with -fsanitize=address,undefined; the key is written into a heap block of exactly the
// computed size, so a write past the end is reported.
//   shape FILE        "rc=<code>" and, when 0, "wires= public= M= N= records= total=" and the ten section sizes
//   columns FILE      every row of the column plan as the kernel walks it: "<row> : <constraint>:<coefficient hex> ...", after
//                     "plan=<0 or the number of the failed structural check>"
//   frame FILE OUT    the key with all-zero points, written to OUT
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "setup_plan.h"

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
static std::string hex(const R1csFr& x)
{
    char b[65];
    snprintf(b, sizeof b, "%016llx%016llx%016llx%016llx", (unsigned long long)x.v[3], (unsigned long long)x.v[2],
             (unsigned long long)x.v[1], (unsigned long long)x.v[0]);
    return b;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (argc < 3) return 2;
    const std::vector<uint8_t> in = slurp(argv[2]);
    R1csFile                   f;
    if (r1cs_parse(in.data(), in.size(), &f)) {
        printf("rc=parse\n");
        return 0;
    }
    SetupShape  sh;
    const char* why = "";
    const int   rc  = setup_shape(f, &sh, &why);
    if (mode == "shape") {
        printf("rc=%d\n", rc);
        if (rc) {
            printf("%s\n", why);
            return 0;
        }
        printf("wires=%u public=%u M=%u N=%u records=%llu total=%llu\n", sh.n_wires, sh.n_public, sh.M, sh.N,
               (unsigned long long)sh.n_records, (unsigned long long)sh.total);
        for (int k = 1; k <= 10; k++) printf("%llu%s", (unsigned long long)sh.size[k], k < 10 ? " " : "\n");
        return 0;
    }
    if (rc) return 3;
    if (mode == "columns") {
        SetupColumns cols;
        if (setup_columns_build(f, sh, &cols)) return 4;
        const SpmvPlan& pl     = cols.plan;
        const size_t    n_rows = 3 * (size_t)sh.n_wires;
        const uint64_t  n      = pl.n_entries;
        // the walk of spmv_walk, entry by entry: every entry belongs to exactly one (row, k) or is padding (0, 0)
        std::vector<std::vector<uint64_t>> row_entries(n_rows);
        std::vector<uint8_t>               seen(n_rows, 0), owned(n ? n : 1, 0);
        int                                bad = 0;
        uint32_t                           prev = ~0u;
        for (uint32_t s = 0; s < pl.n_slices && !bad; s++) {
            const SpmvSlice sl = pl.slices[s];
            if (sl.len > SPMV_LONG || sl.len > prev) bad = 1;
            prev = sl.len;
            for (uint32_t lane = 0; lane < 64 && !bad; lane++) {
                const uint32_t row = pl.row_of[64ull * s + lane];
                if (row != 0xffffffffu && (row >= n_rows || seen[row]++)) bad = 2;
                for (uint32_t k = 0; k < sl.len && !bad; k++) {
                    const uint64_t e = (uint64_t)sl.off + 64ull * k + lane;
                    if (e >= n || owned[e]++) bad = 3;
                    else if (row != 0xffffffffu) row_entries[row].push_back(e);
                    else if (cols.cons[e] != 0 || !r1cs_fr_is_zero(cols.coef[e])) bad = 4;
                }
            }
        }
        for (uint32_t k = 0; k < pl.n_long && !bad; k++) {
            const SpmvLong L = pl.longs[k];
            if (L.row >= n_rows || seen[L.row]++ || L.len <= SPMV_LONG) bad = 5;
            for (uint32_t j = 0; j < L.len && !bad; j++) {
                const uint64_t e = (uint64_t)L.off + j;
                if (e >= n || owned[e]++) bad = 6;
                else row_entries[L.row].push_back(e);
            }
        }
        for (size_t r = 0; r < n_rows && !bad; r++)
            if (!seen[r]) bad = 7;
        for (uint64_t e = 0; e < n && !bad; e++)
            if (!owned[e]) bad = 8;
        printf("plan=%d\n", bad);
        if (bad) return 0;
        for (size_t r = 0; r < n_rows; r++) {
            printf("%zu :", r);
            // a padded tail of a slice row is (0, 0): a term with coefficient 0 is printed, padding is told apart by position
            size_t last = row_entries[r].size();
            while (last > 0 && cols.cons[row_entries[r][last - 1]] == 0 && r1cs_fr_is_zero(cols.coef[row_entries[r][last - 1]])) last--;
            for (size_t k = 0; k < last; k++) {
                const uint64_t e = row_entries[r][k];
                printf(" %u:%s", cols.cons[e], hex(cols.coef[e]).c_str());
            }
            printf("\n");
        }
        return 0;
    }
    if (mode == "frame" && argc == 4) {
        uint8_t* key = (uint8_t*)calloc(1, (size_t)sh.total);
        setup_write_frame(f, sh, key);
        FILE* o = fopen(argv[3], "wb");
        if (!o || fwrite(key, 1, (size_t)sh.total, o) != sh.total) return 5;
        fclose(o);
        free(key);
        printf("ok\n");
        return 0;
    }
    return 2;
}
