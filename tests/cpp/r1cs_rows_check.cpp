// r1cs_rows_check.cpp -- stand-alone driver of keyless-zk-proofs_amd/csrc/r1cs_rows.h for tests/test_solve_host.py (built with
// -fsanitize=address,undefined, run as a plain subprocess):
//   r1cs_rows_check FILE.r1cs...   per file: "rc=<status>", then "rows=<3 M> terms=<n>" and one line per row,
//                                  "<matrix> <constraint>" followed by " <wire>:<coefficient>" per term in the row's order -- the
//                                  coefficient as 64 hex digits, resolved through the term's position in the check's coefficient
//                                  array the way the kernel resolves it.  row_start must tile the terms, and no two terms may
//                                  share a position.
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "r1cs_rows.h"

using namespace k16;

static void die(const char* what)
{
    printf("FAIL %s\n", what);
    exit(1);
}

static std::string hex(const R1csFr& x)
{
    char buf[65];
    snprintf(buf, sizeof buf, "%016llx%016llx%016llx%016llx", (unsigned long long)x.v[3], (unsigned long long)x.v[2],
             (unsigned long long)x.v[1], (unsigned long long)x.v[0]);
    return buf;
}

static int one(const char* path)
{
    FILE* fp = fopen(path, "rb");
    if (!fp) die("open");
    std::vector<uint8_t> raw;
    uint8_t              buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof buf, fp)) > 0;) raw.insert(raw.end(), buf, buf + n);
    fclose(fp);
    R1csFile f;
    int      rc = r1cs_parse(raw.data(), raw.size(), &f);
    R1csPlan plan;
    if (!rc) rc = r1cs_plan_build(f, &plan);
    R1csRows V;
    if (!rc) rc = r1cs_rows_build(f, plan, &V);
    printf("rc=%d\n", rc);
    if (rc) return 0;
    // the check's coefficient array, as k16_r1cs_create_mem fills it (unscaled here)
    std::vector<R1csFr> entries(std::max<uint64_t>(plan.plan.n_entries, 1), R1csFr{{0, 0, 0, 0}});
    std::vector<bool>   filled(entries.size(), false), named(entries.size(), false);
    for (uint64_t t = 0; t < f.n_terms(); t++) {
        if (plan.pos[t] >= plan.plan.n_entries || filled[plan.pos[t]]) die("plan position");
        filled[plan.pos[t]]  = true;
        entries[plan.pos[t]] = f.coef[t];
    }
    const size_t n_rows = 3 * (size_t)f.n_constraints;
    if (V.row_start.size() != n_rows + 1 || V.row_start[0] != 0 || V.row_start[n_rows] != V.term.size()) die("row_start");
    if (V.term.size() != f.n_terms()) die("terms");
    printf("rows=%zu terms=%zu\n", n_rows, V.term.size());
    for (size_t id = 0; id < n_rows; id++) {
        if (V.row_start[id + 1] < V.row_start[id]) die("row_start not ascending");
        printf("%zu %zu", f.n_constraints ? id / f.n_constraints : 0, f.n_constraints ? id % f.n_constraints : 0);
        for (uint32_t t = V.row_start[id]; t < V.row_start[id + 1]; t++) {
            const R1csRowRef e = V.term[t];
            if (e.wire >= f.n_wires) die("wire of a term");
            if (e.pos >= plan.plan.n_entries || !filled[e.pos]) die("position names a padding entry");
            if (named[e.pos]) die("two terms share a position");
            named[e.pos] = true;
            printf(" %u:%s", e.wire, hex(entries[e.pos]).c_str());
        }
        printf("\n");
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: r1cs_rows_check FILE.r1cs...\n");
        return 2;
    }
    for (int i = 1; i < argc; i++) one(argv[i]);
    return 0;
}
