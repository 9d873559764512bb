// r1cs_pairs_check.cpp -- stand-alone driver of keyless-zk-proofs_amd/csrc/r1cs_pairs.h for tests/test_unbound_host.py (built
// with -fsanitize=address,undefined, run as a plain subprocess):
//   r1cs_pairs_check FILE.r1cs...   per file: "rc=<status>", then "pairs=<n> side=<k> wires=<n_wires>", one line
//                                   "<wire> <constraint> <A^> <B^> <C^>" per incidence in the list's order -- the merged
//                                   coefficients as 64 hex digits, resolved through the positions the way the kernel resolves
//                                   them (an entry of the check's coefficient array, the side table, or zero) -- and
//                                   "present=<wires with a column>".  The columns (start[]) must tile the list.
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "r1cs_pairs.h"

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
    R1csPairs P;
    if (!rc) rc = r1cs_pairs_build(f, plan, &P);
    printf("rc=%d\n", rc);
    if (rc) return 0;
    // the check's coefficient array, as k16_r1cs_create_mem fills it (unscaled here)
    std::vector<R1csFr> entries(std::max<uint64_t>(plan.plan.n_entries, 1), R1csFr{{0, 0, 0, 0}});
    std::vector<bool>   used(entries.size(), false);
    for (uint64_t t = 0; t < f.n_terms(); t++) {
        if (plan.pos[t] >= plan.plan.n_entries || used[plan.pos[t]]) die("plan position");
        used[plan.pos[t]]    = true;
        entries[plan.pos[t]] = f.coef[t];
    }
    if (P.n_entries != plan.plan.n_entries) die("n_entries");
    auto at = [&](uint32_t p) -> R1csFr {
        if (p == R1CS_PAIR_NONE) return R1csFr{{0, 0, 0, 0}};
        if (p < P.n_entries) {
            if (!used[p]) die("position names a padding entry");
            return entries[p];
        }
        if (p - P.n_entries >= P.side.size()) die("position beyond the side table");
        return P.side[p - P.n_entries];
    };
    if (P.start.size() != (size_t)f.n_wires + 1 || P.start[0] != 0 || P.start[f.n_wires] != P.n_pairs()) die("start");
    if (P.wire.size() != P.pair.size() || P.present.size() != ((size_t)f.n_wires + 63) / 64) die("sizes");
    printf("pairs=%llu side=%zu wires=%u\n", (unsigned long long)P.n_pairs(), P.side.size(), f.n_wires);
    for (uint32_t w = 0; w < f.n_wires; w++) {
        if (P.start[w + 1] < P.start[w]) die("start not ascending");
        for (uint32_t k = P.start[w]; k < P.start[w + 1]; k++) {
            if (P.wire[k] != w) die("wire of an incidence");
            if (P.pair[k].constraint >= f.n_constraints) die("constraint of an incidence");
            if (k > P.start[w] && P.pair[k].constraint <= P.pair[k - 1].constraint) die("constraints of a wire not ascending");
            printf("%u %u %s %s %s\n", w, P.pair[k].constraint, hex(at(P.pair[k].a)).c_str(), hex(at(P.pair[k].b)).c_str(),
                   hex(at(P.pair[k].c)).c_str());
        }
    }
    for (const R1csFr& s : P.side)
        if (r1cs_fr_is_zero(s) || r1cs_fr_geq_r(s)) die("side table value");
    printf("present=");
    for (uint32_t w = 0; w < f.n_wires; w++)
        if ((P.present[w >> 6] >> (w & 63)) & 1) printf(" %u", w);
    printf("\n");
    for (size_t i = f.n_wires; i < P.present.size() * 64; i++)
        if ((P.present[i >> 6] >> (i & 63)) & 1) die("present bit beyond the wires");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: r1cs_pairs_check FILE.r1cs...\n");
        return 2;
    }
    for (int i = 1; i < argc; i++) one(argv[i]);
    return 0;
}
