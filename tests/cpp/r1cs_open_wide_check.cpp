// r1cs_open_wide_check.cpp -- stand-alone driver of keyless-zk-proofs_amd/csrc/r1cs_open.h with a cap, for
// tests/test_open_wide_host.py (built with -fsanitize=address,undefined, run as a plain subprocess):
//   r1cs_open_wide_check FILE.r1cs FIXED BROKEN CAP [WIRE]
// FIXED / BROKEN: comma-separated wires held fixed / constraints the check found broken, "-" for none; CAP: max_wires, 64 .. 256.
// Without WIRE the whole work list (r1cs_open_build), with it the component of that wire alone (r1cs_open_one).  Output:
//   "kinds <one digit per constraint>"            (r1cs_open_build only)
//   "counts components=<n> skipped=<n> absent=<n> classes=<n16>,<n32>,<n64>,<n128>,<n256>"
//   "cls <one digit per wire>"   "comp <id or - per wire>"
//   per eliminated component, in the work list's order: "component <id> cross=<n> wires=<w>,<w>,..." and per LINEAR row
//   "row <constraint> <column>:<wire> ..."
//   r1cs_open_one adds "one class=<c> wires=<n> rows=<n> cross=<n>"
// Every entry is checked against the incidence list, every component against its size class and the cap.  That CAP 64 gives
// the work list of the builder as it was before it took a cap is the test's to check: it compares this output with dumps of
// that builder under tests/golden/open_wide/.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "r1cs_open.h"

using namespace k16;

static void die(const char* what)
{
    printf("FAIL %s\n", what);
    exit(1);
}

static std::vector<uint32_t> numbers(const char* s)
{
    std::vector<uint32_t> out;
    if (!strcmp(s, "-")) return out;
    for (const char* p = s; *p;) {
        char* end;
        out.push_back((uint32_t)strtoul(p, &end, 10));
        if (end == p) die("number list");
        p = *end == ',' ? end + 1 : end;
    }
    return out;
}

static void print_work(const R1csPairs& P, const R1csOpenWork& W, uint32_t n_wires, uint32_t cap)
{
    const uint32_t skip = P.start[1];
    printf("counts components=%llu skipped=%llu absent=%llu classes=%u,%u,%u,%u,%u\n", (unsigned long long)W.n_components,
           (unsigned long long)W.n_skipped, (unsigned long long)W.n_absent, W.n_class[0], W.n_class[1], W.n_class[2], W.n_class[3], W.n_class[4]);
    if (W.cls.size() == n_wires) {
        printf("cls ");
        for (uint32_t i = 0; i < n_wires; i++) printf("%u", W.cls[i]);
        printf("\ncomp");
        for (uint32_t i = 0; i < n_wires; i++) W.comp[i] == R1CS_OPEN_NONE ? printf(" -") : printf(" %u", W.comp[i]);
        printf("\n");
    }
    size_t total = 0;
    for (uint32_t k = 0; k < R1CS_OPEN_CLASSES; k++) total += W.n_class[k];
    if (total != W.comps.size()) die("classes do not tile the components");
    if (W.row_start.size() != W.row.size() + 1 && !(W.comps.empty() && W.row_start.empty())) die("row_start");
    size_t at = 0;
    for (uint32_t k = 0; k < R1CS_OPEN_CLASSES; k++)
        for (uint32_t j = 0; j < W.n_class[k]; j++, at++) {
            const R1csOpenComp& c = W.comps[at];
            if (c.n_wires > cap || c.n_wires > r1cs_open_class_wires(k) || (k && c.n_wires <= r1cs_open_class_wires(k - 1))) die("size class");
            if ((size_t)c.wire0 + c.n_wires > W.wires.size() || (size_t)c.row0 + c.n_rows > W.row.size()) die("component range");
            if (!c.n_wires || W.wires[c.wire0] != c.id) die("component id");
            printf("component %u cross=%u wires=", c.id, c.n_cross);
            for (uint32_t i = 0; i < c.n_wires; i++) {
                if (i && W.wires[c.wire0 + i] <= W.wires[c.wire0 + i - 1]) die("wires not ascending");
                printf(i ? ",%u" : "%u", W.wires[c.wire0 + i]);
            }
            printf("\n");
            for (uint32_t r = c.row0; r < c.row0 + c.n_rows; r++) {
                if (W.row_start[r + 1] < W.row_start[r] || W.row_start[r + 1] > W.ent.size()) die("row range");
                if (W.row_start[r + 1] - W.row_start[r] > c.n_wires) die("a row with more entries than the component has columns");
                if (r > c.row0 && W.row[r] <= W.row[r - 1]) die("rows not ascending");
                printf("row %u", W.row[r]);
                for (uint32_t e = W.row_start[r]; e < W.row_start[r + 1]; e++) {
                    const R1csOpenEntry& en = W.ent[e];
                    if (en.column >= c.n_wires) die("column");
                    if (e > W.row_start[r] && en.column <= W.ent[e - 1].column) die("columns not ascending");
                    const size_t i = (size_t)en.inc + skip;
                    if (i >= P.pair.size() || P.wire[i] != W.wires[c.wire0 + en.column] || P.pair[i].constraint != W.row[r]) die("incidence");
                    printf(" %u:%u", en.column, P.wire[i]);
                }
                printf("\n");
            }
        }
}

int main(int argc, char** argv)
{
    if (argc < 5) {
        fprintf(stderr, "usage: r1cs_open_wide_check FILE.r1cs FIXED BROKEN CAP [WIRE]\n");
        return 2;
    }
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) die("open");
    std::vector<uint8_t> raw;
    uint8_t              buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof buf, fp)) > 0;) raw.insert(raw.end(), buf, buf + n);
    fclose(fp);
    R1csFile f;
    R1csPlan plan;
    R1csPairs P;
    if (r1cs_parse(raw.data(), raw.size(), &f) || r1cs_plan_build(f, &plan) || r1cs_pairs_build(f, plan, &P)) die("parse");
    const uint32_t n_wires = (uint32_t)f.n_wires, M = (uint32_t)f.n_constraints;
    std::vector<uint8_t>  fixed(n_wires, 0);
    std::vector<uint64_t> verdict(((size_t)M + 63) / 64 + 1, 0);
    for (uint32_t w : numbers(argv[2])) {
        if (w >= n_wires) die("fixed wire");
        fixed[w] = 1;
    }
    for (uint32_t c : numbers(argv[3])) {
        if (c >= M) die("broken constraint");
        verdict[c >> 6] |= 1ull << (c & 63);
    }
    const uint32_t cap = (uint32_t)strtoul(argv[4], nullptr, 10);
    if (cap < R1CS_OPEN_MAX_WIRES || cap > R1CS_OPEN_MAX_WIRES_EX) die("cap");
    R1csOpenIndex X;
    r1cs_open_index(P, M, &X);
    R1csOpenWork W;
    if (argc == 5) {
        r1cs_open_build(P, X, n_wires, M, fixed.data(), verdict.data(), &W, cap);
        printf("kinds ");
        for (uint32_t c = 0; c < M; c++) printf("%u", W.kind[c]);
        printf("\n");
        print_work(P, W, n_wires, cap);
    } else {
        const uint32_t wire = (uint32_t)strtoul(argv[5], nullptr, 10);
        if (wire >= n_wires) die("wire");
        uint32_t      nw, nr, nx;
        const uint8_t cls = r1cs_open_one(P, X, n_wires, M, fixed.data(), verdict.data(), wire, &W, &nw, &nr, &nx, cap);
        printf("one class=%u wires=%u rows=%u cross=%u\n", cls, nw, nr, nx);
        print_work(P, W, n_wires, cap);
    }
    return 0;
}
