// r1cs_held_check.cpp -- stand-alone driver of the marking rows keyless-zk-proofs_amd/csrc/r1cs_bools.h hands out for
// tests/test_determined_bits_host.py (built with -fsanitize=address,undefined, run as a plain subprocess):
//   r1cs_held_check FILE.r1cs...   per file: "rc=<status>", then "rows=<marking rows> n=<boolean wires> wires=<n_wires>" and one
//                                  line "c:x c:x ..." of the marking rows and the wires they mark.  The rows must ascend, name
//                                  constraints and wires of the file, and mark exactly the wires of the mask.
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "r1cs_bools.h"

using namespace k16;

static void die(const char* what)
{
    printf("FAIL %s\n", what);
    exit(1);
}

static int one(const char* path)
{
    FILE* fp = fopen(path, "rb");
    if (!fp) die("open");
    std::vector<uint8_t> raw;
    uint8_t              buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof buf, fp)) > 0;) raw.insert(raw.end(), buf, buf + n);
    fclose(fp);
    R1csFile  f;
    const int rc = r1cs_parse(raw.data(), raw.size(), &f);
    printf("rc=%d\n", rc);
    if (rc) return 0;
    R1csBools B;
    B.row.assign(3, 7); // (a build starts the lists over)
    B.row_wire.assign(5, 7);
    r1cs_bools_build(f, &B);
    if (B.row.size() != B.row_wire.size()) die("two lengths");
    std::vector<uint64_t> seen(B.mark.size(), 0);
    std::string           line;
    for (size_t k = 0; k < B.row.size(); k++) {
        if (k && B.row[k] <= B.row[k - 1]) die("the rows do not ascend");
        if (B.row[k] >= f.n_constraints) die("a row beyond the constraints");
        const uint32_t x = B.row_wire[k];
        if (x == 0 || x >= f.n_wires) die("a marked wire out of range");
        if (!((B.mark[x >> 6] >> (x & 63)) & 1)) die("a row marks a wire the mask does not");
        seen[x >> 6] |= 1ull << (x & 63);
        line += (k ? " " : "") + std::to_string(B.row[k]) + ":" + std::to_string(x);
    }
    if (seen != B.mark) die("a marked wire without a row");
    printf("rows=%zu n=%llu wires=%u\n%s\n", B.row.size(), (unsigned long long)B.n, f.n_wires, line.c_str());
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: r1cs_held_check FILE.r1cs...\n");
        return 2;
    }
    for (int i = 1; i < argc; i++) one(argv[i]);
    return 0;
}
