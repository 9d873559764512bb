// r1cs_bools_check.cpp -- stand-alone driver of keyless-zk-proofs_amd/csrc/r1cs_bools.h for tests/test_solve_bits_host.py (built
// with -fsanitize=address,undefined, run as a plain subprocess):
//   r1cs_bools_check FILE.r1cs...   per file: "rc=<status>", then "n=<boolean wires> wires=<n_wires>" and one line of n_wires
//                                   characters, '1' for a BOOLEAN wire and '0' for any other.  The count must be the mask's.
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
    r1cs_bools_build(f, &B);
    if (B.mark.size() != ((size_t)f.n_wires + 63) / 64) die("mask size");
    uint64_t    n = 0;
    std::string line;
    for (uint32_t i = 0; i < f.n_wires; i++) {
        const bool on = (B.mark[i >> 6] >> (i & 63)) & 1;
        n += on;
        line += on ? '1' : '0';
    }
    for (size_t i = f.n_wires; i < 64 * B.mark.size(); i++)
        if ((B.mark[i >> 6] >> (i & 63)) & 1) die("a bit beyond n_wires");
    if (n != B.n) die("count");
    if (f.n_wires && (B.mark[0] & 1)) die("wire 0 is marked");
    printf("n=%llu wires=%u\n%s\n", (unsigned long long)B.n, f.n_wires, line.c_str());
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: r1cs_bools_check FILE.r1cs...\n");
        return 2;
    }
    for (int i = 1; i < argc; i++) one(argv[i]);
    return 0;
}
