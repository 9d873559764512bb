// tests/cpp/fullprover_verify_harness.cpp -- the drop-in FullProver with verified proving switched on
// (k16_fullprover_set_verify, include/k16.h), as a program of its own: tests/cpp/fullprover_harness.cpp stands for the Rust
// crate as it is today and stays as it is.
//   harness <zkey> <wtns>      prints state=, verify=<rc of k16_fullprover_set_verify(.., 1)>, then per leg
//                              "file type=<t> error=<e>" + JSON (FullProver::prove) and "mem rc=<rc>" + JSON
//                              (k16_fullprover_prove_mem; rc < 0 on failure)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "k16.h"
#include "k16_fullprover.hpp"

struct Peek {
    void*           impl;
    FullProverState state;
};

// payload of section 2 of an iden3 .wtns file
static bool read_wtns_values(const char* path, std::vector<unsigned char>* out)
{
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    std::vector<unsigned char> all;
    unsigned char              buf[1 << 16];
    size_t                     k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) all.insert(all.end(), buf, buf + k);
    fclose(f);
    if (all.size() < 12 || memcmp(all.data(), "wtns", 4) != 0) return false;
    uint32_t nsec;
    memcpy(&nsec, &all[8], 4);
    size_t pos = 12;
    for (uint32_t i = 0; i < nsec && pos + 12 <= all.size(); i++) {
        uint32_t typ;
        uint64_t size;
        memcpy(&typ, &all[pos], 4);
        memcpy(&size, &all[pos + 4], 8);
        if (pos + 12 + size > all.size()) return false;
        if (typ == 2) {
            out->assign(all.begin() + pos + 12, all.begin() + pos + 12 + size);
            return true;
        }
        pos += 12 + size;
    }
    return false;
}

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    FullProver p(argv[1]);
    Peek       pk;
    static_assert(sizeof(Peek) == sizeof(FullProver), "FullProver layout");
    memcpy(&pk, &p, sizeof pk);
    printf("state=%d\n", (int)pk.state);
    printf("verify=%d\n", k16_fullprover_set_verify(&p, 1));
    {
        ProverResponse r = p.prove(argv[2]);
        printf("file type=%d error=%d\n%s\n", (int)r.type, (int)r.error, r.raw_json);
    }
    std::vector<unsigned char> values;
    if (!read_wtns_values(argv[2], &values)) return 3;
    char      js[4096] = "";
    int       ms = 0;
    const int rc = k16_fullprover_prove_mem(&p, values.data(), values.size() / 32, js, sizeof js, &ms);
    printf("mem rc=%d\n%s\n", rc < 0 ? rc : 0, rc < 0 ? "" : js);
    return 0;
}
