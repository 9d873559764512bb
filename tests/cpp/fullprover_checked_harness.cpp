// tests/cpp/fullprover_checked_harness.cpp -- the drop-in FullProver with checked proving switched on
// (k16_fullprover_set_r1cs / k16_fullprover_last_rejection, include/k16.h), as a program of its own.
//   harness <zkey> <r1cs> <w0.wtns,w1.wtns,...> <verify 0|1> <reps>
// prints state=, r1cs=<rc of k16_fullprover_set_r1cs>, with verify = 1 also verify=<rc of k16_fullprover_set_verify(.., 1)>;
// then one thread per witness proves it <reps> times through k16_fullprover_prove_mem and through FullProver::prove, all
// threads at once, and after every call asks k16_fullprover_last_rejection.  One line per call:
//   t=<witness> mem rc=<0 | negative status> status=<K16_CHECK_*> n=<count> list=<c0,c1,...>
//   t=<witness> file type=<t> error=<e> status=<..> n=<..> list=<..>
// A last line "idle status=<s> n=<n>" comes from a thread that never proved.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include <string>
#include <thread>
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

static std::string rejection()
{
    uint64_t n      = 0;
    int      status = -1;
    uint32_t list[K16_R1CS_REPORT_MAX + 6];
    for (uint32_t& x : list) x = 0xFFFFFFFFu;
    const int   rc = k16_fullprover_last_rejection(&n, list, K16_R1CS_REPORT_MAX + 6, &status);
    std::string s  = "status=" + std::to_string(rc ? -100 : status) + " n=" + std::to_string(n) + " list=";
    for (size_t k = 0; k < K16_R1CS_REPORT_MAX + 6 && list[k] != 0xFFFFFFFFu; k++) s += (k ? "," : "") + std::to_string(list[k]);
    return s;
}

int main(int argc, char** argv)
{
    if (argc < 6) return 2;
    std::vector<std::string> paths;
    for (char* tok = strtok(argv[3], ","); tok; tok = strtok(nullptr, ",")) paths.push_back(tok);
    const bool verify = atoi(argv[4]) != 0;
    const int  reps   = atoi(argv[5]);
    FullProver p(argv[1]);
    Peek       pk;
    static_assert(sizeof(Peek) == sizeof(FullProver), "FullProver layout");
    memcpy(&pk, &p, sizeof pk);
    printf("state=%d\n", (int)pk.state);
    printf("r1cs=%d\n", k16_fullprover_set_r1cs(&p, argv[2]));
    if (verify) printf("verify=%d\n", k16_fullprover_set_verify(&p, 1));
    fflush(stdout);
    std::vector<std::vector<unsigned char>> values(paths.size());
    for (size_t t = 0; t < paths.size(); t++)
        if (!read_wtns_values(paths[t].c_str(), &values[t])) return 3;
    std::mutex               out_mu;
    std::vector<std::thread> threads;
    for (size_t t = 0; t < paths.size(); t++)
        threads.emplace_back([&, t]() {
            for (int k = 0; k < reps; k++) {
                char      js[4096] = "";
                const int rc       = k16_fullprover_prove_mem(&p, values[t].data(), values[t].size() / 32, js, sizeof js, nullptr);
                std::string line   = "t=" + std::to_string(t) + " mem rc=" + std::to_string(rc < 0 ? rc : 0) + " " + rejection();
                {
                    std::lock_guard<std::mutex> lk(out_mu);
                    printf("%s\n", line.c_str());
                }
                ProverResponse r = p.prove(paths[t].c_str());
                line = "t=" + std::to_string(t) + " file type=" + std::to_string((int)r.type) + " error=" + std::to_string((int)r.error) + " " +
                       rejection();
                std::lock_guard<std::mutex> lk(out_mu);
                printf("%s\n", line.c_str());
            }
        });
    for (auto& th : threads) th.join();
    std::thread idle([&]() { printf("idle %s\n", rejection().c_str()); });
    idle.join();
    return 0;
}
