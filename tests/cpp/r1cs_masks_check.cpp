// r1cs_masks_check.cpp -- stand-alone driver of keyless-zk-proofs_amd/csrc/r1cs_masks.h for tests/test_r1cs_masks_host.py (built
// with -fsanitize=address,undefined, run as a plain subprocess):
//   r1cs_masks_check CASES.txt     one case per line, one line of output per case.  Masks are W = ceil(n_wires / 64) hex words;
//                                  `outs` is a bit set of the output pointers that are NOT null.
//     unbound n_wires cap outs present[W] bound[W]            outs: 1 h_wires, 2 h_class, 4 h_status
//     second  n_wires cap outs present[W] pinned[W] rooted[W] outs: 1 list, 4 h_status
//     closure n_wires cap outs present[W] seed[W] known[W]    outs: 1 h_wires, 4 h_status, 8 h_round
//     seed    n_wires n_pub_out n_pub_in n_prv_in default | list k wire...
// Every buffer is a heap block of exactly the size the call may touch -- a list has `cap` places, a status map n_wires bytes, a
// mask W words -- so a step beyond one stops the program; lists and maps are filled with a pattern first and printed whole.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include "r1cs_masks.h"

using namespace k16;

template <class T>
static std::unique_ptr<T[]> block(size_t n, T fill)
{
    std::unique_ptr<T[]> p(new T[n]);
    for (size_t i = 0; i < n; i++) p[i] = fill;
    return p;
}
template <class T>
static std::unique_ptr<T[]> words(std::istringstream& in, size_t n)
{
    std::unique_ptr<T[]> p(new T[n]);
    for (size_t i = 0; i < n; i++) {
        unsigned long long v = 0;
        in >> std::hex >> v >> std::dec;
        p[i] = (T)v;
    }
    return p;
}
template <class T>
static void show(const char* name, const T* p, size_t n, bool there)
{
    printf(" %s=", name);
    if (!there) printf("-");
    for (size_t i = 0; there && i < n; i++) printf("%s%llx", i ? "," : "", (unsigned long long)p[i]);
}

int main(int argc, char** argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: r1cs_masks_check CASES.txt\n");
        return 2;
    }
    std::ifstream file(argv[1]);
    std::string   line, kind;
    while (std::getline(file, line)) {
        std::istringstream in(line);
        uint32_t           n = 0, cap = 0, outs = 0;
        in >> kind >> n;
        const size_t W = ((size_t)n + 63) / 64;
        if (kind == "seed") {
            uint32_t    po = 0, pi = 0, pr = 0, k = 0;
            std::string mode;
            in >> po >> pi >> pr >> mode;
            if (mode == "list") in >> k;
            auto list = block<uint32_t>(k, 0);
            for (uint32_t i = 0; i < k; i++) in >> list[i];
            auto        seed = block<unsigned long long>(W, 0x5a5a5a5a5a5a5a5aull);
            const char* why  = r1cs_seed_mask(n, po, pi, pr, mode == "list" ? list.get() : nullptr, k, seed.get());
            printf("refused=%s", why ? why : "-");
            show("seed", seed.get(), W, true);
            printf("\n");
            continue;
        }
        in >> cap >> outs;
        auto present = words<uint64_t>(in, W);
        auto m1      = words<unsigned long long>(in, W);
        auto wires   = block<uint32_t>(cap, 0xa5a5a5a5u);
        auto cls     = block<uint8_t>(cap, 0xa5);
        auto status  = block<uint8_t>(n, 0xa5);
        auto round   = block<uint32_t>(n, 7);
        uint32_t* h_wires  = outs & 1 ? wires.get() : nullptr;
        uint8_t*  h_status = outs & 4 ? status.get() : nullptr;
        if (kind == "unbound") {
            uint64_t absent = 99, unbound = 99;
            r1cs_masks_unbound(n, present.get(), m1.get(), &absent, &unbound, h_wires, outs & 2 ? cls.get() : nullptr, cap, h_status);
            printf("absent=%llu unbound=%llu", (unsigned long long)absent, (unsigned long long)unbound);
            show("wires", wires.get(), cap, h_wires);
            show("class", cls.get(), cap, outs & 2);
        } else if (kind == "second") {
            auto           rooted = words<unsigned long long>(in, W);
            uint64_t       two    = 99;
            const uint32_t listed = r1cs_masks_second(n, present.get(), m1.get(), rooted.get(), &two, h_wires, cap, h_status);
            printf("two=%llu listed=%u", (unsigned long long)two, listed);
            show("wires", wires.get(), cap, h_wires);
        } else if (kind == "closure") {
            auto     known   = words<unsigned long long>(in, W);
            uint64_t derived = 99, absent = 99, open = 99;
            r1cs_masks_closure(n, present.get(), m1.get(), known.get(), &derived, &absent, &open, h_wires, cap, h_status,
                               outs & 8 ? round.get() : nullptr);
            printf("derived=%llu absent=%llu open=%llu", (unsigned long long)derived, (unsigned long long)absent, (unsigned long long)open);
            show("wires", wires.get(), cap, h_wires);
            show("round", round.get(), n, outs & 8);
        } else {
            printf("FAIL unknown case %s\n", kind.c_str());
            return 1;
        }
        if (!in) {
            printf("FAIL short case\n");
            return 1;
        }
        show("status", status.get(), n, h_status);
        printf("\n");
    }
    return 0;
}
