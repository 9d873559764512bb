// tests/cpp/fold_script_check.cpp -- the folded verifier's PROGRAM (csrc/verify_script.h, coop_build_finalexp_program: ONE
// final exponentiation for the wave-cooperative interpreter) executed on the host with the concrete field, against
// final_exponentiation of the straight-line code: byte-equal for random Fp12 inputs.  Prints the program's shape.
//   hipcc -O1 -std=c++17 -I keyless-zk-proofs_amd/csrc tests/cpp/fold_script_check.cpp -o fsc   (host code only)
#include <stdio.h>
#include <string.h>
#include "verify_script.h"

using namespace k16;

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd()
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static Fq rand_fq()
{
    Fq x;
    for (int i = 0; i < 4; i++) {
        const uint64_t v = rnd();
        memcpy((uint8_t*)x.v + 8 * i, &v, 8);
    }
    x.v[7] &= 0x1fffffffu; // < 2^253 < p: canonical
    return x;
}

int main()
{
    PairConsts K;
    pairing_consts_init(&K);
    CoopProgram P;
    coop_build_finalexp_program(K, &P);
    size_t nm = 0, nl = 0, ni = 0;
    for (uint8_t c : P.step_class) (c == CS_MUL ? nm : c == CS_LIN ? nl : ni)++;
    printf("fold program: %zu steps (mul %zu, lin %zu, inv %zu); ops mul %u lin %u inv %u; terms %zu; slots %u (constants %u, inputs %u)\n",
           P.step_class.size(), nm, nl, ni, P.n_mul_ops, P.n_lin_ops, P.n_inv_ops, P.terms.size(), P.n_slots, P.n_const, COOP_FE_INPUTS);
    if (P.n_const != COOP_FE_NCONST || P.in_base != COOP_FE_NCONST) {
        printf("constant layout\n");
        return 1;
    }
    // the constants: the head of the per-proof program's table
    Fq pc[COOP_NPC];
    coop_flatten_consts(K, pc);
    int bad = 0;
    for (int trial = 0; trial < 5; trial++) {
        Fp12 f, want;
        Fq2* fv = &f.c0.c0;
        for (int i = 0; i < 6; i++) fv[i] = Fq2{rand_fq(), rand_fq()};
        if (trial == 4) { // the value of an all-valid fold before the final exponentiation may be anything; after it, of 1: 1
            f = f12_one();
        }
        const bool good = final_exponentiation(&want, &f, &K);
        std::vector<Fq> slots(P.n_slots, Fq::zero());
        slots[1] = Fq::one();
        for (uint32_t i = 0; i < COOP_NPC; i++) slots[2 + i] = pc[i];
        for (int i = 0; i < 6; i++) {
            slots[P.in_base + 2 * i]     = fv[i].a;
            slots[P.in_base + 2 * i + 1] = fv[i].b;
        }
        coop_run_host(P, slots);
        const Fq2* w = &want.c0.c0;
        int        diff = good ? 0 : 1;
        for (int i = 0; i < 6; i++)
            if (memcmp(&slots[P.out_slot[2 * i]], &w[i].a, 32) || memcmp(&slots[P.out_slot[2 * i + 1]], &w[i].b, 32)) diff++;
        bad += diff;
        printf("trial %d: %s\n", trial, diff ? "MISMATCH" : "final exponentiation identical");
    }
    return bad ? 1 : 0;
}
