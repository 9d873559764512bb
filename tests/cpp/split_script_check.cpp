// tests/cpp/split_script_check.cpp -- the split check's two PROGRAMS (csrc/verify_script.h: coop_build_early_program,
// coop_build_late_program) executed on the host with the concrete field, for random points:
//   - late(early(A, B, vk_x), C) must equal final_exponentiation(miller(A,B) miller(vk_x,-gamma) miller(C,-delta)) of the
//     straight-line code AND the output of the single per-proof program for the same inputs;
//   - final_exponentiation(early output) must equal that of the two-pair product (the raw early value is not canonical:
//     vk_x's lines carry Fq factors).
// Prints the step counts of both programs and of the single one: how much of the check moves under the prover's H MSM.
//   hipcc -O1 -std=c++17 -I keyless-zk-proofs_amd/csrc tests/cpp/split_script_check.cpp -o ssc   (host code only)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "verify_script.h"

using namespace k16;

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint64_t rnd()
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static void rand_scalar(uint8_t k[32])
{
    for (int i = 0; i < 4; i++) {
        uint64_t v = rnd();
        memcpy(k + 8 * i, &v, 8);
    }
    k[31] &= 0x1f;
}
static G1Aff g1_gen()
{
    Fq one = Fq::one(), two = fadd(one, one);
    return G1Aff{one, two};
}
static G2Aff g2_gen()
{
    return G2Aff{Fq2{fq_from_dec("10857046999023057135944570762232829481370756359578518086990519993285655852781"),
                     fq_from_dec("11559732032986387107991004021392285783925812861821192530917403151452391805634")},
                 Fq2{fq_from_dec("8495653923123431417604973247489272438418190587263600148770280649306958101930"),
                     fq_from_dec("4082367875863433681332203403145435568316851327593401208105741076214120093531")}};
}
static void shape(const char* name, const CoopProgram& P)
{
    size_t nm = 0, nl = 0, ni = 0;
    for (uint8_t c : P.step_class) (c == CS_MUL ? nm : c == CS_LIN ? nl : ni)++;
    printf("%s program: %zu steps (mul %zu, lin %zu, inv %zu); ops mul %u lin %u inv %u; terms %zu; slots %u (constants %u)\n", name,
           P.step_class.size(), nm, nl, ni, P.n_mul_ops, P.n_lin_ops, P.n_inv_ops, P.terms.size(), P.n_slots, P.n_const);
}
static bool same12(const std::vector<Fq>& slots, const uint32_t out_slot[12], const Fp12& want)
{
    const Fq2* w = &want.c0.c0;
    for (int i = 0; i < 6; i++)
        if (memcmp(&slots[out_slot[2 * i]], &w[i].a, 32) || memcmp(&slots[out_slot[2 * i + 1]], &w[i].b, 32)) return false;
    return true;
}

int main()
{
    PairConsts K;
    pairing_consts_init(&K);
    CoopProgram S, E, L;
    coop_build_program(K, &S);
    coop_build_early_program(K, &E);
    coop_build_late_program(K, &L);
    shape("single", S);
    shape("early", E);
    shape("late", L);
    const size_t ns = S.step_class.size(), ne = E.step_class.size(), nl = L.step_class.size();
    printf("steps: single %zu early %zu late %zu\n", ns, ne, nl);
    // the split is worth a launch only if what has to wait for C is less than the whole check, and it may not cost more than a
    // second Miller loop's worth of steps in total (the late program squares once more per digit)
    if (!(ne > 0 && nl > 0 && nl < ns && ne < ns && ne + nl < 2 * ns)) {
        printf("step counts out of range\n");
        return 1;
    }
    if (E.n_const != S.n_const || L.n_const != S.n_const || E.in_base != S.in_base || L.in_base != S.in_base ||
        E.target_const != S.target_const) {
        printf("constant layout differs from the single program's\n");
        return 1;
    }
    int bad = 0;
    for (int trial = 0; trial < 3; trial++) {
        uint8_t k[6][32];
        for (auto& x : k) rand_scalar(x);
        G1Aff a = to_affine(pmul_scalar(G1Xyzz::from_aff(g1_gen()), k[0]));
        G1Aff c = to_affine(pmul_scalar(G1Xyzz::from_aff(g1_gen()), k[1]));
        G1Aff v = to_affine(pmul_scalar(G1Xyzz::from_aff(g1_gen()), k[2]));
        G2Aff b = to_affine(pmul_scalar(G2Xyzz::from_aff(g2_gen()), k[3]));
        G2Aff g = to_affine(pmul_scalar(G2Xyzz::from_aff(g2_gen()), k[4]));
        G2Aff d = to_affine(pmul_scalar(G2Xyzz::from_aff(g2_gen()), k[5]));
        Fp12 f0, f1, f2, two, three, want, want_early;
        miller_loop(&f0, &a, &b, &K);
        miller_loop(&f1, &v, &g, &K);
        miller_loop(&f2, &c, &d, &K);
        f12_mul(&two, &f0, &f1);
        f12_mul(&three, &two, &f2);
        final_exponentiation(&want, &three, &K);
        final_exponentiation(&want_early, &two, &K);
        std::vector<Ell> l1, l2;
        coop_prepare_lines(g, K, &l1);
        coop_prepare_lines(d, K, &l2);
        std::vector<Fq> ctab;
        coop_const_table(K, want /* any target */, l1, l2, &ctab);
        if (ctab.size() != E.n_const) {
            printf("constant table %zu != %u\n", ctab.size(), E.n_const);
            return 1;
        }
        // vk_x in projective form with a random Z, as in verify_script_check.cpp
        uint8_t kz[32];
        rand_scalar(kz);
        Fq z;
        memcpy(z.v, kz, 32);
        const Fq zz = fsqr(z), zzz = fmul(zz, z), X = fmul(v.x, zz), Y = fmul(v.y, zzz);
        const Fq sx = fmul(X, zzz), sy = fmul(Y, zz), sz = fmul(zz, zzz);
        int      diff = 0;
        // early
        std::vector<Fq> se = ctab;
        se.resize(E.n_slots, Fq::zero());
        const Fq ein[COOP_EARLY_INPUTS] = {a.x, a.y, b.x.a, b.x.b, b.y.a, b.y.b, sx, sy, sz};
        for (uint32_t i = 0; i < COOP_EARLY_INPUTS; i++) se[E.in_base + i] = ein[i];
        coop_run_host(E, se);
        Fp12 ev, ev_fe;
        Fq2* evp = &ev.c0.c0;
        for (int i = 0; i < 6; i++) evp[i] = Fq2{se[E.out_slot[2 * i]], se[E.out_slot[2 * i + 1]]};
        final_exponentiation(&ev_fe, &ev, &K);
        if (!f12_eq(ev_fe, want_early)) {
            printf("trial %d: final_exponentiation(early) differs from the two-pair product's\n", trial);
            diff++;
        }
        // late
        std::vector<Fq> sl = ctab;
        sl.resize(L.n_slots, Fq::zero());
        for (int i = 0; i < 6; i++) {
            sl[L.in_base + 2 * i]     = evp[i].a;
            sl[L.in_base + 2 * i + 1] = evp[i].b;
        }
        sl[L.in_base + 12] = c.x;
        sl[L.in_base + 13] = c.y;
        coop_run_host(L, sl);
        if (!same12(sl, L.out_slot, want)) {
            printf("trial %d: late output differs from the straight-line GT value\n", trial);
            diff++;
        }
        // the single program, same inputs
        std::vector<Fq> ss = ctab;
        ss.resize(S.n_slots, Fq::zero());
        const Fq sin[COOP_N_INPUTS] = {a.x, a.y, b.x.a, b.x.b, b.y.a, b.y.b, c.x, c.y, sx, sy, sz};
        for (uint32_t i = 0; i < COOP_N_INPUTS; i++) ss[S.in_base + i] = sin[i];
        coop_run_host(S, ss);
        for (int i = 0; i < 12; i++)
            if (memcmp(&ss[S.out_slot[i]], &sl[L.out_slot[i]], 32)) {
                printf("trial %d: late output differs from the single program's\n", trial);
                diff++;
                break;
            }
        bad += diff;
        printf("trial %d: %s\n", trial, diff ? "MISMATCH" : "split GT value identical");
    }
    return bad ? 1 : 0;
}
