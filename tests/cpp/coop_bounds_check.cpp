// tests/cpp/coop_bounds_check.cpp -- the bounds the wave-cooperative interpreter (k_verify_coop, csrc/verify.hip) rests on,
// EVALUATED on the four programs that actually run (full, early, late, final exponentiation), and a dump of the
// final-exponentiation program in the array format of k16_coop_exec for tests/coop_asm.py.
//   hipcc -O1 -std=c++17 -I keyless-zk-proofs_amd/csrc tests/cpp/coop_bounds_check.cpp -o cbc   (host code only)
//   cbc [--dump FILE]
//
// Every slot carries an upper bound of its value as a multiple of p, in units of p / 1024, rounded up, in integers.
//   constants, inputs   < 2p   (fq9_from_fq; the key's table is made with it)
//   MUL   needs A B <= 128, gives 1 + A B / 169                     (fmul9: (a b + m p) / R', m < R', 169 p < R' = 2^261)
//   INV   needs < 6p, gives < 2p                                    (Fermat ladder of fsqr9 / fmul9: 2 * 6 <= 128)
//   LIN   T = 2^15 p + sum cf v, with pos / neg the positive / negative part of the sum as multiples of p:
//         (a) neg < 2^15: T > 0.
//         (b) limbs 0..6 of T's accumulators add less than 2^-13 and more than -2^-16 to T / 2^232 (each |A_k| < 2^44 +
//             2^41), and limb 7 enters top_est = A_8 + floor(A_7 / 2^29) by its floor, so
//                 top_est - 2^-16 < T / 2^232 < top_est + 1 + 2^-13.
//             With p / 2^232 < 3171407:  top_est <= floor((2^15 + pos) * 3171407) + 1 =: tmax, required < 2^38.
//         (c) q = floor(floor(t / 2^11) * 5547123 / 2^33) - 2, t = top_est.  5547123 * 3171407 = 2^44 - 1332355 (the constant
//             is floor(2^44 / 3171407): the estimate errs low), so with e(t) = t * 1332355 / 2^44 (< 20819 for t < 2^38)
//                 t / 3171407 - (e(t) + 2048) / 3171407 - 3 < q <= t / 3171407 - 2,
//             i.e.  3171407 q <= t - 2 * 3171407, hence T - q p > 0;  t - 3171407 q <= 3 * 3171407 + floor(e(tmax)) + 2049;
//             and q <= qmax := floor(tmax * 5547123 / 2^44), required < 2^17.
//         (d) the result R = T - q p = (T - 3171407 * 2^232 q) + q (3171407 * 2^232 - p):
//                 R / 2^232 < 3 * 3171407 + e(tmax) + 2049 + 1 + 2^-13 + qmax d,     d = 3171407 - p / 2^232 <= 1 - P[7] / 2^29,
//             and p / 2^232 > 3171406 turns that into a multiple of p.
//             At the documented limits (operands below 5p, sum |cf| <= COOP_MAX_COEF = 4096: pos <= 20480, tmax < 2^37.3,
//             qmax = 53248) this is 3.0146 p: what the comments call "below 5p".  (Without clamping, R > 2p - 2^-16.)
//         (e) accumulators: |A_k| <= 2^44 + sum |cf| * 2^29 before, + qmax * 2^29 after the quotient: within int64.
//   outputs  <= 12p (fq9_to_fq)
#include <stdio.h>
#include <string.h>
#include <string>
#include "verify_script.h"

using namespace k16;
typedef unsigned __int128 u128;

constexpr uint64_t U = 1024; // units per p
#ifndef AUDIT_MUL_LIMIT
#define AUDIT_MUL_LIMIT 128
#endif

struct ClassMax {
    uint64_t mul_in = 0, mul_out = 0, lin_out = 0, lin_pos = 0, lin_neg = 0, inv_in = 0, out = 0, tmax = 0, qmax = 0, coef = 0, nterms = 0;
};

static bool lin_bound(u128 pos, u128 neg, uint64_t sumabs, uint64_t* res, uint64_t* tmax_o, uint64_t* qmax_o, std::string* why)
{
    if (neg >= ((u128)1 << 15) * U) return *why = "LIN: negative part reaches the 2^15 p bias", false;
    const u128 tmax = ((((u128)1 << 15) * U + pos) * 3171407u) / U + 2;
    if (tmax >= ((u128)1 << 38)) return *why = "LIN: top_est may reach 2^38", false;
    const u128 qmax = (tmax * 5547123u) >> 44;
    if (qmax >= ((u128)1 << 17)) return *why = "LIN: q may reach 2^17", false;
    const u128 acc = ((u128)1 << 44) + (u128)sumabs * ((u128)1 << 29) /* every limb of an operand below 169p is below 2^29 */ + qmax * ((u128)1 << 29) + ((u128)1 << 40);
    if (acc >= ((u128)1 << 63)) return *why = "LIN: an accumulator may leave int64", false;
    const u128 slack = ((tmax * 1332355u) >> 44) + 1 + 2049 + 2; // e(tmax) + 2049 + 1 + 2^-13, rounded up
    const u128 rn = (((u128)3u * 3171407u + slack) << 29) + qmax * (((u128)1 << 29) - Fq9C::P[7]);
    const u128 den = (u128)3171406u << 29;
    *res    = (uint64_t)((rn * U + den - 1) / den);
    *tmax_o = (uint64_t)tmax;
    *qmax_o = (uint64_t)qmax;
    return true;
}

static bool audit(const char* name, const CoopProgram& P, uint32_t n_inputs, ClassMax* M)
{
    std::string why;
    if (!coop_program_check(P, &why, n_inputs)) {
        printf("%s: coop_program_check: %s\n", name, why.c_str());
        return false;
    }
    constexpr uint64_t    UNDEF = ~0ull;
    std::vector<uint64_t> b(P.n_slots, UNDEF);
    for (uint32_t i = 0; i < P.in_base + n_inputs; i++) b[i] = 2 * U;
    b[0] = 0;
    auto rd = [&](uint32_t s, size_t step) -> uint64_t {
        if (b[s] == UNDEF) {
            printf("%s: step %zu reads slot %u before anything wrote it\n", name, step, s);
            throw 1;
        }
        return b[s];
    };
    try {
        for (size_t s = 0; s < P.step_class.size(); s++) {
            std::vector<std::pair<uint32_t, uint64_t>> wr;
            for (int l = 0; l < 64; l++) {
                const uint64_t w = P.words[s * 64 + l];
                if (!(w >> 63)) continue;
                const uint32_t dst = w & 0x3fff, a = (w >> 14) & 0x3fff, bb = (w >> 28) & 0x3fff;
                if (P.step_class[s] == CS_MUL) {
                    const u128 ab = (u128)rd(a, s) * rd(bb, s);
                    if (ab > (u128)AUDIT_MUL_LIMIT * U * U) {
                        printf("%s: step %zu lane %d: MUL operand bounds multiply to %.2f > %d\n", name, s, l, (double)ab / (U * U), AUDIT_MUL_LIMIT);
                        return false;
                    }
                    const uint64_t r = U + (uint64_t)((ab + (u128)U * 169 - 1) / ((u128)U * 169));
                    M->mul_in  = std::max<uint64_t>(M->mul_in, (uint64_t)((ab + U - 1) / U));
                    M->mul_out = std::max(M->mul_out, r);
                    wr.push_back({dst, r});
                } else if (P.step_class[s] == CS_INV) {
                    if (rd(a, s) > 6 * U) {
                        printf("%s: step %zu lane %d: INV operand bound %.3f p\n", name, s, l, (double)rd(a, s) / U);
                        return false;
                    }
                    M->inv_in = std::max(M->inv_in, rd(a, s));
                    wr.push_back({dst, 2 * U});
                } else {
                    if (l != (l / 16) * 16 + ((l % 16) / 3) * 3) continue; // first lane of a group
                    const uint32_t nt = (w >> 14) & 0x3f, t0 = (uint32_t)((w >> 20) & 0xffffff);
                    u128           pos = 0, neg = 0;
                    uint64_t       sumabs = 0;
                    for (uint32_t k = 0; k < nt; k++) {
                        const int32_t cf = (int16_t)(P.terms[t0 + k] >> 16);
                        const u128    v  = rd(P.terms[t0 + k] & 0xffff, s);
                        if (cf >= 0) pos += v * (u128)cf; else neg += v * (u128)(-cf);
                        sumabs += cf < 0 ? -cf : cf;
                    }
                    uint64_t r, tm, qm;
                    if (!lin_bound(pos, neg, sumabs, &r, &tm, &qm, &why)) {
                        printf("%s: step %zu group at lane %d: %s (pos %.2f p, neg %.2f p, sum |cf| %llu)\n", name, s, l, why.c_str(),
                               (double)pos / U, (double)neg / U, (unsigned long long)sumabs);
                        return false;
                    }
                    M->lin_out = std::max(M->lin_out, r);
                    M->lin_pos = std::max<uint64_t>(M->lin_pos, (uint64_t)((pos + U - 1) / U));
                    M->lin_neg = std::max<uint64_t>(M->lin_neg, (uint64_t)((neg + U - 1) / U));
                    M->tmax = std::max(M->tmax, tm);
                    M->qmax = std::max(M->qmax, qm);
                    M->coef = std::max(M->coef, sumabs);
                    M->nterms = std::max<uint64_t>(M->nterms, nt);
                    wr.push_back({dst, r});
                }
            }
            for (auto& x : wr) b[x.first] = x.second;
        }
        for (int i = 0; i < 12; i++) {
            const uint64_t v = rd(P.out_slot[i], P.step_class.size());
            if (v > 12 * U) {
                printf("%s: output %d bound %.3f p > 12 p\n", name, i, (double)v / U);
                return false;
            }
            M->out = std::max(M->out, v);
        }
    } catch (int) {
        return false;
    }
    printf("%s: %zu steps, %u slots | MUL A*B <= %.3f -> < %.4f p | INV operand < %.4f p | LIN pos <= %llu p neg <= %llu p, sum |cf| <= %llu, "
           "terms <= %llu, top_est < %llu (2^%.2f), q <= %llu -> < %.4f p | outputs < %.4f p\n",
           name, P.step_class.size(), P.n_slots, (double)M->mul_in / U, (double)M->mul_out / U, (double)M->inv_in / U,
           (unsigned long long)M->lin_pos, (unsigned long long)M->lin_neg, (unsigned long long)M->coef, (unsigned long long)M->nterms,
           (unsigned long long)M->tmax, __builtin_log2((double)M->tmax), (unsigned long long)M->qmax, (double)M->lin_out / U, (double)M->out / U);
    return true;
}

int main(int argc, char** argv)
{
    static_assert((u128)5547123u * 3171407u == ((u128)1 << 44) - 1332355u, "the quotient estimate's constant");
    static_assert((uint64_t)169 * (0x0030644eu + 1) < (1u << 29), "169 p < R'");
    PairConsts K;
    pairing_consts_init(&K);
    CoopProgram full, early, late, fe;
    coop_build_program(K, &full);
    coop_build_early_program(K, &early);
    coop_build_late_program(K, &late);
    coop_build_finalexp_program(K, &fe);
    {   // the documented limits themselves
        uint64_t    r, tm, qm;
        std::string why;
        if (!lin_bound((u128)COOP_MAX_COEF * 5 * U, 0, COOP_MAX_COEF, &r, &tm, &qm, &why) ||
            !lin_bound(0, (u128)COOP_MAX_COEF * 5 * U, COOP_MAX_COEF, &r, &tm, &qm, &why)) {
            printf("documented limits: %s\n", why.c_str());
            return 1;
        }
        (void)lin_bound((u128)COOP_MAX_COEF * 5 * U, 0, COOP_MAX_COEF, &r, &tm, &qm, &why);
        printf("documented limits (operands < 5p, sum |cf| <= %d): top_est < %llu (2^%.2f), q <= %llu, result < %.4f p\n", (int)COOP_MAX_COEF,
               (unsigned long long)tm, __builtin_log2((double)tm), (unsigned long long)qm, (double)r / U);
        if (r > 5 * U) {
            printf("documented limits: the result may reach 5p\n");
            return 1;
        }
    }
    ClassMax m[4];
    bool     ok = audit("full", full, COOP_N_INPUTS, &m[0]);
    ok          = audit("early", early, COOP_EARLY_INPUTS, &m[1]) && ok;
    ok          = audit("late", late, COOP_LATE_INPUTS, &m[2]) && ok;
    ok          = audit("finalexp", fe, COOP_FE_INPUTS, &m[3]) && ok;
    if (!ok) return 1;
    printf("bounds audit: 4 programs OK\n");
    // the final-exponentiation program and its constants, as k16_coop_exec takes them
    std::vector<Fq> cf(COOP_FE_NCONST, Fq::zero());
    cf[1] = Fq::one();
    {
        Fq pc[COOP_NPC];
        coop_flatten_consts(K, pc);
        for (uint32_t i = 0; i < COOP_NPC; i++) cf[2 + i] = pc[i];
    }
    std::vector<uint32_t> c9(COOP_FE_NCONST * 9);
    for (uint32_t i = 0; i < COOP_FE_NCONST; i++) {
        const Fq9 v = fq9_from_fq(cf[i]);
        memcpy(&c9[i * 9], v.l, 36);
    }
    std::string why;
    if (!coop_consts_check(c9.data(), COOP_FE_NCONST, &why)) {
        printf("finalexp constants: %s\n", why.c_str());
        return 1;
    }
    for (int i = 1; i + 1 < argc; i++)
        if (!strcmp(argv[i], "--dump")) {
            FILE* f = fopen(argv[i + 1], "wb");
            if (!f) return 2;
            uint32_t hd[16] = {(uint32_t)fe.step_class.size(), (uint32_t)fe.terms.size(), fe.n_const, fe.n_slots};
            for (int k = 0; k < 12; k++) hd[4 + k] = fe.out_slot[k];
            fwrite(hd, 4, 16, f);
            fwrite(fe.words.data(), 8, fe.words.size(), f);
            fwrite(fe.terms.data(), 4, fe.terms.size(), f);
            fwrite(c9.data(), 4, c9.size(), f);
            fwrite(fe.step_class.data(), 1, fe.step_class.size(), f);
            fclose(f);
            printf("dumped the final-exponentiation program: %zu steps, %zu terms, %u constants\n", fe.step_class.size(), fe.terms.size(), fe.n_const);
        }
    return 0;
}
