// bn254_points.h -- validation of encoded points: canonical coordinates, on the curve / the twist, and membership of a
// twist point in G2 (the order-r subgroup of E'(Fq2)).  What ark-serialize's validated deserialisation checks.
// __host__ __device__: the verifier's kernels (verify.hip), the batched point checks (points_check.hip) and the host-side
// cross-check (tests/cpp/subgroup_check.cpp) compile the same code.
//
// G1 has cofactor 1, so a G1 point on the curve is in the group.  The twist has cofactor h = 2p - r = 10069 * (241-bit
// prime), so a point on the twist need not be in G2: it is tested with the endomorphism psi (g2_mul_by_char), which acts
// on G2 as multiplication by p = 6x^2 (mod r).  El Housni, Guillevic, Piellard, "Co-factor clearing and subgroup
// membership testing on pairing-friendly curves", eprint 2022/348, section 5.1 (BN curves):
//     Q in G2   <=>   [x + 1] Q + psi([x] Q) + psi^2([x] Q) == psi^3([2x] Q),      x = 4965661367192848881
// 62 doublings and 27 additions for [x] Q, three more additions and a doubling; the two sides are compared projectively.
// The generic XYZZ formulas of bn254_curve.h keep the reference's exceptional cases (P = Q, P = -Q, infinity), but for a
// point on the twist the [x] Q chain cannot reach them: it would need ord(Q) to divide a partial multiple s, s - 1 or s + 1
// (all < 2^63), the only order that small is 10069, and no partial multiple of the chain is 0 or +-1 mod 10069
// (x = 2636 mod 10069).  None of the test fixtures reaches them after the chain either: they are kept, not exercised.
#pragma once
#include "bn254_curve.h"
#include "bn254_fq9.h"

namespace k16 {

// per-point status (include/k16.h K16_PT_*): the first check that fails, in this order
enum : uint8_t { PT_OK = 0, PT_NONCANONICAL = 1, PT_OFF_CURVE = 2, PT_NOT_IN_SUBGROUP = 3 };

// the twist's curve constant and the two constants of psi (PairConsts::twist_b, twqx, twqy of bn254_pairing.h)
struct G2Consts {
    Fq2 twist_b, twqx, twqy;
};

K16_HD bool fq_canonical(const Fq& x)
{
    uint32_t borrow = 0; // x - p borrows  <=>  x < p
#pragma unroll
    for (int i = 0; i < 8; i++) borrow = (uint32_t)(((uint64_t)x.v[i] - FqParams::P[i] - borrow) >> 63);
    return borrow != 0;
}
// canonical coordinates first, then y^2 = x^3 + 3; the all-zero encoding is the point at infinity
K16_HD uint8_t g1_point_status(const G1Aff& a)
{
    if (!fq_canonical(a.x) || !fq_canonical(a.y)) return PT_NONCANONICAL;
    if (a.is_zero()) return PT_OK;
    const Fq three = fadd(fadd(Fq::one(), Fq::one()), Fq::one());
    return fsqr(a.y) == fadd(fmul(fsqr(a.x), a.x), three) ? PT_OK : PT_OFF_CURVE;
}
K16_HD bool g1_input_ok(const G1Aff& a) { return g1_point_status(a) == PT_OK; }
// canonical coordinates first, then y^2 = x^3 + 3 / (9 + u)
K16_HD uint8_t g2_twist_status(const G2Aff& b, const Fq2& twist_b)
{
    if (!fq_canonical(b.x.a) || !fq_canonical(b.x.b) || !fq_canonical(b.y.a) || !fq_canonical(b.y.b)) return PT_NONCANONICAL;
    if (b.is_zero()) return PT_OK;
    return fsqr(b.y) == fadd(fmul(fsqr(b.x), b.x), twist_b) ? PT_OK : PT_OFF_CURVE;
}
K16_HD bool g2_input_ok(const G2Aff& b, const Fq2& twist_b) { return g2_twist_status(b, twist_b) == PT_OK; }

// ---------------------------------------------------------------- the G2 test, on any Fq2 representation F
// F needs fadd / fsub / fmul / fsqr / fdbl / fneg, is_zero() (exact mod p), g2_conj and fq2_to (canonical Fq2 -> F):
// Fq2 (canonical), Fq2n (one lane, radix 2^29) and Fq2h (a lane pair, points_check.hip).
K16_HD Fq2  g2_conj(const Fq2& x) { return Fq2{x.a, fneg(x.b)}; }
K16_HD Fq2n g2_conj(const Fq2n& x) { return Fq2n{x.a, fred9(fsub9<4>(fq9_zero(), x.b))}; }
K16_HD void fq2_to(const Fq2& x, Fq2& out) { out = x; }
K16_HD void fq2_to(const Fq2& x, Fq2n& out) { out = fq2n_from_canonical(x); }

constexpr uint64_t BN_X = 4965661367192848881ull; // the BN parameter of BN254 (0x44e992b44a6909f1: 63 bits, 28 set)

// psi on XYZZ (x = X / ZZ, y = Y / ZZZ): conjugate all four coordinates, X *= twqx, Y *= twqy
template <class F>
K16_HD Xyzz<F> g2_psi(const Xyzz<F>& p, const F& wx, const F& wy)
{
    return Xyzz<F>{fmul(g2_conj(p.x), wx), fmul(g2_conj(p.y), wy), g2_conj(p.zz), g2_conj(p.zzz)};
}
// P == Q without inversion: X1 ZZ2 == X2 ZZ1 and Y1 ZZZ2 == Y2 ZZZ1
template <class F>
K16_HD bool xyzz_equal(const Xyzz<F>& p, const Xyzz<F>& q)
{
    const bool pz = p.is_zero(), qz = q.is_zero();
    if (pz || qz) return pz && qz;
    return fsub(fmul(p.x, q.zz), fmul(q.x, p.zz)).is_zero() && fsub(fmul(p.y, q.zzz), fmul(q.y, p.zzz)).is_zero();
}
// q: a point of the twist (infinity allowed) -> q in G2 (eprint 2022/348 section 5.1, see the top of this file)
template <class F>
K16_HD bool g2_in_subgroup(const Aff<F>& q, const F& wx, const F& wy)
{
    Xyzz<F> a = Xyzz<F>::from_aff(q); // the top bit of x
#pragma clang loop unroll(disable)
    for (int i = 61; i >= 0; i--) {
        a = pdbl(a);
        if ((BN_X >> i) & 1) a = padd_mixed(a, q);
    }
    const Xyzz<F> p1  = g2_psi(a, wx, wy);                  // psi([x] Q)
    const Xyzz<F> p2  = g2_psi(p1, wx, wy);                 // psi^2([x] Q)
    const Xyzz<F> lhs = padd(padd(padd_mixed(a, q), p1), p2); // [x + 1] Q + psi([x] Q) + psi^2([x] Q)
    const Xyzz<F> rhs = g2_psi(pdbl(p2), wx, wy);           // psi^3([2x] Q) = psi([2] psi^2([x] Q))
    return xyzz_equal(lhs, rhs);
}
// the status of an encoded G2 point: canonical, on the twist, in G2 (the arithmetic of the last test in F)
template <class F>
K16_HD uint8_t g2_point_status(const G2Aff& b, const G2Consts& K)
{
    const uint8_t s = g2_twist_status(b, K.twist_b);
    if (s != PT_OK || b.is_zero()) return s;
    Aff<F> q;
    F      wx, wy;
    fq2_to(b.x, q.x);
    fq2_to(b.y, q.y);
    fq2_to(K.twqx, wx);
    fq2_to(K.twqy, wy);
    return g2_in_subgroup(q, wx, wy) ? PT_OK : PT_NOT_IN_SUBGROUP;
}

} // namespace k16
