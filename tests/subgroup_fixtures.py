"""Fixture points for the point checks (csrc/bn254_points.h, k16_points_check): twist points in and out of G2, points of
small order, infinity, non-canonical encodings and points off the curve / the twist -- each one's class asserted by the
definitional test [r] Q = O over pymodel's affine arithmetic, which shares nothing with the implementation under test.

The twist E'(Fq2): y^2 = x^3 + 3 / (9 + u) has h * r points, h = 2p - r = 10069 * (a 241-bit prime).  A random twist point
R (a square root in Fq2, p = 3 mod 4) is almost never in G2; [h] R is; T = [r h / 10069] R has order exactly 10069 (the
r-part of R is cleared as well as the 241-bit part of h)."""
import functools

import numpy as np

import pymodel as pm

Q, R = pm.Q, pm.R
F2 = pm.Fq2Ops
H = 2 * Q - R                      # the twist's cofactor
SMALL = 10069                      # its small prime factor
H2 = H // SMALL
TWIST_B = pm.f2_mul((3, 0), pm.f2_inv((9, 1)))
OK, NONCANONICAL, OFF_CURVE, NOT_IN_SUBGROUP = 0, 1, 2, 3


def _fp_sqrt(a):
    s = pow(a, (Q + 1) // 4, Q)    # p = 3 mod 4
    return s if s * s % Q == a % Q else None


def fq2_sqrt(a):
    """A square root of a = a0 + a1 u in Fq2 (u^2 = -1), or None: through the norm a0^2 + a1^2 and the real part."""
    a0, a1 = a
    if a1 == 0:
        s = _fp_sqrt(a0)
        if s is not None:
            return (s, 0)
        s = _fp_sqrt(-a0 % Q)      # a0 = -s^2 = (s u)^2
        return None if s is None else (0, s)
    n = _fp_sqrt((a0 * a0 + a1 * a1) % Q)
    if n is None:
        return None
    inv2 = pow(2, -1, Q)
    for sgn in (1, -1):
        x0 = _fp_sqrt((a0 + sgn * n) * inv2 % Q)
        if x0:
            x1 = a1 * pow(2 * x0, -1, Q) % Q
            if pm.f2_mul((x0, x1), (x0, x1)) == (a0 % Q, a1 % Q):
                return (x0, x1)
    return None


def on_twist(p):
    x, y = p
    return pm.f2_mul(y, y) == pm.f2_add(pm.f2_mul(pm.f2_mul(x, x), x), TWIST_B)


def random_twist_point(rs):
    while True:
        x = (int.from_bytes(rs.bytes(32), "little") % Q, int.from_bytes(rs.bytes(32), "little") % Q)
        y = fq2_sqrt(pm.f2_add(pm.f2_mul(pm.f2_mul(x, x), x), TWIST_B))
        if y is not None:
            assert on_twist((x, y))
            return (x, y)


def in_g2(p):
    """The definitional test."""
    return p is None or pm.ec_mul(F2, p, R) is None


def g2_bytes(p):
    return np.frombuffer(pm.g2_aff_bytes(p), dtype=np.uint8)


def plus_p(b, coord):
    """The encoding with coordinate `coord` (0..3: x.a, x.b, y.a, y.b) raised by p: the same value, not canonical."""
    b = bytearray(bytes(b))
    v = pm.unlimbs(b[32 * coord:32 * coord + 32]) + Q
    b[32 * coord:32 * coord + 32] = pm.limbs(v)
    return np.frombuffer(bytes(b), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def g2_fixtures(seed=5, n_random=8):
    """(points (n, 128) uint8, expected status (n,) uint8, small_order (n,) bool).  Every on-twist point's class is the
    definitional one; small-order points are multiples of points T of order exactly 10069."""
    rs = np.random.RandomState(seed)
    on_pts, small = [], []

    def add(p, is_small=False):
        on_pts.append(p)
        small.append(is_small)

    for k in (1, 2, 3, 5, 7, 1000003, R - 1, R - 2):                  # multiples of the generator
        add(pm.ec_mul(F2, pm.G2, k))
    for _ in range(n_random):
        Rp = random_twist_point(rs)
        g = pm.ec_mul(F2, Rp, H)                                       # in G2
        T = pm.ec_mul(F2, Rp, H2 * R)                                  # order 10069
        assert T is not None and pm.ec_mul(F2, T, SMALL) is None
        k = int(rs.randint(1, 2**62))
        kG = pm.ec_mul(F2, pm.G2, k)
        for p in (Rp, g, pm.ec_add(F2, kG, T), pm.ec_add(F2, kG, Rp)):
            add(p)
            add(pm.ec_neg(F2, p))
        for m in (1, 2, 3, SMALL - 1, SMALL - 2, int(rs.randint(4, SMALL - 3))):
            t = pm.ec_mul(F2, T, m)                                    # still order 10069 (prime)
            add(t, True)
            add(pm.ec_neg(F2, t), True)
        add(pm.ec_add(F2, g, Rp))
    pts, want, sm = [], [], []
    for p, s in zip(on_pts, small):
        assert p is None or on_twist(p)
        pts.append(g2_bytes(p))
        want.append(OK if in_g2(p) else NOT_IN_SUBGROUP)
        sm.append(s)
    pts.append(g2_bytes(None))                                         # infinity
    want.append(OK)
    sm.append(False)
    # encodings: x + p (every coordinate in turn) of points in and out of G2, and points off the twist
    for i, p in enumerate(on_pts[:16]):
        if p is None:
            continue
        pts.append(plus_p(g2_bytes(p), i % 4))
        want.append(NONCANONICAL)
        sm.append(False)
        x, y = p
        off = (x, ((y[0] + 1) % Q, y[1]))
        assert not on_twist(off)
        pts.append(g2_bytes(off))
        want.append(OFF_CURVE)
        sm.append(False)
    pts.append(np.frombuffer(pm.limbs(Q) + b"\0" * 96, dtype=np.uint8))   # x.a = p, the rest 0: not canonical
    want.append(NONCANONICAL)
    sm.append(False)
    pts.append(np.frombuffer(pm.limbs(pm.to_mont(1, Q)) + b"\0" * 96, dtype=np.uint8))  # (1, 0): off the twist
    want.append(OFF_CURVE)
    sm.append(False)
    return np.stack(pts), np.array(want, dtype=np.uint8), np.array(sm, dtype=bool)


@functools.lru_cache(maxsize=None)
def g1_fixtures():
    """(points (n, 64) uint8, expected status): multiples of G1, infinity, x + p / y + p encodings, points off the curve."""
    pts, want = [], []
    for k in (1, 2, 3, 12345, R - 1):
        p = pm.ec_mul(pm.Fq1Ops, pm.G1, k)
        b = pm.g1_aff_bytes(p)
        pts.append(b)
        want.append(OK)
        for c in (0, 1):
            v = bytearray(b)
            v[32 * c:32 * c + 32] = pm.limbs(pm.unlimbs(b[32 * c:32 * c + 32]) + Q)
            pts.append(bytes(v))
            want.append(NONCANONICAL)
        pts.append(pm.g1_aff_bytes((p[0], (p[1] + 1) % Q)))
        want.append(OFF_CURVE)
    pts.append(b"\0" * 64)
    want.append(OK)
    return np.stack([np.frombuffer(b, dtype=np.uint8) for b in pts]), np.array(want, dtype=np.uint8)


def non_g2_points(count, seed=11):
    """`count` encoded twist points outside G2 (k G2 + T and random R, cycled), all asserted by the definitional test."""
    pts, st, _ = g2_fixtures()
    bad = pts[st == NOT_IN_SUBGROUP]
    return np.stack([bad[i % len(bad)] for i in range(count)])


@functools.lru_cache(maxsize=None)
def small_order_point(seed=21):
    """A twist point T of order exactly 10069 (pymodel affine ints)."""
    rs = np.random.RandomState(seed)
    while True:
        T = pm.ec_mul(F2, random_twist_point(rs), H2 * R)
        if T is not None:
            assert pm.ec_mul(F2, T, SMALL) is None
            return T


@functools.lru_cache(maxsize=None)
def outside_g2_point(seed=23):
    """A random twist point that the definitional test places outside G2."""
    p = random_twist_point(np.random.RandomState(seed))
    assert not in_g2(p)
    return p
