"""The reference of the set-up from a trapdoor (include/k16.h k16_r1cs_setup*): Python big integers from the formulas of
tests/valid_key_builder.py and DESIGN.md section 11, points through a caller-supplied points(group, scalars) -- the tests pass
valid_key_builder.oracle_points, so the reference shares no code with the product.  Also the model of the host-side plan
(csrc/setup_plan.h) for tests/test_setup_host.py, and the test circuits both test files share.

A circuit is (n_wires, rowsA, rowsB, rowsC, n_pub_out, n_pub_in): rows of (wire, coefficient) as in tests/r1cs_builder.py."""
import struct

import pymodel as pm

R = pm.R
Q = pm.Q
G1, G2 = 0, 1
SPMV_LONG = 64


def domain(M, n_public):
    N = 1
    while N < M + n_public + 1:
        N *= 2
    return N


def roots(N):
    """(g, omega): g = 5^((r-1)/2N), omega = g^2."""
    g = pow(5, (R - 1) // (2 * N), R)
    return g, g * g % R


def lagrange_at(t, N, omega):
    """L_j(t) = (t^N - 1)/N * omega^j / (t - omega^j), one inversion each (no shared trick with the product)."""
    c = (pow(t, N, R) - 1) * pow(N, -1, R) % R
    return [c * pow(omega, j, R) % R * pow((t - pow(omega, j, R)) % R, -1, R) % R for j in range(N)]


def scalars(circuit, trapdoor):
    """dict of the scalar lists of the key: a, b (all wires), ic, c, h."""
    n_wires, rowsA, rowsB, rowsC, n_pub_out, n_pub_in = circuit
    tau, alpha, beta, gamma, delta = trapdoor
    M, n_public = len(rowsA), n_pub_out + n_pub_in
    N = domain(M, n_public)
    g, omega = roots(N)
    L = lagrange_at(tau, N, omega)
    a, b, c = [0] * n_wires, [0] * n_wires, [0] * n_wires
    for col, rows in ((a, rowsA), (b, rowsB), (c, rowsC)):
        for j, row in enumerate(rows):
            for wire, k in row:
                col[wire] = (col[wire] + k * L[j]) % R
    for i in range(n_public + 1):
        a[i] = (a[i] + L[M + i]) % R
    mix = [(beta * a[i] + alpha * b[i] + c[i]) % R for i in range(n_wires)]
    ginv, dinv = pow(gamma, -1, R), pow(delta, -1, R)
    Lc = lagrange_at(tau * pow(g, -1, R) % R, N, omega)
    hk = (pow(tau, N, R) - 1) * pow((R - 2) * delta % R, -1, R) % R
    return dict(a=a, b=b, ic=[mix[i] * ginv % R for i in range(n_public + 1)],
                c=[mix[i] * dinv % R for i in range(n_public + 1, n_wires)], h=[hk * x % R for x in Lc], N=N)


def section4(circuit):
    n_wires, rowsA, rowsB, rowsC, n_pub_out, n_pub_in = circuit
    M, n_public = len(rowsA), n_pub_out + n_pub_in
    r2 = pow(2, 512, R)
    recs = []
    for c in range(M):
        recs += [(0, c, w, k) for w, k in rowsA[c]] + [(1, c, w, k) for w, k in rowsB[c]]
    recs += [(0, M + i, i, 1) for i in range(n_public + 1)]
    return struct.pack("<I", len(recs)) + b"".join(struct.pack("<III", m, c, w) + pm.limbs(k * r2 % R) for m, c, w, k in recs)


def _section(t, payload):
    return struct.pack("<IQ", t, len(payload)) + payload


def header_ints(n_wires, n_public, N):
    return struct.pack("<I", 32) + pm.limbs(Q) + struct.pack("<I", 32) + pm.limbs(R) + struct.pack("<III", n_wires, n_public, N)


def zkey(circuit, trapdoor, points):
    """The whole key as bytes.  points(group, [int]) -> uint8 array (n, 64 | 128); points=None writes all-zero points (the
    frame the host-side writer makes before the device fills the points in)."""
    n_wires, rowsA, rowsB, rowsC, n_pub_out, n_pub_in = circuit
    n_public = n_pub_out + n_pub_in
    tau, alpha, beta, gamma, delta = trapdoor
    if points is None:
        N = domain(len(rowsA), n_public)
        pts = lambda group, n: bytes(n * (64 if group == G1 else 128))
        s = dict(a=[0] * n_wires, b=[0] * n_wires, ic=[0] * (n_public + 1), c=[0] * (n_wires - n_public - 1), h=[0] * N, N=N)
        run = lambda group, v: pts(group, len(v))
    else:
        s = scalars(circuit, trapdoor)
        run = lambda group, v: bytes(points(group, v).tobytes()) if len(v) else b""
    h1, h2 = run(G1, [alpha, beta, delta]), run(G2, [beta, gamma, delta])
    hdr = header_ints(n_wires, n_public, s["N"]) + h1[0:64] + h1[64:128] + h2[0:128] + h2[128:256] + h1[128:192] + h2[256:384]
    secs = [_section(1, struct.pack("<I", 1)), _section(2, hdr), _section(3, run(G1, s["ic"])), _section(4, section4(circuit)),
            _section(5, run(G1, s["a"])), _section(6, run(G1, s["b"])), _section(7, run(G2, s["b"])),
            _section(8, run(G1, s["c"])), _section(9, run(G1, s["h"])), _section(10, bytes(64) + struct.pack("<I", 0))]
    return b"zkey" + struct.pack("<II", 1, len(secs)) + b"".join(secs)


def sections(raw):
    """{type: payload} of an iden3 container."""
    out, pos = {}, 12
    for _ in range(struct.unpack_from("<I", raw, 8)[0]):
        t, n = struct.unpack_from("<IQ", raw, pos)
        out[t] = raw[pos + 12:pos + 12 + n]
        pos += 12 + n
    assert pos == len(raw)
    return out


def columns(circuit):
    """The transposed plan's rows as the model sees them: row m * n_wires + wire -> [(constraint, coefficient)] in constraint
    order, the file's order within a constraint, the appended public row last."""
    n_wires, rowsA, rowsB, rowsC, n_pub_out, n_pub_in = circuit
    M = len(rowsA)
    rows = [[] for _ in range(3 * n_wires)]
    for m, mat in enumerate((rowsA, rowsB, rowsC)):
        for c, row in enumerate(mat):
            for wire, k in row:
                rows[m * n_wires + wire].append((c, k))
    for i in range(n_pub_out + n_pub_in + 1):
        rows[i].append((M + i, 1))
    return rows


# ---------------------------------------------------------------- the test circuits
TRAPDOOR = tuple(1 + pm.SplitMix64(4000 + i).below(R - 1) for i in range(5))
TOY = (3, [[(1, R - 1)]], [[(2, 1)]], [[(0, R - 6)]], 1, 0)
TOY_WITNESS = [1, 2, 3]                     # -w1 * w2 = -6, wire 1 the public output


def mixed(M, n_pub_out, n_pub_in, seed=1):
    """(circuit, witness ints): M constraints over 40 + M wires, satisfied by the witness.  Whatever M is, the set holds rows
    of 0, 1, 2 and 5 terms, a wire listed twice in one combination (once summing to zero), C terms on wire 0 and on a public
    wire, a coefficient r - 1, a wire in no constraint, wire 0 in every row of B, and -- from M = 90 on -- A-columns of exactly
    64 and 65 terms (the boundary SPMV_LONG of the plan's long-row path; wire 0's column in B has M terms: the long path
    from M = 65 on)."""
    rng = pm.SplitMix64(seed * 104729 + M * 31 + n_pub_out * 7 + n_pub_in)
    n_public = n_pub_out + n_pub_in
    n_wires = 40 + M
    unused = n_wires - 1                                        # in no constraint
    w = [1] + [(rng.next() & 0xFF if rng.next() % 2 else 1 + rng.below(R - 1)) for _ in range(n_wires - 1)]
    free = list(range(n_public + 1, n_wires - 1))               # private wires that may appear
    col64, col65 = free[0], free[1]                             # A-columns of exactly 64 / 65 terms when M allows
    lengths = [0, 1, 2, 5]

    def terms(n):
        return [(free[2 + rng.next() % (len(free) - 2)], rng.below(R)) for _ in range(n)]

    def dot(row):
        return sum(k * w[s] for s, k in row) % R

    rowsA, rowsB, rowsC = [], [], []
    n64 = n65 = 0
    for c in range(M):
        a = terms(lengths[c % 4])                               # rows of 0, 1, 2, 5 terms ...
        if c % 7 == 1:                                          # a wire listed twice, summing to zero
            s = free[3 + c % 5]
            a += [(s, 5), (s, R - 5)]
        if c % 7 == 2:                                          # a wire listed twice, not summing to zero; coefficient r - 1
            s = free[4 + c % 5]
            a += [(s, R - 1), (s, 9)]
        if c % 4 and n64 < SPMV_LONG:                           # ... the non-empty ones also feed the two counted columns
            a.append((col64, 1 + rng.below(R - 1)))
            n64 += 1
        if c % 4 and n65 < SPMV_LONG + 1:
            a.append((col65, 1 + rng.below(R - 1)))
            n65 += 1
        b = [(0, 1 + rng.below(R - 1))] + terms(max(lengths[(c + 1) % 4] - 1, 0))   # wire 0 in every row of B: 1, 2, 5, 1 terms
        cc = terms(lengths[(c + 2) % 4])
        if n_public and c % 3 == 0:
            cc.append((1 + c % n_public, rng.below(R)))         # C on a public wire
        # C on wire 0, solved so that the constraint holds
        cc.append((0, (dot(a) * dot(b) - dot(cc)) % R))
        rowsA.append(a), rowsB.append(b), rowsC.append(cc)
    for row_set in (rowsA, rowsB, rowsC):
        assert all(s != unused for row in row_set for s, _ in row)
    assert all(dot(a) * dot(b) % R == dot(c) for a, b, c in zip(rowsA, rowsB, rowsC))
    if M >= 90:
        colA = columns((n_wires, rowsA, rowsB, rowsC, n_pub_out, n_pub_in))
        assert len(colA[col64]) == SPMV_LONG and len(colA[col65]) == SPMV_LONG + 1
    return (n_wires, rowsA, rowsB, rowsC, n_pub_out, n_pub_in), w


# (M, nPubOut, nPubIn): need = M + nPublic + 1 below, at and just above a power of two (62 + 2 = 64, 63 + 2 = 65)
MIXED_SHAPES = [(1, 1, 0), (61, 0, 0), (62, 1, 0), (63, 0, 1), (130, 2, 1)]
