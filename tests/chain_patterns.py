"""Directed circuits and witnesses for the prover's quotient chain (k_spmv -> inverse k_ntt_pass9 passes with the TAIL store ->
forward passes -> k_mul -> k_hscalars), shared by tests/test_chain_directed_host.py (CPU) and tests/test_gpu_chain_directed.py.

Every circuit is CONSTRUCTED: the evaluation vectors A.w and B.w, the products and the row sums are chosen, not drawn.  All
witness values and coefficients are canonical (< r): every input is a valid input of the reference prover.

Also here: the integer meaning of the device's lazy product and reduction (bn254_fq9.h: fmul9_t, fred9_t), used to pick wire
values whose stored representative is >= r (what k_spmv stores for whole rows comes from tests/cpp/chain_spmv_model.cpp, the
device headers compiled for the host), and a plain big-integer computation of the H scalars straight from the reference's
definition (RS/groth16.cpp:137-275) with O(N^2) transforms.
"""
import numpy as np

import pymodel as pm

R = pm.R

# ---------------------------------------------------------------------------------------------------------------- device model
# Fr9 values are integers congruent to x * 2^261 mod r.  fmul9_t returns exactly (a b + m r) / 2^261 with m = -a b / r mod 2^261;
# fmul9_small_t is the same integer for a single-limb operand; fred9_t subtracts floor(top limb / 3171407) * r.
R9 = 1 << 261
_RINV9 = pow(R, -1, R9)
K522 = pow(2, 522, R)
FRED_KEEPS_BELOW = 3171407 << 232      # fred9_t leaves a value below this alone: r < this < r (1 + 2.3e-7)
SPMV_LONG = 64


def mont9(a, b):
    t = a * b
    return (t + ((-t * _RINV9) % R9) * R) >> 261


def fred9(v):
    return v - ((v >> 232) // 3171407) * R


def coef9(c):
    """what k16_prover_create stores for a coefficient c: c * 2^522 mod r, canonical"""
    return c * K522 % R


def term9(coef, w):
    """k_spmv's term(): wire value w (standard form, as the witness holds it) times the stored coefficient"""
    return mont9(w, coef9(coef))


# ------------------------------------------------------------------------------------------- the reference, in big integers
def root_of_unity(logk):
    """the primitive 2^logk-th root the reference's FFT uses (RS/fft.cpp:40-136: 5 is the smallest non-residue)"""
    return pow(5, (R - 1) >> logk, R)


def reference_h(N, matrix, constraint, wire, value, w):
    """RS/groth16.cpp:137-275 in plain integers: a = A.w, b = B.w, c = a * b pointwise; each polynomial interpolated over the
    N-th roots (O(N^2) inverse DFT), its coefficient i multiplied by g^i (g the 2N-th root), evaluated again (O(N^2) DFT);
    h = a * b - c, in standard form."""
    a, b = [0] * N, [0] * N
    for m, c, s, v in zip(matrix, constraint, wire, value):
        t = (a if m == 0 else b)
        t[int(c)] = (t[int(c)] + int(w[int(s)]) * int(v)) % R
    c_ = [x * y % R for x, y in zip(a, b)]
    logn = N.bit_length() - 1
    om, g = root_of_unity(logn), root_of_unity(logn + 1)
    om_pow = [pow(om, i, R) for i in range(N)]
    ninv = pow(N, -1, R)

    def coset(ev):
        co = [sum(ev[i] * om_pow[(-i * j) % N] for i in range(N)) * ninv % R for j in range(N)]
        co = [x * pow(g, j, R) % R for j, x in enumerate(co)]
        return [sum(co[j] * om_pow[(i * j) % N] for j in range(N)) % R for i in range(N)]

    a, b, c_ = coset(a), coset(b), coset(c_)
    return [(x * y - z) % R for x, y, z in zip(a, b, c_)]


# ---------------------------------------------------------------------------------------------------------- extremal values
def above_r_wires(count, coef=1, narrow=None):
    """Values v for which the product k_spmv forms -- coef * v with v in a wire, or v * narrow with v the COEFFICIENT of a wire
    holding `narrow` < 256 -- has a device representative in [r, FRED_KEEPS_BELOW): fred9_t leaves it alone, so a row of that
    single term is stored >= r.  The Montgomery product's result is the residue or the residue + r; it is residue + r
    whenever the residue is small against the product's size, which the loop checks with the model."""
    out, j = [], 0
    step = (FRED_KEEPS_BELOW - R) // (4 * count + 9)
    inv = pow(pow(2, 261, R), -1, R)
    while len(out) < count:
        j += 1
        target = R + 1 + j * step
        assert target < FRED_KEEPS_BELOW
        x = target * inv % R                                 # the field element whose representative we want to be `target`
        if narrow is None:
            v = x * pow(coef, -1, R) % R
            got = term9(coef, v)
        else:
            v = x * pow(narrow, -1, R) % R
            got = term9(v, narrow)
        if got == target and fred9(got) >= R:
            out.append(v)
    return out


ABOVE = above_r_wires(2)
EXTREMAL = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, 255, 256, (1 << 15) - 1, 1 << 15, (1 << 29) - 1, 1 << 29,
            1 << 232, 1 << 253] + ABOVE
EXTREMAL_IDS = ["0", "1", "2", "r-1", "r-2", "(r-1)/2", "(r+1)/2", "255", "256", "2^15-1", "2^15", "2^29-1", "2^29", "2^232",
                "2^253", "above_r_0", "above_r_1"]


class _Rng(pm.SplitMix64):
    """pm.SplitMix64.below rejects 254-bit draws (made for field elements); small ranges take one 64-bit word"""

    def below(self, n):
        return self.next() % n if n < (1 << 32) else pm.SplitMix64.below(self, n)


class Circuit:
    """Coefficient list + witness under construction.  Wire 0 is the constant 1, wire 1 the public signal."""

    def __init__(self, N, n_public=1, one_is_wire0=True):
        self.N, self.n_public = N, n_public
        self.m, self.c, self.s, self.v = [], [], [], []
        self.w = [1]
        self._wire = {1: 0} if one_is_wire0 else {}    # value -> wire; without wire 0 a witness of zeros zeroes every row
        self.targets = {}                  # what the host teeth tests assert: name -> list of row ids
        self.sel = None                    # selector(): per matrix (even wire, odd wire, {special row: wire})

    def wire(self, value, fresh=False):
        value = int(value) % R
        if fresh or value not in self._wire:
            self.w.append(value)
            if fresh:
                return len(self.w) - 1
            self._wire[value] = len(self.w) - 1
        return self._wire[value]

    def add(self, m, c, s, v):
        assert 0 <= c < self.N and 0 <= s < len(self.w) and 0 <= v < R
        self.m.append(m), self.c.append(c), self.s.append(s), self.v.append(v)

    def put(self, m, c, value, form="wire"):
        """a one-term row contribution equal to `value`: the value in a wire with coefficient 1 ("wire": narrow product for
        values below 256, wide otherwise), as the coefficient of wire 0 ("coef": narrow product), or as a coefficient of the
        wide wire r - 2 ("wide")"""
        value %= R
        if form == "wire":
            self.add(m, c, self.wire(value), 1)
        elif form == "coef":
            self.add(m, c, 0, value)
        else:
            self.add(m, c, self.wire(R - 2), value * pow(R - 2, -1, R) % R)

    def pad_vars(self, n_vars):
        """unused wires up to n_vars: bytes, every eighth one an extremal value (13 of the 17 are wide: about a tenth of the
        wires, so that the witness fits the compact upload's lists -- see compact_upload_fits)"""
        k = 0
        while len(self.w) < n_vars:
            self.w.append(EXTREMAL[(k // 8) % len(EXTREMAL)] if k % 8 == 0 else k % 256)
            k += 1
        return self

    @property
    def n_vars(self):
        return len(self.w)

    def finish(self):
        while len(self.w) < self.n_public + 3:
            self.w.append(0)
        return self

    def rows(self):
        return self.m, self.c, self.s, self.v

    def row_sums(self, w=None):
        w = self.w if w is None else w
        out = {}
        for m, c, s, v in zip(*self.rows()):
            row = (0 if m == 0 else self.N) + c
            out[row] = (out.get(row, 0) + w[s] * v) % R
        return out

    def write(self, zkey_path, wtns_path=None):
        import zkey_builder as zb
        self.finish()
        zb.build_zkey_rows(zkey_path, self.n_vars, self.n_public, self.N, *self.rows())
        if wtns_path:
            zb.write_wtns(wtns_path, self.w)

    def witness_bytes(self, w=None):
        return np.frombuffer(b"".join(pm.limbs(int(v)) for v in (self.w if w is None else w)), dtype=np.uint8).reshape(-1, 32)


def compact_upload_fits(w):
    """prover.hip WitnessPacker: a witness of >= 2^16 wires crosses in compact form when each of the 32 ranges
    [n t / 32, n (t + 1) / 32) holds at most (n / 32) / 4 + 64 values >= 256; otherwise the proof copies it plainly"""
    n = len(w)
    cap = (n // 32) // 4 + 64
    return n >= (1 << 16) and all(sum(1 for v in w[n * t // 32:n * (t + 1) // 32] if v >= 256) <= cap for t in range(32))


def brev(v, logn):
    return int(format(v, "0%db" % logn)[::-1], 2) if logn else 0


def first_pass_stages(logn):
    """ntt_passes (ntt.hip): the first pass of a transform runs min(logn, 10) stages; an odd count opens with one radix-2 stage"""
    return min(logn, 10)


# ---------------------------------------------------------------------------------------------------------- SpMV patterns
ROW_LENGTHS = (1, 2, 63, 64, 65, 128, 129, 4096)


def _spread(N, k):
    return (k * 2654435761 + 17) % N


def spmv_maximal(N, wide):
    """every term maximal: coefficient r - 1 times a wire of 255 (single-limb product) or r - 1 (full product); rows of every
    listed length in A and in B, several of each"""
    cir = Circuit(N)
    wv = R - 1 if wide else 255
    k, lengths = 0, {}
    for ln in ROW_LENGTHS:
        for _ in range(2 if ln > 200 else 3):
            for m in (0, 1):
                c = _spread(N, k)
                k += 1
                while (0 if m == 0 else N) + c in lengths:
                    c = (c + 1) % N
                lengths[(0 if m == 0 else N) + c] = ln
                for _ in range(ln):
                    cir.add(m, c, cir.wire(wv), R - 1)
    cir.targets["row_lengths"] = lengths
    return cir.finish()


def spmv_cancel(N):
    """rows whose terms cancel to exactly 0 mod r: x and r - x in both orders, as wire values and as coefficients, for every
    extremal x; long rows with the cancelling partner in the next lane and in the same lane one round later"""
    cir = Circuit(N)
    zero_rows, k = [], 0
    xs = [x for x in EXTREMAL if x]
    for x in xs:
        for order in (0, 1):
            for form in ("wire", "coef", "wide"):
                m, c = k & 1, _spread(N, k) if N > 256 else (k // 2) % N
                while (0 if m == 0 else N) + c in zero_rows:
                    c = (c + 1) % N
                k += 1
                pair = (x, R - x) if order == 0 else (R - x, x)
                for t in pair:
                    cir.put(m, c, t, form)
                zero_rows.append((0 if m == 0 else N) + c)
    for j, (ln, dist) in enumerate(((65, 1), (129, 1), (129, 64), (200, 64), (4096, 1), (4096, 64))):
        m = j & 1
        c = (N - 1 - j) % N
        while (0 if m == 0 else N) + c in zero_rows:
            c = (c - 1) % N
        vals = [0] * ln
        for i in range(ln):
            if vals[i] == 0 and i + dist < ln and vals[i + dist] == 0:
                x = xs[(i + j) % len(xs)]
                vals[i], vals[i + dist] = x, R - x
        for i, t in enumerate(vals):                      # the unpaired entries are products with a zero coefficient
            if t:
                cir.put(m, c, t, ("wire", "coef", "wide")[i % 3])
            else:
                cir.add(m, c, cir.wire(R - 1), 0)
        zero_rows.append((0 if m == 0 else N) + c)
    cir.targets["zero_rows"] = zero_rows
    return cir.finish()


def spmv_sum_r_minus_1(N):
    """rows that sum to r - 1: maximal terms, the last one chosen to land on r - 1"""
    cir = Circuit(N)
    rows = []
    k = 0
    for ln in (1, 2, 3, 63, 64, 65, 128, 129, 4096):
        for m in (0, 1):
            c = _spread(N, k) if N > 256 else k % N
            k += 1
            while (0 if m == 0 else N) + c in rows:
                c = (c + 1) % N
            total = 0
            for i in range(ln - 1):
                wv = (255, R - 1, R - 2)[i % 3]
                cir.add(m, c, cir.wire(wv), R - 1)
                total = (total + wv * (R - 1)) % R
            cir.put(m, c, (R - 1 - total) % R, ("wire", "coef", "wide")[ln % 3])
            rows.append((0 if m == 0 else N) + c)
    cir.targets["r_minus_1_rows"] = rows
    return cir.finish()


def spmv_mixed(N):
    """rows that alternate narrow and wide wires, every coefficient extremal"""
    cir = Circuit(N)
    k = 0
    for ln in (2, 3, 64, 65, 200):
        for m in (0, 1):
            c = _spread(N, k) if N > 256 else (5 * k + 1) % N
            k += 1
            for i in range(ln):
                wv = (255, R - 1, 1, 1 << 253, 0, 256)[i % 6]
                cir.add(m, c, cir.wire(wv), EXTREMAL[(i + k) % len(EXTREMAL)])
    return cir.finish()


def spmv_wire0(N):
    """wire 0 (the constant 1) with every extremal coefficient: one row each, and all of them in one row"""
    cir = Circuit(N)
    for m in (0, 1):
        for i, x in enumerate(EXTREMAL):
            cir.add(m, (i + 3 * m) % N, 0, x)
        for x in EXTREMAL:
            cir.add(m, N - 1 - m if N > 2 else 0, 0, x)
    return cir.finish()


SPMV_PATTERNS = {
    "maximal_narrow": lambda N: spmv_maximal(N, False),
    "maximal_wide": lambda N: spmv_maximal(N, True),
    "cancel_to_zero": spmv_cancel,
    "sum_r_minus_1": spmv_sum_r_minus_1,
    "mixed_narrow_wide": spmv_mixed,
    "wire0_extremal_coefs": spmv_wire0,
}


# ---------------------------------------------------------------------------------------------------- degenerate matrices
def dense(N, seed=1, matrices=(0, 1)):
    """every row of the given matrices: two terms, extremal coefficient times extremal wire; wire 0 is not used, so a witness
    of zeros makes every evaluation zero"""
    cir = Circuit(N, one_is_wire0=False)
    rng = _Rng(seed)
    for m in matrices:
        for c in range(N):
            for _ in range(2):
                cir.add(m, c, cir.wire(EXTREMAL[rng.below(len(EXTREMAL))]), EXTREMAL[1 + rng.below(len(EXTREMAL) - 1)])
    return cir.finish()


def single_row(N, c):
    cir = Circuit(N)
    for m in (0, 1):
        cir.add(m, c, cir.wire(R - 2), R - 1)
        cir.add(m, c, cir.wire(255), (R + 1) // 2)
    return cir.finish()


def matrix1_sparse(N):
    cir = Circuit(N)
    for k in range(max(1, N // 8)):
        cir.add(1, _spread(N, k), cir.wire(EXTREMAL[k % len(EXTREMAL)]), EXTREMAL[(k + 5) % len(EXTREMAL)])
    return cir.finish()


DEGENERATE_PATTERNS = {
    "a_zero_b_dense": lambda N: dense(N, 3, (1,)),
    "a_dense_b_zero": lambda N: dense(N, 4, (0,)),
    "both_zero": lambda N: Circuit(N).finish(),
    "single_row_0": lambda N: single_row(N, 0),
    "single_row_half": lambda N: single_row(N, N // 2),
    "single_row_last": lambda N: single_row(N, N - 1),
    "only_matrix_1_rows": matrix1_sparse,
}


# -------------------------------------------------------------------------------------------------- structured polynomials
# One key per size carries every witness-driven pattern: row i of A reads wire A_even / A_odd by the parity of i, except the
# rows 0, 1, N/2, N-1, which read a wire of their own; B likewise.  The witness then sets constants, deltas and alternations.
def special_rows(N):
    return sorted({0, 1 % N, N // 2, N - 1})


def selector(N):
    cir = Circuit(N)
    sp = special_rows(N)
    cir.sel = {}
    for m in (0, 1):
        ev, od = cir.wire(0, fresh=True), cir.wire(0, fresh=True)
        spw = {c: cir.wire(0, fresh=True) for c in sp}
        cir.sel[m] = (ev, od, spw)
        for c in range(N):
            cir.add(m, c, spw[c] if c in spw else (od if c & 1 else ev), 1)
    return cir.finish()


def selector_witness(cir, a, b):
    """a, b: functions row -> value; must be constant on the even and on the odd ordinary rows"""
    w = list(cir.w)
    N = cir.N
    for m, f in ((0, a), (1, b)):
        ev, od, spw = cir.sel[m]
        ordinary = [c for c in range(min(N, 16)) if c not in spw]
        evs, ods = [c for c in ordinary if not c & 1], [c for c in ordinary if c & 1]
        w[ev] = f(evs[0]) % R if evs else 0
        w[od] = f(ods[0]) % R if ods else 0
        for c, i in spw.items():
            w[i] = f(c) % R
    return w


# name -> N -> (a, b), the value of row c of A and of B
STRUCTURED_WITNESSES = {}
for _i, _x in enumerate(EXTREMAL):
    STRUCTURED_WITNESSES["const[%s]" % EXTREMAL_IDS[_i]] = \
        lambda N, x=_x, y=EXTREMAL[(_i + 3) % len(EXTREMAL)]: (lambda c: x, lambda c: y)
for _name, _at in (("at_0", lambda N: 0), ("at_1", lambda N: 1 % N), ("at_half", lambda N: N // 2), ("at_last", lambda N: N - 1)):
    STRUCTURED_WITNESSES["delta[%s]" % _name] = \
        lambda N, at=_at: (lambda c: R - 1 if c == at(N) else 0, lambda c: ABOVE[0] if c == at(N) else 0)
STRUCTURED_WITNESSES["alternating"] = lambda N: (lambda c: R - 1 if c & 1 else 1, lambda c: 1 if c & 1 else R - 1)


def structured_witness(cir, name):
    return selector_witness(cir, *STRUCTURED_WITNESSES[name](cir.N))


def geometric(N, k):
    """evaluations g^(k i) with g the N-th root: the interpolated polynomial has one non-zero coefficient (x^k).  A carries
    the exponent k, B the exponent N - 1 - k; the values are coefficients of wire 0 on the even rows (single-limb product)
    and of a wide wire on the odd rows (full product)"""
    cir = Circuit(N)
    om = root_of_unity(N.bit_length() - 1)
    kb = (N - 1 - k) % N if N > 2 else 1
    for m, e in ((0, k), (1, kb)):
        step, x = pow(om, e, R), 1
        for c in range(N):
            cir.put(m, c, x, "coef" if c % 2 == 0 else "wide")
            x = x * step % R
    return cir.finish()


def _extremal_evals(N, seed):
    rng = _Rng(seed)
    return [EXTREMAL[rng.below(len(EXTREMAL))] for _ in range(N)]


def squares(N):
    cir = Circuit(N)
    for c, x in enumerate(_extremal_evals(N, 11)):
        cir.put(0, c, x, "wire")
        cir.put(1, c, x, "wire")
    return cir.finish()


def negated(N):
    cir = Circuit(N)
    for c, x in enumerate(_extremal_evals(N, 12)):
        cir.put(0, c, x, "wire")
        cir.put(1, c, (R - x) % R, "wire")
    return cir.finish()


STRUCTURED_KEYS = {
    "geometric[1]": lambda N: geometric(N, 1 % N),
    "geometric[N/2-1]": lambda N: geometric(N, (N // 2 - 1) % N),
    "geometric[N-1]": lambda N: geometric(N, N - 1),
    "squares": squares,
    "a_equals_minus_b": negated,
}


# ------------------------------------------------------------------- representatives above r at the chain's first butterflies
def above_r(N, which):
    """which in "a", "b", "both", "c".  The inverse transforms read the SpMV's output in place, rows at their bit-reversed
    positions.  Even first-pass stage count: quads of positions 4q .. 4q+3 with the first two rows empty (stored as 0) and
    the third and fourth stored >= r -- the twiddle-free opening double stage then forms (x0 + x1) - (x2 + x3) + 4r (the
    historical defect: + 2r went negative).  Odd count (N = 2, 8, 32): the opening stage is the single radix-2 one; pairs of
    positions 2p, 2p+1 with a small first and a second stored >= r.  "c": a and b at the third and fourth position are
    chosen so that their PRODUCT (k_mul stores frmul9's result as it is) is >= r.  The remaining rows carry extremal values."""
    logn = N.bit_length() - 1
    cir = Circuit(N)
    odd = first_pass_stages(logn) & 1
    group = 2 if odd else 4
    n_groups = N // group
    picks = sorted({0, n_groups // 3, n_groups - 1, (n_groups // 2) | 1 if n_groups > 2 else 0} & set(range(n_groups)))
    mats = {"a": (0,), "b": (1,), "both": (0, 1), "c": (0, 1)}[which]
    n_hi = len(picks) * (1 if odd else 2)
    wide = above_r_wires(n_hi + 1)
    used = set()
    targets = {m: [] for m in mats}
    if which == "c":
        rng = _Rng(99)
        prods = []
        while len(prods) < n_hi:
            x, y = R - 1 - (rng.next() << 64 | rng.next()), R - 1 - (rng.next() << 64 | rng.next())
            ra, rb = fred9(term9(1, x)), fred9(term9(1, y))
            if mont9(ra, rb) >= R:
                prods.append((x, y))
    k = 0
    for q in picks:
        pos = [brev(group * q + j, logn) for j in range(group)]
        used.update(pos)
        lo, hi = (pos[:1], pos[1:]) if odd else (pos[:2], pos[2:])
        for j, c in enumerate(lo):
            if odd and j == 0 and q:                      # "small": 0 (row left empty), or 1 / 2 in a narrow wire
                for m in mats:
                    cir.put(m, c, q % 3, "wire")
        for c in hi:
            for m in mats:
                if which == "c":
                    cir.put(m, c, prods[k][m], "wire")
                else:
                    cir.put(m, c, wide[k], "wire")
                targets[m].append((0 if m == 0 else N) + c)
            k += 1
    cir.targets = {"above_r_rows": targets, "odd": odd, "hi_positions": k}
    rng = _Rng(7 + logn)
    for c in range(N):
        for m in (0, 1):
            if c in used and m in mats:
                continue
            # the polynomial that is not aimed at is non-zero on the quads' rows: the other one's transform then shows in h
            if c in used or rng.below(4):
                cir.put(m, c, EXTREMAL[1 + rng.below(len(EXTREMAL) - 1)], "wire")
    return cir.finish()


ABOVE_R_KINDS = ("a", "b", "both", "c")


# ---------------------------------------------------------------------------------------------------- extremal mix sweep
def extremal_mix(seed):
    """a small circuit whose every coefficient and wire value comes from the extremal set; row lengths from the set below"""
    rng = _Rng(1000 + seed)
    N = 1 << (1 + rng.below(12))
    cir = Circuit(N)
    for x in EXTREMAL:
        cir.wire(x)
    for x in EXTREMAL[:6]:
        cir.wire(x, fresh=True)
    budget = 200 + rng.below(400)
    lens = (1, 2, 3, 63, 64, 65, 200)
    while budget > 0:
        ln = lens[rng.below(len(lens))]
        m, c = rng.below(2), rng.below(N)
        for _ in range(ln):
            cir.add(m, c, rng.below(cir.n_vars), EXTREMAL[rng.below(len(EXTREMAL))])
        budget -= ln
    return cir.finish()


N_MIX = 40
SIZES_STRUCTURED = (2, 4, 8, 1 << 5, 1 << 10, 1 << 11, 1 << 12, 1 << 14, 1 << 17)
SIZES_OTHER = (64, 1 << 12)
