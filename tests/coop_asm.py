"""Programs for the wave-cooperative verifier's interpreter (k_verify_coop, csrc/verify.hip), written by hand.

Three things live here:
  * an ASSEMBLER: a list of steps as plain tuples -> (step_class, words, terms) exactly as coop_compile (verify_script.h)
    encodes them -- word fields, the lanes of a linear group, padding to whole trips -- and the decoder back;
  * a REFERENCE: a big-integer interpreter on residues mod p.  It shares nothing with coop_run_host: MUL is a b / R',
    LIN is sum cf v, INV is R'^2 / x (0 for x = 0), inputs are m 2^5, outputs raw / 2^5 (R' = 2^261, m = x 2^256);
  * a MODEL of the device's linear step (accumulators, top_est, q, carries), transcribed line by line from verify.hip.  It
    is used to CHOOSE operands that sit on the step's edges and to state its invariants; expected values always come from
    the reference.

A step is one of
    ("mul", [(dst, a, b), ...])                      up to 64 lanes
    ("inv", [(dst, a), ...])                         up to 64 lanes
    ("lin", [(dst, [(cf, slot), ...]), ...])         up to 20 groups (None leaves a group idle); an optional third element
                                                     {"gap": k} puts k unused term words in front of every group's term list
"""
from fractions import Fraction

import numpy as np

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
RP = 1 << 261                       # the Montgomery radix of the radix-2^29 field (bn254_fq9.h)
MASK = (1 << 29) - 1
CS_MUL, CS_LIN, CS_INV = 1, 2, 3
TRIP = 8                            # COOP_TRIP
MAX_TERMS = 16                      # COOP_MAX_TERMS
MAX_COEF = 1 << 12                  # COOP_MAX_COEF
LIN_GROUPS = 20
OPERAND_BOUND = 5                   # a linear step's operands are below 5p (what the validator asks of a constant)
VALID = 1 << 63

P9 = [(P >> (29 * i)) & MASK for i in range(8)] + [P >> 232]
ONE9 = None                         # set below


def to_limbs(v):
    """The normalised 9-limb form of a non-negative integer below 2^261: limbs 0..7 below 2^29, the top limb keeps the rest."""
    assert 0 <= v < (1 << 261)
    return [(v >> (29 * i)) & MASK for i in range(8)] + [v >> 232]


def from_limbs(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


ONE9 = to_limbs(RP % P)


def group_lane(k):
    """First of the three lanes of linear group k: five groups per 16-lane row, lane 15 of every row idle."""
    return 16 * (k // 5) + 3 * (k % 5)


class Program:
    def __init__(self, step_class, words, terms, n_const, n_slots, out_slot):
        self.step_class = np.ascontiguousarray(step_class, dtype=np.uint8)
        self.words = np.ascontiguousarray(words, dtype=np.uint64)
        self.terms = np.ascontiguousarray(terms, dtype=np.uint32)
        self.n_const, self.n_slots, self.out_slot = int(n_const), int(n_slots), [int(s) for s in out_slot]
        assert self.words.size == 64 * self.step_class.size and len(self.out_slot) == 12

    @property
    def in_base(self):
        return self.n_const

    def copy(self):
        return Program(self.step_class.copy(), self.words.copy(), self.terms.copy(), self.n_const, self.n_slots, list(self.out_slot))


def term_word(cf, slot):
    assert -32768 <= cf < 32768 and 0 <= slot < (1 << 16)
    return ((cf & 0xffff) << 16) | slot


def assemble(steps, n_const, n_slots, out_slot):
    cls, words, terms = [], [], []
    for st in steps:
        kind, ops = st[0], st[1]
        opt = st[2] if len(st) > 2 else {}
        w = [0] * 64
        if kind == "mul":
            assert 1 <= len(ops) <= 64
            for lane, (dst, a, b) in enumerate(ops):
                w[lane] = VALID | dst | (a << 14) | (b << 28)
            cls.append(CS_MUL)
        elif kind == "inv":
            assert 1 <= len(ops) <= 64
            for lane, (dst, a) in enumerate(ops):
                w[lane] = VALID | dst | (a << 14)
            cls.append(CS_INV)
        elif kind == "lin":
            assert 1 <= len(ops) <= LIN_GROUPS
            for k, op in enumerate(ops):
                if op is None:                 # this group stays idle
                    continue
                dst, comb = op
                assert int(opt.get("gap", 0)) % TRIP == 0          # (term lists start on trip boundaries)
                terms.extend([0] * int(opt.get("gap", 0)))
                word = VALID | dst | (len(comb) << 14) | (len(terms) << 20)
                terms.extend(term_word(cf, s) for cf, s in comb)
                terms.extend([0] * (-len(comb) % TRIP))    # whole trips of its own: 0 x slot 0
                l0 = group_lane(k)
                w[l0] = w[l0 + 1] = w[l0 + 2] = word
            cls.append(CS_LIN)
        else:
            raise ValueError(kind)
        words.extend(w)
    if not terms:
        terms = [0] * TRIP                     # (an empty array has no address to pass)
    return Program(cls, words, terms, n_const, n_slots, out_slot)


def decode(step_class, words, terms):
    """The arrays of a program back to the list of steps (gaps are not reconstructed: they carry no meaning)."""
    steps = []
    words = [int(x) for x in np.asarray(words).reshape(-1)]
    terms = [int(x) for x in np.asarray(terms).reshape(-1)]
    for s, c in enumerate(int(x) for x in np.asarray(step_class).reshape(-1)):
        w = words[64 * s:64 * s + 64]
        ops = []
        if c == CS_LIN:
            for k in range(LIN_GROUPS):
                x = w[group_lane(k)]
                if not x >> 63:
                    continue
                assert w[group_lane(k) + 1] == x and w[group_lane(k) + 2] == x
                nt, t0 = (x >> 14) & 0x3f, (x >> 20) & 0xffffff
                comb = []
                for tw in terms[t0:t0 + nt]:
                    cf = tw >> 16
                    comb.append((cf - 65536 if cf >= 32768 else cf, tw & 0xffff))
                ops.append((x & 0x3fff, comb))
            steps.append(("lin", ops))
        else:
            for x in w:
                if not x >> 63:
                    continue
                if c == CS_MUL:
                    ops.append((x & 0x3fff, (x >> 14) & 0x3fff, (x >> 28) & 0x3fff))
                else:
                    ops.append((x & 0x3fff, (x >> 14) & 0x3fff))
            steps.append(("mul" if c == CS_MUL else "inv", ops))
    return steps


# ------------------------------------------------------------------------------------------------ the reference
RP_INV = pow(RP, -1, P)
RP2 = RP * RP % P
IN_SCALE = 1 << 5                   # canonical Montgomery m = x 2^256 -> x 2^261
OUT_SCALE = pow(1 << 5, -1, P)


def run_reference(steps, consts, inputs, n_slots, out_slot):
    """consts: the residues (or any representatives) of the constant slots; inputs: 12 canonical Montgomery values (ints).
    Returns the 12 output values as canonical Montgomery ints.  All lanes of a step read before any lane writes."""
    n_const = len(consts)
    slots = [0] * n_slots
    for i, c in enumerate(consts):
        slots[i] = int(c) % P
    for i, m in enumerate(inputs):
        slots[n_const + i] = int(m) * IN_SCALE % P
    for st in steps:
        kind, ops = st[0], st[1]
        if kind == "mul":
            res = [(dst, slots[a] * slots[b] * RP_INV % P) for dst, a, b in ops]
        elif kind == "inv":
            res = [(dst, RP2 * pow(slots[a], -1, P) % P if slots[a] else 0) for dst, a in ops]
        else:
            res = [(op[0], sum(cf * slots[s] for cf, s in op[1]) % P) for op in ops if op is not None]
        for dst, v in res:
            slots[dst] = v
    return [slots[s] * OUT_SCALE % P for s in out_slot]


def out_bytes(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


# ------------------------------------------------------------------------------------------------ the linear step's model
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
# The bound of a linear step's result, derived in tests/cpp/coop_bounds_check.cpp's header: with t = top_est,
#   R / 2^232 < t + 1 + 2^-13 - 3171407 q + q d,   t - 3171407 q <= 3 * 3171407 + t 1332355 / 2^44 + 2049,   d = 3171407 - p / 2^232 < 1,
#   q <= t 5547123 / 2^44,   t <= (2^15 + pos) p / 2^232 + 2^-16,   pos <= COOP_MAX_COEF * 5
D_NUM, D_DEN = (3171407 << 232) - P, 1 << 232          # d, exactly


def lin_result_bound(pos_in_p):
    """Upper bound, as a multiple of p (a Fraction), of a linear step's result whose positive part is below pos_in_p * p."""
    tmax = ((1 << 15) + pos_in_p) * P // (1 << 232) + 1
    qmax = tmax * 5547123 >> 44
    r = Fraction(3 * 3171407 + (tmax * 1332355 >> 44) + 1 + 2049 + 2) + qmax * Fraction(D_NUM, D_DEN)
    return r * (1 << 232) / P


LIN_RESULT_BOUND = lin_result_bound(MAX_COEF * OPERAND_BOUND)   # 3.0146...: what "below 5p" stands for


class LinTrace:
    pass


def lin_model(comb):
    """comb: [(cf, limbs[9]), ...].  Runs the device's linear step on integers and records what it passes through."""
    tr = LinTrace()
    tr.overflow = False

    def chk(x):
        if not I64_MIN <= x <= I64_MAX:
            tr.overflow = True
        return x

    a = [chk(P9[k] << 15) for k in range(9)]
    padded = list(comb) + [(0, [0] * 9)] * (-len(comb) % TRIP)
    for cf, lim in padded:
        for k in range(9):
            a[k] = chk(a[k] + chk(cf * int(lim[k])))
    tr.acc = list(a)
    top_est = chk(a[8] + (a[7] >> 29))             # lane g = 2: a3[2] + (a3[1] >> 29), then taken as uint64
    tr.top_est = top_est
    t_u = top_est & ((1 << 64) - 1)
    prod = (t_u >> 11) * 5547123
    if prod >> 64:
        tr.overflow = True
    q = ((prod & ((1 << 64) - 1)) >> 33) - 2
    q = 0 if q < 0 else q
    tr.q = q
    qd = q & 0xffffffff                             # it travels as 32 bits
    a = [chk(a[k] - chk(qd * P9[k])) for k in range(9)]
    tr.acc_q = list(a)
    out, cin, tr.carries = [0] * 9, 0, []
    for g in range(3):
        t = chk(a[3 * g] + cin)
        out[3 * g] = t & MASK
        t = chk(a[3 * g + 1] + (t >> 29))
        out[3 * g + 1] = t & MASK
        t = chk(a[3 * g + 2] + (t >> 29))
        if g < 2:
            out[3 * g + 2] = t & MASK
            cin = t >> 29
            tr.carries.append(cin)
        else:
            tr.top = t                              # stored as uint32
            out[8] = t & 0xffffffff
    tr.out = out
    tr.value = from_limbs(out)
    tr.total = sum(cf * from_limbs(l) for cf, l in comb)
    return tr


# ------------------------------------------------------------------------------------------------ shared test material
def load_dump(path):
    """The final-exponentiation program and its constant slots as tests/cpp/coop_bounds_check.cpp --dump writes them."""
    raw = np.fromfile(path, dtype=np.uint8)
    hd = raw[:64].view(np.uint32)
    n_steps, n_terms, n_const, n_slots = (int(x) for x in hd[:4])
    o = 64
    words = raw[o:o + n_steps * 512].view(np.uint64).copy()
    o += n_steps * 512
    terms = raw[o:o + n_terms * 4].view(np.uint32).copy()
    o += n_terms * 4
    const9 = raw[o:o + n_const * 36].view(np.uint32).copy().reshape(n_const, 9)
    o += n_const * 36
    cls = raw[o:o + n_steps].copy()
    assert o + n_steps == raw.size
    return Program(cls, words, terms, n_const, n_slots, [int(x) for x in hd[4:16]]), const9


def build_dump(root, workdir):
    """Compiles tests/cpp/coop_bounds_check.cpp (host code only) and runs it; returns (its output, path of the dump)."""
    import os
    import subprocess
    exe, dump = os.path.join(str(workdir), "cbc"), os.path.join(str(workdir), "finalexp.bin")
    cc = subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-I", os.path.join(root, "keyless-zk-proofs_amd", "csrc"),
                         os.path.join(root, "tests", "cpp", "coop_bounds_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, "coop_bounds_check.cpp does not compile:\n" + cc.stderr[-4000:]
    out = subprocess.run([exe, "--dump", dump], capture_output=True, text=True, timeout=300)
    return out, dump


CHUNK_BYTES = 24576                 # COOP_CHUNK_BYTES


def chunk_layout(prog):
    """coop_layout's greedy cut of a program into the chunks the loader wave stages (csrc/verify.hip), restated: a list of
    (first step, steps, term base, terms).  A step's terms span from its lowest term offset to the end of its highest padded
    list; a chunk takes consecutive steps while 512 bytes of words per step plus its term span fit CHUNK_BYTES."""
    n_steps = prog.step_class.size
    words = [int(x) for x in prog.words]
    span = []
    for s in range(n_steps):
        lo, hi = None, 0
        if int(prog.step_class[s]) == CS_LIN:
            for w in words[64 * s:64 * s + 64]:
                if w >> 63:
                    nt, t0 = (w >> 14) & 0x3f, (w >> 20) & 0xffffff
                    lo = t0 if lo is None else min(lo, t0)
                    hi = max(hi, t0 + ((nt + TRIP - 1) & ~(TRIP - 1)))
        span.append((lo, hi) if hi else None)
    chunks, s0 = [], 0
    while s0 < n_steps:
        s1, cur = s0, None
        while s1 < n_steps:
            nxt = cur
            if span[s1]:
                nxt = span[s1] if cur is None else (min(cur[0], span[s1][0]), max(cur[1], span[s1][1]))
            if (s1 + 1 - s0) * 512 + (nxt[1] - nxt[0] if nxt else 0) * 4 > CHUNK_BYTES and s1 > s0:
                break
            cur = nxt
            s1 += 1
        chunks.append((s0, s1 - s0, cur[0] if cur else 0, cur[1] - cur[0] if cur else 0))
        s0 = s1
    return chunks


BOUND = OPERAND_BOUND * P           # operands of a linear step are below this
TOP_MAX = (BOUND - 1) >> 232        # the largest admissible top limb
LOW_ONES = (1 << 232) - 1


HI_Q = [(MAX_COEF, TOP_MAX << 232)]                  # the largest quotient of a linear step; every carry negative
LO_Q = [(-MAX_COEF, BOUND - 1)]                      # the smallest quotient; a positive carry


def directed_operands():
    """Representatives below 5p at the edges of the radix-2^29 form."""
    v = [0, 1, P - 1, P, P + 1, 2 * P - 1]
    for k in range(1, OPERAND_BOUND + 1):
        v += [k * P - 1, k * P + 1] if k < OPERAND_BOUND else [k * P - 1]
    tops = [0, 1, P9[8] - 1, P9[8], P9[8] + 1, 2 * P9[8] + 1, 3 * P9[8] + 2, TOP_MAX - 1, TOP_MAX]
    v += [(t << 232) | LOW_ONES for t in tops if t < TOP_MAX]   # all low limbs 2^29 - 1 under the top limb
    v += [t << 232 for t in tops if t]                  # only the top limb set
    v += [MASK << (29 * 7), MASK << (29 * 6), (MASK << (29 * 6)) | (MASK << (29 * 7))]
    assert all(0 <= x < BOUND for x in v)
    return v


def _split(total, n):
    c = [total // n] * n
    c[-1] += total - sum(c)
    return c


def _base_top_est():
    return (P9[8] << 15) + ((P9[7] << 15) >> 29)


def directed_combinations():
    """[(name, [(cf, value), ...])]: the linear step's edges.  The comments name what lin_model shows for each family;
    tests/test_coop_bounds_host.py asserts those properties, so the families cannot silently miss their edge."""
    ops = directed_operands()
    out = []
    for i, v in enumerate(ops):
        out.append(("single +1 #%d" % i, [(1, v)]))
        out.append(("single -1 #%d" % i, [(-1, v)]))
    out.append(("+4096 x (5p - 1)", [(MAX_COEF, BOUND - 1)]))
    out.append(("-4096 x (5p - 1)", [(-MAX_COEF, BOUND - 1)]))
    out.append(("+4096 x top limb only", [(MAX_COEF, TOP_MAX << 232)]))        # limbs 0..7 go negative after the quotient
    out.append(("-4096 x low ones", [(-MAX_COEF, LOW_ONES)]))
    ext = [BOUND - 1, ((TOP_MAX - 1) << 232) | LOW_ONES, TOP_MAX << 232, LOW_ONES, P - 1, 4 * P + 1, 2 * P - 1, MASK << (29 * 7)]
    for n in (1, 7, 8, 9, 15, 16):
        cs = _split(MAX_COEF, n)
        for sign in ("pos", "neg", "alt"):
            comb = []
            for k in range(n):
                s = 1 if sign == "pos" else -1 if sign == "neg" else (1 if k % 2 == 0 else -1)
                comb.append((s * cs[k], ext[(k + n) % len(ext)]))
            out.append(("%d terms %s" % (n, sign), comb))
    # totals on k p and k p +- 1
    out.append(("total 3p", [(1, P), (1, 2 * P)]))
    out.append(("total 0 = p - p", [(1, P), (-1, P)]))
    out.append(("total 4096 p", [(MAX_COEF, P)]))
    out.append(("total 4096 p + 1", [(MAX_COEF - 1, P), (1, P + 1)]))
    out.append(("total 4096 p - 1", [(MAX_COEF - 1, P), (1, P - 1)]))
    out.append(("total -4096 p", [(-MAX_COEF, P)]))
    out.append(("total -4096 p + 1", [(-(MAX_COEF - 1), P), (-1, P - 1)]))
    out.append(("total -20479 p - 1", [(-(MAX_COEF - 1), BOUND - 1), (-1, 4 * P + 4096)]))
    out.append(("total 1", [(2048, 2 * P), (-2047, 2 * P), (-1, 2 * P - 1)]))
    # top_est on multiples of 3171407 and of 2^11, +-1: a top-limb-only operand moves top_est by exactly its top limb
    b0 = _base_top_est()
    for mod in (3171407, 1 << 11):
        for m in (1, 2, 4):
            t0 = -b0 % mod + (m - 1) * mod
            for d in (-1, 0, 1):
                t = t0 + d
                if 0 < t <= TOP_MAX:
                    out.append(("top_est = %d k %+d (#%d)" % (mod, d, m), [(1, t << 232)]))
    # the same with a quotient above 2^15 p's: a large positive part beside the adjusting operand
    big = 4000 * (4 * P9[8])
    for mod in (3171407, 1 << 11):
        t0 = -(b0 + big) % mod + mod
        for d in (-1, 0, 1):
            out.append(("top_est = %d k %+d (large)" % (mod, d), [(4000, (4 * P9[8]) << 232), (1, (t0 + d) << 232)]))
    # limb-6 accumulator negative before the quotient, limb-7 accumulator negative after it, total positive
    out.append(("limb 6 negative", [(-MAX_COEF + 1, MASK << (29 * 6)), (1, TOP_MAX << 232)]))
    out.append(("limb 7 negative after q", [(MAX_COEF - 1, TOP_MAX << 232), (-1, MASK << (29 * 7))]))
    out.append(("limbs 0..7 negative after q", [(2048, TOP_MAX << 232), (2048, (TOP_MAX - 1) << 232)]))
    return out


class Rng:
    """SplitMix64: the same stream everywhere"""

    def __init__(self, seed):
        self.s = seed & ((1 << 64) - 1)

    def next(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & ((1 << 64) - 1)
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & ((1 << 64) - 1)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & ((1 << 64) - 1)
        return z ^ (z >> 31)

    def below(self, n):
        v = 0
        for _ in range((n.bit_length() + 63) // 64 + 1):
            v = (v << 64) | self.next()
        return v % n


def random_combination(rng, n_terms=None, pool=None):
    """A combination at the documented limits: sum |cf| = COOP_MAX_COEF, operands below 5p (extremal ones among them)."""
    n = n_terms or 1 + rng.below(MAX_TERMS)
    cuts = sorted(rng.below(MAX_COEF - n + 1) for _ in range(n - 1))
    mags = [b - a + 1 for a, b in zip([0] + cuts, cuts + [MAX_COEF - n])]
    assert sum(mags) == MAX_COEF and min(mags) >= 1
    comb = []
    for m in mags:
        v = pool[rng.below(len(pool))] if pool and rng.below(3) == 0 else rng.below(BOUND)
        comb.append((m if rng.below(2) else -m, v))
    return comb


def random_program(seed, n_steps=40, n_consts=8, n_temps=48, max_lanes=14):
    """A legal program: every value stays below 5p (MUL results < 2p, LIN results < 3.02p, INV results < 2p), so any defined
    slot may feed any operation.  Destinations are drawn among ALL temporaries, defined or not: slots are reused freely, a
    destination may be an operand of its own or of a neighbouring lane.  Returns (steps, consts, n_slots, out_slot)."""
    rng = Rng(seed)
    pool = directed_operands()
    consts = [0, RP % P] + [pool[rng.below(len(pool))] if rng.below(2) else rng.below(BOUND) for _ in range(n_consts - 2)]
    first = n_consts + 12
    temps = list(range(first, first + n_temps))
    defined = list(range(n_consts + 12))
    steps = []

    def pick_dsts(k):
        t = list(temps)
        res = []
        for _ in range(k):
            res.append(t.pop(rng.below(len(t))))
        return res

    for s in range(n_steps):
        r = rng.below(20)
        if s == 0:
            dsts = temps[:16]
            ops = [(d, defined[rng.below(len(defined))], defined[rng.below(len(defined))]) for d in dsts]
            steps.append(("mul", ops))
        elif r < 9:
            dsts = pick_dsts(1 + rng.below(max_lanes))
            steps.append(("mul", [(d, defined[rng.below(len(defined))], defined[rng.below(len(defined))]) for d in dsts]))
        elif r < 18:
            dsts = pick_dsts(1 + rng.below(min(max_lanes, LIN_GROUPS)))
            ops = []
            for d in dsts:
                comb = random_combination(rng, 1 + rng.below(MAX_TERMS))
                ops.append((d, [(cf, defined[rng.below(len(defined))]) for cf, _ in comb]))
            steps.append(("lin", ops))
        else:
            dsts = pick_dsts(1 + rng.below(2))
            steps.append(("inv", [(d, defined[rng.below(len(defined))]) for d in dsts]))
        for d in dsts:
            if d not in defined:
                defined.append(d)
    written = [d for d in defined if d >= first]
    out_slot = [written[rng.below(len(written))] for _ in range(12)]
    return steps, consts, first + n_temps, out_slot
