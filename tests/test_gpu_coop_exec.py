"""-m gpu : the wave-cooperative verifier's interpreter (k_verify_coop, csrc/verify.hip) on DIRECTED programs, through
k16_coop_exec -- the production kernel instantiation of the fold, a caller's program.  Programs come from the assembler of
tests/coop_asm.py; every expected value comes from its big-integer reference (residues mod p), compared byte for byte on
all 12 x 32 output bytes of every block.  The integer model of the linear step only chooses operands."""
import os
import time

import numpy as np
import pytest

import coop_asm as ca
import oracle_lib as ol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ca.P
ONE_M = (1 << 256) % P                        # the canonical Montgomery one


@pytest.fixture(scope="module")
def ctx():
    import k16
    c = k16.Context(0)
    t0 = time.time()
    yield c
    print("\n[test_gpu_coop_exec: %.1f s]" % (time.time() - t0))
    c.close()


def _const9(consts):
    return np.array([ca.to_limbs(int(c)) for c in consts], dtype=np.uint32)


def _inputs_bytes(inputs):
    return np.frombuffer(b"".join(ca.out_bytes(row) for row in inputs), dtype=np.uint8).reshape(len(inputs), 12, 32)


def _exec(ctx, prog, const9, inputs):
    return ctx.coop_exec(prog.step_class, prog.words, prog.terms, prog.n_const, prog.n_slots, prog.out_slot, const9, _inputs_bytes(inputs))


def _check(ctx, steps, consts, n_slots, out_slot, inputs=None, what=""):
    """Runs the program on the GPU for every row of inputs and compares with the reference."""
    inputs = inputs or [[0] * 12]
    prog = ca.assemble(steps, len(consts), n_slots, out_slot)
    got = _exec(ctx, prog, _const9(consts), inputs)
    for i, row in enumerate(inputs):
        want = ca.out_bytes(ca.run_reference(steps, consts, row, n_slots, out_slot))
        assert got[i].tobytes() == want, "%s: block %d" % (what, i)


def _rand_inputs(seed, n):
    rng = ca.Rng(seed)
    edge = [0, 1, P - 1, ONE_M]
    return [[edge[(i + j) % 4] if (i + 3 * j) % 11 == 0 else rng.below(P) for j in range(12)] for i in range(n)]


def _lin_program(cases, places=None):
    """cases: up to 20 combinations [(cf, value), ...]; places[i] = the group case i sits in.  One linear step; returns
    (steps, consts, n_slots, dst slots of the cases)."""
    consts, index = [0, ca.RP % P], {}
    for comb in cases:
        for _, v in comb:
            if v not in index:
                index[v] = len(consts)
                consts.append(v)
    first = len(consts) + 12
    places = places or list(range(len(cases)))
    groups = [None] * (max(places) + 1)
    for i, comb in enumerate(cases):
        groups[places[i]] = (first + i, [(cf, index[v]) for cf, v in comb])
    return [("lin", groups)], consts, first + len(cases), [first + i for i in range(len(cases))]


# ------------------------------------------------------------------------------------------------ LIN on directed values
def test_lin_on_directed_values(ctx):
    cases = ca.directed_combinations()
    assert len(cases) > 120
    for k in range(0, len(cases), 12):
        pack = cases[k:k + 12]
        while len(pack) < 12:
            pack.append(cases[len(pack)])
        # the pack's first group moves through the rows: 0, 3, 6 (groups 3..14 cross two row boundaries) ...
        g0 = (k // 12 * 3) % 9
        steps, consts, n_slots, dsts = _lin_program([c for _, c in pack], places=[g0 + i for i in range(12)])
        _check(ctx, steps, consts, n_slots, dsts, what="pack %d (%s ...)" % (k // 12, pack[0][0]))


@pytest.mark.parametrize("seed", [5, 6])
def test_lin_on_random_combinations_at_the_limits(ctx, seed):
    rng = ca.Rng(seed)
    pool = ca.directed_operands()
    for n in (1, 7, 8, 9, 15, 16):
        for _ in range(3):
            cases = [ca.random_combination(rng, n, pool) for _ in range(12)]
            steps, consts, n_slots, dsts = _lin_program(cases)
            _check(ctx, steps, consts, n_slots, dsts, what="%d terms" % n)


# ------------------------------------------------------------------------------------------------ neighbouring groups
HI_Q, LO_Q = ca.HI_Q, ca.LO_Q       # the largest quotient, every carry negative | the smallest, a positive carry
MID = [(1, P + 1), (-1, (ca.MASK << (29 * 6)) | (ca.MASK << (29 * 7)))]


@pytest.mark.parametrize("flip", [0, 1])
def test_all_twenty_groups_with_opposite_neighbours(ctx, flip):
    cases = [(HI_Q if (k + flip) % 2 == 0 else LO_Q) if k % 5 != 2 else MID for k in range(20)]
    steps, consts, n_slots, dsts = _lin_program(cases)
    _check(ctx, steps, consts, n_slots, dsts[:12], what="groups 0..11")
    _check(ctx, steps, consts, n_slots, dsts[8:], what="groups 8..19")


@pytest.mark.parametrize("places", [[0], [4], [5], [19], [4, 5], [9, 10], [14, 15], [0, 19]])
def test_one_or_two_groups_alone_in_a_step(ctx, places):
    for a, b in ((HI_Q, LO_Q), (LO_Q, HI_Q)):
        cases = [a, b][:len(places)]
        steps, consts, n_slots, dsts = _lin_program(cases, places=places)
        _check(ctx, steps, consts, n_slots, (dsts * 12)[:12], what=str(places))


# ------------------------------------------------------------------------------------------------ what follows a LIN
def _top_of_bound(count):
    """The directed combinations whose results are the largest, by the model (close to 3.01 p)."""
    scored = []
    for name, comb in ca.directed_combinations():
        tr = ca.lin_model([(cf, ca.to_limbs(v)) for cf, v in comb])
        scored.append((tr.value, name, comb))
    scored.sort(key=lambda x: -x[0])
    assert scored[0][0] > 3 * P
    return [c for _, _, c in scored[:count]]


def test_lin_results_at_the_top_of_their_bound_feed_every_class(ctx):
    tops = _top_of_bound(6)
    steps, consts, n_slots, l = _lin_program(tops)
    t = n_slots                                              # further temporaries
    n_slots += 40
    # MUL: lin x lin, and squarings MUL(a, a)
    steps.append(("mul", [(t + 0, l[0], l[1]), (t + 1, l[2], l[3]), (t + 2, l[4], l[5]), (t + 3, l[0], l[0]), (t + 4, l[5], l[5]),
                          (t + 5, l[1], l[1])]))
    # LIN of LIN results as atoms, sum |cf| = 4096
    steps.append(("lin", [(t + 6, [(ca.MAX_COEF, l[0])]), (t + 7, [(-ca.MAX_COEF, l[0])]),
                          (t + 8, [(1024, l[0]), (-1024, l[1]), (1024, l[2]), (-1024, l[3])]),
                          (t + 9, [(683, l[k]) for k in range(5)] + [(681, l[5])]),
                          (t + 10, [(-683, l[k]) for k in range(5)] + [(-681, l[5])])]))
    # INV
    steps.append(("inv", [(t + 11, l[0]), (t + 12, l[3])]))
    _check(ctx, steps, consts, n_slots, [t + k for k in range(12)], what="mul / lin")
    _check(ctx, steps, consts, n_slots, [t + 11, t + 12] + l + [t + 6, t + 7, t + 8, t + 9], what="inv / the results themselves")
    # and once more through a second level: the linear results of linear results into products and an inversion
    steps.append(("mul", [(t + 13, t + 6, t + 7), (t + 14, t + 9, t + 9), (t + 15, t + 10, t + 8)]))
    steps.append(("inv", [(t + 16, t + 9)]))
    _check(ctx, steps, consts, n_slots, [t + 13, t + 14, t + 15, t + 16] * 3, what="second level")


def test_inversions(ctx):
    rnd = ca.Rng(77).below(P)
    consts = [0, ca.RP % P, P - 1, rnd, P, 2 * P, 4 * P + 1, 3 * P - 1, rnd + 3 * P]
    first = len(consts) + 12
    steps = [("inv", [(first + k, 1 + k) for k in range(8)] + [(first + 8, len(consts) + k) for k in range(0, 1)]),
             ("inv", [(first + 9, first + 2)]),              # the inverse of an inverse
             ("mul", [(first + 10, first + 2, 3), (first + 11, first + 5, 6)])]   # x^-1 x
    inputs = _rand_inputs(3, 3) + [[0] * 12, [P - 1] * 12]
    _check(ctx, steps, consts, first + 12, [first + k for k in range(12)], inputs, what="inversions")
    # zero's representatives invert to zero: checked against plain zeros too
    prog = ca.assemble(steps, len(consts), first + 12, [first + k for k in range(12)])
    got = _exec(ctx, prog, _const9(consts), [[0] * 12])
    assert got[0, 3].tobytes() == bytes(32) and got[0, 4].tobytes() == bytes(32) and got[0, 8].tobytes() == bytes(32)


def test_mul_steps_with_64_lanes_and_with_one(ctx):
    pool = ca.directed_operands()
    consts = [0, ca.RP % P] + [pool[k] for k in range(2, len(pool), 2)][:18]
    nc = len(consts)
    first = nc + 12
    src = list(range(1, nc + 12))
    steps = [("mul", [(first + k, src[k % len(src)], src[(7 * k + 3) % len(src)]) for k in range(64)]),
             ("mul", [(first + 64, first + 63, first + 0)])]
    # every one of the 65 products reaches an output: 12 sums with distinct coefficients
    groups = []
    for o in range(12):
        members = [first + k for k in range(65) if k % 12 == o]
        groups.append((first + 65 + o, [(3 * i + 1 if i % 2 else -(5 * i + 2), s) for i, s in enumerate(members)]))
    steps.append(("lin", groups))
    _check(ctx, steps, consts, first + 77, [first + 65 + o for o in range(12)], _rand_inputs(8, 4), what="64 lanes")


# ------------------------------------------------------------------------------------------------ plumbing
def _chain_program(n_steps):
    """12 values updated IN PLACE step after step: every destination is one of its operation's own operands, and every
    lane reads its neighbour's old value in the step that overwrites it (slot reuse in the step of the last read).
    110 consecutive MUL / INV steps hold a whole chunk without terms (a chunk takes 48 such steps, wherever the cut before it
    falls); linear steps with gaps spread term lists over a chunk."""
    consts = [0, ca.RP % P, P - 1, 3 * P + 5, ca.BOUND - 1, (ca.TOP_MAX - 1) << 232 | ca.LOW_ONES]
    nc = len(consts)
    x = [nc + 12 + k for k in range(12)]
    steps = [("lin", [(x[k], [(1, nc + k), (k + 1, 2 + k % 4)]) for k in range(12)])]
    for s in range(n_steps):
        if s % 40 == 39:
            steps.append(("inv", [(x[k], x[k]) for k in range(0, 12, 5)]))
        elif 20 <= s < 130 or s % 2 == 0:
            steps.append(("mul", [(x[k], x[k], x[(k + 1 + s) % 12]) for k in range(12)]))
        else:
            ops = []
            for k in range(12):
                n = (1, 7, 8, 9, 15, 16)[(s + k) % 6]
                cs = ca._split(ca.MAX_COEF - 16 * (k % 3), n)
                ops.append((x[k], [((-c if (i + k) % 3 == 0 else c), x[(k + i) % 12] if i < 12 else 2 + i % 4) for i, c in enumerate(cs)]))
            steps.append(("lin", ops, {"gap": 304 if s % 16 == 5 else 0}))
    return steps, consts, nc + 24, x


def test_long_dependent_chain_over_several_chunks_and_many_blocks(ctx):
    steps, consts, n_slots, x = _chain_program(230)
    kinds = [s[0] for s in steps]
    assert len(steps) > 150 and kinds.count("inv") >= 2 and kinds.count("lin") > 40
    # the chunks as the loader wave will stage them: several, one without any term, one whose term lists lie far apart
    chunks = ca.chunk_layout(ca.assemble(steps, len(consts), n_slots, x))
    assert len(chunks) >= 3 and sum(c[1] for c in chunks) == len(steps)
    free = [c for c in chunks if c[3] == 0]
    assert free and all("lin" not in kinds[c[0]:c[0] + c[1]] for c in free) and any("inv" in kinds[c[0]:c[0] + c[1]] for c in free)
    assert any(c[3] > 12 * 304 and c[1] > 1 for c in chunks)
    _check(ctx, steps, consts, n_slots, x, _rand_inputs(21, 72), what="chain")


def test_slot_reuse_in_the_step_of_the_last_read(ctx):
    consts = [0, ca.RP % P, 2 * P + 7, P - 2]
    nc = len(consts)
    t = nc + 12
    steps = [("mul", [(t + k, nc + k, nc + (k + 1) % 12) for k in range(12)]),
             # MUL: dst = own operand a, own operand b, both (a squaring); lane k reads what lane k + 1 overwrites
             ("mul", [(t + 0, t + 0, t + 1), (t + 1, t + 2, t + 1), (t + 2, t + 2, t + 2), (t + 3, t + 0, t + 2)]),
             # LIN: dst among its own terms; a swap through two groups; a value every group reads while group 0 overwrites it
             ("lin", [(t + 4, [(3, t + 4), (-2, t + 5)]), (t + 5, [(1, t + 4)]), (t + 6, [(-1, t + 6)]), (t + 7, [(7, t + 4), (1, t + 7)])]),
             # INV: in place, and into the slot a neighbour inverts
             ("inv", [(t + 8, t + 8), (t + 9, t + 8), (t + 10, t + 9)]),
             # a slot written by each class is read again and overwritten by each other class
             ("lin", [(t + 8, [(2, t + 0), (1, t + 8)]), (t + 0, [(1, t + 9), (-1, t + 0)])]),
             ("mul", [(t + 4, t + 8, t + 4), (t + 9, t + 4, t + 10)]),
             ("inv", [(t + 5, t + 4), (t + 4, t + 5)])]
    _check(ctx, steps, consts, t + 12, [t + k for k in range(12)], _rand_inputs(31, 5), what="reuse")


# ------------------------------------------------------------------------------------------------ random sweep
@pytest.mark.parametrize("seed", [101, 102, 103])
def test_random_legal_programs(ctx, seed):
    steps, consts, n_slots, out_slot = ca.random_program(seed)
    assert len(steps) == 40 and {s[0] for s in steps} == {"mul", "lin", "inv"}
    _check(ctx, steps, consts, n_slots, out_slot, _rand_inputs(seed, 2000), what="seed %d" % seed)


# ------------------------------------------------------------------------------------------------ the real program
@pytest.fixture(scope="module")
def finalexp(tmp_path_factory):
    out, dump = ca.build_dump(ROOT, tmp_path_factory.mktemp("cbc"))
    assert out.returncode == 0, out.stdout + out.stderr
    return ca.load_dump(dump)


def test_real_final_exponentiation_program(ctx, finalexp):
    prog, const9 = finalexp
    rng = ca.Rng(4242)
    f = [[rng.below(P) for _ in range(12)] for _ in range(20)]
    f.append([ONE_M] + [0] * 11)
    f.append([P - ONE_M] + [0] * 11)
    for k in range(12):
        f.append([(rng.below(P - 1) + 1) if j == k else 0 for j in range(12)])
    f.append([P - 1] * 12)
    got = _exec(ctx, prog, const9, f)
    for i, row in enumerate(f):
        assert got[i].tobytes() == ol.final_exp(ca.out_bytes(row)), "input %d" % i
    assert got[20].tobytes() == ca.out_bytes([ONE_M] + [0] * 11)


# ------------------------------------------------------------------------------------------------ refusals
def _base():
    consts = [0, ca.RP % P, 5, P + 9]
    t = len(consts) + 12
    steps = [("mul", [(t + k, 4 + k, 2 + k % 2) for k in range(12)]),
             ("lin", [(t + 12 + k, [(2, t + k), (-1, 3), (5, t + (k + 1) % 12)]) for k in range(6)]),
             ("inv", [(t + 18, t + 12)])]
    out_slot = [t + 12, t + 13, t + 14, t + 15, t + 16, t + 17, t + 18, t + 0, t + 1, t + 2, t + 3, t + 4]
    return steps, consts, t + 19, out_slot


def _mutations():
    """(name, function(prog, const9, kw) mutating a valid call, fragment of the expected message)"""
    V, L0 = ca.VALID, 64                                     # the linear step is step 1: its words start at 64
    muts = []

    def m(name, frag):
        def deco(fn):
            muts.append((name, fn, frag))
            return fn
        return deco

    @m("class 0", "unknown class")
    def _(p, c, kw): p.step_class[0] = 0

    @m("class 4", "unknown class")
    def _(p, c, kw): p.step_class[2] = 4

    @m("one constant", "inputs follow the constants")
    def _(p, c, kw): kw["n_const"] = 1; kw["const9"] = c[:1]

    @m("slot 0 not zero", "slot 0 must hold 0")
    def _(p, c, kw): c[0, 0] = 1

    @m("slot 1 not one", "slot 0 must hold 0")
    def _(p, c, kw): c[1, 3] ^= 1

    @m("too many slots", "14 bits")
    def _(p, c, kw): p.n_slots = 1 << 14

    @m("slot file larger than LDS", "bytes of LDS")
    def _(p, c, kw): p.n_slots = 6000

    @m("slot file ends inside the inputs", "ends inside the input slots")
    def _(p, c, kw): p.n_slots = p.n_const + 11

    @m("no steps", "steps, 1 ..")
    def _(p, c, kw): kw["n_steps"] = 0

    @m("2^20 steps", "steps, 1 ..")
    def _(p, c, kw): kw["n_steps"] = 1 << 20

    @m("empty term array", "2^24 - 1 terms")
    def _(p, c, kw): kw["n_terms"] = 0

    @m("2^24 terms", "2^24 - 1 terms")
    def _(p, c, kw): kw["n_terms"] = 1 << 24

    @m("no words", "null argument")
    def _(p, c, kw): kw["null"] = "words"

    @m("no constants", "null argument")
    def _(p, c, kw): kw["null"] = "const9"

    @m("no output buffer", "null argument")
    def _(p, c, kw): kw["null"] = "out"

    @m("no input set", "input sets")
    def _(p, c, kw): kw["n"] = 0

    @m("too many input sets", "input sets")
    def _(p, c, kw): kw["n"] = (1 << 16) + 1

    @m("MUL operand a", "MUL operand outside")
    def _(p, c, kw): p.words[0] = (int(p.words[0]) & ~(0x3fff << 14)) | (p.n_slots << 14)

    @m("MUL operand b", "MUL operand outside")
    def _(p, c, kw): p.words[1] = (int(p.words[1]) & ~(0x3fff << 28)) | (0x3fff << 28)

    @m("INV operand", "INV operand outside")
    def _(p, c, kw): p.words[128] = (int(p.words[128]) & ~(0x3fff << 14)) | (p.n_slots << 14)

    @m("term slot", "term slot outside")
    def _(p, c, kw): p.terms[1] = (int(p.terms[1]) & 0xffff0000) | p.n_slots

    @m("term slot above 14 bits", "term slot outside")
    def _(p, c, kw): p.terms[0] = (int(p.terms[0]) & 0xffff0000) | 0x8000 | 3

    @m("output slot", "output slot")
    def _(p, c, kw): p.out_slot[11] = p.n_slots

    @m("destination is a constant", "constant or input slot")
    def _(p, c, kw): p.words[2] = (int(p.words[2]) & ~0x3fff) | 3

    @m("destination is an input", "constant or input slot")
    def _(p, c, kw): p.words[128] = (int(p.words[128]) & ~0x3fff) | (p.n_const + 11)

    @m("destination outside", "destination outside")
    def _(p, c, kw): p.words[3] = (int(p.words[3]) & ~0x3fff) | p.n_slots

    @m("two MUL lanes, one slot", "write the same slot")
    def _(p, c, kw): p.words[5] = (int(p.words[5]) & ~0x3fff) | (int(p.words[4]) & 0x3fff)

    @m("two LIN groups, one slot", "write the same slot")
    def _(p, c, kw):
        for g in range(3):
            p.words[L0 + 3 + g] = (int(p.words[L0 + 3 + g]) & ~0x3fff) | (int(p.words[L0]) & 0x3fff)

    @m("LIN word in lane 15", "lane 15")
    def _(p, c, kw): p.words[L0 + 15] = p.words[L0]

    @m("LIN group with two lanes", "same word")
    def _(p, c, kw): p.words[L0 + 2] = 0

    @m("LIN group's lanes differ", "same word")
    def _(p, c, kw): p.words[L0 + 1] = int(p.words[L0 + 1]) ^ (1 << 20)

    @m("LIN group one lane late", "same word")
    def _(p, c, kw): p.words[L0 + 18] = p.words[L0 + 19] = p.words[L0 + 20] = p.words[L0]

    @m("LIN with zero terms", "1 .. 56 terms")
    def _(p, c, kw):
        for g in range(3):
            p.words[L0 + g] = int(p.words[L0 + g]) & ~(0x3f << 14)

    @m("57 terms", "1 .. 56 terms")
    def _(p, c, kw):
        for g in range(3):
            p.words[L0 + g] = (int(p.words[L0 + g]) & ~(0x3f << 14)) | (57 << 14)

    @m("term list past the array", "past the term array")
    def _(p, c, kw):
        for g in range(3):
            p.words[L0 + g] = (int(p.words[L0 + g]) & ~(0xffffff << 20)) | (p.terms.size << 20)

    @m("padding past the array", "past the term array")
    def _(p, c, kw):
        for g in range(3):
            p.words[L0 + g] = (int(p.words[L0 + g]) & ~((0xffffff << 20) | (0x3f << 14))) | ((p.terms.size - 8) << 20) | (9 << 14)

    @m("term list not on a trip boundary", "multiple of COOP_TRIP")
    def _(p, c, kw):
        for g in range(3):
            p.words[L0 + g] = int(p.words[L0 + g]) + (4 << 20)

    @m("padding term not zero", "padding terms")
    def _(p, c, kw): p.terms[7] = 1 << 16

    @m("coefficients sum to 4097", "COOP_MAX_COEF")
    def _(p, c, kw): p.terms[0] = ca.term_word(4091, int(p.terms[0]) & 0xffff)

    @m("coefficient -32768", "COOP_MAX_COEF")
    def _(p, c, kw): p.terms[8] = ca.term_word(-32768, 2)

    @m("constant limb of 2^29", "not below 2^29")
    def _(p, c, kw): c[2, 4] = 1 << 29

    @m("constant 5p", "not below 5p")
    def _(p, c, kw): c[3] = ca.to_limbs(5 * P)

    return muts


@pytest.mark.parametrize("which", range(len(_mutations())), ids=[m[0].replace(" ", "_") for m in _mutations()])
def test_refusals(ctx, which):
    import k16
    name, fn, frag = _mutations()[which]
    steps, consts, n_slots, out_slot = _base()
    inputs = _rand_inputs(9, 2)
    good = ca.assemble(steps, len(consts), n_slots, out_slot)
    want = [ca.out_bytes(ca.run_reference(steps, consts, row, n_slots, out_slot)) for row in inputs]
    prog, c9, kw = good.copy(), _const9(consts), {}
    fn(prog, c9, kw)
    inp = _inputs_bytes(inputs)
    n = kw.get("n", len(inputs))
    if n != len(inputs):
        inp = np.zeros((max(n, 1), 12, 32), dtype=np.uint8)
    L = ctx.L
    sc, w, t = prog.step_class, prog.words, prog.terms
    c9 = np.ascontiguousarray(kw.get("const9", c9), dtype=np.uint32)
    osl = np.array(prog.out_slot, dtype=np.uint32)
    out = np.zeros_like(inp)
    ptr = {"sc": sc, "words": w, "terms": t, "osl": osl, "const9": c9, "inp": inp, "out": out}
    ptr = {k: None if kw.get("null") == k else k16._p(v) for k, v in ptr.items()}
    # (the counts are checked before any array is read: the refused calls with wrong counts touch nothing)
    rc = L.k16_coop_exec(ctx.h, ptr["sc"], kw.get("n_steps", sc.size), ptr["words"], ptr["terms"], kw.get("n_terms", t.size),
                         kw.get("n_const", prog.n_const), prog.n_slots, ptr["osl"], ptr["const9"], ptr["inp"], n, ptr["out"])
    msg = (L.k16_last_error(ctx.h) or b"").decode()
    assert rc == -3, (name, rc, msg)                         # K16_ERR_ARG
    assert "k16_coop_exec" in msg and frag in msg, (name, msg)
    assert not out.any()
    # the context still works, and the unmutated program gives the right values
    got = _exec(ctx, good, _const9(consts), inputs)
    assert [got[i].tobytes() for i in range(len(inputs))] == want
