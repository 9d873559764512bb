"""CPU: what the wave-cooperative interpreter's linear step (k_verify_coop, csrc/verify.hip) rests on.

  * tests/cpp/coop_bounds_check.cpp validates the four real programs (coop_program_check) and propagates an upper bound
    per slot through every step: MUL operand products, INV operands, the linear step's bias, top_est, q, accumulators and
    result, the outputs' bound.  Its header derives the linear step's result bound.
  * the integer model of the linear step (tests/coop_asm.py, transcribed from verify.hip) keeps its invariants on directed
    and seeded-random combinations at the documented limits, and the directed families really sit on the edges they name.
  * the assembler and the big-integer reference of tests/coop_asm.py against the real encoder: the dumped
    final-exponentiation program decodes, re-assembles to the same arrays, and the reference run on it equals the oracle's
    final exponentiation bit for bit.
"""
import os

import pytest

import coop_asm as ca
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cbc(tmp_path_factory):
    return ca.build_dump(ROOT, tmp_path_factory.mktemp("cbc"))


def test_bounds_audit_of_the_four_real_programs(cbc):
    out, _ = cbc
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bounds audit: 4 programs OK" in out.stdout
    for name in ("full:", "early:", "late:", "finalexp:", "documented limits"):
        assert name in out.stdout


def _check_invariants(name, comb):
    tr = ca.lin_model([(cf, ca.to_limbs(v)) for cf, v in comb])
    assert not tr.overflow, name
    assert 0 <= tr.top_est < (1 << 38), name
    assert 0 <= tr.q < (1 << 17), name
    assert all(0 <= x < (1 << 29) for x in tr.out[:8]), name
    assert 0 <= tr.top < (1 << 32), name
    total = sum(cf * v for cf, v in comb)
    assert tr.value % ca.P == total % ca.P, name
    assert tr.value == (ca.P << 15) + total - tr.q * ca.P, name
    assert 0 <= tr.value < ca.LIN_RESULT_BOUND * ca.P, name
    return tr


def test_model_invariants_on_directed_combinations():
    fam = {}
    for name, comb in ca.directed_combinations():
        assert sum(abs(cf) for cf, _ in comb) <= ca.MAX_COEF and 1 <= len(comb) <= ca.MAX_TERMS
        fam[name] = _check_invariants(name, comb)
    # the families sit where they say
    for name, tr in fam.items():
        if name.startswith("top_est = "):
            mod, d = int(name.split()[2]), int(name.split()[4])
            assert (tr.top_est - d) % mod == 0, name
    assert fam["limb 6 negative"].acc[6] < 0
    assert fam["limb 7 negative after q"].acc_q[7] < 0
    assert all(x < 0 for x in fam["limbs 0..7 negative after q"].acc_q[:8])
    assert any(c < 0 for tr in fam.values() for c in tr.carries)       # the carry's upper half matters
    assert any(c > 0 for tr in fam.values() for c in tr.carries)
    assert fam["+4096 x (5p - 1)"].q > (1 << 15) > fam["-4096 x (5p - 1)"].q
    assert fam["total 4096 p"].value % ca.P == 0 and fam["total 0 = p - p"].value % ca.P == 0
    assert len({tr.q for tr in fam.values()}) > 25


def test_model_says_the_neighbouring_group_extremes_are_opposite():
    """what tests/test_gpu_coop_exec.py puts into adjacent groups"""
    hi = ca.lin_model([(cf, ca.to_limbs(v)) for cf, v in ca.HI_Q])
    lo = ca.lin_model([(cf, ca.to_limbs(v)) for cf, v in ca.LO_Q])
    assert hi.q > 50000 and lo.q < 13000 and all(c < 0 for c in hi.carries) and lo.carries[0] > 0 and lo.carries[1] >= 0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_invariants_on_random_combinations_at_the_limits(seed):
    rng = ca.Rng(seed)
    pool = ca.directed_operands()
    lo, hi = ca.LIN_RESULT_BOUND * ca.P, 0
    for n in list(range(1, ca.MAX_TERMS + 1)) * 60:
        comb = ca.random_combination(rng, n, pool)
        assert sum(abs(cf) for cf, _ in comb) == ca.MAX_COEF
        tr = _check_invariants("seed %d" % seed, comb)
        lo, hi = min(lo, tr.value), max(hi, tr.value)
    print("results in [%.4f p, %.4f p]; derived bound %.4f p" % (lo / ca.P, hi / ca.P, float(ca.LIN_RESULT_BOUND)))


def test_derived_bound_is_below_the_documented_one():
    assert 3 < ca.LIN_RESULT_BOUND < 3.02 < ca.OPERAND_BOUND
    assert 5547123 * 3171407 == (1 << 44) - 1332355 and 3171406 << 232 < ca.P < 3171407 << 232 and 169 * ca.P < ca.RP


def test_assembler_reproduces_the_encoders_arrays(cbc):
    out, dump = cbc
    assert out.returncode == 0, out.stdout + out.stderr
    prog, _ = ca.load_dump(dump)
    steps = ca.decode(prog.step_class, prog.words, prog.terms)
    again = ca.assemble(steps, prog.n_const, prog.n_slots, prog.out_slot)
    assert (again.step_class == prog.step_class).all()
    assert (again.words == prog.words).all()
    assert again.terms.size == prog.terms.size and (again.terms == prog.terms).all()


def test_reference_on_the_dumped_program_equals_the_oracles_final_exponentiation(cbc):
    out, dump = cbc
    assert out.returncode == 0, out.stdout + out.stderr
    prog, const9 = ca.load_dump(dump)
    steps = ca.decode(prog.step_class, prog.words, prog.terms)
    consts = [ca.from_limbs(c) for c in const9]
    assert consts[0] == 0 and consts[1] == ca.RP % ca.P and all(c < 2 * ca.P for c in consts)
    rng = ca.Rng(2024)
    for trial in range(20):
        f = [rng.below(ca.P) for _ in range(12)]
        got = ca.out_bytes(ca.run_reference(steps, consts, f, prog.n_slots, prog.out_slot))
        assert got == ol.final_exp(ca.out_bytes(f)), trial
