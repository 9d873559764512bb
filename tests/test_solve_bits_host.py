"""CPU: the reference of the witness completion's bit rule (tests/solve_bits_reference.py) asserted on itself -- the boolean
marks on the forms and the non-forms, the rule's output against the generating witness and against brute force over the 0/1
assignments, rules = 1 against solve_reference -- and keyless-zk-proofs_amd/csrc/r1cs_bools.h, the marks of the product,
through tests/cpp/r1cs_bools_check.cpp: a stand-alone program built with -fsanitize=address,undefined and run as a plain
subprocess."""
import itertools
import os
import subprocess

import pytest

import determined_reference as dr
import r1cs_builder as rb
import solve_bits_reference as sb
import solve_reference as sr
from determined_reference import Rows, const, v
from solve_bits_reference import BITS, LINEAR, R
from solve_reference import GIVEN, NONE, OPEN, SOLVED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the marks
def marks_of(a, b, c, n_wires=4):
    rows = Rows()
    rows.mul(a, b, c)
    return sb.boolean_wires(rows.circuit(n_wires))


FORMS = {
    "b(b-1)=0": (v(1), v(1) + const(-1), []),
    "b(1-b)=0": (v(1), const(1) + v(1, -1), []),
    "bb=b": (v(1), v(1), v(1)),
    "scaled": (v(1, 5), v(1, 7) + const(-7), []),
    "scaled_with_C": (v(1, 5) + const(3), v(1, 7) + const(-7), v(1, 21) + const(-21)),       # (5b + 3)(7b - 7) = 21 b - 21
    "listed_twice": (v(1, 2) + v(1, -1), v(1) + const(-1), v(2, 9) + v(2, -9)),                # merged: b (b - 1) = 0
}
NON_FORMS = {
    "k_not_zero": (v(1), v(1) + const(-1), const(1)),                                          # b (b - 1) = 1
    "lin_not_minus_quad": (v(1), v(1) + const(-2), []),                                        # b (b - 2) = 0: roots 0, 2
    "third_wire": (v(1), v(1) + const(-1), v(2)),
    "third_wire_in_A": (v(1) + v(2), v(1) + const(-1), []),
    "quad_zero": (v(1), const(1), v(1)),                                                       # b = b
    "quad_zero_linear": (v(1), const(1), const(1)),                                            # b = 1
    "square": (v(1), v(1), const(1)),                                                          # b b = 1: roots 1, -1
}


@pytest.mark.parametrize("name", sorted(FORMS))
def test_the_forms_mark_their_wire(name):
    assert marks_of(*FORMS[name]) == [0, 1, 0, 0]
    a, b, c = FORMS[name]
    for x in range(-3, 4):                                                                     # and the roots are exactly 0 and 1
        holds = rb.dot(a, [1, x % R, 0, 0]) * rb.dot(b, [1, x % R, 0, 0]) % R == rb.dot(c, [1, x % R, 0, 0])
        assert holds == (x in (0, 1)), (name, x)


@pytest.mark.parametrize("name", sorted(NON_FORMS))
def test_the_non_forms_mark_nothing(name):
    assert marks_of(*NON_FORMS[name]) == [0, 0, 0, 0]


def test_wire_0_is_never_marked():
    assert marks_of(const(1), const(1) + const(-1), []) == [0, 0, 0, 0]


# ---------------------------------------------------------------- the rule
def all_cases():
    out = {"width_%d" % k: sb.width(k)[0] for k in sb.WIDTHS + (254,)}
    out.update({"orient_" + n: sb.oriented(n)[0] for n in sb.ORIENTATIONS})
    out.update({"refusal_" + n: sb.refusal(n)[0] for n in sb.REFUSALS})
    out["partly_given"] = sb.partly_given(12, [0, 5, 11])[0]
    out["infeasible"] = sb.infeasible_rows()[0]
    out["long_257"] = sb.long_row(257)[0]
    out.update({"alternation_%d" % s: sb.alternation(s)[0] for s in (1, 2, 3)})
    out.update({"conflict_%d_%d_%d" % k: sb.conflict(*k)[0] for k in sb.CONFLICTS})
    return out


CASES = all_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_a_satisfiable_case_gets_its_generating_witness(name):
    circuit, w, _, given = CASES[name]
    res = sb.complete(circuit, w, given)
    if rb.check(circuit[1], circuit[2], circuit[3], w) == []:
        assert all(res["wtns"][s] == w[s] for s, k in enumerate(res["status"]) if k in (GIVEN, SOLVED)), name
        assert res["failed"] == [] and res["infeasible"] == [], name


@pytest.mark.parametrize("k", sb.WIDTHS)
def test_widths_solve_every_bit_in_round_1(k):
    (circuit, w, _, given), info = sb.width(k)
    res = sb.complete(circuit, w, given)
    assert res["wtns"] == w and res["n_by_bits"] == k and sb.summary(res)[:4] == (k, 0, 0, 1)
    assert all((res["round"][b], res["by"][b], res["rule"][b]) == (1, info["row"], BITS) for b in info["bits"])


def test_width_254_is_refused_and_width_1_is_the_linear_rule():
    (circuit, w, _, given), info = sb.width(254)
    res = sb.complete(circuit, w, given)
    assert res["n_by_bits"] == 0 and sb.open_wires(res) == info["bits"] and res["infeasible"] == []
    (circuit, w, _, given), info = sb.width(1)
    res = sb.complete(circuit, w, given)
    assert res["wtns"] == w and [res["rule"][b] for b in info["bits"]] == [LINEAR] and res["n_by_bits"] == 0


@pytest.mark.parametrize("name", sb.ORIENTATIONS)
def test_orientations(name):
    (circuit, w, _, given), info = sb.oriented(name)
    res = sb.complete(circuit, w, given)
    if info["solved"]:
        assert res["wtns"] == w and all(res["rule"][b] == BITS and res["by"][b] == info["row"] for b in info["bits"]), name
    else:
        assert sb.open_wires(res) == info["bits"] and res["n_by_bits"] == 0 and res["infeasible"] == [], name


@pytest.mark.parametrize("name", sb.REFUSALS)
def test_refusals_leave_the_bits_open_and_change_nothing_else(name):
    (circuit, w, _, given), info = sb.refusal(name)
    res, lin = sb.complete(circuit, w, given), sr.complete(circuit, w, given)
    assert sb.open_wires(res) == sorted(info["bits"]) and res["infeasible"] == [] and res["n_by_bits"] == 0, name
    assert all(res[k] == lin[k] for k in lin), name


def test_partly_given_bits_carry_their_weight_in_k0():
    (circuit, w, _, given), info = sb.partly_given(12, [0, 5, 11], "C", 12345)
    res = sb.complete(circuit, w, given)
    assert res["wtns"] == w and res["n_by_bits"] == 9
    assert [res["status"][b] for b in info["bits"]] == [GIVEN if i in (0, 5, 11) else SOLVED for i in range(12)]


def test_infeasible_rows_are_named_and_give_nothing():
    (circuit, w, _, given), rows, good, good_bits = sb.infeasible_rows()
    res = sb.complete(circuit, w, given)
    assert res["infeasible"] == rows and res["n_by_bits"] == len(good_bits) and res["failed"] == []
    assert all(res["by"][b] == good for b in good_bits) and sb.summary(res)[3] == 1


@pytest.mark.parametrize("stages", (1, 2, 3))
def test_alternation_numbers_the_rounds(stages):
    (circuit, w, _, given), plan = sb.alternation(stages)
    res = sb.complete(circuit, w, given)
    assert res["wtns"] == w and sb.summary(res)[3] == 2 * stages + 1
    for kind, wires, rnd in plan:
        assert all((res["rule"][s], res["round"][s]) == (kind, rnd) for s in wires)


@pytest.mark.parametrize("n,last,behind", sb.CONFLICTS)
def test_conflicts_commit_the_lowest_row(n, last, behind):
    (circuit, w, _, given), info = sb.conflict(n, last, behind)
    res = sb.complete(circuit, w, given)
    assert info["row0"] == (sb.CONFLICT_BITS + 1 if behind else 0)
    assert {res["by"][b] for b in info["bits"]} == {info["row0"]} and {res["round"][b] for b in info["bits"]} == {1}
    assert sum(res["wtns"][b] << i for i, b in enumerate(info["bits"])) == info["value"]
    assert res["failed"] == list(range(info["row0"] + 1, info["row0"] + n)) and len(res["failed"]) == info["n_failed"] == n - 1
    if behind:                                                                                 # the refused row closes a round later
        assert (res["rule"][info["y"]], res["round"][info["y"]], res["by"][info["y"]]) == (LINEAR, 2, sb.CONFLICT_BITS)


def unknowns_at(ms, known):
    return sorted(s for s in set(ms[0]) | set(ms[1]) | set(ms[2]) if s not in known)


def satisfying(ms, val, unknown):
    """the 0/1 assignments of `unknown` under which the constraint with merged rows ms holds, the other wires from val"""
    out = []
    for bits in itertools.product((0, 1), repeat=len(unknown)):
        full = {**val, **dict(zip(unknown, bits))}
        a, b, c = (sum(k * full[s] for s, k in m.items()) % R for m in ms)
        if a * b % R == c:
            out.append(bits)
    return out


@pytest.mark.parametrize("i", range(sb.N_RANDOM))
def test_random_circuits_against_brute_force(i):
    circuit, w, _, given = sb.random_case(i)
    res = sb.complete(circuit, w, given)
    merged = sb.merged_of(circuit)
    val = {s: res["wtns"][s] for s, k in enumerate(res["status"]) if k in (GIVEN, SOLVED)}
    for c in res["infeasible"]:                                                                # INFEASIBLE: no 0/1 assignment at all
        unknown = unknowns_at(merged[c], val)
        assert 2 <= len(unknown) <= 12 and satisfying(merged[c], val, unknown) == [], (i, c)
    for x, rule in enumerate(res["rule"]):                                                     # FEASIBLE: the one there is
        if rule != BITS:
            continue
        before = {s: t for s, t in val.items() if res["round"][s] < res["round"][x]}
        unknown = unknowns_at(merged[res["by"][x]], before)
        assert x in unknown and len(unknown) <= 12
        found = satisfying(merged[res["by"][x]], before, unknown)
        assert len(found) == 1 and res["wtns"][x] == found[0][unknown.index(x)], (i, x)
    assert res["n_by_bits"] == res["rule"].count(BITS)


def test_the_random_circuits_exercise_the_rule():
    got = [sb.complete(*(sb.random_case(i)[k] for k in (0, 1, 3))) for i in range(sb.N_RANDOM)]
    assert sum(1 for r in got if r["n_by_bits"]) >= 10 and sum(1 for r in got if r["infeasible"]) >= 5
    assert sum(1 for r in got if LINEAR in r["rule"] and BITS in r["rule"]) >= 5
    assert any(max(r["round"][s] for s, k in enumerate(r["rule"]) if k) >= 3 for r in got if r["n_by_bits"])


@pytest.mark.parametrize("i", range(sr.N_FORWARD))
def test_rules_1_is_the_linear_completion(i):
    (circuit, w, header, given), _ = sr.forward_circuit(i)
    given = dr.default_seed(header) if given is None else given
    res, lin = sb.complete(circuit, w, given, rules=LINEAR), sr.complete(circuit, w, given)
    assert all(res[k] == lin[k] for k in lin)
    assert res["n_by_bits"] == 0 and res["infeasible"] == [] and res["rule"] == [int(k == SOLVED) for k in lin["status"]]


@pytest.mark.parametrize("i", range(0, sb.N_RANDOM, 4))
def test_rules_1_on_the_random_circuits(i):
    circuit, w, _, given = sb.random_case(i)
    res, lin = sb.complete(circuit, w, given, rules=LINEAR), sr.complete(circuit, w, given)
    assert all(res[k] == lin[k] for k in lin) and res["n_by_bits"] == 0 and res["infeasible"] == []


# ---------------------------------------------------------------- the product's marks (csrc/r1cs_bools.h)
@pytest.fixture(scope="module")
def bools_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("solve_bits_host") / "r1cs_bools_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "keyless-zk-proofs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "r1cs_bools_check.cpp"), "-o", out], timeout=600)
    return out


def marks_by_the_program(exe, tmp_path, circuits):
    paths = []
    for i, circ in enumerate(circuits):
        p = tmp_path / ("c%d.r1cs" % i)
        p.write_bytes(rb.write(*circ[:4]))
        paths.append(str(p))
    out = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr[-4000:]     # the sanitizers stay silent
    lines = out.stdout.split("\n")
    assert "FAIL" not in out.stdout and len(lines) == 3 * len(circuits) + 1
    got = []
    for i in range(len(circuits)):
        assert lines[3 * i] == "rc=0"
        got.append([int(ch) for ch in lines[3 * i + 2]])
        assert lines[3 * i + 1] == "n=%d wires=%d" % (sum(got[-1]), circuits[i][0])
    return got


def test_the_program_marks_what_the_reference_marks(bools_exe, tmp_path):
    circuits = []
    for a, b, c in list(FORMS.values()) + list(NON_FORMS.values()):
        rows = Rows()
        rows.mul(a, b, c)
        circuits.append(rows.circuit(4))
    circuits += [case[0] for case in CASES.values() if case[0][0] <= 2000]
    circuits += [sb.random_case(i)[0] for i in range(sb.N_RANDOM)]
    circuits += [dr.random_case(i)[0] for i in range(0, dr.N_RANDOM, 5)]
    circuits.append((70, [], [], []))                                                          # no constraint at all
    got = marks_by_the_program(bools_exe, tmp_path, circuits)
    for circ, marks in zip(circuits, got):
        assert marks == sb.boolean_wires(circ)
    assert sum(map(sum, got)) > 500
