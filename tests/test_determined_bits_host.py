"""-m "not gpu" : the reference of the determinism closure's bit rule (tests/determined_bits_reference.py) on itself -- HELD and
the uniqueness of every rule-2 row against brute force, rules = 1 against determined_reference, the closure against the
completion on section 10f's generated circuit, the replayer against tampered certificates -- and the marking rows of
csrc/r1cs_bools.h through tests/cpp/r1cs_held_check.cpp: a stand-alone program built with -fsanitize=address,undefined and run
as a plain subprocess."""
import os
import subprocess

import pytest

import determined_bits_reference as db
import determined_reference as dr
import r1cs_builder as rb
import solve_bits_reference as sb
import solve_reference as sr
from determined_bits_reference import BITS, PIN
from determined_reference import ABSENT, DERIVED, NONE, OPEN, SEED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = db.R


def residual(circuit, w, c):
    a, b, cc = rb.values(circuit[1], circuit[2], circuit[3], w, c)
    return (a * b - cc) % R


def held_by_brute_force(circuit, w):
    """x is HELD when some constraint is 0 under w, does not move with any wire but x (tried: every other wire at two further
    values), is 0 at x = 0 and x = 1 and not at x = 2 -- a polynomial of degree <= 2 in x with the roots 0 and 1 that is not 0"""
    n_wires = circuit[0]
    mark = [0] * n_wires
    for c in range(len(circuit[1])):
        if residual(circuit, w, c):
            continue
        named = {s for rows in circuit[1:] for s, _ in rows[c]} - {0}
        for x in named:
            def at(t, other=None, shift=0):
                trial = list(w)
                trial[x] = t
                if other is not None:
                    trial[other] = (trial[other] + shift) % R
                return residual(circuit, trial, c)
            if at(0) or at(1) or not at(2):
                continue
            if all(at(t, y, d) == at(t) for y in named - {x} for t in (0, 1, 2, 5) for d in (1, 12345)):
                mark[x] = 1
    return mark


ALL_CASES = {}
ALL_CASES.update({"width_%d" % k: db.width(k)[0] for k in db.WIDTHS + (254, 1)})
ALL_CASES.update({"coef_" + n: db.coefficient_case(n)[0] for n in db.COEFFICIENTS})
ALL_CASES.update({"unknown_" + n: db.unknown_case(n)[0] for n in db.UNKNOWNS})
ALL_CASES.update({"orient_" + n: db.seeded(sb.oriented(n)[0]) for n in sb.ORIENTATIONS})
ALL_CASES.update({"long_row": db.long_row()[0], "pin_bits_pin": db.pin_bits_pin()[0], "pin_first": db.pin_first()[0],
                  "falls_to_0": db.falls_to_0_behind_bits()[0], "conflict_2": db.conflict(2)[0], "conflict_65": db.conflict(65)[0],
                  "partly_seeded": db.partly_seeded()[0], "generated": db.generated(8, 5)})


@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_held_against_brute_force_on_the_directed_circuits(name):
    circuit, w, _, _ = ALL_CASES[name]
    held = db.held_wires(circuit, w)
    assert held == held_by_brute_force(circuit, w)
    boolean = sb.boolean_wires(circuit)
    assert all(b >= h for b, h in zip(boolean, held))                                  # HELD is a subset of BOOLEAN
    if rb.check(circuit[1], circuit[2], circuit[3], w) == []:
        assert held == boolean                                                         # ... and all of it on a satisfying witness


@pytest.mark.parametrize("i", range(db.N_RANDOM))
def test_held_against_brute_force_on_the_random_circuits(i):
    circuit, w, _, _ = db.random_case(i)
    held = db.held_wires(circuit, w)
    assert held == held_by_brute_force(circuit, w)
    assert all(b >= h for b, h in zip(sb.boolean_wires(circuit), held))


def test_the_random_circuits_break_marking_rows():
    """some wires are BOOLEAN and not HELD, or the subset claim is never tried"""
    lost = 0
    for i in range(db.N_RANDOM):
        circuit, w, _, _ = db.random_case(i)
        lost += sum(sb.boolean_wires(circuit)) - sum(db.held_wires(circuit, w))
    assert lost >= 5


@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_the_reference_replays_its_own_certificates(name):
    circuit, w, _, seed = ALL_CASES[name]
    for rules in (PIN, PIN | BITS):
        res = db.closure(circuit, w, seed, rules)
        assert db.replay(circuit, w, seed, res["status"], res["round"], res["by"], res["rule"]) is None, (name, rules)


@pytest.mark.parametrize("i", range(db.N_RANDOM))
def test_satisfying_circuits_against_brute_force(i):
    """every rule-2 row: over the 0/1 assignments of its unknowns -- the wires of the row that have no smaller round -- the
    witness's is the only one that satisfies the row"""
    circuit, w, _, seed = db.satisfying_case(i)
    assert rb.check(circuit[1], circuit[2], circuit[3], w) == []
    res = db.closure(circuit, w, seed)
    assert db.replay(circuit, w, seed, res["status"], res["round"], res["by"], res["rule"]) is None
    merged = sb.merged_of(circuit)
    for c in sorted({res["by"][x] for x in range(circuit[0]) if res["rule"][x] == BITS}):
        level = min(res["round"][x] for x in range(circuit[0]) if res["rule"][x] == BITS and res["by"][x] == c)
        out = sorted(s for s in set().union(*merged[c]) if res["round"][s] == NONE or res["round"][s] >= level)
        assert 2 <= len(out) <= 12 and all(w[x] in (0, 1) for x in out)
        assert db.unique_by_brute_force(circuit, w, None, c, out) == 1, (i, c)


def test_the_satisfying_circuits_exercise_both_rules():
    got = [db.closure(*(db.satisfying_case(i)[k] for k in (0, 1, 3))) for i in range(db.N_RANDOM)]
    assert sum(1 for r in got if r["n_by_bits"]) >= 25
    assert sum(1 for r in got if any(k == PIN and ro > 1 for k, ro in zip(r["rule"], r["round"]))) >= 5     # PIN behind a bit level
    assert sum(1 for r in got if OPEN in r["status"]) >= 5


@pytest.mark.parametrize("i", range(dr.N_RANDOM))
def test_rules_1_is_determined_reference_on_its_random_circuits(i):
    circuit, w, header, seed = dr.resolved(dr.random_case(i))
    res = db.closure(circuit, w, seed, rules=PIN)
    status, rounds, by = dr.closure(circuit, w, seed)
    assert (res["status"], res["round"], res["by"]) == (status, rounds, by) and res["n_by_bits"] == 0
    assert res["rule"] == [int(s == DERIVED) for s in status]


@pytest.mark.parametrize("name", sorted(dr.DIRECTED))
def test_rules_1_is_determined_reference_on_its_directed_circuits(name):
    circuit, w, header, seed = dr.resolved(dr.DIRECTED[name])
    res = db.closure(circuit, w, seed, rules=PIN)
    assert (res["status"], res["round"], res["by"]) == dr.closure(circuit, w, seed)


@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_rules_1_is_determined_reference_on_these_circuits(name):
    circuit, w, _, seed = ALL_CASES[name]
    res = db.closure(circuit, w, seed, rules=PIN)
    assert (res["status"], res["round"], res["by"]) == dr.closure(circuit, w, seed)


def test_the_closure_is_the_completion_on_the_generated_circuit():
    """section 10f's generator at 8 decompositions of 5 bits: from the same wires, the closure names what the completion solves,
    in the same rounds, by the same constraints.  The GPU's cross-check relies on this."""
    circuit, w, _, seed = db.generated(8, 5)
    assert circuit[0] == 1 + 8 * (1 + 5 + 2) and len(seed) == 8
    res = db.closure(circuit, w, seed)
    want = sb.complete(circuit, w, seed, sb.LINEAR | sb.BITS)
    assert (SEED, DERIVED, ABSENT, OPEN) == (sr.GIVEN, sr.SOLVED, sr.ABSENT, sr.OPEN)
    assert (res["status"], res["round"], res["by"], res["rule"]) == (want["status"], want["round"], want["by"], want["rule"])
    assert want["wtns"] == w and db.summary(res)[:5] == (8 * 7, 0, 0, 3, 8 * 5)
    assert db.summary(db.closure(circuit, w, seed, PIN))[:4] == (0, 0, 8 * 7, 0)           # the PIN rule alone: all OPEN


@pytest.mark.parametrize("k", db.WIDTHS)
def test_widths_derive_every_bit_in_round_1(k):
    (circuit, w, _, seed), info = db.width(k)
    res = db.closure(circuit, w, seed)
    assert db.summary(res)[:5] == (k, 0, 0, 1, k)
    assert all((res["round"][b], res["by"][b], res["rule"][b]) == (1, info["row"], BITS) for b in info["bits"])


def test_width_254_is_refused_and_width_1_is_the_pin_rule():
    (circuit, w, _, seed), info = db.width(254)
    res = db.closure(circuit, w, seed)
    assert res["n_by_bits"] == 0 and db.summary(res)[5] == info["bits"]
    (circuit, w, _, seed), info = db.width(1)
    res = db.closure(circuit, w, seed)
    assert res["n_by_bits"] == 0 and res["rule"][info["bits"][0]] == PIN


@pytest.mark.parametrize("name", sb.ORIENTATIONS)
def test_orientations(name):
    case, info = sb.oriented(name)
    circuit, w, _, seed = db.seeded(case)
    res = db.closure(circuit, w, seed)
    assert res["n_by_bits"] == (len(info["bits"]) if info["solved"] else 0), name
    if not info["solved"]:
        assert db.summary(res)[5] == sorted(info["bits"])


@pytest.mark.parametrize("name", db.COEFFICIENTS)
def test_refusals_by_coefficient(name):
    (circuit, w, _, seed), info = db.coefficient_case(name)
    res = db.closure(circuit, w, seed)
    assert res["n_by_bits"] == (4 if info["derives"] else 0), name
    assert db.summary(res)[5] == ([] if info["derives"] else sorted(info["bits"]))


@pytest.mark.parametrize("name", db.UNKNOWNS)
def test_refusals_by_unknowns(name):
    (circuit, w, _, seed), info = db.unknown_case(name)
    res = db.closure(circuit, w, seed)
    assert sorted(s for s, k in enumerate(res["rule"]) if k == BITS) == sorted(info["derives"]), name
    assert db.summary(res)[5] == sorted(set(info["bits"]) - set(info["derives"])), name
    broken = rb.check(circuit[1], circuit[2], circuit[3], w)
    held = db.held_wires(circuit, w)
    if name in ("marking_row_broken", "two_marking_rows_broken"):
        assert info["row"] not in broken and held[info["bits"][1]] == 0 and sb.boolean_wires(circuit)[info["bits"][1]] == 1
        assert len(broken) == (1 if name == "marking_row_broken" else 2)
    if name == "two_marking_rows_unbroken":
        assert sum(1 for c, x in db.marking_rows(circuit) if x == info["bits"][1]) == 2 and broken == []
    if name == "row_broken":
        assert broken == [info["row"]] and all(held[b] for b in info["bits"])
    if name == "free_incidence":
        assert broken == [] and all(held[b] for b in info["bits"])


def test_long_row_and_partly_seeded_bits():
    (circuit, w, _, seed), info = db.long_row()
    assert len(sb.merged_of(circuit)[info["row"]][0]) > 64
    assert db.closure(circuit, w, seed)["n_by_bits"] == 3
    (circuit, w, _, seed), info = db.partly_seeded()
    assert db.closure(circuit, w, seed)["n_by_bits"] == 65


@pytest.mark.parametrize("n", (2, 65))
def test_conflicts_name_the_lowest_row(n):
    (circuit, w, _, seed), info = db.conflict(n)
    assert rb.check(circuit[1], circuit[2], circuit[3], w) == [] and info["row0"] > 0
    res = db.closure(circuit, w, seed)
    assert {res["by"][b] for b in info["bits"]} == {info["row0"]} and res["n_by_bits"] == sb.CONFLICT_BITS
    merged, known = sb.merged_of(circuit), set(seed) | {0}
    rows = [c for c, ms in enumerate(merged) if db.bit_row(ms, *rb.values(circuit[1], circuit[2], circuit[3], w, c)[:2], known, db.held_wires(circuit, w))]
    assert rows == list(range(info["row0"], info["row0"] + n))                         # all n qualify in the one level


def test_alternation_numbers_the_rounds():
    for make in (db.pin_bits_pin, db.pin_first):
        (circuit, w, _, seed), want = make()
        res = db.closure(circuit, w, seed)
        assert {x: (res["round"][x], res["rule"][x]) for x in want} == want
        assert db.summary(res)[2] == 0 and db.summary(res)[3] == max(r for r, _ in want.values())


def test_a_row_falls_from_2_to_0_behind_the_bit_frontier():
    (circuit, w, _, seed), opened, (p, q) = db.falls_to_0_behind_bits()
    res = db.closure(circuit, w, seed)
    assert db.summary(res)[5] == sorted(opened) and (res["round"][p], res["round"][q]) == (1, 1)
    assert (res["rule"][p], res["rule"][q]) == (BITS, BITS)
    assert set(sb.merged_of(circuit)[1][0]) | set(sb.merged_of(circuit)[1][2]) == {p, q}   # constraint 1 holds exactly the two


def test_the_replayer_refuses_tampered_certificates():
    (circuit, w, _, seed), want = db.pin_bits_pin()
    res = db.closure(circuit, w, seed)
    maps = lambda: [list(res[k]) for k in ("status", "round", "by", "rule")]
    bit = next(x for x, (_, k) in want.items() if k == BITS and res["round"][x] == 4)
    pin = next(x for x, (r, k) in want.items() if k == PIN and r == 2)
    st, ro, by, ru = maps()
    ro[bit] = 1                                                                        # before z is known, the row holds z outside
    assert db.replay(circuit, w, seed, st, ro, by, ru) is not None
    st, ro, by, ru = maps()
    ru[pin] = BITS                                                                     # a PIN's row is no decomposition
    assert db.replay(circuit, w, seed, st, ro, by, ru) is not None
    st, ro, by, ru = maps()
    ru[bit] = PIN                                                                      # a bit row has six wires outside
    assert db.replay(circuit, w, seed, st, ro, by, ru) is not None
    st, ro, by, ru = maps()
    by[bit] = 0                                                                        # a row that does not name the wire
    assert db.replay(circuit, w, seed, st, ro, by, ru) is not None
    (circuit, w, _, seed), info = db.unknown_case("marking_row_broken")                # a certificate through a wire that is not HELD
    good = db.closure(*db.unknown_case("two_marking_rows_unbroken")[0][:2], seed)
    res = db.closure(circuit, w, seed)
    st, ro, by, ru = (list(res[k]) for k in ("status", "round", "by", "rule"))
    for b in info["bits"]:
        st[b], ro[b], by[b], ru[b] = DERIVED, 1, info["row"], BITS
    assert db.replay(circuit, w, seed, st, ro, by, ru) is not None and good["n_by_bits"] == 4


# ---------------------------------------------------------------- the host code of csrc/r1cs_bools.h under the sanitizers
@pytest.fixture(scope="module")
def held_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("determined_bits_host") / "r1cs_held_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "keyless-zk-proofs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "r1cs_held_check.cpp"), "-o", out], timeout=600)
    return out


def test_the_program_hands_out_the_reference_s_marking_rows(held_exe, tmp_path):
    names = sorted(ALL_CASES)
    circuits = [ALL_CASES[n][0] for n in names] + [db.random_case(i)[0] for i in range(0, db.N_RANDOM, 4)] + list(db.EMPTY.values())
    paths = []
    for k, circuit in enumerate(circuits):
        paths.append(str(tmp_path / ("c%d.r1cs" % k)))
        with open(paths[-1], "wb") as f:
            f.write(rb.write(*circuit))
    out = subprocess.run([held_exe] + paths, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr[-4000:]     # the sanitizers stay silent
    lines = out.stdout.split("\n")
    assert "FAIL" not in out.stdout and len(lines) == 3 * len(circuits) + 1
    for k, circuit in enumerate(circuits):
        rows = db.marking_rows(circuit)
        assert lines[3 * k] == "rc=0"
        assert lines[3 * k + 1] == "rows=%d n=%d wires=%d" % (len(rows), sum(sb.boolean_wires(circuit)), circuit[0]), k
        assert lines[3 * k + 2] == " ".join("%d:%d" % cx for cx in rows), k
