"""CPU tests of the witness completion's host side and of its reference: tests/solve_reference.py on circuits whose answer is
stated by hand, its relation to the determinism closure's reference on every shared circuit, and
keyless-zk-proofs_amd/csrc/r1cs_rows.h, the row view, through tests/cpp/r1cs_rows_check.cpp -- a stand-alone program built with
-fsanitize=address,undefined and run as a plain subprocess."""
import os
import subprocess

import pytest

import determined_reference as dr
import r1cs_builder as rb
import solve_reference as sr
import unbound_reference as ur
from solve_reference import ABSENT, GIVEN, NONE, OPEN, SOLVED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = sr.R


def run(c):
    circuit, w, header, given = sr.resolved(c)
    return sr.complete(circuit, w, given)


def test_classes_are_numbered_as_the_closures():
    assert (GIVEN, SOLVED, ABSENT, OPEN, NONE) == (dr.SEED, dr.DERIVED, dr.ABSENT, dr.OPEN, dr.NONE) == (0, 1, 2, 3, 0xFFFFFFFF)


@pytest.mark.parametrize("name", sorted(sr.SIDES))
def test_sides_of_the_unknown_by_hand(name):
    res = run(sr.SIDES[name])
    for wire, (status, rnd, by, value) in sr.SIDES_EXPECTED[name].items():
        assert (res["status"][wire], res["round"][wire], res["by"][wire], res["wtns"][wire]) == (status, rnd, by, value % R), (name, wire)
    assert res["failed"] == []


def test_sides_by_hand_the_counts():
    want = {"x_on_A_and_B": (0, 0, 1, 0, 0, 1), "lin_zero_A_b0_is_C": (0, 0, 1, 0, 0, 1), "lin_zero_k0_not": (0, 0, 1, 0, 0, 1),
            "lin_zero_only_modulo_r": (0, 0, 1, 0, 0, 1), "zero_is_a_value": (2, 0, 0, 2, 0, 0), "merged_and_cancelling": (2, 1, 1, 1, 0, 1)}
    for name, c in sr.SIDES.items():
        assert sr.summary(run(c)) == want.get(name, (1, 0, 0, 1, 0, 0)), name


def test_directed_circuits_of_the_closure_by_hand():
    """what some of determined_reference's circuits must give here: {wire: (status, round, by)}"""
    want = {
        "chain_3": {1: (GIVEN, 0, NONE), 2: (SOLVED, 1, 0), 3: (SOLVED, 2, 1), 4: (SOLVED, 3, 2)},
        "diamond": {2: (SOLVED, 1, 0), 3: (SOLVED, 1, 1), 4: (SOLVED, 2, 2)},
        "delayed": {2: (SOLVED, 1, 0), 3: (SOLVED, 2, 2), 5: (SOLVED, 2, 5), 4: (SOLVED, 1, 3), 6: (SOLVED, 1, 4)},
        "falls_to_0": {1: (OPEN, NONE, NONE), 2: (OPEN, NONE, NONE), 3: (OPEN, NONE, NONE), 5: (SOLVED, 1, 1), 6: (SOLVED, 1, 2)},
        "square_root_at_3": {2: (OPEN, NONE, NONE)},
        "square_root_at_0": {2: (OPEN, NONE, NONE)},                   # the closure derives it: a PIN with quad != 0; no root is taken here
        "mux_sel0_x": {2: (OPEN, NONE, NONE)}, "mux_sel1_x": {2: (SOLVED, 1, 0)},
        "free_but_counted": {3: (SOLVED, 1, 1), 4: (SOLVED, 2, 2), 5: (SOLVED, 3, 0), 6: (OPEN, NONE, NONE), 7: (OPEN, NONE, NONE)},
        "moving_pair_tmp_seeded": {1: (SOLVED, 1, 0), 2: (ABSENT, NONE, NONE), 3: (GIVEN, 0, NONE)},
        "seventy": {70: (SOLVED, 1, 0)},
    }
    for name, wires in want.items():
        res = run(dr.DIRECTED[name])
        for wire, expect in wires.items():
            assert (res["status"][wire], res["round"][wire], res["by"][wire]) == expect, (name, wire)


def test_broken_link_rederives_the_corrupted_wire():
    circuit, w_bad, header, _ = dr.DIRECTED["broken_link"]
    res = run(dr.DIRECTED["broken_link"])
    assert [s for s, k in enumerate(res["status"]) if k == SOLVED] == [2, 3, 4] and res["failed"] == []
    assert res["wtns"] == dr.DIRECTED["repaired_link"][1] != w_bad


def satisfying(name_or_index):
    """(circuit, a satisfying witness, given) of a shared case: the corrupted ones through their sound twin"""
    if isinstance(name_or_index, int):
        circuit, _, header, given = sr.resolved(dr.random_case(name_or_index))
        return circuit, ur.random_circuit(name_or_index)[4], given
    circuit, w, header, given = sr.resolved(dr.DIRECTED["repaired_link" if name_or_index == "broken_link" else name_or_index])
    return circuit, w, given


@pytest.mark.parametrize("case", sorted(dr.DIRECTED) + list(range(dr.N_RANDOM)), ids=str)
def test_solved_is_inside_the_closure_and_equal_to_the_witness(case):
    circuit, w, given = satisfying(case)
    assert rb.check(*circuit[1:], w) == []
    res = sr.complete(circuit, w, given)
    status, rounds, by = dr.closure(circuit, w, given)
    solved = {s for s, k in enumerate(res["status"]) if k == SOLVED}
    derived = {s for s, k in enumerate(status) if k == dr.DERIVED}
    assert solved <= derived
    assert all(res["wtns"][s] == w[s] for s in solved)
    assert res["failed"] == []
    missing = derived - solved
    if missing:                                                        # the first wire the closure has and this does not: a PIN with quad != 0
        x = min(missing, key=lambda s: (rounds[s], s))
        ma, mb = ur.merged_row(circuit[1][by[x]]), ur.merged_row(circuit[2][by[x]])
        assert ma.get(x, 0) * mb.get(x, 0) % R != 0, (case, x)


def test_square_root_at_0_is_the_example_of_a_missing_wire():
    circuit, w, given = satisfying("square_root_at_0")
    assert dr.closure(circuit, w, given)[0][2] == dr.DERIVED and sr.complete(circuit, w, given)["status"][2] == OPEN


def test_random_cases_are_not_degenerate():
    """totals over the 40 random cases with their own (odd: corrupted) witness; the reference gives 491 / 10 / 5"""
    solved = odd_failed = all_known = 0
    for i in range(dr.N_RANDOM):
        res = run(dr.random_case(i))
        n_solved, _, n_open, _, n_failed, _ = sr.summary(res)
        solved += n_solved
        odd_failed += bool(i & 1 and n_failed)
        all_known += n_open == 0
        if not i & 1:
            assert n_failed == 0, i
    assert solved >= 400 and odd_failed >= 8 and all_known >= 3, (solved, odd_failed, all_known)
    assert (solved, odd_failed, all_known) == (491, 10, 5)


def test_long_rows_conflicts_and_forward_circuits_by_construction():
    for n in sr.LONG_ROWS:
        for at in (None, 0, n // 2, n - 1):
            circuit, w, header, given = sr.long_row(n, at)
            res = sr.complete(circuit, w, given)
            assert res["wtns"] == w and sr.summary(res) == (1, 0, 0, 1, 0, 0), (n, at)
    for n, last, deep in sr.CONFLICTS:
        circuit, w, header, given = sr.conflict(n, last, deep)
        res = sr.complete(circuit, w, given)
        x = n + 2 if last else 1
        assert (res["status"][x], res["by"][x], res["wtns"][x]) == (SOLVED, 0, w[x]), (n, last, deep)
        assert res["failed"] == list(range(1, n)) and res["round"][x] == (2 if deep else 1)
    for i in range(sr.N_FORWARD):
        (circuit, w, header, given), depth = sr.forward_circuit(i)
        res = sr.complete(circuit, w, dr.default_seed(header))
        assert res["wtns"] == w and sr.summary(res)[2:5] == (0, depth, 0), i


# ---------------------------------------------------------------- the row view
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("solve_host") / "r1cs_rows_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "keyless-zk-proofs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "r1cs_rows_check.cpp"), "-o", out], timeout=600)
    return out


def rows_of(exe, tmp_path, circuits):
    """the program's output for a list of circuits, one file each, in one run: per circuit [(matrix, constraint, [(wire, coef)])]"""
    paths = []
    for i, circ in enumerate(circuits):
        p = tmp_path / ("c%d.r1cs" % i)
        p.write_bytes(rb.write(*circ[:4]))
        paths.append(str(p))
    out = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr[-4000:]         # the sanitizers stay silent
    lines, res, at = out.stdout.splitlines(), [], 0
    for circ in circuits:
        assert lines[at] == "rc=0", lines[at]
        head = dict(x.split("=") for x in lines[at + 1].split())
        n_rows = int(head["rows"])
        rows = []
        for line in lines[at + 2:at + 2 + n_rows]:
            f = line.split()
            rows.append((int(f[0]), int(f[1]), [(int(t.split(":")[0]), int(t.split(":")[1], 16)) for t in f[2:]]))
        assert sum(len(r[2]) for r in rows) == int(head["terms"])
        res.append(rows)
        at += 2 + n_rows
    assert at == len(lines)
    return res


def builder_rows(circ):
    n_wires, rowsA, rowsB, rowsC = circ[:4]
    M = len(rowsA)
    return [(m, c, [(s, k % R) for s, k in rows[c]]) for m, rows in enumerate((rowsA, rowsB, rowsC)) for c in range(M)]


def test_row_view_equals_the_builders_rows(exe, tmp_path):
    circuits = [sr.resolved(c)[0] for c in sr.SIDES.values()]
    circuits += [dr.DIRECTED[k][0] for k in ("seventy", "fan_64", "merged_and_cancelling", "falls_to_0")]
    circuits += [dr.random_case(i)[0] for i in range(0, dr.N_RANDOM, 5)]
    circuits += [sr.long_row(129, None)[0], sr.forward_circuit(3)[0][0]]
    circuits += [(3, [], [], []),                                                              # zero constraints
                 (3, [[(1, 2)], []], [[], [(2, 3)]], [[(1, 5), (1, 6)], []])]                  # empty rows, a constraint of three
    for circ, got in zip(circuits, rows_of(exe, tmp_path, circuits)):
        assert got == builder_rows(circ)
