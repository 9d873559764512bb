"""-m gpu : the bit rule of the witness completion (include/k16.h k16_r1cs_complete_witness_ex, k16_r1cs_boolean_wires;
csrc/r1cs_scan.hip k_r1cs_bits_filter, k_r1cs_solve_bits, k_r1cs_bits_commit) against the big-integer reference of
tests/solve_bits_reference.py.  Every case compares all counts, the three ascending lists, status, round, by and rule of every
wire and the returned bytes of every wire with the reference, runs twice and asks for equal bytes; the positions outside the
givens go in as 0xFF bytes.  What the directed circuits must give is asserted of the reference in tests/test_solve_bits_host.py."""
import ctypes as C

import numpy as np
import pytest

import determined_reference as dr
import r1cs_builder as rb
import solve_bits_reference as sb
import solve_reference as sr
from solve_bits_reference import BITS, LINEAR

pytestmark = pytest.mark.gpu

ERR_ARG = -3
FILL32 = 0xA5A5A5A5
U64, U32 = C.c_uint64, C.c_uint32


@pytest.fixture(scope="module")
def ctx():
    import k16
    c = k16.Context(0)
    yield c
    c.close()


def make(ctx, circuit, header=(0, 0, 0)):
    import k16
    n_wires, rowsA, rowsB, rowsC = circuit
    return k16.R1cs(ctx, rb.write(n_wires, rowsA, rowsB, rowsC, n_pub_out=header[0], n_pub_in=header[1], n_prv_in=header[2]))


def entry_bytes(w, given_list, junk=0xFF):
    out = np.full((len(w), 32), junk, dtype=np.uint8)
    for s in set(given_list) | {0}:
        out[s] = np.frombuffer(int(w[s]).to_bytes(32, "little"), dtype=np.uint8)
    return out.reshape(-1)


def raw(circ, wtns, given, rules, cap_infeasible=None, outputs=True):
    """k16_r1cs_complete_witness_ex: (rc, the eight counts, wtns, failed, wires, infeasible, status, round, by, rule); the buffers
    pre-filled so that what the call did not write shows; outputs=False: every optional output NULL"""
    info = circ.info()
    n_wires, M = info["n_wires"], info["n_constraints"]
    cap_infeasible = M if cap_infeasible is None else cap_infeasible
    wt = np.array(wtns, dtype=np.uint8)
    fl, wi, nf = (np.full(n + 1, FILL32, dtype=np.uint32) if outputs else None for n in (M, n_wires, M))
    st, ru = (np.full(n_wires, 0xA5, dtype=np.uint8) if outputs else None for _ in range(2))
    ro, b = (np.full(n_wires, FILL32, dtype=np.uint32) if outputs else None for _ in range(2))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    gv = np.array(list(given) + [0], dtype=np.uint32)
    ns, na, no, nfl, noc, nb, ni = (U64(77) for _ in range(7))
    nr = U32(77)
    rc = circ.ctx.L.k16_r1cs_complete_witness_ex(circ.h, ptr(wt), ptr(gv), len(given), rules, C.byref(ns), C.byref(na), C.byref(no),
                                                 C.byref(nr), C.byref(nfl), ptr(fl), M, C.byref(noc), ptr(wi), n_wires, ptr(st), ptr(ro),
                                                 ptr(b), C.byref(nb), C.byref(ni), ptr(nf), cap_infeasible, ptr(ru))
    return rc, tuple(int(x.value) for x in (ns, na, no, nr, nfl, noc, nb, ni)), wt, fl, wi, nf, st, ro, b, ru


def same_bytes(x, y):
    return x[:2] == y[:2] and all((a is None and b is None) or a.tobytes() == b.tobytes() for a, b in zip(x[2:], y[2:]))


def assert_complete(circ, case, rules=LINEAR | BITS, what=None):
    circuit, w, _, given = case
    want = sb.complete(circuit, w, given, rules)
    counts = sr.summary(want) + (want["n_by_bits"], len(want["infeasible"]))
    opened = sr.open_wires(want)
    got = raw(circ, entry_bytes(w, given), given, rules)
    rc, cnt, wt, fl, wi, nf, st, ro, b, ru = got
    assert rc == 0 and cnt == counts, (what, cnt, counts)
    assert fl[:counts[4]].tolist() == want["failed"] and (fl[counts[4]:] == FILL32).all(), what
    assert wi[:counts[2]].tolist() == opened and (wi[counts[2]:] == FILL32).all(), what
    assert nf[:counts[7]].tolist() == want["infeasible"] and (nf[counts[7]:] == FILL32).all(), what
    assert st.tolist() == want["status"], what
    assert ro.tolist() == want["round"], what
    assert b.tolist() == want["by"], what
    assert ru.tolist() == want["rule"], what
    assert wt.tobytes() == rb.witness_bytes(want["wtns"]).tobytes(), what
    assert same_bytes(got, raw(circ, entry_bytes(w, given), given, rules)), what            # the same bytes on every run
    return want, got


def run_case(ctx, case, rules=LINEAR | BITS, what=None):
    circ = make(ctx, case[0])
    try:
        return assert_complete(circ, case, rules, what)
    finally:
        circ.close()


def test_constants_are_the_headers():
    import k16
    assert (k16.SOLVE_RULE_LINEAR, k16.SOLVE_RULE_BITS) == (LINEAR, BITS) == (1, 2)


@pytest.mark.parametrize("k", sb.WIDTHS + (254, 1))
def test_widths(ctx, k):
    case, info = sb.width(k)
    want, _ = run_case(ctx, case, what=k)
    assert want["n_by_bits"] == (k if 2 <= k <= 253 else 0)


@pytest.mark.parametrize("k", (64, 65, 253))
@pytest.mark.parametrize("orient", ("B", "C"))
def test_widths_on_the_other_sides(ctx, k, orient):
    want, _ = run_case(ctx, sb.width(k, orient)[0], what=(k, orient))
    assert want["n_by_bits"] == k


@pytest.mark.parametrize("name", sb.ORIENTATIONS)
def test_orientations(ctx, name):
    case, info = sb.oriented(name)
    want, _ = run_case(ctx, case, what=name)
    assert want["n_by_bits"] == (len(info["bits"]) if info["solved"] else 0)


@pytest.mark.parametrize("name", sb.REFUSALS)
def test_refusals(ctx, name):
    case, info = sb.refusal(name)
    want, got = run_case(ctx, case, what=name)
    assert sr.open_wires(want) == sorted(info["bits"]) and want["n_by_bits"] == 0
    lin, got1 = run_case(ctx, case, rules=LINEAR, what=name)                                 # ... and changes nothing else
    assert same_bytes(got[:2] + got[2:5] + got[6:9], got1[:2] + got1[2:5] + got1[6:9])


@pytest.mark.parametrize("orient,lam", (("A", 1), ("C", 12345), ("B", sb.R - 2)))
def test_partly_given_bits(ctx, orient, lam):
    case, _ = sb.partly_given(70, [0, 5, 63, 64, 69], orient, lam)
    want, _ = run_case(ctx, case)
    assert want["n_by_bits"] == 65


def test_infeasible_rows_counts_and_the_lowest_of_them(ctx):
    case, rows, good, good_bits = sb.infeasible_rows()
    circ = make(ctx, case[0])
    try:
        want, _ = assert_complete(circ, case)
        assert want["infeasible"] == rows and len(rows) == 4
        for cap in (0, 1, 3):                                                                # the count is exact, the list is cut
            rc, cnt, _, _, _, nf, *_ = raw(circ, entry_bytes(case[1], case[3]), case[3], LINEAR | BITS, cap_infeasible=cap)
            assert rc == 0 and cnt[7] == 4 and nf[:cap].tolist() == rows[:cap] and (nf[cap:] == FILL32).all()
        res = circ.complete_witness(entry_bytes(case[1], case[3]), given=case[3], rules=LINEAR | BITS, cap_infeasible=2, want_maps=True)
        assert (res["n_infeasible"], res["infeasible"].tolist(), res["n_by_bits"]) == (4, rows[:2], len(good_bits))
        assert res["rule"].tolist() == want["rule"]
    finally:
        circ.close()


@pytest.mark.parametrize("n_known", (257, 1025))
def test_long_rows(ctx, n_known):
    want, _ = run_case(ctx, sb.long_row(n_known)[0], what=n_known)
    assert want["n_by_bits"] == 64


@pytest.mark.parametrize("stages", (1, 2, 3))
def test_alternation(ctx, stages):
    case, plan = sb.alternation(stages)
    want, (_, cnt, *_rest) = run_case(ctx, case, what=stages)
    assert cnt[3] == 2 * stages + 1 and cnt[2] == 0 and cnt[4] == 0
    for kind, wires, rnd in plan:
        assert all((want["rule"][s], want["round"][s]) == (kind, rnd) for s in wires)


@pytest.mark.parametrize("n,last,behind", sb.CONFLICTS)
def test_conflicts(ctx, n, last, behind):
    case, info = sb.conflict(n, last, behind)
    want, (_, cnt, wt, fl, _wi, _nf, _st, _ro, b, _ru) = run_case(ctx, case, what=(n, last, behind))
    assert {int(b[s]) for s in info["bits"]} == {info["row0"]} and info["row0"] == (sb.CONFLICT_BITS + 1 if behind else 0)
    assert cnt[4] == info["n_failed"] == n - 1 and fl[:n - 1].tolist() == list(range(info["row0"] + 1, info["row0"] + n))
    assert sum(int(wt[32 * s]) << i for i, s in enumerate(info["bits"])) == info["value"]


@pytest.mark.parametrize("circuit", ((70, [], [], []), (5, [[(0, 2)], [(0, 1)]], [[(0, 3)], [(0, 1)]], [[(0, 6)], [(0, 2)]])),
                         ids=("no_constraints", "no_incidences"))
def test_circuits_that_take_no_bit_level(ctx, circuit):
    """no constraint at all, and constraints over wire 0 alone (the second is broken): nothing to count, no level is taken"""
    w = [1] + [9] * (circuit[0] - 1)
    want, (_, cnt, *_rest) = run_case(ctx, (circuit, w, (0, 0, 0), [1, 2]))
    assert cnt == (0, circuit[0] - 3, 0, 0, len(want["failed"]), 0, 0, 0) and want["failed"] == ([1] if circuit[1] else [])


@pytest.mark.parametrize("i", range(sb.N_RANDOM))
def test_random_circuits(ctx, i):
    run_case(ctx, sb.random_case(i), what=i)


@pytest.mark.parametrize("i", range(sr.N_FORWARD))
def test_rules_1_is_the_existing_call(ctx, i):
    (circuit, w, header, given), _ = sr.forward_circuit(i)
    given = dr.default_seed(header) if given is None else given
    circ = make(ctx, circuit, header)
    try:
        _, got = assert_complete(circ, (circuit, w, header, given), rules=LINEAR)
        old = circ.complete_witness(entry_bytes(w, given), given=given, want_maps=True)
        new = circ.complete_witness(entry_bytes(w, given), given=given, want_maps=True, rules=LINEAR)
        for k in old:
            assert np.array_equal(old[k], new[k]), k
        assert (new["n_by_bits"], new["n_infeasible"]) == (0, 0) and new["rule"].tolist() == [int(s == sr.SOLVED) for s in old["status"]]
    finally:
        circ.close()


def test_the_object_ends_as_a_check_of_the_returned_bytes(ctx):
    case, _ = sb.alternation(2)
    circ, other = make(ctx, case[0]), make(ctx, case[0])
    try:
        res = circ.complete_witness(entry_bytes(case[1], case[3]), given=case[3], rules=LINEAR | BITS)
        other.check(res["wtns"])
        for c in range(len(case[0][1])):
            assert circ.values(c) == other.values(c) == rb.values(case[0][1], case[0][2], case[0][3], rb.witness_ints(res["wtns"].reshape(-1, 32)), c)
    finally:
        circ.close(), other.close()


def test_null_outputs_and_bad_rules(ctx):
    case, rows, _, _ = sb.infeasible_rows()
    circ = make(ctx, case[0])
    try:
        full = raw(circ, entry_bytes(case[1], case[3]), case[3], LINEAR | BITS)
        bare = raw(circ, entry_bytes(case[1], case[3]), case[3], LINEAR | BITS, outputs=False)
        assert bare[0] == 0 and bare[1] == full[1] and bare[2].tobytes() == full[2].tobytes()
        circ.check(full[2])
        for rules in (0, 2, 4, 7, 0xFFFFFFFF):
            rc, cnt, wt, *_rest = raw(circ, entry_bytes(case[1], case[3]), case[3], rules)
            assert rc == ERR_ARG and cnt == (0,) * 8 and wt.tobytes() == entry_bytes(case[1], case[3]).tobytes()
        circ.values(0)                                                                       # the object keeps the check it had
        L, n = circ.ctx.L, U64(5)
        args = (circ.h, full[2].ctypes.data_as(C.c_void_p), None, 0, 3) + tuple(C.byref(U64()) for _ in range(3)) + (C.byref(U32()),
                C.byref(U64()), None, 0, C.byref(U64()), None, 0, None, None, None)
        assert L.k16_r1cs_complete_witness_ex(*args, None, C.byref(n), None, 0, None) == ERR_ARG       # n_by_bits is required
        assert L.k16_r1cs_complete_witness_ex(*args, C.byref(n), None, None, 0, None) == ERR_ARG       # n_infeasible is required
        assert L.k16_r1cs_boolean_wires(circ.h, None, None) == ERR_ARG
    finally:
        circ.close()


@pytest.mark.parametrize("first", ("marks", "completion"))
def test_boolean_wires_and_the_two_calls_in_either_order(ctx, first):
    case = sb.random_case(3)
    circ = make(ctx, case[0])
    try:
        want = sb.boolean_wires(case[0])
        if first == "completion":
            assert_complete(circ, case)
        n, mark = circ.boolean_wires(mark=True)                                              # needs no completed check
        assert (n, mark.tolist()) == (sum(want), want) and circ.boolean_wires() == n
        assert_complete(circ, case)
        assert_complete(circ, case, rules=LINEAR)
        assert circ.boolean_wires(mark=True)[1].tolist() == want
    finally:
        circ.close()
