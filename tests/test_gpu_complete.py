"""-m gpu : the witness completion (include/k16.h k16_r1cs_complete_witness; csrc/r1cs_scan.hip k_r1cs_solve_mask, _derive,
_commit, _close on the closure's frontier) against the big-integer reference of tests/solve_reference.py.  Every case compares
all counts, both ascending lists, the status, round and by of every wire and the returned bytes of every wire with the
reference; the positions outside the givens go in as 0xFF bytes.  What the directed circuits must give is stated by hand and
asserted of the reference in tests/test_solve_host.py."""
import ctypes as C

import numpy as np
import pytest

import determined_reference as dr
import pymodel as pm
import r1cs_builder as rb
import solve_reference as sr
import unbound_reference as ur
from solve_reference import ABSENT, GIVEN, NONE, OPEN, SOLVED

pytestmark = pytest.mark.gpu

R = pm.R
ERR_ARG, ERR_FORMAT = -3, -5
FILL32 = 0xA5A5A5A5


@pytest.fixture(scope="module")
def ctx():
    import k16
    c = k16.Context(0)
    yield c
    c.close()


def make(ctx, circuit, header):
    import k16
    n_wires, rowsA, rowsB, rowsC = circuit
    return k16.R1cs(ctx, rb.write(n_wires, rowsA, rowsB, rowsC, n_pub_out=header[0], n_pub_in=header[1], n_prv_in=header[2]))


def entry_bytes(w, given_list, junk=0xFF):
    """the witness as the call gets it: the given values, wire 0, and junk bytes everywhere else"""
    out = np.full((len(w), 32), junk, dtype=np.uint8)
    for s in set(given_list) | {0}:
        out[s] = np.frombuffer(int(w[s]).to_bytes(32, "little"), dtype=np.uint8)
    return out.reshape(-1)


def raw(circ, wtns, given, cap, cap_failed, failed=True, wires=True, status=True, rounds=True, by=True):
    """k16_r1cs_complete_witness with any optional output left out: (rc, (n_solved, n_absent, n_open, n_rounds, n_failed,
    n_open_constraints), wtns, failed, wires, status, round, by); the buffers pre-filled so that what the call did not write shows"""
    info = circ.info()
    n_wires, M = info["n_wires"], info["n_constraints"]
    wt = np.array(wtns, dtype=np.uint8)
    fl = np.full(max(cap_failed, M) + 1, FILL32, dtype=np.uint32) if failed else None
    wi = np.full(max(cap, n_wires) + 1, FILL32, dtype=np.uint32) if wires else None
    st = np.full(n_wires, 0xA5, dtype=np.uint8) if status else None
    ro = np.full(n_wires, FILL32, dtype=np.uint32) if rounds else None
    b = np.full(n_wires, FILL32, dtype=np.uint32) if by else None
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    gv = np.array(list(given) + [0], dtype=np.uint32) if given is not None else None      # (+ [0]: never an empty buffer)
    ns, na, no, nf, noc, nr = tuple(C.c_uint64(77) for _ in range(5)) + (C.c_uint32(77),)
    rc = circ.ctx.L.k16_r1cs_complete_witness(circ.h, ptr(wt), ptr(gv), 0 if given is None else len(given), C.byref(ns), C.byref(na),
                                              C.byref(no), C.byref(nr), C.byref(nf), ptr(fl), cap_failed, C.byref(noc), ptr(wi), cap,
                                              ptr(st), ptr(ro), ptr(b))
    return rc, tuple(int(x.value) for x in (ns, na, no, nr, nf, noc)), wt, fl, wi, st, ro, b


def same_bytes(x, y):
    return x[:2] == y[:2] and all((a is None and b is None) or a.tobytes() == b.tobytes() for a, b in zip(x[2:], y[2:]))


def assert_complete(circ, circuit, w, given, given_list, what=None):
    """one call with everything asked for against the reference; given: what the call gets (None: the default), given_list: the
    same as wires.  Returns (the reference's result, the raw call's)."""
    want = sr.complete(circuit, w, given_list)
    counts, opened = sr.summary(want), sr.open_wires(want)
    got = raw(circ, entry_bytes(w, given_list), given, circuit[0], len(circuit[1]))
    rc, cnt, wt, fl, wi, st, ro, b = got
    assert rc == 0 and cnt == counts, (what, cnt, counts)
    assert fl[:counts[4]].tolist() == want["failed"] and (fl[counts[4]:] == FILL32).all(), what
    assert wi[:counts[2]].tolist() == opened and (wi[counts[2]:] == FILL32).all(), what
    assert st.tolist() == want["status"], what
    assert ro.tolist() == want["round"], what
    assert b.tolist() == want["by"], what
    assert wt.tobytes() == rb.witness_bytes(want["wtns"]).tobytes(), what
    res = circ.complete_witness(entry_bytes(w, given_list), given=given, want_maps=True)         # the binding: the same
    assert tuple(res[k] for k in ("n_solved", "n_absent", "n_open", "n_rounds", "n_failed", "n_open_constraints")) == counts, what
    assert res["failed"].tolist() == want["failed"] and res["wires"].tolist() == opened, what
    assert (res["status"].tolist(), res["round"].tolist(), res["by"].tolist()) == (want["status"], want["round"], want["by"]), what
    assert res["wtns"].tobytes() == wt.tobytes(), what
    return want, got


def run_case(ctx, c, what=None):
    circuit, w, header, given = c
    given_list = dr.default_seed(header) if given is None else given
    circ = make(ctx, circuit, header)
    try:
        return assert_complete(circ, circuit, w, given, given_list, what)
    finally:
        circ.close()


def test_constants_are_the_headers():
    import k16
    assert (k16.SOLVE_GIVEN, k16.SOLVE_SOLVED, k16.SOLVE_ABSENT, k16.SOLVE_OPEN) == (GIVEN, SOLVED, ABSENT, OPEN) == (0, 1, 2, 3)
    assert (k16.SOLVE_GIVEN, k16.SOLVE_SOLVED, k16.SOLVE_ABSENT, k16.SOLVE_OPEN) == (k16.DET_SEED, k16.DET_DERIVED, k16.DET_ABSENT, k16.DET_OPEN)


@pytest.mark.parametrize("name", sorted(sr.SIDES))
def test_sides_of_the_unknown(ctx, name):
    want, _ = run_case(ctx, sr.SIDES[name], name)
    for wire, (status, rnd, by, value) in sr.SIDES_EXPECTED[name].items():
        assert (want["status"][wire], want["round"][wire], want["by"][wire], want["wtns"][wire]) == (status, rnd, by, value % R)


@pytest.mark.parametrize("name", sorted(dr.DIRECTED))
def test_directed_circuits_of_the_closure(ctx, name):
    run_case(ctx, dr.DIRECTED[name], name)


def test_chain_of_300_takes_300_rounds_and_gives_the_witness(ctx):
    circuit, w, header, _ = dr.DIRECTED["chain_300"]
    circ = make(ctx, circuit, header)
    try:
        res = circ.complete_witness(entry_bytes(w, [1]), want_maps=True)
        assert (res["n_solved"], res["n_open"], res["n_rounds"], res["n_failed"], res["n_open_constraints"]) == (300, 0, 300, 0, 0)
        assert res["round"].tolist() == [0, 0] + list(range(1, 301)) and res["by"].tolist() == [NONE, NONE] + list(range(300))
        assert res["wtns"].tobytes() == rb.witness_bytes(w).tobytes()
    finally:
        circ.close()


def test_broken_link_rederives_the_corrupted_wire(ctx):
    want, _ = run_case(ctx, dr.DIRECTED["broken_link"])
    assert [s for s, k in enumerate(want["status"]) if k == SOLVED] == [2, 3, 4] and want["failed"] == []
    assert want["wtns"] == dr.DIRECTED["repaired_link"][1]


@pytest.mark.parametrize("n", sr.LONG_ROWS)
def test_long_rows(ctx, n):
    """(k_1 x_1 + .. + k_n x_n) s = y: n + 2 terms in the candidate's three rows, on both sides of SOLVE_SHORT and of the wave;
    the unknown behind the sum, and inside it at the first, a middle and the last position"""
    for at in (None, 0, n // 2, n - 1):
        circuit, w, header, given = sr.long_row(n, at)
        want, _ = run_case(ctx, (circuit, w, header, given), (n, at))
        assert want["wtns"] == w and sr.summary(want) == (1, 0, 0, 1, 0, 0)


@pytest.mark.parametrize("n,lowest_last,deep", sr.CONFLICTS, ids=lambda x: str(int(x)))
def test_conflicts_commit_the_lowest_constraints_value(ctx, n, lowest_last, deep):
    circuit, w, header, given = sr.conflict(n, lowest_last, deep)
    x = n + 2 if lowest_last else 1
    circ = make(ctx, circuit, header)
    try:
        want, first = assert_complete(circ, circuit, w, given, given)
        assert (want["by"][x], want["wtns"][x], want["failed"]) == (0, w[x], list(range(1, n)))
        again = raw(circ, entry_bytes(w, given), given, circuit[0], len(circuit[1]))
        assert same_bytes(first, again)                                    # the same bytes on every run
    finally:
        circ.close()


@pytest.mark.parametrize("i", range(sr.N_FORWARD))
def test_forward_circuits_are_completed(ctx, i):
    (circuit, w, header, given), depth = sr.forward_circuit(i)
    circ = make(ctx, circuit, header)
    try:
        want, got = assert_complete(circ, circuit, w, None, dr.default_seed(header), i)
        assert got[1][2:5] == (0, depth, 0) and got[2].tobytes() == rb.witness_bytes(w).tobytes()
        assert circ.check(got[2])[0] == 0
    finally:
        circ.close()


@pytest.mark.parametrize("block", range(4))
def test_random_circuits(ctx, block):
    """40 random circuits, satisfying and corrupted witnesses as the source of the given values, default and listed givens"""
    for i in range(block * 10, block * 10 + 10):
        run_case(ctx, dr.random_case(i), i)


# ---------------------------------------------------------------- the contract
def test_givens_defaults_duplicates_caps_and_null_outputs(ctx):
    circuit, w, header, _ = dr.DIRECTED["free_but_counted"]               # 3 solved, wires 6 and 7 open, constraint 3 open
    n_wires, M = circuit[0], len(circuit[1])
    default = dr.default_seed(header)
    circ = make(ctx, circuit, header)
    try:
        wb = entry_bytes(w, default)
        by_null = raw(circ, wb, None, n_wires, M)
        assert by_null[0] == 0 and by_null[1] == (3, 0, 2, 3, 0, 1)
        for given in (default, default[1:], default[::-1], default + default + [default[-1]]):
            assert same_bytes(by_null, raw(circ, wb, given, n_wires, M)), given
        assert_complete(circ, circuit, w, [], [0])                         # an empty list is wire 0 alone
        for cap in (0, 1, 2, 3, n_wires + 70):                             # nothing behind min(n_open, cap) is touched
            got = raw(circ, wb, None, cap, M)
            k = min(cap, 2)
            assert got[0] == 0 and got[1] == by_null[1] and got[4][:k].tolist() == [6, 7][:k] and (got[4][k:] == FILL32).all(), cap
            assert circ.complete_witness(wb, cap=cap)["wires"].tolist() == [6, 7][:k]
        for on in ((0, 0, 0, 0, 0), (1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1), (1, 0, 1, 1, 0)):
            got = raw(circ, wb, None, n_wires, M, *on)
            assert got[:2] == by_null[:2] and got[2].tobytes() == by_null[2].tobytes(), on
            for k in range(5):
                assert (got[3 + k] is None) if not on[k] else (got[3 + k].tobytes() == by_null[3 + k].tobytes()), (on, k)
        n64, n32 = C.c_uint64(), C.c_uint32()
        L, q, p = circ.ctx.L, C.byref(n64), wb.ctypes.data_as(C.c_void_p)
        assert L.k16_r1cs_complete_witness(circ.h, p, None, 0, None, q, q, C.byref(n32), q, None, 0, q, None, 0, None, None, None) == ERR_ARG
        assert L.k16_r1cs_complete_witness(circ.h, p, None, 0, q, q, q, None, q, None, 0, q, None, 0, None, None, None) == ERR_ARG
        assert L.k16_r1cs_complete_witness(circ.h, p, None, 0, q, q, q, C.byref(n32), None, None, 0, q, None, 0, None, None, None) == ERR_ARG
        assert L.k16_r1cs_complete_witness(circ.h, None, None, 0, q, q, q, C.byref(n32), q, None, 0, q, None, 0, None, None, None) == ERR_ARG
        assert L.k16_r1cs_complete_witness(circ.h, p, None, 2, q, q, q, C.byref(n32), q, None, 0, q, None, 0, None, None, None) == ERR_ARG
        assert L.k16_r1cs_complete_witness(None, p, None, 0, q, q, q, C.byref(n32), q, None, 0, q, None, 0, None, None, None) == ERR_ARG
    finally:
        circ.close()


def test_cap_failed_below_the_count(ctx):
    circuit, w, header, given = sr.conflict(65)
    circ = make(ctx, circuit, header)
    try:
        wb = entry_bytes(w, given)
        for cap_failed in (0, 1, 63, 64, 200):
            got = raw(circ, wb, given, circuit[0], cap_failed)
            k = min(cap_failed, 64)
            assert got[0] == 0 and got[1][4] == 64 and got[3][:k].tolist() == list(range(1, 1 + k)) and (got[3][k:] == FILL32).all()
            assert circ.complete_witness(wb, given=given, cap_failed=cap_failed)["failed"].tolist() == list(range(1, 1 + k))
    finally:
        circ.close()


def test_header_inputs_beyond_the_wires_are_refused(ctx):
    import k16
    circuit, w, header, _ = dr.DIRECTED["chain_3"]
    circ = make(ctx, circuit, (0, 1, circuit[0]))
    try:
        with pytest.raises(k16.K16Error) as e:
            circ.complete_witness(rb.witness_bytes(w))
        assert e.value.rc == ERR_ARG
        assert circ.complete_witness(entry_bytes(w, [1]), given=[1])["n_solved"] == 3
    finally:
        circ.close()


def untouched(got, wb):
    rc, counts, wt, fl, wi, st, ro, b = got
    return (wt.tobytes() == wb.tobytes() and (fl == FILL32).all() and (wi == FILL32).all() and (st == 0xA5).all() and (ro == FILL32).all()
            and (b == FILL32).all() and counts == (0, 0, 0, 0, 0, 0))


def test_refused_givens_leave_the_buffers_and_no_completed_check(ctx):
    import k16
    circuit, w, header, _ = dr.DIRECTED["diamond"]
    n_wires, M = circuit[0], len(circuit[1])
    circ = make(ctx, circuit, header)
    try:
        wb = entry_bytes(w, [1])
        good = raw(circ, wb, None, n_wires, M)
        assert good[0] == 0 and circ.values(0) == rb.values(*circuit[1:], w, 0)
        for given in ([n_wires], [1, 0xFFFFFFFF], [n_wires + 63]):         # a given wire >= nWires
            assert circ.check(rb.witness_bytes(w))[0] == 0
            got = raw(circ, wb, given, n_wires, M)
            assert got[0] == ERR_ARG and untouched(got, wb), given
            with pytest.raises(k16.K16Error) as e:                         # after an error: no completed check
                circ.values(0)
            assert e.value.rc == ERR_ARG
        bad_value, bad_one = np.array(wb), np.array(wb)
        bad_value[32:64] = np.frombuffer(R.to_bytes(32, "little"), dtype=np.uint8)            # the given wire 1 holds r
        bad_one[0] = 2                                                                           # wire 0 holds 2
        for bad in (bad_value, bad_one, entry_bytes(w, [1], junk=0xFF) | 0xFF):                  # ... and everything 0xFF
            assert circ.check(rb.witness_bytes(w))[0] == 0
            got = raw(circ, bad, None, n_wires, M)
            assert got[0] == ERR_FORMAT and untouched(got, bad)
            with pytest.raises(k16.K16Error) as e:
                circ.values(0)
            assert e.value.rc == ERR_ARG
            with pytest.raises(k16.K16Error) as e:
                circ.unbound_wires()
            assert e.value.rc == ERR_ARG
        assert same_bytes(good, raw(circ, wb, None, n_wires, M))           # an error moved nothing
        # values >= r outside the givens are ignored: r itself, 2^256 - 1 and small junk give the same bytes
        for junk in (0x00, 0x01, 0xFF):
            assert same_bytes(good, raw(circ, entry_bytes(w, [1], junk=junk), None, n_wires, M)), junk
        over = np.array(wb)
        over[64:96] = np.frombuffer(R.to_bytes(32, "little"), dtype=np.uint8)
        assert same_bytes(good, raw(circ, over, None, n_wires, M))
    finally:
        circ.close()


@pytest.mark.parametrize("i", [3, 8, 20, 21])
def test_the_object_is_left_as_a_check_of_the_returned_assignment(ctx, i):
    """no check beforehand; afterwards values(c), the scans and the closure read the sums of the RETURNED assignment, and the
    closure with the same seed derives at least what was solved"""
    import second_value_reference as sv
    circuit, w, header, given = dr.random_case(i)
    given_list = dr.default_seed(header) if given is None else given
    circ = make(ctx, circuit, header)
    try:
        want, got = assert_complete(circ, circuit, w, given, given_list, i)
        out = want["wtns"]
        for c in range(len(circuit[1])):
            assert circ.values(c) == rb.values(*circuit[1:], out, c), (i, c)
        assert circ.unbound_wires(status=True)[4].tolist() == ur.classify(*circuit, out)
        assert circ.second_values(status=True)[3].tolist() == sv.classify(*circuit, out)[0]
        det = circ.determined_wires(seed=given, want_maps=True)
        status, rounds, by = dr.closure(circuit, out, given_list)
        assert (det[5].tolist(), det[6].tolist(), det[7].tolist()) == (status, rounds, by)
        if want["failed"] == []:                                           # (a broken constraint derives nothing in the closure)
            assert all(status[s] == dr.DERIVED for s, k in enumerate(want["status"]) if k == SOLVED)
        # the same object under check_mem of the returned bytes: the same scans
        assert circ.check(got[2])[0] == len(rb.check(*circuit[1:], out))
        again = circ.determined_wires(seed=given, want_maps=True)
        assert det[:4] == again[:4] and all(a.tobytes() == b.tobytes() for a, b in zip(det[4:], again[4:]))
    finally:
        circ.close()


def test_two_calls_with_different_givens_on_one_object(ctx):
    circuit, w, header, _ = dr.DIRECTED["free_but_counted"]
    circ = make(ctx, circuit, header)
    try:
        for given in ([1, 2], [1, 2, 6], [1], [1, 2]):
            assert_complete(circ, circuit, w, given, given, given)
    finally:
        circ.close()


def test_whichever_call_makes_the_device_list(ctx):
    """the completion first, then the scans; and behind them: the same bytes"""
    circuit, w, header, given = dr.random_case(22)
    given_list = dr.default_seed(header) if given is None else given
    first = run_case(ctx, (circuit, w, header, given))[1]
    circ = make(ctx, circuit, header)
    try:
        circ.check(rb.witness_bytes(w)), circ.unbound_wires(), circ.second_values(), circ.determined_wires(seed=given)
        assert same_bytes(first, raw(circ, entry_bytes(w, given_list), given, circuit[0], len(circuit[1])))
    finally:
        circ.close()


def test_complete_then_prove_and_a_completion_between_two_proofs(ctx, tmp_path):
    """out = in^3 + 5 over wires 1 out (public output), 2 in (public input), 3 t: the input alone gives the witness, the witness
    gives the proof; on the attached object a completion between two prove calls leaves last_check and the next proof alone"""
    from test_gpu_second_values import R_INJ, S_INJ
    from test_gpu_setup import Made
    x = 7
    rowsA, rowsB, rowsC = [[(2, 1)], [(3, 1)]], [[(2, 1)], [(2, 1)]], [[(3, 1)], [(1, 1), (0, R - 5)]]
    w = [1, x ** 3 + 5, x, x * x]
    m = Made(ctx, tmp_path, (4, rowsA, rowsB, rowsC, 1, 1), w)
    try:
        res = m.circ.complete_witness(entry_bytes(w, [2]), given=[2])          # (the fixture's header calls every private wire an input)
        assert (res["n_solved"], res["n_open"], res["n_failed"], res["n_rounds"]) == (2, 0, 0, 2)
        assert res["wtns"].tobytes() == m.witness.tobytes()
        proof = m.p.prove_mem(res["wtns"], R_INJ, S_INJ)                    # complete -> prove_mem
        assert proof
        m.p.set_r1cs(m.circ)
        assert m.p.prove_mem(res["wtns"], R_INJ, S_INJ) == proof
        before = m.p.last_check()
        assert before[0] == 1
        other = m.circ.complete_witness(entry_bytes([1, 0, 3, 0], [2]), given=[2])    # between two prove calls, another input
        assert other["n_failed"] == 0 and rb.witness_ints(other["wtns"].reshape(-1, 32)) == [1, 32, 3, 9]
        assert m.p.last_check() == before
        assert m.p.prove_mem(res["wtns"], R_INJ, S_INJ) == proof and m.p.last_check()[0] == 1
        m.p.set_r1cs(None)
    finally:
        m.close()
