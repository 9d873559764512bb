"""-m gpu : the bit rule of the determinism closure (include/k16.h k16_r1cs_determined_wires_ex, k16_r1cs_held_wires;
csrc/r1cs_scan.hip k_r1cs_held, k_r1cs_det_bits) against the big-integer reference of tests/determined_bits_reference.py.  Every
case compares all counts, the ascending OPEN list, status, round, by and rule of every wire and the HELD marks with the
reference, runs twice and asks for equal bytes, and runs the reference's independent replayer on the GPU's own certificate.
What the directed circuits must give is asserted of the reference in tests/test_determined_bits_host.py."""
import ctypes as C

import numpy as np
import pytest

import determined_bits_reference as db
import determined_reference as dr
import r1cs_builder as rb
import solve_bits_reference as sb
from determined_bits_reference import BITS, PIN
from determined_reference import NONE, OPEN

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


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def raw(circ, seed, rules, cap=None, outputs=True):
    """k16_r1cs_determined_wires_ex: (rc, (n_derived, n_absent, n_open, n_rounds, n_by_bits), wires, status, round, by, rule), the
    buffers pre-filled so that what the call did not write shows; outputs=False: every optional output NULL"""
    n_wires = circ.info()["n_wires"]
    cap = n_wires if cap is None else cap
    w = np.full(max(cap, n_wires) + 1, FILL32, dtype=np.uint32) if outputs else None
    st, ru = (np.full(n_wires, 0xA5, dtype=np.uint8) if outputs else None for _ in range(2))
    ro, b = (np.full(n_wires, FILL32, dtype=np.uint32) if outputs else None for _ in range(2))
    sd = np.array(list(seed) + [0], dtype=np.uint32) if seed is not None else None       # (+ [0]: never an empty buffer)
    nd, na, no, nb = (U64(77) for _ in range(4))
    nr = U32(77)
    rc = circ.ctx.L.k16_r1cs_determined_wires_ex(circ.h, ptr(sd), 0 if seed is None else len(seed), rules, C.byref(nd), C.byref(na),
                                                 C.byref(no), C.byref(nr), ptr(w), cap, ptr(st), ptr(ro), ptr(b), C.byref(nb), ptr(ru))
    return rc, tuple(int(x.value) for x in (nd, na, no, nr, nb)), w, st, ro, b, ru


def same_bytes(x, y):
    return x[:2] == y[:2] and all((a is None and b is None) or a.tobytes() == b.tobytes() for a, b in zip(x[2:], y[2:]))


def assert_closure(circ, case, rules=PIN | BITS, what=None):
    """one call with everything asked for against the reference, twice; HELD; the replayer; the binding.  Returns (the
    reference's dict, the call's tuple)."""
    circuit, w, _, seed = case
    want = db.closure(circuit, w, seed, rules)
    n_derived, n_absent, n_open, n_rounds, n_by_bits, opened = db.summary(want)
    got = raw(circ, seed, rules)
    rc, counts, wires, st, ro, b, ru = got
    assert rc == 0 and counts == (n_derived, n_absent, n_open, n_rounds, n_by_bits), (what, counts)
    assert wires[:n_open].tolist() == opened and (wires[n_open:] == FILL32).all(), what
    assert st.tolist() == want["status"], what
    assert ro.tolist() == want["round"], what
    assert b.tolist() == want["by"], what
    assert ru.tolist() == want["rule"], what
    assert same_bytes(got, raw(circ, seed, rules)), what                                   # the same bytes on every run
    assert db.replay(circuit, w, seed, st.tolist(), ro.tolist(), b.tolist(), ru.tolist()) is None, what   # the GPU's own certificate
    held = db.held_wires(circuit, w)
    n, mark = circ.held_wires(mark=True)
    assert (n, mark.tolist()) == (sum(held), held) and circ.held_wires() == n, what
    res = circ.determined_wires(seed=seed, want_maps=True, rules=rules)                    # the binding: the same
    assert res[:4] == counts[:4] and res[4].tolist() == opened and res[8] == n_by_bits, what
    assert [res[k].tolist() for k in (5, 6, 7, 9)] == [want[k] for k in ("status", "round", "by", "rule")], what
    return want, got


def run_case(ctx, case, rules=PIN | BITS, what=None):
    """check + closure of one case on a fresh object"""
    circuit, w, header, seed = case
    circ = make(ctx, circuit, header)
    try:
        n_failed, _ = circ.check(rb.witness_bytes(w))
        assert n_failed == len(rb.check(*circuit[1:], w)), what
        return assert_closure(circ, case, rules, what)
    finally:
        circ.close()


def test_constants_are_the_headers():
    import k16
    assert (k16.DET_RULE_PIN, k16.DET_RULE_BITS) == (PIN, BITS) == (1, 2)


@pytest.mark.parametrize("k", db.WIDTHS + (254, 1))
def test_widths(ctx, k):
    """2, 63 | 64, 65, 128 | 129, 253: the lane and register boundaries of the slot layout; 254 is refused, 1 is the PIN rule's"""
    case, info = db.width(k)
    want, _ = run_case(ctx, case, what=k)
    assert want["n_by_bits"] == (k if 2 <= k <= 253 else 0)
    assert db.summary(want)[5] == (info["bits"] if k == 254 else [])


@pytest.mark.parametrize("orient", ("B", "C"))
def test_width_65_on_the_other_sides(ctx, orient):
    want, _ = run_case(ctx, db.width(65, orient)[0], what=orient)
    assert want["n_by_bits"] == 65


def test_long_row(ctx):
    """74 incidences, 3 of them outside: the gather takes two steps and compacts across them"""
    case, info = db.long_row()
    want, _ = run_case(ctx, case)
    assert want["n_by_bits"] == 3 and len(sb.merged_of(case[0])[info["row"]][0]) > 64


@pytest.mark.parametrize("name", sb.ORIENTATIONS)
def test_orientations_and_lambda(ctx, name):
    case, info = sb.oriented(name)
    want, _ = run_case(ctx, db.seeded(case), what=name)
    assert want["n_by_bits"] == (len(info["bits"]) if info["solved"] else 0)


@pytest.mark.parametrize("name", db.COEFFICIENTS)
def test_refusals_by_coefficient(ctx, name):
    case, info = db.coefficient_case(name)
    want, _ = run_case(ctx, case, what=name)
    assert want["n_by_bits"] == (4 if info["derives"] else 0)


@pytest.mark.parametrize("name", db.UNKNOWNS)
def test_refusals_by_unknowns(ctx, name):
    case, info = db.unknown_case(name)
    want, got = run_case(ctx, case, what=name)
    assert sorted(s for s, k in enumerate(want["rule"]) if k == BITS) == sorted(info["derives"])
    if not info["derives"]:                                                                # ... and changes nothing else
        _, pin = run_case(ctx, case, rules=PIN, what=name)
        assert same_bytes(got, pin)


def test_partly_seeded_bits(ctx):
    want, _ = run_case(ctx, db.partly_seeded()[0])
    assert want["n_by_bits"] == 65


@pytest.mark.parametrize("n", (2, 65))
def test_conflicts(ctx, n):
    case, info = db.conflict(n)
    want, (_, _, _, _, _, b, _) = run_case(ctx, case, what=n)
    assert {int(b[s]) for s in info["bits"]} == {info["row0"]} and want["n_by_bits"] == sb.CONFLICT_BITS


@pytest.mark.parametrize("make_case", (db.pin_bits_pin, db.pin_first), ids=("bits_pin_pin_bits", "pin_bits_pin"))
def test_alternation(ctx, make_case):
    case, plan = make_case()
    want, (_, counts, _, _, ro, _, ru) = run_case(ctx, case)
    assert {x: (int(ro[x]), int(ru[x])) for x in plan} == plan
    assert counts[2] == 0 and counts[3] == max(r for r, _ in plan.values())


def test_a_row_falls_from_2_to_0_behind_the_bit_frontier(ctx):
    case, opened, (p, q) = db.falls_to_0_behind_bits()
    want, (_, counts, wires, st, ro, b, ru) = run_case(ctx, case)
    assert wires[:counts[2]].tolist() == sorted(opened) and all(st[s] == OPEN and b[s] == NONE for s in opened)
    assert (int(ro[p]), int(ro[q]), int(ru[p]), int(ru[q])) == (1, 1, BITS, BITS)


@pytest.mark.parametrize("name", sorted(db.EMPTY))
def test_circuits_that_take_no_bit_level(ctx, name):
    circuit = db.EMPTY[name]
    w = [1] + [9] * (circuit[0] - 1)
    want, (_, counts, *_rest) = run_case(ctx, (circuit, w, (0, 0, 0), [1, 2]))
    assert counts == (0, circuit[0] - 3, 0, 0, 0)


@pytest.mark.parametrize("block", range(4))
def test_random_circuits(ctx, block):
    for i in range(block * 10, block * 10 + 10):
        run_case(ctx, db.random_case(i), what=i)


@pytest.mark.parametrize("block", range(2))
def test_satisfying_circuits(ctx, block):
    for i in range(block * 20, block * 20 + 20):
        run_case(ctx, db.satisfying_case(i), what=i)


def test_random_circuits_are_not_degenerate():
    """the reference's verdict; no device needed"""
    got = [db.closure(*(db.random_case(i)[k] for k in (0, 1, 3))) for i in range(db.N_RANDOM)]
    assert sum(1 for r in got if r["n_by_bits"]) >= 10 and sum(1 for r in got if OPEN in r["status"]) >= 20
    assert sum(1 for r in got if PIN in r["rule"] and BITS in r["rule"]) >= 5


@pytest.mark.parametrize("i", range(0, dr.N_RANDOM, 5))
def test_rules_1_is_the_existing_call(ctx, i):
    """byte for byte, on the closure's own random circuits (default and listed seeds)"""
    from test_gpu_determined import raw as raw_old
    circuit, w, header, seed = dr.random_case(i)
    circ = make(ctx, circuit, header)
    try:
        circ.check(rb.witness_bytes(w))
        old = raw_old(circ, seed, circuit[0])
        rc, counts, wires, st, ro, b, ru = raw(circ, seed, PIN)
        assert rc == old[0] == 0 and counts == old[1] + (0,)
        assert all(x.tobytes() == y.tobytes() for x, y in zip((wires, st, ro, b), old[2:]))
        assert ru.tolist() == [int(s == dr.DERIVED) for s in st.tolist()]
        status, rounds, by = dr.closure(circuit, w, dr.default_seed(header) if seed is None else seed)
        assert (st.tolist(), ro.tolist(), b.tolist()) == (status, rounds, by)
        got = circ.determined_wires(seed=seed, want_maps=True, rules=PIN)
        plain = circ.determined_wires(seed=seed, want_maps=True)
        assert got[:4] == plain[:4] and all(x.tobytes() == y.tobytes() for x, y in zip(got[4:8], plain[4:])) and got[8] == 0
    finally:
        circ.close()


def test_arguments_and_state(ctx):
    import k16
    case, plan = db.pin_bits_pin()
    circuit, w, header, seed = case
    circ = make(ctx, circuit, header)
    try:
        # before any check
        rc, counts, wires, st, ro, b, ru = raw(circ, seed, PIN | BITS)
        assert (rc, counts) == (ERR_ARG, (0,) * 5) and (st == 0xA5).all() and (ru == 0xA5).all() and (wires == FILL32).all()
        n = U64(77)
        assert circ.ctx.L.k16_r1cs_held_wires(circ.h, C.byref(n), None) == ERR_ARG and n.value == 0
        with pytest.raises(k16.K16Error) as e:
            circ.held_wires()
        assert e.value.rc == ERR_ARG
        assert circ.check(rb.witness_bytes(w))[0] == 0
        want, full = assert_closure(circ, case)
        # bad rules: an error before anything is launched, and the object keeps its check
        for rules in (0, 2, 4, 7, 0xFFFFFFFF):
            rc, counts, wires, st, ro, b, ru = raw(circ, seed, rules)
            assert (rc, counts) == (ERR_ARG, (0,) * 5), rules
            assert (st == 0xA5).all() and (ru == 0xA5).all() and (ro == FILL32).all() and (b == FILL32).all() and (wires == FILL32).all()
            with pytest.raises(k16.K16Error) as e:
                circ.determined_wires(seed=seed, rules=rules)
            assert e.value.rc == ERR_ARG
        assert same_bytes(full, raw(circ, seed, PIN | BITS))
        # a seed wire out of range, as the existing call
        rc, counts, *_rest = raw(circ, [circuit[0]], PIN | BITS)
        assert (rc, counts) == (ERR_ARG, (0,) * 5)
        # NULL outputs: the counts stay; n_by_bits is required
        bare = raw(circ, seed, PIN | BITS, outputs=False)
        assert bare[:2] == full[:2]
        L, nd, nr = circ.ctx.L, U64(), U32()
        assert L.k16_r1cs_determined_wires_ex(circ.h, None, 0, 3, C.byref(nd), C.byref(nd), C.byref(nd), C.byref(nr), None, 0, None, None,
                                              None, None, None) == ERR_ARG
        assert L.k16_r1cs_determined_wires_ex(None, None, 0, 3, C.byref(nd), C.byref(nd), C.byref(nd), C.byref(nr), None, 0, None, None,
                                              None, C.byref(nd), None) == ERR_ARG
        assert L.k16_r1cs_held_wires(circ.h, None, None) == ERR_ARG and L.k16_r1cs_held_wires(None, C.byref(nd), None) == ERR_ARG
        # caps: nothing behind min(n_open, cap) is touched (the PIN rule alone leaves wires open here)
        pin = raw(circ, seed, PIN)
        assert pin[1][2] > 2
        for cap in (0, 1, 2):
            rc, counts, wires, *_rest = raw(circ, seed, PIN, cap=cap)
            assert rc == 0 and counts == pin[1] and wires[:cap].tolist() == pin[2][:cap].tolist() and (wires[cap:] == FILL32).all()
        # the rule byte alone, without the rounds
        n_wires = circuit[0]
        ru, nb = np.full(n_wires, 0xA5, dtype=np.uint8), U64()
        sd = np.array(seed, dtype=np.uint32)
        assert L.k16_r1cs_determined_wires_ex(circ.h, ptr(sd), len(seed), 3, C.byref(nd), C.byref(nd), C.byref(nd), C.byref(nr), None, 0,
                                              None, None, None, C.byref(nb), ptr(ru)) == 0
        assert ru.tolist() == want["rule"] and nb.value == want["n_by_bits"]
    finally:
        circ.close()


@pytest.mark.parametrize("order", ["ex_first", "held_first", "after_the_old_call", "after_the_scans", "after_a_completion"])
def test_calls_in_any_order(ctx, order):
    """whichever call comes first makes the stages the others share: the closure's bytes are the same behind each, and the other
    calls' bytes are the same behind the closure"""
    from test_gpu_complete_bits import entry_bytes
    case = db.generated(8, 5)                                                              # (its completion is its witness)
    circuit, w, header, seed = case
    circ, other = make(ctx, circuit, header), make(ctx, circuit, header)
    try:
        wb = rb.witness_bytes(w)
        circ.check(wb), other.check(wb)
        plain = other.determined_wires(seed=seed, want_maps=True)                          # an object that never sees the new calls
        unbound, second = other.unbound_wires(status=True), other.second_values(status=True)
        solved = other.complete_witness(entry_bytes(w, seed), given=seed, rules=3, want_maps=True)
        if order == "held_first":
            assert circ.held_wires() == sum(db.held_wires(circuit, w))
        if order == "after_the_old_call":
            circ.determined_wires(seed=seed)
        if order == "after_the_scans":
            circ.unbound_wires(), circ.second_values()
        if order == "after_a_completion":                                                  # (it leaves the check of its own result: w)
            got = circ.complete_witness(entry_bytes(w, seed), given=seed, rules=3, want_maps=True)
            assert all(np.array_equal(got[k], solved[k]) for k in solved)
        _, first = assert_closure(circ, case)
        again = circ.determined_wires(seed=seed, want_maps=True)
        assert plain[:4] == again[:4] and all(x.tobytes() == y.tobytes() for x, y in zip(plain[4:], again[4:]))
        assert all(np.array_equal(x, y) for x, y in zip(circ.unbound_wires(status=True), unbound))
        got2 = circ.second_values(status=True)
        assert got2[0] == second[0] and got2[1].tolist() == second[1].tolist() and got2[2] == second[2] and got2[3].tolist() == second[3].tolist()
        got = circ.complete_witness(entry_bytes(w, seed), given=seed, rules=3, want_maps=True)
        assert all(np.array_equal(got[k], solved[k]) for k in solved)
        assert same_bytes(first, raw(circ, seed, PIN | BITS))
    finally:
        circ.close(), other.close()


def test_the_closure_names_what_the_completion_solves(ctx):
    """section 10f's generated circuit at 8 decompositions of 5 bits: the completion (rules = 3) from the seed's values, then the
    closure (rules = 3) on the check it leaves: equal status, round and by maps, nothing OPEN; the PIN rule alone: all OPEN"""
    from test_gpu_complete_bits import entry_bytes
    case = db.generated(8, 5)
    circuit, w, header, seed = case
    circ = make(ctx, circuit, header)
    try:
        solved = circ.complete_witness(entry_bytes(w, seed), given=seed, rules=3, want_maps=True)
        assert solved["wtns"].tobytes() == rb.witness_bytes(w).tobytes() and solved["n_open"] == 0 and solved["n_failed"] == 0
        want, (_, counts, _, st, ro, b, ru) = assert_closure(circ, case)
        assert counts == (56, 0, 0, 3, 40)
        assert all(np.array_equal(x, solved[k]) for x, k in ((st, "status"), (ro, "round"), (b, "by"), (ru, "rule")))
        assert raw(circ, seed, PIN)[1] == (0, 0, 56, 0, 0)
    finally:
        circ.close()


def test_a_witness_of_the_prover_s(ctx, tmp_path):
    """HELD and the closure read the check's sums and verdicts, never the witness: check_mem, check_file and a prove call on the
    attached object leave the same bytes"""
    from test_gpu_second_values import R_INJ, S_INJ, finding
    from test_gpu_setup import Made
    circuit, w = finding()                                                # y public, x x = y, a lone boolean b, a pinned z
    m = Made(ctx, tmp_path, circuit, w)
    try:
        plain, seed = circuit[:4], [1]
        case = (plain, w, (0, 0, 0), seed)
        assert m.circ.check(m.witness)[0] == 0
        _, from_mem = assert_closure(m.circ, case, what="check_mem")
        held = m.circ.held_wires(mark=True)[1].tolist()
        assert m.circ.check_file(m.wt)[0] == 0
        from_file = raw(m.circ, seed, 3)
        m.p.set_r1cs(m.circ)
        assert m.p.prove_mem(m.witness, R_INJ, S_INJ)
        from_prove = raw(m.circ, seed, 3)
        assert m.circ.held_wires(mark=True)[1].tolist() == held == db.held_wires(plain, w)
        assert m.p.prove_mem(m.witness, R_INJ, S_INJ)                     # and the prover goes on
        for other in (from_file, from_prove, raw(m.circ, seed, 3)):
            assert other[0] == 0 and same_bytes(from_mem, other)
        m.p.set_r1cs(None)
    finally:
        m.close()


def free_device_bytes():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def marked_bits(n):
    """n wires, each with its own b (b - 1) = 0 and nothing else: n marking rows, n incidences, nothing derived from wire 0"""
    rows = dr.Rows()
    for b in range(1, n + 1):
        rows.mul(dr.v(b), dr.v(b) + dr.const(-1), [])
    return rows.circuit(n + 1), [1] + [b & 1 for b in range(1, n + 1)]


def test_only_the_bit_rule_pays_for_the_bit_rule(ctx):
    """along three call orders: the existing closure call, the scans and the check allocate what they do on an object that never
    sees the new calls; the new buffers come with the first call that asks for the bit rule (or for HELD), every call behind it
    adds nothing, rules = 1 through the new entry adds nothing at all, and destroying the object returns everything.
    hipMemGetInfo moves in steps of 2 MB.  On 300,000 marked bits the new stage (8 bytes a marking row, 4 a constraint, 1 a
    wire: 3.9 MB) and the index (4 bytes a constraint, 4 an incidence: 2.4 MB) are each more than a step: either of them on an
    old path would show."""
    n, step = 300000, 2 << 20
    circuit, w = marked_bits(n)
    image, wb, seed = rb.write(*circuit), rb.witness_bytes(w), []

    def create():
        import k16
        return k16.R1cs(ctx, image)

    def took_by(call):
        before = free_device_bytes()
        call()
        return before - free_device_bytes()

    warm = create()                                                       # (the first kernels of a process load their code)
    warm.check(wb), warm.unbound_wires(), warm.second_values()
    assert warm.held_wires() == n and warm.determined_wires(seed=seed, cap=0, rules=PIN | BITS)[:4] == (0, 0, n, 0)
    warm.close()

    def old_calls(circ):
        """the existing closure call, both scans, a check: the bytes each of them took"""
        return [took_by(call) for call in (lambda: circ.determined_wires(seed=seed, cap=0), circ.unbound_wires, circ.second_values,
                                           lambda: circ.check(wb))]

    def steps(order):
        start = free_device_bytes()
        circ = create()
        circ.check(wb)
        took = {"create_and_check": start - free_device_bytes()}
        if order == "old_first":
            took["old"] = old_calls(circ)
        if order == "held_first":
            took["held"] = took_by(circ.held_wires)
        took["rules_1"] = took_by(lambda: circ.determined_wires(seed=seed, cap=0, rules=PIN))
        took["rules_3"] = took_by(lambda: circ.determined_wires(seed=seed, cap=0, rules=PIN | BITS))
        took["again"] = took_by(lambda: (circ.determined_wires(seed=seed, cap=0, rules=PIN | BITS, want_maps=True), circ.held_wires(mark=True),
                                         circ.determined_wires(seed=seed, cap=0, rules=PIN)))
        took["old_behind"] = old_calls(circ)
        circ.close()
        assert free_device_bytes() == start                               # nothing is left behind
        print(order, took)
        return took

    plain_start = free_device_bytes()
    circ = create()
    circ.check(wb)
    plain_made = plain_start - free_device_bytes()
    plain = old_calls(circ)                                               # an object that never sees the new calls
    assert old_calls(circ) == [0, 0, 0, 0]
    circ.close()
    assert free_device_bytes() == plain_start
    print("plain", plain_made, plain)
    assert plain[0] > 0 and plain[1] == 0 and plain[2] > 0 and plain[3] == 0      # (the list comes with the closure, the first here)
    for order in ("old_first", "ex_first", "held_first"):
        took = steps(order)
        assert took["create_and_check"] == plain_made, order
        assert took["again"] == 0, order
        if order == "old_first":
            assert took["old"] == plain and took["rules_1"] == 0, order           # the new entry with rules = 1 is the old call
            assert took["rules_3"] > step, order                                  # the new stage and the index: with the first BITS call
            assert took["old_behind"] == [0, 0, 0, 0], order
        else:
            # ... and allocates what the old call does; behind it the second-value scan's own buffers, as ever
            assert took["rules_1"] == plain[0], order
            assert took["old_behind"] == [0, 0, plain[2], 0], order
            if order == "ex_first":
                assert took["rules_3"] > step, order
            else:                                                                 # HELD made the new stage; the BITS call adds the index
                assert took["held"] > step and took["rules_3"] > 0, order
