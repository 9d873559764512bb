"""-m gpu : the second-value scan (include/k16.h k16_r1cs_second_values; csrc/r1cs_scan.hip k_r1cs_kinds, k_r1cs_agree,
k_r1cs_shifts) against the big-integer reference of tests/second_value_reference.py.  Every case compares the class of every
wire, the count, the ascending list and the shifts' bytes with the reference; what each directed circuit's classes and shifts
must be is stated by hand there and asserted of the reference in tests/test_second_value_host.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import pymodel as pm
import r1cs_builder as rb
import second_value_reference as sv
import unbound_reference as ur
import valid_key_builder as vkb
from second_value_reference import BOUND, TWO_VALUED

pytestmark = pytest.mark.gpu

R = pm.R
ERR_ARG, ERR_FORMAT = -3, -5
R_INJ, S_INJ = pm.limbs(pm.SplitMix64(491).below(R)), pm.limbs(pm.SplitMix64(492).below(R))


@pytest.fixture(scope="module")
def ctx():
    import k16
    c = k16.Context(0)
    yield c
    c.close()


def raw_scan(circ, cap, wires=True, shifts=True, status=True, fill=0xFF):
    """k16_r1cs_second_values with any of its optional outputs left out: (rc, n, wires, shift bytes, status), the buffers
    pre-filled so that what the call did not write shows"""
    n_wires = circ.info()["n_wires"]
    room = max(cap, n_wires) + 1
    w = np.full(room, 0xFFFFFFFF, dtype=np.uint32) if wires else None
    sh = np.full((room, 32), fill, dtype=np.uint8) if shifts else None
    st = np.full(n_wires, fill, dtype=np.uint8) if status else None
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    n = C.c_uint64(12345)
    rc = circ.ctx.L.k16_r1cs_second_values(circ.h, C.byref(n), ptr(w), ptr(sh), cap, ptr(st))
    return rc, int(n.value), w, sh, st


def shift_bytes(shifts):
    return b"".join(int(d).to_bytes(32, "little") for d in shifts)


def assert_scan(circ, classes, shifts, what=None):
    """the full map, the count, the ascending list and the shifts' bytes of a scan against the reference"""
    want_n, want_wires, want_shifts = sv.summary(classes, shifts)
    rc, n, wires, sh, status = raw_scan(circ, len(classes))
    assert rc == 0 and n == want_n, what
    assert status.tolist() == classes, what
    assert wires[:n].tolist() == want_wires and (wires[n:] == 0xFFFFFFFF).all(), what
    assert sh[:n].tobytes() == shift_bytes(want_shifts) and (sh[n:] == 0xFF).all(), what
    got = circ.second_values(status=True)                             # the binding: the same
    assert (got[0], got[1].tolist(), got[2], got[3].tolist()) == (want_n, want_wires, want_shifts, classes), what
    # class 3 read as BOUND: the bytes of the unbound-wire scan on the same sums
    assert np.where(status == TWO_VALUED, BOUND, status).tobytes() == circ.unbound_wires(status=True)[4].tobytes(), what


def scanned(ctx, circuit, witnesses, what=None):
    """check + scan of every witness on one object; returns the reference's (classes, shifts) per witness"""
    import k16
    n_wires, rowsA, rowsB, rowsC = circuit
    circ = k16.R1cs(ctx, rb.write(n_wires, rowsA, rowsB, rowsC))
    out = []
    try:
        for w in witnesses:
            n_failed, _ = circ.check(rb.witness_bytes(w))
            assert n_failed == len(rb.check(rowsA, rowsB, rowsC, w)), what
            out.append(sv.classify(n_wires, rowsA, rowsB, rowsC, w))
            assert_scan(circ, *out[-1], what)
    finally:
        circ.close()
    return out


def test_constant_is_the_headers():
    import k16
    assert k16.WIRE_TWO_VALUED == TWO_VALUED == 3


@pytest.mark.parametrize("name", sorted(sv.DIRECTED))
def test_directed_circuits(ctx, name):
    circ, classes, shifts = sv.DIRECTED[name]
    assert scanned(ctx, circ[:4], [circ[4]], name)[0] == (classes, shifts)


@pytest.mark.parametrize("target", [255, 256, 257])
def test_block_edges_reach_the_kernels(ctx, target):
    """the launches cover exactly 255, 256 and 257 incidences: one lane short of a block, a whole block, one lane into the next"""
    import k16
    for last in (sv.AGREE, sv.CLASH, sv.PINNED):
        circuit = sv.DIRECTED["walked_%d_%s" % (target, last)][0]
        circ = k16.R1cs(ctx, rb.write(*circuit[:4]))
        try:
            assert circ.incidences() - circ.wire_constraints(0)[0] == target
        finally:
            circ.close()


@functools.lru_cache(maxsize=None)
def large():
    shape = ur.large_shape()
    n_wires, rowsA, rowsB, rowsC, _ = rb.from_shape(shape)
    w = rb.witness_ints(vkb.fast_witness(shape, 5)[0])
    return (n_wires, rowsA, rowsB, rowsC), w, sv.classify(n_wires, rowsA, rowsB, rowsC, w)


def assert_second_witness(circ, circuit, w, wire, d, broken):
    """the loop closed through the existing check: w + d e_wire breaks the same constraints as w, and every constraint of the
    wire's column keeps its residual"""
    n_wires, rowsA, rowsB, rowsC = circuit
    w2 = sv.shifted(w, wire, d)
    n, lst = circ.check(rb.witness_bytes(w2))
    assert (n, lst.tolist()) == (len(broken), broken), wire
    for c in ur.wire_constraints(n_wires, rowsA, rowsB, rowsC, wire):
        a, b, cc = circ.values(c)
        assert (a, b, cc) == rb.values(rowsA, rowsB, rowsC, w2, c), (wire, c)
        assert (a * b - cc) % R == sv.residuals(rowsA, rowsB, rowsC, w, [c])[0], (wire, c)


@pytest.mark.parametrize("block", range(4))
def test_random_circuits_satisfied_and_broken(ctx, block):
    import k16
    for seed in range(block * 10, block * 10 + 10):
        n_wires, rowsA, rowsB, rowsC, w, w_broken, _ = ur.random_circuit(seed)
        circuit = (n_wires, rowsA, rowsB, rowsC)
        found = scanned(ctx, circuit, [w, w_broken, w], seed)
        circ = k16.R1cs(ctx, rb.write(*circuit))
        try:
            for ww, (classes, shifts) in zip((w, w_broken), found):
                broken = rb.check(rowsA, rowsB, rowsC, ww)
                for wire, d in sorted(shifts.items()):
                    assert_second_witness(circ, circuit, ww, wire, d, broken)
        finally:
            circ.close()


def test_larger_shape_and_its_second_witnesses(ctx):
    import k16
    circuit, w, (classes, shifts) = large()
    assert 19000 <= circuit[0] <= 21000 and classes.count(TWO_VALUED) > 1000
    circ = k16.R1cs(ctx, rb.write(*circuit))
    try:
        assert circ.check(rb.witness_bytes(w))[0] == 0
        assert_scan(circ, classes, shifts)
        n, wires, got = circ.second_values(cap=200)
        assert n == classes.count(TWO_VALUED) and len(got) == 200
        wb = rb.witness_bytes(w)
        cols = {}
        for s, c, _, _, _ in ur.incidences(*circuit):
            cols.setdefault(s, []).append(c)
        rowsA, rowsB, rowsC = circuit[1:]
        for wire, d in zip(wires.tolist(), got):
            w2b = wb.copy()
            w2b[wire] = np.frombuffer(((w[wire] + d) % R).to_bytes(32, "little"), dtype=np.uint8)
            assert circ.check(w2b)[0] == 0, wire
            w2 = sv.shifted(w, wire, d)
            for c in cols[wire]:
                a, b, cc = circ.values(c)
                assert (a, b, cc) == rb.values(rowsA, rowsB, rowsC, w2, c) and (a * b - cc) % R == 0, (wire, c)
    finally:
        circ.close()


def test_errors_caps_null_outputs_and_repeatability(ctx):
    import k16
    circuit, classes, shifts = sv.DIRECTED["wires_129"]
    n_wires, rowsA, rowsB, rowsC, w = circuit
    want_n, want_wires, want_shifts = sv.summary(classes, shifts)
    assert want_n == 4
    circ = k16.R1cs(ctx, rb.write(n_wires, rowsA, rowsB, rowsC))
    try:
        with pytest.raises(k16.K16Error) as e:                                 # before any check
            circ.second_values()
        assert e.value.rc == ERR_ARG
        w_refused = [2] + w[1:]
        with pytest.raises(k16.K16Error) as e:
            circ.check(rb.witness_bytes(w_refused))
        assert e.value.rc == ERR_FORMAT
        with pytest.raises(k16.K16Error) as e:                                 # a refused witness completes no check
            circ.second_values()
        assert e.value.rc == ERR_ARG
        assert circ.check(rb.witness_bytes(w))[0] == 0
        with pytest.raises(k16.K16Error) as e:                                 # a completed check, then a refused one: none again
            circ.check(rb.witness_bytes(w_refused))
        assert e.value.rc == ERR_FORMAT
        rc, n, _, _, _ = raw_scan(circ, n_wires)
        assert (rc, n) == (ERR_ARG, 0)
        assert circ.check(rb.witness_bytes(w))[0] == 0
        for cap in (0, 1, want_n - 1, want_n, want_n + 1, n_wires + 70):
            rc, n, wires, sh, status = raw_scan(circ, cap)
            k = min(cap, want_n)
            assert (rc, n) == (0, want_n) and status.tolist() == classes, cap
            assert wires[:k].tolist() == want_wires[:k] and (wires[k:] == 0xFFFFFFFF).all(), cap   # nothing behind cap is touched
            assert sh[:k].tobytes() == shift_bytes(want_shifts[:k]) and (sh[k:] == 0xFF).all(), cap
            got = circ.second_values(cap=cap)
            assert (got[0], got[1].tolist(), got[2]) == (want_n, want_wires[:k], want_shifts[:k]), cap
        # NULL outputs, each alone and all together: the count stays, what is asked for is written
        for wires_on, shifts_on, status_on in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1)):
            rc, n, wires, sh, status = raw_scan(circ, n_wires, wires_on, shifts_on, status_on)
            assert (rc, n) == (0, want_n)
            assert wires is None or wires[:n].tolist() == want_wires
            assert sh is None or sh[:n].tobytes() == shift_bytes(want_shifts)
            assert status is None or status.tolist() == classes
        assert circ.ctx.L.k16_r1cs_second_values(circ.h, None, None, None, 0, None) == ERR_ARG
        n = C.c_uint64()
        assert circ.ctx.L.k16_r1cs_second_values(None, C.byref(n), None, None, 0, None) == ERR_ARG
        # two scans: byte-equal outputs
        a, b = raw_scan(circ, n_wires), raw_scan(circ, n_wires)
        assert a[:2] == b[:2] and all(x.tobytes() == y.tobytes() for x, y in zip(a[2:], b[2:]))
    finally:
        circ.close()


def test_a_scan_moves_nothing_else(ctx):
    """neither what k16_r1cs_unbound_wires returns, nor the sums, nor a following check"""
    import k16
    n_wires, rowsA, rowsB, rowsC, w, w_broken, _ = ur.random_circuit(11)
    circ = k16.R1cs(ctx, rb.write(n_wires, rowsA, rowsB, rowsC))
    try:
        wb = rb.witness_bytes(w_broken)
        n_before, list_before = circ.check(wb)
        assert n_before == len(rb.check(rowsA, rowsB, rowsC, w_broken)) > 0
        values_before = [circ.values(c) for c in range(len(rowsA))]
        unbound_before = circ.unbound_wires(status=True)
        circ.second_values(status=True)
        unbound_after = circ.unbound_wires(status=True)
        assert unbound_before[:2] == unbound_after[:2]
        assert all(x.tobytes() == y.tobytes() for x, y in zip(unbound_before[2:], unbound_after[2:]))
        assert unbound_after[4].tolist() == ur.classify(n_wires, rowsA, rowsB, rowsC, w_broken)
        assert [circ.values(c) for c in range(len(rowsA))] == values_before    # the sums the scan read are still there
        n_after, list_after = circ.check(wb)
        assert n_after == n_before and list_after.tolist() == list_before.tolist()
        circ.second_values()
        assert [circ.values(c) for c in range(len(rowsA))] == values_before
    finally:
        circ.close()


def test_second_scan_first_then_the_unbound_scan(ctx):
    """the incidence list's device copy is made by whichever scan comes first"""
    import k16
    circuit, classes, shifts = sv.DIRECTED["roots_agree"]
    circ = k16.R1cs(ctx, rb.write(*circuit[:4]))
    try:
        assert circ.check(rb.witness_bytes(circuit[4]))[0] == 0
        assert circ.second_values()[:1] == (1,)
        assert circ.unbound_wires(status=True)[4].tolist() == ur.classify(*circuit)
        assert_scan(circ, classes, shifts)
    finally:
        circ.close()


def finding():
    """y public, x x = y, y one = y; a lone boolean b and a pinned z beside them: wires 1 y, 2 x, 3 b, 4 z"""
    x, z = 3, 5
    rowsA = [[(2, 1)], [(1, 1)], [(3, 1)], [(4, 1)]]
    rowsB = [[(2, 1)], [(0, 1)], [(3, 1), (0, R - 1)], [(0, 1)]]
    rowsC = [[(1, 1)], [(1, 1)], [], [(0, z)]]
    return (5, rowsA, rowsB, rowsC, 0, 1), [1, x * x, x, 1, z]


def test_three_witness_sources_agree(ctx, tmp_path):
    """check_mem, check_file and a prove call on the attached object leave the same sums: the same scan"""
    from test_gpu_setup import Made
    circuit, w = finding()
    m = Made(ctx, tmp_path, circuit, w)
    try:
        n_wires, rowsA, rowsB, rowsC = circuit[:4]
        classes, shifts = sv.classify(n_wires, rowsA, rowsB, rowsC, w)
        assert (classes, shifts) == ([BOUND, BOUND, TWO_VALUED, TWO_VALUED, BOUND], {2: R - 6, 3: R - 1})
        assert m.circ.check(m.witness)[0] == 0
        assert_scan(m.circ, classes, shifts, "check_mem")
        from_mem = raw_scan(m.circ, n_wires)
        assert m.circ.check_file(m.wt)[0] == 0
        assert_scan(m.circ, classes, shifts, "check_file")
        from_file = raw_scan(m.circ, n_wires)
        m.p.set_r1cs(m.circ)
        assert m.p.prove_mem(m.witness, R_INJ, S_INJ)
        assert m.p.last_check()[0] == 1
        assert_scan(m.circ, classes, shifts, "prove_mem")                      # between prove calls: the sums of the last prove
        from_prove = raw_scan(m.circ, n_wires)
        assert m.circ.check_prover(m.p)[0] == 0
        assert_scan(m.circ, classes, shifts, "check_prover")
        for other in (from_file, from_prove, raw_scan(m.circ, n_wires)):
            assert from_mem[:2] == other[:2] and all(x.tobytes() == y.tobytes() for x, y in zip(from_mem[2:], other[2:]))
        m.p.set_r1cs(None)
    finally:
        m.close()


def test_the_finding_made_concrete(ctx, tmp_path):
    """the scan names x; the witness with x's second value proves, and both proofs verify under the SAME public input"""
    from test_gpu_setup import Made
    circuit, w = finding()
    m = Made(ctx, tmp_path, circuit, w)
    try:
        assert m.circ.check(m.witness)[0] == 0
        n, wires, shifts = m.circ.second_values()
        assert 2 in wires.tolist()
        d = shifts[wires.tolist().index(2)]
        w2 = sv.shifted(w, 2, d)
        assert w2[2] == R - 3 and w2[1] == w[1] and rb.check(*circuit[1:4], w2) == []
        _, proof1, ok1 = m.p.prove_mem_verified(m.witness, R_INJ, S_INJ)
        _, proof2, ok2 = m.p.prove_mem_verified(rb.witness_bytes(w2), R_INJ, S_INJ)
        assert (ok1, ok2) == (1, 1) and bytes(proof1) != bytes(proof2)
        assert m.public == [9]
        assert m.V.verify_batch([proof1, proof2], [m.public, m.public]) == [True, True]
    finally:
        m.close()
