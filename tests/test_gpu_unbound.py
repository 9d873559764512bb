"""-m gpu : the unbound-wire scan (include/k16.h k16_r1cs_unbound_wires / _wire_constraints / _incidences; csrc/r1cs_scan.hip
k_r1cs_incidences, csrc/r1cs_pairs.h) against the big-integer reference of tests/unbound_reference.py.  Every case compares the
class of every wire, both counts and the ascending list with the reference; what each directed circuit's classes must be is
asserted of the reference itself in tests/test_unbound_host.py."""
import ctypes as C

import numpy as np
import pytest

import pymodel as pm
import r1cs_builder as rb
import setup_reference as sr
import unbound_reference as ur
import valid_key_builder as vkb
from unbound_reference import ABSENT, BOUND, UNBOUND

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


def assert_scan(circ, classes, what=None):
    """the full map, the counts and the ascending list of a scan against the reference's classes"""
    n_absent, n_unbound, wires, cls, status = circ.unbound_wires(status=True)
    want = ur.summary(classes)
    assert status.tolist() == classes, what
    assert (n_absent, n_unbound, wires.tolist(), cls.tolist()) == want, what


def scanned(ctx, circuit, witnesses, what=None):
    """check + scan of every witness on one object; returns the reference's classes per witness"""
    import k16
    n_wires, rowsA, rowsB, rowsC = circuit
    circ = k16.R1cs(ctx, rb.write(n_wires, rowsA, rowsB, rowsC))
    out = []
    try:
        for w in witnesses:
            n_failed, _ = circ.check(rb.witness_bytes(w))
            assert n_failed == len(rb.check(rowsA, rowsB, rowsC, w)), what
            out.append(ur.classify(n_wires, rowsA, rowsB, rowsC, w))
            assert_scan(circ, out[-1], what)
        inc = ur.incidences(*circuit)
        assert circ.incidences() == len(inc), what
    finally:
        circ.close()
    return out


def test_constants_are_the_headers():
    import k16
    assert (k16.WIRE_BOUND, k16.WIRE_ABSENT, k16.WIRE_UNBOUND) == (BOUND, ABSENT, UNBOUND) == (0, 1, 2)


def test_directed_circuits(ctx):
    got = {name: scanned(ctx, circ[:4], [circ[4]], name)[0] for name, circ in sorted(ur.DIRECTED.items())}
    assert got["mux_sel0"] == [BOUND, BOUND, UNBOUND, BOUND, BOUND] and got["mux_sel1"][2] == BOUND
    assert got["square_at_zero"][1] == BOUND                                  # quad alone binds x
    assert got["zero_only_modulo_r"][1] == UNBOUND                            # lin is a non-zero multiple of r
    assert got["cancellation_alone"][2] == ABSENT and got["cancellation_elsewhere"][2] == BOUND
    for n, at in ur.COLUMN_CASES:
        assert got["column_%d_%s" % (n, at)][1] == (UNBOUND if at is None else BOUND), (n, at)


@pytest.mark.parametrize("target", [255, 256, 257])
@pytest.mark.parametrize("last", ["bound", "free"])
def test_block_edges_reach_the_kernel(ctx, target, last):
    """the launch covers the incidences of the wires from 1 on: exactly 255, 256 and 257 of them -- one lane short of a block, a
    whole block, one lane into the next -- with the last incidence bound and free"""
    import k16
    n_wires, rowsA, rowsB, rowsC, w = ur.DIRECTED["pairs_%d_%s" % (target, last)]
    circ = k16.R1cs(ctx, rb.write(n_wires, rowsA, rowsB, rowsC))
    try:
        assert circ.incidences() - circ.wire_constraints(0)[0] == target
        assert circ.check(rb.witness_bytes(w))[0] == 0
        classes = ur.classify(n_wires, rowsA, rowsB, rowsC, w)
        assert classes[-1] == (BOUND if last == "bound" else UNBOUND)
        assert_scan(circ, classes)
    finally:
        circ.close()


@pytest.mark.parametrize("block", range(4))
def test_random_circuits_satisfied_and_broken(ctx, block):
    for seed in range(block * 10, block * 10 + 10):
        n_wires, rowsA, rowsB, rowsC, w, w_broken, _ = ur.random_circuit(seed)
        scanned(ctx, (n_wires, rowsA, rowsB, rowsC), [w, w_broken, w], seed)


def test_larger_shape(ctx):
    shape = ur.large_shape()
    n_wires, rowsA, rowsB, rowsC, _ = rb.from_shape(shape)
    assert 19000 <= n_wires <= 21000
    wb, _ = vkb.fast_witness(shape, 5)
    classes = scanned(ctx, (n_wires, rowsA, rowsB, rowsC), [rb.witness_ints(wb)])[0]
    assert min(classes.count(k) for k in (BOUND, ABSENT, UNBOUND)) > 100      # all three classes occur in numbers


def raw_scan(circ, wires, cls, cap, status):
    """k16_r1cs_unbound_wires with any of its optional outputs left out"""
    na, nu = C.c_uint64(), C.c_uint64()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    rc = circ.ctx.L.k16_r1cs_unbound_wires(circ.h, C.byref(na), C.byref(nu), ptr(wires), ptr(cls), cap, ptr(status))
    return rc, int(na.value), int(nu.value)


def test_errors_caps_null_outputs_and_repeatability(ctx):
    import k16
    n_wires, rowsA, rowsB, rowsC, w, _, _ = ur.random_circuit(3)
    circ = k16.R1cs(ctx, rb.write(n_wires, rowsA, rowsB, rowsC))
    try:
        with pytest.raises(k16.K16Error) as e:                                 # before any check
            circ.unbound_wires()
        assert e.value.rc == ERR_ARG
        w_refused = [2] + w[1:]
        with pytest.raises(k16.K16Error) as e:
            circ.check(rb.witness_bytes(w_refused))
        assert e.value.rc == ERR_FORMAT
        with pytest.raises(k16.K16Error) as e:                                 # a refused witness completes no check
            circ.unbound_wires()
        assert e.value.rc == ERR_ARG
        for wire in (n_wires, n_wires + 1, 2 ** 32 - 1):
            with pytest.raises(k16.K16Error) as e:
                circ.wire_constraints(wire)
            assert e.value.rc == ERR_ARG
        assert circ.check(rb.witness_bytes(w))[0] == 0
        with pytest.raises(k16.K16Error) as e:                                 # a completed check, then a refused one: none again
            circ.check(rb.witness_bytes(w_refused))
        assert e.value.rc == ERR_FORMAT
        with pytest.raises(k16.K16Error) as e:
            circ.unbound_wires()
        assert e.value.rc == ERR_ARG
        assert circ.check(rb.witness_bytes(w))[0] == 0
        classes = ur.classify(n_wires, rowsA, rowsB, rowsC, w)
        n_absent, n_unbound, free, free_cls = ur.summary(classes)
        assert len(free) >= 3
        for cap in sorted({0, 1, len(free) - 1, len(free), len(free) + 1, n_wires + 70}):
            got = circ.unbound_wires(cap=cap)
            assert (got[0], got[1], got[2].tolist(), got[3].tolist()) == (n_absent, n_unbound, free[:cap], free_cls[:cap]), cap
        # NULL outputs, each alone and all together: the counts stay, what is asked for is written
        assert raw_scan(circ, None, None, 0, None) == (0, n_absent, n_unbound)
        assert raw_scan(circ, None, None, n_wires, None) == (0, n_absent, n_unbound)
        wires, cls = np.full(n_wires, 0xFFFFFFFF, dtype=np.uint32), np.full(n_wires, 0xFF, dtype=np.uint8)
        assert raw_scan(circ, wires, None, n_wires, None) == (0, n_absent, n_unbound)
        assert wires[:len(free)].tolist() == free and (wires[len(free):] == 0xFFFFFFFF).all()
        assert raw_scan(circ, None, cls, 2, None) == (0, n_absent, n_unbound)
        assert cls[:2].tolist() == free_cls[:2] and (cls[2:] == 0xFF).all()                # nothing behind cap is touched
        status = np.full(n_wires, 0xFF, dtype=np.uint8)
        assert raw_scan(circ, None, None, 0, status) == (0, n_absent, n_unbound) and status.tolist() == classes
        na = C.c_uint64()
        assert circ.ctx.L.k16_r1cs_unbound_wires(circ.h, None, C.byref(na), None, None, 0, None) == ERR_ARG
        assert circ.ctx.L.k16_r1cs_unbound_wires(None, C.byref(na), C.byref(na), None, None, 0, None) == ERR_ARG
        # two scans: byte-equal outputs
        a, b = circ.unbound_wires(status=True), circ.unbound_wires(status=True)
        assert a[:2] == b[:2] and all(x.tobytes() == y.tobytes() for x, y in zip(a[2:], b[2:]))
    finally:
        circ.close()


def test_wire_constraints_and_incidences_need_no_check(ctx):
    import k16
    for circuit in (ur.random_circuit(5)[:4], ur.DIRECTED["cancellation_alone"][:4], ur.DIRECTED["column_129_64"][:4]):
        circ = k16.R1cs(ctx, rb.write(*circuit))
        try:
            assert circ.incidences() == len(ur.incidences(*circuit))           # host only: no check has run
            for wire in range(circuit[0]):
                want = ur.wire_constraints(*circuit, wire)
                n, got = circ.wire_constraints(wire)
                assert n == len(want) and got.tolist() == want, wire
                for cap in sorted({0, 1, max(len(want) - 1, 0)}):
                    n, got = circ.wire_constraints(wire, cap=cap)
                    assert n == len(want) and got.tolist() == want[:cap], (wire, cap)
            n = C.c_uint64()
            assert circ.ctx.L.k16_r1cs_wire_constraints(circ.h, 1, C.byref(n), None, 5) == 0  # a NULL list is accepted
            assert n.value == len(ur.wire_constraints(*circuit, 1))
        finally:
            circ.close()
    assert ur.wire_constraints(*ur.DIRECTED["cancellation_alone"][:4], 2) == []    # (the wire whose coefficients cancel: n = 0)


def test_three_witness_sources_agree(ctx, tmp_path):
    """check_mem, check_file and a prove call on the attached object leave the same sums: the same scan"""
    from test_gpu_setup import Made
    circuit, w = sr.mixed(63, 0, 1)
    m = Made(ctx, tmp_path, circuit, w)
    try:
        n_wires, rowsA, rowsB, rowsC = circuit[:4]
        classes = ur.classify(n_wires, rowsA, rowsB, rowsC, w)
        assert {ABSENT, BOUND} <= set(classes)                                 # (sr.mixed keeps a wire in no constraint)
        assert m.circ.check(m.witness)[0] == 0
        assert_scan(m.circ, classes, "check_mem")
        from_mem = m.circ.unbound_wires(status=True)
        assert m.circ.check_file(m.wt)[0] == 0
        assert_scan(m.circ, classes, "check_file")
        m.p.set_r1cs(m.circ)
        assert m.p.prove_mem(m.witness, R_INJ, S_INJ)
        assert m.p.last_check()[0] == 1
        assert_scan(m.circ, classes, "prove_mem")                              # between prove calls: the sums of the last prove
        from_prove = m.circ.unbound_wires(status=True)
        assert from_mem[:2] == from_prove[:2] and all(x.tobytes() == y.tobytes() for x, y in zip(from_mem[2:], from_prove[2:]))
        # another witness through the prover: the scan follows it
        w2 = list(w)
        w2[m.n_public + 1] = (w2[m.n_public + 1] + 1) % R
        m.p.prove_mem(rb.witness_bytes(w2), R_INJ, S_INJ)
        assert_scan(m.circ, ur.classify(n_wires, rowsA, rowsB, rowsC, w2), "prove_mem, changed witness")
        m.p.set_r1cs(None)
    finally:
        m.close()


def test_a_scan_moves_nothing_else(ctx):
    import k16
    n_wires, rowsA, rowsB, rowsC, w, w_broken, _ = ur.random_circuit(11)
    circ = k16.R1cs(ctx, rb.write(n_wires, rowsA, rowsB, rowsC))
    try:
        wb = rb.witness_bytes(w_broken)
        n_before, list_before = circ.check(wb)
        assert n_before == len(rb.check(rowsA, rowsB, rowsC, w_broken)) > 0
        values_before = [circ.values(c) for c in range(len(rowsA))]
        circ.unbound_wires(status=True)
        assert [circ.values(c) for c in range(len(rowsA))] == values_before    # the sums the scan read are still there
        assert values_before == [rb.values(rowsA, rowsB, rowsC, w_broken, c) for c in range(len(rowsA))]
        n_after, list_after = circ.check(wb)
        assert n_after == n_before and list_after.tolist() == list_before.tolist()
        circ.unbound_wires()
        assert [circ.values(c) for c in range(len(rowsA))] == values_before
    finally:
        circ.close()
