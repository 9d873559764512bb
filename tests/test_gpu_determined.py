"""-m gpu : the determinism closure (include/k16.h k16_r1cs_determined_wires; csrc/r1cs_scan.hip k_r1cs_det_init, _first,
_derive, _expand) against the big-integer reference of tests/determined_reference.py.  Every case compares the counts, the
ascending OPEN list and the status, round and by of every wire with the reference, and runs the reference's independent
certificate replayer on the GPU's own output; what the directed circuits must give is stated by hand there and asserted of the
reference in tests/test_determined_host.py."""
import ctypes as C

import numpy as np
import pytest

import determined_reference as dr
import pymodel as pm
import r1cs_builder as rb
import second_value_reference as sv
import unbound_reference as ur
from determined_reference import ABSENT, DERIVED, NONE, OPEN, SEED

pytestmark = pytest.mark.gpu

R = pm.R
ERR_ARG = -3


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


def raw(circ, seed, cap, wires=True, status=True, rounds=True, by=True, fill=0xA5):
    """k16_r1cs_determined_wires with any optional output left out: (rc, (n_derived, n_absent, n_open, n_rounds), wires, status,
    round, by), the buffers pre-filled so that what the call did not write shows"""
    n_wires = circ.info()["n_wires"]
    room = max(cap, n_wires) + 1
    w = np.full(room, 0xA5A5A5A5, dtype=np.uint32) if wires else None
    st = np.full(n_wires, fill, dtype=np.uint8) if status else None
    ro = np.full(n_wires, 0xA5A5A5A5, dtype=np.uint32) if rounds else None
    b = np.full(n_wires, 0xA5A5A5A5, dtype=np.uint32) if by else None
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    sd = np.array(list(seed) + [0], dtype=np.uint32) if seed is not None else None       # (+ [0]: never an empty buffer)
    nd, na, no, nr = C.c_uint64(77), C.c_uint64(77), C.c_uint64(77), C.c_uint32(77)
    rc = circ.ctx.L.k16_r1cs_determined_wires(circ.h, ptr(sd), 0 if seed is None else len(seed), C.byref(nd), C.byref(na),
                                              C.byref(no), C.byref(nr), ptr(w), cap, ptr(st), ptr(ro), ptr(b))
    return rc, (int(nd.value), int(na.value), int(no.value), int(nr.value)), w, st, ro, b


def same_bytes(x, y):
    return x[:2] == y[:2] and all(a.tobytes() == b.tobytes() for a, b in zip(x[2:], y[2:]))


def assert_closure(circ, circuit, w, seed, seed_list, what=None):
    """one call with everything asked for against the reference; seed: what the call is given (None: the default), seed_list: the
    same as wires.  Returns the reference's (status, round, by)."""
    status, rounds, by = dr.closure(circuit, w, seed_list)
    n_derived, n_absent, n_open, n_rounds, opened = dr.summary(status, rounds)
    rc, counts, wires, st, ro, b = raw(circ, seed, circuit[0])
    assert rc == 0 and counts == (n_derived, n_absent, n_open, n_rounds), what
    assert wires[:n_open].tolist() == opened and (wires[n_open:] == 0xA5A5A5A5).all(), what
    assert st.tolist() == status, what
    assert ro.tolist() == rounds, what
    assert b.tolist() == by, what
    assert dr.replay(circuit, w, seed_list, st.tolist(), ro.tolist(), b.tolist()) is None, what    # the GPU's own certificate
    got = circ.determined_wires(seed=seed, want_maps=True)                                      # the binding: the same
    assert got[:4] == counts and got[4].tolist() == opened, what
    assert (got[5].tolist(), got[6].tolist(), got[7].tolist()) == (status, rounds, by), what
    return status, rounds, by


def run_case(ctx, c, what=None):
    """check + closure of one case on a fresh object"""
    circuit, w, header, seed = c
    seed_list = dr.default_seed(header) if seed is None else seed
    circ = make(ctx, circuit, header)
    try:
        n_failed, _ = circ.check(rb.witness_bytes(w))
        assert n_failed == len(rb.check(*circuit[1:], w)), what
        return assert_closure(circ, circuit, w, seed, seed_list, what)
    finally:
        circ.close()


def test_constants_are_the_headers():
    import k16
    assert (k16.DET_SEED, k16.DET_DERIVED, k16.DET_ABSENT, k16.DET_OPEN, k16.DET_NONE) == (SEED, DERIVED, ABSENT, OPEN, NONE) == (0, 1, 2, 3, 0xFFFFFFFF)


@pytest.mark.parametrize("name", sorted(dr.DIRECTED))
def test_directed_circuits(ctx, name):
    status, rounds, by = run_case(ctx, dr.DIRECTED[name], name)
    for wire, want in dr.EXPECTED.get(name, {}).items():
        assert (status[wire], rounds[wire], by[wire]) == want, (name, wire)


def test_chain_of_300_takes_300_rounds(ctx):
    circuit, w, header, seed = dr.DIRECTED["chain_300"]
    circ = make(ctx, circuit, header)
    try:
        assert circ.check(rb.witness_bytes(w))[0] == 0
        n_derived, n_absent, n_open, n_rounds, opened, status, rounds, by = circ.determined_wires(want_maps=True)
        assert (n_derived, n_absent, n_open, n_rounds, len(opened)) == (300, 0, 0, 300, 0)
        assert rounds.tolist() == [0, 0] + list(range(1, 301)) and by.tolist() == [NONE, NONE] + list(range(300))
    finally:
        circ.close()


EDGES = [("wide_%d" % n, 2 * n, 1, None) for n in (63, 64, 65, 255, 256, 257)] + \
        [("fan_%d" % n, 2 + 3 * n, 2, n + 1) for n in (62, 63, 64, 255, 256, 257)]


@pytest.mark.parametrize("name,pairs,rounds,column", EDGES, ids=[e[0] for e in EDGES])
def test_block_and_wave_edges_reach_the_kernels(ctx, name, pairs, rounds, column):
    """the circuits' incidences avoid wire 0, so the launches cover exactly what is stated: wide_n has 2 n incidences, n first
    candidates and a frontier of n in round 1 (63 / 64 / 65, 255 / 256 / 257); fan_n gives ONE frontier wire a column of n + 1
    incidences (63 / 64 / 65, 256 / 257 / 258), whose expansion lists n candidates (255 / 256 / 257 among them) and round 2
    has a frontier of n"""
    circuit, w, header, seed = dr.DIRECTED[name]
    circ = make(ctx, circuit, header)
    try:
        assert circ.wire_constraints(0)[0] == 0 and circ.incidences() == pairs
        if column:
            assert circ.wire_constraints(2)[0] == column
        assert circ.check(rb.witness_bytes(w))[0] == 0
        got = circ.determined_wires()
        assert got[:4] == (circuit[0] - 2, 0, 0, rounds)
    finally:
        circ.close()


def test_mux_on_one_object_under_both_selectors(ctx):
    """the closure is the witness's: the same object, the same seed, two selector values"""
    circuit, w0, header, seed = dr.DIRECTED["mux_sel0_x"]
    w1 = dr.DIRECTED["mux_sel1_x"][1]
    circ = make(ctx, circuit, header)
    try:
        for w, want in ((w0, OPEN), (w1, DERIVED), (w0, OPEN)):
            assert circ.check(rb.witness_bytes(w))[0] == 0
            assert assert_closure(circ, circuit, w, seed, seed)[0][2] == want
    finally:
        circ.close()


def test_broken_then_repaired_on_one_object(ctx):
    circuit, w_bad, header, seed = dr.DIRECTED["broken_link"]
    w_good = dr.DIRECTED["repaired_link"][1]
    seed_list = dr.default_seed(header)
    circ = make(ctx, circuit, header)
    try:
        n, lst = circ.check(rb.witness_bytes(w_bad))
        assert (n, lst.tolist()) == (1, [1])
        assert assert_closure(circ, circuit, w_bad, None, seed_list)[0][3] == OPEN
        assert circ.check(rb.witness_bytes(w_good))[0] == 0
        assert assert_closure(circ, circuit, w_good, None, seed_list)[0][3] == DERIVED
    finally:
        circ.close()


def test_seeds_arguments_caps_and_null_outputs(ctx):
    import k16
    circuit, w, header, _ = dr.DIRECTED["free_but_counted"]
    n_wires = circuit[0]
    default = dr.default_seed(header)
    circ = make(ctx, circuit, header)
    try:
        with pytest.raises(k16.K16Error) as e:                                 # before any check
            circ.determined_wires()
        assert e.value.rc == ERR_ARG
        rc, counts, _, _, _, _ = raw(circ, None, n_wires)
        assert (rc, counts) == (ERR_ARG, (0, 0, 0, 0))
        assert circ.check(rb.witness_bytes(w))[0] == 0
        by_null = raw(circ, None, n_wires)
        assert by_null[0] == 0 and by_null[1] == (3, 0, 2, 3)
        # NULL is the explicit default list, with and without wire 0, in any order, with duplicates: the same bytes
        for seed in (default, default[1:], default[::-1], default + default + [default[-1]]):
            assert same_bytes(by_null, raw(circ, seed, n_wires)), seed
        assert same_bytes(by_null, raw(circ, None, n_wires))                  # two calls in a row
        # an empty list is wire 0 alone; an ABSENT wire in the seed is SEED
        assert_closure(circ, circuit, w, [], [0])
        circuit2, w2, header2, _ = dr.DIRECTED["merged_and_cancelling"]
        circ2 = make(ctx, circuit2, header2)
        try:
            assert circ2.check(rb.witness_bytes(w2))[0] == 0
            status = assert_closure(circ2, circuit2, w2, [1, 2, 3, 6], [1, 2, 3, 6])[0]
            assert status[6] == SEED and dr.closure(circuit2, w2, [1, 2, 3])[0][6] == ABSENT
        finally:
            circ2.close()
        # a wire >= nWires
        for seed in ([n_wires], [1, 2, 0xFFFFFFFF], [n_wires + 63]):
            rc, counts, wires, st, ro, b = raw(circ, seed, n_wires)
            assert (rc, counts) == (ERR_ARG, (0, 0, 0, 0))
            assert (st == 0xA5).all() and (ro == 0xA5A5A5A5).all() and (b == 0xA5A5A5A5).all() and (wires == 0xA5A5A5A5).all()
            with pytest.raises(k16.K16Error) as e:
                circ.determined_wires(seed=seed)
            assert e.value.rc == ERR_ARG
        assert same_bytes(by_null, raw(circ, None, n_wires))                  # an error moved nothing
        # caps: nothing behind min(n_open, cap) is touched
        opened = [6, 7]
        for cap in (0, 1, 2, 3, n_wires + 70):
            rc, counts, wires, st, ro, b = raw(circ, None, cap)
            k = min(cap, 2)
            assert rc == 0 and counts == by_null[1], cap
            assert wires[:k].tolist() == opened[:k] and (wires[k:] == 0xA5A5A5A5).all(), cap
            assert circ.determined_wires(cap=cap)[4].tolist() == opened[:k], cap
        # NULL outputs, each alone and all together: the counts stay, what is asked for is written
        for on in ((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 0, 1, 1), (0, 1, 1, 0)):
            got = raw(circ, None, n_wires, *on)
            assert got[:2] == by_null[:2], on
            for k in range(4):
                assert (got[2 + k] is None) if not on[k] else (got[2 + k].tobytes() == by_null[2 + k].tobytes()), (on, k)
        nd, nr = C.c_uint64(), C.c_uint32()
        L = circ.ctx.L
        assert L.k16_r1cs_determined_wires(circ.h, None, 0, None, C.byref(nd), C.byref(nd), C.byref(nr), None, 0, None, None, None) == ERR_ARG
        assert L.k16_r1cs_determined_wires(circ.h, None, 0, C.byref(nd), C.byref(nd), C.byref(nd), None, None, 0, None, None, None) == ERR_ARG
        assert L.k16_r1cs_determined_wires(None, None, 0, C.byref(nd), C.byref(nd), C.byref(nd), C.byref(nr), None, 0, None, None, None) == ERR_ARG
        assert L.k16_r1cs_determined_wires(circ.h, None, 2, C.byref(nd), C.byref(nd), C.byref(nd), C.byref(nr), None, 0, None, None, None) == ERR_ARG
    finally:
        circ.close()


def test_header_inputs_beyond_the_wires_are_refused(ctx):
    import k16
    circuit, w, header, _ = dr.DIRECTED["chain_3"]
    circ = make(ctx, circuit, (0, 1, circuit[0]))
    try:
        assert circ.check(rb.witness_bytes(w))[0] == 0
        with pytest.raises(k16.K16Error) as e:
            circ.determined_wires()
        assert e.value.rc == ERR_ARG
        assert circ.determined_wires(seed=[1])[:4] == (3, 0, 0, 3)            # a list of the caller's does not need the header
    finally:
        circ.close()


@pytest.mark.parametrize("order", ["closure_first", "after_unbound", "after_second", "after_both"])
def test_the_device_list_is_shared_with_the_scans(ctx, order):
    """whichever call comes first makes the incidence list's device copy: the closure's bytes are the same behind each, and the
    scans' bytes are the same behind the closure"""
    circuit, w, header, seed = dr.resolved(dr.random_case(20))
    want = dr.closure(circuit, w, seed)
    circ = make(ctx, circuit, header)
    try:
        circ.check(rb.witness_bytes(w))
        if order in ("after_unbound", "after_both"):
            circ.unbound_wires()
        if order in ("after_second", "after_both"):
            circ.second_values()
        got = circ.determined_wires(seed=seed, want_maps=True)
        assert (got[5].tolist(), got[6].tolist(), got[7].tolist()) == want
        assert circ.unbound_wires(status=True)[4].tolist() == ur.classify(*circuit, w)
        classes, shifts = sv.classify(*circuit, w)
        n, wires, d, full = circ.second_values(status=True)
        assert full.tolist() == classes and dict(zip(wires.tolist(), d)) == shifts
        again = circ.determined_wires(seed=seed, want_maps=True)
        assert got[:4] == again[:4] and all(x.tobytes() == y.tobytes() for x, y in zip(got[4:], again[4:]))
    finally:
        circ.close()


@pytest.mark.parametrize("block", range(4))
def test_random_circuits(ctx, block):
    """40 random circuits, satisfying and corrupted witnesses, default and listed seeds; beside the reference, the existing scans
    on the same sums: a wire they call UNBOUND or TWO_VALUED has no PIN, so outside the seed it is never DERIVED"""
    for i in range(block * 10, block * 10 + 10):
        circuit, w, header, seed = dr.random_case(i)
        seed_list = dr.default_seed(header) if seed is None else seed
        circ = make(ctx, circuit, header)
        try:
            circ.check(rb.witness_bytes(w))
            status, rounds, by = assert_closure(circ, circuit, w, seed, seed_list, i)
            unbound = circ.unbound_wires(status=True)[4].tolist()
            second = circ.second_values(status=True)[3].tolist()
            for s in range(1, circuit[0]):
                if s not in seed_list and (unbound[s] == ur.UNBOUND or second[s] == sv.TWO_VALUED):
                    assert status[s] in (OPEN, ABSENT), (i, s)
                assert (status[s] == ABSENT) == (unbound[s] == ur.ABSENT and s not in seed_list), (i, s)
        finally:
            circ.close()


def test_random_circuits_are_not_degenerate():
    """at least 30 of the 40 derive something and leave something open (the reference's verdict; no device needed)"""
    good = 0
    for i in range(dr.N_RANDOM):
        circuit, w, header, seed = dr.resolved(dr.random_case(i))
        status = dr.closure(circuit, w, seed)[0]
        good += status.count(DERIVED) > 0 and status.count(OPEN) > 0
    assert good >= 30


def test_three_witness_sources_agree(ctx, tmp_path):
    """check_mem, check_file and a prove call on the attached object leave the same sums: the same closure, and the call is
    legal between prove calls"""
    from test_gpu_second_values import R_INJ, S_INJ, finding
    from test_gpu_setup import Made
    circuit, w = finding()                                                # y public, x x = y, a lone boolean b, a pinned z
    m = Made(ctx, tmp_path, circuit, w)
    try:
        plain = circuit[:4]
        seed = [1]                                                        # the public wire y
        status, rounds, by = dr.closure(plain, w, seed)
        assert status == [SEED, SEED, OPEN, OPEN, DERIVED]                # x is a ROOT of y, b of nothing; z is pinned to a constant
        assert m.circ.check(m.witness)[0] == 0
        assert_closure(m.circ, plain, w, seed, seed, "check_mem")
        from_mem = raw(m.circ, seed, plain[0])
        assert m.circ.check_file(m.wt)[0] == 0
        from_file = raw(m.circ, seed, plain[0])
        m.p.set_r1cs(m.circ)
        assert m.p.prove_mem(m.witness, R_INJ, S_INJ)
        assert m.p.last_check()[0] == 1
        from_prove = raw(m.circ, seed, plain[0])
        assert m.p.prove_mem(m.witness, R_INJ, S_INJ) and m.p.last_check()[0] == 1    # and the prover goes on
        for other in (from_file, from_prove, raw(m.circ, seed, plain[0])):
            assert other[0] == 0 and same_bytes(from_mem, other)
        m.p.set_r1cs(None)
    finally:
        m.close()


def free_device_bytes():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_only_the_closure_pays_for_the_closure(ctx):
    """creation, a check and the two existing scans allocate what they do on an object that never sees a closure call; the
    closure's own buffers come with its first call, its second call adds nothing, and destroying the object returns everything"""
    n = 150000                                                            # hipMemGetInfo moves in steps of 2 MB: buffers that show
    circuit, w, header, seed = dr.wide(n)
    wb = rb.witness_bytes(w)
    warm = make(ctx, circuit, header)                                     # (the first kernels of a process load their code)
    warm.check(wb), warm.unbound_wires(), warm.second_values()
    assert warm.determined_wires(cap=0)[:4] == (n, 0, 0, 1)               # (a frontier of 150,000 wires in one round)
    warm.close()

    def steps(closure_at):
        """free device bytes at the start, after create, check, [closure], both scans, [closure], check, destroy"""
        marks = [free_device_bytes()]
        circ = make(ctx, circuit, header)
        marks.append(free_device_bytes())
        circ.check(wb)
        marks.append(free_device_bytes())
        for at in ("first", "last"):
            if closure_at == at:
                circ.determined_wires()
                once = free_device_bytes()
                circ.determined_wires(want_maps=True)
                assert free_device_bytes() == once                        # the second call allocates nothing
            marks.append(free_device_bytes())
            if at == "first":
                circ.unbound_wires()
                circ.second_values()
                marks.append(free_device_bytes())
        circ.check(wb)
        marks.append(free_device_bytes())
        circ.close()
        marks.append(free_device_bytes())
        return marks

    plain, first, last = steps(None), steps("first"), steps("last")
    for m in (plain, first, last):
        assert m[0] == m[-1]                                              # nothing is left behind
        assert m[0] - m[1] == plain[0] - plain[1] >= 0                    # create
        assert m[1] == m[2] and m[5] == m[6]                              # a check allocates nothing, before or after
    assert plain[2] == plain[3] and plain[4] == plain[5]
    scans = plain[3] - plain[4]
    assert scans > 0 and last[3] - last[4] == scans                       # the scans before a closure call: as ever
    assert 0 <= first[3] - first[4] <= scans                              # behind one: the list is there already, nothing is added
    assert last[4] - last[5] >= 0 and first[2] - first[3] >= 0            # the closure's own buffers (+ the list when it is first)
