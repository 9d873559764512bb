"""-m gpu : checked proving (include/k16.h k16_prover_set_r1cs, k16_prover_last_check; csrc/r1cs_check.hip k_r1cs_summary) --
with a circuit attached, every prove call carries the verdict of the R1CS check on its own witness: status, exact count and
the lowest 64 broken constraints.  Circuits come from tests/r1cs_builder.py, their keys from the set-up on the GPU, the
reference verdicts from rb.check (Python big integers, row by row), the proofs from the CPU oracle.  All arithmetic is
exact: every comparison is equality."""
import ctypes as C
import threading

import numpy as np
import pytest

import oracle_lib as ol
import pymodel as pm
import r1cs_builder as rb
import setup_reference as sr
import valid_key_builder as vkb
from test_gpu_r1cs_check import c_off_by_one, mixed_circuit
from test_gpu_setup import Made

pytestmark = pytest.mark.gpu

R = pm.R
ERR_ARG, ERR_FORMAT = -3, -5
NONE, SATISFIED, BROKEN, REFUSED = 0, 1, 2, 3
REPORT_MAX = 64
R_INJ, S_INJ = pm.limbs(pm.SplitMix64(391).below(R)), pm.limbs(pm.SplitMix64(392).below(R))


@pytest.fixture(scope="module")
def ctx():
    import k16
    c = k16.Context(0)
    yield c
    c.close()


def test_constants_are_the_headers():
    import k16
    assert (k16.CHECK_NONE, k16.CHECK_SATISFIED, k16.CHECK_BROKEN, k16.CHECK_WITNESS_REFUSED) == (NONE, SATISFIED, BROKEN, REFUSED)
    assert k16.R1CS_REPORT_MAX == REPORT_MAX


def assert_capped(p, want):
    """k16_prover_last_check under caps below, equal to and above the count"""
    n = len(want)
    for cap in sorted({0, 1, max(n - 1, 0), n, n + 1, n + 70}):
        assert p.last_check(cap) == (BROKEN if n else SATISFIED, n, want[:min(cap, REPORT_MAX)]), cap
    assert p.last_check() == (BROKEN if n else SATISFIED, n, want[:REPORT_MAX])


def breaking_witness(m):
    """m's witness with one private wire changed so that the reference checker names at least one constraint"""
    for wire in range(m.n_public + 1, m.circuit[0]):
        w2 = list(m.w)
        w2[wire] = (w2[wire] + 1) % R
        want = rb.check(*m.rows, w2)
        if want:
            return w2, want
    raise AssertionError("no private wire of this circuit breaks a constraint")


# ---------------------------------------------------------------- 1. mixed shapes and the toy circuit
@pytest.fixture(scope="module", params=sr.MIXED_SHAPES + ["toy"], ids=lambda s: "toy" if s == "toy" else "M%d_out%d_in%d" % s)
def made(request, ctx, tmp_path_factory):
    circuit, w = (sr.TOY, sr.TOY_WITNESS) if request.param == "toy" else sr.mixed(*request.param)
    m = Made(ctx, tmp_path_factory.mktemp("checked"), circuit, w)
    m.p.set_r1cs(m.circ)
    yield m
    m.close()


def test_attached_circuit_changes_no_proof_and_names_the_constraints(made):
    m = made
    js, proof, ok = m.p.prove_mem_verified(m.witness, R_INJ, S_INJ)
    assert ok == 1 and len(proof) == 256 and m.p.last_device_ms > 0
    assert js == ol.prove_files(m.zk, m.wt, R_INJ, S_INJ)
    assert m.p.last_check() == (SATISFIED, 0, [])
    assert_capped(m.p, [])
    w2, want = breaking_witness(m)
    js, proof, ok = m.p.prove_mem_verified(rb.witness_bytes(w2), R_INJ, S_INJ)
    assert ok == 0 and js and m.p.last_device_ms > 0              # the pairing agrees with the verdict; a proof is still written
    assert_capped(m.p, want)
    for c in sorted({want[0], want[-1]}):
        assert m.circ.values(c) == rb.values(*m.rows, w2, c)
    assert m.circ.check_prover(m.p)[1].tolist() == want           # the stand-alone call keeps working on the attached object
    assert m.p.prove_mem(m.witness, R_INJ, S_INJ) == ol.prove_files(m.zk, m.wt, R_INJ, S_INJ)
    assert m.p.last_check() == (SATISFIED, 0, [])


# ---------------------------------------------------------------- 2. every entry point
@pytest.fixture(scope="module")
def made130(ctx, tmp_path_factory):
    circuit, w = sr.mixed(130, 2, 1)
    m = Made(ctx, tmp_path_factory.mktemp("checked130"), circuit, w)
    yield m
    m.close()


def test_every_entry_point_runs_the_check(made130, tmp_path):
    m = made130
    w2, want = breaking_witness(m)
    bad, bad_path = rb.witness_bytes(w2), str(tmp_path / "bad.wtns")
    vkb.write_wtns(bad_path, bad)
    calls = {
        "prove_mem": lambda wb, path: (m.p.prove_mem(wb, R_INJ, S_INJ), None),
        "prove_file": lambda wb, path: (m.p.prove_file(path, R_INJ, S_INJ), None),
        "prove_mem_verified": lambda wb, path: m.p.prove_mem_verified(wb, R_INJ, S_INJ)[::2],
        "prove_file_verified": lambda wb, path: m.p.prove_file_verified(path, R_INJ, S_INJ)[::2],
    }
    m.p.set_r1cs(None)
    plain = {name: (call(m.witness, m.wt), call(bad, bad_path)) for name, call in calls.items()}
    assert m.p.last_check() == (NONE, 0, [])
    m.p.set_r1cs(m.circ)
    try:
        good_js = ol.prove_files(m.zk, m.wt, R_INJ, S_INJ)
        for name, call in calls.items():
            got = call(m.witness, m.wt)
            assert got == plain[name][0] and got[0] == good_js and got[1] in (None, 1), name
            assert m.p.last_check() == (SATISFIED, 0, []), name
            got = call(bad, bad_path)
            assert got == plain[name][1] and got[1] in (None, 0), name
            assert_capped(m.p, want)
    finally:
        m.p.set_r1cs(None)


def test_compact_and_packed_upload(ctx, tmp_path):
    """The smallest shape whose prover uploads in compact form (2^16 + 2 wires): prove_mem packs, prove_compact(_verified)
    take the caller's packing; the check reads the witness the expansion kernels rebuilt."""
    import k16
    key = vkb.build(lambda g, s: np.zeros((len(s), 64 << g), dtype=np.uint8), 65235, 1, 300, seed=11)
    n_wires, rowsA, rowsB, rowsC, n_pub_in = rb.from_shape(key["shape"])
    assert n_wires == (1 << 16) + 2
    good = key["witness"]
    bad = good.copy()
    bad[key["shape"]["prods"][7][0]] = np.frombuffer((99).to_bytes(32, "little"), dtype=np.uint8)
    want = rb.check(rowsA, rowsB, rowsC, rb.witness_ints(bad))
    assert want and rb.check(rowsA, rowsB, rowsC, rb.witness_ints(good)) == []
    circ = k16.R1cs(ctx, rb.write(n_wires, rowsA, rowsB, rowsC, n_pub_in=n_pub_in))
    try:
        zk = str(tmp_path / "packed.zkey")
        open(zk, "wb").write(circ.setup(sr.TRAPDOOR))
        p, V = k16.Prover(ctx, zk), k16.VerifyingKey.from_zkey(ctx, zk)
        try:
            p.set_vk(V)
            narrow, idx, val = p.compact_buffers()

            def compact(wb, verified):
                wide = np.flatnonzero(wb[:, 1:].any(axis=1))
                narrow[:] = wb[:, 0]
                narrow[wide] = 0
                idx[:len(wide)] = wide
                val[:len(wide)] = wb[wide]
                return p.prove_compact_verified(len(wide), R_INJ, S_INJ)[::2] if verified else (p.prove_compact(len(wide), R_INJ, S_INJ), None)

            plain = {(which, v): compact(wb, v) for which, wb in (("good", good), ("bad", bad)) for v in (False, True)}
            plain_mem = p.prove_mem(good, R_INJ, S_INJ)
            assert p.last_check() == (NONE, 0, [])
            p.set_r1cs(circ)
            for v in (False, True):
                assert compact(good, v) == plain["good", v] and plain["good", v][1] in (None, 1)
                assert p.last_check() == (SATISFIED, 0, [])
                assert compact(bad, v) == plain["bad", v] and plain["bad", v][1] in (None, 0)
                assert_capped(p, want)
            assert p.prove_mem(good, R_INJ, S_INJ) == plain_mem == plain["good", False][0]     # the packed upload of prove_mem
            assert p.last_check() == (SATISFIED, 0, [])
            p.prove_mem(bad, R_INJ, S_INJ)
            assert_capped(p, want)
            assert circ.values(want[0]) == rb.values(rowsA, rowsB, rowsC, rb.witness_ints(bad), want[0])
        finally:
            p.close()
            V.close()
    finally:
        circ.close()


# ---------------------------------------------------------------- 3. the summary kernel's edges
def short_rows_circuit(M, n_wires=40, seed=3):
    """M constraints of 1-2-term rows over n_wires wires and an assignment that satisfies them (C's last coefficient solved for)"""
    rng = pm.SplitMix64(seed * 104729 + M)
    w = [1] + [1 + rng.below(R - 1) for _ in range(n_wires - 1)]
    rowsA, rowsB, rowsC = [], [], []
    for c in range(M):
        a = [(1 + c % (n_wires - 1), 1 + rng.next() % 1000)] + ([(1 + (c // 3) % (n_wires - 1), 7)] if c % 3 == 0 else [])
        b = [(1 + (c * 7) % (n_wires - 1), 1 + rng.next() % 1000)] + ([(0, 5)] if c % 5 == 0 else [])
        head = [(1 + (c * 11) % (n_wires - 1), 3)] if c % 2 else []
        k = 1 + (c * 13) % (n_wires - 1)
        target = rb.dot(a, w) * rb.dot(b, w) % R
        rowsA.append(a), rowsB.append(b)
        rowsC.append(head + [(k, (target - rb.dot(head, w)) * pow(w[k], -1, R) % R)])
    return n_wires, rowsA, rowsB, rowsC, w


class Keyed:
    """A short-rows circuit, its set-up key and a prover; attach(where) attaches the circuit with C off by one in `where`"""

    def __init__(self, ctx, tmp, M):
        import k16
        self.ctx, self.M = ctx, M
        self.n_wires, self.A, self.B, self.Cc, self.w = short_rows_circuit(M)
        assert rb.check(self.A, self.B, self.Cc, self.w) == []
        self.wb = rb.witness_bytes(self.w)
        base = k16.R1cs(ctx, rb.write(self.n_wires, self.A, self.B, self.Cc))
        try:
            zk = str(tmp / ("short%d.zkey" % M))
            open(zk, "wb").write(base.setup(sr.TRAPDOOR))
        finally:
            base.close()
        self.p = k16.Prover(ctx, zk)

    def verdict(self, where):
        """(last_check of a proof of the satisfying witness under the planted circuit, the reference checker's list)"""
        import k16
        bad_c = c_off_by_one(self.Cc, set(where))
        want = rb.check(self.A, self.B, bad_c, self.w)
        circ = k16.R1cs(self.ctx, rb.write(self.n_wires, self.A, self.B, bad_c))
        try:
            self.p.set_r1cs(circ)
            assert self.p.last_check() == (NONE, 0, [])
            self.p.prove_mem(self.wb, R_INJ, S_INJ)
            got = self.p.last_check(REPORT_MAX + 6)
            if want:
                assert circ.values(want[-1]) == rb.values(self.A, self.B, bad_c, self.w, want[-1])
        finally:
            self.p.set_r1cs(None)
            circ.close()
        return got, want

    def close(self):
        self.p.close()


M_BIG = 20000
# the kernel's tile is 256 mask words = 2^14 constraints: its boundaries are the k = 14 case
PLANTED = {
    "none": [], "first": [0], "last": [M_BIG - 1], "all": list(range(M_BIG)), "every_third": list(range(0, M_BIG, 3)),
    "last_70": list(range(M_BIG - 70, M_BIG)), "exactly_64": list(range(100, 100 + 64 * 300, 300)),
    "exactly_65": list(range(100, 100 + 65 * 300, 300)),
}
PLANTED.update({"around_2^%d" % k: [2 ** k - 1, 2 ** k, 2 ** k + 1] for k in range(6, 15)})


@pytest.fixture(scope="module")
def big(ctx, tmp_path_factory):
    k = Keyed(ctx, tmp_path_factory.mktemp("short_rows"), M_BIG)
    yield k
    k.close()


@pytest.mark.parametrize("name", list(PLANTED))
def test_summary_of_planted_failures(big, name):
    where = PLANTED[name]
    assert len(PLANTED["exactly_64"]) == 64 and len(PLANTED["exactly_65"]) == 65 and max(PLANTED["exactly_65"]) < M_BIG
    got, want = big.verdict(where)
    assert want == sorted(where)
    assert got == (BROKEN if want else SATISFIED, len(want), want[:REPORT_MAX])


@pytest.mark.parametrize("M", [1, 63, 64, 65, 129])
def test_summary_small_circuits_all_or_none_failing(ctx, tmp_path, M):
    k = Keyed(ctx, tmp_path, M)
    try:
        for where in ([], list(range(M))):
            got, want = k.verdict(where)
            assert want == where
            assert got == (BROKEN if want else SATISFIED, len(want), want[:REPORT_MAX])
    finally:
        k.close()


# ---------------------------------------------------------------- 4. refused witnesses, lifecycle, attach refusals
def outcome(call):
    import k16
    try:
        return call()
    except k16.K16Error as e:
        return ("error", e.rc)


def test_refused_witnesses(made130):
    import k16
    m = made130
    n_wires = m.circuit[0]
    for wire, value in ((n_wires - 1, R), (0, 2)):
        bad = list(m.w)
        bad[wire] = value
        wb = rb.witness_bytes(bad)
        m.p.set_r1cs(None)
        plain = [outcome(lambda: m.p.prove_mem(wb, R_INJ, S_INJ)), outcome(lambda: m.p.prove_mem_verified(wb, R_INJ, S_INJ))]
        m.p.set_r1cs(m.circ)
        try:
            m.p.prove_mem(m.witness, R_INJ, S_INJ)
            assert m.p.last_check() == (SATISFIED, 0, []) and m.circ.values(0) == rb.values(*m.rows, m.w, 0)
            for k, call in enumerate((lambda: m.p.prove_mem(wb, R_INJ, S_INJ), lambda: m.p.prove_mem_verified(wb, R_INJ, S_INJ))):
                assert outcome(call) == plain[k], (wire, k)
                if plain[k][0] != "error":
                    assert m.p.last_check() == (REFUSED, 0, []), (wire, k)
                    with pytest.raises(k16.K16Error) as e:
                        m.circ.values(0)                          # a refused witness completes no check
                    assert e.value.rc == ERR_ARG
                else:
                    assert m.p.last_check() == (NONE, 0, []), (wire, k)
            assert plain[0][0] != "error"                         # (the plain prove call takes any 32-byte values)
        finally:
            m.p.set_r1cs(None)


def test_lifecycle(ctx, made130):
    import k16
    m = made130
    p = k16.Prover(ctx, m.zk)
    try:
        assert p.last_check() == (NONE, 0, [])                    # the create-time warm-up is no prove call
        p.prove_mem(m.witness, R_INJ, S_INJ)
        assert p.last_check() == (NONE, 0, [])                    # nothing attached
        p.set_r1cs(m.circ)
        assert p.last_check() == (NONE, 0, [])
        w2, want = breaking_witness(m)
        p.prove_mem(rb.witness_bytes(w2), R_INJ, S_INJ)
        assert p.last_check() == (BROKEN, len(want), want[:REPORT_MAX])
        with pytest.raises(k16.K16Error) as e:
            p.prove_mem(m.witness[:-1], R_INJ, S_INJ)             # a wrong witness length
        assert e.value.rc == ERR_FORMAT
        assert p.last_check() == (NONE, 0, [])
        p.prove_mem(m.witness, R_INJ, S_INJ)
        assert p.last_check() == (SATISFIED, 0, [])
        p.set_r1cs(None)
        assert p.last_check() == (NONE, 0, [])
        p.prove_mem(rb.witness_bytes(w2), R_INJ, S_INJ)
        assert p.last_check() == (NONE, 0, [])
    finally:
        p.close()


def test_attach_refusals_and_a_correct_call_afterwards(ctx, made130):
    import k16
    m = made130
    n_wires, rowsA, rowsB, rowsC, n_pub_out, n_pub_in = m.circuit
    other_ctx = k16.Context(0)
    strangers = []
    try:
        strangers.append(k16.R1cs(other_ctx, m.r1cs_bytes))                                       # another context
        sw, sA, sB, sC, _ = mixed_circuit(65)
        assert sw != n_wires
        strangers.append(k16.R1cs(ctx, rb.write(sw, sA, sB, sC, n_pub_out=n_pub_out, n_pub_in=n_pub_in)))   # another wire count
        strangers.append(k16.R1cs(ctx, rb.write(n_wires, rowsA, rowsB, rowsC, n_pub_out=n_pub_out + 1, n_pub_in=n_pub_in)))
        m.p.set_r1cs(m.circ)
        for s in strangers:
            with pytest.raises(k16.K16Error) as e:
                m.p.set_r1cs(s)
            assert e.value.rc == ERR_ARG
        m.p.prove_mem(m.witness, R_INJ, S_INJ)                    # the refusals left the attached circuit in place
        assert m.p.last_check() == (SATISFIED, 0, [])
    finally:
        m.p.set_r1cs(None)
        for s in strangers:
            s.close()
        other_ctx.close()


# ---------------------------------------------------------------- 5. two provers, alternating witnesses
def test_two_provers_sharing_a_key_alternate_good_and_broken_witnesses(made130):
    import k16
    m = made130
    w2, want = breaking_witness(m)
    bad = rb.witness_bytes(w2)
    ctxs = [k16.Context(0), k16.Context(0)]
    provers, circs, verdicts = [], [], [[], []]
    try:
        provers.append(k16.Prover(ctxs[0], m.zk))
        provers.append(k16.Prover(ctxs[1], m.zk, share_key_of=provers[0]))
        for c, p in zip(ctxs, provers):
            circs.append(k16.R1cs(c, m.r1cs_bytes))
            p.set_r1cs(circs[-1])

        def work(k):
            for i in range(10):
                provers[k].prove_mem(bad if (i + k) % 2 else m.witness, R_INJ, S_INJ)
                verdicts[k].append(provers[k].last_check())

        threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        for k in range(2):
            assert verdicts[k] == [(BROKEN, len(want), want[:REPORT_MAX]) if (i + k) % 2 else (SATISFIED, 0, []) for i in range(10)]
    finally:
        for p in provers[::-1]:
            p.close()
        for c in circs:
            c.close()
        for c in ctxs:
            c.close()


# ---------------------------------------------------------------- 6. footprint
def free_device_bytes():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_attach_detach_destroy_leave_no_device_allocation(ctx, made130):
    """One cycle = an R1CS object made, (attached,) a proof, (detached,) the object destroyed.  What the cycle with the
    attachment leaves allocated is at most what the same cycle leaves without it."""
    import k16
    m = made130

    def cycle(attach):
        before = free_device_bytes()
        circ = k16.R1cs(ctx, m.r1cs_bytes)
        if attach:
            m.p.set_r1cs(circ)
        m.p.prove_mem(m.witness, R_INJ, S_INJ)
        assert m.p.last_check()[0] == (SATISFIED if attach else NONE)
        m.p.set_r1cs(None)
        circ.close()
        ctx.sync()
        return before - free_device_bytes()

    cycle(True), cycle(False)                                     # (whatever the runtime sets up on first use)
    leak_plain = max(cycle(False), 0)
    assert cycle(True) <= leak_plain
