"""-m gpu : the R1CS witness check (include/k16.h k16_r1cs_*, csrc/r1cs_check.hip) against the reference checker of
tests/r1cs_builder.py (Python big integers, row by row): which constraints a witness breaks, as an exact count and an
ascending list; the values A.w, B.w, C.w of a constraint; the three witness sources; and the purpose -- after a verified
prove has rejected a proof, the check names the constraints."""
import functools

import numpy as np
import pytest

import pymodel as pm
import r1cs_builder as rb
import valid_key_builder as vkb

pytestmark = pytest.mark.gpu

R = pm.R
ERR_ARG, ERR_FORMAT = -3, -5
R_INJ, S_INJ = pm.limbs(pm.SplitMix64(191).below(R)), pm.limbs(pm.SplitMix64(192).below(R))
EDGE_LENGTHS = [0, 1, 63, 64, 65, 200]


@pytest.fixture(scope="module")
def ctx():
    import k16
    c = k16.Context(0)
    yield c
    c.close()


def row_length(c, k):
    """Length of row c of matrix k: the edge lengths in every matrix (at different constraints), short rows between them."""
    j = (c + 2 * k) % 32
    return EDGE_LENGTHS[j] if j < 6 else (c + k) % 4


@functools.lru_cache(maxsize=None)
def mixed_circuit(M, seed=1):
    """(n_wires, rowsA, rowsB, rowsC, w): random rows of row_length() terms and an assignment that satisfies them -- the last
    coefficient of C (of B where C is empty) is solved for.  Wires: 60 % bits and bytes, the rest full-width values."""
    rng = pm.SplitMix64(seed * 7919 + M)
    n_wires = 260
    w = [1] + [(rng.next() & 0xFF if rng.next() % 10 < 6 else 1 + rng.below(R - 1)) for _ in range(n_wires - 1)]
    nonzero = [i for i in range(n_wires) if w[i]]

    def row(n):
        r = [(x % n_wires, x * (R // 3) % R) for x in (rng.next() for _ in range(n))]          # full-width coefficients
        if n:
            r[-1] = (nonzero[rng.next() % len(nonzero)], r[-1][1])
        return r

    def solved(r, target):
        """r with its last coefficient chosen so that r.w = target"""
        (s, _), head = r[-1], r[:-1]
        return head + [(s, (target - rb.dot(head, w)) * pow(w[s], -1, R) % R)]

    rowsA, rowsB, rowsC = [], [], []
    for c in range(M):
        a, b, cc = row(row_length(c, 0)), row(row_length(c, 1)), row(row_length(c, 2))
        if cc:
            cc = solved(cc, rb.dot(a, w) * rb.dot(b, w) % R)
        elif b:
            b = solved(b, 0)
        rowsA.append(a), rowsB.append(b), rowsC.append(cc)
    assert rb.check(rowsA, rowsB, rowsC, w) == []
    return n_wires, rowsA, rowsB, rowsC, w


def c_off_by_one(rowsC, where):
    """C.w of the constraints in `where` raised by exactly 1 (wire 0 = 1): nothing but the C side changes."""
    return [r + [(0, 1)] if c in where else r for c, r in enumerate(rowsC)]


def assert_capped_lists(circ, wb, want):
    """cap below, equal to and above the count: the exact count and the lowest constraint numbers, ascending"""
    n = len(want)
    for cap in sorted({0, 1, max(n - 1, 0), n, n + 1, n + 70}):
        got_n, got = circ.check(wb, cap=cap)
        assert got_n == n and got.tolist() == want[:cap], cap
    got_n, got = circ.check(wb)
    assert got_n == n and got.tolist() == want


@pytest.mark.parametrize("M", [1, 63, 64, 65, 129, 5000])
def test_layout_and_mask_edges_against_the_reference_checker(ctx, M):
    import k16
    n_wires, rowsA, rowsB, rowsC, w = mixed_circuit(M)
    wb = rb.witness_bytes(w)
    circ = k16.R1cs(ctx, rb.write(n_wires, rowsA, rowsB, rowsC))
    try:
        info = circ.info()
        assert (info["n_wires"], info["n_constraints"]) == (n_wires, M)
        assert info["n_terms"] == sum(len(r) for mat in (rowsA, rowsB, rowsC) for r in mat)
        assert_capped_lists(circ, wb, [])
        for c in sorted({0, M // 2, M - 1}):
            assert circ.values(c) == rb.values(rowsA, rowsB, rowsC, w, c)
        # a changed wire: whatever the reference checker names (rows on all three sides use it)
        w2 = list(w)
        w2[7] = (w2[7] + 1) % R
        want = rb.check(rowsA, rowsB, rowsC, w2)
        assert want or M < 3
        assert_capped_lists(circ, rb.witness_bytes(w2), want)
        if want:
            assert circ.values(want[0]) == rb.values(rowsA, rowsB, rowsC, w2, want[0])
    finally:
        circ.close()
    # failures planted on the C side only, off by exactly 1: at the edges of the mask words, then in every constraint
    for where in (sorted({0, 63, 64, M - 1} & set(range(M))), list(range(M))):
        bad_c = c_off_by_one(rowsC, set(where))
        assert rb.check(rowsA, rowsB, bad_c, w) == where
        circ = k16.R1cs(ctx, rb.write(n_wires, rowsA, rowsB, bad_c))
        try:
            assert_capped_lists(circ, wb, where)
            a, b, c = circ.values(where[-1])
            assert (a, b, c) == rb.values(rowsA, rowsB, bad_c, w, where[-1]) and (a * b + 1) % R == c
            if len(where) < M:
                ok_row = next(i for i in range(M) if i not in where)
                assert circ.values(ok_row) == rb.values(rowsA, rowsB, bad_c, w, ok_row)
        finally:
            circ.close()


def test_field_extremes_row_sums_beyond_r(ctx):
    """Coefficients and wires of r - 1 in rows of 1 / 64 / 65 / 200 terms: every product is 1 or r - 1, the row sums pass r many
    times over and their lazy representatives are not canonical; a * b = c holds only after reduction."""
    import k16
    n_wires = 210
    w = [1] + [R - 1] * (n_wires - 3) + [255, 256]
    ones = lambda n: [(1 + i, R - 1) for i in range(n)]          # n terms (r-1)(r-1) = 1 each: n
    minus = lambda n: [(0, R - 1)] * n                            # n terms (r-1) * 1, the same wire n times: -n
    rowsA, rowsB, rowsC = [], [], []
    for n in (1, 64, 65, 200):
        rowsA.append(ones(1)), rowsB.append(ones(n)), rowsC.append(ones(n))              # 1 * n = n
        rowsA.append(minus(n)), rowsB.append(ones(1)), rowsC.append(minus(n))            # -n * 1 = -n
        rowsA.append(minus(n)), rowsB.append(minus(n)), rowsC.append([(0, n * n)])       # (-n)(-n) = n^2
        rowsA.append(ones(n)), rowsB.append(minus(1)), rowsC.append(minus(n))            # n * -1 = -n
    rowsA.append([(n_wires - 2, R - 1), (n_wires - 1, R - 1)])   # values 255 | 256 side by side: the narrow and the wide path
    rowsB.append([(n_wires - 2, 1), (n_wires - 1, 1)])
    rowsC.append([(0, (R - 511) * 511 % R)])
    M = len(rowsA)
    assert rb.check(rowsA, rowsB, rowsC, w) == []
    wb = rb.witness_bytes(w)
    circ = k16.R1cs(ctx, rb.write(n_wires, rowsA, rowsB, rowsC))
    try:
        n, idx = circ.check(wb)
        assert n == 0 and idx.tolist() == []
        for c in range(M):
            assert circ.values(c) == rb.values(rowsA, rowsB, rowsC, w, c), c
    finally:
        circ.close()
    for delta in (1, R - 1):                                      # the same cases with C changed by 1, up and down
        bad_c = [r + [(0, delta)] for r in rowsC]
        assert rb.check(rowsA, rowsB, bad_c, w) == list(range(M))
        circ = k16.R1cs(ctx, rb.write(n_wires, rowsA, rowsB, bad_c))
        try:
            n, idx = circ.check(wb)
            assert n == M and idx.tolist() == list(range(M))
        finally:
            circ.close()


def test_refused_witnesses(ctx):
    import k16
    n_wires, rowsA, rowsB, rowsC, w = mixed_circuit(65)
    circ = k16.R1cs(ctx, rb.write(n_wires, rowsA, rowsB, rowsC))
    try:
        with pytest.raises(k16.K16Error) as e:
            circ.values(0)                                        # no check yet
        assert e.value.rc == ERR_ARG
        for wrong in (w[:-1], w + [0]):                           # not the circuit's number of wires
            with pytest.raises(k16.K16Error) as e:
                circ.check(rb.witness_bytes(wrong))
            assert e.value.rc == ERR_ARG
        assert circ.check(rb.witness_bytes(w))[0] == 0
        # wire 200 is used by no row of this check's making: the witness is refused for what it IS
        for wire, value in ((200, R), (200, 2 ** 256 - 1), (n_wires - 1, R), (0, 0), (0, 2), (0, 256), (0, R + 1)):
            bad = list(w)
            bad[wire] = value
            with pytest.raises(k16.K16Error) as e:
                circ.check(rb.witness_bytes(bad))
            assert e.value.rc == ERR_FORMAT, (wire, value)
            with pytest.raises(k16.K16Error) as e:
                circ.values(0)                                    # a refused witness completes no check
            assert e.value.rc == ERR_ARG
        top = list(w)
        top[200] = R - 1                                          # the largest value there is
        assert circ.check(rb.witness_bytes(top))[0] == len(rb.check(rowsA, rowsB, rowsC, top))
        assert circ.check(rb.witness_bytes(w))[0] == 0            # the object is fine after the refusals
        with pytest.raises(k16.K16Error) as e:
            circ.values(65)
        assert e.value.rc == ERR_ARG
    finally:
        circ.close()


class Key:
    """A valid synthetic key with its prover, the key's own verification key attached, and its circuit as an R1cs object."""

    def __init__(self, ctx, tmp, shape, seed):
        import k16
        key = vkb.build(lambda g, s: ctx.synth_points_scalars(g, s), *shape, seed=seed)
        self.zkey, self.shape, self.witness = key["zkey"], key["shape"], key["witness"]
        self.zk, self.wt = str(tmp / "v.zkey"), str(tmp / "v.wtns")
        open(self.zk, "wb").write(self.zkey)
        vkb.write_wtns(self.wt, self.witness)
        self.rows = rb.from_shape(self.shape)[1:4]
        self.r1cs_bytes = rb.write_from_shape(self.shape)
        self.p = k16.Prover(ctx, self.zk)
        self.V = k16.VerifyingKey.from_zkey(ctx, self.zk)
        self.p.set_vk(self.V)
        self.circ = k16.R1cs(ctx, self.r1cs_bytes)

    def reference(self, wb):
        return rb.check(*self.rows, rb.witness_ints(wb))

    def altered(self, wire, value):
        bad = self.witness.copy()
        bad[wire] = np.frombuffer(int(value).to_bytes(32, "little"), dtype=np.uint8)
        return bad

    def close(self):
        self.circ.close()
        self.p.close()
        self.V.close()


@pytest.fixture(scope="module")
def small_key(ctx, tmp_path_factory):
    k = Key(ctx, tmp_path_factory.mktemp("r1cs_small"), (300, 40, 120), seed=5)
    yield k
    k.close()


@pytest.fixture(scope="module")
def packed_key(ctx, tmp_path_factory):
    """The smallest valid key whose prover uploads in compact form: 2^16 + 2 wires."""
    k = Key(ctx, tmp_path_factory.mktemp("r1cs_packed"), (65235, 1, 300), seed=11)
    yield k
    k.close()


def test_circuit_and_key_belong_together(small_key):
    k = small_key
    assert k.circ.match_zkey(k.zkey) == 0
    n_wires, rowsA, rowsB, rowsC, n_pub = rb.from_shape(k.shape)
    import k16
    other = k16.R1cs(k.circ.ctx, rb.write(n_wires, rowsB, rowsA, rowsC, n_pub_in=n_pub))
    try:
        assert other.match_zkey(k.zkey) == 2 and "constraint 0, wire 0" in other.last_error()
    finally:
        other.close()


def test_three_sources_agree(ctx, small_key, tmp_path):
    import k16
    k = small_key
    fresh = k16.Prover(ctx, k.zk)
    try:
        with pytest.raises(k16.K16Error) as e:
            k.circ.check_prover(fresh)                            # no prove call yet (the warm-up of create is none)
        assert e.value.rc == ERR_ARG
    finally:
        fresh.close()
    prods = k.shape["prods"]
    bad = k.altered(prods[len(prods) // 2][0], 12345)
    bad_path = str(tmp_path / "bad.wtns")
    vkb.write_wtns(bad_path, bad)
    for wb, path in ((k.witness, k.wt), (bad, bad_path)):
        want = k.reference(wb)
        assert bool(want) == (wb is bad)
        from_mem, from_file = k.circ.check(wb), k.circ.check_file(path)
        k.p.prove_mem(wb, R_INJ, S_INJ)
        from_prover = k.circ.check_prover(k.p)
        for n, idx in (from_mem, from_file, from_prover):
            assert n == len(want) and idx.tolist() == want
    with pytest.raises(k16.K16Error) as e:                        # a failed prove leaves no complete witness behind
        k.p.prove_mem(k.witness[:-1], R_INJ, S_INJ)
    assert e.value.rc == ERR_FORMAT
    with pytest.raises(k16.K16Error) as e:
        k.circ.check_prover(k.p)
    assert e.value.rc == ERR_ARG
    other_ctx = k16.Context(0)
    try:
        elsewhere = k16.R1cs(other_ctx, k.r1cs_bytes)
        k.p.prove_mem(k.witness, R_INJ, S_INJ)
        with pytest.raises(k16.K16Error) as e:
            elsewhere.check_prover(k.p)                           # an R1CS object of another context
        assert e.value.rc == ERR_ARG
        assert elsewhere.check(k.witness)[0] == 0
        elsewhere.close()
    finally:
        other_ctx.close()
    n_wires, rowsA, rowsB, rowsC, _ = mixed_circuit(65)
    stranger = k16.R1cs(ctx, rb.write(n_wires, rowsA, rowsB, rowsC))
    try:
        with pytest.raises(k16.K16Error) as e:
            stranger.check_prover(k.p)                            # another circuit: nWires is not the key's nVars
        assert e.value.rc == ERR_ARG
        with pytest.raises(k16.K16Error) as e:
            stranger.check_file(k.wt)
        assert e.value.rc == ERR_FORMAT
    finally:
        stranger.close()
    n, idx = k.circ.check_prover(k.p)                             # the refusals left the prover's witness where it was
    assert n == 0 and idx.tolist() == []


def test_prover_witness_after_compact_and_packed_upload(packed_key):
    """At 2^16 + 2 wires prove_mem packs its upload and prove_compact takes the caller's packing: the witness the check reads
    in place was rebuilt on the device by the expansion kernels."""
    k = packed_key
    assert k.circ.match_zkey(k.zkey) == 0
    narrow, idx, val = k.p.compact_buffers()
    prods = k.shape["prods"]
    for wb in (k.witness, k.altered(prods[7][0], 99), k.altered(k.shape["bit0"] + 40000, 2)):
        want = k.reference(wb)
        assert bool(want) == (wb is not k.witness)
        k.p.prove_mem(wb, R_INJ, S_INJ)
        n, got = k.circ.check_prover(k.p)
        assert n == len(want) and got.tolist() == want
        wide = np.flatnonzero(wb[:, 1:].any(axis=1))
        narrow[:] = wb[:, 0]
        narrow[wide] = 0
        idx[:len(wide)] = wide
        val[:len(wide)] = wb[wide]
        k.p.prove_compact(len(wide), R_INJ, S_INJ)
        n, got = k.circ.check_prover(k.p)
        assert n == len(want) and got.tolist() == want
        n, got = k.circ.check(wb)
        assert n == len(want) and got.tolist() == want


def test_rejected_proof_then_the_check_names_the_constraints(small_key):
    k = small_key
    js, proof, ok = k.p.prove_mem_verified(k.witness, R_INJ, S_INJ)
    assert ok == 1 and k.circ.check_prover(k.p)[0] == 0
    sh, prods = k.shape, k.shape["prods"]
    used = {x for pr in prods for x in pr[1:4]}
    byte_wire = next(i for i in range(sh["byte0"], sh["prod0"]) if i in used)
    cases = {
        "product wire": k.altered(prods[3][0], (int.from_bytes(k.witness[prods[3][0]].tobytes(), "little") + 1) % R),
        "bit wire = 2": k.altered(sh["bit0"] + 17, 2),
        "byte wire": k.altered(byte_wire, int(k.witness[byte_wire, 0]) ^ 0x55),
    }
    for what, wb in cases.items():
        want = k.reference(wb)
        assert want, what
        js, proof, ok = k.p.prove_mem_verified(wb, R_INJ, S_INJ)
        assert ok == 0, what
        n, got = k.circ.check_prover(k.p)
        assert n == len(want) and got.tolist() == want, what
        a, b, c = k.circ.values(want[0])
        assert (a, b, c) == rb.values(*k.rows, rb.witness_ints(wb), want[0]) and a * b % R != c


def test_toy_circuit_matches_the_reference_made_key_and_accepts_its_witness(ctx, toy_paths):
    import k16
    zkey, wtns, _ = toy_paths
    toy = k16.R1cs(ctx, rb.write(3, [[(1, R - 1)]], [[(2, 1)]], [[(0, R - 6)]], n_pub_out=1))
    try:
        assert toy.info() == dict(n_wires=3, n_public=1, n_constraints=1, n_terms=3)
        assert toy.match_zkey(open(zkey, "rb").read()) == 0
        n, idx = toy.check_file(wtns)
        assert n == 0 and idx.tolist() == []
        assert toy.values(0) == (R - 2, 3, R - 6)
        n, idx = toy.check(rb.witness_bytes([1, 2, 4]))
        assert n == 1 and idx.tolist() == [0]
    finally:
        toy.close()
