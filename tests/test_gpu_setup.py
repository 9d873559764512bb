"""-m gpu : the set-up from a trapdoor (include/k16.h k16_r1cs_setup*, k16_generator_mul; csrc/setup.hip) against the Python
big-integer reference of tests/setup_reference.py with points from the CPU oracle (valid_key_builder.oracle_points): the key
is byte-equal to the reference's, the prover proves with it and the proofs verify.  All arithmetic is exact: every comparison
is byte equality."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import oracle_lib as ol
import pymodel as pm
import r1cs_builder as rb
import setup_reference as sr
import valid_key_builder as vkb

pytestmark = pytest.mark.gpu

R = pm.R
ERR_ARG, ERR_BUFFER = -3, -7
R_INJ, S_INJ = pm.limbs(pm.SplitMix64(291).below(R)), pm.limbs(pm.SplitMix64(292).below(R))
G1, G2 = 0, 1


@pytest.fixture(scope="module")
def ctx():
    import k16
    c = k16.Context(0)
    yield c
    c.close()


def oracle(group, scalars):
    return vkb.oracle_points(group, [int(s) for s in scalars])


# ---------------------------------------------------------------- 1. k16_generator_mul
def directed_scalars(group):
    """Extremal scalars, and -- from k16_generator_mul_info's w -- the scalars whose LAST window addition doubles or cancels.
    The kernel walks the windows low to high with unsigned digits: after the windows below k the accumulator is
    (s mod 2^(wk)) G, the table entry is d_k 2^(wk) G.
      s = P + D 2^(wk), k the top window, D = ceil(r / 2^(wk)), P = D 2^(wk) - r: the top addition adds (P + r) G to P G -- it doubles
      s = r, s = 2r: the top addition adds -(s mod 2^(wk)) G -- it cancels
      s = r + 2 d0, d0 = (-r) mod 2^w: the scalar whose last addition doubles in a high-to-low walk, kept for any other order"""
    import k16
    w, n_windows = k16.generator_mul_info(group)
    assert n_windows == (256 + w - 1) // w
    s = [0, 1, 2, R - 1, R, R + 1, 2 * R, 2 * R + 1, 2 ** 256 - 1]
    s += [1 << k for k in range(256)]
    s += [(((1 << w) - 1) << (w * k)) & (2 ** 256 - 1) for k in range(n_windows)]
    d0 = (-R) % (1 << w)
    s.append(R + 2 * d0)
    k = n_windows - 1
    D = -(-R // (1 << (w * k)))
    P = D * (1 << (w * k)) - R
    assert 0 <= P < (1 << (w * k)) and (P + (D << (w * k))) < 2 ** 256
    s.append(P + (D << (w * k)))
    for lower in range(1, n_windows):          # the same two cases at every window boundary: the addition of window `lower`
        m = 1 << (w * lower)
        Dl = -(-R // m)
        if (Dl * m - R) + Dl * m < 2 ** 256 and Dl < (1 << w):
            s.append((Dl * m - R) + Dl * m)
    return s


@pytest.mark.parametrize("group", [G1, G2])
def test_generator_mul_directed_scalars(ctx, group):
    s = directed_scalars(group)
    got = ctx.generator_mul(group, s)
    assert np.array_equal(got, ctx.synth_points_scalars_raw(group, s))
    assert np.array_equal(got, oracle(group, s))
    zero = [i for i, x in enumerate(s) if x % R == 0]
    assert len(zero) >= 3 and not got[zero].any()                 # 0, r, 2r: the all-zero affine point


@pytest.mark.parametrize("group", [G1, G2])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_generator_mul_random_256_bit_scalars(ctx, group, n):
    rs = np.random.RandomState(1000 * group + n)
    s = rs.randint(0, 256, size=(n, 32), dtype=np.uint8)          # any 256-bit value, most of them above r
    got = ctx.generator_mul(group, s)
    assert got.shape == (n, 64 << group)
    assert np.array_equal(got, ctx.synth_points_scalars_raw(group, s))
    k = min(n, 65)                                                # the oracle on the first and the last rows
    ints = [int.from_bytes(row.tobytes(), "little") for row in np.concatenate([s[:k], s[-k:]])]
    assert np.array_equal(np.concatenate([got[:k], got[-k:]]), oracle(group, ints))


# ---------------------------------------------------------------- 2. / 3. the keys
class Made:
    """A circuit, the key the set-up makes for it, and a prover with the key's own verification key attached."""

    def __init__(self, ctx, tmp, circuit, witness, trapdoor=sr.TRAPDOOR):
        import k16
        self.circuit, self.w = circuit, witness
        n_wires, rowsA, rowsB, rowsC, n_pub_out, n_pub_in = circuit
        self.rows, self.n_public = (rowsA, rowsB, rowsC), n_pub_out + n_pub_in
        self.r1cs_bytes = rb.write(n_wires, rowsA, rowsB, rowsC, n_pub_out=n_pub_out, n_pub_in=n_pub_in)
        self.circ = k16.R1cs(ctx, self.r1cs_bytes)
        self.zkey = self.circ.setup(trapdoor)
        self.zk, self.wt = str(tmp / "s.zkey"), str(tmp / "s.wtns")
        open(self.zk, "wb").write(self.zkey)
        self.witness = rb.witness_bytes(witness)
        vkb.write_wtns(self.wt, self.witness)
        self.p = k16.Prover(ctx, self.zk)
        self.V = k16.VerifyingKey.from_zkey(ctx, self.zk)
        self.p.set_vk(self.V)
        self.public = [int(x) for x in witness[1:1 + self.n_public]]

    def close(self):
        self.p.close()
        self.V.close()
        self.circ.close()


@functools.lru_cache(maxsize=None)
def reference_key(shape):
    return sr.zkey(sr.mixed(*shape)[0], sr.TRAPDOOR, oracle)


@pytest.fixture(scope="module", params=sr.MIXED_SHAPES, ids=lambda s: "M%d_out%d_in%d" % s)
def made(request, ctx, tmp_path_factory):
    circuit, w = sr.mixed(*request.param)
    m = Made(ctx, tmp_path_factory.mktemp("setup"), circuit, w)
    m.shape = request.param
    yield m
    m.close()


def test_whole_key_is_byte_equal_to_the_references(made):
    want = reference_key(made.shape)
    assert made.circ.setup_size() == len(want) == len(made.zkey)
    got, ref = sr.sections(made.zkey), sr.sections(want)
    for k in range(1, 11):
        assert got[k] == ref[k], "section %d" % k
    assert made.zkey == want
    n_wires = made.circuit[0]
    for k, width in ((5, 64), (6, 64), (7, 128)):                 # the wire in no constraint: A, B1, B2 all-zero points
        assert not any(got[k][(n_wires - 1) * width:])
    assert not any(got[8][-64:])                                  # ... and C


def test_key_end_to_end(ctx, made, tmp_path):
    import k16
    m = made
    assert k16.zkey_check(ctx, m.zkey)["n_bad"] == 0
    assert m.circ.match_zkey(m.zkey) == 0
    n_wires, rowsA, rowsB = m.circuit[0], m.rows[0], m.rows[1]
    assert ol.zkey_info(m.zk) == dict(n_vars=n_wires, n_public=m.n_public, domain_size=sr.domain(len(rowsA), m.n_public),
                                      n_coefs=sum(len(r) for r in rowsA) + sum(len(r) for r in rowsB) + m.n_public + 1)
    js, proof, ok = m.p.prove_mem_verified(m.witness, R_INJ, S_INJ)
    assert ok == 1
    assert js == ol.prove_files(m.zk, m.wt, R_INJ, S_INJ)
    assert m.circ.check_prover(m.p)[0] == 0
    if m.n_public:
        changed = list(m.public)
        changed[-1] = (changed[-1] + 1) % R
        assert m.V.verify_batch([proof, proof], [m.public, changed]) == [True, False]
    # a witness that breaks exactly one constraint
    for wire in range(m.n_public + 1, n_wires):
        w2 = list(m.w)
        w2[wire] = (w2[wire] + 1) % R
        want = rb.check(*m.rows, w2)
        if len(want) == 1:
            break
    assert len(want) == 1
    js, proof, ok = m.p.prove_mem_verified(rb.witness_bytes(w2), R_INJ, S_INJ)
    assert ok == 0
    n, got = m.circ.check_prover(m.p)
    assert n == 1 and got.tolist() == want


def test_toy_circuit_key_proves_the_reference_witness(ctx, tmp_path, toy_paths):
    """The toy circuit through the set-up: section 4 is the reference-made key's, and the reference's own witness file proves."""
    m = Made(ctx, tmp_path, sr.TOY, sr.TOY_WITNESS)
    try:
        golden = sr.sections(open(toy_paths[0], "rb").read())
        assert sr.sections(m.zkey)[4] == golden[4]
        assert m.zkey == sr.zkey(sr.TOY, sr.TRAPDOOR, oracle)
        js, proof, ok = m.p.prove_mem_verified(m.witness, R_INJ, S_INJ)
        assert ok == 1 and js == ol.prove_files(m.zk, toy_paths[1], R_INJ, S_INJ)
    finally:
        m.close()


# ---------------------------------------------------------------- 4. the smallest shape whose prover uploads in compact form
def test_packed_upload_shape_verifies(ctx, tmp_path):
    import k16
    # the builder's circuit and witness; its own set-up runs on all-zero points and is thrown away
    key = vkb.build(lambda g, s: np.zeros((len(s), 64 << g), dtype=np.uint8), 65235, 1, 300, seed=11)
    n_wires, rowsA, rowsB, rowsC, n_pub_in = rb.from_shape(key["shape"])
    assert n_wires == (1 << 16) + 2
    wb, pub = key["witness"], key["public"]
    circ = k16.R1cs(ctx, rb.write(n_wires, rowsA, rowsB, rowsC, n_pub_in=n_pub_in))
    try:
        zkey = circ.setup(sr.TRAPDOOR)
        assert circ.match_zkey(zkey) == 0
        zk = str(tmp_path / "packed.zkey")
        open(zk, "wb").write(zkey)
        p, V = k16.Prover(ctx, zk), k16.VerifyingKey.from_zkey(ctx, zk)
        try:
            p.set_vk(V)
            js, proof, ok = p.prove_mem_verified(wb, R_INJ, S_INJ)
            assert ok == 1 and circ.check_prover(p)[0] == 0
            assert V.verify_batch([proof], [[(pub[0] + 1) % R]]) == [False]
        finally:
            p.close()
            V.close()
    finally:
        circ.close()


# ---------------------------------------------------------------- 5. NULL trapdoor
def test_null_trapdoor_draws_a_fresh_key_each_time(ctx, tmp_path):
    circuit, w = sr.mixed(*sr.MIXED_SHAPES[1])
    keys = []
    for i in range(2):
        (tmp_path / str(i)).mkdir()
        m = Made(ctx, tmp_path / str(i), circuit, w, trapdoor=None)
        try:
            js, proof, ok = m.p.prove_mem_verified(m.witness, R_INJ, S_INJ)
            assert ok == 1
            keys.append(sr.sections(m.zkey))
        finally:
            m.close()
    assert keys[0][4] == keys[1][4] and keys[0][1] == keys[1][1]
    for k in (2, 3, 5, 6, 7, 8, 9):
        assert keys[0][k] != keys[1][k], k


# ---------------------------------------------------------------- 6. refusals
def test_every_refusal_and_a_correct_call_afterwards(ctx, tmp_path):
    import k16
    circuit, w = sr.mixed(*sr.MIXED_SHAPES[1])
    n_wires, rowsA, rowsB, rowsC, n_pub_out, n_pub_in = circuit
    raw = rb.write(n_wires, rowsA, rowsB, rowsC, n_pub_out=n_pub_out, n_pub_in=n_pub_in)
    circ = k16.R1cs(ctx, raw)
    g, omega = sr.roots(sr.domain(len(rowsA), n_pub_out + n_pub_in))
    good = list(sr.TRAPDOOR)

    def refused(call):
        with pytest.raises(k16.K16Error) as e:
            call()
        assert e.value.rc == ERR_ARG

    try:
        want = circ.setup(good)
        for i in range(5):                                        # a value of 0, r, r + 1, 2^256 - 1 in every position
            for bad in (0, R, R + 1, 2 ** 256 - 1):
                refused(lambda: circ.setup(good[:i] + [bad] + good[i + 1:]))
        for tau in (omega ** 3 % R, g, 1, omega, g ** 3 % R, R - 1):   # in the domain or in its odd coset: tau^(2N) = 1
            refused(lambda: circ.setup([tau] + good[1:]))
        other = k16.Context(0)
        try:
            refused(lambda: circ.setup(good, ctx=other))          # an R1CS object of another context
        finally:
            other.close()
        empty = k16.R1cs(ctx, rb.write(3, [], [], []))            # no constraint
        try:
            refused(lambda: empty.setup(good))
            refused(lambda: empty.setup_size())
        finally:
            empty.close()
        # a buffer too small: K16_ERR_BUFFER, and the needed size all the same
        need, n = circ.setup_size(), C.c_size_t()
        td = b"".join(int(x).to_bytes(32, "little") for x in good)
        for cap in (0, 1, need - 1):
            buf = np.zeros(max(cap, 1), dtype=np.uint8)
            assert ctx.L.k16_r1cs_setup(ctx.h, circ.h, td, buf.ctypes.data_as(C.c_void_p), cap, C.byref(n)) == ERR_BUFFER
            assert n.value == need and not buf.any()
        # the file variant leaves no partial file behind
        out = tmp_path / "never.zkey"
        refused(lambda: circ.setup_file(out, [g] + good[1:]))
        with pytest.raises(k16.K16Error):
            circ.setup_file(tmp_path / "no_such_directory" / "k.zkey", good)
        assert os.listdir(tmp_path) == []
        # the same objects still work
        assert circ.setup(good) == want
        circ.setup_file(out, good)
        assert out.read_bytes() == want and os.listdir(tmp_path) == ["never.zkey"]
    finally:
        circ.close()


def test_wire_count_beyond_32_bit_row_numbers_is_refused(ctx):
    """3 * nWires >= 2^32: a header with that many wires over a one-constraint circuit (the file itself is small)."""
    import k16
    n_wires = (1 << 32) // 3 + 1
    big = k16.R1cs(ctx, rb.write(n_wires, [[(1, 1)]], [[(2, 1)]], [[(3, 1)]], with_labels=False))
    try:
        for call in (big.setup_size, lambda: big.setup(list(sr.TRAPDOOR))):
            with pytest.raises(k16.K16Error) as e:
                call()
            assert e.value.rc == ERR_ARG
    finally:
        big.close()
