"""-m gpu : verified proving (include/k16.h: k16_vk_create_from_zkey, k16_prover_set_vk, k16_prover_prove_*_verified,
k16_verify_split_gt; k16_fullprover_set_verify behind the FullProver facade) against the CPU oracle and the library's own plain calls.
The check is split where the prover's data arrive (csrc/verify_script.h, early / late programs): its values must be the
single program's and the oracle's, byte for byte."""
import os
import struct
import subprocess

import numpy as np
import pytest

import groth16_io as gio
import oracle_lib as ol
import pymodel as pm
from test_oracle_prove import KNOWN_RS0

pytestmark = pytest.mark.gpu

R_INJ, S_INJ = pm.limbs(pm.SplitMix64(91).below(pm.R)), pm.limbs(pm.SplitMix64(92).below(pm.R))
ERR_ARG, ERR_FORMAT = -3, -5


@pytest.fixture(scope="module")
def ctx():
    import k16
    c = k16.Context(0)
    yield c
    c.close()


def without_section(zkey, drop):
    """A copy of an iden3 container with every section of type `drop` cut out."""
    nsec = struct.unpack_from("<I", zkey, 8)[0]
    pos, kept = 12, []
    for _ in range(nsec):
        typ, size = struct.unpack_from("<IQ", zkey, pos)
        if typ != drop:
            kept.append(zkey[pos:pos + 12 + size])
        pos += 12 + size
    return zkey[:8] + struct.pack("<I", len(kept)) + b"".join(kept)


def flipped(witness):
    """The witness with one bit of its last wire flipped: it violates a constraint, the proof is produced and is wrong."""
    bad = witness.copy()
    bad[-1, 0] ^= 1
    return bad


class Key:
    """A valid synthetic key on disk with a prover, the key made from the zkey attached, and the oracle's vk."""

    def __init__(self, ctx, tmp, shape, seed):
        import k16
        import valid_key_builder as vkb
        key = vkb.build(lambda g, s: ctx.synth_points_scalars(g, s), *shape, seed=seed)
        self.zk, self.wt, self.wt_bad = (str(tmp / n) for n in ("v.zkey", "v.wtns", "bad.wtns"))
        open(self.zk, "wb").write(key["zkey"])
        self.zk_no3 = str(tmp / "no3.zkey")
        open(self.zk_no3, "wb").write(without_section(key["zkey"], 3))
        self.witness, self.bad, self.public, self.vk, self.n_vars = key["witness"], flipped(key["witness"]), key["public"], key["vk"], key["n_vars"]
        vkb.write_wtns(self.wt, self.witness)
        vkb.write_wtns(self.wt_bad, self.bad)
        self.p = k16.Prover(ctx, self.zk)
        self.V = k16.VerifyingKey.from_zkey(ctx, self.zk)
        self.p.set_vk(self.V)

    def close(self):
        self.p.close()
        self.V.close()


@pytest.fixture(scope="module")
def key14(ctx, tmp_path_factory):
    k = Key(ctx, tmp_path_factory.mktemp("pv14"), (12000, 1000, 300), seed=7)
    yield k
    k.close()


@pytest.fixture(scope="module")
def key17(ctx, tmp_path_factory):
    """The smallest valid key on the packed-upload path: 2^16 + 2 wires, 2^16 + 1 constraint rows -> domain 2^17."""
    k = Key(ctx, tmp_path_factory.mktemp("pv17"), (65235, 1, 300), seed=11)
    assert k.n_vars == (1 << 16) + 2 and k.p.info()["domain_size"] == 1 << 17
    yield k
    k.close()


def _verified_against_plain_and_oracle(k, oracle_threads):
    """The assertions shared by the 2^14 key and the toy key: JSON byte-equal to prove_mem's and the oracle's, proof bytes
    equal to the JSON's, flag 1; one witness bit flipped: flag 0, JSON still prove_mem's; the oracle's verifier agrees."""
    js, proof, ok = k.p.prove_mem_verified(k.witness, R_INJ, S_INJ)
    assert js == k.p.prove_mem(k.witness, R_INJ, S_INJ)
    assert js == ol.prove_files(k.zk, k.wt, R_INJ, S_INJ, nthreads=oracle_threads)
    assert proof == gio.proof_from_json(js) and ok == 1
    assert ol.groth16_verify(k.vk, proof, k.public)
    js_b, proof_b, ok_b = k.p.prove_mem_verified(k.bad, R_INJ, S_INJ)
    assert js_b == k.p.prove_mem(k.bad, R_INJ, S_INJ) and js_b != js
    assert proof_b == gio.proof_from_json(js_b) and ok_b == 0
    assert not ol.groth16_verify(k.vk, proof_b, k.public)
    fresh = [k.p.prove_mem_verified(k.witness) for _ in range(3)]           # CSPRNG blinding
    assert len({f[1] for f in fresh}) == 3 and [f[2] for f in fresh] == [1, 1, 1]
    assert all(f[1] == gio.proof_from_json(f[0]) for f in fresh)
    assert k.V.verify_batch([f[1] for f in fresh], [k.public] * 3) == [True] * 3


def test_key_from_zkey_equals_key_from_vkey_file(ctx, toy_paths, tmp_path):
    import k16
    zkey, wtns, vkp = toy_paths
    Vz = k16.VerifyingKey.from_zkey(ctx, zkey)
    Vb = k16.VerifyingKey.from_zkey(ctx, open(zkey, "rb").read())
    Vj = k16.VerifyingKey(ctx, gio.vk_from_json(vkp))
    good = gio.proof_from_json(KNOWN_RS0)
    bad = good[:192] + good[:64]                                             # C replaced by A
    assert Vz.n_ic == Vj.n_ic == 2
    want = Vj.coop_gt([good, bad], [[2], [2]])
    for V in (Vz, Vb):
        assert np.array_equal(V.coop_gt([good, bad], [[2], [2]]), want)
        assert V.verify_batch([good, bad, good], [[2], [2], [3]]) == Vj.verify_batch([good, bad, good], [[2], [2], [3]]) == [True, False, False]
    cut = without_section(open(zkey, "rb").read(), 3)
    with pytest.raises(k16.K16Error) as e:
        k16.VerifyingKey.from_zkey(ctx, cut)
    assert e.value.rc == ERR_FORMAT
    path = str(tmp_path / "no3.zkey")
    open(path, "wb").write(cut)
    with pytest.raises(k16.K16Error) as e:
        k16.VerifyingKey.from_zkey(ctx, path)
    assert e.value.rc == ERR_FORMAT
    for V in (Vz, Vb, Vj):
        V.close()


class ScalarKey:
    """A (key, proof) family from known discrete logs, three public inputs (as test_verify_key_with_several_public_inputs,
    with gamma and delta of their own): A = aG, B = bH, C = cG verify iff ab = alpha beta + vkx gamma + c delta."""
    IC, AL, BE, GA, DE = [11, 22, 33, 44], 7, 9, 3, 5

    def __init__(self):
        g, h = ol.generator(0), ol.generator(1)
        self.g1 = lambda k: ol.pt_to_affine(0, ol.mul_scalar(0, g, pm.limbs(k % pm.R)))
        self.g2 = lambda k: ol.pt_to_affine(1, ol.mul_scalar(1, h, pm.limbs(k % pm.R)))
        self.vk = dict(alpha1=self.g1(self.AL), beta2=self.g2(self.BE), gamma2=self.g2(self.GA), delta2=self.g2(self.DE),
                       ic=[self.g1(k) for k in self.IC])

    def vkx(self, xs):
        return (self.IC[0] + sum(x * k for x, k in zip(xs, self.IC[1:]))) % pm.R

    def proof(self, a, b, xs, dc=0):
        c = (a * b - self.AL * self.BE - self.vkx(xs) * self.GA) * pow(self.DE, -1, pm.R) % pm.R
        return self.g1(a) + self.g2(b) + self.g1(c + dc)

    def oracle_values(self, proof, xs):
        """(e(A,B) e(vk_x,-gamma), that times e(C,-delta)) from the oracle's pairings"""
        two = ol.gt_mul(ol.pairing(proof[:64], proof[64:192]), ol.pairing(self.g1(self.vkx(xs)), self.g2(pm.R - self.GA)))
        return two, ol.gt_mul(two, ol.pairing(proof[192:], self.g2(pm.R - self.DE)))


@pytest.fixture(scope="module")
def scalar_key(ctx):
    import k16
    sk = ScalarKey()
    V = k16.VerifyingKey(ctx, sk.vk)
    yield sk, V
    V.close()


@pytest.mark.parametrize("n", [1, 5])
def test_split_values_equal_single_program_and_oracle(scalar_key, n):
    sk, V = scalar_key
    xs = [5, pm.R - 3, 123456789]
    cases = [(sk.proof(1001, 2002, xs), xs), (sk.proof(1001, 2002, xs), [xs[0], xs[1], xs[2] + 1]),     # accepted; wrong input
             (sk.proof(77, 88, xs, dc=1), xs), (sk.proof(31337, 4242, [1, 2, 3]), [1, 2, 3]),             # C + G; accepted
             (sk.proof(pm.R - 1, 2, xs), xs)][:n]
    proofs, ins = [c[0] for c in cases], [c[1] for c in cases]
    early, gt = V.split_gt(proofs, ins)
    assert np.array_equal(gt, V.coop_gt(proofs, ins))
    for i, (pr, x) in enumerate(cases):
        two, three = sk.oracle_values(pr, x)
        assert gt[i].tobytes() == three, i
        assert ol.final_exp(early[i].tobytes()) == two, i
    want = [True, False, False, True, True][:n]
    assert V.verify_batch(proofs, ins) == want == [ol.groth16_verify(sk.vk, p, x) for p, x in cases]
    target = ol.pairing(sk.vk["alpha1"], sk.vk["beta2"])
    assert [gt[i].tobytes() == target for i in range(n)] == want


def test_undecidable_inputs_are_left_to_verify_batch(scalar_key):
    """A = 0 and vk_x = infinity: the split programs record the generic case only.  k16_verify_split_gt (no fallback) refuses
    them; the path its callers take for such a proof, k16_verify_batch, gives the oracle's flag."""
    import k16
    sk, V = scalar_key
    xs = [5, 6, 7]
    x_inf = [(-sk.IC[0] * pow(sk.IC[1], -1, pm.R)) % pm.R, 0, 0]
    assert sk.vkx(x_inf) == 0
    good = sk.proof(12, 34, xs)
    a_zero = bytes(64) + good[64:]
    at_inf = sk.proof(12, 34, x_inf)          # verifies: e(vk_x, -gamma) = 1
    for pr, x in ((a_zero, xs), (at_inf, x_inf)):
        with pytest.raises(k16.K16Error) as e:
            V.split_gt([good, pr], [xs, x])
        assert e.value.rc == ERR_ARG
    got = V.verify_batch([a_zero, at_inf, good], [xs, x_inf, xs])
    assert got == [ol.groth16_verify(sk.vk, a_zero, xs), ol.groth16_verify(sk.vk, at_inf, x_inf), True] == [False, True, True]
    off_curve = good[:192] + good[:32] + good[192:224]                       # C = (A.x, C.x)
    with pytest.raises(k16.K16Error) as e:
        V.split_gt([off_curve], [xs])
    assert e.value.rc == ERR_ARG
    early, gt = V.split_gt([good], [xs])                                     # the key's buffers are fine after the refusals
    assert gt[0].tobytes() == sk.oracle_values(good, xs)[1]


def test_verified_prove_2p14(key14):
    _verified_against_plain_and_oracle(key14, min(16, os.cpu_count() or 8))


def test_verified_prove_toy_key_plain_upload(ctx, toy_paths):
    import k16
    zkey, wtns, vkp = toy_paths

    class Toy:
        pass
    k = Toy()
    k.zk, k.wt, k.vk, k.public = zkey, wtns, gio.vk_from_json(vkp), [2]
    raw = open(wtns, "rb").read()
    k.witness = np.frombuffer(raw[-3 * 32:], dtype=np.uint8).reshape(3, 32).copy()
    k.bad = flipped(k.witness)
    k.p = k16.Prover(ctx, zkey)
    k.V = k16.VerifyingKey.from_zkey(ctx, zkey)
    k.p.set_vk(k.V)
    try:
        assert k.p.info()["n_vars"] == 3
        # the oracle proves from files: the flipped witness is compared with prove_mem only (inside), the good one with both
        _verified_against_plain_and_oracle(k, 1)
        with pytest.raises(k16.K16Error) as e:
            k.p.prove_compact_verified(0, R_INJ, S_INJ)
        assert e.value.rc == ERR_ARG
        with pytest.raises(k16.K16Error) as e:
            k.p.prove_compact(0, R_INJ, S_INJ)
        assert e.value.rc == ERR_ARG
    finally:
        k.p.close()
        k.V.close()


def test_verified_prove_packed_upload_compact_equals_mem(key17):
    k = key17
    narrow, idx, val = k.p.compact_buffers()
    for w in (k.witness, k.bad):
        js, proof, ok = k.p.prove_mem_verified(w, R_INJ, S_INJ)
        wide = np.flatnonzero(w[:, 1:].any(axis=1))
        assert 1 in wide and 0 < len(wide) <= len(idx)                       # the public input is a wide value: read from the list
        narrow[:] = w[:, 0]
        narrow[wide] = 0
        idx[:len(wide)] = wide
        val[:len(wide)] = w[wide]
        assert k.p.prove_compact_verified(len(wide), R_INJ, S_INJ) == (js, proof, ok)
        assert js == k.p.prove_mem(w, R_INJ, S_INJ) and proof == gio.proof_from_json(js)
        assert ok == (1 if w is k.witness else 0) == int(ol.groth16_verify(k.vk, proof, k.public))


def test_argument_errors(ctx, key14, scalar_key):
    import k16
    p2 = k16.Prover(ctx, key14.zk)
    other = k16.Context(0)
    try:
        with pytest.raises(k16.K16Error) as e:
            p2.prove_mem_verified(key14.witness, R_INJ, S_INJ)               # no key attached
        assert e.value.rc == ERR_ARG
        V_other = k16.VerifyingKey.from_zkey(other, key14.zk)
        with pytest.raises(k16.K16Error) as e:
            p2.set_vk(V_other)                                               # a key of another context
        assert e.value.rc == ERR_ARG
        V_other.close()
        with pytest.raises(k16.K16Error) as e:
            p2.set_vk(scalar_key[1])                                         # n_ic = 4, the circuit has one public input
        assert e.value.rc == ERR_ARG
        p2.set_vk(key14.V)
        assert p2.prove_mem_verified(key14.witness, R_INJ, S_INJ)[2] == 1
        p2.set_vk(None)                                                      # detached again
        with pytest.raises(k16.K16Error) as e:
            p2.prove_mem_verified(key14.witness, R_INJ, S_INJ)
        assert e.value.rc == ERR_ARG
        assert p2.prove_mem(key14.witness, R_INJ, S_INJ) == key14.p.prove_mem(key14.witness, R_INJ, S_INJ)
    finally:
        p2.close()
        other.close()


def test_key_without_the_programs_falls_back_to_verify_batch(key14, monkeypatch):
    """A context made under K16_VERIFY_NO_COOP=1 has keys without the wave-cooperative programs: the verified calls then
    settle every proof through k16_verify_batch's general path after the prove -- the path an undecidable proof (zero point,
    vk_x at infinity) takes.  Same JSON, same proof bytes, same flags."""
    import k16
    monkeypatch.setenv("K16_VERIFY_NO_COOP", "1")
    c = k16.Context(0)
    monkeypatch.delenv("K16_VERIFY_NO_COOP")
    p = V = None
    try:
        p = k16.Prover(c, key14.zk)
        V = k16.VerifyingKey.from_zkey(c, key14.zk)
        with pytest.raises(k16.K16Error) as e:
            V.split_gt([bytes(256)], [key14.public])                         # no split programs on this key
        assert e.value.rc == ERR_ARG
        p.set_vk(V)
        for w, want in ((key14.witness, 1), (key14.bad, 0)):
            assert p.prove_mem_verified(w, R_INJ, S_INJ) == key14.p.prove_mem_verified(w, R_INJ, S_INJ)
            assert p.prove_mem_verified(w, R_INJ, S_INJ)[2] == want
    finally:
        for o in (p, V, c):
            if o is not None:
                o.close()


def test_facade_with_verification_switched_on(key14, tmp_path):
    """k16_fullprover_set_verify behind the drop-in FullProver (tests/cpp/fullprover_verify_harness.cpp, a child process):
    a good witness gives a proof as before, through prove(path) and through k16_fullprover_prove_mem; the flipped witness
    is answered with INVALID_INPUT (type=1 error=2) / K16_ERR_FORMAT; a zkey without section 3 makes the call itself
    report K16_ERR_FORMAT and leaves the provers working unverified.  The unmodified harness -- no call -- behaves as ever."""
    import json
    from test_boundary import build_harness, ROOT, PKG
    exe = str(tmp_path / "fullprover_verify_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "fullprover_verify_harness.cpp"),
                           "-L", PKG, "-lk16", "-Wl,-rpath," + PKG, "-pthread", "-o", exe])

    def run(exe, zk, wt):
        out = subprocess.run([exe, zk, wt], capture_output=True, text=True, timeout=300)
        return out.stdout.splitlines(), out.stderr

    lines, err = run(exe, key14.zk, key14.wt)
    assert lines[:3] == ["state=0", "verify=0", "file type=0 error=0"] and lines[4] == "mem rc=0", (lines, err[-2000:])
    for js in (lines[3], lines[5]):                                          # CSPRNG blinding: the proofs verify
        assert set(json.loads(js)) == {"pi_a", "pi_b", "pi_c", "protocol"}
        assert key14.V.verify_batch([gio.proof_from_json(js)], [key14.public]) == [True]
    lines, err = run(exe, key14.zk, key14.wt_bad)
    assert lines[:3] == ["state=0", "verify=0", "file type=1 error=2"] and lines[4] == "mem rc=%d" % ERR_FORMAT, (lines, err[-2000:])
    lines, err = run(exe, key14.zk_no3, key14.wt_bad)                        # no section 3: refused, proofs go out unverified
    assert lines[:3] == ["state=0", "verify=%d" % ERR_FORMAT, "file type=0 error=0"] and lines[4] == "mem rc=0", (lines, err[-2000:])
    assert "verification key" in err
    plain = build_harness(tmp_path)                                          # without the call nothing changes
    lines, err = run(plain, key14.zk, key14.wt_bad)
    assert lines[0] == "state=0" and lines[1].startswith("type=0 error=0"), err[-2000:]
