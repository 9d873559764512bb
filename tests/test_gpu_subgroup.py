"""-m gpu : the point checks on the GPU (csrc/points_check.hip): k16_points_check, k16_verify_batch_checked and
k16_zkey_check against the definitional classes of tests/subgroup_fixtures.py ([r] Q = O over pymodel)."""
import os
import struct
import sys
import time

import numpy as np
import pytest

import groth16_io as gio
import pymodel as pm
import subgroup_fixtures as sf
import valid_key_builder as vkb
from test_oracle_prove import KNOWN_RS0

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import k16
    c = k16.Context(0)
    yield c
    c.close()


def _with_failures(good, bad, bad_status, n, per_wave):
    """n points cycling through `good`, with failing points at the first and last point of the first two wavefronts, the
    last point, and (when there is room) every failing fixture point at a stride."""
    pts = good[np.arange(n) % len(good)].copy()
    want = np.zeros(n, dtype=np.uint8)
    pos = [p for p in (0, per_wave - 1, per_wave, 2 * per_wave - 1, n - 1) if 0 <= p < n]
    if n - 2 * per_wave - 2 >= len(bad):
        pos += list(range(2 * per_wave + 1, n - 1, (n - 2 * per_wave - 2) // len(bad)))[:len(bad)]
    for j, p in enumerate(sorted(set(pos))):
        pts[p] = bad[j % len(bad)]
        want[p] = bad_status[j % len(bad)]
    return pts, want


@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
def test_points_check_small_sets(ctx, group):
    import k16
    if group == k16.G2:
        pts, want, small = sf.g2_fixtures()
        per_wave = 32                    # a lane pair per point
    else:
        pts, want = sf.g1_fixtures()
        per_wave = 64
    got = ctx.points_check(group, pts)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:10], got[bad[:10]], want[bad[:10]])
    good, fail, fail_st = pts[want == 0], pts[want != 0], want[want != 0]
    for n in (0, 1, 63, 64, 65, 4097):
        p, w = _with_failures(good, fail, fail_st, n, per_wave)
        got = ctx.points_check(group, p)
        assert got.shape == (n,) and (got == w).all(), n


def test_points_check_at_scale(ctx):
    """2^20 G2 points of k16_synth_points all pass; 1,000 seeded positions overwritten by non-G2 points get status 3."""
    import k16
    n = 1 << 20
    d = ctx.synth_points(k16.G2, 0, n)
    pts = d.download(np.uint8, (n, 128)).copy()
    d.free()
    t0 = time.time()
    st = ctx.points_check(k16.G2, pts)
    t1 = time.time()
    assert (st == 0).all(), np.nonzero(st)[0][:10]
    pos = np.random.RandomState(3).choice(n, 1000, replace=False)
    pts[pos] = sf.non_g2_points(1000)
    st = ctx.points_check(k16.G2, pts)
    assert set(np.nonzero(st)[0].tolist()) == set(pos.tolist())
    assert (st[pos] == k16.PT_NOT_IN_SUBGROUP).all()
    print("k16_points_check G2 n=2^20: %.1f ms from host memory" % ((t1 - t0) * 1e3))


# ---------------------------------------------------------------- checked verification
def _b_of(proof):
    return pm.g2_aff_from_bytes(proof[64:192])


def _with_b(proof, q):
    return proof[:64] + pm.g2_aff_bytes(q) + proof[192:]


def _raise(proof, off, coord_value):
    b = bytearray(proof)
    b[off:off + 32] = pm.limbs(coord_value)
    return bytes(b)


def _variants(known):
    """(proof, input, b_in_g2, reason) of the kinds a foreign batch may hold."""
    T = sf.small_order_point()
    Rq = sf.outside_g2_point()
    B = _b_of(known)
    A = pm.g1_aff_from_bytes(known[0:64])
    C = pm.g1_aff_from_bytes(known[192:256])
    return [
        (known, 2, True, 0),
        (known, 3, True, 4),                                                      # wrong public input
        (_with_b(known, pm.ec_add(sf.F2, B, T)), 2, False, 3),                    # B + T
        (_with_b(known, Rq), 2, False, 3),                                        # a random twist point
        (_raise(known, 0, pm.unlimbs(known[0:32]) + pm.Q), 2, True, 1),           # A.x + p
        (known[:192] + pm.g1_aff_bytes((C[0], (C[1] + 1) % pm.Q)), 2, True, 2),   # C off the curve
        (pm.g1_aff_bytes((A[0], (A[1] + 1) % pm.Q)) + known[64:], 2, True, 2),    # A off the curve
        (_raise(known, 64 + 96, pm.unlimbs(known[160:192]) + pm.Q), 2, True, 1),  # B.y.b + p
    ]


def _check_toy(V, known):
    assert V.verify_batch_checked([known], [[2]]) == ([True], [0])
    for proof, x, _, reason in _variants(known):
        assert V.verify_batch_checked([proof], [[x]]) == ([reason == 0], [reason]), reason


def test_checked_verification_toy_key_both_paths(ctx, toy_paths, monkeypatch):
    import k16
    vk = gio.vk_from_json(toy_paths[2])
    known = gio.proof_from_json(KNOWN_RS0)
    V = k16.VerifyingKey(ctx, vk)
    _check_toy(V, known)                               # the wave-cooperative path
    V.close()
    monkeypatch.setenv("K16_VERIFY_NO_COOP", "1")      # a context that takes the general path
    c2 = k16.Context(0)
    V2 = k16.VerifyingKey(c2, vk)
    _check_toy(V2, known)
    V2.close()
    c2.close()


@pytest.mark.parametrize("n", [64, 3000])
def test_checked_verification_mixed_batches(ctx, toy_paths, n):
    """ok_checked == ok_unchecked & (B in G2) for every proof of a mixed batch; reasons as the variant says."""
    import k16
    V = k16.VerifyingKey(ctx, gio.vk_from_json(toy_paths[2]))
    var = _variants(gio.proof_from_json(KNOWN_RS0))
    pick = np.random.RandomState(n).randint(0, len(var), size=n)
    proofs = [var[k][0] for k in pick]
    inputs = [[var[k][1]] for k in pick]
    ok_u = V.verify_batch(proofs, inputs)
    ok_c, why = V.verify_batch_checked(proofs, inputs)
    assert ok_c == [u and var[k][2] for u, k in zip(ok_u, pick)]
    assert why == [var[k][3] for k in pick]
    V.close()


def test_forged_proof_with_a_non_g2_b(ctx):
    """A key with known discrete logs; A = infinity, C = c G1 with c = -(alpha beta + gamma v) / delta: the pairing check
    holds whatever B is.  k16_verify_batch accepts B outside G2, k16_verify_batch_checked rejects it (reason 3); with
    B = infinity both accept."""
    import k16
    r = pm.R
    a, b, g, d, i0, i1, x = 5, 7, 11, 13, 17, 19, 2
    g1 = lambda k: pm.g1_aff_bytes(pm.ec_mul(pm.Fq1Ops, pm.G1, k % r))
    g2 = lambda k: pm.g2_aff_bytes(pm.ec_mul(sf.F2, pm.G2, k % r))
    V = k16.VerifyingKey(ctx, dict(alpha1=g1(a), beta2=g2(b), gamma2=g2(g), delta2=g2(d), ic=[g1(i0), g1(i1)]))
    v = (i0 + i1 * x) % r
    c = -(a * b + g * v) * pow(d, -1, r) % r
    forged = b"\0" * 64 + pm.g2_aff_bytes(sf.outside_g2_point()) + g1(c)
    assert V.verify_batch([forged], [[x]]) == [True]
    assert V.verify_batch_checked([forged], [[x]]) == ([False], [3])
    inf_b = b"\0" * 64 + b"\0" * 128 + g1(c)
    assert V.verify_batch([inf_b], [[x]]) == [True]
    assert V.verify_batch_checked([inf_b], [[x]]) == ([True], [0])
    V.close()


# ---------------------------------------------------------------- zkey check
def _sections(zk):
    """{section type: payload offset} of an iden3 container (first occurrence)."""
    nsec = struct.unpack_from("<I", zk, 8)[0]
    pos, out = 12, {}
    for _ in range(nsec):
        t, sz = struct.unpack_from("<IQ", zk, pos)
        pos += 12
        out.setdefault(t, pos)
        pos += sz
    return out


HDR_PTS = 4 + 32 + 4 + 32 + 12            # section 2: alpha1 at this offset, then beta1, beta2, gamma2, delta1, delta2


def _corrupt(zk, sec, off, new):
    b = bytearray(zk)
    o = _sections(zk)[sec] + off
    b[o:o + len(new)] = new
    return bytes(b)


@pytest.fixture(scope="module")
def small_key(ctx):
    return vkb.build(lambda group, scalars: ctx.synth_points_scalars(group, scalars), 40, 6, 9, seed=3)


def test_zkey_check_valid_and_corrupted(ctx, toy_paths, small_key):
    import k16
    assert k16.zkey_check(ctx, toy_paths[0])["ok"]
    assert k16.zkey_check(ctx, open(toy_paths[0], "rb").read())["ok"]
    zk = small_key["zkey"]
    assert k16.zkey_check(ctx, zk) == dict(ok=True, n_bad=0, section=0, index=0, status=0)
    nv = small_key["n_vars"]
    a_pts = [pm.g1_aff_from_bytes(zk[_sections(zk)[5] + 64 * i:][:64]) for i in range(nv)]
    ja = next(i for i in range(3, nv) if a_pts[i] is not None)
    A = a_pts[ja]
    jb, jc = nv - 2, 1
    c_off = _sections(zk)[8] + 64 * jc
    bad_b2 = _corrupt(zk, 7, 128 * jb, pm.g2_aff_bytes(sf.outside_g2_point()))
    bad_a = _corrupt(zk, 5, 64 * ja, pm.g1_aff_bytes((A[0], (A[1] + 1) % pm.Q)))
    bad_c = _corrupt(zk, 8, 64 * jc, pm.limbs(pm.unlimbs(zk[c_off:c_off + 32]) + pm.Q))
    bad_beta2 = _corrupt(zk, 2, HDR_PTS + 128, pm.g2_aff_bytes(pm.ec_add(sf.F2, pm.ec_mul(sf.F2, pm.G2, 5), sf.small_order_point())))
    assert k16.zkey_check(ctx, bad_b2) == dict(ok=False, n_bad=1, section=7, index=jb, status=3)
    assert k16.zkey_check(ctx, bad_a) == dict(ok=False, n_bad=1, section=5, index=ja, status=2)
    assert k16.zkey_check(ctx, bad_c) == dict(ok=False, n_bad=1, section=8, index=jc, status=1)
    assert k16.zkey_check(ctx, bad_beta2) == dict(ok=False, n_bad=1, section=2, index=2, status=3)
    # several at once: the first in (section, index) order, all of them counted
    both = _corrupt(bad_b2, 8, 64 * jc, pm.limbs(pm.unlimbs(zk[c_off:c_off + 32]) + pm.Q))
    assert k16.zkey_check(ctx, both) == dict(ok=False, n_bad=2, section=7, index=jb, status=3)


def _container(zk, patch):
    """The iden3 container of zk rebuilt from its sections, each payload through patch(type, payload) (None drops it)."""
    nsec = struct.unpack_from("<I", zk, 8)[0]
    pos, secs = 12, []
    for _ in range(nsec):
        t, sz = struct.unpack_from("<IQ", zk, pos)
        pos += 12
        p = patch(t, zk[pos:pos + sz])
        pos += sz
        if p is not None:
            secs.append(struct.pack("<IQ", t, len(p)) + p)
    return zk[:8] + struct.pack("<I", len(secs)) + b"".join(secs)


def test_zkey_check_rejects_a_wrapping_public_count(ctx, toy_paths, tmp_path):
    """nPublic = 2^32 - 1, no IC section, section 8 as long as nVars points: in 32-bit arithmetic nPublic + 1 and
    nVars - nPublic - 1 wrap and every size check passes.  The header check is 64-bit: K16_ERR_FORMAT from the key check
    (memory and file) and from the prover, before any point is read."""
    import ctypes as C
    import k16
    zk = open(toy_paths[0], "rb").read()
    n_vars = struct.unpack_from("<I", zk, _sections(zk)[2] + HDR_PTS - 12)[0]

    def patch(t, p):
        if t == 2:
            return p[:HDR_PTS - 8] + struct.pack("<I", 0xFFFFFFFF) + p[HDR_PTS - 4:]
        if t == 3:
            return None
        if t == 8:
            return p + b"\0" * (64 * n_vars - len(p))
        return p
    bad = _container(zk, patch)
    assert struct.unpack_from("<I", bad, _sections(bad)[2] + HDR_PTS - 8)[0] == 0xFFFFFFFF and 3 not in _sections(bad)
    with pytest.raises(k16.K16Error) as e:
        k16.zkey_check(ctx, bad)
    assert e.value.rc == -5
    p = tmp_path / "wrap.zkey"
    p.write_bytes(bad)
    with pytest.raises(k16.K16Error) as e:
        k16.zkey_check(ctx, str(p))
    assert e.value.rc == -5
    buf = np.frombuffer(bad, dtype=np.uint8)
    h = C.c_void_p()
    assert ctx.L.k16_prover_create_mem(ctx.h, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(h)) == -5
    # the same container with the true nPublic is a valid key
    ok = _container(zk, lambda t, q: q)
    assert k16.zkey_check(ctx, ok)["ok"]


def test_zkey_check_errors(ctx, toy_paths, tmp_path):
    import ctypes as C
    import k16
    zk = open(toy_paths[0], "rb").read()
    with pytest.raises(k16.K16Error) as e:
        k16.zkey_check(ctx, zk[:len(zk) // 2])
    assert e.value.rc == -5
    p = tmp_path / "trunc.zkey"
    p.write_bytes(zk[:len(zk) - 100])
    with pytest.raises(k16.K16Error) as e:
        k16.zkey_check(ctx, str(p))
    assert e.value.rc == -5
    sec, idx, st, nb = C.c_uint32(), C.c_uint64(), C.c_uint8(), C.c_uint64()
    buf = np.frombuffer(zk, dtype=np.uint8)
    L = ctx.L
    assert L.k16_zkey_check(ctx.h, None, len(zk), C.byref(sec), C.byref(idx), C.byref(st), C.byref(nb)) == -3
    assert L.k16_zkey_check(ctx.h, buf.ctypes.data_as(C.c_void_p), len(zk), None, C.byref(idx), C.byref(st), C.byref(nb)) == -3
    assert L.k16_zkey_check(None, buf.ctypes.data_as(C.c_void_p), len(zk), C.byref(sec), C.byref(idx), C.byref(st), C.byref(nb)) == -3
    assert L.k16_zkey_check_file(ctx.h, None, C.byref(sec), C.byref(idx), C.byref(st), C.byref(nb)) == -3
    assert L.k16_points_check(ctx.h, 2, buf.ctypes.data_as(C.c_void_p), 1, None) == -3
    assert L.k16_verify_batch_checked(None, None, None, None, 1, None, None) == -3


def test_zkey_check_keyless_shape(ctx):
    """A full Keyless-shape synthetic key (bench.synth_zkey_bytes at nVars 1,343,588, domain 2^21, as bench.py's proof leg
    builds it; no IC section, half of B1 / B2 at infinity) passes.  The time is printed, not asserted."""
    import k16
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    zk = bench.synth_zkey_bytes(ctx, k16, 1343588, 1, 1 << 21, 1000)
    t0 = time.time()
    r = k16.zkey_check(ctx, zk)
    dt = time.time() - t0
    assert r == dict(ok=True, n_bad=0, section=0, index=0, status=0)
    print("k16_zkey_check Keyless shape (%.0f MB): %.1f ms" % (len(zk) / 2**20, dt * 1e3))
