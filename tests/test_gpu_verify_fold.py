"""-m gpu : folded batch verification (k16_verify_batch_folded, k16_verify_fold_gt): the fold's GT value byte-equal to the
product of the oracle's pairings (tests/fold_reference.py), flags and reasons equal to k16_verify_batch_checked's."""
import numpy as np
import pytest

import fold_reference as fr
import groth16_io as gio
import pymodel as pm
import subgroup_fixtures as sf
from test_oracle_prove import KNOWN_RS0

pytestmark = pytest.mark.gpu

W_MAX = (1 << 128) - 1


@pytest.fixture(scope="module")
def ctx():
    import k16
    c = k16.Context(0)
    yield c
    c.close()


def _gpu_points(ctx):
    return lambda group, scalars: ctx.synth_points_scalars(group, scalars)


def _weights(seed, n):
    rng = pm.SplitMix64(seed)
    return [(rng.next() | (rng.next() << 64)) or 1 for _ in range(n)]


def _inputs(seed, n, n_in):
    """rows of public inputs: random below r, with 0, r - 1 and values >= r (they act modulo r) among them"""
    rng = pm.SplitMix64(seed)
    edge = [0, pm.R - 1, pm.R + 5, (1 << 256) - 1, pm.R]
    return [[edge[(i + j) % len(edge)] if (i + j) % 3 == 0 else rng.below(pm.R) for j in range(n_in)] for i in range(n)]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 300])
@pytest.mark.parametrize("n_ic", [2, 4])
def test_fold_value_equals_the_product_of_the_oracles_pairings(ctx, n_ic, n):
    import k16
    vk, t = fr.build_key(n_ic, seed=100 + n_ic)
    V = k16.VerifyingKey(ctx, vk)
    inputs = _inputs(n, n, n_ic - 1)
    w = _weights(1000 + n, n)
    for pos, val in zip(range(n), [1, W_MAX, 0]):     # the special weights, as far as the batch has room
        w[pos] = val
    if n == 1:
        w = [_weights(77, 1)[0]]
    good = fr.make_proofs(t, inputs, seed=n)
    got = V.fold_gt(good, inputs, w)
    assert got == fr.GT_ONE
    assert got == fr.fold_value(vk, good, inputs, w)
    # wrong proofs among them (not under the zero weight): V != 1, and still the oracle's bytes
    shift = {0: 1} if n < 63 else {0: 1, n // 2: 12345, n - 1: -7}
    bad = fr.make_proofs(t, inputs, seed=n, c_shift=shift)
    got = V.fold_gt(bad, inputs, w)
    assert got != fr.GT_ONE
    assert got == fr.fold_value(vk, bad, inputs, w)
    wrong_in = [list(r) for r in inputs]
    wrong_in[0][0] = (wrong_in[0][0] + 1) % (1 << 256)
    got = V.fold_gt(good, wrong_in, w)
    assert got != fr.GT_ONE and got == fr.fold_value(vk, good, wrong_in, w)
    if n == 1:   # the single weight 0: every sum is the point at infinity and V = 1, also for a wrong proof
        assert V.fold_gt(bad, inputs, [0]) == fr.GT_ONE == fr.fold_value(vk, bad, inputs, [0])
        assert V.fold_gt(good, inputs, [1]) == fr.GT_ONE
        assert V.fold_gt(good, inputs, [W_MAX]) == fr.GT_ONE
    V.close()


def test_cancelling_errors_fool_an_unweighted_fold_only(ctx):
    """C_1 + 5G and C_4 - 5G: under equal weights the fold's value is 1 (the test has teeth), under distinct weights it is
    not, and verify_batch_folded -- whose weights are random -- rejects exactly those two, in each of ten calls."""
    import k16
    n = k16.VERIFY_FOLD_MIN + 5
    vk, t = fr.build_key(2, seed=31, points=_gpu_points(ctx))
    V = k16.VerifyingKey(ctx, vk)
    inputs = _inputs(9, n, 1)
    proofs = fr.make_proofs(t, inputs, seed=4, points=_gpu_points(ctx), c_shift={1: 5, 4: -5})
    small = proofs[:6]
    assert V.fold_gt(small, inputs[:6], [1] * 6) == fr.GT_ONE
    assert V.fold_gt(proofs, inputs, [1] * n) == fr.GT_ONE
    w = _weights(5, 6)
    assert V.fold_gt(small, inputs[:6], w) == fr.fold_value(vk, small, inputs[:6], w) != fr.GT_ONE
    want = [i not in (1, 4) for i in range(n)]
    for _ in range(10):
        ok, why, folded = V.verify_batch_folded(proofs, inputs)
        assert ok == want and not folded
        assert why == [0 if g else 4 for g in want]
    V.close()


def _swap_a_c(p):
    return p[192:256] + p[64:192] + p[0:64]


def test_mixed_batch_flags_and_reasons_equal_checked_verification(ctx):
    import k16
    n_good = k16.VERIFY_FOLD_MIN + 40
    vk, t = fr.build_key(2, seed=41, points=_gpu_points(ctx))
    V = k16.VerifyingKey(ctx, vk)
    inputs = _inputs(3, n_good, 1)
    proofs = fr.make_proofs(t, inputs, seed=6, points=_gpu_points(ctx))
    g = proofs[7]
    A = pm.g1_aff_from_bytes(g[0:64])
    bad = [  # (proof, input row, expected reason or None: whatever the checked call says)
        (fr.make_proofs(t, inputs[:1], seed=6, points=_gpu_points(ctx), c_shift={0: 3})[0], inputs[0], 4),      # wrong C
        (proofs[1], [(inputs[1][0] + 1) % pm.R], 4),                                                             # wrong public input
        (_swap_a_c(proofs[2]), inputs[2], 4),                                                                    # A and C swapped
        (g[:64] + bytes(sf.plus_p(g[64:192], 1)) + g[192:], inputs[7], 1),                                       # B.x.b + p
        (pm.g1_aff_bytes((A[0], (A[1] + 1) % pm.Q)) + g[64:], inputs[7], 2),                                     # A off the curve
        (g[:64] + pm.g2_aff_bytes(sf.outside_g2_point()) + g[192:], inputs[7], 3),                               # B on the twist, outside G2
        (g[:64] + pm.g2_aff_bytes(sf.small_order_point()) + g[192:], inputs[7], 3),                              # B of order 10069
        (bytes(64) + g[64:], inputs[7], None),                                                                   # A = infinity
        (g[:64] + bytes(128) + g[192:], inputs[7], None),                                                        # B = infinity
        (g[:192] + bytes(64), inputs[7], None),                                                                  # C = infinity
    ]
    mixed_p, mixed_x, is_bad = list(proofs), [list(r) for r in inputs], [None] * n_good
    stride = n_good // (len(bad) + 1)
    for k, (p, x, why) in reversed(list(enumerate(bad))):      # inserted back to front: earlier positions stay put
        pos = (k + 1) * stride if k else 0     # the first one leads the batch
        mixed_p.insert(pos, p)
        mixed_x.insert(pos, list(x))
        is_bad.insert(pos, k)
    ok_c, why_c = V.verify_batch_checked(mixed_p, mixed_x)
    ok_f, why_f, folded = V.verify_batch_folded(mixed_p, mixed_x)
    assert (ok_f, why_f) == (ok_c, why_c) and not folded
    for i, k in enumerate(is_bad):
        if k is None:
            assert ok_f[i] and why_f[i] == 0
        else:
            assert not ok_f[i]
            assert bad[k][2] is None or why_f[i] == bad[k][2], (k, why_f[i])
    # only proofs with a bad POINT among valid ones: the fold leaves them out, accepts the rest, and says so
    keep = [i for i, k in enumerate(is_bad) if k is None or bad[k][2] in (1, 2, 3)]
    ok_f, why_f, folded = V.verify_batch_folded([mixed_p[i] for i in keep], [mixed_x[i] for i in keep])
    assert folded
    assert (ok_f, why_f) == V.verify_batch_checked([mixed_p[i] for i in keep], [mixed_x[i] for i in keep])
    assert why_f == [0 if is_bad[i] is None else bad[is_bad[i]][2] for i in keep]
    # the bad entries removed
    ok_f, why_f, folded = V.verify_batch_folded(proofs, inputs)
    assert ok_f == [True] * n_good and why_f == [0] * n_good and folded
    # a zero point among valid proofs: settled by the per-proof path, the others by the fold
    zp, zx = list(proofs), [list(r) for r in inputs]
    zp[5] = bytes(64) + g[64:]
    ok_f, why_f, folded = V.verify_batch_folded(zp, zx)
    assert (ok_f, why_f) == V.verify_batch_checked(zp, zx) and not ok_f[5] and sum(ok_f) == n_good - 1
    V.close()


def test_large_all_valid_batch_and_the_toy_key(ctx, toy_paths):
    import k16
    n = max(16384, 2 * k16.VERIFY_FOLD_MIN)
    vk, t = fr.build_key(2, seed=51, points=_gpu_points(ctx))
    V = k16.VerifyingKey(ctx, vk)
    inputs = _inputs(8, n, 1)
    proofs = fr.make_proofs(t, inputs, seed=9, points=_gpu_points(ctx))
    ok, why, folded = V.verify_batch_folded(proofs, inputs)
    assert folded and all(ok) and not any(why) and len(ok) == n
    V.close()
    # the toy key's known proof, repeated
    T = k16.VerifyingKey(ctx, gio.vk_from_json(toy_paths[2]))
    known = gio.proof_from_json(KNOWN_RS0)
    m = k16.VERIFY_FOLD_MIN + 1
    ok, why, folded = T.verify_batch_folded([known] * m, [[2]] * m)
    assert folded and all(ok) and not any(why)
    xs = [[2]] * m
    xs[m // 3] = [3]
    ok, why, folded = T.verify_batch_folded([known] * m, xs)
    assert not folded and ok == [i != m // 3 for i in range(m)] and why == [0 if i != m // 3 else 4 for i in range(m)]
    T.close()


def test_small_batches_forward_to_checked_verification(ctx, toy_paths):
    import k16
    T = k16.VerifyingKey(ctx, gio.vk_from_json(toy_paths[2]))
    known = gio.proof_from_json(KNOWN_RS0)
    assert T.verify_batch_folded([], []) == ([], [], False)
    for n in (1, 64, k16.VERIFY_FOLD_MIN - 1):
        xs = [[2 + (i % 5 == 3)] for i in range(n)]
        ok, why, folded = T.verify_batch_folded([known] * n, xs)
        assert not folded and (ok, why) == T.verify_batch_checked([known] * n, xs)
        assert ok == [x == [2] for x in xs]
    T.close()


def test_fold_gt_refusals(ctx):
    import k16
    vk, t = fr.build_key(2, seed=61)
    V = k16.VerifyingKey(ctx, vk)
    inputs = _inputs(2, 4, 1)
    proofs = fr.make_proofs(t, inputs, seed=2)
    w = _weights(3, 4)
    assert V.fold_gt(proofs, inputs, w) == fr.GT_ONE
    g = proofs[2]
    for broken in (bytes(64) + g[64:], g[:64] + bytes(128) + g[192:], g[:192] + bytes(64),
                   g[:64] + pm.g2_aff_bytes(sf.outside_g2_point()) + g[192:]):
        with pytest.raises(k16.K16Error) as e:
            V.fold_gt(proofs[:2] + [broken] + proofs[3:], inputs, w)
        assert e.value.rc == -3
    # an MSM in flight on the context: refused, and the MSM's result is untouched
    import oracle_lib as ol
    bases = ol.gen_points(0, 0, 256)
    scalars = np.random.RandomState(1).randint(0, 256, size=(256, 32), dtype=np.uint8)
    d_b, d_s = ctx.to_device(bases), ctx.to_device(scalars)
    ctx.msm_enqueue(0, d_b, d_s, 256)
    assert ctx.msm_pending() == 1
    for call in (lambda: V.fold_gt(proofs, inputs, w), lambda: V.verify_batch_folded(proofs, inputs)):
        with pytest.raises(k16.K16Error) as e:
            call()
        assert e.value.rc == -3
    _, aff = ctx.msm_finish(0)
    assert aff == ol.msm(0, bases, scalars)[1]
    d_b.free()
    d_s.free()
    assert V.fold_gt(proofs, inputs, w) == fr.GT_ONE
    V.close()


def test_resident_prover_proves_the_same_proof_around_a_folded_verification(ctx, toy_paths):
    import k16
    zkey, wtns, vkp = toy_paths
    p = k16.Prover(ctx, zkey)
    T = k16.VerifyingKey(ctx, gio.vk_from_json(vkp))
    z = pm.limbs(0)
    before = p.prove_file(wtns, z, z)
    known = gio.proof_from_json(KNOWN_RS0)
    assert gio.proof_from_json(before) == known
    m = k16.VERIFY_FOLD_MIN + 3
    ok, _, folded = T.verify_batch_folded([known] * m, [[2]] * m)
    assert folded and all(ok)
    assert p.prove_file(wtns, z, z) == before
    xs = [[2]] * m
    xs[0] = [3]
    ok, _, folded = T.verify_batch_folded([known] * m, xs)     # ... and around one that falls back
    assert not folded and ok == [False] + [True] * (m - 1)
    assert p.prove_file(wtns, z, z) == before
    T.close()
    p.close()
