"""Reference for folded batch verification (k16_verify_batch_folded / k16_verify_fold_gt).

* build_key / make_proofs: a Groth16 verifying key and VALID proofs from known discrete logs, by the thousand: with
  alpha = al G, beta = be H, gamma = ga H, delta = de H, IC[j] = ic_j G, A = a G, B = b H, C = c G the pairing check reads
  a b = al be + ga vk_x + de c in the exponent, vk_x = ic_0 + sum_j x_j ic_{j+1}, which fixes c.
* fold_value: the left-hand side of the fold's equation,
      prod_i e(w_i A_i, B_i) * e(S_x, -gamma) * e(S_C, -delta) * e(-s alpha, beta),
  as the product of the ORACLE's pairings of the n + 3 pairs (ol.pairing, ol.gt_mul; points from ol.mul_scalar / ol.msm).
  Field arithmetic is exact, so the GPU's value must be byte-equal to it whatever projective scaling its kernels use."""
import numpy as np

import oracle_lib as ol
import pymodel as pm

GT_ONE = pm.limbs(pm.to_mont(1, pm.Q)) + bytes(352)


def oracle_points(group, scalars):
    """scalars -> (n, AFF_BYTES) uint8 of scalar * generator, on the CPU (the signature of Context.synth_points_scalars)."""
    g = ol.generator(group)
    rows = [np.frombuffer(ol.pt_to_affine(group, ol.mul_scalar(group, g, pm.limbs(int(k) % pm.R))), dtype=np.uint8) for k in scalars]
    return np.stack(rows) if rows else np.zeros((0, ol.AFF_BYTES[group]), dtype=np.uint8)


def build_key(n_ic, seed=1, points=oracle_points):
    """(vk, trapdoor): independent non-trivial alpha, beta, gamma, delta and IC scalars."""
    rng = pm.SplitMix64(seed)
    t = dict(al=rng.below(pm.R - 2) + 2, be=rng.below(pm.R - 2) + 2, ga=rng.below(pm.R - 2) + 2, de=rng.below(pm.R - 2) + 2,
             ic=[rng.below(pm.R - 2) + 2 for _ in range(n_ic)])
    g1 = points(0, [t["al"]] + t["ic"])
    g2 = points(1, [t["be"], t["ga"], t["de"]])
    vk = dict(alpha1=g1[0].tobytes(), beta2=g2[0].tobytes(), gamma2=g2[1].tobytes(), delta2=g2[2].tobytes(),
              ic=[g1[1 + j].tobytes() for j in range(n_ic)])
    return vk, t


def proof_scalars(t, inputs, rng):
    """(a, b, c) of a valid proof for one row of public inputs (any integers: they act modulo r)."""
    a, b = rng.below(pm.R - 1) + 1, rng.below(pm.R - 1) + 1
    vkx = (t["ic"][0] + sum(int(x) * k for x, k in zip(inputs, t["ic"][1:]))) % pm.R
    c = (a * b - t["al"] * t["be"] - t["ga"] * vkx) * pow(t["de"], -1, pm.R) % pm.R
    return a, b, c


def make_proofs(t, inputs, seed=2, points=oracle_points, c_shift=None):
    """Valid proofs (256-byte A | B | C) for the rows of `inputs`; c_shift: {index: k} makes C_index = (c + k) G, a wrong proof."""
    rng = pm.SplitMix64(seed)
    abc = [proof_scalars(t, row, rng) for row in inputs]
    cs = [(c + (c_shift or {}).get(i, 0)) % pm.R for i, (_, _, c) in enumerate(abc)]
    g1 = points(0, [a for a, _, _ in abc] + cs)
    g2 = points(1, [b for _, b, _ in abc])
    n = len(abc)
    return [g1[i].tobytes() + g2[i].tobytes() + g1[n + i].tobytes() for i in range(n)]


def _neg_g2(q):
    if q == bytes(128):
        return q
    ya, yb = pm.unlimbs(q[64:96]), pm.unlimbs(q[96:128])
    return q[:64] + pm.limbs((pm.Q - ya) % pm.Q) + pm.limbs((pm.Q - yb) % pm.Q)


def fold_value(vk, proofs, inputs, weights):
    """The 384-byte GT value of the fold under `weights` (ints below 2^128; zero leaves the proof out)."""
    n_ic = len(vk["ic"])
    s = sum(weights) % pm.R
    tj = [sum(w * int(row[j]) for w, row in zip(weights, inputs)) % pm.R for j in range(n_ic - 1)]
    pairs = []
    for p, w in zip(proofs, weights):
        if w:
            pairs.append((ol.pt_to_affine(0, ol.mul_scalar(0, p[:64], pm.limbs(w))), p[64:192]))
    cb = np.stack([np.frombuffer(p[192:256], dtype=np.uint8) for p in proofs])
    ws = np.stack([np.frombuffer(pm.limbs(w), dtype=np.uint8) for w in weights])
    s_c = ol.msm(0, cb, ws)[1]
    icb = np.stack([np.frombuffer(b, dtype=np.uint8) for b in vk["ic"]])
    ks = np.stack([np.frombuffer(pm.limbs(k), dtype=np.uint8) for k in [s] + tj])
    s_x = ol.msm(0, icb, ks)[1]
    nsa = ol.pt_to_affine(0, ol.mul_scalar(0, vk["alpha1"], pm.limbs((pm.R - s) % pm.R)))
    pairs += [(s_x, _neg_g2(vk["gamma2"])), (s_c, _neg_g2(vk["delta2"])), (nsa, vk["beta2"])]
    v = GT_ONE
    for g1, g2 in pairs:
        v = ol.gt_mul(v, ol.pairing(g1, g2))
    return v
