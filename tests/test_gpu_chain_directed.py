"""-m gpu : directed values through the prover's quotient chain -- k_spmv, the inverse k_ntt_pass9 passes with the fused TAIL
store, the forward passes on three polynomials per launch, k_mul, k_hscalars -- against the CPU oracle.  The circuits and
witnesses are constructed (tests/chain_patterns.py), not drawn: extremal coefficients and wire values, rows that cancel to 0
or sum to r - 1, maximal rows of every layout, empty matrices, constant / delta / alternating / single-coefficient
polynomials, and rows that k_spmv stores >= r at the positions the first butterflies read together.  Proof JSON and all H
scalars are compared for equality (integer arithmetic: no tolerances), through prove_mem and prove_file, with fixed r, s.
tests/test_chain_directed_host.py shows without a GPU that the oracle is right on these inputs and that they reach the
conditions they aim for."""
import numpy as np
import pytest

import chain_patterns as cp
import oracle_lib as ol
import pymodel as pm
import zkey_builder as zb
from gpu_common import rand_fe_array

pytestmark = pytest.mark.gpu

R = pm.R
BLIND_R, BLIND_S = pm.limbs(pm.SplitMix64(301).below(R)), pm.limbs(R - 1)
ORACLE_THREADS = 16


@pytest.fixture(scope="module")
def ctx():
    import k16
    c = k16.Context(0)   # raises if libk16.so is missing or there is no GPU: no fallback
    yield c
    c.close()


def _check(prover, zk, wt, w, tag=""):
    """one witness on a prover: H scalars and proof JSON equal to the oracle's, in memory and from the file"""
    wb = zb.write_wtns(wt, w)
    want, h_ref = ol.prove_files(zk, wt, BLIND_R, BLIND_S, nthreads=ORACLE_THREADS, want_h=True)
    got = prover.prove_mem(wb, BLIND_R, BLIND_S)
    h_gpu = prover.last_h()
    if not np.array_equal(h_gpu, h_ref):
        bad = np.flatnonzero((h_gpu != h_ref).any(axis=1))
        raise AssertionError("%s: %d H scalars differ, first at index %d" % (tag, len(bad), bad[0]))
    assert got == want, tag
    assert prover.prove_file(wt, BLIND_R, BLIND_S) == want, tag
    return h_ref


def _run(ctx, tmp_path, cir, w=None, tag=""):
    import k16
    zk, wt = str(tmp_path / "k.zkey"), str(tmp_path / "k.wtns")
    cir.write(zk)
    p = k16.Prover(ctx, zk)
    try:
        assert p.info() == dict(n_vars=cir.n_vars, n_public=1, domain_size=cir.N, n_coefs=len(cir.m))
        return _check(p, zk, wt, cir.w if w is None else w, tag)
    finally:
        p.close()


# ---------------------------------------------------------------------------------------------------------------- SpMV forms
@pytest.mark.parametrize("N", cp.SIZES_OTHER)
@pytest.mark.parametrize("pattern", list(cp.SPMV_PATTERNS))
def test_spmv_forms(ctx, tmp_path, pattern, N):
    """both product forms (single-limb product for wires below 256, full product for wide wires), both row layouts (slices
    of rows <= 64 entries, a wave per longer row): maximal terms in rows of 1 ... 4096 entries, rows cancelling to 0 mod r
    (stored as r), rows summing to r - 1, rows mixing the forms, wire 0 with every extremal coefficient"""
    _run(ctx, tmp_path, cp.SPMV_PATTERNS[pattern](N), tag=pattern)


# ------------------------------------------------------------------------------------------------------ degenerate matrices
@pytest.mark.parametrize("N", cp.SIZES_OTHER)
@pytest.mark.parametrize("pattern", list(cp.DEGENERATE_PATTERNS))
def test_degenerate_matrices_on_a_warm_context(ctx, tmp_path, pattern, N):
    """A prover holds one key, so "degenerate after dense on a warm prover" is two things here.  (i) The dense key's prover,
    after a dense proof, proves a witness of zeros: A.w == B.w == 0 over buffers that have just held dense polynomials.
    (ii) The degenerate key -- empty and nearly empty matrices -- proves twice on its own prover: the second proof finds the
    first one's a / b / c, transform buffers and H scalars, and the rows no coefficient touches must be zero again.  (The
    dense proof in between runs on the other prover and only keeps the context busy.)  With both matrices empty every H
    scalar is 0 and the H MSM runs on all-zero scalars."""
    import k16
    d = cp.dense(N)
    zkd, wtd = str(tmp_path / "d.zkey"), str(tmp_path / "d.wtns")
    d.write(zkd)
    pd = k16.Prover(ctx, zkd)
    try:
        _check(pd, zkd, wtd, d.w, "dense")
        # the dense key with a witness of zeros: A.w == B.w == 0 on a prover that has just held dense polynomials
        h = _check(pd, zkd, wtd, [1] + [0] * (d.n_vars - 1), "dense key, zero witness")
        assert not h.any()
        cir = cp.DEGENERATE_PATTERNS[pattern](N)
        zk, wt = str(tmp_path / "k.zkey"), str(tmp_path / "k.wtns")
        cir.write(zk)
        p = k16.Prover(ctx, zk)
        try:
            h1 = _check(p, zk, wt, cir.w, pattern)
            _check(pd, zkd, wtd, d.w, "dense again")
            h2 = _check(p, zk, wt, cir.w, pattern + " (warm)")
            assert np.array_equal(h1, h2)
            if pattern == "both_zero":
                assert not h1.any()
        finally:
            p.close()
    finally:
        pd.close()


# -------------------------------------------------------------------------------------------------- structured polynomials
@pytest.fixture(scope="module")
def selectors(ctx, tmp_path_factory):
    """one key and one prover per size for the witness-driven patterns (constants, deltas, alternation)"""
    import k16
    cache = {}

    def get(N):
        if N not in cache:
            d = tmp_path_factory.mktemp("sel%d" % N)
            cir = cp.selector(N)
            zk = str(d / "k.zkey")
            cir.write(zk)
            cache[N] = (cir, zk, str(d / "k.wtns"), k16.Prover(ctx, zk))
        return cache[N]

    yield get
    for entry in cache.values():
        entry[3].close()


@pytest.mark.parametrize("N", cp.SIZES_STRUCTURED)
@pytest.mark.parametrize("name", list(cp.STRUCTURED_WITNESSES))
def test_structured_polynomials_by_witness(selectors, name, N):
    """evaluations all equal to c for every extremal c (b: another extremal constant), a single non-zero evaluation at
    0, 1, N/2, N-1, alternating 1, r-1: butterflies meet equal and opposite operands at every stage"""
    cir, zk, wt, p = selectors(N)
    _check(p, zk, wt, cp.structured_witness(cir, name), name)


@pytest.mark.parametrize("N", cp.SIZES_STRUCTURED)
@pytest.mark.parametrize("name", list(cp.STRUCTURED_KEYS))
def test_structured_polynomials_by_key(ctx, tmp_path, name, N):
    """evaluations g^(k i) (one non-zero coefficient) for k = 1, N/2 - 1, N - 1; A == B; A == -B"""
    _run(ctx, tmp_path, cp.STRUCTURED_KEYS[name](N), tag=name)


# ------------------------------------------------------------------- representatives above r at the chain's first butterflies
@pytest.mark.parametrize("N", cp.SIZES_STRUCTURED)
@pytest.mark.parametrize("kind", cp.ABOVE_R_KINDS)
def test_above_r_at_the_first_butterflies_of_the_chain(ctx, tmp_path, kind, N):
    """The chain's own version of test_ntt_first_stage_pair_with_representatives_above_r: k16_ntt_coset_chain reads k_spmv's
    sums (a, b) and k_mul's products (c) in place.  Quads in bit-reversed row order whose first two rows are 0 and whose
    third and fourth are stored >= r, in a, in b, in both, and in c; for the sizes whose first pass opens with the single
    radix-2 stage, pairs of a small and a >= r row.  (The opening double stage computed (x0 + x1) - (x2 + x3) + 2r, negative
    for such quads; it has to be + 4r.)"""
    _run(ctx, tmp_path, cp.above_r(N, kind), tag="above_r " + kind)


# ---------------------------------------------------------------------------------------------------- extremal mix sweep
@pytest.mark.parametrize("seed", range(cp.N_MIX))
def test_extremal_mix_sweep(ctx, tmp_path, seed):
    """small circuits whose every coefficient and every wire comes from the extremal set, row lengths from
    {1, 2, 3, 63, 64, 65, 200}"""
    _run(ctx, tmp_path, cp.extremal_mix(seed), tag="mix %d" % seed)


# ------------------------------------------------------------------------------------------- the same through the compact upload
def test_patterns_through_the_compact_witness_upload(ctx, tmp_path):
    """>= 2^16 wires: the witness crosses as one byte per wire + the lists of wide values (k_wtns_expand_*), and k_spmv reads
    the n16 words those kernels leave.  The padding wires are mostly bytes, so that every one of the packer's 32 ranges holds
    its wide values (asserted: a witness that overflows a range is copied plainly and would not test this); one witness is
    also handed over through the caller-filled buffers (prove_compact)."""
    import k16
    N = 1 << 12
    cir = cp.selector(N).pad_vars((1 << 16) + 3)
    zk, wt = str(tmp_path / "k.zkey"), str(tmp_path / "k.wtns")
    cir.write(zk)
    p = k16.Prover(ctx, zk)
    try:
        for name in ("const[r-1]", "const[255]", "const[256]", "const[above_r_0]", "delta[at_half]", "alternating"):
            w = cp.structured_witness(cir, name)
            assert cp.compact_upload_fits(w), name
            h_ref = _check(p, zk, wt, w, name)
        narrow, idx, val = p.compact_buffers()
        wb = cir.witness_bytes(w)
        wide = np.flatnonzero(wb[:, 1:].any(axis=1))
        assert 0 < len(wide) <= len(idx)
        narrow[:] = wb[:, 0]
        narrow[wide] = 0
        idx[:len(wide)] = wide
        val[:len(wide)] = wb[wide]
        got = p.prove_compact(len(wide), BLIND_R, BLIND_S)
        assert np.array_equal(p.last_h(), h_ref)
        assert got == ol.prove_files(zk, wt, BLIND_R, BLIND_S, nthreads=ORACLE_THREADS)
    finally:
        p.close()
    for kind in ("both", "c"):
        cir = cp.above_r(N, kind).pad_vars((1 << 16) + 300)
        assert cp.compact_upload_fits(cir.w)
        _run(ctx, tmp_path, cir, tag="above_r " + kind)


# ------------------------------------------------------------------------------------------ the public NTT entry point
@pytest.mark.parametrize("log2n", [4, 5, 6, 7, 9, 10, 11, 13, 14, 15])
def test_ntt_vs_oracle_remaining_sizes(ctx, log2n):
    """the sizes test_ntt_vs_oracle leaves out, both directions, tables of the size and of twice the size"""
    n = 1 << log2n
    a = rand_fe_array(pm.SplitMix64(100 + log2n), R, n)
    for inverse in (False, True):
        for md in (n, 2 * n):
            assert np.array_equal(ctx.ntt(a, max_domain=md, inverse=inverse), ol.ntt(a, max_domain=md, inverse=inverse)), \
                (log2n, inverse, md)


@pytest.mark.parametrize("md_kind", ["4n", "8n", "2^18", "2^22"])
@pytest.mark.parametrize("log2n", [3, 10, 13])
def test_ntt_with_a_larger_table(ctx, log2n, md_kind):
    """a table much larger than the transform: the twiddles are read with a root stride; 2^18 and 2^22 tables carry the
    per-stage twiddle tables"""
    n = 1 << log2n
    md = {"4n": 4 * n, "8n": 8 * n, "2^18": 1 << 18, "2^22": 1 << 22}[md_kind]
    a = rand_fe_array(pm.SplitMix64(200 + log2n), R, n)
    for inverse in (False, True):
        assert np.array_equal(ctx.ntt(a, max_domain=md, inverse=inverse), ol.ntt(a, max_domain=md, inverse=inverse)), \
            (log2n, inverse, md)
