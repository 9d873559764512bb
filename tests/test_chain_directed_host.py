"""CPU side of the directed quotient-chain tests (tests/chain_patterns.py holds the circuits; tests/test_gpu_chain_directed.py
runs them on the device).  What makes the GPU tests trustworthy:

* the CPU oracle, which the device is held to, equals an independent plain-integer computation of the H scalars
  (RS/groth16.cpp:137-275 with O(N^2) transforms) on every pattern at N <= 64 -- inputs the oracle had never been looked at on;
* the directed inputs reach the condition they aim for: the value k_spmv stores is computed with the device's own arithmetic
  (tests/cpp/chain_spmv_model.cpp compiles bn254_fq9.h and spmv_plan.h for the host): every stored row is congruent to its
  true sum and below 2r, the targeted rows are stored >= r, cancelling rows are 0 mod r (stored as r), maximal rows sit in
  the layout (slice / wave per row, lanes, entries per lane) they were built for;
* the explicit-row key builder writes build_zkey's bytes when handed build_zkey's rows.
"""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import chain_patterns as cp
import oracle_lib as ol
import pymodel as pm
import zkey_builder as zb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = pm.R
SMALL = (2, 4, 8, 32)
K261 = pow(2, 261, R)          # the device holds x as an integer congruent to x * 2^261


@pytest.fixture(scope="module")
def model_exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("chain_model") / "chain_spmv_model")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only",
                           "-I", os.path.join(ROOT, "keyless-zk-proofs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "chain_spmv_model.cpp"), "-o", exe], timeout=600)
    return exe


def device_rows(exe, zk, wt):
    """{row id: (kind, p, q, stored integer)} from the host build of the device arithmetic"""
    out = subprocess.run([exe, zk, wt], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = {}
    for line in out.stdout.splitlines()[1:]:
        f = line.split()
        rows[int(f[0])] = (f[1], int(f[2]), int(f[3]), int(f[4], 16))
    return rows


def small_cases():
    for name, f in cp.SPMV_PATTERNS.items():
        yield "spmv-%s-64" % name, (lambda f=f: (f(64), None))
    for name, f in cp.DEGENERATE_PATTERNS.items():
        yield "degenerate-%s-64" % name, (lambda f=f: (f(64), None))
    yield "dense-64", (lambda: (cp.dense(64), None))
    for N in SMALL:
        for name in cp.STRUCTURED_WITNESSES:
            def sel(N=N, name=name):
                cir = cp.selector(N)
                return cir, cp.structured_witness(cir, name)
            yield "structured-%s-%d" % (name, N), sel
        for name, f in cp.STRUCTURED_KEYS.items():
            yield "structured-%s-%d" % (name, N), (lambda f=f, N=N: (f(N), None))
        for kind in cp.ABOVE_R_KINDS:
            yield "above_r-%s-%d" % (kind, N), (lambda kind=kind, N=N: (cp.above_r(N, kind), None))
    for seed in range(cp.N_MIX):
        yield "mix-%d" % seed, (lambda seed=seed: (cp.extremal_mix(seed), None))


SMALL_CASES = dict(small_cases())


def _h_ints(h):
    return [int.from_bytes(h[i].tobytes(), "little") for i in range(h.shape[0])]


@pytest.mark.parametrize("case", list(SMALL_CASES))
def test_oracle_h_equals_plain_integer_reference_and_spmv_model_holds_the_row_sums(case, tmp_path, model_exe):
    cir, w = SMALL_CASES[case]()
    zk, wt = str(tmp_path / "k.zkey"), str(tmp_path / "k.wtns")
    cir.write(zk, wt)
    if w is not None:
        zb.write_wtns(wt, w)
    else:
        w = cir.w
    assert all(0 <= x < R for x in w) and all(0 <= x < R for x in cir.v)          # valid inputs of the reference
    if cir.N <= 64:
        _, h = ol.prove_files(zk, wt, pm.limbs(5), pm.limbs(R - 7), nthreads=2, want_h=True)
        assert _h_ints(h) == cp.reference_h(cir.N, *cir.rows(), w)
    got = device_rows(model_exe, zk, wt)
    sums = cir.row_sums(w)
    assert set(got) == set(sums)
    assert all(got[row][3] % R == sums[row] * K261 % R and got[row][3] < 2 * R for row in got)   # right residue, within the 2r invariant


@pytest.mark.parametrize("kind", cp.ABOVE_R_KINDS)
@pytest.mark.parametrize("N", cp.SIZES_STRUCTURED)
def test_above_r_inputs_reach_the_first_butterflies_above_r(N, kind, tmp_path, model_exe):
    """Teeth of the above-r group: at the positions the opening stage of the first inverse pass reads together, the rows meant
    to be 0 are stored as 0 and the others are stored >= r -- by the device's own arithmetic."""
    cir = cp.above_r(N, kind)
    zk, wt = str(tmp_path / "k.zkey"), str(tmp_path / "k.wtns")
    cir.write(zk, wt)
    got = device_rows(model_exe, zk, wt)
    logn = N.bit_length() - 1
    odd = cp.first_pass_stages(logn) & 1
    assert cir.targets["odd"] == odd
    group = 2 if odd else 4
    n_checked = 0
    for m, rows in cir.targets["above_r_rows"].items():
        assert len(rows) >= (1 if N <= 4 else 3 if odd else 6)                 # >= three quads (pairs) per polynomial
        for row in rows:
            pos = cp.brev(row % N, logn)
            base = pos - pos % group
            hi = range(base + group // 2, base + group)
            assert pos in hi
            if kind != "c":
                assert R <= got[row][3] < cp.FRED_KEEPS_BELOW
            for p in range(base, base + group // 2):                          # the partner positions: zero, or small
                partner = (0 if m == 0 else N) + cp.brev(p, logn)
                assert partner not in got or (odd and got[partner][3] in (0, K261, 2 * K261 % R))
                if not odd:
                    assert partner not in got
            n_checked += 1
    assert n_checked
    if kind == "c":       # k_mul stores frmul9(a, b) as it is: the product's representative is what the c transform reads
        for ra, rb in zip(*(cir.targets["above_r_rows"][m] for m in (0, 1))):
            assert ra + N == rb and cp.mont9(got[ra][3], got[rb][3]) >= R


def test_cancelling_and_maximal_rows_are_what_they_claim(tmp_path, model_exe):
    zk, wt = str(tmp_path / "k.zkey"), str(tmp_path / "k.wtns")
    for N in cp.SIZES_OTHER:
        cir = cp.spmv_cancel(N)
        cir.write(zk, wt)
        got = device_rows(model_exe, zk, wt)
        sums = cir.row_sums()
        zero_rows = cir.targets["zero_rows"]
        assert len(zero_rows) > 90 and all(sums[row] == 0 for row in zero_rows)
        stored = [got[row][3] for row in zero_rows]
        assert all(v % R == 0 for v in stored)
        assert stored.count(R) > 50                     # a zero that is represented as r
        assert {got[row][0] for row in zero_rows} == {"S", "L"}
        cir = cp.spmv_sum_r_minus_1(N)
        cir.write(zk, wt)
        got = device_rows(model_exe, zk, wt)
        assert all(got[row][3] % R == (R - 1) * K261 % R for row in cir.targets["r_minus_1_rows"])
        for wide in (False, True):
            cir = cp.spmv_maximal(N, wide)
            cir.write(zk, wt)
            got = device_rows(model_exe, zk, wt)
            lengths = cir.targets["row_lengths"]
            assert sorted(set(lengths.values())) == sorted(cp.ROW_LENGTHS)
            for row, ln in lengths.items():
                kind, p, q, _ = got[row]
                if ln <= cp.SPMV_LONG:
                    assert (kind, q) == ("S", ln) and ln <= p <= cp.SPMV_LONG     # one lane walks the slice's length
                else:
                    assert (kind, p, q) == ("L", 64, (ln + 63) // 64)             # a wave: 64 lanes, ceil(len / 64) entries each
            assert all(v == (R - 1) * (R - 1 if wide else 255) % R for v in
                       {(cir.w[s] * v) % R for s, v in zip(cir.s, cir.v)})


def test_extremal_set_has_representatives_above_r():
    for v in cp.ABOVE:
        assert v < R and R <= cp.fred9(cp.term9(1, v)) < cp.FRED_KEEPS_BELOW
    assert R < cp.FRED_KEEPS_BELOW < R + (R >> 21)
    assert cp.root_of_unity(28) != 1 and pow(cp.root_of_unity(28), 1 << 27, R) == R - 1


def test_explicit_row_builder_reproduces_build_zkey_bytes(tmp_path):
    """the rows build_zkey draws (same generator, same order of draws), handed to build_zkey_rows: the same file"""
    n_vars, n_pub, N, n_coefs, seed, long_rows = 700, 1, 2048, 2000, 11, (65, 200, 64)
    a, b = str(tmp_path / "a.zkey"), str(tmp_path / "b.zkey")
    zb.build_zkey(a, n_vars, n_pub, N, n_coefs, seed=seed, long_rows=long_rows)
    rs = np.random.RandomState(seed)
    m = rs.randint(0, 2, size=n_coefs).astype(np.uint32)
    c = rs.randint(0, N, size=n_coefs).astype(np.uint32)
    at = 0
    for k, ln in enumerate(long_rows):
        c[at:at + ln] = (k * 7919 + 5) % N
        m[at:at + ln] = k & 1
        at += ln
    order = np.argsort(c, kind="stable")
    c, m = c[order], m[order]
    s = rs.randint(0, n_vars, size=n_coefs).astype(np.uint32)
    v = [int(rs.randint(1, 1 << 30)) if rs.rand() < 0.7 else pm.SplitMix64(seed * 7919 + i).below(R) for i in range(n_coefs)]
    zb.build_zkey_rows(b, n_vars, n_pub, N, m, c, s, v, rs=rs, sort_by=("c",))
    with open(a, "rb") as fa, open(b, "rb") as fb:
        assert fa.read() == fb.read()
    # the default order (constraint, then matrix) holds the same rows: same proof, same H scalars
    wt = str(tmp_path / "w.wtns")
    zb.build_wtns(wt, n_vars, seed=12)
    zb.build_zkey_rows(b, n_vars, n_pub, N, m, c, s, v, rs=np.random.RandomState(seed), sort_by=("c", "m"))
    with open(b, "rb") as fb:
        sec = fb.read()
    at = sec.index(struct.pack("<IQ", 4, 4 + 44 * n_coefs)) + 16
    rec = np.frombuffer(sec[at:at + 44 * n_coefs], dtype=zb.COEF_DTYPE)
    key = rec["c"].astype(np.int64) * 2 + rec["m"]
    assert np.all(np.diff(key) >= 0)
    js_a, h_a = ol.prove_files(a, wt, pm.limbs(3), pm.limbs(4), nthreads=2, want_h=True)
    js_b, h_b = ol.prove_files(b, wt, pm.limbs(3), pm.limbs(4), nthreads=2, want_h=True)
    assert np.array_equal(h_a, h_b)


def test_explicit_row_builder_at_2p17(tmp_path):
    """2^17 constraints, 2^18 coefficients: the size the GPU tests build their largest keys at"""
    N = 1 << 17
    cir = cp.selector(N)
    cir.write(str(tmp_path / "k.zkey"))
    assert ol.zkey_info(str(tmp_path / "k.zkey")) == dict(n_vars=cir.n_vars, n_public=1, domain_size=N, n_coefs=2 * N)


def test_padded_witnesses_fit_the_compact_upload():
    """what test_patterns_through_the_compact_witness_upload proves really crosses in compact form"""
    cir = cp.selector(1 << 12).pad_vars((1 << 16) + 3)
    for name in cp.STRUCTURED_WITNESSES:
        assert cp.compact_upload_fits(cp.structured_witness(cir, name)), name
    for kind in cp.ABOVE_R_KINDS:
        w = cp.above_r(1 << 12, kind).pad_vars((1 << 16) + 300).w
        assert cp.compact_upload_fits(w) and sum(1 for v in w if v >= 256) > 5000
    assert not cp.compact_upload_fits([1 << 200] * (1 << 16)) and not cp.compact_upload_fits([1] * 1000)
